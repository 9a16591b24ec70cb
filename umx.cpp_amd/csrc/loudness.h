// loudness.h -- K-weighted hop energies of what leaves the whole-track drivers: the sums of squares behind ITU-R BS.1770-4 /
// EBU R128 loudness, in a form that does not depend on regions, lanes, the queue or reset mode.  One statement of the rule, for the
// host entry points (umx_hip_kweight_coeffs, umx_hip_kweight_hops_host, umx_hip_loudness_gate) and for the kernel below:
//   hop      hop = (rate + 5) / 10 frames; hop b of an output is the frames [b hop, (b + 1) hop) of the caller's track; a last
//            incomplete hop is not measured
//   filter   two biquads per rate (shelf, then high-pass), formed in double from the analogue prototypes as libebur128 does
//            (kweight_coeffs), run in double in transposed direct form II in the operation order of kweight_biquad
//   E[b]     per channel: the cascade starts from a zero state at frame max(0, b - 1) hop, runs over the frames up to (b + 1) hop, and
//            the squares of its outputs over hop b are added in frame order (fused multiply-adds throughout, on host and device)
//   gate     blocks of four hops, both channels with weight 1: the absolute gate at -70, the relative gate 10 below the mean of the
//            absolutely gated blocks (loudness_gate)
// A hop is a function of 2 hop samples and of nothing else: one thread computes it, start to end, whatever launch it is part of.
#pragma once
#include "common.h"
#include <cmath>

namespace umx
{

constexpr int KW_RATE_MIN = 8000, KW_RATE_MAX = 192000;
inline bool kweight_rate_ok(int rate) { return rate >= KW_RATE_MIN && rate <= KW_RATE_MAX; }
inline int kweight_hop(int rate) { return (rate + 5) / 10; }

struct KWeight // b0 b1 b2 a1 a2 of the shelf and of the high-pass stage
{
    double pb[3], pa[2], rb[3], ra[2];
};

// ITU-R BS.1770-4's two stages at any rate: the bilinear transform of the analogue prototypes whose 48 kHz image is the standard's
// table (the derivation of libebur128's ebur128_init_filter, restated; constants to the digits given there)
inline KWeight kweight_coeffs(int rate)
{
    const double pi = 3.14159265358979323846;
    KWeight k;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        k.pb[0] = (Vh + Vb * K / Q + K * K) / a0;
        k.pb[1] = 2.0 * (K * K - Vh) / a0;
        k.pb[2] = (Vh - Vb * K / Q + K * K) / a0;
        k.pa[0] = 2.0 * (K * K - 1.0) / a0;
        k.pa[1] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / rate), a0 = 1.0 + K / Q + K * K;
        k.rb[0] = 1.0;
        k.rb[1] = -2.0;
        k.rb[2] = 1.0;
        k.ra[0] = 2.0 * (K * K - 1.0) / a0;
        k.ra[1] = (1.0 - K / Q + K * K) / a0;
    }
    return k;
}

// one sample through one stage, transposed direct form II, state (s1, s2): four fused multiply-adds and one product, two of them on
// the path from one output to the next
__host__ __device__ inline double kweight_biquad(const double b[3], const double a[2], double x, double &s1, double &s2)
{
    const double u = __builtin_fma(b[1], x, s2);
    const double y = __builtin_fma(b[0], x, s1);
    s1 = __builtin_fma(-a[0], y, u);
    s2 = __builtin_fma(-a[1], y, b[2] * x);
    return y;
}

struct KWeightState
{
    double p1 = 0, p2 = 0, r1 = 0, r2 = 0;
};
// one sample through the cascade
__host__ __device__ inline double kweight_sample(const KWeight &k, float x, KWeightState &s)
{
    return kweight_biquad(k.rb, k.ra, kweight_biquad(k.pb, k.pa, (double)x, s.p1, s.p2), s.r1, s.r2);
}

// the rule on the host: hops [first_hop, first_hop + n_hops) of n interleaved stereo frames, into E[channel * hops_total + b],
// hops_total = n / hop
inline void kweight_hops_host(const float *x, long long n, int rate, long long first_hop, long long n_hops, double *E)
{
    const KWeight k = kweight_coeffs(rate);
    const long long hop = kweight_hop(rate), hops_total = n / hop;
    for (int ch = 0; ch < 2; ++ch)
        for (long long b = first_hop; b < first_hop + n_hops; ++b)
        {
            KWeightState s;
            double e = 0;
            for (long long f = (b > 0 ? b - 1 : 0) * hop; f < (b + 1) * hop; ++f)
            {
                const double y = kweight_sample(k, x[2 * f + ch], s);
                if (f >= b * hop)
                    e = __builtin_fma(y, y, e);
            }
            E[ch * hops_total + b] = e;
        }
}

// Blocks and gates of one output from its hop energies E[channel * hops + b].  Comparisons are IEEE: a NaN block passes no gate and
// is no maximum, an inf block passes.  No block, or none gated in: -inf.
inline void loudness_gate(const double *E, long long hops, int hop, double &integrated, double &momentary_max, long long &blocks, long long &gated)
{
    const long long nb = hops >= 4 ? hops - 3 : 0;
    const double ninf = -INFINITY;
    auto power = [&](long long j) {
        double p = 0;
        for (int ch = 0; ch < 2; ++ch)
            for (int h = 0; h < 4; ++h)
                p += E[ch * hops + j + h];
        return p / (4.0 * hop);
    };
    auto lufs = [](double p) { return -0.691 + 10.0 * std::log10(p); };
    integrated = momentary_max = ninf;
    blocks = nb;
    gated = 0;
    double sum = 0;
    long long n_abs = 0;
    for (long long j = 0; j < nb; ++j)
    {
        const double p = power(j), l = lufs(p);
        if (l > momentary_max)
            momentary_max = l;
        if (l > -70.0)
        {
            sum += p;
            ++n_abs;
        }
    }
    if (n_abs == 0)
        return;
    const double gamma = lufs(sum / (double)n_abs) - 10.0;
    sum = 0;
    for (long long j = 0; j < nb; ++j)
    {
        const double p = power(j), l = lufs(p);
        if (l > -70.0 && l > gamma)
        {
            sum += p;
            ++gated;
        }
    }
    if (gated > 0)
        integrated = lufs(sum / (double)gated);
}

// what a whole-track call reports from a job's hop energies E[(m * 2 + channel) * hops + b]
inline void loudness_report(const double *E, long long hops, int hop, int n_out, umx_loudness &ld)
{
    ld = umx_loudness{};
    ld.n_out = n_out;
    ld.hop = hop;
    ld.hops = hops;
    for (int m = 0; m < 4; ++m)
    {
        ld.integrated[m] = ld.momentary_max[m] = -INFINITY;
        if (m < n_out)
            loudness_gate(E + (size_t)m * 2 * hops, hops, hop, ld.integrated[m], ld.momentary_max[m], ld.blocks[m], ld.gated[m]);
    }
}

// ---------------------------------------------------------------- the kernel
// A thread is one hop of one buffer, both channels: two independent chains of 2 hop samples.  The 64 hops of a workgroup (one wave)
// start `hop` frames (8 hop bytes) apart, so a load per thread would touch 64 cache lines per instruction for 8 bytes each.  The
// samples are staged through LDS instead: chunk by chunk of KW_CHUNK frames, the wave reads each of its 64 rows with ONE coalesced
// 512-byte load and every thread then walks its own row.  Rows are KW_CHUNK + 1 frames apart: thread t reads dword banks 2 t + 2 i
// and 2 t + 2 i + 1 (mod 64), no conflict within the 32-lane groups of an 8-byte read.  The 64 loads of the NEXT chunk are issued,
// without a branch between them, into 128 registers before this chunk's arithmetic and waited for behind it (the first form, a
// guarded load and its LDS store row by row, paid one memory latency per row: 2.85 ms for one 45 s region's 450 hops).
#define KW_THREADS 64
#define KW_CHUNK 64
#define KW_ROW (KW_CHUNK + 1)

struct KWeightArgs
{
    const float2 *src[4]; // frame 0 of the caller's track first; grid.y picks one
    KWeight k;
    double *E;            // [buffer][channel][hops_total]
    long long hops_total;
    long long first_hop;
    int n_hops, hop;
};

__global__ __launch_bounds__(KW_THREADS) void kweight_hops_kernel(KWeightArgs a)
{
    __shared__ float2 stage[KW_THREADS * KW_ROW];
    const int t = threadIdx.x, m = blockIdx.y;
    const float2 *__restrict__ src = a.src[m];
    const int row0 = blockIdx.x * KW_THREADS;              // the workgroup's first hop, counted from first_hop
    const int rows = min(KW_THREADS, a.n_hops - row0);     // (>= 1 by the grid)
    const long long b0 = a.first_hop + row0;               // hop of row 0; row r: hop b0 + r, its window starts at frame (b0 + r - 1) hop
    const int hop = a.hop, span = 2 * hop;                 // (hop 0's window starts at frame -hop: zeros, which leave the state at rest)
    KWeightState sl, sr;
    double el = 0, er = 0;
    // The chunk at c0 of all 64 rows, one frame per row in each thread's registers: 64 loads in flight, no branch between them.
    // Frame numbers fit an int (the launcher's frames are at most 2^30).  A frame nobody consumes -- a row beyond `rows`, a frame
    // beyond the span -- is read from the nearest frame of the launch's own range [0, last]; hop 0's frames before the track are
    // read from frame 0 and masked to +0.
    const int last = (int)((a.first_hop + a.n_hops) * hop) - 1, f0 = (int)((b0 - 1) * hop) + t;
    float2 pre[KW_THREADS];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int r = 0; r < KW_THREADS; ++r)
        {
            const int f = f0 + c0 + r * hop; // a consumed one: < (b0 + r + 1) hop <= last + 1
            pre[r] = src[min(max(f, 0), last)];
        }
    };
    auto store_chunk = [&](int c0) { // (the mask is applied here, so that nothing waits for a load before the arithmetic it runs under)
#pragma unroll
        for (int r = 0; r < KW_THREADS; ++r)
        {
            const uint32_t keep = f0 + c0 + r * hop < 0 ? 0u : ~0u;
            stage[r * KW_ROW + t] = make_float2(__uint_as_float(__float_as_uint(pre[r].x) & keep), __uint_as_float(__float_as_uint(pre[r].y) & keep));
        }
    };
    load_chunk(0);
    for (int c0 = 0; c0 < span; c0 += KW_CHUNK)
    {
        const int cn = min(KW_CHUNK, span - c0);
        __syncthreads(); // the previous chunk has been consumed
        store_chunk(c0);
        __syncthreads();
        if (c0 + KW_CHUNK < span) // the next chunk's loads run under this chunk's arithmetic
            load_chunk(c0 + KW_CHUNK);
        if (t < rows)
            for (int i = 0; i < cn; ++i)
            {
                const float2 v = stage[t * KW_ROW + i];
                const double yl = kweight_sample(a.k, v.x, sl), yr = kweight_sample(a.k, v.y, sr);
                if (c0 + i >= hop)
                {
                    el = __builtin_fma(yl, yl, el);
                    er = __builtin_fma(yr, yr, er);
                }
            }
    }
    if (t < rows)
    {
        double *E = a.E + (size_t)m * 2 * a.hops_total + (b0 + t);
        E[0] = el;
        E[a.hops_total] = er;
    }
}

// Hops [first_hop, first_hop + n_hops) of buffers 0 .. nb-1 (frame 0 of the caller's track at src[b]) into E, laid out
// [buffer][channel][hops_total].  The caller has checked that (first_hop + n_hops) hop frames are there and final.
inline void launch_kweight_hops(int nb, const float2 *const *src, const KWeight &k, int hop, long long hops_total, long long first_hop,
                                long long n_hops, double *E, hipStream_t st)
{
    if (nb < 1 || n_hops < 1)
        return;
    KWeightArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.src[b] = src[b];
    a.k = k;
    a.E = E;
    a.hops_total = hops_total;
    a.first_hop = first_hop;
    a.n_hops = (int)n_hops;
    a.hop = hop;
    hipLaunchKernelGGL(kweight_hops_kernel, dim3((unsigned)((n_hops + KW_THREADS - 1) / KW_THREADS), std::min(nb, 4)), dim3(KW_THREADS), 0, st, a);
}

} // namespace umx
