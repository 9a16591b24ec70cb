// resample.h -- band-limited sample-rate conversion of (2,n) interleaved buffers on the device.
// The filter is torchaudio's default `sinc_interp_hann` resampler (6 zero crossings, rolloff 0.99), which Open-Unmix's
// `preprocess` applies to input that is not at the model's 44.1 kHz.  For rates r_in -> r_out with g = gcd, M = r_in / g,
// L = r_out / g, b = 0.99 min(M, L), W = 6:
//     y[j] = sum_i x[i] (b / M) k(b (i / M - j / L)),   k(t) = sinc(t) cos^2(pi t / 2W) for |t| < W, else 0
// with x zero outside [0, n_in).  In polyphase form output j reads the input frames c + d, c = floor(j M / L), for d in
// [-D, D + 1], D = ceil(W M / b), with the taps of phase (j M) mod L: a table of L phases x K = 2D + 2 taps, built on the host
// in double and rounded to fp32.  Every output is the fp32 sum over d ascending (separate multiply and add: the build has
// -ffp-contract=off), so its bits depend on neither the blocking nor the number of buffers of a launch.
#pragma once
#include "common.h"

#include <cmath>
#include <numeric>
#include <vector>

namespace umx
{

constexpr int RS_THREADS = 256;
constexpr int RS_BLOCK_MAX = 2048;     // output frames per workgroup (even: a thread stores two frames at a time)
constexpr int RS_SPAN_MAX = 4096;      // input frames a workgroup stages in LDS (32 KB)
constexpr int RS_TAPS_LDS_MAX = 8192;  // tap tables up to 32 KB (rows padded to K + 1) go to LDS; larger ones are read through the L2
constexpr int RS_MIN_RATE = 8000, RS_MAX_RATE = 192000;
constexpr int RS_MODEL_RATE = 44100; // the rate the model runs at (dsp.hpp:16)

struct ResampleGeom
{
    int M = 0, L = 0, D = 0, K = 0;
    double b = 0;
    int block = 0; // output frames per workgroup
    int span = 0;  // input frames a workgroup stages, at most
};

inline bool resample_rate_ok(int r) { return r >= RS_MIN_RATE && r <= RS_MAX_RATE; }

inline bool resample_geom(int rate_in, int rate_out, ResampleGeom &g)
{
    if (!resample_rate_ok(rate_in) || !resample_rate_ok(rate_out))
        return false;
    const int gc = std::gcd(rate_in, rate_out);
    g.M = rate_in / gc;
    g.L = rate_out / gc;
    g.b = 0.99 * std::min(g.M, g.L);
    g.D = (int)std::ceil(6.0 * g.M / g.b);
    g.K = 2 * g.D + 2;
    // a block of B outputs reads floor((B - 1) M / L) + 1 + K input frames at most
    auto span_of = [&](long long bo) { return (long long)((bo - 1) * g.M / g.L) + 1 + g.K; };
    long long bo = RS_BLOCK_MAX;
    while (bo > 2 && span_of(bo) > RS_SPAN_MAX)
        bo -= 2;
    g.block = (int)bo;
    g.span = (int)span_of(bo);
    return true;
}

// The range rule, host arithmetic in 64-bit integers.  Output j reads the input frames c - D .. c + D + 1, c = floor(j M / L):
// the whole window, zero taps included.
// resample_needs: the leading input frames that outputs [0, n_out_wanted) read: floor((n_out_wanted - 1) M / L) + D + 2, at most n_in.
inline long long resample_needs(long long n_out_wanted, int rate_in, int rate_out, long long n_in)
{
    ResampleGeom g;
    if (n_out_wanted < 0 || n_in < 0 || !resample_geom(rate_in, rate_out, g))
        return -1;
    if (n_out_wanted == 0)
        return 0;
    return std::min(n_in, (n_out_wanted - 1) * g.M / g.L + g.D + 2);
}
// resample_ready: the leading output frames whose whole window lies inside the first n_in_final input frames: j with
// floor(j M / L) + D + 1 <= n_in_final - 1, that is j < (n_in_final - D - 1) L / M.  Beyond n_in the input is zeros, which are known:
// n_in_final >= n_in makes all n_out outputs ready.
inline long long resample_ready(long long n_in_final, int rate_in, int rate_out, long long n_in, long long n_out)
{
    ResampleGeom g;
    if (n_in_final < 0 || n_in < 0 || n_out < 0 || !resample_geom(rate_in, rate_out, g))
        return -1;
    if (n_in_final >= n_in)
        return n_out;
    const long long a = n_in_final - g.D - 1;
    if (a <= 0)
        return 0;
    return std::min(n_out, (a * g.L + g.M - 1) / g.M);
}

// natural output length ceil(n L / M) (torchaudio's target_length)
inline long long resampled_length(long long n, int rate_in, int rate_out)
{
    ResampleGeom g;
    if (n < 0 || !resample_geom(rate_in, rate_out, g))
        return -1;
    return (n * g.L + g.M - 1) / g.M;
}

// taps[phi * K + (d + D)] = (b / M) k(b (d L - phi) / (M L)), in double, rounded once to fp32
inline void resample_taps(const ResampleGeom &g, std::vector<float> &taps)
{
    const double pi = 3.14159265358979323846, W = 6.0;
    taps.assign((size_t)g.L * g.K, 0.f);
    for (int phi = 0; phi < g.L; ++phi)
        for (int d = -g.D; d <= g.D + 1; ++d)
        {
            const double t = g.b * ((double)d * g.L - phi) / ((double)g.M * g.L);
            if (std::fabs(t) >= W)
                continue;
            const double s = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t), w = std::cos(pi * t / (2.0 * W));
            taps[(size_t)phi * g.K + (d + g.D)] = (float)(g.b / g.M * s * w * w);
        }
}

struct ResampleIO
{
    const float *in[4];
    float *out[4];
};

typedef float rs_f4 __attribute__((ext_vector_type(4)));
typedef float rs_f2 __attribute__((ext_vector_type(2)));
typedef unsigned rs_u4 __attribute__((ext_vector_type(4)));
typedef unsigned rs_u2 __attribute__((ext_vector_type(2)));

// One workgroup: `block` consecutive output frames of buffer blockIdx.y, of the range [first, end) of the n_out outputs: the grid starts
// at frame `first` (even, so that a range's 16-byte stores are aligned as the whole launch's are), the last workgroup is clipped to `end`.
// Everything is computed from the absolute frame j0, so a range gives the bits of the same frames of the whole launch.  The input span those frames read is staged in LDS
// (16-byte loads through a buffer resource whose range is the valid part of the span: zeros outside [0, n_in) are written, not
// loaded), the tap table too if it is small; then each thread forms two adjacent outputs and stores them as one 16-byte
// non-temporal store.  The output resource covers exactly this workgroup's frames of [first, end).
// LDS: span frames (float2), then the L x K taps if TAPS_LDS, in rows of K + 1: adjacent lanes read rows of different phases, and
// with an even row stride (K is even) their addresses would fall on a few banks only (16 taps = 64 bytes: 16-way conflicts).
template <bool TAPS_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleIO io, const float *__restrict__ taps, int n_in, int n_out,
                                                              int first, int end, int M, int L, int D, int K, int block, int span_cap)
{
    extern __shared__ float2 rs_lds[];
    float2 *xs = rs_lds;
    const int buf = blockIdx.y, tid = threadIdx.x;
    const long long j0 = (long long)first + (long long)blockIdx.x * block;
    const int nloc = (int)min((long long)block, (long long)min(end, n_out) - j0);
    const long long c0 = j0 * M / L, c1 = (j0 + nloc - 1) * M / L;
    const int phi0 = (int)(j0 * M - c0 * L);
    const long long s_lo = c0 - D, s_hi = c1 + D + 2; // staged input frames [s_lo, s_hi)
    const int span = (int)(s_hi - s_lo);
    const long long v_lo = max(s_lo, 0LL), v_hi = min(s_hi, (long long)n_in);
    const int nv = v_hi > v_lo ? (int)(v_hi - v_lo) : 0;
    const int a = nv ? (int)(v_lo - s_lo) : span; // LDS frames [a, a + nv) hold input, the rest is zero
    for (int f = tid; f < span; f += RS_THREADS)
        if (f < a || f >= a + nv)
            xs[f] = make_float2(0.f, 0.f);
    if (nv)
    {
        const __amdgpu_buffer_rsrc_t rs_in =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(io.in[buf]) + 2 * v_lo, 0, nv * 8, 0x00020000);
        for (int p = tid; 2 * p < nv; p += RS_THREADS)
        {
            if (2 * p + 1 < nv)
            {
                const rs_f4 v = __builtin_bit_cast(rs_f4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, 16 * p, 0, 0));
                xs[a + 2 * p] = make_float2(v.x, v.y);
                xs[a + 2 * p + 1] = make_float2(v.z, v.w);
            }
            else
            {
                const rs_f2 v = __builtin_bit_cast(rs_f2, __builtin_amdgcn_raw_buffer_load_b64(rs_in, 16 * p, 0, 0));
                xs[a + 2 * p] = make_float2(v.x, v.y);
            }
        }
    }
    const float *tp = taps;
    int row = K;
    if (TAPS_LDS)
    {
        float *tl = reinterpret_cast<float *>(xs + span_cap);
        row = K + 1;
        for (int i = tid; i < L * K; i += RS_THREADS)
        {
            const int r = i / K;
            tl[i + r] = taps[i];
        }
        tp = tl;
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(io.out[buf] + 2 * j0, 0, nloc * 8, 0x00020000);
    for (int k = 2 * tid; k < nloc; k += 2 * RS_THREADS)
    {
        float y[4] = {};
        for (int u = 0; u < min(2, nloc - k); ++u)
        {
            // j = j0 + k + u: c = c0 + dc, phase = q - dc L (block M + L < 2^32 by construction)
            const unsigned q = (unsigned)phi0 + (unsigned)(k + u) * (unsigned)M, dc = q / (unsigned)L, phi = q - dc * (unsigned)L;
            const float2 *x = xs + dc; // frame c - D of the span
            const float *t = tp + (size_t)phi * row;
            float sx = 0.f, sy = 0.f;
#pragma unroll 4
            for (int d = 0; d < K; ++d)
            {
                const float2 v = x[d];
                const float w = t[d];
                sx = sx + v.x * w;
                sy = sy + v.y * w;
            }
            y[2 * u] = sx;
            y[2 * u + 1] = sy;
        }
        if (k + 1 < nloc)
        {
            const rs_f4 v = {y[0], y[1], y[2], y[3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(rs_u4, v), rs_out, 8 * k, 0, 2 /* nt */);
        }
        else
        {
            const rs_f2 v = {y[0], y[1]};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(rs_u2, v), rs_out, 8 * k, 0, 2 /* nt */);
        }
    }
}

// n_buffers (1 .. 4) buffers of n_in frames -> frames [first, first + count) of their n_out output frames each (first even, the range
// inside [0, n_out): the caller checks); taps_dev = the table of resample_taps in device memory.  (0, n_out) is the whole-buffer launch.
inline hipError_t launch_resample(const ResampleGeom &g, const float *taps_dev, int n_buffers, const float *const *in, int n_in,
                                  float *const *out, int n_out, int first, int count, hipStream_t st)
{
    if (count < 1)
        return hipSuccess;
    ResampleIO io = {};
    for (int b = 0; b < n_buffers; ++b)
    {
        io.in[b] = in[b];
        io.out[b] = out[b];
    }
    const dim3 grid((unsigned)(((long long)count + g.block - 1) / g.block), (unsigned)n_buffers);
    const bool taps_lds = (long long)g.L * (g.K + 1) <= RS_TAPS_LDS_MAX;
    const size_t lds = (size_t)g.span * sizeof(float2) + (taps_lds ? (size_t)g.L * (g.K + 1) * sizeof(float) : 0);
    if (taps_lds)
        hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), lds, st, io, taps_dev, n_in, n_out, first, first + count, g.M, g.L, g.D, g.K, g.block,
                           g.span);
    else
        hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), lds, st, io, taps_dev, n_in, n_out, first, first + count, g.M, g.L, g.D, g.K, g.block,
                           g.span);
    return hipGetLastError();
}

} // namespace umx
