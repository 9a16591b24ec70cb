// limiter.h -- a look-ahead peak limiter at the edge of the whole-track drivers: gain dips only around the frames that
// exceed a ceiling, ramps down before a peak arrives, and every frame farther than a window from an over leaves bit for bit.  One
// statement of the rule, for the host entry point (limit_host), the kernels below and the header (include/umx_hip.h):
//   peak      p[n] = the unsigned maximum of the bit patterns of |x_b[n][ch]| over the B = 1 .. 4 outputs and both channels; NaN and
//             +-inf are ignored, none left: 0
//   required  r[n] = 2^21 if p[n] <= c, else max(1, floor(((double)c / (double)p[n]) * 2097152.0)); 2^21 for n < 0 and n >= N
//   window    W = 256 frames for a rate <= 50000 Hz, 512 for <= 100000 Hz, 1024 above
//   minimum   m[k] = min(r[k .. k + W - 1]);   sum  S[n] = m[n - W + 1] + ... + m[n]  (<= 1024 * 2^21 = 2^31: exact in 32 bits)
//   gain      q[n] = S[n] / W (a shift), g[n] = (float)q[n] * 2^-21 (exact);   output  y_b[n][ch] = x_b[n][ch] * g[n], one fp32 product
//   report    min_gain = the smallest g, limited_frames = the frames with g < 1: an integer minimum and an integer count over q
// So g[n] <= r[n] 2^-21 (|y| <= nextafterf(c, inf) wherever p[n] < 2^20), g[n] == 1.0f where no frame within +-(W - 1) exceeds c, a NaN
// stays a NaN and an inf an inf (g > 0) without pulling the gain down, and g[n] depends on the frames n - W + 1 .. n + W - 1 alone,
// through integers: tiles, ranges, lanes and reruns give the same bits.
// The report words on the device: word 0 is the DEFICIT 2^21 - min q (an unsigned maximum), word 1 the count, so that zeroed words are
// the report of an untouched track.
#pragma once
#include "common.h"
#include "levels.h"

namespace umx
{

constexpr uint32_t LIMIT_UNITY = 1u << 21;
constexpr int LIMIT_MAX_WINDOW = 1024;

inline int limit_window(int rate) { return rate < 1 || rate > 655350 ? 0 : rate <= 50000 ? 256 : rate <= 100000 ? 512 : 1024; }
inline bool limit_ceiling_ok(float c) { return c > 0.0f && c <= 1.0f; } // (a NaN: false)

// what a sample contributes to a frame's peak: the bit pattern of |x|, nothing for a NaN or an inf
__host__ __device__ inline uint32_t limit_peak_term(float x)
{
    const uint32_t u = levels_abs_bits(x);
    return levels_is_nonfinite(u) ? 0u : u;
}
// r of a frame whose peak has the bit pattern p; c_bits: the ceiling's
__host__ __device__ inline uint32_t limit_required(uint32_t p, uint32_t c_bits)
{
    if (p <= c_bits)
        return LIMIT_UNITY;
    const double r = floor(((double)levels_float(c_bits) / (double)levels_float(p)) * 2097152.0);
    return r < 1.0 ? 1u : (uint32_t)r;
}
__host__ __device__ inline float limit_gain_of(uint32_t q) { return (float)q * 4.76837158203125e-07f; } // q 2^-21, exact: q <= 2^21

#define LIMIT_THREADS 256
#define LIMIT_WAVES (LIMIT_THREADS / 64)
// A workgroup's tile: T frames of gain from T + 2 W - 2 frames of r.  Two LDS arrays of that many words (and 10 words of slack each for
// the 16-byte reads past the valid end, rounded to 16 bytes): 2 x 6152 x 4 = 49216 bytes at every W, three workgroups in a CU's 160 KiB.
#define LIMIT_TILE 4096
#define LIMIT_LDS_WORDS (LIMIT_TILE + 2 * LIMIT_MAX_WINDOW - 2 + 10)
static_assert(LIMIT_LDS_WORDS % 4 == 0, "the arrays are read 16 bytes at a time");

struct LimitSrc
{
    const float2 *p[4]; // frame 0 of the track; nullptr: none.  All share their address modulo 16 (`odd`)
};

struct LimitMin
{
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};
struct LimitSum
{
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};

// The window reduction of both passes, by doubling: out[i] = op(in[i], in[i + 2^j]) for j = 0 .. log_w - 1 leaves op over in[i .. i + W - 1]
// at i.  `len` valid words in `a` going in, len - W + 1 coming out; the passes alternate between the two arrays (a lane reads words
// that another lane of the same pass replaces), one barrier a pass.  Four words a lane and step, read as 16-byte pieces: the piece at
// i + s itself where s is a multiple of 4, else the pieces at i and i + 4, from which the words i + s .. i + s + 3 are picked.  Words
// past the valid end are read (inside the arrays: their slack) and only reach words past the new valid end.
// Returns the array that holds the result; entered and left behind a barrier.
template <class Op> __device__ inline uint32_t *limit_window_reduce(uint32_t *a, uint32_t *b, int len, int log_w, Op op)
{
    for (int j = 0; j < log_w; ++j)
    {
        const int s = 1 << j;
        len -= s;
        for (int i = 4 * (int)threadIdx.x; i < len; i += 4 * LIMIT_THREADS)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(a + i);
            uint4 w;
            if (s >= 4)
                w = *reinterpret_cast<const uint4 *>(a + i + s);
            else
            {
                const uint4 n = *reinterpret_cast<const uint4 *>(a + i + 4);
                w = s == 1 ? make_uint4(v.y, v.z, v.w, n.x) : make_uint4(v.z, v.w, n.x, n.y);
            }
            *reinterpret_cast<uint4 *>(b + i) = make_uint4(op(v.x, w.x), op(v.y, w.y), op(v.z, w.z), op(v.w, w.w));
        }
        __syncthreads();
        uint32_t *t = a;
        a = b;
        b = t;
    }
    return a;
}

// Frames [first + T blockIdx.x, ...) of the range [first, first + n) of a track of n_track frames: gain[k - first] = g[k], and the
// range's part of the report.  Word i of the arrays is frame f0 + i, f0 = the tile's first frame - (W - 1).
__global__ __launch_bounds__(LIMIT_THREADS) void limit_gain_kernel(LimitSrc src, int odd, long long n_track, long long first, int n, int log_w,
                                                                   uint32_t c_bits, float *__restrict__ gain, unsigned *report)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_a[LIMIT_LDS_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t lds_b[LIMIT_LDS_WORDS];
    __shared__ uint32_t red[2 * LIMIT_WAVES];
    const int W = 1 << log_w;
    const int t0 = LIMIT_TILE * (int)blockIdx.x;                 // the tile's first frame, in the range
    const int cnt = n - t0 < LIMIT_TILE ? n - t0 : LIMIT_TILE;   // its frames
    const int len = cnt + 2 * W - 2;                             // words of r
    const long long f0 = first + t0 - (W - 1);
    // Phase 1: r into lds_a.  A lane takes 16-byte pieces, two frames of every output: the pair (2 j - e, 2 j - e + 1) of words, e
    // chosen so that the pair's first frame sits at a multiple of 16 bytes in every buffer.  A pair that straddles an end of the track
    // or of the array is read frame by frame; frames outside the track are unity.
    const int e = (int)((f0 + odd) & 1);
    for (int j = threadIdx.x; 2 * j - e < len; j += LIMIT_THREADS)
    {
        const int i = 2 * j - e;
        const long long k = f0 + i;
        uint32_t p0 = 0, p1 = 0;
        const bool in0 = i >= 0 && k >= 0 && k < n_track, in1 = i + 1 < len && k + 1 >= 0 && k + 1 < n_track;
        if (in0 && in1)
        {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (src.p[b])
                {
                    const float4 x = *reinterpret_cast<const float4 *>(src.p[b] + k);
                    p0 = max(p0, max(limit_peak_term(x.x), limit_peak_term(x.y)));
                    p1 = max(p1, max(limit_peak_term(x.z), limit_peak_term(x.w)));
                }
        }
        else
        {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (src.p[b])
                {
                    if (in0)
                    {
                        const float2 x = src.p[b][k];
                        p0 = max(p0, max(limit_peak_term(x.x), limit_peak_term(x.y)));
                    }
                    if (in1)
                    {
                        const float2 x = src.p[b][k + 1];
                        p1 = max(p1, max(limit_peak_term(x.x), limit_peak_term(x.y)));
                    }
                }
        }
        if (i >= 0)
            lds_a[i] = limit_required(p0, c_bits); // (a frame outside the track: p = 0, unity)
        if (i + 1 < len)
            lds_a[i + 1] = limit_required(p1, c_bits);
    }
    __syncthreads();
    // Phase 2: m[f0 + i] at word i (len - W + 1 of them), then S[k] at the word of k - W + 1: frame t0 + o of the range at word o
    uint32_t *m = limit_window_reduce(lds_a, lds_b, len, log_w, LimitMin());
    const uint32_t *S = limit_window_reduce(m, m == lds_a ? lds_b : lds_a, len - W + 1, log_w, LimitSum());
    // Phase 3: the gains, and the tile's smallest q (as the largest deficit) and its count of q below unity
    uint32_t deficit = 0, limited = 0;
    for (int o = threadIdx.x; o < cnt; o += LIMIT_THREADS)
    {
        const uint32_t q = S[o] >> log_w;
        gain[(size_t)t0 + o] = limit_gain_of(q);
        deficit = max(deficit, LIMIT_UNITY - q);
        limited += q < LIMIT_UNITY ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        deficit = max(deficit, (uint32_t)__shfl_xor((int)deficit, d, 64));
        limited += (uint32_t)__shfl_xor((int)limited, d, 64);
    }
    if ((threadIdx.x & 63) == 0)
    {
        red[threadIdx.x >> 6] = deficit;
        red[LIMIT_WAVES + (threadIdx.x >> 6)] = limited;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < LIMIT_WAVES; ++w)
        {
            deficit = max(deficit, red[w]);
            limited += red[LIMIT_WAVES + w];
        }
        if (limited) // (an untouched tile adds nothing)
        {
            atomicMax(&report[0], deficit);
            atomicAdd(&report[1], limited);
        }
    }
}

struct LimitBufs
{
    float2 *p[4]; // the range's first frame; nullptr: none.  All share their address modulo 16 (`odd`)
};

// y = x g in place over n frames, 16 bytes (two frames) of every buffer a lane and step: the pair (2 j - odd, 2 j - odd + 1), a frame
// alone at an end.  Nothing is written where the lane's gains are both 1.0f.
__global__ __launch_bounds__(LIMIT_THREADS) void limit_apply_kernel(LimitBufs a, int odd, int n, const float *__restrict__ gain)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * (long long)j - odd < n; j += step)
    {
        const long long i = 2 * (long long)j - odd;
        const bool in0 = i >= 0, in1 = i + 1 < n;
        const float g0 = in0 ? gain[i] : 1.0f, g1 = in1 ? gain[i + 1] : 1.0f;
        if (g0 == 1.0f && g1 == 1.0f)
            continue;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.p[b])
            {
                if (in0 && in1)
                {
                    float4 *p = reinterpret_cast<float4 *>(a.p[b] + i);
                    const float4 x = *p;
                    *p = make_float4(x.x * g0, x.y * g0, x.z * g1, x.w * g1);
                }
                else
                {
                    float2 *p = a.p[b] + (in0 ? i : i + 1);
                    const float g = in0 ? g0 : g1;
                    const float2 x = *p;
                    *p = make_float2(x.x * g, x.y * g);
                }
            }
    }
}

inline int limit_log_window(int window) { return window == 256 ? 8 : window == 512 ? 9 : 10; }
// 1 .. 4 buffers that share their address modulo 16 (a multiple of 8): 0 or 1, the frames in front of the first 16-byte boundary; -1: they do not
template <class P> inline int limit_phase(int nb, P *const *bufs)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(bufs[0]);
    for (int b = 0; b < nb; ++b)
        if ((reinterpret_cast<uintptr_t>(bufs[b]) & 7) != 0 || ((reinterpret_cast<uintptr_t>(bufs[b]) ^ a0) & 15) != 0)
            return -1;
    return (int)((a0 >> 3) & 1);
}

// frames [first, first + n) of a track of n_track frames whose frame 0 is at src[b]: gain[0 .. n) and the report words (added to)
inline void launch_limit_gain(int nb, const float2 *const *src, long long n_track, long long first, int n, int window, float ceiling, float *gain,
                              unsigned *report, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    LimitSrc a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.p[b] = src[b];
    hipLaunchKernelGGL(limit_gain_kernel, dim3((n + LIMIT_TILE - 1) / LIMIT_TILE), dim3(LIMIT_THREADS), 0, st, a, limit_phase(nb, src), n_track, first, n,
                       limit_log_window(window), levels_bits(ceiling), gain, report);
}
inline void launch_limit_apply(int nb, float2 *const *bufs, int n, const float *gain, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    LimitBufs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.p[b] = bufs[b];
    const int pairs = n / 2 + 1;
    hipLaunchKernelGGL(limit_apply_kernel, dim3(std::max(1, std::min((pairs + LIMIT_THREADS - 1) / LIMIT_THREADS, 4096))), dim3(LIMIT_THREADS), 0, st, a,
                       limit_phase(nb, bufs), n, gain);
}

// the report of the device's two words
inline void limit_report_of(const unsigned *words, umx_limit_report &r)
{
    r.min_gain = limit_gain_of(LIMIT_UNITY - words[0]);
    r.limited_frames = words[1];
}

// The rule on the host, in one pass each: r padded by W - 1 unity frames on both sides, its sliding minimum (a monotonic queue), the
// running window sum.  gain (n floats) and y (nb buffers of n frames, may be x) may be missing.
inline void limit_host(int nb, const float *const *x, long long n, int window, float ceiling, float *gain, float *const *y, umx_limit_report &rep)
{
    const long long W = window, len = n + 2 * W - 2, nm = len - W + 1;
    const uint32_t c_bits = levels_bits(ceiling);
    std::vector<uint32_t> r((size_t)len, LIMIT_UNITY), m((size_t)nm);
    for (long long k = 0; k < n; ++k)
    {
        uint32_t p = 0;
        for (int b = 0; b < nb; ++b)
            for (int ch = 0; ch < 2; ++ch)
                p = std::max(p, limit_peak_term(x[b][2 * k + ch]));
        r[(size_t)(k + W - 1)] = limit_required(p, c_bits);
    }
    std::vector<long long> queue((size_t)len); // indices of r, their values increasing from head to tail
    long long head = 0, tail = 0;
    for (long long i = 0; i < len; ++i)
    {
        while (tail > head && r[(size_t)queue[(size_t)tail - 1]] >= r[(size_t)i])
            --tail;
        queue[(size_t)tail++] = i;
        if (queue[(size_t)head] <= i - W)
            ++head;
        if (i >= W - 1)
            m[(size_t)(i - W + 1)] = r[(size_t)queue[(size_t)head]];
    }
    unsigned long long S = 0;
    uint32_t qmin = LIMIT_UNITY;
    rep.limited_frames = 0;
    const int log_w = limit_log_window(window);
    for (long long i = 0; i < nm; ++i) // word i of m is frame i - (W - 1); S[k] sums the words k .. k + W - 1
    {
        S += m[(size_t)i];
        if (i >= W)
            S -= m[(size_t)(i - W)];
        const long long k = i - (W - 1);
        if (k < 0)
            continue;
        const uint32_t q = (uint32_t)(S >> log_w);
        const float g = limit_gain_of(q);
        qmin = std::min(qmin, q);
        rep.limited_frames += q < LIMIT_UNITY ? 1 : 0;
        if (gain)
            gain[k] = g;
        for (int b = 0; y && b < nb; ++b)
            for (int ch = 0; ch < 2; ++ch)
                y[b][2 * k + ch] = x[b][2 * k + ch] * g;
    }
    rep.min_gain = limit_gain_of(qmin);
}

} // namespace umx
