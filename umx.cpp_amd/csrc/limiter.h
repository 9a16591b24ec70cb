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
// The true-peak detector (UMX_LIMIT_TRUE_PEAK) changes p and nothing behind it.  F, the taps h and y_b(k, f)[ch] are those of
// true_peak.h (f = 1 .. F-1, fp32 fused multiply-adds in its order, frames outside [0, N) read as +0); y(k, f) lies at time k + f/F:
//   between   e[n] = the unsigned maximum of the bit patterns of |y_b(n, f)[ch]| over b, ch and f; a NaN or +-inf value contributes
//             nothing, none left: 0; 0 at F = 1; e[-1] = 0
//   peak      p[n] = max(s[n], e[n], e[n-1]), s[n] the sample peak above: a point between two frames binds the gain of both
// So g[n] <= r[n] 2^-21 as before, y == x bit for bit where no frame within +-(W - 1) has p > c, at 192 kHz (F = 1) the gains are the
// sample detector's bit for bit, and g[n] depends on the frames n - W + 1 - 24/F .. n + W - 1 + 24/F alone, through fixed-order fp32
// chains and integers.  Within 24/F frames of a NaN or an inf the interpolated values are not finite and ignored: there the sample
// peaks alone detect.  The true peak of the LIMITED output is not bounded to the bit: the interpolator reads 24/F frames to either side
// of a point and the gain moves across them; where the gain is constant over that reach, TP(y) <= c (1 + 1e-5) (g p <= c, one product
// rounding a sample, 48/F fma roundings of 2^-24, per-phase sum |h| < 2.5).  What happened elsewhere: the report's true_peak_after.
#pragma once
#include "common.h"
#include "levels.h"
#include "true_peak.h"

namespace umx
{

constexpr uint32_t LIMIT_UNITY = 1u << 21;
constexpr int LIMIT_MAX_WINDOW = 1024;

inline int limit_window(int rate) { return rate < 1 || rate > 655350 ? 0 : rate <= 50000 ? 256 : rate <= 100000 ? 512 : 1024; }
inline int limit_log_window(int window) { return window == 256 ? 8 : window == 512 ? 9 : 10; }
inline bool limit_ceiling_ok(float c) { return c > 0.0f && c <= 1.0f; } // (a NaN: false)
inline bool limit_detector_ok(int d) { return d == UMX_LIMIT_SAMPLE_PEAK || d == UMX_LIMIT_TRUE_PEAK; }
constexpr const char *limit_tp_rate_refusal = "limiter: the true-peak detector needs a sample rate of 8000 .. 192000 Hz";

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

__device__ inline void limit_gain_finish(uint32_t *lds_a, uint32_t *lds_b, uint32_t *red, int t0, int cnt, int log_w, float *__restrict__ gain,
                                         unsigned *report);

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
    limit_gain_finish(lds_a, lds_b, red, t0, cnt, log_w, gain, report);
}

// Phases 2 and 3 of a gain kernel: lds_a holds r of the tile's cnt frames and W - 1 frames to either side, behind a barrier
__device__ inline void limit_gain_finish(uint32_t *lds_a, uint32_t *lds_b, uint32_t *red, int t0, int cnt, int log_w, float *__restrict__ gain,
                                         unsigned *report)
{
    const int W = 1 << log_w, len = cnt + 2 * W - 2;
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

// ---------------------------------------------------------------- the true-peak detector
// The gain kernel in its word-input form: phase 1 loads r of the tile and its W - 1 frames to either side from words that a detector
// launch has formed -- r[k - r_first] is frame k's, there for every frame of the track that the range's tiles read -- and is unity
// outside the track.  Phases 2 and 3 are limit_gain_kernel's.
__global__ __launch_bounds__(LIMIT_THREADS) void limit_gain_words_kernel(const uint32_t *__restrict__ r, long long r_first, long long n_track, long long first,
                                                                         int n, int log_w, float *__restrict__ gain, unsigned *report)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_a[LIMIT_LDS_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t lds_b[LIMIT_LDS_WORDS];
    __shared__ uint32_t red[2 * LIMIT_WAVES];
    const int W = 1 << log_w;
    const int t0 = LIMIT_TILE * (int)blockIdx.x;
    const int cnt = n - t0 < LIMIT_TILE ? n - t0 : LIMIT_TILE;
    const int len = cnt + 2 * W - 2;
    const long long f0 = first + t0 - (W - 1);
    for (int i = threadIdx.x; i < len; i += LIMIT_THREADS)
    {
        const long long k = f0 + i;
        lds_a[i] = k >= 0 && k < n_track ? r[k - r_first] : LIMIT_UNITY;
    }
    __syncthreads();
    limit_gain_finish(lds_a, lds_b, red, t0, cnt, log_w, gain, report);
}

// The detector: r[k - first] of the frames [first, first + count) of a track of n frames, from the interpolated waveform of ALL its
// outputs -- p is a maximum over them, so one workgroup covers every output of a tile, where true_peak_kernel gives each buffer a
// workgroup of its own.  A workgroup walks tiles of LIMIT_TP_TILE frames, gridDim.x tiles apart, and computes LIMIT_TP_TILE + 1 frames
// of each: the tile and THE FRAME IN FRONT OF IT, whose e binds the tile's first frame (1023 + 1: four frames a lane, no lane idle).
// Per output: those frames and the interpolator's halo (TP_HALO to either side) are staged as float2 in LDS, from clamped,
// unbranched, coalesced loads that are masked to +0 outside [0, n) where they are stored; the loads of the next output -- or of the
// next tile's first -- are issued into registers before this output's arithmetic and stored behind it.  Lane t takes the frames t,
// t + 256, ... of the stage: a wave reads consecutive 8-byte frames, which the LDS serves without a conflict, and a frame read feeds
// the F - 1 phases of both channels.  The integer maxima s and e of a lane's four frames stay in registers across the outputs.
// Behind the last output e goes through LDS once, so that a frame picks up e of the frame before it (another lane's, or the frame in
// front of the tile; frame -1: 0), and the double quotient of limit_required runs for a frame over the ceiling alone.  The taps are
// kernel arguments: every index is a constant after unrolling.
#define LIMIT_TP_TILE 1023
#define LIMIT_TP_FRAMES (LIMIT_TP_TILE + 1)
#define LIMIT_TP_PER (LIMIT_TP_FRAMES / LIMIT_THREADS)
#define LIMIT_TP_STAGE (LIMIT_TP_FRAMES + 2 * TP_HALO)
#define LIMIT_TP_LOADS ((LIMIT_TP_STAGE + LIMIT_THREADS - 1) / LIMIT_THREADS)
#define LIMIT_TP_MAX_BLOCKS 2048
static_assert(LIMIT_TP_FRAMES % LIMIT_THREADS == 0, "every lane takes the same number of frames");

struct LimitTpArgs
{
    const float2 *src[4]; // frame 0 of the track; the first nb are read
    TruePeakTaps taps;
    uint32_t *r;          // count words
    int nb, n, first, count; // the range lies inside [0, n)
    uint32_t c_bits;
};

template <int F> __global__ __launch_bounds__(LIMIT_THREADS) void limit_detect_tp_kernel(LimitTpArgs a)
{
    constexpr int NT = (TP_TAPS - 1) / F, BACK = F > 1 ? TP_CENTRE / F - 1 : 0;
    static_assert(F == 1 || (BACK <= TP_HALO && NT - 1 - BACK <= TP_HALO), "the halo covers the window");
    __shared__ float2 stage[LIMIT_TP_STAGE];
    __shared__ uint32_t between[LIMIT_TP_FRAMES];
    const int t = threadIdx.x, last = a.n - 1;
    const int ntiles = (a.count + LIMIT_TP_TILE - 1) / LIMIT_TP_TILE;
    float2 pre[LIMIT_TP_LOADS];
    // slot i of the stage is frame t0 - 1 - TP_HALO + i (a slot beyond the stage reads a frame of the buffer too, and is dropped)
    auto load_stage = [&](int t0, int b) {
        const float2 *__restrict__ src = a.src[b];
#pragma unroll
        for (int j = 0; j < LIMIT_TP_LOADS; ++j)
            pre[j] = src[min(max(t0 - 1 - TP_HALO + t + j * LIMIT_THREADS, 0), last)]; // (t0 <= 2^30 - 1: no overflow)
    };
    auto store_stage = [&](int t0) {
#pragma unroll
        for (int j = 0; j < LIMIT_TP_LOADS; ++j)
        {
            const int i = t + j * LIMIT_THREADS, f = t0 - 1 - TP_HALO + i;
            const uint32_t keep = f < 0 || f > last ? 0u : ~0u;
            if (i < LIMIT_TP_STAGE)
                stage[i] = make_float2(__uint_as_float(__float_as_uint(pre[j].x) & keep), __uint_as_float(__float_as_uint(pre[j].y) & keep));
        }
    };
    load_stage(a.first + (int)blockIdx.x * LIMIT_TP_TILE, 0); // (blockIdx.x < ntiles by the grid)
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int t0 = a.first + tile * LIMIT_TP_TILE; // the tile's first frame; lane t's j-th frame is t0 - 1 + t + 256 j
        uint32_t s[LIMIT_TP_PER], e[LIMIT_TP_PER];
#pragma unroll
        for (int j = 0; j < LIMIT_TP_PER; ++j)
            s[j] = e[j] = 0u;
        for (int b = 0; b < a.nb; ++b)
        {
            __syncthreads(); // the previous output has been consumed
            store_stage(t0);
            __syncthreads();
            if (b + 1 < a.nb) // what comes next is loaded under this output's arithmetic
                load_stage(t0, b + 1);
            else if (tile + (int)gridDim.x < ntiles)
                load_stage(t0 + (int)gridDim.x * LIMIT_TP_TILE, 0);
#pragma unroll
            for (int j = 0; j < LIMIT_TP_PER; ++j)
            {
                const int i = TP_HALO + t + j * LIMIT_THREADS;
                const float2 x = stage[i];
                s[j] = max(s[j], max(limit_peak_term(x.x), limit_peak_term(x.y)));
                if constexpr (F > 1)
                {
                    float yl[F], yr[F]; // (phase 0 unused)
#pragma unroll
                    for (int f = 1; f < F; ++f)
                        yl[f] = yr[f] = 0.0f;
#pragma unroll
                    for (int u = 0; u < NT; ++u) // tap u of every phase reads frame k + 24/F - u
                    {
                        const float2 w = stage[i - BACK + (NT - 1 - u)];
#pragma unroll
                        for (int f = 1; f < F; ++f)
                        {
                            yl[f] = __builtin_fmaf(a.taps.h[f + F * u], w.x, yl[f]);
                            yr[f] = __builtin_fmaf(a.taps.h[f + F * u], w.y, yr[f]);
                        }
                    }
#pragma unroll
                    for (int f = 1; f < F; ++f)
                        e[j] = max(e[j], max(limit_peak_term(yl[f]), limit_peak_term(yr[f])));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LIMIT_TP_PER; ++j) // (the barriers of the next tile's first output lie between these reads and its writes)
            between[t + j * LIMIT_THREADS] = t0 - 1 + t + j * LIMIT_THREADS >= 0 ? e[j] : 0u; // e[-1] = 0
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LIMIT_TP_PER; ++j)
        {
            const int i = t + j * LIMIT_THREADS, k = t0 - 1 + i;
            if (i >= 1 && k < a.first + a.count)
                a.r[k - a.first] = limit_required(max(s[j], max(e[j], between[i - 1])), a.c_bits);
        }
    }
}

// the words of r that launch_limit_gain_tp needs for a range of n frames
inline size_t limit_tp_scratch_words(long long n, int window) { return (size_t)(n + 2 * (long long)window - 2); }

// launch_limit_gain under the true-peak detector: the detector over the range and the W - 1 frames of the track to either side of it
// into r (limit_tp_scratch_words(n, window) words), then the gains from those words.  The caller has checked the rate (true_peak_rate_ok).
inline void launch_limit_gain_tp(int nb, const float2 *const *src, long long n_track, long long first, int n, int rate, float ceiling, uint32_t *r,
                                 float *gain, unsigned *report, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    const int window = limit_window(rate), F = true_peak_factor(rate);
    const long long lo = std::max<long long>(first - (window - 1), 0), hi = std::min<long long>(first + n + window - 1, n_track);
    LimitTpArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.src[b] = src[b];
    a.taps = true_peak_taps(F);
    a.r = r;
    a.nb = std::min(nb, 4);
    a.n = (int)n_track;
    a.first = (int)lo;
    a.count = (int)(hi - lo);
    a.c_bits = levels_bits(ceiling);
    const dim3 grid((unsigned)std::min((a.count + LIMIT_TP_TILE - 1) / LIMIT_TP_TILE, LIMIT_TP_MAX_BLOCKS));
    if (F == 4)
        hipLaunchKernelGGL(limit_detect_tp_kernel<4>, grid, dim3(LIMIT_THREADS), 0, st, a);
    else if (F == 2)
        hipLaunchKernelGGL(limit_detect_tp_kernel<2>, grid, dim3(LIMIT_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(limit_detect_tp_kernel<1>, grid, dim3(LIMIT_THREADS), 0, st, a);
    hipLaunchKernelGGL(limit_gain_words_kernel, dim3((n + LIMIT_TILE - 1) / LIMIT_TILE), dim3(LIMIT_THREADS), 0, st, r, lo, n_track, first, n,
                       limit_log_window(window), gain, report);
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

// e[k] of the true-peak detector on the host: true_peak_host_f's chains over every output and channel, the values that are not finite dropped
template <int F> inline uint32_t limit_between_host(const TruePeakTaps &tp, int nb, const float *const *x, long long n, long long k)
{
    constexpr int NT = (TP_TAPS - 1) / F, BACK = F > 1 ? TP_CENTRE / F - 1 : 0;
    uint32_t e = 0;
    for (int b = 0; F > 1 && b < nb; ++b)
        for (int ch = 0; ch < 2; ++ch)
        {
            float y[F] = {}; // (phase 0 unused)
            for (int t = 0; t < NT; ++t)
            {
                const long long fr = k - BACK + (NT - 1 - t); // frame k + 24/F - t
                const float w = fr >= 0 && fr < n ? x[b][2 * fr + ch] : 0.0f;
                for (int f = 1; f < F; ++f)
                    y[f] = __builtin_fmaf(tp.h[f + F * t], w, y[f]);
            }
            for (int f = 1; f < F; ++f)
                e = std::max(e, limit_peak_term(y[f]));
        }
    return e;
}

// The rule on the host, in one pass each: r padded by W - 1 unity frames on both sides, its sliding minimum (a monotonic queue), the
// running window sum.  gain (n floats) and y (nb buffers of n frames, may be x) may be missing.  factor: 1, the sample detector; 2 or
// 4 (true_peak_factor of the rate): the true-peak detector, p[k] = max(s[k], e[k], e[k-1]).
inline void limit_host(int nb, const float *const *x, long long n, int window, float ceiling, float *gain, float *const *y, umx_limit_report &rep,
                       int factor = 1)
{
    const long long W = window, len = n + 2 * W - 2, nm = len - W + 1;
    const uint32_t c_bits = levels_bits(ceiling);
    const TruePeakTaps tp = true_peak_taps(factor);
    std::vector<uint32_t> r((size_t)len, LIMIT_UNITY), m((size_t)nm);
    uint32_t before = 0; // e[k - 1]
    for (long long k = 0; k < n; ++k)
    {
        const uint32_t e = factor == 4 ? limit_between_host<4>(tp, nb, x, n, k) : factor == 2 ? limit_between_host<2>(tp, nb, x, n, k) : 0u;
        uint32_t p = std::max(e, before);
        before = e;
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
