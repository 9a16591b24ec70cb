// levels.h -- output levels and clip handling at the edge of the whole-track drivers: what leaves is measured where it is
// final, on the device, and a track can leave divided by one common divisor instead of clamped.  One statement of each rule, for the
// host entry points (umx_hip_levels_host, umx_hip_rescale_gain) and for the kernels below:
//   peak        the unsigned maximum of the bit patterns of |x| over the samples that are not NaN (+inf counts), 0 when there is none
//   over_unity  samples with |x| > 1.0f; nonfinite: NaN or +-inf
//   clipped     integer outputs only: samples whose rounded value r of the output format's encode rule (pcm16_round / pcm24_round,
//               with its dither, on x / g when a divisor applies) lies outside the format's codes: > 32767.f or < -32768.f for
//               int16, > 8388607 or < -8388608 for packed 24-bit; +-inf counts, NaN does not
//   rescale     P = max peak over the outputs that leave, g = 1.01f * P (one fp32 product); P not finite or !(g > 1.0f): divisor 1,
//               nothing is divided; else every sample is x / g, correctly rounded, and the unchanged encode follows
// All of it is maxima and integer counts: regions, lanes, the queue and a rerun give the same record.  The record (umx_levels_acc) is
// in HBM and accumulates across launches: per workgroup one unsigned max and up to three 64-bit integer adds per buffer, no float atomics.
#pragma once
#include "common.h"
#include "pcm16.h"
#include "pcm24.h"

namespace umx
{

__host__ __device__ inline uint32_t levels_bits(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
#endif
}
__host__ __device__ inline float levels_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, sizeof x);
    return x;
#endif
}

constexpr uint32_t LEVELS_INF_BITS = 0x7f800000u, LEVELS_ONE_BITS = 0x3f800000u;

// the bit pattern of |x|: ordered as the magnitudes are, +inf above every finite value, every NaN above +inf
__host__ __device__ inline uint32_t levels_abs_bits(float x) { return levels_bits(x) & 0x7fffffffu; }
__host__ __device__ inline bool levels_is_nan(uint32_t abs_bits) { return abs_bits > LEVELS_INF_BITS; }
__host__ __device__ inline bool levels_is_nonfinite(uint32_t abs_bits) { return abs_bits >= LEVELS_INF_BITS; }
__host__ __device__ inline bool levels_is_over_unity(uint32_t abs_bits) { return abs_bits > LEVELS_ONE_BITS && abs_bits <= LEVELS_INF_BITS; }
// what a sample contributes to the peak (a NaN: nothing)
__host__ __device__ inline uint32_t levels_peak_term(uint32_t abs_bits) { return levels_is_nan(abs_bits) ? 0u : abs_bits; }
// did the clamp of the encode rule change the rounded value r (a NaN r: no)
__host__ __device__ inline bool levels_is_clipped(float r) { return r > 32767.f || r < -32768.f; }
// the same question of sample x as it leaves in clip_format (UMX_SAMPLE_S16 or UMX_SAMPLE_S24; an fp32 output: never)
__host__ __device__ inline bool levels_clips(float x, int clip_format, bool dither, uint32_t key, long long k)
{
    if (clip_format == UMX_SAMPLE_S16)
        return levels_is_clipped(pcm16_round(x, dither, key, k));
    if (clip_format == UMX_SAMPLE_S24)
        return pcm24_is_clipped(pcm24_round(x, dither, key, k));
    return false;
}

// the divisor of a track whose largest peak has the bit pattern peak_bits (the maximum of the record's peak words); 1: none
__host__ __device__ inline float levels_divisor(uint32_t peak_bits)
{
    if (peak_bits >= LEVELS_INF_BITS)
        return 1.0f;
    const float g = 1.01f * levels_float(peak_bits);
    return g > 1.0f ? g : 1.0f;
}
__host__ __device__ inline float levels_divisor(const umx_levels_acc &acc)
{
    uint32_t p = acc.peak_bits[0];
    for (int m = 1; m < 4; ++m)
        p = acc.peak_bits[m] > p ? acc.peak_bits[m] : p;
    return levels_divisor(p);
}
// x over a divisor g > 1 (levels_divisor's other answer, 1, divides nothing: the callers test for it)
__host__ __device__ inline float levels_rescaled(float x, float g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(x, g);
#else
    return x / g;
#endif
}

// src[b] from the first frame on; b = the output's index in the call's `out` list, nullptr: none
struct LevelsArgs
{
    const float2 *src[4];
    uint32_t key[4][2]; // pcm16_dither_key of (seed, b, channel)
    long long first_frame;
    int dither;
    int clip_format; // UMX_SAMPLE_S16 / UMX_SAMPLE_S24: the outputs leave through that format's plain encode, count what it clamps; else nothing
};

#define LEVELS_THREADS 256
#define LEVELS_WAVES (LEVELS_THREADS / 64)

// NV values per thread, the first NMAX of them maxima and the rest sums, over the workgroup: wave by wave with shuffles, the waves
// through LDS (red: LEVELS_WAVES * NV words).  Thread i < NV returns the workgroup's value i.
template <int NV, int NMAX> __device__ inline uint32_t levels_block_reduce(uint32_t (&v)[NV], uint32_t *red)
{
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
        {
            const uint32_t o = (uint32_t)__shfl_xor((int)v[i], d, 64);
            v[i] = i < NMAX ? (o > v[i] ? o : v[i]) : v[i] + o;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i)
            red[wave * NV + i] = v[i];
    __syncthreads();
    uint32_t total = 0;
    if (threadIdx.x < NV)
        for (int w = 0; w < LEVELS_WAVES; ++w)
        {
            const uint32_t o = red[w * NV + threadIdx.x];
            total = (int)threadIdx.x < NMAX ? (o > total ? o : total) : total + o;
        }
    return total;
}

// n frames of up to four buffers, one frame per thread, grid-strided: frame i of buffer b is frame first_frame + i of the caller's
// track.  8 B read per frame and buffer; per workgroup one atomic per quantity and buffer that has something to add.
__global__ __launch_bounds__(LEVELS_THREADS) void stem_levels_kernel(LevelsArgs a, int n, umx_levels_acc *acc)
{
    __shared__ uint32_t red[LEVELS_WAVES * 16];
    uint32_t v[16] = {}; // [quantity: peak, over_unity, clipped, nonfinite][buffer]
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        const long long k = a.first_frame + (long long)i;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.src[b])
            {
                const float2 x = a.src[b][i];
                const float xs[2] = {x.x, x.y};
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)
                {
                    const uint32_t u = levels_abs_bits(xs[ch]);
                    const uint32_t p = levels_peak_term(u);
                    v[b] = p > v[b] ? p : v[b];
                    v[4 + b] += levels_is_over_unity(u) ? 1u : 0u;
                    if (a.clip_format == UMX_SAMPLE_S16)
                        v[8 + b] += levels_is_clipped(pcm16_round(xs[ch], a.dither != 0, a.key[b][ch], k)) ? 1u : 0u;
                    else if (a.clip_format == UMX_SAMPLE_S24)
                        v[8 + b] += pcm24_is_clipped(pcm24_round(xs[ch], a.dither != 0, a.key[b][ch], k)) ? 1u : 0u;
                    v[12 + b] += levels_is_nonfinite(u) ? 1u : 0u;
                }
            }
    }
    const uint32_t total = levels_block_reduce<16, 4>(v, red);
    const int q = threadIdx.x >> 2, b = threadIdx.x & 3;
    if (threadIdx.x < 16 && total != 0)
    {
        if (q == 0)
            atomicMax(&acc->peak_bits[b], total);
        else
            atomicAdd(q == 1 ? &acc->over_unity[b] : q == 2 ? &acc->clipped[b] : &acc->nonfinite[b], (unsigned long long)total);
    }
}

// pcm16_encode_kernel on x / g, g formed here from the record's peak words (final in stream order: the measuring launches precede
// this one).  Where the divisor is 1 these are the plain encode's bits, and only there a sample can clamp: those are counted into
// the record's `clipped`, which the measuring launches of a rescaled track leave alone.
__global__ __launch_bounds__(LEVELS_THREADS) void pcm16_encode_rescaled_kernel(Pcm16EncodeArgs a, int n, umx_levels_acc *acc)
{
    __shared__ uint32_t red[LEVELS_WAVES * 4];
    const float g = levels_divisor(*acc);
    const bool divide = g != 1.0f;
    uint32_t v[4] = {};
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        const long long k = a.first_frame + (long long)i;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.dst[b])
            {
                float2 x = a.src[b][i];
                if (divide)
                    x = make_float2(levels_rescaled(x.x, g), levels_rescaled(x.y, g));
                v[b] += (levels_is_clipped(pcm16_round(x.x, a.dither != 0, a.key[b][0], k)) ? 1u : 0u) +
                        (levels_is_clipped(pcm16_round(x.y, a.dither != 0, a.key[b][1], k)) ? 1u : 0u);
                a.dst[b][i] = pcm16_frame(pcm16_encode(x.x, a.dither != 0, a.key[b][0], k), pcm16_encode(x.y, a.dither != 0, a.key[b][1], k));
            }
    }
    const uint32_t total = levels_block_reduce<4, 0>(v, red);
    if (threadIdx.x < 4 && total != 0)
        atomicAdd(&acc->clipped[threadIdx.x], (unsigned long long)total);
}

// pcm24_encode_kernel (pcm24.h) on x / g, the twin of the kernel above: the same divisor, the same count of what it clamps
struct Pcm24Rescaled
{
    float g;
    bool divide;
    __device__ float operator()(float x) const { return divide ? levels_rescaled(x, g) : x; }
};
__global__ __launch_bounds__(LEVELS_THREADS) void pcm24_encode_rescaled_kernel(Pcm24EncodeArgs a, int n, umx_levels_acc *acc)
{
    __shared__ uint32_t red[LEVELS_WAVES * 4];
    const float g = levels_divisor(*acc);
    uint32_t v[4] = {};
    pcm24_encode_frames<true>(a, n, Pcm24Rescaled{g, g != 1.0f}, v);
    const uint32_t total = levels_block_reduce<4, 0>(v, red);
    if (threadIdx.x < 4 && total != 0)
        atomicAdd(&acc->clipped[threadIdx.x], (unsigned long long)total);
}

struct RescaleBufs
{
    float2 *p[4]; // nullptr: none
};

// x / g in place over n frames of up to four buffers; divisor 1: nothing is written
__global__ __launch_bounds__(LEVELS_THREADS) void stem_rescale_kernel(RescaleBufs a, int n, const umx_levels_acc *__restrict__ acc)
{
    const float g = levels_divisor(*acc);
    if (g == 1.0f)
        return;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.p[b])
            {
                const float2 x = a.p[b][i];
                a.p[b][i] = make_float2(levels_rescaled(x.x, g), levels_rescaled(x.y, g));
            }
}

// (fewer, longer workgroups than the encode's: every workgroup ends in up to 16 atomics on one record)
inline int levels_blocks(int n) { return std::max(1, std::min((n + LEVELS_THREADS - 1) / LEVELS_THREADS, 1024)); }

// buffers 0 .. nb-1 of a call's `out` list, n frames from frame first_frame of the caller's track on, into the record acc
inline void launch_stem_levels(int nb, const float2 *const *src, int n, long long first_frame, int clip_format, bool dither, uint32_t seed,
                               umx_levels_acc *acc, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    LevelsArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
    {
        a.src[b] = src[b];
        a.key[b][0] = pcm16_dither_key(seed, b, 0);
        a.key[b][1] = pcm16_dither_key(seed, b, 1);
    }
    a.first_frame = first_frame;
    a.dither = dither ? 1 : 0;
    a.clip_format = clip_format;
    hipLaunchKernelGGL(stem_levels_kernel, dim3(levels_blocks(n)), dim3(LEVELS_THREADS), 0, st, a, n, acc);
}

inline void launch_pcm16_encode_rescaled(int nb, const float2 *const *src, uint32_t *const *dst, int n, long long first_frame, bool dither,
                                         uint32_t seed, umx_levels_acc *acc, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    Pcm16EncodeArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
    {
        a.src[b] = src[b];
        a.dst[b] = dst[b];
        a.key[b][0] = pcm16_dither_key(seed, b, 0);
        a.key[b][1] = pcm16_dither_key(seed, b, 1);
    }
    a.first_frame = first_frame;
    a.dither = dither ? 1 : 0;
    hipLaunchKernelGGL(pcm16_encode_rescaled_kernel, dim3(pcm16_blocks(n)), dim3(LEVELS_THREADS), 0, st, a, n, acc);
}

inline void launch_pcm24_encode_rescaled(int nb, const float2 *const *src, uint8_t *const *dst, int n, long long first_frame, bool dither,
                                         uint32_t seed, umx_levels_acc *acc, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    hipLaunchKernelGGL(pcm24_encode_rescaled_kernel, dim3(pcm24_blocks(n)), dim3(LEVELS_THREADS), 0, st,
                       pcm24_encode_args(nb, src, dst, first_frame, dither, seed), n, acc);
}

inline void launch_stem_rescale(int nb, float2 *const *bufs, int n, const umx_levels_acc *acc, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    RescaleBufs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.p[b] = bufs[b];
    hipLaunchKernelGGL(stem_rescale_kernel, dim3(pcm16_blocks(n)), dim3(LEVELS_THREADS), 0, st, a, n, acc);
}

// the rules over n_frames interleaved stereo frames of output buffer `buffer`, into a host record (umx_hip_levels_host)
inline void levels_host(const float *x, int n_frames, int buffer, long long first_frame, int clip_format, bool dither, uint32_t seed,
                        float divisor, umx_levels_acc &acc)
{
    const uint32_t key[2] = {pcm16_dither_key(seed, buffer, 0), pcm16_dither_key(seed, buffer, 1)};
    for (int i = 0; i < n_frames; ++i)
        for (int ch = 0; ch < 2; ++ch)
        {
            const float s = x[2 * (size_t)i + ch];
            const uint32_t u = levels_abs_bits(s), p = levels_peak_term(u);
            acc.peak_bits[buffer] = p > acc.peak_bits[buffer] ? p : acc.peak_bits[buffer];
            acc.over_unity[buffer] += levels_is_over_unity(u) ? 1 : 0;
            acc.nonfinite[buffer] += levels_is_nonfinite(u) ? 1 : 0;
            acc.clipped[buffer] += levels_clips(divisor != 1.0f ? levels_rescaled(s, divisor) : s, clip_format, dither, key[ch], first_frame + i) ? 1 : 0;
        }
}

// what a whole-track call reports from a job's record
inline void levels_report(const umx_levels_acc &acc, int n_out, bool rescaled, umx_levels &lv)
{
    lv = umx_levels{};
    lv.n_out = n_out;
    for (int m = 0; m < 4; ++m)
    {
        lv.peak[m] = levels_float(acc.peak_bits[m]);
        lv.over_unity[m] = acc.over_unity[m];
        lv.clipped[m] = acc.clipped[m];
        lv.nonfinite[m] = acc.nonfinite[m];
    }
    lv.gain = rescaled ? levels_divisor(acc) : 1.0f;
}

inline const char *clip_mode_refusal(int clip_mode)
{
    return clip_mode == UMX_CLIP_CLAMP || clip_mode == UMX_CLIP_RESCALE ? nullptr : "clip mode: unknown (UMX_CLIP_CLAMP or UMX_CLIP_RESCALE)";
}

} // namespace umx
