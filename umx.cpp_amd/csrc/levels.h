// levels.h -- output levels and clip handling at the edge of the whole-track drivers: what leaves is measured where it is
// final, on the device, and a track can leave divided by one common divisor instead of clamped.  One statement of each rule, for the
// host entry points (umx_hip_levels_host, umx_hip_rescale_gain) and for the kernels below:
//   peak        the unsigned maximum of the bit patterns of |x| over the samples that are not NaN (+inf counts), 0 when there is none
//   over_unity  samples with |x| > 1.0f; nonfinite: NaN or +-inf
//   clipped     integer outputs only: samples whose rounded value r of the output format's encode rule (the trait's round,
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

// the divisor of a track whose largest peak has the bit pattern peak_bits (the maximum of the record's peak words); 1: none
__host__ __device__ inline float levels_divisor(uint32_t peak_bits)
{
    if (peak_bits >= LEVELS_INF_BITS)
        return 1.0f;
    const float g = 1.01f * levels_float(peak_bits);
    return g > 1.0f ? g : 1.0f;
}
// ... of the four words the divisor comes from: the record's peak words, or a true-peak record's (true_peak.h)
__host__ __device__ inline float levels_divisor(const uint32_t *words)
{
    uint32_t p = words[0];
    for (int m = 1; m < 4; ++m)
        p = words[m] > p ? words[m] : p;
    return levels_divisor(p);
}
__host__ __device__ inline float levels_divisor(const umx_levels_acc &acc) { return levels_divisor(acc.peak_bits); }
// (x over that divisor: sample_rescaled; whether a format's clamp changes a sample: sample_clips -- both in sample_format.h)

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
__global__ __launch_bounds__(LEVELS_THREADS) void stem_levels_kernel(EncodeArgs a, int clip_format, int n, umx_levels_acc *acc)
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
                    v[8 + b] += sample_clips(xs[ch], clip_format, a.dither != 0, a.key[b][ch], k) ? 1u : 0u;
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

// The encode of format T (its memory shape: encode_frames of pcm16.h / pcm24.h), plain ...
template <class T> __global__ __launch_bounds__(LEVELS_THREADS) void encode_kernel(EncodeArgs a, int n)
{
    uint32_t unused[4] = {};
    encode_frames<false>(T(), a, n, Plain(), unused);
}
// ... and on x / g, g formed here from `words`, the record's peak words or a true-peak record's (final in stream order: the measuring
// launches precede this one).
// Where the divisor is 1 these are the plain encode's bits, and only there a sample can clamp: those are counted into the record's
// `clipped`, which the measuring launches of a rescaled track leave alone.
template <class T> __global__ __launch_bounds__(LEVELS_THREADS) void encode_rescaled_kernel(EncodeArgs a, int n, umx_levels_acc *acc, const uint32_t *__restrict__ words)
{
    __shared__ uint32_t red[LEVELS_WAVES * 4];
    const float g = levels_divisor(words);
    uint32_t v[4] = {};
    encode_frames<true>(T(), a, n, Rescaled{g, g != 1.0f}, v);
    const uint32_t total = levels_block_reduce<4, 0>(v, red);
    if (threadIdx.x < 4 && total != 0)
        atomicAdd(&acc->clipped[threadIdx.x], (unsigned long long)total);
}

struct RescaleBufs
{
    float2 *p[4]; // nullptr: none
};

// x / g in place over n frames of up to four buffers; divisor 1: nothing is written
__global__ __launch_bounds__(LEVELS_THREADS) void stem_rescale_kernel(RescaleBufs a, int n, const uint32_t *__restrict__ words)
{
    const float g = levels_divisor(words);
    if (g == 1.0f)
        return;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.p[b])
            {
                const float2 x = a.p[b][i];
                a.p[b][i] = make_float2(sample_rescaled(x.x, g), sample_rescaled(x.y, g));
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
    hipLaunchKernelGGL(stem_levels_kernel, dim3(levels_blocks(n)), dim3(LEVELS_THREADS), 0, st,
                       encode_args(nb, src, nullptr, first_frame, dither, seed), clip_format, n, acc);
}

// the device address of a device record's peak words (no access: the record's first member)
inline const uint32_t *levels_peak_words(const umx_levels_acc *acc_dev) { return reinterpret_cast<const uint32_t *>(acc_dev); }
static_assert(offsetof(umx_levels_acc, peak_bits) == 0, "the peak words lead the record");

// the same buffers into dst (byte addresses) as `format` encodes them; acc: over the divisor of `words` (nullptr: that record's peak
// words), counting into the record (acc nullptr: the plain encode).  An fp32 format: nothing.
inline void launch_encode(int format, int nb, const float2 *const *src, uint8_t *const *dst, int n, long long first_frame, bool dither,
                          uint32_t seed, umx_levels_acc *acc, hipStream_t st, const uint32_t *words = nullptr)
{
    if (n < 1 || nb < 1)
        return;
    const EncodeArgs a = encode_args(nb, src, dst, first_frame, dither, seed);
    with_sample_format(format, [&](auto t) {
        using T = decltype(t);
        if (acc)
            hipLaunchKernelGGL(encode_rescaled_kernel<T>, dim3(encode_blocks(t, n)), dim3(LEVELS_THREADS), 0, st, a, n, acc,
                               words ? words : levels_peak_words(acc));
        else
            hipLaunchKernelGGL(encode_kernel<T>, dim3(encode_blocks(t, n)), dim3(LEVELS_THREADS), 0, st, a, n);
    });
}

// n frames of `format` at `in` -> out[0 .. n)
inline void launch_decode(int format, const void *in, float2 *out, int n, hipStream_t st)
{
    if (n >= 1)
        with_sample_format(format, [&](auto t) { launch_decode_as(t, in, out, n, st); });
}

inline void launch_stem_rescale(int nb, float2 *const *bufs, int n, const uint32_t *words, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    RescaleBufs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.p[b] = bufs[b];
    hipLaunchKernelGGL(stem_rescale_kernel, dim3(pcm16_blocks(n)), dim3(LEVELS_THREADS), 0, st, a, n, words);
}

// the rules over n_frames interleaved stereo frames of output buffer `buffer`, into a host record (umx_hip_levels_host)
inline void levels_host(const float *x, int n_frames, int buffer, long long first_frame, int clip_format, bool dither, uint32_t seed,
                        float divisor, umx_levels_acc &acc)
{
    const uint32_t key[2] = {sample_dither_key(seed, buffer, 0), sample_dither_key(seed, buffer, 1)};
    for (int i = 0; i < n_frames; ++i)
        for (int ch = 0; ch < 2; ++ch)
        {
            const float s = x[2 * (size_t)i + ch];
            const uint32_t u = levels_abs_bits(s), p = levels_peak_term(u);
            acc.peak_bits[buffer] = p > acc.peak_bits[buffer] ? p : acc.peak_bits[buffer];
            acc.over_unity[buffer] += levels_is_over_unity(u) ? 1 : 0;
            acc.nonfinite[buffer] += levels_is_nonfinite(u) ? 1 : 0;
            acc.clipped[buffer] += sample_clips(divisor != 1.0f ? sample_rescaled(s, divisor) : s, clip_format, dither, key[ch], first_frame + i) ? 1 : 0;
        }
}

// what a whole-track call reports from a job's record; `words`: what its divisor came from
inline void levels_report(const umx_levels_acc &acc, int n_out, bool rescaled, const uint32_t *words, umx_levels &lv)
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
    lv.gain = rescaled ? levels_divisor(words) : 1.0f;
}

inline const char *clip_mode_refusal(int clip_mode)
{
    return clip_mode == UMX_CLIP_CLAMP || clip_mode == UMX_CLIP_RESCALE ? nullptr : "clip mode: unknown (UMX_CLIP_CLAMP or UMX_CLIP_RESCALE)";
}

} // namespace umx
