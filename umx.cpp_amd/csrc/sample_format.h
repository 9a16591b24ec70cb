// sample_format.h -- what a sample format at the edge of the whole-track drivers IS, stated once for pcm16.h, pcm24.h and
// levels.h, for their kernels and for the host entry points:
//   dither      TPDF, counter based: d depends on (seed, output buffer m, channel ch, frame k of the CALLER's track) alone, so regions,
//               lanes and a rerun after a timeout give the same bits.  h = the 32-bit mixer below,
//               a = h(seed + 0x9e3779b9 (2 m + ch + 1)), w = h(a ^ (uint32)k), d = ((w & 0xffff) + (w >> 16) - 65535) / 65536: the sum
//               of two uniform 16-bit integers, in (-1, 1), every step exact in fp32.  Both integer formats add it in their own LSB.
//   a format    a compile-time trait per integer format (SampleS16, SampleS24) with the SAMPLE rule only: round, is_clipped, clamp,
//               the frame's bytes and the alignment an entry point asks of a buffer.  How frames move through memory is not part of
//               it: that is encode_frames / launch_decode_as of pcm16.h (a frame per thread) and pcm24.h (a pair of frames per lane).
//   dispatch    with_sample_format: the one place where a UMX_SAMPLE_* value picks a trait
//   EncodeArgs  up to four buffers of a call's `out` list with their dither keys; encode_args fills it
#pragma once
#include "common.h"

namespace umx
{

__host__ __device__ inline uint32_t sample_hash(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// the key of one (seed, output buffer, channel) sequence, the word of its frame k, and the dither of that word
__host__ __device__ inline uint32_t sample_dither_key(uint32_t seed, int m, int ch) { return sample_hash(seed + 0x9e3779b9u * (uint32_t)(2 * m + ch + 1)); }
__host__ __device__ inline uint32_t sample_dither_word(uint32_t key, long long k) { return sample_hash(key ^ (uint32_t)k); }
__host__ __device__ inline float sample_dither_value(uint32_t w) { return (((float)(w & 0xffffu) + (float)(w >> 16)) - 65535.0f) * (1.0f / 65536.0f); }

// 16-bit PCM.  decode x = (float)q / 32767.0f, the correctly rounded quotient; encode v = x * 32767.0f; with dither
// v = v + d; r = rintf(v) (nearest, ties to even); q = NaN ? 0 : clamp(r, -32768, 32767).  One fp32 rounding per line.
struct SampleS16
{
    static constexpr int format = UMX_SAMPLE_S16, frame_bytes = 4;
    static constexpr int align = 1; // (a frame is stored as one word; the entry points have never refused an address for it)
    static const char *misaligned() { return ""; }
    __host__ __device__ static float decode(int16_t q)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __fdiv_rn((float)q, 32767.0f);
#else
        return (float)q / 32767.0f;
#endif
    }
    // the encode rule up to and including its rounding: r, before the NaN test and the clamp
    __host__ __device__ static float round(float x, bool dither, uint32_t key, long long k)
    {
        float v = x * 32767.0f;
        if (dither)
            v = v + sample_dither_value(sample_dither_word(key, k));
        return rintf(v);
    }
    // did the clamp change the rounded value r (a NaN r: no)
    __host__ __device__ static bool is_clipped(float r) { return r > 32767.f || r < -32768.f; }
    __host__ __device__ static int16_t clamp(float r)
    {
        if (r != r)
            return 0;
        return (int16_t)(r < -32768.f ? -32768.f : r > 32767.f ? 32767.f : r);
    }
};

// packed 24-bit PCM.  decode x = (float)q * 2^-23, exact; encode v = x * 8388608.0f (exact short of overflow);
// r = rint((double)v + (dither ? (double)d : 0.0)), the sum formed in double and rounded once (an fp32 v + d falls on a 0.5 grid at
// |v| >= 2^22, before the rounding); q = NaN ? 0 : clamp(r, -8388608, 8388607).  +1.0f encodes to 8388607 and counts as clipped.
struct SampleS24
{
    static constexpr int format = UMX_SAMPLE_S24, frame_bytes = 6;
    static constexpr int align = 2; // (its frames are 6 bytes, so an even base is all it takes)
    static const char *misaligned() { return "a packed 24-bit buffer must be 2-byte aligned"; }
    __host__ __device__ static float decode(int32_t q) { return (float)q * (1.0f / 8388608.0f); }
    __host__ __device__ static double round(float x, bool dither, uint32_t key, long long k)
    {
        const float v = x * 8388608.0f;
        double s = (double)v;
        if (dither)
            s = s + (double)sample_dither_value(sample_dither_word(key, k));
        return rint(s);
    }
    __host__ __device__ static bool is_clipped(double r) { return r > 8388607.0 || r < -8388608.0; }
    __host__ __device__ static int32_t clamp(double r)
    {
        if (r != r)
            return 0;
        return (int32_t)(r < -8388608.0 ? -8388608.0 : r > 8388607.0 ? 8388607.0 : r);
    }
};

// f(the trait of `format`); an fp32 format, or an unknown one: f is not called, and the answer is f's type's zero (false, nothing)
template <class F> __host__ __device__ inline auto with_sample_format(int format, F &&f) -> decltype(f(SampleS16()))
{
    switch (format)
    {
    case UMX_SAMPLE_S16:
        return f(SampleS16());
    case UMX_SAMPLE_S24:
        return f(SampleS24());
    default:
        return decltype(f(SampleS16()))();
    }
}

// bytes of a stereo frame of a host or integer-side buffer in a format
inline size_t sample_frame_bytes(int format)
{
    const int fb = with_sample_format(format, [](auto t) { return decltype(t)::frame_bytes; });
    return fb ? (size_t)fb : 8;
}
inline bool sample_format_known(int f) { return f == UMX_SAMPLE_F32 || with_sample_format(f, [](auto) { return true; }); }

// what an entry point refuses (nullptr: fine): io == nullptr is the fp32 call
inline const char *sample_io_refusal(const umx_sample_io *io)
{
    if (!io)
        return nullptr;
    if (!sample_format_known(io->in_format) || !sample_format_known(io->out_format))
        return "sample io: unknown sample format (UMX_SAMPLE_F32, UMX_SAMPLE_S16 or UMX_SAMPLE_S24)";
    if (io->dither && io->out_format == UMX_SAMPLE_F32)
        return "sample io: dither goes with a UMX_SAMPLE_S16 or UMX_SAMPLE_S24 output only";
    return nullptr;
}

// would sample x, as it leaves in clip_format, be changed by that format's clamp (an fp32 output: never)
__host__ __device__ inline bool sample_clips(float x, int clip_format, bool dither, uint32_t key, long long k)
{
    return with_sample_format(clip_format, [=](auto t) { return decltype(t)::is_clipped(decltype(t)::round(x, dither, key, k)); });
}

// src[b] / dst[b] from the first frame on; b = the output's index in the call's `out` list (the m of the dither), nullptr: none.
// dst is addressed in bytes (frame i of a format at dst + frame_bytes * i); a launch that only measures leaves it empty.
struct EncodeArgs
{
    const float2 *src[4];
    uint8_t *dst[4];
    uint32_t key[4][2]; // sample_dither_key of (seed, b, channel)
    long long first_frame;
    int dither;
};

// buffers 0 .. nb-1 of a call's `out` list from frame first_frame of the caller's track on (dst == nullptr: no destinations)
inline EncodeArgs encode_args(int nb, const float2 *const *src, uint8_t *const *dst, long long first_frame, bool dither, uint32_t seed)
{
    EncodeArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
    {
        a.src[b] = src[b];
        a.dst[b] = dst ? dst[b] : nullptr;
        a.key[b][0] = sample_dither_key(seed, b, 0);
        a.key[b][1] = sample_dither_key(seed, b, 1);
    }
    a.first_frame = first_frame;
    a.dither = dither ? 1 : 0;
    return a;
}

// x over a divisor g > 1, correctly rounded (levels.h: the rescale rule; its other divisor, 1, divides nothing: the callers test for it)
__host__ __device__ inline float sample_rescaled(float x, float g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(x, g);
#else
    return x / g;
#endif
}

// what a sample goes through before the encode rule: nothing, or the track's divisor
struct Plain
{
    __device__ float operator()(float x) const { return x; }
};
struct Rescaled
{
    float g;
    bool divide;
    __device__ float operator()(float x) const { return divide ? sample_rescaled(x, g) : x; }
};

// one sample through `pre` and the encode rule of format T; COUNT: clip += 1 where the clamp changed it
template <class T, bool COUNT, class Pre>
__device__ inline auto encode_sample(float x, const Pre &pre, bool dither, uint32_t key, long long k, uint32_t &clip) -> decltype(T::clamp(0))
{
    const auto r = T::round(pre(x), dither, key, k);
    if (COUNT)
        clip += T::is_clipped(r) ? 1u : 0u;
    return T::clamp(r);
}

} // namespace umx
