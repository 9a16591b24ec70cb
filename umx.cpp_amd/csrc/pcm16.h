// pcm16.h -- 16-bit PCM at the edges of the whole-track drivers: int16 stereo frames cross PCIe, the conversion to and
// from the fp32 the kernels work in runs where the samples already are.  One statement of each rule, for the host entry points
// (umx_hip_pcm16_decode_host / _encode_host) and for the two kernels below:
//   decode   x = (float)q / 32767.0f, the correctly rounded quotient -- the float WAV loader's expression (host/wav.cpp), so an
//            int16 upload gives the bits the float loader gives
//   encode   v = x * 32767.0f; with dither v = v + d; r = rintf(v) (nearest, ties to even); q = NaN ? 0 : clamp(r, -32768, 32767).
//            One fp32 rounding per line, no fused multiply-add (the Makefile compiles with -ffp-contract=off).
//   dither   TPDF, counter based: d depends on (seed, output buffer m, channel ch, frame k of the CALLER's track) alone, so regions,
//            lanes and a rerun after a timeout give the same bits.  h = the 32-bit mixer below,
//            a = h(seed + 0x9e3779b9 (2 m + ch + 1)), w = h(a ^ (uint32)k), d = ((w & 0xffff) + (w >> 16) - 65535) / 65536: the sum
//            of two uniform 16-bit integers, in (-1, 1), every step exact in fp32.
// An int16 stereo frame is one 32-bit word (left in the low half, as the file holds it): the kernels load and store whole frames, one
// per thread, so a pointer needs the frame's own alignment only (4 B for int16, 8 B for fp32) and there is no head or tail.
#pragma once
#include "common.h"

namespace umx
{

__host__ __device__ inline float pcm16_decode(int16_t q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)q, 32767.0f);
#else
    return (float)q / 32767.0f;
#endif
}

__host__ __device__ inline uint32_t pcm16_hash(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// the key of one (seed, output buffer, channel) sequence, and the word of its frame k
__host__ __device__ inline uint32_t pcm16_dither_key(uint32_t seed, int m, int ch) { return pcm16_hash(seed + 0x9e3779b9u * (uint32_t)(2 * m + ch + 1)); }
__host__ __device__ inline uint32_t pcm16_dither_word(uint32_t key, long long k) { return pcm16_hash(key ^ (uint32_t)k); }
__host__ __device__ inline float pcm16_dither(uint32_t w) { return (((float)(w & 0xffffu) + (float)(w >> 16)) - 65535.0f) * (1.0f / 65536.0f); }

// the encode rule up to and including its rounding: r, before the NaN test and the clamp (levels.h counts the clamped samples from it)
__host__ __device__ inline float pcm16_round(float x, bool dither, uint32_t key, long long k)
{
    float v = x * 32767.0f;
    if (dither)
        v = v + pcm16_dither(pcm16_dither_word(key, k));
    return rintf(v);
}

__host__ __device__ inline int16_t pcm16_encode(float x, bool dither, uint32_t key, long long k)
{
    const float r = pcm16_round(x, dither, key, k);
    if (r != r)
        return 0;
    return (int16_t)(r < -32768.f ? -32768.f : r > 32767.f ? 32767.f : r);
}

__host__ __device__ inline uint32_t pcm16_frame(int16_t l, int16_t r) { return (uint32_t)(uint16_t)l | ((uint32_t)(uint16_t)r << 16); }

// n frames: in[i] (one word) -> out[i]; a stream, 4 B read and 8 B written per frame
__global__ void pcm16_decode_kernel(const uint32_t *__restrict__ in, float2 *__restrict__ out, int n)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        const uint32_t w = in[i];
        out[i] = make_float2(pcm16_decode((int16_t)(w & 0xffffu)), pcm16_decode((int16_t)(w >> 16)));
    }
}

// src[b] / dst[b] from the first frame on; b = the output's index in the call's `out` list (the m of the dither), nullptr: none
struct Pcm16EncodeArgs
{
    const float2 *src[4];
    uint32_t *dst[4];
    uint32_t key[4][2]; // pcm16_dither_key of (seed, b, channel)
    long long first_frame;
    int dither;
};

// n frames of up to four buffers in one launch: frame i of buffer b is frame first_frame + i of the caller's track
__global__ void pcm16_encode_kernel(Pcm16EncodeArgs a, int n)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        const long long k = a.first_frame + (long long)i;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.dst[b])
            {
                const float2 x = a.src[b][i];
                a.dst[b][i] = pcm16_frame(pcm16_encode(x.x, a.dither != 0, a.key[b][0], k), pcm16_encode(x.y, a.dither != 0, a.key[b][1], k));
            }
    }
}

inline int pcm16_blocks(int n) { return std::max(1, std::min((n + 255) / 256, 2048)); }

inline void launch_pcm16_decode(const uint32_t *in, float2 *out, int n, hipStream_t st)
{
    if (n >= 1)
        hipLaunchKernelGGL(pcm16_decode_kernel, dim3(pcm16_blocks(n)), dim3(256), 0, st, in, out, n);
}

// buffers 0 .. nb-1 of a call's `out` list, n frames from frame first_frame of the caller's track on
inline void launch_pcm16_encode(int nb, const float2 *const *src, uint32_t *const *dst, int n, long long first_frame, bool dither,
                                uint32_t seed, hipStream_t st)
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
    hipLaunchKernelGGL(pcm16_encode_kernel, dim3(pcm16_blocks(n)), dim3(256), 0, st, a, n);
}

// (what an entry point refuses of a umx_sample_io: sample_io_refusal, pcm24.h, which knows every format)

} // namespace umx
