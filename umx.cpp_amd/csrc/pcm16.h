// pcm16.h -- 16-bit PCM at the edges of the whole-track drivers: int16 stereo frames cross PCIe, the conversion to and
// from the fp32 the kernels work in runs where the samples already are.  One statement of each rule (sample_format.h: SampleS16 and
// the dither), for the host entry points (umx_hip_pcm16_decode_host / _encode_host) and for the kernels:
//   decode   x = (float)q / 32767.0f, the correctly rounded quotient -- the float WAV loader's expression (host/wav.cpp), so an
//            int16 upload gives the bits the float loader gives
//   encode   v = x * 32767.0f; with dither v = v + d; r = rintf(v) (nearest, ties to even); q = NaN ? 0 : clamp(r, -32768, 32767).
//            One fp32 rounding per line, no fused multiply-add (the Makefile compiles with -ffp-contract=off).
// This file is the format's MEMORY SHAPE.  An int16 stereo frame is one 32-bit word (left in the low half, as the file holds it): the
// kernels load and store whole frames, one per thread, so a pointer needs the frame's own alignment only (4 B for int16, 8 B for
// fp32) and there is no head or tail.
#pragma once
#include "common.h"
#include "sample_format.h"

namespace umx
{

__host__ __device__ inline float pcm16_decode(int16_t q) { return SampleS16::decode(q); }
__host__ __device__ inline uint32_t pcm16_frame(int16_t l, int16_t r) { return (uint32_t)(uint16_t)l | ((uint32_t)(uint16_t)r << 16); }

// sample i of a host buffer of the format (the host entry points)
inline float load_sample(SampleS16, const void *q, size_t i) { return SampleS16::decode(static_cast<const int16_t *>(q)[i]); }
inline void store_sample(SampleS16, void *q, size_t i, int16_t v) { static_cast<int16_t *>(q)[i] = v; }

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

// n frames of up to four buffers: frame i of buffer b is frame first_frame + i of the caller's track, `pre` is applied to every sample
// first.  COUNT: clip[b] += the samples of buffer b that the clamp changed.
template <bool COUNT, class Pre> __device__ inline void encode_frames(SampleS16, const EncodeArgs &a, int n, const Pre &pre, uint32_t (&clip)[4])
{
    const bool dither = a.dither != 0;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        const long long k = a.first_frame + (long long)i;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a.dst[b])
            {
                const float2 x = a.src[b][i];
                reinterpret_cast<uint32_t *>(a.dst[b])[i] = pcm16_frame(encode_sample<SampleS16, COUNT>(x.x, pre, dither, a.key[b][0], k, clip[b]),
                                                                      encode_sample<SampleS16, COUNT>(x.y, pre, dither, a.key[b][1], k, clip[b]));
            }
    }
}

inline int pcm16_blocks(int n) { return std::max(1, std::min((n + 255) / 256, 2048)); }
inline int encode_blocks(SampleS16, int n) { return pcm16_blocks(n); }

inline void launch_decode_as(SampleS16, const void *in, float2 *out, int n, hipStream_t st)
{
    hipLaunchKernelGGL(pcm16_decode_kernel, dim3(pcm16_blocks(n)), dim3(256), 0, st, static_cast<const uint32_t *>(in), out, n);
}

} // namespace umx
