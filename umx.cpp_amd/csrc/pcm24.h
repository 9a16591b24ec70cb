// pcm24.h -- packed 24-bit PCM at the edges of the whole-track drivers: 6 B per stereo frame cross PCIe, as a WAV data
// chunk holds them (3 bytes per sample, little-endian, two's complement, L then R).  One statement of each rule (sample_format.h:
// SampleS24 and the dither), for the host entry points (umx_hip_pcm24_decode_host / _encode_host, umx_hip_levels_host) and for the
// kernels below and in levels.h:
//   decode   x = (float)q * 2^-23: exact, and the float WAV loader's q / 8388608.f (host/wav.cpp), so a packed upload gives the
//            bits the float loader gives
//   encode   v = x * 8388608.0f (exact short of overflow); r = rint((double)v + (dither ? (double)d : 0.0)), the sum formed in double
//            and rounded once (an fp32 v + d falls on a 0.5 grid at |v| >= 2^22, before the rounding); q = NaN ? 0 :
//            clamp(r, -8388608, 8388607).  +1.0f encodes to 8388607 and counts as clipped: the loader's scale is 2^23.
//   dither   sample_format.h's d, with its keys (seed, m, ch) and the frame k of the CALLER's track: in (-1, 1) LSB of the 24-bit grid
// This file is the format's MEMORY SHAPE.  A frame is 6 bytes, so a frame per thread would mean byte-wide or misaligned stores.  The smallest unit that is word-aligned on
// both sides is a PAIR of frames: 16 B of fp32, 12 B packed (3 dwords).  The body of every kernel runs on such pairs, one per lane,
// lane-contiguous (a wave moves 1 KiB of fp32 and 768 B packed per instruction); a packed address that is 2 mod 4 -- every region
// that starts at an odd frame of its track -- has one head frame before the first pair, and one tail frame may follow the last.
// Head and tail are read and written 16 bits at a time: a launch touches its own 6 n bytes only, never a neighbouring byte (the
// adjacent region may belong to another launch, or to a download already in flight).  A packed pointer needs 2-byte alignment, an
// fp32 pointer its frame's 8 (the 16-byte fp32 accesses are issued on 8-byte aligned addresses, which global memory takes).
#pragma once
#include "common.h"
#include "sample_format.h"

namespace umx
{

__host__ __device__ inline float pcm24_decode(int32_t q) { return SampleS24::decode(q); }

// one sample <-> its 3 bytes (the host entry points; the kernels move whole pairs of frames and 16-bit pieces)
__host__ __device__ inline int32_t pcm24_load(const uint8_t *p)
{
    return (int32_t)(((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) << 8) >> 8;
}
__host__ __device__ inline void pcm24_store(uint8_t *p, int32_t q)
{
    p[0] = (uint8_t)q;
    p[1] = (uint8_t)((uint32_t)q >> 8);
    p[2] = (uint8_t)((uint32_t)q >> 16);
}
// sample i of a host buffer of the format (the host entry points)
inline float load_sample(SampleS24, const void *q, size_t i) { return SampleS24::decode(pcm24_load(static_cast<const uint8_t *>(q) + 3 * i)); }
inline void store_sample(SampleS24, void *q, size_t i, int32_t v) { pcm24_store(static_cast<uint8_t *>(q) + 3 * i, v); }

// two frames as the three words that hold them, and one frame as its three 16-bit pieces
struct Pcm24Pair
{
    uint32_t w[3];
};
struct __attribute__((aligned(8))) Pcm24Floats // two fp32 frames behind an 8-byte aligned pointer: one 16-byte access
{
    float l0, r0, l1, r1;
};
__device__ inline uint32_t pcm24_sext(uint32_t low24) { return (uint32_t)((int32_t)(low24 << 8) >> 8); }
__device__ inline Pcm24Floats pcm24_unpack_pair(const Pcm24Pair &p)
{
    Pcm24Floats f;
    f.l0 = pcm24_decode((int32_t)pcm24_sext(p.w[0]));
    f.r0 = pcm24_decode((int32_t)pcm24_sext((p.w[0] >> 24) | (p.w[1] << 8)));
    f.l1 = pcm24_decode((int32_t)pcm24_sext((p.w[1] >> 16) | (p.w[2] << 16)));
    f.r1 = pcm24_decode((int32_t)p.w[2] >> 8);
    return f;
}
__device__ inline Pcm24Pair pcm24_pack_pair(int32_t l0, int32_t r0, int32_t l1, int32_t r1)
{
    const uint32_t a = (uint32_t)l0 & 0xffffffu, b = (uint32_t)r0 & 0xffffffu, c = (uint32_t)l1 & 0xffffffu, d = (uint32_t)r1 & 0xffffffu;
    Pcm24Pair p;
    p.w[0] = a | (b << 24);
    p.w[1] = (b >> 8) | (c << 16);
    p.w[2] = (c >> 16) | (d << 8);
    return p;
}
__device__ inline float2 pcm24_load_frame(const uint16_t *p)
{
    const uint32_t h0 = p[0], h1 = p[1], h2 = p[2];
    return make_float2(pcm24_decode((int32_t)pcm24_sext(h0 | (h1 << 16))), pcm24_decode((int32_t)pcm24_sext((h1 >> 8) | (h2 << 8))));
}
__device__ inline void pcm24_store_frame(uint16_t *p, int32_t l, int32_t r)
{
    const uint32_t a = (uint32_t)l & 0xffffffu, b = (uint32_t)r & 0xffffffu;
    p[0] = (uint16_t)a;
    p[1] = (uint16_t)((a >> 16) | (b << 8));
    p[2] = (uint16_t)(b >> 8);
}
// frames before the first pair of a packed buffer of n >= 1 frames at address p
__device__ inline int pcm24_head(const void *p) { return (int)(((uintptr_t)p >> 1) & 1); }

// n frames: 6 n bytes at `in` -> out[0 .. n).  A stream, 6 B read and 8 B written per frame.
__global__ void pcm24_decode_kernel(const uint8_t *__restrict__ in, float2 *__restrict__ out, int n)
{
    const int head = pcm24_head(in), pairs = (n - head) >> 1;
    const Pcm24Pair *__restrict__ pin = reinterpret_cast<const Pcm24Pair *>(in + 6 * head);
    Pcm24Floats *__restrict__ pout = reinterpret_cast<Pcm24Floats *>(out + head);
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t j = first; j < (size_t)pairs; j += step)
        pout[j] = pcm24_unpack_pair(pin[j]);
    // the odd frames, 16 bits at a time: the head (thread 0) and the tail (thread 1)
    if (first == 0 && head)
        out[0] = pcm24_load_frame(reinterpret_cast<const uint16_t *>(in));
    if (first == 1 && ((n - head) & 1))
        out[n - 1] = pcm24_load_frame(reinterpret_cast<const uint16_t *>(in + 6 * (size_t)(n - 1)));
}

// n frames of up to four buffers: frame i of buffer b is frame first_frame + i of the caller's track, `pre` is applied to every sample
// first.  COUNT: clip[b] += the samples of buffer b that the clamp changed.  Every buffer has its own head (its own address).
template <bool COUNT, class Pre> __device__ inline void encode_frames(SampleS24, const EncodeArgs &a, int n, const Pre &pre, uint32_t (&clip)[4])
{
    const bool dither = a.dither != 0;
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto code = [&](float x, int b, int ch, long long k) { return encode_sample<SampleS24, COUNT>(x, pre, dither, a.key[b][ch], k, clip[b]); };
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (a.dst[b])
        {
            const int head = pcm24_head(a.dst[b]), pairs = (n - head) >> 1;
            const Pcm24Floats *__restrict__ pin = reinterpret_cast<const Pcm24Floats *>(a.src[b] + head);
            Pcm24Pair *__restrict__ pout = reinterpret_cast<Pcm24Pair *>(a.dst[b] + 6 * head);
            for (size_t j = first; j < (size_t)pairs; j += step)
            {
                const Pcm24Floats f = pin[j];
                const long long k = a.first_frame + head + 2 * (long long)j;
                pout[j] = pcm24_pack_pair(code(f.l0, b, 0, k), code(f.r0, b, 1, k), code(f.l1, b, 0, k + 1), code(f.r1, b, 1, k + 1));
            }
            // the odd frames, 16 bits at a time: the head (thread 0) and the tail (thread 1)
            const bool tail = ((n - head) & 1) != 0;
            if ((first == 0 && head) || (first == 1 && tail))
            {
                const int i = first == 0 ? 0 : n - 1;
                const float2 x = a.src[b][i];
                const long long k = a.first_frame + i;
                pcm24_store_frame(reinterpret_cast<uint16_t *>(a.dst[b] + 6 * (size_t)i), code(x.x, b, 0, k), code(x.y, b, 1, k));
            }
        }
}

// (a thread per pair of frames; at least two threads: the head's and the tail's)
inline int pcm24_blocks(int n) { return std::max(1, std::min((n / 2 + 255) / 256, 2048)); }
inline int encode_blocks(SampleS24, int n) { return pcm24_blocks(n); }

inline void launch_decode_as(SampleS24, const void *in, float2 *out, int n, hipStream_t st)
{
    hipLaunchKernelGGL(pcm24_decode_kernel, dim3(pcm24_blocks(n)), dim3(256), 0, st, static_cast<const uint8_t *>(in), out, n);
}

} // namespace umx
