// pcm16_shaped.h -- noise-shaped dither for 16-bit outputs: the UMX_DITHER_SHAPED encode of include/umx_hip.h.  The rule
// is sample_format.h's (shaped_round: error feedback through the five-tap filter, history zero at the first frame of every block of
// SHAPED_BLOCK = 4096 frames of the caller's track); this file is how it runs on the device.
// Error feedback is a recurrence, so a frame is not a thread here.  A LANE owns one (block, channel) of one buffer and walks the
// block's frames in order with e1 .. e5 in registers; everything that does not hang on the previous frame's error -- the load, the
// divisor, x * 32767, the dither hash, the products c2 e2 .. c5 e5, the clamp, the store -- is off the dependent chain
// (c1 e1, four adds, y = v - s, y + d, rint, r - y, the finite test: about ten dependent fp32 operations a sample).
// A WORKGROUP is one wave: 32 consecutive blocks x 2 channels of buffer blockIdx.y.  A lane's frames lie 32 KB from its neighbour's,
// so memory is never touched lane by lane: the wave moves a chunk of 64 frames of each of its 32 blocks as 32 coalesced rows of 512
// bytes into a [32][64] float2 tile in LDS, pitched at 65 float2 so that lane (b, ch) walks bank 2 b + ch (+ 2 n): no conflicts.
// The rows of the NEXT chunk are loaded into registers before the current one is walked, so HBM latency hides behind the walk.  The two
// lanes of a block exchange their codes with one DPP quad permute, the even lane puts the 32-bit frame into a second tile (pitch 65
// words: bank b + n), and the tile leaves as coalesced rows of 256 bytes, each frame predicated on [first_frame, first_frame + n):
// the frames from the block's start up to first_frame are computed and not stored, nor counted.
#pragma once
#include "common.h"
#include "levels.h"

namespace umx
{

#define SHAPED_ROWS 32  // blocks of a workgroup: a lane per block and channel
#define SHAPED_CHUNK 64 // frames of every block in LDS at a time: a row of 512 bytes in, of 256 bytes out
#define SHAPED_PITCH 65 // of both tiles, in float2 and in words

// frames [lo, end), counted from frame `base` (a multiple of SHAPED_BLOCK) of the caller's track, of up to four buffers
struct ShapedArgs
{
    const float2 *src[4]; // frame `base` of buffer b
    uint32_t *dst[4];     // frame base + lo of buffer b
    uint32_t key[4][2];   // sample_dither_key of (seed, b, channel)
    long long base;
    int lo, end;
};

__device__ inline Plain shaped_pre(const Plain *, const uint32_t *) { return Plain(); }
__device__ inline Rescaled shaped_pre(const Rescaled *, const uint32_t *words)
{
    const float g = levels_divisor(words);
    return Rescaled{g, g != 1.0f};
}

// COUNT: acc->clipped[b] += the stored samples of buffer b that the clamp changed.  Pre: Plain, or Rescaled over the divisor of `words`.
template <bool COUNT, class Pre>
__global__ __launch_bounds__(64) void pcm16_shaped_encode_kernel(ShapedArgs a, umx_levels_acc *acc, const uint32_t *__restrict__ words)
{
    __shared__ float2 tin[SHAPED_ROWS * SHAPED_PITCH];
    __shared__ uint32_t tout[SHAPED_ROWS * SHAPED_PITCH];
    const int lane = threadIdx.x, blk = lane >> 1, ch = lane & 1, buf = blockIdx.y;
    const Pre pre = shaped_pre(static_cast<const Pre *>(nullptr), words);
    const float2 *__restrict__ src = a.src[buf];
    uint32_t *__restrict__ dst = a.dst[buf];
    const uint32_t key = a.key[buf][ch];
    const int first = (int)blockIdx.x * (SHAPED_ROWS * SHAPED_BLOCK); // the workgroup's first frame (< end: the grid is sized by it)
    // its first block reaches furthest into [0, end): the chunks that hold a frame of it hold every frame of the others
    const int chunks = (min(SHAPED_BLOCK, a.end - first) + SHAPED_CHUNK - 1) / SHAPED_CHUNK;
    float2 row[SHAPED_ROWS]; // lane's frame of every row of a chunk: +0 behind the last frame (never stored)
    auto load = [&](int c) {
#pragma unroll
        for (int r = 0; r < SHAPED_ROWS; ++r)
        {
            const int f = first + r * SHAPED_BLOCK + c * SHAPED_CHUNK + lane;
            row[r] = f < a.end ? src[(size_t)f] : make_float2(0.f, 0.f);
        }
    };
    ShapedHistory h = {};
    uint32_t clip = 0;
    const float *mine = reinterpret_cast<const float *>(tin + blk * SHAPED_PITCH) + ch;
    load(0);
    for (int c = 0; c < chunks; ++c)
    {
#pragma unroll
        for (int r = 0; r < SHAPED_ROWS; ++r)
            tin[r * SHAPED_PITCH + lane] = row[r];
        __syncthreads();
        if (c + 1 < chunks)
            load(c + 1);
        const int f0 = first + blk * SHAPED_BLOCK + c * SHAPED_CHUNK;
#pragma unroll 8
        for (int n = 0; n < SHAPED_CHUNK; ++n)
        {
            const int f = f0 + n;
            const float d = sample_dither_value(sample_dither_word(key, a.base + f));
            const float r = shaped_round(h, pre(mine[2 * n]) * 32767.0f, d);
            if (COUNT)
                clip += SampleS16::is_clipped(r) && f >= a.lo && f < a.end ? 1u : 0u;
            const int q = (int)(uint16_t)SampleS16::clamp(r);
            const int other = __builtin_amdgcn_mov_dpp(q, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]: the block's other channel
            if (ch == 0)
                tout[blk * SHAPED_PITCH + n] = (uint32_t)q | ((uint32_t)other << 16);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SHAPED_ROWS; ++r)
        {
            const int f = first + r * SHAPED_BLOCK + c * SHAPED_CHUNK + lane;
            if (f >= a.lo && f < a.end)
                dst[(size_t)(f - a.lo)] = tout[r * SHAPED_PITCH + lane];
        }
        __syncthreads();
    }
    if (COUNT)
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            clip += (uint32_t)__shfl_xor((int)clip, d, 64);
        if (lane == 0 && clip != 0)
            atomicAdd(&acc->clipped[buf], (unsigned long long)clip);
    }
}

// n frames of buffers 0 .. nb-1 of a call's `out` list from frame first_frame of the caller's track on: src[b] and dst[b] are that
// frame, and the first_frame % SHAPED_BLOCK frames in front of src[b] are read.  acc: what clamps is counted into its `clipped`
// (nullptr: not counted); words (with acc): over the divisor of these peak words (nullptr: no divisor).
inline void launch_shaped_encode(int nb, const float2 *const *src, uint8_t *const *dst, int n, long long first_frame, uint32_t seed,
                                 umx_levels_acc *acc, const uint32_t *words, hipStream_t st)
{
    if (n < 1 || nb < 1)
        return;
    ShapedArgs a = {};
    a.lo = (int)(first_frame % SHAPED_BLOCK);
    a.base = first_frame - a.lo;
    a.end = a.lo + n;
    for (int b = 0; b < nb && b < 4; ++b)
    {
        a.src[b] = src[b] - a.lo;
        a.dst[b] = reinterpret_cast<uint32_t *>(dst[b]);
        a.key[b][0] = sample_dither_key(seed, b, 0);
        a.key[b][1] = sample_dither_key(seed, b, 1);
    }
    const int blocks = (a.end + SHAPED_BLOCK - 1) / SHAPED_BLOCK;
    const dim3 grid((blocks + SHAPED_ROWS - 1) / SHAPED_ROWS, std::min(nb, 4));
    if (!acc)
        hipLaunchKernelGGL((pcm16_shaped_encode_kernel<false, Plain>), grid, dim3(64), 0, st, a, nullptr, nullptr);
    else if (!words)
        hipLaunchKernelGGL((pcm16_shaped_encode_kernel<true, Plain>), grid, dim3(64), 0, st, a, acc, nullptr);
    else
        hipLaunchKernelGGL((pcm16_shaped_encode_kernel<true, Rescaled>), grid, dim3(64), 0, st, a, acc, words);
}

} // namespace umx
