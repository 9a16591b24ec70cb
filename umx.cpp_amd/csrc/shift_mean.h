// shift_mean.h -- the shift ensemble: the fp32 mean of K whole-track separations of ONE track that differ in the
// shift offset, each resident in its own track lane's stem accumulators.  Per stem, channel and sample
//     out = (((s_0 + s_1) + s_2) + ... + s_{K-1}) / (float)K
// summed left to right in lane order and divided once (the correctly rounded quotient, no reciprocal): K = 1 returns s_0,
// two equal lanes return that lane, bit for bit.  Nothing here multiplies, so there is nothing to contract.
#pragma once
#include "common.h"
#include "track_kernels.h"

namespace umx
{

// stem t of lane k from its first output frame on (the lane's shift already added to the pointer); passed by value
struct ShiftMeanLanes
{
    const float2 *src[UMX_MAX_SHIFTS][4];
};

// One launch for the four stems (blockIdx.y), frames grid-strided over blockIdx.x.  A stream: 4 K 8 B read and 32 B written per
// frame, each once.  The lanes' shifts differ, so a lane's frames are only 8-byte aligned: float2 loads; the k loop carries no
// store, so its loads are issued ahead of the adds.  The mean goes to a buffer of its own (non-temporal: nobody on the device
// reads it again), never into a lane's accumulator.
__global__ void shift_mean_kernel(ShiftMeanLanes lanes, int K, Stems4 mean, int n)
{
    const int t = blockIdx.y;
    const float fk = (float)K;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        float2 s = lanes.src[0][t][i];
#pragma unroll 8
        for (int k = 1; k < K; ++k)
        {
            const float2 v = lanes.src[k][t][i];
            s.x += v.x;
            s.y += v.y;
        }
        stream_store2(&mean.p[t][i], make_float2(__fdiv_rn(s.x, fk), __fdiv_rn(s.y, fk)));
    }
}

// grid: enough blocks to fill the chip a few times over, the rest of the frames by the grid stride
inline void launch_shift_mean(const ShiftMeanLanes &lanes, int K, Stems4 mean, int n, hipStream_t st)
{
    const int blocks = std::max(1, std::min((n + 255) / 256, 512));
    hipLaunchKernelGGL(shift_mean_kernel, dim3(blocks, 4), dim3(256), 0, st, lanes, K, mean, n);
}

} // namespace umx
