// track_kernels.h -- on-device overlap-add of split_inference (umx.cpp:197-273): the whole track stays in HBM,
// each segment's stems are blended into the track accumulators with the triangular transition weight and the
// sum of weights normalises at the end.  Same fp32 operations in the same order as host/split.cpp (which
// follows the reference), so the two drivers agree bit for bit.
#pragma once
#include "common.h"

namespace umx
{

struct Stems4
{
    float2 *p[4]; // (2,n) interleaved = one float2 per sample
};

// umx.cpp:197-206, 246: weight[i] = weight[N-1-i] = i+1 (i < N/2), divided by the maximum, ^1.0
__device__ __forceinline__ float transition_weight(int k, int N)
{
    const float raw = (float)((k < N / 2) ? k + 1 : N - k);
    return raw / (float)(N / 2);
}

// umx.cpp:234-260: out(:, offset+k) += w(k) * chunk_out(:, k); sum_weight(offset+k) += w(k)
__global__ void track_accumulate_kernel(Stems4 track, float *sum_w, Stems4 seg, int offset, int n, int N)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (k >= n)
        return;
    const float w = transition_weight(k, N);
    const float2 s = seg.p[t][k];
    float2 o = track.p[t][(size_t)offset + k];
    o.x += w * s.x;
    o.y += w * s.y;
    track.p[t][(size_t)offset + k] = o;
    if (t == 0)
        sum_w[(size_t)offset + k] += w;
}

// the two halves of that update for a multi-GPU driver: the rank that ran the segment multiplies (w * chunk, one
// rounding), the rank that owns the track adds (a second rounding) -- the same two fp32 operations as above
__global__ void track_weight_kernel(Stems4 seg, int n, int N)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (k >= n)
        return;
    const float w = transition_weight(k, N);
    float2 s = seg.p[t][k];
    s.x = w * s.x;
    s.y = w * s.y;
    seg.p[t][k] = s;
}
__global__ void track_add_weighted_kernel(Stems4 track, float *sum_w, Stems4 wseg, int offset, int n, int N)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (k >= n)
        return;
    const float2 s = wseg.p[t][k];
    float2 o = track.p[t][(size_t)offset + k];
    o.x += s.x;
    o.y += s.y;
    track.p[t][(size_t)offset + k] = o;
    if (t == 0)
        sum_w[(size_t)offset + k] += transition_weight(k, N);
}

// umx.cpp:264-273: out /= sum_weight, for samples [start, start + count)
__global__ void track_normalise_kernel(Stems4 track, const float *sum_w, int start, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (i >= count)
        return;
    const size_t k = (size_t)start + i;
    const float sw = sum_w[k];
    float2 o = track.p[t][k];
    o.x /= sw;
    o.y /= sw;
    track.p[t][k] = o;
}

// Track queue (engine_queue.h): what a job must find clean when it takes a lane, zeroed in ONE launch in stream order --
// the spans of its accumulator set (4 stems and the weight sum over the padded length, the shift padding either side of the track
// in the padded input) and the lane's slice of the streaming LSTM state (umx.cpp:167-171, 186-195).
#define TRACK_BEGIN_SPANS 8
struct TrackBeginSpans
{
    float *p[TRACK_BEGIN_SPANS]; // each at least 4-byte aligned
    unsigned long long n[TRACK_BEGIN_SPANS]; // floats
    int count;
};

// 16-byte stores over the aligned body of every span, scalar stores for the up to 3 floats either side; grid-stride
__global__ void track_begin_kernel(TrackBeginSpans sp)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    for (int k = 0; k < sp.count; ++k)
    {
        float *p = sp.p[k];
        const size_t n = (size_t)sp.n[k];
        size_t head = ((16 - (reinterpret_cast<size_t>(p) & 15)) & 15) / 4;
        if (head > n)
            head = n;
        const size_t nv = (n - head) / 4, tail0 = head + 4 * nv;
        if (tid < head)
            p[tid] = 0.f;
        float4 *q = reinterpret_cast<float4 *>(p + head);
        for (size_t i = tid; i < nv; i += nthreads)
            q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < n - tail0)
            p[tail0 + tid] = 0.f;
    }
}

inline void launch_track_begin(const TrackBeginSpans &sp, hipStream_t st)
{
    unsigned long long total = 0;
    for (int k = 0; k < sp.count; ++k)
        total += sp.n[k];
    const unsigned long long want = (total / 4 + 255) / 256;
    const unsigned blocks = want < 1 ? 1u : want > 2048 ? 2048u : (unsigned)want;
    hipLaunchKernelGGL(track_begin_kernel, dim3(blocks), dim3(256), 0, st, sp);
}

} // namespace umx
