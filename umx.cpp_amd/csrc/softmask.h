// softmask.h -- UMX_FLAG_SOFTMASK: Open-Unmix's `Separator(softmask=True)` takes a source's first estimate as
//     y_j = X g_j / (eps + sum_k g_k),   g_j = mask_j |X|
// instead of mask_j |X| X/|X|, so that the first estimates add up to the mixture whatever the masks sum to.  Every consumer here forms
// mask |X| X/|X|; so the mask planes fc3 has just written are rewritten in place, per channel, frame and bin b <= 2048, fp32:
//     a = mix_magnitude(X)    g_j = m_j * a    d = WIENER_EPS + (((g_j1 + g_j2) + g_j3) + g_j4)    m'_j = g_j / d
// over the active targets j1 < j2 < ... (as many terms as there are; `/` is the correctly rounded IEEE quotient: d reaches down to
// 1e-10, g down to the subnormals).  m'_j a X/|X| is then the soft-masked estimate and everything downstream runs unchanged.  A silent
// bin (a = 0) gives 0 / eps = 0; the padding columns >= 2049 are neither read nor written.
//
// A pure streaming kernel in the manner of residual_mask.h: one launch covers the active lanes of a call (grid z = the LaneSet, pointers
// are lane 0's, WienerStrides::mag / ::spec apart per lane), a 256-thread workgroup takes SM_ROWS = 8 consecutive rows of the planes
// [2][T][MAGP] -- row r is also row r of the spectrogram [2][T][2049] --, two rows at a time: float4 columns tid and tid + 256 of every
// active plane (16-byte non-temporal buffer loads and stores) and the eight mixture bins that go with them.  Bin 2048 of the eight rows
// is a one-element tail (4-byte accesses, threads 0, 32, .. 224).  A thread reads and writes only its own elements: in place, no LDS.
// The mixture: a row of spec is 2049 x 8 B, so row r starts 8 (r & 1) bytes behind a 16-byte boundary.  Both alignments are handled
// with naturally aligned loads: an even row's four bins are two 16-byte loads, an odd row's 8 + 16 + 8 bytes.  A workgroup's first row
// is even (SM_ROWS is), so which form a row takes is known at compile time.
#pragma once
#include "residual_mask.h"

namespace umx
{

constexpr int SM_ROWS = 8; // rows of a plane per workgroup
static_assert(SM_ROWS % 2 == 0 && 256 / SM_ROWS == 32, "a workgroup starts on an even row; one tail thread per row, 32 apart");
static_assert((NBINS * 8) % 16 == 8, "the 16-byte alignment of a spectrogram row alternates");

struct SoftmaskPlanes
{
    float *m[4]; // lane 0's mask planes of the active targets, ascending
};

__device__ __forceinline__ void sm_store4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float4 v)
{
    const wi_u4 t = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, voff, soff, 2); // non-temporal: the filter reads the plane long after it has left the L2
}

// one bin: m_k <- (m_k a) / (eps + sum_k m_k a), the sum in ascending order
template <int NA> __device__ __forceinline__ void sm_bin(float2 X, float (&m)[NA])
{
    const float a = mix_magnitude(X);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NA; ++k)
    {
        m[k] = m[k] * a;
        s = k == 0 ? m[0] : s + m[k];
    }
    const float d = WIENER_EPS + s;
#pragma unroll
    for (int k = 0; k < NA; ++k)
        m[k] = m[k] / d;
}

// four consecutive bins of every active plane
template <int NA> __device__ __forceinline__ void sm_bin4(const float2 (&X)[4], float4 (&m)[NA])
{
    float c[4][NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
    {
        c[0][k] = m[k].x;
        c[1][k] = m[k].y;
        c[2][k] = m[k].z;
        c[3][k] = m[k].w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        sm_bin<NA>(X[e], c[e]);
#pragma unroll
    for (int k = 0; k < NA; ++k)
        m[k] = make_float4(c[0][k], c[1][k], c[2][k], c[3][k]);
}

// grid (ceil(2 T / SM_ROWS), 1, lanes), 256 threads
template <int NA>
__global__ __launch_bounds__(256) void softmask_kernel(SoftmaskPlanes pl, const float2 *__restrict__ spec, int T, LaneSet lanes, WienerStrides ls)
{
    static_assert(NA >= 1 && NA <= 4, "one to four active targets");
    const int ln = lanes.id[blockIdx.z];
    const int rows = 2 * T, plane_bytes = rows * MAGP * 4, spec_bytes = rows * NBINS * 8; // (T <= 4095, engine_init.h: at most 71 / 134 MB)
    constexpr int ROWB = MAGP * 4, SROWB = NBINS * 8;
    __amdgpu_buffer_rsrc_t rs[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        rs[k] = __builtin_amdgcn_make_buffer_rsrc(pl.m[k] + (size_t)ln * ls.mag, 0, plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_spec = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(spec + (size_t)ln * ls.spec), 0, spec_bytes, 0x00020000);
    const int tid = threadIdx.x;
    const int r0 = (int)blockIdx.x * SM_ROWS; // even
    // the tail first (its loads travel under the main part): bin 2048 of row r0 + tid / 32, on the threads with tid % 32 == 0
    const int trow = r0 + (tid >> 5);
    const bool tail = (tid & 31) == 0 && trow < rows;
    const int tvoff = (tid >> 5) * ROWB + (NBINS - 1) * 4, tsvoff = (tid >> 5) * SROWB + (NBINS - 1) * 8;
    float tm[NA];
    float2 tX = make_float2(0.f, 0.f);
    if (tail)
    {
        tX = bld2<2>(rs_spec, tsvoff, r0 * SROWB);
#pragma unroll
        for (int k = 0; k < NA; ++k)
            tm[k] = bld1<2>(rs[k], tvoff, r0 * ROWB);
    }
    // the main part, an even and an odd row at a time: 4 NA + 8 sixteen-byte units in flight per thread
#pragma unroll
    for (int h = 0; h < SM_ROWS; h += 2)
    {
        float4 m[2][2][NA];
        float2 X[2][2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
        {
            const int row = r0 + h + i; // uniform; its parity is i's
            if (row < rows)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                {
#pragma unroll
                    for (int k = 0; k < NA; ++k)
                        m[i][q][k] = bld4<2>(rs[k], tid * 16, row * ROWB + q * 4096);
                    const int so = row * SROWB + q * 8192; // bins 4 (tid + 256 q) .. + 3: 32 bytes from here
                    if (i == 0)
                    {
                        const float4 lo = bld4<2>(rs_spec, tid * 32, so), hi = bld4<2>(rs_spec, tid * 32 + 16, so);
                        X[i][q][0] = make_float2(lo.x, lo.y);
                        X[i][q][1] = make_float2(lo.z, lo.w);
                        X[i][q][2] = make_float2(hi.x, hi.y);
                        X[i][q][3] = make_float2(hi.z, hi.w);
                    }
                    else
                    {
                        X[i][q][0] = bld2<2>(rs_spec, tid * 32, so);
                        const float4 mid = bld4<2>(rs_spec, tid * 32 + 8, so);
                        X[i][q][1] = make_float2(mid.x, mid.y);
                        X[i][q][2] = make_float2(mid.z, mid.w);
                        X[i][q][3] = bld2<2>(rs_spec, tid * 32 + 24, so);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
        {
            const int row = r0 + h + i;
            if (row < rows)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                {
                    sm_bin4<NA>(X[i][q], m[i][q]);
#pragma unroll
                    for (int k = 0; k < NA; ++k)
                        sm_store4(rs[k], tid * 16, row * ROWB + q * 4096, m[i][q][k]);
                }
        }
    }
    if (tail)
    {
        sm_bin<NA>(tX, tm);
#pragma unroll
        for (int k = 0; k < NA; ++k)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(tm[k]), rs[k], tvoff, r0 * ROWB, 2);
    }
}

} // namespace umx
