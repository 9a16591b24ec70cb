// residual_mask.h -- the residual source of UMX_FLAG_RESIDUAL: Open-Unmix's `Separator(residual=True)` appends one more
// source to the targets it was asked for, the mixture minus their estimates, and hands it to the EM like any other.  Here the slot of
// a SKIPPED target carries it: instead of the zero plane a skipped target contributes, slot r gets the mask
//     rho[c][f][b] = 1.0f - ((m_j1 + m_j2) + m_j3)        b <= 2048, zero in the padding columns
// over the active targets j1 < j2 < j3 (as many terms as there are), from the masks fc3 has just written.  rho x |X| is then that
// slot's "magnitude" and rho |X| X/|X| = X - sum_j m_j |X| X/|X| its first estimate, formed by the unchanged Wiener kernels.
//
// A pure streaming kernel: reads NA planes [2][T][MAGP], writes one, 16 bytes per access (MAGP % 4 == 0: a row is 544 float4).  One
// launch covers the active lanes of a call (grid z = the LaneSet, pointers are lane 0's, WienerStrides::mag apart per lane).  A
// 256-thread workgroup takes RM_ROWS = 8 consecutive rows: columns 0 .. 511 of a row as two float4 per thread, and the 32 float4 that
// remain of each of the eight rows (columns 512 .. 543: bin 2048, then padding) as one more float4 per thread.  Every access goes
// through a buffer resource: the row in the scalar offset, the thread's part in one register per shape (wiener_istft.h).  No LDS.
#pragma once
#include "wiener_istft.h"

namespace umx
{

constexpr int RM_ROWS = 8;          // rows of a plane per workgroup
constexpr int RM_ROW4 = MAGP / 4;   // float4 per row: 544 = 2 x 256 + 32
static_assert(MAGP % 4 == 0 && RM_ROW4 == 2 * 256 + 256 / RM_ROWS, "a workgroup's column split");
static_assert(NBINS == 2049 && NBINS - 1 == 4 * 512, "bin 2048 is the first float of float4 column 512");

struct ResidualSrc
{
    const float *m[3]; // lane 0's mask planes of the active targets, ascending
};

__device__ __forceinline__ void rm_store4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float4 v)
{
    const wi_u4 t = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, voff, soff, 0);
}

// 1 - ((a + b) + c) per component, fp32, in that order; only the first NA terms exist
template <int NA> __device__ __forceinline__ float4 rm_rho(const float4 (&m)[NA])
{
    float4 s = m[0];
#pragma unroll
    for (int k = 1; k < NA; ++k)
        s = make_float4(s.x + m[k].x, s.y + m[k].y, s.z + m[k].z, s.w + m[k].w);
    return make_float4(1.0f - s.x, 1.0f - s.y, 1.0f - s.z, 1.0f - s.w);
}

// grid (ceil(2 T / RM_ROWS), 1, lanes), 256 threads
template <int NA>
__global__ __launch_bounds__(256) void residual_mask_kernel(ResidualSrc src, float *__restrict__ dst, int T, LaneSet lanes, WienerStrides ls)
{
    static_assert(NA >= 1 && NA <= 3, "one to three active targets");
    const int ln = lanes.id[blockIdx.z];
    const int rows = 2 * T, plane_bytes = rows * MAGP * 4; // (T <= 4095, engine_init.h: at most 71 MB)
    __amdgpu_buffer_rsrc_t rs_src[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        rs_src[k] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(src.m[k] + (size_t)ln * ls.mag), 0, plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc(dst + (size_t)ln * ls.mag, 0, plane_bytes, 0x00020000);
    const int tid = threadIdx.x;
    const int r0 = (int)blockIdx.x * RM_ROWS;
    // the tail first (its loads travel under the main part): row r0 + tid / 32, float4 column 512 + tid % 32.  Only column 512 holds a
    // bin (2048, in .x); the other 31 are padding and are not read.
    const int trow = r0 + (tid >> 5), tcol = 512 + (tid & 31);
    const int tvoff = (tid >> 5) * (MAGP * 4) + tcol * 16;
    float4 tm[NA];
    const bool tail_bin = tcol == 512 && trow < rows;
#pragma unroll
    for (int k = 0; k < NA; ++k)
        tm[k] = tail_bin ? bld4<2>(rs_src[k], tvoff, r0 * (MAGP * 4)) : make_float4(0.f, 0.f, 0.f, 0.f);
    // the main part, four rows at a time: 8 NA float4 in flight per thread
#pragma unroll
    for (int h = 0; h < RM_ROWS; h += 4)
    {
        float4 m[4][2][NA];
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int row = r0 + h + i; // uniform
            if (row < rows)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int k = 0; k < NA; ++k)
                        m[i][q][k] = bld4<2>(rs_src[k], tid * 16, row * (MAGP * 4) + q * 4096);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int row = r0 + h + i;
            if (row < rows)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    rm_store4(rs_dst, tid * 16, row * (MAGP * 4) + q * 4096, rm_rho<NA>(m[i][q]));
        }
    }
    if (trow < rows)
    {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f); // padding columns: zero, as the zero-fill of a skipped target leaves them
        if (tcol == 512)
            o.x = rm_rho<NA>(tm).x;
        rm_store4(rs_dst, tvoff, r0 * (MAGP * 4), o);
    }
}

// the residual slot of a flag word: the lowest skipped target; -1 without UMX_FLAG_RESIDUAL; -2 when the flag is set and no target is
// skipped (five sources) or all four are (nothing to subtract)
inline int residual_slot_of(unsigned flags)
{
    if (!(flags & UMX_FLAG_RESIDUAL))
        return -1;
    const unsigned skip = (flags >> 8) & 0xFu; // UMX_FLAG_SKIP_TARGET(t) = 0x100 << t
    if (skip == 0u || skip == 0xFu)
        return -2;
    int r = 0;
    while (!((skip >> r) & 1u))
        ++r;
    return r;
}

} // namespace umx
