// stem_mix.h -- the stem mix matrix: 1 .. 4 outputs, each a weighted sum of the four stem slots and the input mixture,
// formed where the stems already are (Open-Unmix's `aggregate_dict`, Demucs' --two-stems, "mixture minus vocals", rebalancing).
// gains[m][c]: c = 0 .. 3 the stem slots, c = 4 the mixture.  Per output m, channel and sample, in fp32
//     out_m = ((g_c1 * s_c1 + g_c2 * s_c2) + g_c3 * s_c3) + ...        over the columns c1 < c2 < ... with gains[m][c] != 0.0f
// every product correctly rounded on its own, the terms added left to right with one rounding per addition, the first term the
// product itself (not 0 + product); a row without a nonzero gain gives +0.0f.  No fused multiply-add: the Makefile compiles this
// translation unit with -ffp-contract=off, so `acc + g * s` below stays a multiplication and an addition.  A zero gain (+0 or -0)
// means the column is not a term; a column that no row uses is not loaded at all (its pointer may be null), so an inf or a NaN
// there never reaches an output.
#pragma once
#include "common.h"

namespace umx
{

constexpr int MIX_COLUMNS = 5; // four stem slots + the mixture
constexpr int MIX_MIXTURE = 4;

// a checked matrix: rows beyond n_out are zero; cols = bit c set when any row has a nonzero gain in column c
struct MixSpec
{
    int n_out = 0;
    unsigned cols = 0;
    float g[UMX_MAX_MIX_OUTPUTS][MIX_COLUMNS] = {};
};

// bitmask of the used columns, or -1 (n_out outside 1 .. UMX_MAX_MIX_OUTPUTS, no gains, a gain that is not finite); fills *spec if given
inline int mix_spec_from(int n_out, const float *gains, MixSpec *spec)
{
    if (n_out < 1 || n_out > UMX_MAX_MIX_OUTPUTS || !gains)
        return -1;
    MixSpec s;
    s.n_out = n_out;
    for (int m = 0; m < n_out; ++m)
        for (int c = 0; c < MIX_COLUMNS; ++c)
        {
            const float g = gains[m * MIX_COLUMNS + c];
            if (!std::isfinite(g))
                return -1;
            s.g[m][c] = g;
            if (g != 0.0f)
                s.cols |= 1u << c;
        }
    if (spec)
        *spec = s;
    return (int)s.cols;
}

// pointers from the first frame on (a lane's shift, a region's start already added) and the gains, passed by value.
// src[c] == nullptr: no row uses column c; dst[m] == nullptr: there is no output m (or it already holds its result, see the launcher)
struct StemMixArgs
{
    const float2 *src[MIX_COLUMNS];
    float2 *dst[UMX_MAX_MIX_OUTPUTS];
    float g[UMX_MAX_MIX_OUTPUTS][MIX_COLUMNS];
};

// One frame per thread, frames grid-strided.  A stream: 8 B read per used column and 8 B written per output and frame, each once.
// The pointers carry a lane's shift, so a frame is only 8-byte aligned: float2 loads.  Which columns are loaded and which terms are
// formed depends on the kernel arguments alone (wave-uniform scalar branches).  The operation is pointwise and every used input
// of a frame is in registers before the first output of that frame is stored, so dst[m] may be the buffer src[m] (or any src[c])
// at the same index.
__global__ void stem_mix_kernel(StemMixArgs a, int n)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += step)
    {
        float2 s[MIX_COLUMNS];
#pragma unroll
        for (int c = 0; c < MIX_COLUMNS; ++c)
            s[c] = a.src[c] ? a.src[c][i] : make_float2(0.f, 0.f);
        float2 o[UMX_MAX_MIX_OUTPUTS];
#pragma unroll
        for (int m = 0; m < UMX_MAX_MIX_OUTPUTS; ++m)
        {
            float2 acc = make_float2(0.f, 0.f);
            bool first = true;
#pragma unroll
            for (int c = 0; c < MIX_COLUMNS; ++c)
            {
                const float g = a.g[m][c];
                if (g != 0.0f && a.src[c]) // (the launchers refuse a used column without a pointer)
                {
                    const float px = g * s[c].x, py = g * s[c].y;
                    acc = first ? make_float2(px, py) : make_float2(acc.x + px, acc.y + py);
                    first = false;
                }
            }
            o[m] = acc;
        }
#pragma unroll
        for (int m = 0; m < UMX_MAX_MIX_OUTPUTS; ++m)
            if (a.dst[m])
                stream_store2(&a.dst[m][i], o[m]);
    }
}

// src[c] for the columns of spec.cols (others are ignored), dst[m] for m < spec.n_out, n frames.  An output that is written over
// its own stem (dst[m] == src[m]) with the unit row e_m is 1.0f * s_m = s_m bit for bit: it is left where it is, and a launch
// with nothing else to do (the identity matrix in place) is not made.
inline void launch_stem_mix(const MixSpec &spec, const float2 *const src[MIX_COLUMNS], float2 *const dst[UMX_MAX_MIX_OUTPUTS], int n,
                            hipStream_t st)
{
    StemMixArgs a = {};
    bool any = false;
    for (int m = 0; m < spec.n_out; ++m)
    {
        bool unit = (const float2 *)dst[m] == src[m];
        for (int c = 0; c < MIX_COLUMNS && unit; ++c)
            unit = c == m ? spec.g[m][c] == 1.0f : spec.g[m][c] == 0.0f;
        if (unit)
            continue;
        a.dst[m] = dst[m];
        any = true;
        for (int c = 0; c < MIX_COLUMNS; ++c)
        {
            a.g[m][c] = spec.g[m][c];
            if (spec.g[m][c] != 0.0f)
                a.src[c] = src[c];
        }
    }
    if (!any || n < 1)
        return;
    // grid: enough blocks to fill the chip a few times over, the rest of the frames by the grid stride
    const int blocks = std::max(1, std::min((n + 255) / 256, 2048));
    hipLaunchKernelGGL(stem_mix_kernel, dim3(blocks), dim3(256), 0, st, a, n);
}

} // namespace umx
