// wiener_em.h -- the Wiener EM iterations after the first (UMX_FLAG_WIENER_ITERS >= 2; the loop of wiener.cpp:175-404).
//
// Iteration k filters the mixture with v_k and R_k (wiener.cpp:270-400) and iteration k + 1 forms v_{k+1} and R_{k+1} from that
// y_k with the first iteration's arithmetic (F5, the 200-frame batches).  What the filter needs is v_k(f, b), R_k(b) and X(f, b); what
// the next statistics need is sum_f y y^H and sum_f v -- both formed while y is in registers.  So the only state between iterations
// is v [T][2049][4 sources] (16 B per bin-frame, 85 MB per lane at 60 s) and y [4][2][T][2049] (339 MB) never goes to HBM:
//
//   wiener_stats4_kernel -> wiener_finish4_kernel                                 R_1 (v_1 from the masks, not stored)
//   n - 1 times: wiener_em_step_kernel -> wiener_finish4_kernel                   y_k in registers -> v_{k+1} (in place), R_{k+1}
//   wiener_istft_kernel<true, true> or wiener_apply_kernel<true>                  the last filter, reading v_n
//
// y of an intermediate iteration stays scaled down by max_abs (wiener.cpp:115-146 before the loop, :408-422 after it), and every
// iteration filters the scaled-down MIXTURE (wiener.cpp:381-400), not the previous y.
#pragma once
#include "wiener_kernels.h"

namespace umx
{

// One EM step: the grid and thread mapping of wiener_stats4_kernel (one thread = one bin x one 200-frame batch x one lane, all four
// sources; a ring of WIENER_PF frames' loads in flight) -- grid (ceil(B/64), nchunk x lanes), 64 threads.  Per frame, in frame order:
// load X and v_k (FROM_MASKS: v_1 formed from the masks, the step after the first iteration), y = v_k R_k Cxx^-1 x (scaled down),
// v_{k+1} of y (F5) and the running sums of y y^H and v_{k+1}, then v_{k+1} over v_k: a bin-frame is this thread's alone.  The partial
// sums go out in wiener_stats4_kernel's `part` layout, for the unchanged wiener_finish4_kernel.
struct WienerEmFrame
{
    float2 X0, X1;
    float m0[4], m1[4]; // FROM_MASKS: the masks of both channels; else m0 = v_k
};
template <bool FROM_MASKS>
__device__ __forceinline__ void wiener_em_load(WienerEmFrame &w, const float2 *__restrict__ spec, const WienerMags &mags,
                                               const float4 *v, int T, int f, int b)
{
    w.X0 = spec[((size_t)0 * T + f) * NBINS + b];
    w.X1 = spec[((size_t)1 * T + f) * NBINS + b];
    if (FROM_MASKS)
    {
        const size_t j0 = mask_index(0, T, f, b), j1 = mask_index(1, T, f, b);
#pragma unroll
        for (int s = 0; s < 4; ++s)
        {
            w.m0[s] = mags.m[s][j0];
            w.m1[s] = mags.m[s][j1];
        }
    }
    else
    {
        const float4 vf = v[(size_t)f * NBINS + b];
        w.m0[0] = vf.x;
        w.m0[1] = vf.y;
        w.m0[2] = vf.z;
        w.m0[3] = vf.w;
    }
}

template <bool FROM_MASKS>
__global__ __launch_bounds__(64) void wiener_em_step_kernel(const float2 *__restrict__ spec, WienerMags mags, float *v_, int T,
                                                            const unsigned *__restrict__ maxabs_bits, const float *__restrict__ Rc,
                                                            float *__restrict__ part, LaneSet lanes, WienerStrides ls)
{
    const int nchunk_all = (T + WIENER_CHUNK - 1) / WIENER_CHUNK;
    const int b = blockIdx.x * 64 + threadIdx.x, chunk = blockIdx.y % nchunk_all;
    if (b >= NBINS) // (no surplus threads: v is updated in place, a bin-frame must have one reader and writer)
        return;
    {
        const int ln = lanes.id[blockIdx.y / nchunk_all];
        spec += (size_t)ln * ls.spec;
        part += (size_t)ln * ls.part;
        Rc += (size_t)ln * ls.rc;
        v_ += (size_t)ln * ls.v;
        maxabs_bits += ln;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            mags.m[s] += (size_t)ln * ls.mag;
    }
    float4 *const v = reinterpret_cast<float4 *>(v_);
    const float max_abs = wiener_max_abs(maxabs_bits), rmax = 1.0f / max_abs;
    const int f0 = chunk * WIENER_CHUNK, f1 = min(T, f0 + WIENER_CHUNK);
    float4 rc[4]; // R_k of this bin: constant over the frames
#pragma unroll
    for (int s = 0; s < 4; ++s)
        rc[s] = *reinterpret_cast<const float4 *>(Rc + ((size_t)s * NBINS + b) * 4);
    float r00[4], r01x[4], r01y[4], r11[4], wsum[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
        r00[s] = r01x[s] = r01y[s] = r11[s] = wsum[s] = 0.f;
    auto step = [&](const WienerEmFrame &w, int f) {
        float vk[4];
        if (FROM_MASKS)
        {
            const float h0 = mix_magnitude(w.X0), h1 = mix_magnitude(w.X1);
            float t0[4], t1[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
            {
                t0[s] = w.m0[s] * h0; // target magnitude = mask x |X| (inference.cpp:175-183)
                t1[s] = w.m1[s] * h1;
            }
            wiener_bin_psd(w.X0, w.X1, t0, t1, max_abs, rmax, vk);
        }
        else
        {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                vk[s] = w.m0[s];
        }
        WienerBin wb;
        wiener_bin_setup_v(w.X0, w.X1, vk, rc, max_abs, rmax, wb);
        float vn[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
        {
            float2 y[2];
            wiener_bin_apply(wb, s, rc[s], 1.0f, y); // y stays scaled down between iterations
            vn[s] = wiener_psd_cov(y[0], y[1], r00[s], r01x[s], r01y[s], r11[s]);
            wsum[s] += vn[s];
        }
        v[(size_t)f * NBINS + b] = make_float4(vn[0], vn[1], vn[2], vn[3]);
    };
    // the ring of wiener_stats4_kernel: a slot is refilled (frame + PF) as soon as its frame has been stepped.  (The refills past
    // the batch's end re-read its last frame, whose v this thread may just have replaced: they are never used.)
    constexpr int PF = WIENER_PF;
    WienerEmFrame ringf[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k)
        wiener_em_load<FROM_MASKS>(ringf[k], spec, mags, v, T, min(f0 + k, f1 - 1), b);
    for (int f = f0; f < f1; f += PF)
    {
#pragma unroll
        for (int k = 0; k < PF; ++k)
        {
            if (f + k < f1)
                step(ringf[k], f + k);
            wiener_em_load<FROM_MASKS>(ringf[k], spec, mags, v, T, min(f + PF + k, f1 - 1), b);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        float *o = part + ((size_t)(chunk * 4 + s) * 5) * NBINS + b;
        o[0] = r00[s];
        o[NBINS] = r01x[s];
        o[2 * NBINS] = r01y[s];
        o[3 * NBINS] = r11[s];
        o[4 * NBINS] = wsum[s];
    }
}

} // namespace umx
