// true_peak.h -- the true peak of what leaves the whole-track drivers: the peak of the waveform between the samples as
// well as at them, from a fixed oversampling interpolator, in a form that does not depend on regions, lanes, the queue or reset mode.
// One statement of the rule, for the host entry points (umx_hip_true_peak_taps, umx_hip_true_peak_host) and for the kernel below:
//   factor   F = 4 below 96 kHz, 2 from 96 kHz to below 192 kHz, 1 at 192 kHz (libebur128's factors)
//   taps     49-tap Hann-windowed sinc (libebur128's interpolator restated), formed in double and rounded once to fp32:
//            h[i] = sinc((i - 24) / F) * 0.5 (1 - cos(2 pi i / 48)); h[24] is exactly 1, phase 0 is the sample itself
//   y        frame k, phase f = 1 .. F-1: y = 0; for t = 0 .. 48/F - 1: y = fmaf(h[f + F t], x[k + 24/F - t], y), fp32, frames outside
//            the track read as +0
//   peak     the unsigned maximum of the bit patterns of |x| over the samples and of |y| over the interpolated values, NaN contributing
//            nothing and +inf counting (levels.h's peak rule): true_peak >= peak, equal at F = 1
// A value depends on 48/F fixed frames and on nothing else, and a maximum does not care in which launch a value is met.
#pragma once
#include "common.h"
#include "levels.h"
#include "loudness.h"
#include <cmath>

namespace umx
{

constexpr int TP_TAPS = 49, TP_CENTRE = 24;
inline bool true_peak_rate_ok(int rate) { return kweight_rate_ok(rate); }
inline int true_peak_factor(int rate) { return rate < 96000 ? 4 : rate < 192000 ? 2 : 1; }
// frames behind frame k that its interpolated values read: k is final once frame k + reach is (F = 1: the sample alone)
inline int true_peak_reach(int factor) { return factor > 1 ? TP_CENTRE / factor : 0; }

struct TruePeakTaps
{
    float h[TP_TAPS];
};

inline TruePeakTaps true_peak_taps(int factor)
{
    const double pi = 3.14159265358979323846;
    TruePeakTaps tp;
    for (int i = 0; i < TP_TAPS; ++i)
    {
        const int m = i - TP_CENTRE;
        const double a = pi * m / factor;
        const double sinc = m == 0 ? 1.0 : std::sin(a) / a;
        tp.h[i] = (float)(sinc * (0.5 * (1.0 - std::cos(2.0 * pi * i / (TP_TAPS - 1)))));
    }
    return tp;
}

// the rule on the host: frames [first, first + count) of n interleaved stereo frames -> the maximum with `bits`
template <int F> inline uint32_t true_peak_host_f(const TruePeakTaps &tp, const float *x, long long n, long long first, long long count, uint32_t bits)
{
    constexpr int NT = (TP_TAPS - 1) / F, BACK = F > 1 ? TP_CENTRE / F - 1 : 0;
    for (long long k = first; k < first + count; ++k)
        for (int ch = 0; ch < 2; ++ch)
        {
            const uint32_t p = levels_peak_term(levels_abs_bits(x[2 * k + ch]));
            bits = p > bits ? p : bits;
            if (F == 1)
                continue;
            float y[F] = {}; // (phase 0 unused) tap by tap, every phase's chain in its own order, as the kernel runs them
            for (int t = 0; t < NT; ++t)
            {
                const long long fr = k - BACK + (NT - 1 - t); // frame k + 24/F - t
                const float w = fr >= 0 && fr < n ? x[2 * fr + ch] : 0.0f;
#pragma unroll
                for (int f = 1; f < F; ++f)
                    y[f] = __builtin_fmaf(tp.h[f + F * t], w, y[f]);
            }
            for (int f = 1; f < F; ++f)
            {
                const uint32_t q = levels_peak_term(levels_abs_bits(y[f]));
                bits = q > bits ? q : bits;
            }
        }
    return bits;
}

inline uint32_t true_peak_host(const float *x, long long n, int rate, long long first, long long count, uint32_t bits)
{
    const int F = true_peak_factor(rate);
    const TruePeakTaps tp = true_peak_taps(F);
    return F == 4 ? true_peak_host_f<4>(tp, x, n, first, count, bits)
           : F == 2 ? true_peak_host_f<2>(tp, x, n, first, count, bits)
                    : true_peak_host_f<1>(tp, x, n, first, count, bits);
}

// what a whole-track call reports from a job's record
inline void true_peak_report(const uint32_t bits[4], int n_out, int factor, umx_true_peak &tp)
{
    tp = umx_true_peak{};
    tp.n_out = n_out;
    tp.factor = factor;
    for (int m = 0; m < 4; ++m)
        tp.true_peak[m] = levels_float(bits[m]);
}

inline const char *true_peak_mode_refusal(int mode, int clip_mode)
{
    if (mode != UMX_TRUE_PEAK_OFF && mode != UMX_TRUE_PEAK_MEASURE && mode != UMX_TRUE_PEAK_RESCALE)
        return "true peak mode: unknown (UMX_TRUE_PEAK_OFF, UMX_TRUE_PEAK_MEASURE or UMX_TRUE_PEAK_RESCALE)";
    if (mode == UMX_TRUE_PEAK_RESCALE && clip_mode != UMX_CLIP_RESCALE)
        return "true peak mode: UMX_TRUE_PEAK_RESCALE needs UMX_CLIP_RESCALE";
    return nullptr;
}

// ---------------------------------------------------------------- the kernel
// A workgroup walks tiles of TP_TILE consecutive frames of one buffer (grid.y), counted from the launch's first frame, gridDim.x tiles
// apart.  A tile and its halo -- TP_HALO frames on either side, the F = 2 window's reach rounded up -- are staged in LDS with coalesced
// float2 loads: frame numbers are clamped into [0, n) for the load and the frames outside [0, n) are masked to +0 where they are
// stored, so no load sits under a branch (loudness.h found that form three times faster).  The loads of the NEXT tile are issued into
// registers before this tile's arithmetic and stored behind it.  Thread t takes frames t, t + 256, ... of the tile: the lanes of a
// wave read consecutive 8-byte frames, which the 64-bank LDS serves without a conflict at a pitch of one frame (no padding), and each
// frame read feeds the F - 1 phases of both channels.  The taps are kernel arguments: every index is a constant after unrolling.
// A launch has at most TP_MAX_BLOCKS workgroups, each ending in ONE atomic.  The first form -- a workgroup per tile, 103 000 of them
// for a 600 s track's four outputs, each with its own atomic on one of four words and no load in flight under its arithmetic -- took
// 1.20 ms whatever F, F = 1 included; this one takes 0.38 ms at F = 4 and 0.16 ms at F = 1.
#define TP_TILE 1024
#define TP_HALO 12
#define TP_STAGE (TP_TILE + 2 * TP_HALO)
#define TP_LOADS ((TP_STAGE + LEVELS_THREADS - 1) / LEVELS_THREADS)
#define TP_MAX_BLOCKS 2048

struct TruePeakArgs
{
    const float2 *src[4]; // frame 0 of the caller's track first; grid.y picks one
    TruePeakTaps taps;
    unsigned *bits;       // [4]
    int n, first, count;  // frames of a buffer; the launch measures [first, first + count), inside [0, n)
};

template <int F> __global__ __launch_bounds__(LEVELS_THREADS) void true_peak_kernel(TruePeakArgs a)
{
    constexpr int NT = (TP_TAPS - 1) / F, BACK = F > 1 ? TP_CENTRE / F - 1 : 0;
    static_assert(F == 1 || (BACK <= TP_HALO && NT - 1 - BACK <= TP_HALO), "the halo covers the window");
    __shared__ float2 stage[TP_STAGE];
    __shared__ uint32_t red[LEVELS_WAVES];
    const int m = blockIdx.y, t = threadIdx.x;
    const float2 *__restrict__ src = a.src[m];
    const int ntiles = (a.count + TP_TILE - 1) / TP_TILE, last = a.n - 1;
    float2 pre[TP_LOADS];
    auto load_tile = [&](int t0) { // (a slot beyond the stage reads a frame of the buffer too, and is dropped)
#pragma unroll
        for (int j = 0; j < TP_LOADS; ++j)
            pre[j] = src[min(max(t0 - TP_HALO + t + j * LEVELS_THREADS, 0), last)]; // (t0 <= 2^30 - 1: no overflow)
    };
    auto store_tile = [&](int t0) {
#pragma unroll
        for (int j = 0; j < TP_LOADS; ++j)
        {
            const int i = t + j * LEVELS_THREADS, f = t0 - TP_HALO + i;
            const uint32_t keep = f < 0 || f > last ? 0u : ~0u;
            if (i < TP_STAGE)
                stage[i] = make_float2(__uint_as_float(__float_as_uint(pre[j].x) & keep), __uint_as_float(__float_as_uint(pre[j].y) & keep));
        }
    };
    uint32_t v[1] = {0u};
    load_tile(a.first + blockIdx.x * TP_TILE); // (blockIdx.x < ntiles by the grid)
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int t0 = a.first + tile * TP_TILE;                 // the tile's first frame
        const int frames = min(TP_TILE, a.first + a.count - t0); // frames of the tile that are measured
        __syncthreads(); // the previous tile has been consumed
        store_tile(t0);
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) // the next tile's loads run under this tile's arithmetic
            load_tile(t0 + (int)gridDim.x * TP_TILE);
        for (int i = t; i < frames; i += LEVELS_THREADS)
        {
            const float2 x = stage[TP_HALO + i];
            const uint32_t pl = levels_peak_term(levels_abs_bits(x.x)), pr = levels_peak_term(levels_abs_bits(x.y));
            v[0] = max(v[0], max(pl, pr));
            if constexpr (F > 1)
            {
                float yl[F], yr[F]; // (phase 0 unused)
#pragma unroll
                for (int f = 1; f < F; ++f)
                    yl[f] = yr[f] = 0.0f;
#pragma unroll
                for (int s = 0; s < NT; ++s) // tap s of every phase reads frame k + 24/F - s
                {
                    const float2 w = stage[TP_HALO + i - BACK + (NT - 1 - s)];
#pragma unroll
                    for (int f = 1; f < F; ++f)
                    {
                        yl[f] = __builtin_fmaf(a.taps.h[f + F * s], w.x, yl[f]);
                        yr[f] = __builtin_fmaf(a.taps.h[f + F * s], w.y, yr[f]);
                    }
                }
#pragma unroll
                for (int f = 1; f < F; ++f)
                    v[0] = max(v[0], max(levels_peak_term(levels_abs_bits(yl[f])), levels_peak_term(levels_abs_bits(yr[f]))));
            }
        }
    }
    const uint32_t total = levels_block_reduce<1, 1>(v, red);
    if (t == 0 && total != 0)
        atomicMax(&a.bits[m], total);
}

// Frames [first, first + count) of buffers 0 .. nb-1 (frame 0 of the caller's track at src[b], n frames there and final as far as
// the launch reads them: up to first + count - 1 + reach, or n - 1) into bits[0 .. nb).  The caller has checked the range and the rate.
inline void launch_true_peak(int nb, const float2 *const *src, int n, int rate, long long first, long long count, unsigned *bits, hipStream_t st)
{
    if (nb < 1 || count < 1)
        return;
    const int F = true_peak_factor(rate);
    TruePeakArgs a = {};
    for (int b = 0; b < nb && b < 4; ++b)
        a.src[b] = src[b];
    a.taps = true_peak_taps(F);
    a.bits = bits;
    a.n = n;
    a.first = (int)first;
    a.count = (int)count;
    const int buffers = std::min(nb, 4);
    const dim3 grid((unsigned)std::min<long long>((count + TP_TILE - 1) / TP_TILE, TP_MAX_BLOCKS / buffers), buffers);
    if (F == 4)
        hipLaunchKernelGGL(true_peak_kernel<4>, grid, dim3(LEVELS_THREADS), 0, st, a);
    else if (F == 2)
        hipLaunchKernelGGL(true_peak_kernel<2>, grid, dim3(LEVELS_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(true_peak_kernel<1>, grid, dim3(LEVELS_THREADS), 0, st, a);
}

} // namespace umx
