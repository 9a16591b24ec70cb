// quant_planes.h -- host code only (no device code: any C++17 compiler takes it): how a quantised file tensor becomes the operand of
// the kernels that apply its affine map to the accumulated sum -- the centre of a tensor (quant_centre) and the fp16 planes of
// q - c that the plane GEMMs read (quant_planes), with the fp32 <-> fp16 conversions they need.
//
// The affine map w = q s + o of a quantised tensor is applied to the accumulated sum,
//     sum_k a_k (q_k s + o) = s sum_k a_k (q_k - c) + (o + c s) sum_k a_k,
// and the two terms cancel by |o + c s| sum a: the fp32 roundings of the accumulators and of the row sum are multiplied by
// |o + c s| / s codes.  c is therefore the code that stands for a zero weight, round(-o / s), per source tensor -- |o + c s| <= s / 2,
// whatever outlier skews the tensor's range --, clamped so that q - c stays exact in the kernels' integer planes: 0 .. 255 for u8
// (|q - c| <= 255: one bf16 plane of gemm_bf16x3.h's one-plane form, one fp16 plane of gemm_planes.h), 31 .. 65504 for u16
// (|q - c| <= 65504, the largest finite fp16; fp16(q - c) rounds to infinity from |q - c| = 65520 on, c <= 15 or c >= 65520).  A zero or
// non-finite scale (or a non-finite offset) keeps the middle of the code range, 128 / 32896.  o + c s is formed in double and rounded
// once: the fp32 product c s is not exact for c != 2^n, and its rounding would be multiplied by the row sum again.
// (W_hh in the batched recurrences keeps 128 on purpose: DESIGN 5.)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace umx
{

struct QuantCentre
{
    int c;
    float o2;
};
constexpr int QUANT_U8_MID = 128, QUANT_U8_CMIN = 0, QUANT_U8_CMAX = 255;
constexpr int QUANT_U16_MID = 32896, QUANT_U16_CMIN = 31, QUANT_U16_CMAX = 65504;
// elem_size: 1 = u8 codes, 2 = u16 codes
inline QuantCentre quant_centre(float s, float o, int elem_size = 1)
{
    const bool u16 = elem_size == 2;
    int c = u16 ? QUANT_U16_MID : QUANT_U8_MID;
    if (s - s == 0.f && s != 0.f && o - o == 0.f) // finite, non-zero scale; finite offset
    {
        const double z = std::nearbyint(-(double)o / (double)s), lo = u16 ? QUANT_U16_CMIN : QUANT_U8_CMIN, hi = u16 ? QUANT_U16_CMAX : QUANT_U8_CMAX;
        c = (int)(z < lo ? lo : z > hi ? hi : z);
    }
    return {c, (float)((double)o + (double)c * (double)s)};
}

// fp32 -> fp16 bits, round to nearest even, subnormals and overflow handled (weights at load time)
inline unsigned short f16_rne_bits(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    const unsigned sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u)
        return (unsigned short)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));
    if (u >= 0x477ff000u) // rounds to >= 65520: infinity
        return (unsigned short)(sign | 0x7c00u);
    if (u < 0x38800000u) // below 2^-14: subnormal, in units of 2^-24
    {
        if (u < 0x33000000u) // < 2^-25
            return (unsigned short)sign;
        float a;
        memcpy(&a, &u, 4);
        const float scaled = a * 16777216.0f; // exact
        const float r = nearbyintf(scaled);   // default rounding mode: to nearest even
        return (unsigned short)(sign | (unsigned)r);
    }
    const unsigned mant = u & 0x7fffffu, exp = (u >> 23) - 112u; // rebias 127 -> 15
    unsigned h = (exp << 10) | (mant >> 13);
    const unsigned rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u)))
        ++h; // a carry into the exponent is the correct result
    return (unsigned short)(sign | h);
}
inline float f16_bits_to_float(unsigned short h)
{
    const unsigned sign = (unsigned)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float v;
    if (e == 0)
        v = ldexpf((float)m, -24);
    else if (e == 31)
        v = m ? NAN : INFINITY;
    else
        v = ldexpf((float)(m | 0x400u), (int)e - 25);
    return sign ? -v : v;
}

// One element of a matrix of fp16 planes: fp16(v) and, with a second plane (lo != nullptr), fp16 of the remainder.
inline void f16_split(float v, unsigned short *hi, unsigned short *lo)
{
    *hi = f16_rne_bits(v);
    if (lo)
        *lo = f16_rne_bits(v - f16_bits_to_float(*hi));
}

// One source tensor's codes as the plane GEMMs read them: q (rows x cols, row-major, u8 or u16 by elem_size) -> fp16 planes of q - c,
// c = quant_centre(s, o, elem_size).c.  Source row r goes to row dst_row[r] (nullptr: r) of a matrix of rows cols_pad elements
// long that starts at hi; only its first cols columns are written (the caller's zeros stay in the padding: plane value 0).
// u8: one plane, exact.  u16: hi = fp16(q - c) and lo = the remainder, an integer of at most 16 = 2^-11 of the plane above it, so
// that a2 x remainder need not be formed (gemm_planes.h); lo must then be given, and is indexed like hi.  -> (c, o + c s): the
// kernels take (s, o + c s).
inline QuantCentre quant_planes(const void *q, int elem_size, int rows, int cols, const int *dst_row, size_t cols_pad, float s, float o,
                                unsigned short *hi, unsigned short *lo)
{
    const QuantCentre qc = quant_centre(s, o, elem_size);
    const unsigned char *q8 = static_cast<const unsigned char *>(q);
    for (int r = 0; r < rows; ++r)
    {
        const size_t d0 = (size_t)(dst_row ? dst_row[r] : r) * cols_pad, s0 = (size_t)r * cols;
        for (int k = 0; k < cols; ++k)
        {
            uint16_t qv = q8[s0 + k];
            if (elem_size == 2)
                memcpy(&qv, q8 + (s0 + k) * 2, 2);
            f16_split((float)((int)qv - qc.c), hi + d0 + k, elem_size == 2 ? lo + d0 + k : nullptr);
        }
    }
    return qc;
}

} // namespace umx
