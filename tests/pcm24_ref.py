"""tests/pcm24_ref.py -- the packed 24-bit PCM rules of include/umx_hip.h (UMX_SAMPLE_S24) in numpy, for the CPU and the GPU
tests.  The dither is pcm16_ref's: the same hash h, word w and value d, keyed by (seed, m, ch) and the frame k of the caller's track.

layout   3 bytes per sample, little-endian, two's complement; a stereo frame is 6 bytes, L then R
decode   x = fp32(q) * 2^-23 (exact)
encode   v = x * 8388608 in fp32 (exact short of overflow); r = rint(float64(v) + float64(d)) -- the sum in double, one rounding, ties to
         even; q = 0 for NaN, else clip(r, -8388608, 8388607)
Arrays are (2, n): channel, frame; codes are int32.
"""
import numpy as np

from pcm16_ref import d, h, w  # noqa: F401  (the dither: reused, and re-exported for the tests)

F32 = np.float32
QMIN, QMAX = -8388608, 8388607
SCALE = F32(8388608.0)


def pack(q):
    """(2, n) int32 codes -> 6 n bytes"""
    a = np.ascontiguousarray(np.asarray(q).T).astype("<i4")
    assert a.ndim == 2 and a.shape[1] == 2 and (a.size == 0 or (a.min() >= QMIN and a.max() <= QMAX))
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, 4)[:, :3]).ravel()  # the low three bytes of every little-endian int32


def unpack(b):
    """6 n bytes -> (2, n) int32 codes"""
    b = np.asarray(b, np.uint8).reshape(-1, 3)
    w = np.zeros((b.shape[0], 4), np.uint8)
    w[:, 1:] = b  # the sample in the high three bytes of a little-endian int32: an arithmetic shift extends its sign
    return np.ascontiguousarray((w.view("<i4").ravel().astype(np.int32) >> 8).reshape(-1, 2).T)


def decode(q):
    return np.asarray(q, np.int32).astype(F32) * F32(2.0 ** -23)


def rounded(x, m=0, first_frame=0, dither_seed=None):
    """r of the encode rule, float64 (2, n): before the NaN test and the clamp"""
    x = np.asarray(x, F32)
    assert x.ndim == 2 and x.shape[0] == 2
    with np.errstate(over="ignore", invalid="ignore"):
        s = (x * SCALE).astype(np.float64)
        if dither_seed is not None:
            k = first_frame + np.arange(x.shape[1], dtype=np.int64)
            s = s + np.stack([d(dither_seed, m, ch, k) for ch in range(2)]).astype(np.float64)
        return np.rint(s)


def encode(x, m=0, first_frame=0, dither_seed=None):
    """(2, n) float32 -> (2, n) int32 codes as output buffer m; frame i of x is frame first_frame + i of the track"""
    r = rounded(x, m, first_frame, dither_seed)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(r), 0.0, np.clip(r, float(QMIN), float(QMAX))).astype(np.int32)


def clipped(x, m=0, first_frame=0, dither_seed=None):
    """how many samples the clamp of the encode rule changes"""
    r = rounded(x, m, first_frame, dither_seed)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((r > QMAX) | (r < QMIN)))


def awkward_floats():
    """values at which the encode rule can go wrong, as a (2, n) array: ties k + 0.5 (exact fp32 preimages: (k + 0.5) / 2^23 has at most
    24 significant bits), full scale and beyond, infinities, NaN, the signed zero, subnormals"""
    vals = []
    for k in (0, 1, 2, 100, 8388606, 8388607):
        x = F32((k + 0.5) / 8388608.0)
        assert float(x) * 8388608.0 == k + 0.5
        vals += [x, -x]
    vals += [1.0, -1.0, 2.0, -2.0, -8388609.0 / 8388608.0, np.inf, -np.inf, np.nan, -0.0, 0.0,
             1e-45, -1e-45, 1e-39, -1e-39, np.finfo(F32).tiny, 0.999999, -0.999999, 3.0e38, -3.0e38]
    a = np.array(vals, F32)
    if a.size % 2:
        a = np.append(a, F32(0.25))
    return np.ascontiguousarray(a.reshape(-1, 2).T)
