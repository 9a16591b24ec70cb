"""tests/levels_ref.py -- the output-level and rescale rules of include/umx_hip.h (umx_levels) in numpy, composed with
tests/pcm16_ref.py, for the CPU and the GPU tests.

levels of an output buffer m, over both channels of the frames that leave (before any encode, before any rescale):
  peak        the largest |x| over the samples that are not NaN (+inf counts), 0 when there is none: an unsigned maximum over the bit
              patterns of |x|
  over_unity  samples with |x| > 1 ; nonfinite: NaN or +-inf
  clipped     int16 outputs only: samples whose r = rint(x * 32767 [+ dither]) of the encode rule is > 32767 or < -32768, on x / g
              when a divisor g applies; +-inf counts, NaN does not
rescale       P = max of the peaks, g = fp32(1.01) * P in fp32; P not finite or not g > 1: divisor 1, nothing changes; else x / g,
              correctly rounded in fp32, then the unchanged encode
Arrays are (2, n): channel, frame.
"""
import numpy as np

import pcm16_ref as pcm

F32 = np.float32
U32 = np.uint32
INF_BITS = 0x7F800000


def abs_bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(U32) & U32(0x7FFFFFFF)


def rounded(x, m=0, first_frame=0, dither_seed=None):
    """r of the encode rule (pcm16_ref.encode up to and including its rint)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * F32(32767.0)
        if dither_seed is not None:
            k = first_frame + np.arange(x.shape[1], dtype=np.int64)
            v = v + np.stack([pcm.d(dither_seed, m, ch, k) for ch in range(2)])
        return np.rint(v)


def gain(peaks):
    """the divisor of a track whose outputs peak at `peaks` (float32 values or one value); 1: nothing is divided"""
    bits = int(abs_bits(np.atleast_1d(np.asarray(peaks, F32))).max(initial=0))
    if bits >= INF_BITS:
        return F32(1.0)
    with np.errstate(over="ignore"):
        g = F32(1.01) * np.array([bits], U32).view(F32)[0]
    return F32(g) if g > F32(1.0) else F32(1.0)


def rescaled(x, g):
    """x over the divisor g; g == 1: x itself, bit for bit"""
    x = np.asarray(x, F32)
    if F32(g) == F32(1.0):
        return x
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return (x / F32(g)).astype(F32)


def levels(x, m=0, first_frame=0, s16=False, dither_seed=None, divisor=1.0):
    """the record of one (2, n) buffer as output m: dict of peak_bits, peak, over_unity, clipped, nonfinite"""
    x = np.asarray(x, F32)
    assert x.ndim == 2 and x.shape[0] == 2
    u = abs_bits(x)
    notnan = u[u <= INF_BITS]
    peak_bits = int(notnan.max()) if notnan.size else 0
    clipped = 0
    if s16:
        r = rounded(rescaled(x, divisor), m, first_frame, dither_seed)
        with np.errstate(invalid="ignore"):
            clipped = int(np.count_nonzero((r > F32(32767.0)) | (r < F32(-32768.0))))
    return {"peak_bits": peak_bits, "peak": np.array([peak_bits], U32).view(F32)[0],
            "over_unity": int(np.count_nonzero((u > 0x3F800000) & (u <= INF_BITS))), "clipped": clipped,
            "nonfinite": int(np.count_nonzero(u >= INF_BITS))}


def add(a, b):
    """two records of the same buffer (consecutive spans of it) as one"""
    bits = max(a["peak_bits"], b["peak_bits"])
    return {"peak_bits": bits, "peak": np.array([bits], U32).view(F32)[0], **{k: a[k] + b[k] for k in ("over_unity", "clipped", "nonfinite")}}


def track(outs, s16=False, dither_seed=None, rescale=False):
    """What a whole-track call reports and returns for the fp32 outputs `outs` (a list of (2, n) arrays, buffer m = its index) of the
    clamp fp32 call: (list of per-buffer records, gain, the outputs as they leave).  rescale: every buffer over the common divisor."""
    plain = [levels(x, m) for m, x in enumerate(outs)]
    g = gain([p["peak"] for p in plain]) if rescale else F32(1.0)
    recs = [levels(x, m, 0, s16, dither_seed, g) for m, x in enumerate(outs)]
    left = [rescaled(x, g) for x in outs]
    if s16:
        left = [pcm.encode(x, m, 0, dither_seed) for m, x in enumerate(left)]
    return recs, g, left


def awkward_floats():
    """pcm16_ref's awkward values with the level rules' own: +-1, the neighbours of 1, the encode thresholds +-32767.5 / 32767 and
    -32768.5 / 32767 (real ties, and the floats either side), as a (2, n) array"""
    one = F32(1.0)
    vals = [one, -one, np.nextafter(one, F32(2)), -np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), -np.nextafter(one, F32(0))]
    for t in (32767.5, -32767.5, -32768.5, 32768.5):
        x = pcm.preimage(abs(t)) * F32(np.sign(t))
        vals += [x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))]
    a = np.concatenate([pcm.awkward_floats().T.ravel(), np.array(vals, F32)])
    if a.size % 2:
        a = np.append(a, F32(-0.0))
    return np.ascontiguousarray(a.reshape(-1, 2).T)
