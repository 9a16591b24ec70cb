"""tests/pcm16_ref.py -- the 16-bit PCM rules of include/umx_hip.h (umx_sample_io) in numpy, for the CPU and the GPU tests.

decode   x = fp32(q) / fp32(32767), one correctly rounded fp32 division
encode   v = x * 32767 (one fp32 rounding); with dither v = v + d (one fp32 rounding); r = rint(v) (nearest, ties to even);
         q = 0 for NaN, else int16(clip(r, -32768, 32767))
dither   h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in uint32
         a = h(seed + 0x9e3779b9 (2 m + ch + 1)); w = h(a ^ uint32(k)); d = ((w & 0xffff) + (w >> 16) - 65535) / 65536
m: the output buffer's index in the call's list, ch: the channel, k: the frame in the caller's track at the caller's rate.
Arrays are (2, n): channel, frame.
"""
import numpy as np

F32 = np.float32
U32 = np.uint32
M32 = 0xFFFFFFFF


def h(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x.astype(U32)


def w(seed, m, ch, k):
    """the dither word of frames k (any integers: taken mod 2^32)"""
    a = h((int(seed) + 0x9E3779B9 * (2 * int(m) + int(ch) + 1)) & M32)
    return h(np.uint64(a) ^ (np.asarray(k, np.int64).astype(np.uint64) & M32))


def d(seed, m, ch, k):
    ww = w(seed, m, ch, k)
    s = (ww & 0xFFFF).astype(F32) + (ww >> 16).astype(F32)  # <= 131070: exact
    return (s - F32(65535.0)) * F32(1.0 / 65536.0)


def decode(q):
    return np.asarray(q, np.int16).astype(F32) / F32(32767.0)


def encode(x, m=0, first_frame=0, dither_seed=None):
    """(2, n) float32 -> (2, n) int16 as output buffer m; frame i of x is frame first_frame + i of the track"""
    x = np.asarray(x, F32)
    assert x.ndim == 2 and x.shape[0] == 2
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * F32(32767.0)
        if dither_seed is not None:
            k = first_frame + np.arange(x.shape[1], dtype=np.int64)
            v = v + np.stack([d(dither_seed, m, ch, k) for ch in range(2)])
        r = np.rint(v)
        q = np.where(np.isnan(r), F32(0), np.clip(r, F32(-32768.0), F32(32767.0)))
    return q.astype(np.int16)


def preimage(t):
    """an fp32 x with fp32(x * 32767) == t exactly (a half-way value t = k + 0.5 then IS a tie for the rounding)"""
    x = F32(t / 32767.0)
    for _ in range(8):
        for c in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
            if F32(c * F32(32767.0)) == F32(t):
                return F32(c)
        x = np.nextafter(x, F32(np.inf))
    raise AssertionError(f"no fp32 x with x * 32767 == {t}")


def awkward_floats():
    """values at which the encode rule can go wrong, as a (2, n) array: half-way points (ties to even), full scale and beyond,
    infinities, NaN, the signed zero, subnormals"""
    vals = []
    for half in (0.5, 1.5, 2.5, 3.5, 100.5, 32766.5, 32767.5):
        vals += [preimage(half), -preimage(half)]
    vals += [1.0, -1.0, 2.0, -2.0, 32768.0 / 32767.0, -32768.0 / 32767.0, -32769.0 / 32767.0, np.inf, -np.inf, np.nan, -0.0, 0.0,
             1e-45, -1e-45, 1e-39, -1e-39, np.finfo(F32).tiny, 0.999999, -0.999999, 3.0e38, -3.0e38]
    a = np.array(vals, F32)
    if a.size % 2:
        a = np.append(a, F32(0.25))
    return np.ascontiguousarray(a.reshape(-1, 2).T)
