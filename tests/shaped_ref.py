"""The UMX_DITHER_SHAPED encode rule of include/umx_hip.h restated in numpy float32, written from the header text: vectorised over
the blocks of 4096 frames (and both channels), a loop over the frame n inside the block.  Every line is one fp32 rounding."""
import numpy as np

from pcm16_ref import d as dither  # d(seed, m, ch, k) of the TPDF rule

BLOCK = 4096
C = [np.float32(c) for c in (2.033, -2.165, 1.959, -1.590, 0.6149)]
F = np.float32


def encode(x, buffer=0, first_frame=0, seed=0, divisor=None):
    """(2,n) float32, frame 0 of x being frame first_frame (a multiple of 4096) of the track -> ((2,n) int16, clipped count)"""
    assert first_frame % BLOCK == 0
    x = np.asarray(x, F)
    n = x.shape[1]
    nb = -(-n // BLOCK)
    xp = np.zeros((2, nb * BLOCK), F)
    xp[:, :n] = x if divisor is None else x / F(divisor)
    v = (xp * F(32767.0)).reshape(2, nb, BLOCK)
    k = first_frame + np.arange(nb * BLOCK, dtype=np.int64)
    d = np.stack([dither(seed, buffer, ch, k) for ch in (0, 1)]).reshape(2, nb, BLOCK)
    e = [np.zeros((2, nb), F) for _ in range(5)]
    r = np.empty((2, nb, BLOCK), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(BLOCK):
            s = C[0] * e[0] + C[1] * e[1]
            for j in (2, 3, 4):
                s = s + C[j] * e[j]
            y = v[:, :, i] - s
            r[:, :, i] = np.rint(y + d[:, :, i])
            err = r[:, :, i] - y
            err[~np.isfinite(err)] = 0
            e = [err] + e[:4]
        r = r.reshape(2, -1)[:, :n]
        clipped = int(np.count_nonzero((r > F(32767)) | (r < F(-32768))))
        q = np.where(np.isnan(r), F(0), np.clip(r, F(-32768), F(32767))).astype(np.int16)
    return q, clipped


def ntf_band_mean(lo_hz, hi_hz, rate=44100, points=1 << 16):
    """the mean of |N(f)|^2, N(z) = 1 - sum c_i z^-i, over [lo_hz, hi_hz] in float64"""
    f = np.linspace(lo_hz, hi_hz, points)
    z = np.exp(-2j * np.pi * f / rate)
    n = 1 - sum(float(c) * z ** (i + 1) for i, c in enumerate(C))
    return float(np.mean(np.abs(n) ** 2))
