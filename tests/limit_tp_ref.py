"""tests/limit_tp_ref.py -- the limiter under its true-peak detector (include/umx_hip.h) in numpy float64, written from
the header text: p[n] = max(s[n], e[n], e[n-1]) from true_peak_ref.interpolated with the fp32-rounded taps, values that are not
finite dropped; everything behind p as tests/limit_ref.py states it."""
import numpy as np

import limit_ref
import true_peak_ref


def peaks(xs, rate):
    """xs: a list of (2,n) float32 arrays -> p (n,) float64"""
    h32 = true_peak_ref.taps(rate)[0].astype(np.float32)
    n = xs[0].shape[1]
    s, e = np.zeros(n), np.zeros(n)
    with np.errstate(invalid="ignore"):
        for x in xs:
            x = np.asarray(x, np.float32).astype(np.float64)
            s = np.maximum(s, np.where(np.isfinite(x), np.abs(x), 0.0).max(axis=0))
            y = true_peak_ref.interpolated(x, rate, h32)[0]
            if y.size:
                e = np.maximum(e, np.where(np.isfinite(y), np.abs(y), 0.0).max(axis=(0, 1)))
    return np.maximum(s, np.maximum(e, np.concatenate([[0.0], e[:-1]])))


def limit(xs, rate, ceiling):
    """-> (gain (n,) float32, (min_gain, limited_frames))"""
    p, W, c = peaks(xs, rate), limit_ref.window(rate), np.float64(np.float32(ceiling))
    n = p.size
    r = np.full(n + 2 * (W - 1), limit_ref.UNITY, np.uint32)  # frame k at index k + W - 1
    r[W - 1:W - 1 + n][p > c] = np.maximum(1, np.floor(c / p[p > c] * 2097152.0)).astype(np.uint32)
    m = r[:n + W - 1].copy()
    for d in range(1, W):
        m = np.minimum(m, r[d:d + n + W - 1])
    S = np.zeros(n, np.uint64)
    for d in range(W):
        S += m[d:d + n]
    q = (S // W).astype(np.uint32)
    return q.astype(np.float32) * np.float32(2.0 ** -21), (float(q.min()) * 2.0 ** -21, int((q < limit_ref.UNITY).sum()))


def bursts(xs, frames, amplitude=1.0):
    """fs/4 bursts at 45 degrees in buffer 0: samples of 0.71 amplitude around frame f, the full amplitude between the frames f and f + 1"""
    n = xs[0].shape[1]
    for f in frames:
        k = np.arange(max(f - 7, 0), min(f + 9, n))
        xs[0][:, k] = (amplitude * np.sin(2.0 * np.pi * (k - f) / 4.0 + np.pi / 4.0)).astype(np.float32)
    return xs
