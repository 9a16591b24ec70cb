"""tests/limit_ref.py -- the look-ahead peak limiter's rule (include/umx_hip.h) in numpy, written from the header text:
peaks as unsigned bit patterns, the required gain on a 2^21 grid from a float64 quotient, the sliding minimum and the window sum as
plain maxima / sums over W shifted views, one float32 product."""
import numpy as np

UNITY = 1 << 21
T = 4096  # the gain kernel's tile (csrc/limiter.h), for the sizes of the GPU tests


def window(rate):
    return 256 if rate <= 50000 else 512 if rate <= 100000 else 1024


def limit(xs, rate, ceiling):
    """xs: a list of (2,n) float32 arrays -> (gain (n,) float32, [y], (min_gain, limited_frames))"""
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    n, W, c = xs[0].shape[1], window(rate), np.float32(ceiling)
    bits = np.stack([x.view(np.uint32) & np.uint32(0x7FFFFFFF) for x in xs])      # [b][ch][n]
    p = np.where(bits >= 0x7F800000, np.uint32(0), bits).max(axis=(0, 1)).view(np.float32)
    over = p > c
    r = np.full(n + 2 * (W - 1), UNITY, np.uint32)                                 # frame k at index k + W - 1
    r[W - 1:W - 1 + n][over] = np.maximum(1, np.floor(np.float64(c) / p[over].astype(np.float64) * 2097152.0)).astype(np.uint32)
    m = r[:n + W - 1].copy()                                                       # m[k] at index k + W - 1
    for d in range(1, W):
        m = np.minimum(m, r[d:d + n + W - 1])
    S = np.zeros(n, np.uint64)
    for d in range(W):                                                             # S[n] = m[n - W + 1] + ... + m[n]
        S += m[d:d + n]
    q = (S // W).astype(np.uint32)
    g = q.astype(np.float32) * np.float32(2.0 ** -21)
    return g, [x * g[None, :] for x in xs], (float(g.min()), int((q < UNITY).sum()))


def signals(n, W):
    """name -> frames with a 4.0 spike (the cases of the issue; frames outside the track are dropped)"""
    mid = n // 2
    cases = {"quiet": [], "spike_first": [0], "spike_last": [n - 1], "spike_mid": [mid], "sustained": list(range(mid - W, mid + W)),
             "two_w_minus_1": [mid - W + 1, mid], "two_w": [mid - W, mid], "nonfinite": [mid]}
    return {k: [f for f in v if 0 <= f < n] for k, v in cases.items()}


def make(name, n, nb, W, seed=0, extra=()):
    """nb (2,n) float32 arrays below 0.5 with the signal's spikes (and `extra` frames) at 4.0 in changing buffers and channels;
    "nonfinite": a NaN and a +inf beside the spike"""
    rng = np.random.default_rng(seed)
    xs = [(0.5 * rng.uniform(-1, 1, (2, n))).astype(np.float32) for _ in range(nb)]
    for i, f in enumerate(list(signals(n, W)[name]) + [e for e in extra if 0 <= e < n]):
        xs[i % nb][i & 1, f] = np.float32(-4.0 if i & 2 else 4.0)
    if name == "nonfinite" and n > 2:
        xs[nb - 1][0, max(n // 2 - 1, 0)] = np.nan
        xs[0][1, min(n // 2 + 1, n - 1)] = np.inf
    return xs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
