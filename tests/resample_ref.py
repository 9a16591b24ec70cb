"""Float64 restatement of the device resampler's definition (include/umx_hip.h): torchaudio's default
`sinc_interp_hann` resampler (6 zero crossings, rolloff 0.99), written from the formula alone.

For rates r_in -> r_out with g = gcd, M = r_in / g, L = r_out / g, b = 0.99 min(M, L), W = 6:
    y[j] = sum_i x[i] (b / M) k(b (i / M - j / L)),   k(t) = sinc(t) cos^2(pi t / 2W) for |t| < W, else 0
x is zero outside [0, n_in); every channel is resampled on its own."""
import math

import numpy as np

W = 6.0


def geometry(rate_in, rate_out):
    """(M, L, b, D, K): polyphase form, output j reads input c + d, c = floor(j M / L), d in [-D, D + 1]."""
    g = math.gcd(rate_in, rate_out)
    M, L = rate_in // g, rate_out // g
    b = 0.99 * min(M, L)
    D = math.ceil(W * M / b)
    return M, L, b, D, 2 * D + 2


def kernel(t):
    t = np.asarray(t, np.float64)
    return np.where(np.abs(t) < W, np.sinc(t) * np.cos(np.pi * t / (2 * W)) ** 2, 0.0)


def taps(rate_in, rate_out):
    """float64 table [L][K]: taps[phi][d + D] = (b / M) k(b (d L - phi) / (M L))."""
    M, L, b, D, K = geometry(rate_in, rate_out)
    phi = np.arange(L, dtype=np.float64)[:, None]
    d = np.arange(-D, D + 2, dtype=np.float64)[None, :]
    return b / M * kernel(b * (d * L - phi) / (M * L))


def natural_length(n, rate_in, rate_out):
    M, L, _, _, _ = geometry(rate_in, rate_out)
    return -(-n * L // M)


def resample(x, rate_in, rate_out, n_out=None):
    """x (2, n_in) -> (2, n_out) float64 (n_out None: the natural length ceil(n_in L / M))."""
    x = np.asarray(x, np.float64)
    n_in = x.shape[1]
    M, L, b, D, K = geometry(rate_in, rate_out)
    if n_out is None:
        n_out = natural_length(n_in, rate_in, rate_out)
    tp = taps(rate_in, rate_out)
    j = np.arange(n_out, dtype=np.int64)
    c, phi = (j * M) // L, (j * M) % L
    y = np.zeros((x.shape[0], n_out))
    for k, d in enumerate(range(-D, D + 2)):
        idx = c + d
        ok = (idx >= 0) & (idx < n_in)
        w = np.where(ok, tp[phi, k], 0.0)
        y += x[:, np.clip(idx, 0, n_in - 1)] * w
    return y
