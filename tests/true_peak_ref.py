"""The true-peak rule of DESIGN 26 / include/umx_hip.h in numpy float64, written from the rule's text, not from csrc/true_peak.h: the
taps by the formula, every interpolated value as a direct sum over its window, the maximum with NaN contributing nothing and inf
counting, and the error bound a fp32 evaluation of those sums is held to."""
import numpy as np

TAPS, CENTRE = 49, 24


def factor_of(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def taps(rate):
    """-> (h, F): the 49 taps in float64 (NOT rounded to fp32) and the factor"""
    F = factor_of(rate)
    i = np.arange(TAPS)
    m = (i - CENTRE).astype(np.float64)
    a = np.pi * m / F
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(m == 0, 1.0, np.sin(a) / a)
    return sinc * (0.5 * (1.0 - np.cos(2.0 * np.pi * i / 48.0))), F


def interpolated(x, rate, h=None):
    """x (2, n) -> y (F - 1, 2, n) float64: y[f - 1, ch, k] = sum_t h[f + F t] x[ch, k + 24/F - t], frames outside [0, n) read as 0;
    and the sums of |h| per phase (F - 1,).  h: other taps than the float64 ones (the fp32-rounded ones, say)."""
    hh, F = taps(rate)
    h = hh if h is None else np.asarray(h, np.float64)
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    nt, reach = 48 // F, 24 // F
    pad = np.zeros((2, n + 2 * nt))
    pad[:, nt:nt + n] = x
    y = np.zeros((max(F - 1, 0), 2, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(1, F):
            for t in range(nt):
                lo = nt + reach - t  # frame k + 24/F - t of the padded signal, k = 0
                y[f - 1] += h[f + F * t] * pad[:, lo:lo + n]
    sums = np.array([np.sum(np.abs(h[f:f + F * nt:F][:nt])) for f in range(1, F)])
    return y, sums


def _peak(v):
    """the largest |v| over what is not NaN (inf counts), 0 when there is none"""
    v = np.abs(np.asarray(v, np.float64)).ravel()
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else 0.0


def true_peak(x, rate, first=0, count=None):
    """The rule over frames [first, first + count) of x (2, n) float32 -> float64"""
    x = np.asarray(x, np.float32)
    count = x.shape[1] - first if count is None else count
    y, _ = interpolated(x, rate)
    return max(_peak(x[:, first:first + count]), _peak(y[:, :, first:first + count]))


def sample_peak(x):
    return _peak(np.asarray(x, np.float32))


def bound(x, rate):
    """What a fp32 evaluation of the rule with fp32-rounded taps may deviate by, per interpolated value, over a finite x: the round-off
    of a sum of 48/F fused multiply-adds, (48/F + 1) 2^-24 sum_t |h[f + F t]| max|x| (the largest over the phases), plus the tap
    rounding, 2^-24 (48/F) max|x| (every tap is at most 1 in size).  The largest per-phase sum stands for every value because the
    host function returns only the maximum over the phases: |max a - max b| <= max |a - b|, whichever phases the two maxima fall on."""
    hh, F = taps(rate)
    if F == 1:
        return 0.0
    nt = 48 // F
    mx = float(np.max(np.abs(np.asarray(x, np.float64))))
    sums = max(np.sum(np.abs(hh[f:f + F * nt:F][:nt])) for f in range(1, F))
    return (nt + 1) * 2.0 ** -24 * sums * mx + 2.0 ** -24 * nt * mx


def tone(rate, phase_deg, seconds=0.5, amplitude=0.5):
    """a sine at rate / 4 with a hard onset, both channels, as float64 (2, n)"""
    n = int(round(seconds * rate))
    k = np.arange(n)
    s = amplitude * np.sin(2.0 * np.pi * k / 4.0 + np.deg2rad(phase_deg))
    return np.stack([s, s])


def db(v):
    return 20.0 * np.log10(v) if v > 0 else -np.inf


def stepped(rate, n, seed, dc=0.05):
    """noise plus a DC offset plus a 40 dB step half way, (2, n) float32"""
    r = np.random.default_rng(seed)
    x = r.uniform(-0.5, 0.5, (2, n)) + dc
    x[:, n // 2:] *= 0.01
    return x.astype(np.float32)
