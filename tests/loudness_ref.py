"""The loudness rule of DESIGN 21 / include/umx_hip.h in numpy and scipy float64, written from the rule's text and from ITU-R BS.1770-4,
not from csrc/loudness.h: the coefficients from the analogue prototypes, the hop energies with one hop of warm-up (scipy's lfilter is
a transposed direct form II in double), the full-history filter the warm-up stands in for, and a gate of its own."""
import numpy as np
from scipy.signal import lfilter

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high-pass (its b is 1 -2 1)
BS1770_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285), "shelf_a": (-1.69065929318241, 0.73248077421585),
              "hp_a": (-1.99004745483398, 0.99007225036621)}


def hop_of(rate):
    return (int(rate) + 5) // 10


def coeffs(rate):
    """-> (pb, pa, rb, ra), each a float64 triple, a[0] = 1"""
    def stage(f0, Q):
        K = np.tan(np.pi * f0 / rate)
        return K, Q, 1.0 + K / Q + K * K

    K, Q, a0 = stage(1681.974450955533, 0.7071752369554196)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    pb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    pa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K, Q, a0 = stage(38.13547087602444, 0.5003270373238773)
    rb = np.array([1.0, -2.0, 1.0])
    ra = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return pb, pa, rb, ra


def _cascade(x, c):
    pb, pa, rb, ra = c
    return lfilter(rb, ra, lfilter(pb, pa, np.asarray(x, np.float64), axis=-1), axis=-1)


def hop_energies(x, rate):
    """The rule: x (2, n) float32 -> E (2, n // hop) float64; hop b from a zero state at frame max(0, b - 1) hop."""
    x = np.asarray(x, np.float32)
    hop, c = hop_of(rate), coeffs(rate)
    hops = x.shape[1] // hop
    E = np.zeros((2, hops))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(hops):
            lo = max(0, b - 1) * hop
            y = _cascade(x[:, lo:(b + 1) * hop], c)[:, b * hop - lo:]
            E[:, b] = np.sum(y * y, axis=1)
    return E


def hop_energies_full_history(x, rate):
    """What the warm-up stands in for: ONE run of the filter over the whole signal, its squares summed per hop."""
    x = np.asarray(x, np.float32)
    hop = hop_of(rate)
    hops = x.shape[1] // hop
    y = _cascade(x[:, :hops * hop], coeffs(rate))
    return np.sum((y * y).reshape(2, hops, hop), axis=2)


def gate(E, hop):
    """Blocks and gates of one output's (2, hops) energies -> (integrated, momentary_max, blocks, gated), written block by block."""
    E = np.asarray(E, np.float64)
    hops = E.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        P = [float(np.sum(E[:, j:j + 4])) / (4.0 * hop) for j in range(max(0, hops - 3))]
        # (np.sum of a slice adds in another order than the rule's loop: within an ulp or two of P, far inside what the tests ask)
        L = [-0.691 + 10.0 * np.log10(p) if p == p else np.nan for p in P]
        mom = -np.inf
        for l in L:
            if l > mom:
                mom = l
        absg = [p for p, l in zip(P, L) if l > -70.0]
        if not absg:
            return -np.inf, mom, len(P), 0
        gamma = -0.691 + 10.0 * np.log10(sum(absg) / len(absg)) - 10.0
        rel = [p for p, l in zip(P, L) if l > -70.0 and l > gamma]
        if not rel:
            return -np.inf, mom, len(P), 0
        return -0.691 + 10.0 * np.log10(sum(rel) / len(rel)), mom, len(P), len(rel)


def stepped_noise(rate, n, seed):
    """noise with a DC offset and a 40 dB level step (the signal the rule's warm-up was checked on), (2, n) float32"""
    rng = np.random.default_rng(seed)
    x = 0.2 * rng.standard_normal((2, n)) + 0.05
    x[:, n // 2:] *= 0.01
    x[1] *= 0.7
    return x.astype(np.float32)


def tolerance(E):
    """1e-9 E + 1e-9 E_prev per entry of E (..., hops): double round-off through the high-pass stage is 1.1e-16 x 6.4e5 = 7e-11 at 192 kHz"""
    E = np.abs(np.asarray(E, np.float64))
    prev = np.concatenate([np.zeros(E.shape[:-1] + (1,)), E[..., :-1]], axis=-1)
    return 1e-9 * E + 1e-9 * prev
