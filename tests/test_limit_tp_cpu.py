"""umx_hip_limit_tp_host (csrc/limiter.h) against tests/limit_tp_ref.py and the consequences the header states.  No GPU."""
import numpy as np
import pytest

import limit_ref
import limit_tp_ref
import true_peak_ref
from limit_ref import same_bits

CEILING = np.float32(10 ** (-1 / 20))


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("rate", [44100, 96000, 192000])
def test_host_twin_is_the_rule(pkg, rate, nb):
    """fp32 chains cannot be restated bit for bit in numpy: r = c/p 2^21 only matters where p > c, where an error d of p moves r 2^-21
    by at most d/c (a p that straddles c: by no more), the floor adds 2^-21, and minimum and mean do not amplify."""
    W, F = limit_ref.window(rate), true_peak_ref.factor_of(rate)
    for n in sorted({1, 24 // F if F > 1 else 1, W - 1, W + 1, 3 * W + 5}):
        xs = limit_tp_ref.bursts(limit_ref.make("two_w", n, nb, W, seed=n), [n // 3])
        g, ys, rep = pkg.limit_host(xs, rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
        g_ref, rep_ref = limit_tp_ref.limit(xs, rate, CEILING)
        tol = 2.0 ** -21 + true_peak_ref.bound(np.concatenate(xs), rate) / float(CEILING)
        assert np.abs(g.astype(np.float64) - g_ref).max() <= tol, (n, np.abs(g - g_ref).max(), tol)
        assert abs(rep[0] - rep_ref[0]) <= tol and all(same_bits(y, x * g[None, :]) for x, y in zip(xs, ys))
        if F == 1:  # no interpolator: the sample detector's bits
            assert same_bits(g, pkg.limit_host(xs, rate, CEILING)[0]) and rep == pkg.limit_host(xs, rate, CEILING)[2]


def test_fs4_tone_is_held_between_the_samples(pkg):
    """the header's example: every sample 0.707, the waveform between them 1.0"""
    rate, c, W = 44100, np.float32(0.8), 256
    x = true_peak_ref.tone(rate, 45, seconds=0.1, amplitude=1.0).astype(np.float32)
    n, edge = x.shape[1], W + 12
    assert (pkg.limit_host([x], rate, c)[0] == 1).all()  # the sample detector lets it through
    g, (y,), rep = pkg.limit_host([x], rate, c, detector=pkg.LIMIT_TRUE_PEAK)
    assert (g[edge:n - edge] < 0.81).all() and rep[1] == n
    after = pkg.true_peak_float(pkg.true_peak_host(y, rate, edge, n - 2 * edge))
    assert after <= 0.8 * (1 + 1e-5), after


def test_nonfinite_samples_pass_and_only_silence_the_interpolator_near_them(pkg):
    rate, W, n = 44100, 256, 3 * 256 + 5
    xs = limit_tp_ref.bursts(limit_ref.make("nonfinite", n, 4, W, seed=3), [100, n // 2 + 40])
    bad = np.zeros(n, bool)
    for x in xs:
        bad |= ~np.isfinite(x).all(axis=0)
    zeroed = [np.where(np.isfinite(x), x, np.float32(0)) for x in xs]
    g, ys, _ = pkg.limit_host(xs, rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
    gz = pkg.limit_host(zeroed, rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)[0]
    assert all(same_bits(y[~np.isfinite(x)], x[~np.isfinite(x)]) for x, y in zip(xs, ys))
    # the required gains differ only within 24/F frames of those samples (e of the frame in front included): the gains within W - 1 more
    near = (np.abs(np.arange(n)[:, None] - np.flatnonzero(bad)[None, :]) <= 6 + 1 + W - 1).any(axis=1)
    assert bad.sum() == 2 and same_bits(g[~near], gz[~near])
    assert (g <= pkg.limit_host(zeroed, rate, CEILING)[0]).all() and (g >= gz).all()


def test_quiet_track_leaves_bit_for_bit_and_refusals(pkg):
    x = (0.5 * true_peak_ref.tone(44100, 45, seconds=0.02, amplitude=1.0)).astype(np.float32)  # true peak 0.5
    g, (y,), rep = pkg.limit_host([x], 44100, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
    assert rep == (1.0, 0) and same_bits(y, x) and (g == 1).all()
    for rate, c, reason in [(7999, 0.5, "8000 .. 192000"), (192001, 0.5, "8000 .. 192000"), (44100, 1.5, "ceiling"), (0, 0.5, "sample rate")]:
        with pytest.raises(pkg.UmxError) as e:
            pkg.limit_host([x], rate, c, detector=pkg.LIMIT_TRUE_PEAK)
        assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
    assert pkg.limit_host([x], 7999, 0.5)[2] == (1.0, 0)  # the sample detector keeps its range
