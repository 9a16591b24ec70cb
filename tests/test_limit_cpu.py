"""The look-ahead peak limiter's host call (umx_hip_limit_host, csrc/limiter.h) against the numpy restatement of its rule
(tests/limit_ref.py), bit for bit, and the consequences the header states.  No GPU."""
import numpy as np
import pytest

import limit_ref
from limit_ref import same_bits

CEILING = np.float32(10 ** (-1 / 20))


def sizes(rate):
    W = limit_ref.window(rate)
    return [1, W - 1, W, W + 1, 3 * W + 5]


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("name", list(limit_ref.signals(8, 2)))
@pytest.mark.parametrize("rate", [44100, 96000, 192000])
def test_host_call_is_the_rule(pkg, rate, name, nb):
    W = limit_ref.window(rate)
    assert pkg.limit_window(rate) == W
    for n in sizes(rate):
        xs = limit_ref.make(name, n, nb, W, seed=n)
        g, ys, rep = pkg.limit_host(xs, rate, CEILING)
        g_ref, ys_ref, rep_ref = limit_ref.limit(xs, rate, CEILING)
        assert same_bits(g, g_ref) and all(same_bits(a, b) for a, b in zip(ys, ys_ref)) and rep == rep_ref, (n, rep, rep_ref)
        # what the header promises: the ceiling holds, non-finite samples pass, frames far from every over leave as they came
        over = np.zeros(n, bool)
        for x, y in zip(xs, ys):
            fin = np.isfinite(x)
            assert (np.abs(y[fin]) <= np.nextafter(CEILING, np.float32(np.inf))).all()
            assert same_bits(y[~fin], x[~fin])
            over |= (np.where(fin, np.abs(x), 0) > CEILING).any(axis=0)
        near = (np.abs(np.arange(n)[:, None] - np.flatnonzero(over)[None, :]) <= W - 1).any(axis=1)
        assert (g[~near] == 1).all() and all(same_bits(y[:, ~near], x[:, ~near]) for x, y in zip(xs, ys))
        if name == "quiet":
            assert rep == (1.0, 0) and all(same_bits(x, y) for x, y in zip(xs, ys))
        else:
            assert rep[0] < 1 and rep[1] > 0


def test_window_and_refusals(pkg):
    assert [pkg.limit_window(r) for r in (0, 1, 50000, 50001, 100000, 100001, 655350, 655351)] == [0, 256, 256, 512, 512, 1024, 1024, 0]
    x = np.zeros((2, 8), np.float32)
    for xs, rate, c, reason in [([x], 44100, 0.0, "ceiling"), ([x], 44100, 1.5, "ceiling"), ([x], 44100, float("nan"), "ceiling"),
                                ([x], 0, 0.5, "sample rate"), ([x] * 5, 44100, 0.5, "1 .. 4 buffers"), ([], 44100, 0.5, "1 .. 4 buffers")]:
        with pytest.raises(pkg.UmxError) as e:
            pkg.limit_host(xs, rate, c)
        assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
    assert pkg.limit_host([x], 44100, 1.0)[2] == (1.0, 0)
