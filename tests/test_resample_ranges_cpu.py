"""The range rule of the device resampler (csrc/resample.h, include/umx_hip.h) as host arithmetic: output j reads the input
frames c - D .. c + D + 1, c = floor(j M / L).  umx_hip_resample_needs / umx_hip_resample_ready against that window, stated here in
Python integers, and against the float64 definition (tests/resample_ref.py).  No GPU."""
import numpy as np
import pytest

import resample_ref as rr

PAIRS = [(48000, 44100), (8000, 44100), (96000, 44100), (22050, 44100), (44056, 44100)]
PAIRS = PAIRS + [(b, a) for a, b in PAIRS]
IDS = [f"{a}-{b}" for a, b in PAIRS]
N_IN = 100_003


def _geom(pkg, rin, rout):
    """(M, L, D, K): D and K from the library's own tap table, M and L from the rates."""
    taps, d0 = pkg.resample_taps(rin, rout)
    M, L, _, D, K = rr.geometry(rin, rout)
    assert (-d0, taps.shape[1]) == (D, K) and taps.shape[0] == L and K == 2 * D + 2
    return M, L, D, K


def _sweep(K, n_in, seed):
    rng = np.random.default_rng(seed)
    return sorted(set(range(0, 3 * K + 1)) | {int(v) for v in rng.integers(0, n_in + 1, 3000)} | {n_in - 1, n_in})


def _last_read(j, M, L, D):
    """the last input frame output j reads"""
    return j * M // L + D + 1


@pytest.mark.parametrize("rin,rout", PAIRS, ids=IDS)
def test_ready_is_the_window_rule_and_tight_and_monotone(pkg, rin, rout):
    M, L, D, K = _geom(pkg, rin, rout)
    n_out = pkg.resampled_length(N_IN, rin, rout)
    prev = 0
    for f in _sweep(K, N_IN, 1):
        r = pkg.resample_ready(f, rin, rout, N_IN, n_out)
        assert 0 <= r <= n_out and r >= prev, (f, r, prev)
        prev = r
        if f >= N_IN:  # beyond n_in the input is zeros, which are known
            assert r == n_out, f
            continue
        # the window of j grows with j: the last ready output decides for all before it
        assert r == 0 or _last_read(r - 1, M, L, D) <= f - 1, (f, r)
        assert r == n_out or _last_read(r, M, L, D) >= f, (f, r)  # tight: output r reaches frame f or beyond
        if f <= D + 1:
            assert r == 0, (f, r)
    # every j below ready(f), not just the last, for a few f
    for f in (D + 2, D + 3, 3 * K, N_IN // 2, N_IN - 1):
        r = pkg.resample_ready(f, rin, rout, N_IN, n_out)
        j = np.arange(r, dtype=np.int64)
        assert (j * M // L + D + 1 <= f - 1).all(), f


@pytest.mark.parametrize("rin,rout", PAIRS, ids=IDS)
def test_needs_is_the_window_rule_and_the_two_compose(pkg, rin, rout):
    M, L, D, K = _geom(pkg, rin, rout)
    n_out = pkg.resampled_length(N_IN, rin, rout)
    assert pkg.resample_needs(0, rin, rout, N_IN) == 0
    assert pkg.resample_needs(n_out, rin, rout, N_IN) <= N_IN
    for w in _sweep(K, n_out, 2):
        need = pkg.resample_needs(w, rin, rout, N_IN)
        assert need == (0 if w == 0 else min(N_IN, _last_read(w - 1, M, L, D) + 1)), w
        assert pkg.resample_ready(need, rin, rout, N_IN, n_out) >= w, w
    for f in _sweep(K, N_IN, 3):
        r = pkg.resample_ready(f, rin, rout, N_IN, n_out)
        assert pkg.resample_needs(r, rin, rout, N_IN) <= f, (f, r)


def test_zero_and_bad_arguments(pkg):
    assert pkg.resample_ready(0, 48000, 44100, 10, 10) == 0
    assert pkg.resample_ready(10, 48000, 44100, 10, 10) == 10  # all of a short track: everything beyond it is zeros
    assert pkg.resample_ready(5, 48000, 44100, 0, 7) == 7
    assert pkg.resample_needs(5, 48000, 44100, 0) == 0
    assert pkg.resample_needs(1, 48000, 44100, 1000) == rr.geometry(48000, 44100)[3] + 2
    for rin, rout in ((7999, 44100), (44100, 192001), (0, 44100), (44100, -1)):
        assert pkg.resample_needs(10, rin, rout, 100) < 0
        assert pkg.resample_ready(10, rin, rout, 100, 100) < 0
    assert pkg.resample_needs(-1, 48000, 44100, 100) < 0 and pkg.resample_needs(1, 48000, 44100, -1) < 0
    assert pkg.resample_ready(-1, 48000, 44100, 100, 100) < 0 and pkg.resample_ready(1, 48000, 44100, -1, 100) < 0
    assert pkg.resample_ready(1, 48000, 44100, 100, -1) < 0
    # far beyond 32 bits: the arithmetic is 64-bit
    big = 1 << 40
    assert pkg.resample_needs(big, 44056, 44100, 1 << 41) == (big - 1) * 11014 // 11025 + rr.geometry(44056, 44100)[3] + 2
    for name in ("umx_hip_resample_needs", "umx_hip_resample_ready", "umx_hip_resample_range_device", "umx_hip_debug_resample_launches"):
        assert name in pkg.HIP_SYMBOLS


@pytest.mark.parametrize("rin,rout", [(48000, 44100), (44100, 8000), (8000, 44100)])
def test_against_the_float64_definition(pkg, rin, rout):
    M, L, D, K = _geom(pkg, rin, rout)
    n_in = 6 * K + 301
    n_out = pkg.resampled_length(n_in, rin, rout)
    x = np.random.default_rng(7).uniform(-1, 1, (2, n_in))
    y = rr.resample(x, rin, rout, n_out)
    for w in (1, 2, n_out // 3, n_out // 2 + 1):
        need = pkg.resample_needs(w, rin, rout, n_in)
        assert 0 < need < n_in, (w, need)
        z = x.copy()
        z[:, need:] += 1000.0  # every frame from needs(w) on
        assert np.array_equal(rr.resample(z, rin, rout, n_out)[:, :w], y[:, :w]), w
        # frame needs(w) - 1 is inside output w - 1's window (its tap may be a zero of the filter: the window is what the kernel reads)
        c = (w - 1) * M // L
        assert c - D <= need - 1 <= c + D + 1 and need - 1 == c + D + 1, (w, need, c)
