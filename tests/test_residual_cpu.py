"""The residual source (UMX_FLAG_RESIDUAL) without a GPU: the flag arithmetic of the C-ABI, and what the definition promises
on random spectra and masks -- evaluated with the float64 restatement of tests/residual_ref.py on top of tests/wiener_em_ref.py."""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import residual_ref as rr  # noqa: E402
import wiener_em_ref  # noqa: E402

SETS = [s for k in range(5) for s in itertools.combinations(range(4), k)]  # all 16 skip sets


def _flags(pkg, skip, residual):
    f = pkg.FLAG_RESIDUAL if residual else 0
    for t in skip:
        f |= pkg.FLAG_SKIP_TARGET(t)
    return f


def test_residual_slot_over_all_skip_sets(pkg):
    assert pkg.FLAG_RESIDUAL == 0x8000 == rr.FLAG_RESIDUAL
    assert len(SETS) == 16
    for skip in SETS:
        for other in (0, pkg.FLAG_NO_WIENER, pkg.FLAG_WIENER_ITERS(3) | pkg.FLAG_DEBUG_TAPS):
            assert pkg.residual_slot(_flags(pkg, skip, False) | other) == -1, skip
            want = -2 if len(skip) in (0, 4) else min(skip)
            got = pkg.residual_slot(_flags(pkg, skip, True) | other)
            assert got == want == rr.residual_slot(_flags(pkg, skip, True) | other), (skip, got, want)


def test_flags_for_targets(pkg):
    assert pkg.flags_for_targets(["vocals"], residual=True) == 0x700 | 0x8000
    assert pkg.residual_slot(pkg.flags_for_targets(["vocals"], residual=True)) == 0
    assert pkg.flags_for_targets(["drums", "bass"]) == 0xC00
    assert pkg.residual_slot(pkg.flags_for_targets(["bass", "other"], residual=True)) == 1
    assert pkg.flags_for_targets(pkg.TARGET_NAMES) == 0
    for names, residual in ((["voice"], False), ([], False), (list(pkg.TARGET_NAMES), True)):
        with pytest.raises(ValueError):
            pkg.flags_for_targets(names, residual)


def _random_case(seed, T=230, B=24):
    """Spectra of very different levels per bin and masks that sum past 1 in about half the bins (rho < 0 there)."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(-3, 1.5, (1, 1, B))
    X = (rng.standard_normal((2, T, B)) + 1j * rng.standard_normal((2, T, B))) * level
    masks = [rng.uniform(0.0, 0.7, (2, T, B)) * (rng.uniform(size=(2, T, B)) > 0.2) for _ in range(4)]
    return X, masks


def test_rho_rule_in_float32_and_float64():
    X, masks = _random_case(1)
    m32 = [m.astype(np.float32) for m in masks]
    for skip in ((0, 1, 2), (1,), (0, 2), (2, 3)):
        flags = rr.FLAG_RESIDUAL | sum(0x100 << t for t in skip)
        r32 = rr.rho_f32(m32, flags)
        assert r32.dtype == np.float32
        act = rr.active(flags)
        assert act == [t for t in range(4) if t not in skip]
        # the order of the sum: ((j1 + j2) + j3), then 1 - sum, every step rounded to float32
        s = m32[act[0]]
        for j in act[1:]:
            s = np.float32(s + m32[j])
        assert np.array_equal(r32, np.float32(1.0) - s)
        r64 = rr.rho(m32, flags)
        assert np.abs(r32 - r64).max() <= 4 * np.finfo(np.float32).eps * 3  # three roundings of values below 3
        if len(act) >= 2:
            assert (r64 < 0).any() and (r64 > 0).any()


@pytest.mark.parametrize("skip", [(0, 1, 2), (1,), (0, 2), (2, 3)])
def test_mixture_phase_estimates_sum_to_the_mixture(skip):
    """Zero iterations: sum_j m_j |X| e^{i arg X} + rho |X| e^{i arg X} = X, also where the masks sum past 1."""
    X, masks = _random_case(2)
    flags = rr.FLAG_RESIDUAL | sum(0x100 << t for t in skip)
    mags = rr.magnitudes(np.abs(X), masks, flags)
    y = rr.mixture_phase(X, mags)
    for t in skip[1:]:
        assert not y[t].any()
    assert np.abs(sum(y) - X).max() <= 1e-12 * np.abs(X).max()
    # where rho < 0 the residual estimate is in anti-phase with the mixture
    r = rr.residual_slot(flags)
    neg = rr.rho(masks, flags) < 0
    if len(skip) < 3:
        assert neg.any()
    assert ((y[r] * np.conj(X)).real[neg] < 0).all()
    assert np.abs((y[r] * np.conj(X)).imag).max() <= 1e-12 * (np.abs(X) ** 2).max()


@pytest.mark.parametrize("skip", [(0, 1, 2), (1,), (0, 2), (2, 3)])
def test_one_iteration_sums_to_the_mixture_minus_the_regulariser(skip):
    """sum_j G_j = sum_j v_j R_j Cxx^-1 = (Cxx - 4 sqrt(eps) I) Cxx^-1 (F6: sqrt(eps) I once per source, silent slots included), so
    the four estimates sum to X - 4 sqrt(eps) Cxx^-1 X whatever the sign of the residual's magnitude.  Bound: float64 rounding through
    the 2 x 2 inverse, whose condition number is at most about max(v R) / (4 sqrt(eps)) ~ 1e5 here: 1e-16 x 1e5, with two decades of
    margin, relative to the largest |X|."""
    X, masks = _random_case(3)
    flags = rr.FLAG_RESIDUAL | sum(0x100 << t for t in skip)
    mags = rr.magnitudes(np.abs(X), masks, flags)
    y = wiener_em_ref.wiener_em(X, mags, n_iter=1)
    inv = rr.cxx_inverse(X, mags)
    want = X - 4.0 * np.sqrt(wiener_em_ref.WIENER_EPS) * np.einsum("tbkl,ltb->ktb", inv, X)
    assert np.abs(sum(y) - want).max() <= 1e-9 * np.abs(X).max()
    for t in skip[1:]:
        assert not y[t].any()
    assert y[rr.residual_slot(flags)].any()
    # the same through the packaged restatement
    y2 = rr.wiener(X, np.abs(X), masks, flags)
    for t in range(4):
        assert np.array_equal(y[t], y2[t])
