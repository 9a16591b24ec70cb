"""The soft mask (UMX_FLAG_SOFTMASK) without a GPU: the flag constant of the Python layer, and what the definition promises
on random spectra and masks -- evaluated with the restatement of tests/softmask_ref.py on top of tests/residual_ref.py and
tests/wiener_em_ref.py."""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import residual_ref as rr  # noqa: E402
import softmask_ref as sr  # noqa: E402

SETS = [s for k in range(5) for s in itertools.combinations(range(4), k)]  # all 16 skip sets


def _skip_flags(skip, residual=False):
    return sr.FLAG_SOFTMASK | (rr.FLAG_RESIDUAL if residual else 0) | sum(0x100 << t for t in skip)


def _random_case(seed, T=230, B=24):
    """As tests/test_residual_cpu.py: spectra of very different levels per bin, masks that sum past 1 in about half the bins -- plus
    silent bins (X = 0 in one or both channels) and bins where every mask is 0."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(-3, 1.5, (1, 1, B))
    X = (rng.standard_normal((2, T, B)) + 1j * rng.standard_normal((2, T, B))) * level
    masks = [rng.uniform(0.0, 0.7, (2, T, B)) * (rng.uniform(size=(2, T, B)) > 0.2) for _ in range(4)]
    X[:, 7, :] = 0
    X[0, 11, 3:9] = 0
    X[:, :, B - 1] = 0
    for m in masks:
        m[:, 19, :] = 0
        m[1, 23, 5:12] = 0
    return X, masks


def test_the_flag_constant_and_flags_for_targets(pkg):
    assert pkg.FLAG_SOFTMASK == 0x2 == sr.FLAG_SOFTMASK
    others = {n: getattr(pkg, n) for n in dir(pkg) if n.startswith("FLAG_") and n != "FLAG_SOFTMASK" and isinstance(getattr(pkg, n), int)}
    assert {"FLAG_NO_WIENER", "FLAG_RESIDUAL", "FLAG_DEBUG_TAPS", "FLAG_RESET_SEGMENTS", "FLAG_WIENER_ITERS_MASK"} <= set(others)
    for name, v in others.items():
        assert not v & pkg.FLAG_SOFTMASK, name
    for t in range(4):
        assert not pkg.FLAG_SKIP_TARGET(t) & pkg.FLAG_SOFTMASK
    for n in range(1, 16):
        assert not pkg.FLAG_WIENER_ITERS(n) & pkg.FLAG_SOFTMASK
    # flags_for_targets carries it and leaves today's callers alone
    assert pkg.flags_for_targets(["vocals"], residual=True, softmask=True) == 0x700 | 0x8000 | 0x2
    assert pkg.flags_for_targets(pkg.TARGET_NAMES, softmask=True) == 0x2
    assert pkg.flags_for_targets(["drums", "bass"], False, True) == 0xC00 | 0x2
    assert pkg.flags_for_targets(["vocals"], residual=True) == 0x700 | 0x8000
    assert pkg.flags_for_targets(["drums", "bass"]) == 0xC00
    assert pkg.residual_slot(pkg.flags_for_targets(["bass", "other"], residual=True, softmask=True)) == 1
    with pytest.raises(ValueError):
        pkg.flags_for_targets(list(pkg.TARGET_NAMES), residual=True, softmask=True)


@pytest.mark.parametrize("seed", [11, 12])
def test_the_mask_form_is_open_unmix_s_direct_form(seed):
    """m'_j a X/a against X g_j / (eps + sum g) in float64, per element to 1e-12 relative; exact zeros where X = 0 or the mask is 0."""
    X, masks = _random_case(seed)
    a = np.abs(X)
    assert (a == 0).any() and (sum(masks) == 0).any()
    phasor = np.divide(X, a, out=np.ones_like(X), where=a > 0)  # arg(0) = 0, as unit_phasor (csrc/common.h)
    for skip in ((), (1,), (0, 1, 2), (2, 3)):
        flags = _skip_flags(skip)
        m = sr.masks(a, masks, flags)
        want = sr.direct(X, a, masks, flags)
        for j in rr.active(flags):
            got = m[j] * a * phasor
            assert np.isfinite(got).all() and np.isfinite(want[j]).all()
            assert (np.abs(got - want[j]) <= 1e-12 * np.abs(want[j])).all(), (skip, j)
            assert not got[a == 0].any() and not m[j][a == 0].any(), "a silent bin gives m' = 0"
            assert not got[masks[j] == 0].any()
        for t in skip:
            assert m[t] is masks[t], "a skipped target's plane stays what it is"


def test_the_float32_rule_is_within_its_bound_of_float64():
    """The numpy float32 restatement against the float64 rule from the same float32 inputs: the bound the GPU test holds the kernel to."""
    X, masks = _random_case(13)
    a32 = np.abs(X).astype(np.float32)
    m32 = [m.astype(np.float32) for m in masks]
    for skip in ((), (1,), (0, 1, 2), (2, 3)):
        flags = _skip_flags(skip)
        got = sr.masks(a32, m32, flags, "float32")
        assert all(got[j].dtype == np.float32 for j in rr.active(flags))
        worst = sr.rule_errors(got, a32, m32, flags)
        assert max(worst.values()) <= 1.0, (skip, worst)


@pytest.mark.parametrize("skip", SETS, ids=lambda s: "skip" + ("".join(map(str, s)) or "none"))
def test_first_estimates_sum_to_the_mixture(skip):
    """Zero iterations.  The active targets' estimates sum to X s / (eps + s), s = sum of the active g; with the residual the slots sum
    to X, the residual's share being X eps / (eps + s) -- nearly nothing."""
    X, masks = _random_case(14)
    a = np.abs(X)
    scale = np.abs(X).max()
    act = [t for t in range(4) if t not in skip]
    s = sum((masks[j] * a for j in act), np.zeros_like(a))
    for residual in (False, True):
        if residual and len(skip) in (0, 4):
            continue
        flags = _skip_flags(skip, residual)
        y = rr.mixture_phase(X, sr.magnitudes(a, masks, flags))
        r = rr.residual_slot(flags)
        for t in skip:
            if t != r:
                assert not y[t].any()
        if act:
            assert np.abs(sum(y[j] for j in act) - X * s / (sr.EPS + s)).max() <= 1e-12 * scale
        else:
            assert not any(v.any() for v in y)
        if residual:
            assert np.abs(sum(y) - X).max() <= 1e-12 * scale
            assert np.abs(y[r] - X * sr.EPS / (sr.EPS + s)).max() <= 1e-12 * scale
            loud = s > 1e-3
            assert loud.any() and np.abs(y[r][loud]).max() <= 1e-6 * scale, "the residual's first estimate is nearly empty"


def test_wiener_applies_softmask_then_residual_then_the_em():
    X, masks = _random_case(15, T=40)
    a = np.abs(X)
    flags = _skip_flags((1,), residual=True)
    m = sr.masks(a, masks, flags)
    want = rr.wiener(X, a, m, flags, n_iter=2)
    got = sr.wiener(X, a, masks, flags, n_iter=2)
    for t in range(4):
        assert np.array_equal(got[t], want[t])
    plain = sr.wiener(X, a, masks, flags & ~sr.FLAG_SOFTMASK, n_iter=2)
    assert not np.array_equal(plain[0], got[0])
