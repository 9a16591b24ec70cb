"""Wiener EM iterations (UMX_FLAG_WIENER_ITERS) without a GPU: the float64 restatement of the reference loop (tests/wiener_em_ref.py)
is tied to the oracle at one iteration, and the flag's bits are checked against the header's other flags."""
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import rel_l2
import wiener_em_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "umx_hip.h"


def _case(seed, T, scale=30.0):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((2, T, 2049)) + 1j * rng.standard_normal((2, T, 2049))).astype(np.complex64) * scale
    mags = [(rng.uniform(0, 1.5, (2, T, 2049)) * np.abs(X)).astype(np.float32) for _ in range(4)]
    return X, mags


@pytest.mark.parametrize("T", [41, 230])  # one batch of the reference; two (the 200-frame batch boundary)
def test_restatement_at_one_iteration_matches_the_oracle(po, T):
    X, mags = _case(31 + T, T)
    X_before = X.copy()
    ref = wiener_em_ref.wiener_em(X, mags, n_iter=1)
    assert np.array_equal(X, X_before)  # the restatement divides a copy in place, not the caller's array
    got = po.wiener(X, mags)
    for j in range(4):
        assert rel_l2(got[j], ref[j]) <= 1e-5, (T, j)


def test_restatement_matches_the_float64_golden_vectors():
    """tests/golden/wiener_f64.npz: the reference's filter (one iteration) in float64 at twelve bins of a 230-frame case."""
    g = np.load(ROOT / "tests" / "golden" / "wiener_f64.npz")
    T, bins = int(g["T"]), g["bins"]
    rng = np.random.default_rng(int(g["seed"]))
    X = (rng.standard_normal((2, T, 2049)) + 1j * rng.standard_normal((2, T, 2049))).astype(np.complex64) * 30
    mags = [(rng.uniform(0, 1.5, (2, T, 2049)) * np.abs(X)).astype(np.float32) for _ in range(4)]
    y = wiener_em_ref.wiener_em(X, mags, n_iter=1)
    for j in range(4):
        assert rel_l2(y[j][:, :, bins], g["y"][j]) < 1e-5


def test_more_iterations_change_the_estimate_and_keep_the_mixture():
    """Iteration k >= 2 refines the estimates: they move, and since every iteration filters the mixture with gains that sum to
    (nearly) the identity, the four estimates still sum back to it."""
    X, mags = _case(7, 41)
    y1 = wiener_em_ref.wiener_em(X, mags, n_iter=1)
    y2 = wiener_em_ref.wiener_em(X, mags, n_iter=2)
    y3 = wiener_em_ref.wiener_em(X, mags, n_iter=3)
    for j in range(4):
        assert rel_l2(y2[j], y1[j]) > 1e-3, j
        assert rel_l2(y3[j], y2[j]) > 1e-6, j
    for y in (y2, y3):
        assert rel_l2(sum(y), X.astype(np.complex128)) < 1e-3


def test_float32_restatement_is_the_reference_precision():
    """precision="float32" stays in float32 and, at one iteration, lands where the float32 oracle does (within its rounding)."""
    X, mags = _case(11, 41)
    ref = wiener_em_ref.wiener_em(X, mags, n_iter=1)
    y32 = wiener_em_ref.wiener_em(X, mags, n_iter=1, precision="float32")
    assert all(y.dtype == np.complex64 for y in y32)
    for j in range(4):
        assert rel_l2(y32[j], ref[j]) < 1e-4, j


def _header_flags():
    """Every UMX_FLAG_* of the header as the set of bits it can take."""
    text = HEADER.read_text()
    flags = {}
    for name, arg, expr in re.findall(r"#define\s+UMX_FLAG_(\w+?)(?:\((\w)\))?\s+(\(.*?\)|0x[0-9A-Fa-f]+u?)\s*(?:/\*|$)", text, re.M):
        expr = re.sub(r"(0x[0-9A-Fa-f]+)u", r"\1", expr).replace("(unsigned)", "")
        if arg:
            vals = range(4) if name == "SKIP_TARGET" else range(1, 16)
            bits = 0
            for a in vals:
                bits |= eval(expr, {arg: a})
        else:
            bits = eval(expr)
        flags[name] = bits
    return flags


def test_wiener_iteration_flag_bits(pkg):
    flags = _header_flags()
    assert "WIENER_ITERS" in flags and "WIENER_ITERS_MASK" in flags, sorted(flags)
    assert flags["WIENER_ITERS"] == flags["WIENER_ITERS_MASK"] == 0xF0000
    for name, bits in flags.items():
        if name.startswith("WIENER_ITERS"):
            continue
        assert bits & flags["WIENER_ITERS_MASK"] == 0, name
    # the package's helper gives the header's values and refuses what the field cannot hold
    assert pkg.FLAG_WIENER_ITERS_MASK == 0xF0000
    for n in range(1, 16):
        assert pkg.FLAG_WIENER_ITERS(n) == n << 16
        assert pkg.FLAG_WIENER_ITERS(n) & ~pkg.FLAG_WIENER_ITERS_MASK == 0
    for bad in (0, 16, -1):
        with pytest.raises(ValueError):
            pkg.FLAG_WIENER_ITERS(bad)
    for name in ("FLAG_NO_WIENER", "FLAG_LSTM_STEPWISE", "FLAG_DEBUG_TAPS", "FLAG_LSTM_FORCE_SAFE", "FLAG_LSTM_PROFILE",
                 "FLAG_PRECISE_ACT", "FLAG_DEBUG_LSTM_ABORT", "FLAG_RESET_SEGMENTS"):
        assert getattr(pkg, name) & pkg.FLAG_WIENER_ITERS_MASK == 0, name
    assert all(pkg.FLAG_SKIP_TARGET(t) & pkg.FLAG_WIENER_ITERS_MASK == 0 for t in range(4))
