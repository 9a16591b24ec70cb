"""The fixtures of tests/fp32_weights.py are what they claim, and the float64 check of tests/test_gpu_fp32_weights_f64.py has teeth on
the fp32-resident plane GEMMs, without a GPU: the numpy emulation of form 2 (tests/planes_f32_emu.py) is fed through stage_f64.check on
fc1 (K = 2974, the adaptive row scale) and on the lstm stage behind W_ih (K = 512, two source tensors across bsplit) at hidden 512,
T = 24, targets 0 and 3, for `plain` and `wide`, with C_DEFAULT and FLOOR as they are.

  * The complete form passes: fc1 at 0.48 of its bound on both fixtures (2.2 times the float32 evaluation's distance over the whole
    segment, 2.0 - 2.2 in the worst frame), the lstm stage at 0.16 - 0.18 on `plain` (0.8 / 0.8 - 0.9) and 0.13 on `wide` (0.7 / 0.7).
    fc1's figures on `wide` are `plain`'s to the digit: rows 2^-12 of the tensor's maximum lose no bit under the tensor's one scale
    (the second plane's last bit is at 2^-20 of the scaled value 2^2, above fp16's 2^-24), as csrc/gemm_planes.h says of anything
    within 2^17.  These are the figures a GPU result is judged against (tests/test_gpu_fp32_weights_f64.py quotes both).
  * (a) The low weight plane dropped FAILS fc1 (112 - 126 times the bound) and the lstm stage behind W_ih (110 - 180) on both
    fixtures; it is 8e-5 - 1.9e-4 from float64.
  * (b) The forward tensor's unscale on the reverse tensor's columns and (c) both tensors' planes under one scale from the common
    maximum, each unscaled with its own, FAIL the lstm stage on `wide` (7e5 - 8e5 and 6.5e4 - 6.6e4 times the bound: the reverse
    direction is wrong by a factor of 8).  On `plain` the two directions share one exponent and both faults leave the bits of the
    complete form: no float32 weight the suite ran before `wide` could have shown either.
"""
import numpy as np
import pytest

import fp32_weights as fw
import planes_f32_emu as pe
import stage_f64 as sf

H, T, SEED = 512, 24, 81
TARGETS = (0, fw.ZERO_TARGET)
KINDS = ("plain", "wide")


@pytest.fixture(scope="module")
def weights(pkg):
    return {"plain": fw.plain(pkg.ggml, H, SEED), "wide": fw.wide(pkg.ggml, H, SEED)}


@pytest.fixture(scope="module")
def acts(pkg, weights):
    """(kind, target) -> (x, a1, lo, a2, state) of that target's own weights."""
    return {(k, t): fw.cpu_activations(pkg.ggml, weights[k][t], H, T) for k in KINDS for t in TARGETS}


@pytest.fixture(scope="module")
def measured(weights, acts):
    """(kind, target, fault, stage) -> the row of stage_f64.check."""
    out = {}
    for k in KINDS:
        for t in TARGETS:
            wt = weights[k][t]
            x, a1, lo, a2, state = acts[k, t]
            refs = {"fc1": (sf.fc1(wt, x, "float64"), sf.fc1(wt, x, "float32")),
                    "lstm": (sf.lstm(wt, H, a1, state, "float64"), sf.lstm(wt, H, a1, state, "float32"))}
            for fault in (None,) + pe.FAULTS:
                got = {"lstm": pe.lstm_stage(wt, H, a1, state, fault)}
                if fault in (None, "drop_lo"):  # fc1.weight is one source tensor: the other two faults do not touch it
                    got["fc1"] = pe.fc1_stage(wt, x, fault)
                for stage, g in got.items():
                    r = sf.check(stage, g, *refs[stage], "rows", where=f"[{k}, hidden {H}, target {t}, {fault or 'complete'}]")
                    assert (r["failure"] is None) == (r["excess"] <= 1.0), r  # never the yardstick caps
                    out[k, t, fault, stage] = r
                    print(f"{k} target {t} {fault or 'complete'} {stage}: excess {r['excess']:.2f}, rel L2 {r['rel']:.2e}, "
                          f"ratio to float32 {r['ratio_rel']:.2f} / {r['ratio_blk']:.2f}")
    return out


# ---------------------------------------------------------------- the fixtures are what they claim
def test_plain_keeps_full_mantissas(weights):
    """Not a dequantised tensor: far more than 65536 distinct values, and low mantissa bits in use."""
    w = weights["plain"][0]["fc2.weight"]
    assert w.dtype == np.float32 and np.unique(w).size > 0.9 * w.size
    assert (w.view(np.uint32) & np.uint32(0xFF)).any()


def test_wide_rows_span_two_to_the_twelve_and_stay_exact(weights):
    for t in range(4):
        p, w = weights["plain"][t], weights["wide"][t]
        for fc, bn in fw.DENSE:
            if t == fw.ZERO_TARGET and fc == "fc3":
                assert not w["fc3.weight"].any()
                continue
            g = fw.row_shifts(len(p[fc + ".weight"]))
            assert np.array_equal(w[fc + ".weight"].astype(np.float64) * np.exp2(g)[:, None], p[fc + ".weight"].astype(np.float64))  # exact
            assert np.array_equal(w[bn + ".running_mean"].astype(np.float64) * np.exp2(g), p[bn + ".running_mean"].astype(np.float64))
            assert np.array_equal(w[bn + ".weight"].astype(np.float64), p[bn + ".weight"].astype(np.float64) * np.exp2(g))
            assert 11.0 < fw.row_spread(w[fc + ".weight"]) < 13.0 and fw.row_spread(p[fc + ".weight"]) < 1.0
            assert fw.ROW_SPREAD - 1 == 12 < 17  # inside what csrc/gemm_planes.h documents as loss-free


def test_wide_directions_of_w_ih_carry_different_exponents(weights):
    for t in range(4):
        for layer in range(3):
            ef, er = (fw.load_exponent(weights["wide"][t][f"lstm.weight_ih_l{layer}{s}"]) for s in ("", "_reverse"))
            assert er - ef == fw.REVERSE_IH_SHIFT, (t, layer, ef, er)
            pf, pr = (fw.load_exponent(weights["plain"][t][f"lstm.weight_ih_l{layer}{s}"]) for s in ("", "_reverse"))
            assert pf == pr  # U(-k, k) twice: on plain weights bs[0] == bs[1], and a bsplit fault is invisible
    assert fw.load_exponent(np.zeros((3, 3), np.float32)) is None
    assert fw.load_exponent(np.array([0.75, -16384.0], np.float32)) == 0 and fw.load_exponent(np.array([1.0], np.float32)) == 14


def test_wide_stage_outputs_are_plains_in_float64(weights, acts):
    """fc1, fc2 and mask of `wide` equal `plain`'s to 1e-12 relative from the same inputs; target 3's mask is the constant."""
    for t in TARGETS:
        x, a1, lo, a2, _ = acts["plain", t]
        p, w = weights["plain"][t], weights["wide"][t]
        for name, f in (("fc1", lambda wt: sf.fc1(wt, x, "float64")), ("fc2", lambda wt: sf.fc2(wt, a1, lo, "float64")),
                        ("mask", lambda wt: sf.mask(wt, a2, "float64"))):
            if name == "mask" and t == fw.ZERO_TARGET:
                continue
            a, b = f(w), f(p)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (t, name)
            assert 0.01 < np.sqrt(np.mean(b ** 2)) < 10.0  # O(1): the per-frame metrics weigh every column alike
    wt = weights["wide"][fw.ZERO_TARGET]
    a2 = acts["wide", fw.ZERO_TARGET][3]
    ref = fw.zero_mask_reference(wt, T)
    assert np.array_equal(sf.mask(wt, a2, "float64"), ref) and (ref == ref[0]).all() and ref.max() > 0
    d = {k: np.asarray(v, np.float64) for k, v in wt.items()}
    bn0 = (0.0 - d["bn3.running_mean"]) / np.sqrt(d["bn3.running_var"] + 1e-5) * d["bn3.weight"] + d["bn3.bias"]
    want = np.maximum(bn0 * np.tile(d["output_scale"], 2) + np.tile(d["output_mean"], 2), 0.0)
    assert np.abs(ref[0] - want).max() <= 1e-12


def test_mixed_replaces_two_tensors_of_one_target(pkg, tmp_path):
    path = str(tmp_path / "m128.bin")
    pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=3), 128, compress=False)
    _, targets = pkg.ggml.read_model(path)
    mx = fw.mixed(targets)
    for t in range(4):
        for n, v in mx[t].items():
            if t == fw.MIXED_TARGET and n in fw.MIXED_NAMES:
                assert isinstance(v, np.ndarray) and v.dtype == np.float32 and np.array_equal(v, targets[t][n]["f32"])
            else:
                assert v is targets[t][n]
        assert all(np.array_equal(a, b) for a, b in zip(sf.target_weights(mx[t]).values(), sf.target_weights(targets[t]).values()))
    views, _keep = pkg.views_from_file_tensors(mx)
    f32_views = [(v.target, v.name.decode()) for v in views if v.dtype == pkg.DTYPE_F32]
    assert sorted(f32_views) == sorted((fw.MIXED_TARGET, n) for n in fw.MIXED_NAMES)
    deq = fw.dequantised(targets)
    assert all(v.dtype == pkg.DTYPE_F32 for v in pkg.views_from_file_tensors(deq)[0])


# ---------------------------------------------------------------- the emulation is the product
def test_the_emulated_product_is_the_product():
    rng = np.random.default_rng(2)
    a = np.tanh(rng.standard_normal((5, 200))).astype(np.float32)  # (K = 200: padded to 224)
    fwd = rng.uniform(-0.1, 0.1, (7, 200)).astype(np.float32)
    rev = (rng.uniform(-0.1, 0.1, (6, 200)) / 8).astype(np.float32)
    w = np.concatenate([fwd, rev]).astype(np.float64)
    ref = a.astype(np.float64) @ w.T
    # the split errors of both operands and the term not formed are 2^-22 of sum |a| |w| each, the fp32 accumulation below that
    bound = 4 * 2.0 ** -22 * (np.abs(a).astype(np.float64) @ np.abs(w).T)
    for fixed in (None, fw.SPLIT_FIXED_EXP):
        assert (np.abs(pe.product(a, [fwd, rev], fixed) - ref) <= bound).all()
        for fault in pe.FAULTS:
            assert (np.abs(pe.product(a, [fwd, rev], fixed, fault) - ref) > bound).any(), fault
    hi, lo = pe.weight_planes(fwd, fw.load_exponent(fwd))
    assert 2 ** 14 <= np.abs(hi).max() < 2 ** 15 and np.abs(lo).max() <= 8.0
    assert np.abs((hi.astype(np.float64) + lo) * 2.0 ** -fw.load_exponent(fwd) - fwd).max() <= 2.0 ** -22 * np.abs(fwd).max()
    z = pe.product(a, [np.zeros((4, 200), np.float32)])
    assert not z.any()


# ---------------------------------------------------------------- the check has teeth
@pytest.mark.parametrize("kind", KINDS)
def test_the_complete_form_passes(measured, kind):
    for t in TARGETS:
        for stage in ("fc1", "lstm"):
            r = measured[kind, t, None, stage]
            assert r["failure"] is None and r["excess"] <= 1.0, r


@pytest.mark.parametrize("kind", KINDS)
def test_a_dropped_low_weight_plane_fails(measured, kind):
    for t in TARGETS:
        for stage in ("fc1", "lstm"):
            r = measured[kind, t, "drop_lo", stage]
            assert r["excess"] > 1.0 and r["failure"].startswith(stage), r


@pytest.mark.parametrize("fault", ["unscale_fwd", "common_scale"])
def test_a_scale_of_the_wrong_direction_fails_on_wide_and_is_invisible_on_plain(measured, fault):
    """Both faults sit where the two directions of W_ih meet.  On `plain` the two tensors share one exponent and the faulty product has
    the bits of the complete one: no fixture the suite ran before could have seen either."""
    for t in TARGETS:
        r = measured["wide", t, fault, "lstm"]
        assert r["excess"] > 1.0 and r["failure"].startswith("lstm"), r
        p, c = measured["plain", t, fault, "lstm"], measured["plain", t, None, "lstm"]
        assert p["failure"] is None and p["rel"] == c["rel"] and p["blk"] == c["blk"], (p, c)
