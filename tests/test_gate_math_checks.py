"""The gate-function, cell-step and saturation checks of tests/stage_f64.py have teeth (CPU only): numpy float32 emulations of
tanh_epi, tanh_hw, the fast sigmoid and the quad cell pass every check of tests/test_gpu_gate_math.py, and each planted fault fails
with a message that names the function and the range.  Also: the float64 restatement of the BiLSTM against torch's, and the
saturating weights reach their shares on the oracle's fc1 outputs (the figures in the docstring of tests/test_gpu_gate_math.py).
At the widths of tests/test_gpu_one_track_f64.py, targets 0 and 3, the second of two segments (hidden 256 at T = 45 / hidden 1024 at
T = 41): layer-0 pre-activations beyond |8| 50 - 58 % / 55 - 56 %, deeper layers 55 - 56 % / 54 %, |c| > 4 29 - 31 % / 30 - 32 %, g-gate
arguments inside |x| < 0.125 0.7 - 0.8 % / 0.7 - 0.8 %; the float32 evaluation is 4.9e-6 - 5.8e-6 (worst frame 9.8e-6 - 1.4e-5) /
6.2e-6 - 8.3e-6 (8.7e-6 - 1.3e-5) from float64."""
import numpy as np
import pytest

import stage_f64 as sf

f32 = np.float32


# ---------------------------------------------------------------- numpy float32 emulations of csrc/lstm_kernels.h and gemm_common.h
def _exp2(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(a.astype(f32)).astype(f32)


def _rcp(a):
    with np.errstate(divide="ignore"):
        return (f32(1.0) / a).astype(f32)


def tanh_hw_emu(x, seam=0.125, keep_sign=True):
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = _exp2((f32(-2.0) * np.abs(x)) * f32(1.44269504088896341))
        big = (f32(1.0) - e) * _rcp(f32(1.0) + e)
        big = np.copysign(big, x) if keep_sign else np.where(x < 0, -big, big)
        x2 = x * x
        poly = x * (x2 * (x2 * (x2 * f32(-0.0539682540) + f32(0.133333333)) + f32(-0.333333333)) + f32(1.0))
        if not keep_sign:
            poly = np.where(x == 0, f32(0.0), poly)  # a dropped copysign: -0.0 comes out as +0.0
        return np.where(np.abs(x) < f32(seam), poly, big).astype(f32)


def tanh_epi_emu(x, seam=0.5):
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ax, u = np.abs(x), x * x
        e = _exp2(ax * f32(-2.88539008177792681))
        big = (f32(1.0) - e) * _rcp(f32(1.0) + e)
        q = u * f32(-0.006946978159248829) + f32(0.021472707390785217)
        for k in (-0.05393378809094429, 0.1333322674036026, -0.3333333134651184):
            q = u * q + f32(k)
        small = ax * (u * q + f32(1.0))
        return np.copysign(np.where(ax < f32(seam), small, big), x).astype(f32)


def sigmoid_hw_emu(x, clip=None):
    x = np.asarray(x, f32)
    if clip is not None:
        x = np.where(np.isnan(x), x, np.clip(x, -f32(clip), f32(clip)))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return _rcp(f32(1.0) + _exp2(-x * f32(1.44269504088896341)))


def precise_emu(x):
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.tanh(x).astype(f32), (f32(1.0) / (f32(1.0) + np.exp(-x).astype(f32))).astype(f32)


def cell_emu(pre, c, precise=False, leak=False):
    """The quad cell in float32; leak: unit u takes the o gate of unit u + 1 (a quad shuffle that reads across its quad)."""
    p = np.asarray(pre, f32).reshape(-1, 16, 4)
    c = np.asarray(c, f32)
    th, sg = (lambda v: precise_emu(v)[0], lambda v: precise_emu(v)[1]) if precise else (tanh_hw_emu, sigmoid_hw_emu)
    i, f, g, o = sg(p[..., 0]), sg(p[..., 1]), th(p[..., 2]), sg(p[..., 3])
    if leak:
        o = np.roll(o, -1, axis=1)
    with np.errstate(invalid="ignore"):
        c1 = (f * c + i * g).astype(f32)
        return c1, (o * th(c1)).astype(f32)


def cell_lane_emu(pre, c, order=(0, 1, 2, 3)):
    """The one-lane cell of the batched recurrences (lstm_cell_lane): the lane of a unit takes the quad's four pre-activations as
    (i, f, g, o) arguments.  order: which pre-activation each argument gets ((0, 2, 1, 3): f and g handed over in each other's place)."""
    p = np.asarray(pre, f32).reshape(-1, 16, 4)
    c = np.asarray(c, f32)
    i, f, g, o = (fn(p[..., k]) for fn, k in zip((sigmoid_hw_emu, sigmoid_hw_emu, tanh_hw_emu, sigmoid_hw_emu), order))
    with np.errstate(invalid="ignore"):
        c1 = (f * c + i * g).astype(f32)
        return c1, (o * tanh_hw_emu(c1)).astype(f32)


@pytest.fixture(scope="module")
def mags():
    return sf.gate_magnitudes(seed=0, n_random=60_000)


def _fns(x, **fault):
    t, s = precise_emu(x)
    return {"tanh_epi": tanh_epi_emu(x, **fault.get("tanh_epi", {})), "tanh_hw": tanh_hw_emu(x, **fault.get("tanh_hw", {})),
            "sigmoid_hw": sigmoid_hw_emu(x, **fault.get("sigmoid_hw", {})), "tanhf": t, "sigmoid_ref": s}


def _failures(m, **fault):
    rep = sf.Report()
    sf.check_gate_functions(rep, m, _fns(sf.gate_inputs(m), **fault))
    return rep.failures()


def test_inputs_cover_seams_subnormals_and_the_exp_argument_crossings(mags):
    m = mags
    assert m[0] == 0 and np.isinf(m[-1]) and m[1] == f32(1.4e-45) and np.all(np.diff(m) > 0)
    for lo, hi in ((0.1249, 0.1251), (0.4999, 0.5001), (87.2, 87.5), (43.6, 43.75)):
        w = m[(m >= f32(lo)) & (m <= f32(hi))]
        assert np.all(np.diff(w.view(np.uint32)) == 1), (lo, hi)  # every bit pattern
    assert all(np.any((m >= 10.0 ** d) & (m < 10.0 ** (d + 1))) for d in range(-45, 38))
    x = sf.gate_inputs(m)
    assert np.signbit(x[len(m)]) and x[len(m)] == 0 and np.isnan(x[-1]) and x.size == 2 * m.size + 1


def test_unplanted_emulations_pass_every_check(mags):
    f = _failures(mags)
    assert not f, "\n".join(f)


def test_checks_fail_a_seam_moved_to_0_13(mags):
    """tanh_epi's seam at 0.13 instead of 0.5: the 1 - e form runs where it cancels (1 - e = 0.23 at 0.13) and the relative error
    there passes 3e-7 although the absolute error stays within the yardstick."""
    f = _failures(mags, tanh_epi={"seam": 0.13})
    assert f and all(s.startswith("tanh_epi ") for s in f), f
    assert any("0.125 <= |x| < 0.5" in s and "relative" in s for s in f), f


def test_checks_fail_a_dropped_copysign_at_minus_zero(mags):
    f = _failures(mags, tanh_hw={"keep_sign": False})
    assert len(f) == 1 and f[0].startswith("tanh_hw x = -0.0") and "-0.0 is lost" in f[0], f


def test_checks_fail_a_sigmoid_clipped_at_8(mags):
    f = _failures(mags, sigmoid_hw={"clip": 8.0})
    assert f and all(s.startswith("sigmoid_hw ") for s in f), f
    assert any("|x| in [1e1, 1e2)" in s for s in f) and any("x = +-inf" in s for s in f), f
    assert not any("[1e-1, 1e0)" in s for s in f), f


@pytest.fixture(scope="module")
def cells():
    pre, c, group = sf.cell_inputs(seed=0)
    return pre, c, group, cell_emu(pre, c, precise=True)


def _cell_failures(cells, leak):
    pre, c, group, precise = cells
    rep = sf.Report()
    got = cell_emu(pre, c, leak=leak)
    sf.check_cell_yardstick(rep, "cell_emu", pre, c, group, got, precise)
    sf.check_cell_same_bits(rep, "cell_emu", cell_emu(pre, c), "cell_emu again", got, group)
    pn, units = sf.nan_planted(pre)
    sf.check_cell_nan_isolation(rep, "cell_emu", (got[0][:len(pn)], got[1][:len(pn)]), cell_emu(pn, c[:len(pn)], leak=leak), units)
    return rep.failures()


def test_cell_inputs_reach_the_saturated_corners(cells):
    pre, c, group, _ = cells
    assert np.abs(c).max() > 290 and set(group.tolist()) >= {"saturated corners", "pre ~ N(0, 40), |c| <= 300"}
    corner = pre[group == "saturated corners"][0].reshape(16, 4)
    assert len({tuple(r) for r in np.sign(corner).tolist()}) == 16
    i, f, g, o = (sf.gate_ref(k, corner[:, j]) for j, k in enumerate(("sigmoid", "sigmoid", "tanh", "sigmoid")))
    assert set(np.round(i, 12)) == {0.0, 1.0} and set(np.round(g, 12)) == {-1.0, 1.0}


def test_unplanted_cell_passes(cells):
    f = _cell_failures(cells, leak=False)
    assert not f, "\n".join(f)


def test_checks_fail_a_cell_that_lets_the_neighbouring_units_gate_through(cells):
    f = _cell_failures(cells, leak=True)
    assert any(s.startswith("cell_emu h pre ~ N(0, 1), |c| <= 1:") for s in f), f  # the yardstick, naming cell and range
    assert any("changed unit(s)" in s and "NaN in unit" in s for s in f), f        # the NaN isolation
    assert any("bit for bit" in s for s in f), f


def _lane_cell_failures(cells, order):
    """The checks tests/test_gpu_gate_math.py runs on lstm_cell_lane<false>: the yardstick, the same bits as the quad cell, NaN isolation."""
    pre, c, group, precise = cells
    rep = sf.Report()
    got = cell_lane_emu(pre, c, order)
    sf.check_cell_yardstick(rep, "cell_lane_emu", pre, c, group, got, precise)
    sf.check_cell_same_bits(rep, "cell_emu", cell_emu(pre, c), "cell_lane_emu", got, group)
    pn, units = sf.nan_planted(pre)
    sf.check_cell_nan_isolation(rep, "cell_lane_emu", (got[0][:len(pn)], got[1][:len(pn)]), cell_lane_emu(pn, c[:len(pn)], order), units)
    return rep.failures()


def test_unplanted_lane_cell_passes_and_has_the_quad_cells_bits(cells):
    f = _lane_cell_failures(cells, (0, 1, 2, 3))
    assert not f, "\n".join(f)


def test_checks_fail_a_lane_cell_that_takes_f_and_g_in_each_others_place(cells):
    f = _lane_cell_failures(cells, (0, 2, 1, 3))
    assert any(s.startswith("cell_lane_emu ") and "N(0, 1), |c| <= 1:" in s for s in f), f  # the yardstick, naming cell and range
    assert any("bit for bit" in s for s in f), f
    assert not any("changed unit(s)" in s for s in f), f  # the fault stays inside its unit: the NaN isolation has nothing to report


# ---------------------------------------------------------------- the recurrence on saturated gates
def _weights(pkg, H, seed, sat):
    w = pkg.ggml.synth_weights(H, seed=seed)
    return sf.saturating_weights(w) if sat else w


def test_saturating_weights_touch_only_weight_ih_and_the_forget_bias(pkg):
    w = pkg.ggml.synth_weights(32, seed=1)
    s = sf.saturating_weights(w)
    for t in range(4):
        for k, v in w[t].items():
            if k.startswith("lstm.weight_ih"):
                assert np.array_equal(s[t][k], v * f32(sf.SAT_IH_GAIN))
            elif k.startswith("lstm.bias_ih"):
                d = s[t][k] - v
                assert np.allclose(d[16:32], 3, atol=1e-6) and not d[:16].any() and not d[32:].any()
            else:
                assert np.array_equal(s[t][k], v), k
    with pytest.raises(AssertionError, match="chaotic"):
        sf.saturating_weights(w, hh_gain=16.0)


@pytest.mark.parametrize("sat", [False, True], ids=["plain", "saturating"])
def test_float64_restatement_of_the_bilstm_matches_torch(pkg, sat):
    H, T = 64, 37
    wt = _weights(pkg, H, 5, sat)[2]
    rng = np.random.default_rng(8)
    a1 = np.tanh(rng.standard_normal((T, H)) * 1.5).astype(f32)
    state = (rng.standard_normal(12 * (H // 2)) * np.repeat([0.5, 3.0] * 6, H // 2)).astype(f32)  # h within +-1.5, c larger
    out, pres, cells = sf.bilstm_f64(wt, H, a1, state)
    np.testing.assert_allclose(out, sf.lstm(wt, H, a1, state, "float64"), rtol=0, atol=1e-12)
    assert len(pres) == 3 and pres[0][1].shape == (T, 2 * H) and cells[2][0].shape == (T, H // 2)
    # the last cell state of a forward chain follows from its last pre-activations and the cell before
    g, Hl = pres[0][0][-1], H // 2
    c = sf.gate_ref("sigmoid", g[Hl:2 * Hl]) * cells[0][0][-2] + sf.gate_ref("sigmoid", g[:Hl]) * np.tanh(g[2 * Hl:3 * Hl])
    np.testing.assert_allclose(c, cells[0][0][-1], atol=1e-13)


@pytest.mark.parametrize("H,T", [(128, 45), (512, 40), (256, 45), (1024, 41)])
def test_saturating_weights_reach_their_shares_on_the_oracles_fc1_outputs(pkg, po, tmp_path, H, T):
    """What tests/test_gpu_gate_math.py asserts on the engine's fc1 tap, here on the oracle's: the shares of SAT_MIN_SHARE, and a
    float32 evaluation that stays inside the yardstick caps (the recurrence is still contractive); unscaled weights saturate nothing."""
    N = sf._N(T, 99)
    wave = pkg.ggml.synth_audio(N, seed=41) * f32(sf.SAT_INPUT_LEVEL)
    path = str(tmp_path / "sat.bin")
    pkg.ggml.write_model(path, _weights(pkg, H, 81, True), H, compress=False)
    _, targets = pkg.ggml.read_model(path)
    om = po.Model.load(path)
    state = po.stream_state(H)
    po.umx_inference(om, wave, state=state)  # the second call starts from a carried state
    carried = state.copy()
    _, taps = po.umx_inference(om, wave[:, ::-1].copy(), state=state, want_taps=True)
    for t in (0, 3):
        wt = sf.target_weights(targets[t])
        a1, st = taps["fc1_out"][t], carried[t * 12 * (H // 2):(t + 1) * 12 * (H // 2)]
        out, pres, cells = sf.bilstm_f64(wt, H, a1, st)
        shares = sf.saturation_shares(pres, cells)
        print(f"hidden {H} target {t}: " + ", ".join(f"{k} {v:.1%}" for k, v in shares.items()))
        rep = sf.Report()
        sf.check_saturation(rep, shares, f"hidden {H} target {t}")
        r = rep.add(sf.check("lstm", out.astype(f32), out, sf.lstm(wt, H, a1, st, "float32"), "rows"))
        print(f"  float32 against float64: {r['rel32']:.2e} / worst frame {r['blk32']:.2e}")
        rep.assert_ok()
        np.testing.assert_allclose(taps["lstm_out"][t], out, atol=2e-4)  # the oracle ran these weights too
    plain = sf.target_weights(_file_tensors(pkg, tmp_path, H)[0])
    _, pres, cells = sf.bilstm_f64(plain, H, taps["fc1_out"][0], carried[:12 * (H // 2)] * 0)
    sh = sf.saturation_shares(pres, cells)
    assert sh["layer 0 |pre| > 8"] == 0 and sh["|c| > 4"] == 0, sh


def _file_tensors(pkg, tmp_path, H):
    path = str(tmp_path / "plain.bin")
    pkg.ggml.write_model(path, _weights(pkg, H, 81, False), H, compress=False)
    return pkg.ggml.read_model(path)[1]
