"""The gate functions over the whole float32 range, one cell step, and the three recurrence kernels on saturated gates.

Every other GPU test keeps the gate pre-activations within about +-2 (ggml.synth_weights: "so activations stay out of saturation"),
so a sigmoid near 0 or 1, tanh(c) at |c| > 2 and both polynomial seams went unchecked.  Here:

* umx_hip_debug_gate_math evaluates the device functions the kernels call -- tanh_epi, tanh_hw, the fast sigmoid, lstm_cell<false>,
  lstm_cell_flat, lstm_cell_lane<false> (the cell of both batched recurrences) -- and their PRECISE forms on a few million float32 values (every bit pattern around the seams 0.125 and 0.5 and
  around exp_hw's argument crossing -126, magnitudes from the smallest subnormal to FLT_MAX, +-0, +-inf, NaN, normals at scales 0.1
  to 100) against numpy float64.  A fast form may be C_DEFAULT times as far from float64 as its PRECISE form plus FLOOR, over all
  inputs and in every decade of |x|; tanh_epi meets the 3e-7 relative bound of its comment and tanh_hw a relative bound of C_DEFAULT
  times tanhf's plus FLOOR in each of its three ranges (no relative bound where float64's value is a float32 subnormal); oddness,
  the limits, NaN, the range and monotonicity across the seams hold exactly.  lstm_cell_flat and lstm_cell_lane<false> equal
  lstm_cell<false> bit for bit.
* The recurrences run with tests/stage_f64.py's saturating weights (weight_ih x 32, forget bias + 3, weight_hh untouched) on audio
  at four times the usual level, twice per context so that the second call starts from a saturated carried state, and every stage
  of the network is held against float64 with the unchanged yardstick.  The float64 restatement must show, on the engine's own fc1
  tap, the shares of stage_f64.SAT_MIN_SHARE.  Measured on the CPU on the oracle's fc1 outputs (tests/test_gate_math_checks.py;
  hidden 128 at T = 45 / hidden 512 at T = 40, targets 0 and 3): layer-0 pre-activations beyond |8| 52 - 57 % / 55 - 59 %, deeper
  layers 50 - 54 % / 54 %, |c| > 4 30 - 31 % / 29 - 30 %, g-gate arguments inside |x| < 0.125 0.8 - 0.9 % / 0.7 - 0.8 %; the float32
  evaluation is 1.7e-6 - 2.5e-6 (worst frame 3.4e-6 - 5.5e-6) / 4.8e-6 - 7.6e-6 (8.1e-6 - 1.3e-5) from float64, far inside the caps
  of 1e-3 / 3e-3.  With weight_ih x 16 at the usual level only 0.6 - 1 % of layer 0 passes |8|; unscaled, none.

UMX_STAGE_F64_REPORT=<file>: append every check's figures to that file (JSON lines)."""
import numpy as np
import pytest

import stage_f64 as sf
import test_gpu_geometry_f64 as geo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    import torch
    torch.zeros(1).cuda()  # a current device for the debug entry point


def test_gate_functions_over_the_float32_range(pkg, device):
    m = sf.gate_magnitudes()
    x = sf.gate_inputs(m)
    assert 2_000_000 < x.size < 6_000_000
    fns, _ = pkg.debug_gate_math(x=x)
    rep = sf.Report()
    figures = sf.check_gate_functions(rep, m, fns)
    print("\n".join(f"{k}: {v:.3e}" for k, v in figures.items()))
    geo._finish(rep, "gate_functions")


def test_cell_step_forms_agree_and_keep_a_nan_in_its_quad(pkg, device):
    pre, c, group = sf.cell_inputs()
    pn, units = sf.nan_planted(pre)
    W, Wn = len(pre), len(pn)
    _, cells = pkg.debug_gate_math(pre=np.concatenate([pre, pn]), c=np.concatenate([c, c[:Wn]]))
    rep = sf.Report()
    fast, flat, precise, lane = (cells[k] for k in pkg.CELL_FORMS)
    groups = np.concatenate([group, np.full(Wn, "one NaN")])
    sf.check_cell_same_bits(rep, "lstm_cell<false>", fast, "lstm_cell_flat", flat, groups)
    sf.check_cell_same_bits(rep, "lstm_cell<false>", fast, "lstm_cell_lane<false>", lane, groups)
    for name, got in (("lstm_cell<false>", fast), ("lstm_cell_flat", flat), ("lstm_cell_lane<false>", lane)):
        worst = sf.check_cell_yardstick(rep, name, pre, c, group, (got[0][:W], got[1][:W]), (precise[0][:W], precise[1][:W]))
        print(f"{name}: worst ratio to lstm_cell<true> {worst:.2f}")
    for name, got in zip(pkg.CELL_FORMS, (fast, flat, precise, lane)):
        sf.check_cell_nan_isolation(rep, name, (got[0][:Wn], got[1][:Wn]), (got[0][W:], got[1][W:]), units)
    geo._finish(rep, "cell_step")


# ---------------------------------------------------------------- the recurrence kernels on saturated gates
@pytest.fixture(scope="module")
def models(pkg, tmp_path_factory):
    """(hidden, saturating) -> file tensors; the synthetic weights of a width are drawn once."""
    drawn, made = {}, {}

    def get(H, sat):
        if (H, sat) not in made:
            if H not in drawn:
                drawn[H] = pkg.ggml.synth_weights(H, seed=81)
            path = str(tmp_path_factory.mktemp("gate") / f"m{H}_{int(sat)}.bin")
            pkg.ggml.write_model(path, sf.saturating_weights(drawn[H]) if sat else drawn[H], H, compress=False)
            made[(H, sat)] = pkg.ggml.read_model(path)[1]
        return made[(H, sat)]
    return get


def _state(eng, lane):
    return eng.stream_get() if eng.tracks == 1 else eng.track_stream_get(lane)


def _recurrence_case(pkg, targets, test, H, tracks, T, kernel, check_lanes, which, sat=True, flags=0, loud_lane=None, after_run=None):
    """Two calls of a context; the network stages of the second against float64 on `check_lanes`, and the saturation shares from the
    float64 restatement on the engine's own fc1 tap.  loud_lane: that lane's audio at 30 times the usual level (fc1's tanh_epi
    saturates).  after_run(eng): further assertions on the context after the second call (tests/test_gpu_one_track_f64.py)."""
    N = sf._N(T, 517)
    level = np.float32(sf.SAT_INPUT_LEVEL if sat else 1.0)
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=tracks)
    try:
        geo._run(pkg, eng, [geo._audio(pkg, N - 5 * b, 1100 + b) * level for b in range(tracks)], flags)
        states = {b: _state(eng, b) for b in check_lanes}
        waves = [geo._audio(pkg, N - 11 * b, 1200 + b) * level for b in range(tracks)]
        if loud_lane is not None:
            waves[loud_lane] = geo._audio(pkg, N, 1300) * np.float32(30.0)
        geo._run(pkg, eng, waves, flags)
        assert eng.lstm_kernel_name() == kernel, eng.lstm_kernel_name()
        if after_run is not None:
            after_run(eng)
        for b in check_lanes:
            where = f"{test}, {'saturating' if sat else 'plain'} weights, flags {flags:#x}" + (", audio x 30" if b == loud_lane else "")
            c0 = states[b].reshape(4, 3, 2, 2, H // 2)[:, :, :, 1]
            assert np.abs(c0).max() > (4.0 if sat else 0.0), f"lane {b}: the carried cell states reach only {np.abs(c0).max()}"
            geo.check_network(rep, eng, b, targets, states[b], where, which=which)
            if b == loud_lane:
                a1 = eng.tap("fc1" + geo._sfx(eng, b), which[0])
                assert np.mean(np.abs(a1) > 0.99) > 0.05, f"fc1 of the loud lane is not saturated: {np.mean(np.abs(a1) > 0.99):.2%} beyond 0.99"
            elif sat:
                for t in which:
                    _, pres, cells = sf.bilstm_f64(sf.target_weights(targets[t]), H, eng.tap("fc1" + geo._sfx(eng, b), t),
                                                   states[b][t * 12 * (H // 2):(t + 1) * 12 * (H // 2)])
                    shares = sf.saturation_shares(pres, cells)
                    print(f"{where}, lane {b}, target {t}: " + ", ".join(f"{k} {v:.1%}" for k, v in shares.items()))
                    sf.check_saturation(rep, shares, f"[{where}, lane {b}, target {t}]")
    finally:
        eng.close()
    geo._finish(rep, test)


def test_persistent_kernel_on_saturated_gates(pkg, models):
    _recurrence_case(pkg, models(128, True), "saturated_persistent", 128, 1, 45, "lstm_persistent_kernel", (0,), range(4))


def test_batch_kernel_on_saturated_gates_and_a_lane_at_30_times_the_level(pkg, models):
    _recurrence_case(pkg, models(128, True), "saturated_batch", 128, 3, 45, "lstm_batch_kernel", (0, 1, 2), range(4), loud_lane=1)


def test_batch_kernel_on_saturated_gates_precise_activations(pkg, models):
    _recurrence_case(pkg, models(128, True), "saturated_batch_precise", 128, 3, 45, "lstm_batch_kernel", (0, 2), range(4),
                     flags=pkg.FLAG_PRECISE_ACT)


def test_batch8_kernel_one_octet_per_workgroup_on_saturated_gates(pkg, models):
    _recurrence_case(pkg, models(512, True), "saturated_batch8", 512, 9, 101, "lstm_batch8_kernel", (0, 8), (0, 3))


@pytest.mark.parametrize("sat", [True, False], ids=["saturating", "plain"])
def test_batch8_kernel_two_octets_at_the_production_width(pkg, models, sat):
    """hidden 1024, 40 lanes (33 .. 64: two octets per workgroup in turn), T = 41; lanes 0, 33 and 39.  With plain synth_weights this
    is the production width's fc1, lstm, fc2, mask and target_mag against float64."""
    _recurrence_case(pkg, models(1024, sat), "batch8_two_octets_" + ("saturated" if sat else "plain"), 1024, 40, 41,
                     "lstm_batch8_kernel", (0, 33, 39), (0, 3), sat=sat)
