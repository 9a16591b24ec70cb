"""The one-track context -- what umx-cli runs: gemm_bf16x3_kernel for fc1, W_ih, fc2 and fc3, lstm_persistent_kernel for the recurrence
-- against float64 (tests/stage_f64.py) at hidden 256, 512 and 1024.  The width changes the code that runs: the persistent kernel's
register layout (readlane at 16 and 32 k per wave, DPP rotations at 64), the length of the GEMMs' fp32 accumulation chains (K = 1024
for W_ih and fc3, 2048 for fc2 at hidden 1024), and with T the number of 128-row tiles and how far the recurrence's ring of W_ih rows
(32 rows, filled 16 at a time) gets.  Every context is pkg.Engine(targets, H, N, tracks=1) with default flags, every case asserts the
kernels by name, and every reference is computed from the engine's own tap of the stage's input; no bound of stage_f64 or
skewed_weights is changed.

  * plain weights at every register layout, on the second of two calls (a carried state);
  * T = 130 at hidden 512: a second 128-row tile with two valid rows and 126 rows of padding;
  * saturated gates (stage_f64.saturating_weights) at hidden 256 and 1024, and at 1024 under FLAG_PRECISE_ACT;
  * skewed weight ranges (tests/skewed_weights.py) at the real K: the u8 one-plane form of fc1 (K = 2974) and W_ih (K = 512 / 1024)
    with per-tensor centres, the six-term u16 form of fc2 (K = 1024 / 2048) and fc3, each against both float64 references; and W_hh
    alone skewed at hidden 1024 (the persistent kernel dequantises it per weight in registers);
  * segments shorter than, equal to and just past the ring's bulk and size (T = 5 .. 33), persistent against per-step bit for bit,
    and at hidden 128 against float64.

tests/test_one_track_checks_cpu.py shows on a numpy emulation of the GEMM (tests/bf16x3_emu.py) that these checks fail a kernel with
a second-order term dropped, a fixed centre or a row sum over rounded values -- faults the fp32 oracle's bounds would pass.

UMX_STAGE_F64_REPORT=<file>: append every check's distances to that file (JSON lines), as tests/test_gpu_geometry_f64.py does."""
import numpy as np
import pytest

import skewed_weights as sw
import stage_f64 as sf
import test_gpu_affine_offset as aff
import test_gpu_gate_math as gm
import test_gpu_geometry_f64 as geo

pytestmark = pytest.mark.gpu

GEMM, PERSISTENT, STEP = "gemm_bf16x3_kernel", "lstm_persistent_kernel", "lstm_step_kernel"
RING, BULK = 32, 16  # csrc/lstm_kernels.h LSTM_P_RING, LSTM_P_BULK


@pytest.fixture(scope="module")
def models(pkg, tmp_path_factory):
    """(hidden, saturating) -> file tensors of ggml.synth_weights(hidden, seed=81); each width is drawn once."""
    drawn, made = {}, {}

    def get(H, sat=False):
        if (H, sat) not in made:
            if H not in drawn:
                drawn[H] = pkg.ggml.synth_weights(H, seed=81)
            path = str(tmp_path_factory.mktemp("one_track") / f"m{H}_{int(sat)}.bin")
            pkg.ggml.write_model(path, sf.saturating_weights(drawn[H]) if sat else drawn[H], H, compress=False)
            made[(H, sat)] = pkg.ggml.read_model(path)[1]
        return made[(H, sat)]
    return get


@pytest.fixture(scope="module")
def fixtures(pkg, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sw.make_fixture(pkg.ggml, name, tmp_path_factory.mktemp("skewed_one_track"))
        return made[name]
    return get


def assert_one_track_kernels(eng, persistent=True):
    names = [eng.gemm_kernel_name(m) for m in range(4)]
    assert names == [GEMM] * 4, names
    assert eng.lstm_kernel_name() == (PERSISTENT if persistent else STEP), eng.lstm_kernel_name()
    assert eng.lstm_was_persistent() == persistent


def _two_calls(pkg, eng, N, seed, flags=0):
    """-> (stems of both calls, the state after each)."""
    stems, states = [], []
    for s in (0, 1):
        stems.append(geo._run(pkg, eng, [geo._audio(pkg, N - 5 * s, seed + 10 * s)], flags)[0])
        states.append(eng.stream_get())
    return stems, states


# ---------------------------------------------------------------- a. plain weights, every register layout
@pytest.mark.parametrize("H,which", [(256, (0, 1, 2, 3)), (512, (0, 1, 2, 3)), (1024, (0, 3))], ids=["h256", "h512", "h1024"])
def test_plain_weights_at_every_register_layout(pkg, models, H, which):
    """T = 41, the second of two calls, from the state the first left: fc1, lstm, fc2, mask and target_mag."""
    targets, N = models(H), sf._N(41, 517)
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=1)
    try:
        geo._run(pkg, eng, [geo._audio(pkg, N, 3100)], 0)
        state = eng.stream_get()
        assert np.abs(state).max() > 0
        geo._run(pkg, eng, [geo._audio(pkg, N - 11, 3110)], 0)
        assert_one_track_kernels(eng)
        geo.check_network(rep, eng, 0, targets, state, f"one track, hidden {H}, carried state", which=which)
    finally:
        eng.close()
    geo._finish(rep, f"one_track_plain_{H}")


# ---------------------------------------------------------------- b. two GEMM row tiles
def test_two_row_tiles_of_the_gemm(pkg, models):
    """Hidden 512, T = 130: Tp = 256, the second 128-row tile holds frames 128 and 129 and 126 rows of padding.  The worst-frame
    figure is what a bad tile edge shows in."""
    H, T = 512, 130
    targets, N = models(H), sf._N(T, 517)
    assert -(-T // 128) * 128 == 256
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=1)
    try:
        assert eng.T == T
        state = eng.stream_get()
        assert not state.any()
        geo._run(pkg, eng, [geo._audio(pkg, N, 3200)], 0)
        assert_one_track_kernels(eng)
        geo.check_network(rep, eng, 0, targets, state, "one track, two row tiles", which=(0, 3))
    finally:
        eng.close()
    for r in rep.rows:
        if r["failure"]:
            print(f"{r['stage']}: worst frame {r['block']} of {T} ({'second' if r['block'] >= 128 else 'first'} row tile)")
    geo._finish(rep, "one_track_two_row_tiles")


# ---------------------------------------------------------------- c. saturated gates on the persistent kernel
@pytest.mark.parametrize("H,T,which,precise", [(256, 45, (0, 1, 2, 3), False), (1024, 41, (0, 3), False), (1024, 41, (0, 3), True)],
                         ids=["h256", "h1024", "h1024_precise_activations"])
def test_persistent_kernel_on_saturated_gates(pkg, models, H, T, which, precise):
    """tests/test_gpu_gate_math.py's case at the readlane layout of 16 k per wave and at the DPP layout: saturating weights, audio at
    four times the level, the second of two calls; the shares of SAT_MIN_SHARE are asserted on the engine's fc1 tap."""
    gm._recurrence_case(pkg, models(H, True), f"one_track_saturated_{H}" + ("_precise" if precise else ""), H, 1, T, PERSISTENT, (0,), which,
                        flags=pkg.FLAG_PRECISE_ACT if precise else 0, after_run=assert_one_track_kernels)


# ---------------------------------------------------------------- d. skewed weight ranges at the real K
@pytest.mark.parametrize("segment", ["first_segment", "carried_state"])
@pytest.mark.parametrize("name,which", [("h512_all", (0, 1, 2, 3)), ("h1024_all", (0, 1, 2)), ("h1024_hh", (0, 1))],
                         ids=["h512_all", "h1024_all", "h1024_hh"])
def test_skewed_weights_at_the_real_k(pkg, fixtures, name, which, segment):
    """One track, T = 40: every stage against the float64 evaluation with exact-affine matrices and against the definition's.  On the
    fully skewed models the control target (3, at hidden 512) keeps plain weights and its definition gap is negligible; on h1024_hh
    only W_hh is skewed, which the persistent kernel dequantises per weight: the lstm stage meets both references."""
    H, fams, targets = fixtures(name)
    assert fams == (frozenset({"hh"}) if name.endswith("_hh") else sw.ALL)
    N = sf._N(40, 301)
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=1)
    try:
        state = aff._zero_state(eng)
        if segment == "carried_state":
            geo._run(pkg, eng, aff._waves(pkg, N, 1, 3300), 0)
            state = eng.stream_get()
            assert np.abs(state).max() > 0
        geo._run(pkg, eng, aff._waves(pkg, N, 1, 3310), 0)
        assert_one_track_kernels(eng)
        worst = aff.check_network_both(rep, eng, 0, targets, state, f"one track, {name}, {segment}", which=which)
        print(f"one track, {name}, {segment}: worst ratio to the float32 evaluation {worst:.2f}")
        if sw.CONTROL_TARGET in which:
            gaps = [r["gap_rel"] for r in rep.rows if r["stage"].split()[0].endswith(f"[{sw.CONTROL_TARGET}]")]
            assert gaps and max(gaps) < 0.1 * sw.GAP_BOUND, gaps  # plain U(-k, k): measured on the CPU below 6e-8 (skewed_weights.py)
    finally:
        eng.close()
    geo._finish(rep, f"one_track_{name}_{segment}")


# ---------------------------------------------------------------- e. the W_ih row ring and short segments
def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


RING_CASES = [(128, T) for T in (5, BULK - 1, BULK, BULK + 1, RING - 1, RING, RING + 1)] + [(1024, T) for T in (5, BULK, BULK + 1, RING + 1)]


@pytest.mark.parametrize("H,T", RING_CASES, ids=[f"h{H}_T{T}" for H, T in RING_CASES])
def test_short_segments_persistent_has_the_bits_of_the_per_step_driver(pkg, models, model_small, H, T):
    """Two consecutive calls at T around the ring's bulk (16) and size (32), and T = 5 (N = 4096): the stems, the state after each call
    and the lstm tap of the second call are the per-step driver's bit for bit.  The two drivers share one dot-product order, so this
    shows that the ring hands the recurrence the right W_ih rows, not that the order is right: at hidden 128, T = 5 and 17 also go
    against float64."""
    targets = model_small[2] if H == 128 else models(H)
    N = sf._N(T, 0 if T == 5 else 517)
    assert (N == sf.N_MIN) == (T == 5)
    rep = sf.Report()
    res = {}
    eng = pkg.Engine(targets, H, N, tracks=1)
    try:
        assert eng.T == T
        for name, flags in (("persistent", 0), ("stepwise", pkg.FLAG_LSTM_STEPWISE)):
            eng.stream_reset()
            stems, states = _two_calls(pkg, eng, N, 3400, flags)
            assert_one_track_kernels(eng, persistent=name == "persistent")
            res[name] = (stems, states, [eng.tap("lstm", t) for t in range(4)])
            assert np.abs(states[0]).max() > 0 and all(np.isfinite(s).all() for s in states)
            if name == "persistent" and H == 128 and T in (5, BULK + 1):
                geo.check_network(rep, eng, 0, targets, states[0], f"one track, T = {T}, carried state")
    finally:
        eng.close()
    (sp, tp, lp), (ss, ts, ls) = res["persistent"], res["stepwise"]
    for call in (0, 1):
        assert _bits_equal(tp[call], ts[call]), f"state after call {call}"
        for t in range(4):
            assert _bits_equal(sp[call][t], ss[call][t]), f"stems of call {call}, target {t}"
    for t in range(4):
        bad = np.flatnonzero((lp[t].view(np.uint32) != ls[t].view(np.uint32)).any(axis=1))
        assert bad.size == 0, f"lstm tap, target {t}: frames {bad.tolist()} differ"
    geo._finish(rep, f"one_track_ring_{H}_{T}")
