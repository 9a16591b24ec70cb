"""The offset term of the quantised matrix products on ASYMMETRIC weight ranges (tests/skewed_weights.py), on the GPU.  A quantised
product applies the file's affine map to the accumulated sum, s sum a (q - c) + (o + c s) sum a; on weights whose zero-weight code lies
a quarter of the code range from the centre c the two terms cancel, and the rounding of the fp32 row sum is multiplied by |o + c s|.
No other fixture of the suite is asymmetric (ggml.synth_weights: U(-k, k)).

Each stage is compared twice (skewed_weights.check_both), its references computed from the engine's own tap of the stage's input:
  "arithmetic": against the float64 evaluation with exact-affine matrices float64(q) s + o -- bound C_DEFAULT x yardstick + FLOOR;
  "parity":     against the float64 evaluation of the reference's definition fl(fl(q s) + o) -- the same bound plus the fixture's
                definition gap of that stage, computed here from the same taps;
the yardstick is the float32 evaluation of the definition against the definition's float64, with stage_f64's caps.
tests/test_affine_offset_cpu.py shows on a numpy emulation that this check fails the fixed centres and passes the per-tensor one.

Covered here, every case with the kernels asserted by name:
  * the one-track context (gemm_bf16x3_kernel's u8 one-plane form, which centres every tensor at its zero-weight code);
  * the plane GEMMs of track-batched contexts, whose planes hold q - c with each source tensor's own centre since load_weight
    forms them with csrc/quant_planes.h, on the fully skewed models: hidden 128 at three lanes (gemm_planes_kernel's 128 x 128 tiles,
    lstm_batch_kernel; first segment and carried state), hidden 512 at ten lanes and hidden 1024 at nine (fc1 u8 and fc2 u16 on the
    128 x 128 tiles, W_ih u8 and fc3 u16 on gemm_planes_ps_kernel's 256 x 256 tiles, lstm_batch8_kernel);
  * gemm_planes_kernel / _pp_kernel / _ps_kernel on 256 x 256 tiles bit for bit on the fully skewed hidden-512 model, which ties the
    other two flavours to the one checked against float64;
  * the per-weight form of a three-lane context (UMX_CREATE_U8_DEQUANT);
    (the fp32-resident family that form belongs to -- form 2 of the plane GEMMs, lstm_batch_kernel<WQ = false>, the one-track
    context on float32 tensors -- is held to float64 at hidden 512 / 1024 by tests/test_gpu_fp32_weights_f64.py);
  * the batched recurrences' own W_hh offset term, which keeps the centre 128, on models with only W_hh skewed:
    lstm_batch_kernel at K = 64 (first segment, carried state, FLAG_PRECISE_ACT), lstm_batch8_kernel at K = 256 (hidden 512, ten
    lanes) and K = 512 (hidden 1024: nine lanes = one octet and a lane, 40 lanes = two octets per workgroup in turn), each on the
    first segment and from a carried state.

UMX_STAGE_F64_REPORT=<file>: append every check's distances to that file (JSON lines), as tests/test_gpu_geometry_f64.py does."""
import numpy as np
import pytest

import skewed_weights as sw
import stage_f64 as sf
import test_gpu_geometry_f64 as geo

pytestmark = pytest.mark.gpu

STAGES = ("fc1", "lstm", "fc2", "mask")
LOUD, QUIET = np.float32(30.0), np.float32(1e-5)


@pytest.fixture(scope="module")
def fixtures(pkg, tmp_path_factory):
    """name of skewed_weights.FIXTURES -> (hidden, families, file tensors); written once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = sw.make_fixture(pkg.ggml, name, tmp_path_factory.mktemp("skewed"))
        return made[name]
    return get


def check_network_both(rep, eng, lane, targets, state_before, where, which=range(4), parity_only=False):
    """fc1, lstm, fc2, mask of one lane of the last call, each twice (arithmetic, parity); parity_only: the per-weight form, against
    the definition with no gap allowance.  -> the worst ratio to the float32 evaluation over the added rows."""
    sfx, Hh = geo._sfx(eng, lane), eng.hidden
    T = sf.n_frames(eng.N)
    x = eng.tap("x" + sfx)[:, :2 * sf.CROP]
    worst = 0.0
    for t in which:
        st = state_before[t * 12 * (Hh // 2):(t + 1) * 12 * (Hh // 2)]
        a1, lo, a2, mk = (eng.tap(k + sfx, t) for k in STAGES)
        fns = sw.stage_functions(Hh, x, a1, lo, a2, st)
        for name, got in zip(STAGES, (a1, lo, a2, mk)):
            rows = sw.check_both(f"{name}[{t}]", got, *sw.stage_refs(targets[t], fns[name]), T=T, no_gap=parity_only,
                                 where=f"[{where}, lane {lane}, hidden {Hh}, T={T}]")
            for r in rows[1:] if parity_only else rows:
                rep.add(r)
                worst = max(worst, r["ratio_rel"], r["ratio_blk"])
    return worst


def _waves(pkg, N, lanes, seed, levels=None):
    return [geo._audio(pkg, N - 7 * b, seed + b) * (np.float32(1.0) if levels is None else levels[b]) for b in range(lanes)]


def _zero_state(eng):
    return np.zeros(eng.lib.umx_hip_stream_floats(eng.h), np.float32)


def _state(eng, lane):
    return eng.track_stream_get(lane)


def _lanes_case(pkg, targets, test, *, hidden, lanes, T, lstm_kernel, gemm_kernels, check_lanes, which=range(4), flags=0, carried=False,
                u8_dequant=False, loud=(1,), quiet=(2,)):
    """`lanes` lanes of a track-batched context: the lanes of `loud` at 30 times the level (the adaptive row scale multiplies the
    offset term), those of `quiet` at 1e-5 of it.  carried: two calls, the second checked from the state the first left.
    gemm_kernels: the kernel of fc1, W_ih, fc2, fc3."""
    N = sf._N(T, 517)
    rep = sf.Report()
    eng = pkg.Engine(targets, hidden, N, tracks=lanes, u8_dequant=u8_dequant)
    try:
        levels = [LOUD if b in loud else QUIET if b in quiet else np.float32(1.0) for b in range(lanes)]
        states = [_zero_state(eng)] * lanes
        if carried:
            geo._run(pkg, eng, _waves(pkg, N, lanes, 2100, levels), flags)
            states = [_state(eng, b) for b in range(lanes)]
            assert all(np.abs(states[b]).max() > 0 for b in check_lanes)
        geo._run(pkg, eng, _waves(pkg, N, lanes, 2200, levels), flags)
        assert eng.lstm_kernel_name() == lstm_kernel, eng.lstm_kernel_name()
        names = tuple(eng.gemm_kernel_name(m) for m in range(4))
        assert names == tuple(gemm_kernels), names
        worst = max(check_network_both(rep, eng, b, targets, states[b], test, which=which, parity_only=u8_dequant) for b in check_lanes)
        print(f"{test}: worst ratio to the float32 evaluation {worst:.2f}")
    finally:
        eng.close()
    return rep


SMALL_TILES = ("gemm_planes_kernel",) * 4
# fc1 and fc2 (N = hidden) have too few 256 x 256 tiles at nine or ten lanes; W_ih (N = 4 hidden) and fc3 (N = 4352) take the persistent kernel
MIXED_TILES = ("gemm_planes_kernel", "gemm_planes_ps_kernel", "gemm_planes_kernel", "gemm_planes_ps_kernel")


def _three_lane_case(pkg, targets, test, **kw):
    """hidden 128, three lanes, T = 41: lane 1 at 30 times the level, lane 2 at 1e-5 of it; 128 x 128 tiles, lstm_batch_kernel."""
    return _lanes_case(pkg, targets, test, hidden=128, lanes=3, T=41, lstm_kernel="lstm_batch_kernel", gemm_kernels=SMALL_TILES,
                       check_lanes=(0, 1, 2), **kw)


def test_one_track_staged_u8_one_plane_form(pkg, fixtures):
    """One track, hidden 128, T = 40: gemm_bf16x3_kernel's u8 one-plane form (fc1, W_ih), the persistent recurrence beside it."""
    _, _, targets = fixtures("h128_all")
    N = sf._N(40, 301)
    rep = sf.Report()
    eng = pkg.Engine(targets, 128, N, tracks=1)
    try:
        geo._run(pkg, eng, _waves(pkg, N, 1, 2000), 0)
        assert all(eng.gemm_kernel_name(m) == "gemm_bf16x3_kernel" for m in range(4))
        worst = check_network_both(rep, eng, 0, targets, _zero_state(eng), "one track")
        print(f"one track: worst ratio to the float32 evaluation {worst:.2f}")
    finally:
        eng.close()
    geo._finish(rep, "affine_one_track")


def test_three_lanes_per_weight_form_needs_no_gap_allowance(pkg, fixtures):
    """UMX_CREATE_U8_DEQUANT dequantises every weight as the reference defines it: it meets the definition's float64 with NO gap
    allowance, which shows the fixture itself is sound."""
    _, _, targets = fixtures("h128_all")
    rep = _three_lane_case(pkg, targets, "three lanes, UMX_CREATE_U8_DEQUANT", u8_dequant=True)
    geo._finish(rep, "affine_u8_dequant")


@pytest.mark.parametrize("case", ["first_segment", "carried_state", "precise_activations"])
def test_three_lanes_only_whh_skewed(pkg, fixtures, case):
    """lstm_batch_kernel's u8-resident W_hh offset term on a sharp fixture: only W_hh skewed, so every other product is the plain one.
    The recurrence feeds its own offset term back (a second segment from the state of the first); FLAG_PRECISE_ACT has the same
    offset and other activations."""
    _, fams, targets = fixtures("h128_hh")
    assert fams == {"hh"}
    rep = _three_lane_case(pkg, targets, f"three lanes, h128_hh, {case}", carried=case == "carried_state",
                           flags=pkg.FLAG_PRECISE_ACT if case == "precise_activations" else 0)
    geo._finish(rep, f"affine_h128_hh_{case}")


@pytest.mark.parametrize("case", ["first_segment", "carried_state"])
def test_three_lanes_plane_gemms_on_the_skewed_model(pkg, fixtures, case):
    """gemm_planes_kernel on 128 x 128 tiles (fc1, W_ih: u8, one plane; fc2, fc3: u16, two planes) and lstm_batch_kernel on the fully
    skewed hidden-128 model, all four targets, lanes at 1, 30 and 1e-5 times the level.  With the centres 128 / 32896 fc1 of this
    case is dozens of times outside its bound (tests/test_affine_offset_cpu.py's emulation: 45 - 113)."""
    _, fams, targets = fixtures("h128_all")
    assert fams == sw.ALL
    rep = _three_lane_case(pkg, targets, f"three lanes, h128_all, {case}", carried=case == "carried_state")
    geo._finish(rep, f"affine_h128_all_{case}")


def test_ten_lanes_hidden_512_plane_gemms_on_the_skewed_model(pkg, fixtures):
    """The shape of the bitwise flavour test below: hidden 512, ten lanes, T = 45, the second of two segments.  W_ih and fc3 on
    gemm_planes_ps_kernel's 256 x 256 tiles, fc1 and fc2 on the 128 x 128 ones, lstm_batch8_kernel (K = 256); lanes 0, 1 (loud),
    2 (quiet) and 9, all four targets."""
    Hh, fams, targets = fixtures("h512_all")
    assert fams == sw.ALL
    rep = _lanes_case(pkg, targets, "ten lanes, h512_all", hidden=Hh, lanes=10, T=45, lstm_kernel="lstm_batch8_kernel", gemm_kernels=MIXED_TILES,
                      check_lanes=(0, 1, 2, 9), carried=True)
    geo._finish(rep, "affine_h512_all")


def test_nine_lanes_hidden_1024_plane_gemms_on_the_skewed_model(pkg, fixtures):
    """UMX-L's width, nine lanes (one octet and a lane), T = 41: W_ih (K = 1024) and fc3 on gemm_planes_ps_kernel, fc1 and fc2
    (K = 2048) on the 128 x 128 tiles, lstm_batch8_kernel at K = 512; lanes 0 and 8, targets 0 - 2."""
    Hh, fams, targets = fixtures("h1024_all")
    assert fams == sw.ALL
    rep = _lanes_case(pkg, targets, "nine lanes, h1024_all", hidden=Hh, lanes=9, T=41, lstm_kernel="lstm_batch8_kernel", gemm_kernels=MIXED_TILES,
                      check_lanes=(0, 8), which=range(3))
    geo._finish(rep, "affine_h1024_all")


# fixture, lanes, lanes checked, targets checked (targets 0 and 1 carry opposite variants in every chain), kernels of fc1 / W_ih / fc2 / fc3
BIG_TILES = ("gemm_planes_ps_kernel",) * 4  # 40 lanes: every GEMM has more 256 x 256 tiles than the chip has CUs
WHH_CASES = {"h512_ten_lanes": ("h512_hh", 10, (0, 1, 9), range(4), MIXED_TILES),
             "h1024_nine_lanes": ("h1024_hh", 9, (0, 8), (0, 1, 2), MIXED_TILES),
             "h1024_forty_lanes": ("h1024_hh", 40, (0, 8, 33, 39), (0, 1), BIG_TILES)}


@pytest.mark.parametrize("segment", ["first_segment", "carried_state"])
@pytest.mark.parametrize("case", sorted(WHH_CASES))
def test_batch8_recurrence_only_whh_skewed(pkg, fixtures, case, segment):
    """lstm_batch8_kernel's u8-resident W_hh offset term at its real K (256 at hidden 512, 512 at hidden 1024) on a sharp fixture:
    only W_hh skewed, so every other product is the plain one.  The kernel keeps the centre 128 for W_hh: |h| < 1 and the row sum
    comes out of the same accumulation as the products, so the fixed centre costs little here (the emulation: at most 0.31 of the
    bound) -- this test is what holds that.  Lane 1 at 30 times the level, lane 2 at 1e-5 of it, lane 33 (where present) at 30 times."""
    name, lanes, check_lanes, which, kernels = WHH_CASES[case]
    Hh, fams, targets = fixtures(name)
    assert fams == {"hh"}
    rep = _lanes_case(pkg, targets, f"{case}, {name}, {segment}", hidden=Hh, lanes=lanes, T=41, lstm_kernel="lstm_batch8_kernel",
                      gemm_kernels=kernels, check_lanes=check_lanes, which=which, carried=segment == "carried_state", loud=(1, 33))
    geo._finish(rep, f"affine_{name}_{lanes}_{segment}")


FLAVOURS = ((("UMX_GEMM_PP", "0"), "gemm_planes_kernel"), (("UMX_GEMM_PS", "0"), "gemm_planes_pp_kernel"), (None, "gemm_planes_ps_kernel"))


def test_plane_gemm_flavours_give_the_same_bits_on_the_skewed_model(pkg, fixtures, monkeypatch):
    """gemm_planes_kernel (lock step, UMX_GEMM_PP=0), gemm_planes_pp_kernel (UMX_GEMM_PS=0) and gemm_planes_ps_kernel (as shipped) on
    the fully skewed hidden-512 model, ten lanes, T = 45, two segments: stems, carried state and every stage tap agree bit for bit.
    W_ih (u8, one plane, the two directions' bs / bo2 / bsplit) and fc3 (u16, two planes) have enough 256 x 256 tiles at this size for
    the setting to select the kernel -- asserted by name per flavour; fc1 and fc2 stay on gemm_planes_kernel's 128 x 128 tiles (at
    hidden 128 every GEMM would, and the comparison would be one kernel against itself).  Kernel against kernel: it would fail if one
    flavour formed the offset term differently; test_ten_lanes_hidden_512_plane_gemms_on_the_skewed_model holds the shipped flavour
    of this very context to float64."""
    Hh, _, targets = fixtures("h512_all")
    B, N = 10, sf._N(45, 517)
    levels = [np.float32(1.0), LOUD, QUIET] + [np.float32(1.0)] * (B - 3)
    res = {}
    for env, kernel in FLAVOURS:
        monkeypatch.delenv("UMX_GEMM_PP", raising=False)
        monkeypatch.delenv("UMX_GEMM_PS", raising=False)
        if env:
            monkeypatch.setenv(*env)
        eng = pkg.Engine(targets, Hh, N, tracks=B)
        try:
            stems = [geo._run(pkg, eng, _waves(pkg, N, B, seed, levels), 0) for seed in (2100, 2200)]
            names = [eng.gemm_kernel_name(m) for m in range(4)]
            assert names[1] == names[3] == kernel and names[0] == names[2] == "gemm_planes_kernel", (env, names)
            taps = {(k, b, t): eng.tap(f"{k}#{b}", t) for k in STAGES for b in (0, 1, B - 1) for t in range(4)}
            res[kernel] = (stems, [_state(eng, b) for b in range(B)], taps)
        finally:
            eng.close()
    ref = res["gemm_planes_ps_kernel"]
    for kernel in ("gemm_planes_kernel", "gemm_planes_pp_kernel"):
        for key, v in ref[2].items():
            assert np.array_equal(res[kernel][2][key].view(np.uint32), v.view(np.uint32)), (kernel, key)
        for b in range(B):
            assert np.array_equal(res[kernel][1][b].view(np.uint32), ref[1][b].view(np.uint32)), (kernel, b)
            for s in range(2):
                for t in range(4):
                    assert np.array_equal(res[kernel][0][s][b][t].view(np.uint32), ref[0][s][b][t].view(np.uint32)), (kernel, s, b, t)
