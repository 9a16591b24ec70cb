"""The fp32-resident family of the engine against float64 (tests/stage_f64.py) at the widths people run, on raw float32 weights
(tests/fp32_weights.py).  An engine takes this family when it is handed float32 tensors, told to dequantise at load
(UMX_CREATE_DEQUANTISE_AT_LOAD, UMX_CREATE_U8_DEQUANT), or when any one target brings a matrix as float32 (csrc/engine_init.h
load_weight and the whh_all_u8 block).  It runs other code than the default: the plane GEMMs on two fp16 planes of w 2^e under one
power-of-two scale per source tensor (form 2: the NBP = 2 instantiations for fc1 and W_ih, which the default runs at NBP = 1, and two
scales across bsplit for W_ih's directions), lstm_batch_kernel<HL, WQ = false> also at hidden 512 and 1024 (three bf16 planes of W_hh
and of h, no fused planes or row sums: split_planes_kernel<2> splits la, lb and the concat's right half, fc2 takes rs0 + rs1), and in
the one-track context gemm_bf16x3_kernel<MODE, BQ_F32> with lstm_persistent_kernel / lstm_step_kernel reading fp32 W_hh.

Every stage's reference comes from the engine's own tap of that stage's input (test_gpu_geometry_f64.check_network), every case
asserts GEMM and LSTM kernels by name, and no bound of stage_f64 is changed.  Cases a - d hand bare float32 arrays with
quantised=False; e keeps the file's quantised records beside two float32 arrays (quantised=True leaves a record as it is and a bare
array float32), and f compares the two ways into the family.  Lane 1 plays at 30 times the level and lane 2 at 1e-5 of it
(test_gpu_affine_offset: they drive the adaptive row scale of xs and a2).

  a. ten lanes, hidden 512, T = 45, the second of two calls, `plain` and `wide`: fc1 and fc2 on gemm_planes_kernel's 128 x 128 tiles,
     W_ih and fc3 on gemm_planes_ps_kernel, lstm_batch_kernel; lanes 0, 1, 2, 9, all four targets.  On `wide` target 3's fc3.weight is
     zero (the scale keeps its default): its mask is one constant row, held to its own reference.
  b. nine lanes, hidden 1024, T = 41, first call, `plain`: K = 1024 for W_ih and fc3, 2048 for fc2, lstm_batch_kernel at HL = 512;
     lanes 0 and 8, targets 0 - 2.
  c. forty lanes, hidden 512, T = 45, carried state, `wide`: every GEMM has more 256 x 256 tiles than CUs -- gemm_planes_ps_kernel four
     times, derived from the rule of csrc/engine_stages.h and the device's CU count --, three groups of lstm_batch_kernel; lanes 0, 17
     and 39, targets 0 and 1.  Then the same two calls under UMX_GEMM_PS=0 (gemm_planes_pp_kernel) and UMX_GEMM_PP=0
     (gemm_planes_kernel): stems, state and taps of those lanes bit for bit, which ties the NBP = 2 instantiations of all three
     kernels for fc1 and W_ih to the one held to float64.
  d. one track, default context, hidden 512 (`plain`, `wide`) and 1024 (`plain`), T = 41, second of two calls: gemm_bf16x3_kernel
     four times, lstm_persistent_kernel; at hidden 512 also against FLAG_LSTM_STEPWISE bit for bit.
  e. `mixed`, hidden 128, three lanes, T = 41: W_hh and fc2 expanded for all targets, fc1 / W_ih / fc3 integer; every stage of every
     target against float64 of that target's own dequantised weights; weight_bytes() strictly between the all-integer and the
     all-fp32 context's.
  f. hidden 128, three lanes: Engine(file tensors, quantised_resident=False) and Engine(dequantised arrays, quantised=False) agree
     bit for bit in stems, state and taps of two calls.

tests/test_fp32_weights_cpu.py shows on a numpy emulation of form 2 (tests/planes_f32_emu.py) that this check fails a dropped low
weight plane and a scale of the wrong direction, and records the ratios the correct emulation reaches.

Measured on an MI355X (profiles/fp32_weights_f64_report.jsonl: 470 checks, none failed, the largest 0.72 of its bound), worst ratio
to the float32 evaluation over the whole segment / in the worst frame, per case:
  a. plain  fc1 2.7 / 2.8, lstm 0.9 / 0.9, fc2 1.7 / 1.9, mask 1.4 / 1.4;   wide  fc1 2.7 / 2.8, lstm 0.9 / 0.9, fc2 1.6 / 1.8,
     mask 1.4 / 1.4, the constant mask of target 3 1.0 / 1.0;
  b. fc1 2.6 / 2.6, lstm 0.7 / 0.8, fc2 (K = 2048) 2.3 / 2.4, mask 1.4 / 1.5;
  c. fc1 2.5 / 2.6, lstm 0.9 / 0.9, fc2 1.6 / 1.7, mask 1.2 / 1.2; the three flavours agree bit for bit;
  d. hidden 512 plain and wide alike  fc1 3.5 / 3.5 (0.72 of the bound: the six-term form over K = 2974; the u8 one-plane form of the
     default context measures 2.3), lstm 1.0 / 1.1, fc2 2.1 / 2.3, mask 1.4 / 1.4;   hidden 1024  fc1 3.4 / 3.3, lstm 1.0 / 1.0,
     fc2 2.8 / 3.1 (0.61 of the bound), mask 1.7 / 1.8;
  e. fc1 2.2 / 2.3, lstm 1.3 / 1.4, fc2 1.1 / 1.1, mask 1.0 / 1.1; weight bytes 14,450,688 < 15,630,336 < 20,250,624;
  target_mag 1.0 / 1.0 everywhere.
The emulation of form 2 (hidden 512, T = 24, every lane at the plain level) reaches fc1 2.2 / 2.2 and lstm 0.8 / 0.9 on `plain` and fc1
2.2 / 2.2, lstm 0.7 / 0.7 on `wide` (its recurrence is float64; other audio and T than here).  The kernels' fc1 on the lanes at the
plain level is 2.5 - 2.8 (lane 1, 30 times as loud: 1.6; lane 2, at 1e-5: 2.2): a quarter above the emulation's and 0.58 of the
bound, where a dropped low weight plane is 430 - 580 times the float32 evaluation's distance and a scale of the wrong direction
3e5 - 4e6 times.

UMX_STAGE_F64_REPORT=<file>: append every check's distances to that file (JSON lines), as tests/test_gpu_geometry_f64.py does."""
import numpy as np
import pytest

import fp32_weights as fw
import stage_f64 as sf
import test_gpu_affine_offset as aff
import test_gpu_geometry_f64 as geo
import test_gpu_one_track_f64 as ot

pytestmark = pytest.mark.gpu

SEED = 81
BATCH = "lstm_batch_kernel"
PLAIN, PP, PS = "gemm_planes_kernel", "gemm_planes_pp_kernel", "gemm_planes_ps_kernel"
KX, NOUT_PAD, GP_BK = 2976, 4352, 32  # csrc/common.h, csrc/gemm_planes.h


@pytest.fixture(scope="module")
def n_cus():
    import torch
    torch.zeros(1).cuda()  # a current device
    cus = sf.device_cu_count(0)
    assert cus == torch.cuda.get_device_properties(0).multi_processor_count
    return cus


@pytest.fixture(scope="module")
def weights(pkg):
    """(kind, hidden) -> four targets of bare float32 arrays; each drawn once."""
    made = {}

    def get(kind, H):
        if (kind, H) not in made:
            made[kind, H] = getattr(fw, kind)(pkg.ggml, H, SEED)
        return made[kind, H]
    return get


def plane_gemm_kernels(H, lanes, T, cus, nact=4, gemm_pp=-1, gemm_ps=-1):
    """csrc/engine_stages.h launch_gemm_planes: the kernel of fc1, W_ih, fc2, fc3 when all `lanes` lanes form one launch.
    gemm_pp / gemm_ps: UMX_GEMM_PP / UMX_GEMM_PS (-1: unset; else a bit per stage)."""
    Tp = max(T, 256)
    M = -(-lanes * Tp // 256) * 256
    names = []
    for mode, (N, K) in enumerate(((H, KX), (4 * H, H), (H, 2 * H), (NOUT_PAD, H))):
        blocks_big = (N // 256) * (M // 256) * nact
        big = N % 256 == 0 and blocks_big >= 224
        pp = big and (gemm_pp < 0 or bool((gemm_pp >> mode) & 1))
        ps_wgs = cus // 8 * 8
        ps = pp and (gemm_ps < 0 or bool((gemm_ps >> mode) & 1)) and K // GP_BK >= 6 and ps_wgs >= 8 and blocks_big > ps_wgs and Tp >= 256
        names.append(PS if ps else PP if pp else PLAIN)
    return tuple(names)


def _levels(lanes, loud=(1, 33), quiet=(2,)):
    return [aff.LOUD if b in loud else aff.QUIET if b in quiet else np.float32(1.0) for b in range(lanes)]


def _lanes_run(pkg, eng, N, lanes, carried):
    """One call, or two with the second from the state the first left.  -> (stems of each call, the state of every lane before the
    last call)."""
    levels = _levels(lanes)
    states = [aff._zero_state(eng)] * lanes
    stems = []
    if carried:
        stems.append(geo._run(pkg, eng, aff._waves(pkg, N, lanes, 4100, levels), 0))
        states = [aff._state(eng, b) for b in range(lanes)]
    stems.append(geo._run(pkg, eng, aff._waves(pkg, N, lanes, 4200, levels), 0))
    return stems, states


def _assert_kernels(eng, gemms, lstm):
    names = tuple(eng.gemm_kernel_name(m) for m in range(4))
    assert names == tuple(gemms), names
    assert eng.lstm_kernel_name() == lstm, eng.lstm_kernel_name()


def _check_finite_and_zero_target(rep, eng, lane, wt, where, which):
    """`wide`: every stage tap finite; the mask of the target with the zero fc3.weight is one constant row, held to the constant
    reference relu(bn3(0) x output_scale + output_mean) by the same check as every stage."""
    sfx = geo._sfx(eng, lane)
    for t in which:
        for k in ("fc1", "lstm", "fc2", "mask", "target_mag"):
            rep.exact(f"{k}[{t}]", bool(np.isfinite(eng.tap(k + sfx, t)).all()), f"[{where}, lane {lane}]", "non-finite values")
    if fw.ZERO_TARGET in which:
        mk = eng.tap("mask" + sfx, fw.ZERO_TARGET)
        T = mk.shape[0]
        rep.exact("mask[3]", bool((mk.view(np.uint32) == mk.view(np.uint32)[0]).all()), f"[{where}, lane {lane}]",
                  "a zero fc3.weight: the rows of the mask are not one constant row")
        rep.add(sf.check("mask[3] constant", mk, fw.zero_mask_reference(wt[fw.ZERO_TARGET], T, "float64"),
                         fw.zero_mask_reference(wt[fw.ZERO_TARGET], T, "float32"), "rows", where=f"[{where}, lane {lane}]", T=T))


def _worst(rep):
    rows = [r for r in rep.rows if "ratio_rel" in r]
    by = {}
    for r in rows:
        k = r["stage"].split("[")[0]
        by[k] = (max(by.get(k, (0, 0, 0))[0], r["ratio_rel"]), max(by.get(k, (0, 0, 0))[1], r["ratio_blk"]), max(by.get(k, (0, 0, 0))[2], r["excess"]))
    return ", ".join(f"{k} {a:.1f} / {b:.1f} ({c:.2f} of the bound)" for k, (a, b, c) in by.items())


def _lanes_case(pkg, n_cus, targets, test, *, hidden, lanes, T, check_lanes, which, carried, zero_target=False):
    N = sf._N(T, 517)
    rep = sf.Report()
    eng = pkg.Engine(targets, hidden, N, tracks=lanes, quantised=False)
    try:
        _, states = _lanes_run(pkg, eng, N, lanes, carried)
        assert not carried or all(np.abs(states[b]).max() > 0 for b in check_lanes)
        _assert_kernels(eng, plane_gemm_kernels(hidden, lanes, T, n_cus), BATCH)
        for b in check_lanes:
            geo.check_network(rep, eng, b, targets, states[b], test, which=which)
            if zero_target:
                _check_finite_and_zero_target(rep, eng, b, targets, test, which)
        print(f"{test}: worst ratio to the float32 evaluation, whole segment / worst frame: {_worst(rep)}")
    finally:
        eng.close()
    geo._finish(rep, test)


# ---------------------------------------------------------------- a. ten lanes, hidden 512
@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_ten_lanes_hidden_512(pkg, weights, n_cus, kind):
    assert plane_gemm_kernels(512, 10, 45, n_cus) == (PLAIN, PS, PLAIN, PS)
    _lanes_case(pkg, n_cus, weights(kind, 512), f"fp32_ten_lanes_h512_{kind}", hidden=512, lanes=10, T=45, check_lanes=(0, 1, 2, 9),
                which=range(4), carried=True, zero_target=kind == "wide")


# ---------------------------------------------------------------- b. nine lanes, hidden 1024
def test_nine_lanes_hidden_1024(pkg, weights, n_cus):
    assert plane_gemm_kernels(1024, 9, 41, n_cus) == (PLAIN, PS, PLAIN, PS)
    _lanes_case(pkg, n_cus, weights("plain", 1024), "fp32_nine_lanes_h1024_plain", hidden=1024, lanes=9, T=41, check_lanes=(0, 8),
                which=range(3), carried=False)


# ---------------------------------------------------------------- c. forty lanes, hidden 512: the 256 x 256 tiles, three flavours
FORTY = dict(hidden=512, lanes=40, T=45)
FORTY_LANES = (0, 17, 39)


def test_forty_lanes_hidden_512_every_gemm_persistent(pkg, weights, n_cus):
    assert plane_gemm_kernels(512, 40, 45, n_cus) == (PS,) * 4, (n_cus, plane_gemm_kernels(512, 40, 45, n_cus))
    assert -(-40 // 16) == 3  # lstm_batch_kernel runs groups of 16 lanes, one after the other
    _lanes_case(pkg, n_cus, weights("wide", 512), "fp32_forty_lanes_h512_wide", check_lanes=FORTY_LANES, which=(0, 1), carried=True,
                zero_target=True, **FORTY)


FLAVOURS = ((None, -1, -1), (("UMX_GEMM_PS", "0"), -1, 0), (("UMX_GEMM_PP", "0"), 0, -1))


def test_forty_lanes_plane_gemm_flavours_give_the_same_bits(pkg, weights, n_cus, monkeypatch):
    """gemm_planes_ps_kernel (as shipped), gemm_planes_pp_kernel (UMX_GEMM_PS=0) and gemm_planes_kernel on 256 x 256 tiles
    (UMX_GEMM_PP=0), all four GEMMs at NBP = 2: kernel against kernel, the shipped one held to float64 by the test above."""
    targets, N, B = weights("wide", 512), sf._N(45, 517), 40
    res = {}
    for env, gemm_pp, gemm_ps in FLAVOURS:
        monkeypatch.delenv("UMX_GEMM_PP", raising=False)
        monkeypatch.delenv("UMX_GEMM_PS", raising=False)
        if env:
            monkeypatch.setenv(*env)
        want = plane_gemm_kernels(512, B, 45, n_cus, gemm_pp=gemm_pp, gemm_ps=gemm_ps)
        assert want == ((PS,) * 4 if env is None else (PP,) * 4 if env[0] == "UMX_GEMM_PS" else (PLAIN,) * 4), (env, want)
        eng = pkg.Engine(targets, 512, N, tracks=B, quantised=False)
        try:
            stems, _ = _lanes_run(pkg, eng, N, B, carried=True)
            _assert_kernels(eng, want, BATCH)
            taps = {(k, b, t): eng.tap(f"{k}#{b}", t) for k in aff.STAGES for b in FORTY_LANES for t in range(4)}
            res[want[0]] = ([[s[b] for b in FORTY_LANES] for s in stems], [aff._state(eng, b) for b in FORTY_LANES], taps)
        finally:
            eng.close()
    ref = res[PS]
    for kernel in (PP, PLAIN):
        for key, v in ref[2].items():
            assert np.array_equal(res[kernel][2][key].view(np.uint32), v.view(np.uint32)), (kernel, key)
        for i, b in enumerate(FORTY_LANES):
            assert np.array_equal(res[kernel][1][i].view(np.uint32), ref[1][i].view(np.uint32)), (kernel, "state", b)
            for s in range(2):
                for t in range(4):
                    assert np.array_equal(res[kernel][0][s][i][t].view(np.uint32), ref[0][s][i][t].view(np.uint32)), (kernel, s, b, t)


# ---------------------------------------------------------------- d. one track, default context
@pytest.mark.parametrize("kind,H,which", [("plain", 512, (0, 1, 2, 3)), ("wide", 512, (0, 1, 2, 3)), ("plain", 1024, (0, 3))],
                         ids=["plain_h512", "wide_h512", "plain_h1024"])
def test_one_track_default_context(pkg, weights, kind, H, which):
    targets, N = weights(kind, H), sf._N(41, 517)
    test = f"fp32_one_track_h{H}_{kind}"
    rep = sf.Report()
    res = {}
    eng = pkg.Engine(targets, H, N, tracks=1, quantised=False)
    try:
        for name, flags in (("persistent", 0), ("stepwise", pkg.FLAG_LSTM_STEPWISE)) if H == 512 else (("persistent", 0),):
            eng.stream_reset()
            stems, states = [], []
            for s in (0, 1):
                stems.append(geo._run(pkg, eng, [geo._audio(pkg, N - 11 * s, 4300 + 10 * s)], flags)[0])
                states.append(eng.stream_get())
            ot.assert_one_track_kernels(eng, persistent=name == "persistent")
            assert np.abs(states[0]).max() > 0
            res[name] = (stems, states, [eng.tap("lstm", t) for t in range(4)])
            if name == "persistent":
                geo.check_network(rep, eng, 0, targets, states[0], test, which=which)
                if kind == "wide":
                    _check_finite_and_zero_target(rep, eng, 0, targets, test, which)
        print(f"{test}: worst ratio to the float32 evaluation, whole segment / worst frame: {_worst(rep)}")
    finally:
        eng.close()
    if "stepwise" in res:
        (sp, tp, lp), (ss, ts, ls) = res["persistent"], res["stepwise"]
        for call in (0, 1):
            assert ot._bits_equal(tp[call], ts[call]), f"state after call {call}"
            for t in range(4):
                assert ot._bits_equal(sp[call][t], ss[call][t]), f"stems of call {call}, target {t}"
        for t in range(4):
            assert ot._bits_equal(lp[t], ls[t]), f"lstm tap, target {t}"
    geo._finish(rep, test)


# ---------------------------------------------------------------- e. both families in one context
def test_mixed_weight_forms_three_lanes(pkg, model_small):
    """Target 1 brings lstm.weight_hh_l1 and fc2.weight as float32: W_hh (all layers: the recurrences take one form) and fc2 are
    expanded for all four targets, fc1, W_ih and fc3 keep their integer planes."""
    _, _, file_targets = model_small
    targets, N, B = fw.mixed(file_targets), sf._N(41, 517), 3
    rep = sf.Report()
    sizes = {}
    for name, tg, q in (("integer", file_targets, True), ("fp32", fw.dequantised(file_targets), False)):
        e = pkg.Engine(tg, 128, N, tracks=B, quantised=q)
        sizes[name] = e.weight_bytes()
        e.close()
    eng = pkg.Engine(targets, 128, N, tracks=B)  # quantised=True: a record stays integer, a bare array is float32
    try:
        sizes["mixed"] = eng.weight_bytes()
        _, states = _lanes_run(pkg, eng, N, B, carried=True)
        _assert_kernels(eng, (PLAIN,) * 4, BATCH)
        for b in range(B):
            geo.check_network(rep, eng, b, targets, states[b], "fp32_mixed_h128")
        print(f"fp32_mixed_h128: weight bytes {sizes}; worst ratio to the float32 evaluation: {_worst(rep)}")
    finally:
        eng.close()
    assert sizes["integer"] < sizes["mixed"] < sizes["fp32"], sizes
    geo._finish(rep, "fp32_mixed_h128")


# ---------------------------------------------------------------- f. two ways into the family, one engine
def test_float32_arrays_and_dequantise_at_load_are_the_same_engine(pkg, model_small):
    _, _, file_targets = model_small
    N, B = sf._N(41, 517), 3
    res = []
    for tg, kw in ((file_targets, dict(quantised_resident=False)), (fw.dequantised(file_targets), dict(quantised=False))):
        eng = pkg.Engine(tg, 128, N, tracks=B, **kw)
        try:
            stems, _ = _lanes_run(pkg, eng, N, B, carried=True)
            _assert_kernels(eng, (PLAIN,) * 4, BATCH)
            taps = {(k, b, t): eng.tap(f"{k}#{b}", t) for k in aff.STAGES + ("target_mag",) for b in range(B) for t in range(4)}
            res.append((stems, [aff._state(eng, b) for b in range(B)], taps, eng.weight_bytes()))
        finally:
            eng.close()
    a, b = res
    assert a[3] == b[3]
    for key, v in a[2].items():
        assert ot._bits_equal(v, b[2][key]), key
    for ln in range(B):
        assert ot._bits_equal(a[1][ln], b[1][ln]), ("state", ln)
        for s in range(2):
            for t in range(4):
                assert ot._bits_equal(a[0][s][ln][t], b[0][s][ln][t]), (s, ln, t)
