"""Every stage of the engine against float64 (tests/stage_f64.py) at the segment geometries where the kernels' tiles have edges: STFT
runs of 4 frames, fused Wiener / inverse-STFT runs (last runs of 1 and 2 frames, at one and three active lanes), 200-frame R batches,
the smallest and largest segments, ragged lanes, lane subsets that change the run split, edge inputs, the network stages at odd
lengths and lane counts, and the 32-bit address limit of the plane GEMMs.  Each stage's reference is computed from the engine's own
tap of that stage's input; a stage passes when it is at most C_DEFAULT times as far from float64 as a float32 evaluation of the same
formula, over the whole segment and in its worst frame / hop block.

UMX_STAGE_F64_REPORT=<file>: append every check's distances to that file (JSON lines)."""
import json
import os

import numpy as np
import pytest

import stage_f64 as sf

pytestmark = pytest.mark.gpu

H = 128
# bins of the filter's float64 reference on long segments (the filter is per bin; max_abs is still taken over all of them): the
# edges of the spectrum and of the network's crop, and every 17th bin
BIG_T, BIG_T_BINS = 1000, np.unique(np.r_[0:4, 1023:1026, 1484:1490, 2044:2049, np.arange(0, 2049, 17)])


@pytest.fixture(scope="module")
def n_cus():
    import torch
    torch.zeros(1).cuda()  # a current device for the debug entry points
    cus = sf.device_cu_count(0)
    assert cus == torch.cuda.get_device_properties(0).multi_processor_count
    return cus


@pytest.fixture(scope="module")
def geo(n_cus):
    return sf.geometries(n_cus)


def _finish(rep, test):
    path = os.environ.get("UMX_STAGE_F64_REPORT")
    if path:
        with open(path, "a") as f:
            for r in rep.rows:
                f.write(json.dumps({"test": test, **{k: (float(v) if isinstance(v, (np.floating, np.integer)) else v)
                                                       for k, v in r.items()}}) + "\n")
    rep.assert_ok()


def _sfx(eng, lane):
    return "" if eng.tracks == 1 else f"#{lane}"


def check_front_back(rep, eng, lane, wave, stems, no_wiener, where, run_len=None, n_iter=1):
    """spec, mix_mag, x (bits of the crop of mix_mag), max_abs (1 ulp), y and the stems of one lane of the last call."""
    sfx, N, n = _sfx(eng, lane), eng.N, wave.shape[1]
    T = sf.n_frames(N)
    where = f"[{where}, lane {lane}, N={N}, n={n}, T={T}]"
    spec = eng.tap("spec" + sfx)
    rep.add(sf.check("spec", spec, sf.stft(wave, N, "float64"), sf.stft(wave, N, "float32"), "spectrum", where=where, T=T))
    mm = eng.tap("mix_mag" + sfx)
    rep.add(sf.check("mix_mag", mm, sf.magnitude(spec, "float64"), sf.magnitude(spec, "float32"), "spectrum", where=where, T=T))
    x = eng.tap("x" + sfx)
    rep.exact("x", np.array_equal(x[:, :2 * sf.CROP], sf.crop_x(mm)), where, "not bitwise the crop of mix_mag")
    if not no_wiener:
        got, want = eng.tap("max_abs" + sfx)[0], sf.max_abs(spec)
        rep.exact("max_abs", abs(float(got) - float(want)) <= float(np.spacing(want)), where, f"{got!r} against {want!r}")
    mags = [eng.tap("target_mag" + sfx, t) for t in range(4)]
    y = [eng.tap("y" + sfx, t) for t in range(4)]
    bins = BIG_T_BINS if T > BIG_T else None
    if no_wiener:
        y64, y32 = sf.mixture_phase(spec, mags, "float64", bins), sf.mixture_phase(spec, mags, "float32", bins)
    else:
        y64, y32 = sf.wiener(spec, mags, n_iter, "float64", bins), sf.wiener(spec, mags, n_iter, "float32", bins)
    del mags
    for t in range(4):
        rep.add(sf.check(f"y[{t}]", y[t] if bins is None else y[t][:, :, bins], y64[t], y32[t], "spectrum", where=where, T=T,
                         run_len=run_len))
    del y64, y32
    for t in range(4):
        rep.add(sf.check(f"stems[{t}]", stems[t], sf.istft(y[t], n, N, "float64"), sf.istft(y[t], n, N, "float32"), "stems",
                         where=where, T=T, run_len=run_len))
    del y


def check_network(rep, eng, lane, targets, state_before, where, which=range(4)):
    """fc1, lstm, fc2, mask, target_mag of one lane of the last call, each from the engine's taps of its inputs."""
    sfx, Hh = _sfx(eng, lane), eng.hidden
    T = sf.n_frames(eng.N)
    where = f"[{where}, lane {lane}, hidden {Hh}, T={T}]"
    x = eng.tap("x" + sfx)[:, :2 * sf.CROP]
    mm = eng.tap("mix_mag" + sfx)
    for t in which:
        wt = sf.target_weights(targets[t])
        st = state_before[t * 12 * (Hh // 2):(t + 1) * 12 * (Hh // 2)]
        a1, lo, a2, mk = (eng.tap(k + sfx, t) for k in ("fc1", "lstm", "fc2", "mask"))
        for name, got, f in (("fc1", a1, lambda p: sf.fc1(wt, x, p)),
                             ("lstm", lo, lambda p: sf.lstm(wt, Hh, a1, st, p)),
                             ("fc2", a2, lambda p: sf.fc2(wt, a1, lo, p)),
                             ("mask", mk, lambda p: sf.mask(wt, a2, p))):
            rep.add(sf.check(f"{name}[{t}]", got, f("float64"), f("float32"), "rows", where=where, T=T))
        rep.add(sf.check(f"target_mag[{t}]", eng.tap("target_mag" + sfx, t), sf.target_mag(mk, mm, "float64"),
                         sf.target_mag(mk, mm, "float32"), "spectrum", where=where, T=T))


def _run(pkg, eng, waves, flags):
    """One call; waves: list per lane (None = idle).  -> stems per lane."""
    flags |= pkg.FLAG_DEBUG_TAPS
    if eng.tracks == 1:
        return [eng.infer_segment(waves[0], flags)]
    return eng.infer_batch(waves, flags)


def _audio(pkg, n, seed):
    return pkg.ggml.synth_audio(n, seed)


@pytest.mark.parametrize("tracks", [1, 3], ids=["single_track_unfused", "three_lanes_fused"])
def test_front_and_back_end_sweep(pkg, model_small, geo, n_cus, tracks):
    """spec, max_abs, x, y and stems over every geometry case (T = 4095 at three lanes: test_ragged_lanes_and_lane_subsets), with
    FLAG_NO_WIENER at a few of them."""
    _, _, targets = model_small
    rep = sf.Report()
    no_wiener_at = {"T%4=2,N%1024=1023", "last_fused_run=1@1", "N=4096", "T=201"}
    for case, N in geo.items():
        if tracks == 3 and case == "T=4095":
            continue
        eng = pkg.Engine(targets, H, N, tracks=tracks)
        try:
            lanes = 1 if (tracks == 1 or case.endswith("@1")) else 3
            for flags in (0, pkg.FLAG_NO_WIENER) if case in no_wiener_at else (0,):
                waves = [_audio(pkg, N - 37 * b, 100 + b) for b in range(lanes)]
                if tracks == 3 and lanes == 1:
                    waves = [None, waves[0], None]  # one active lane, not lane 0
                stems = _run(pkg, eng, waves, flags)
                T = sf.n_frames(N)
                run_len = sf.fused_run_split(T, lanes, n_cus)[0] if tracks > 1 else None
                for b, w in enumerate(waves):
                    if w is not None:
                        check_front_back(rep, eng, b, w, stems[b], flags == pkg.FLAG_NO_WIENER, f"{case}, flags {flags:#x}", run_len)
        finally:
            eng.close()
    _finish(rep, f"sweep_{tracks}")


def test_wiener_iterations_last_filter_from_v(pkg, model_small, geo, n_cus):
    """FLAG_WIENER_ITERS(2) in a fused context (the last filter is wiener_istft_v_kernel) at T = 73 (last run of one frame at 256 CUs)
    and T = 4095."""
    _, _, targets = model_small
    rep = sf.Report()
    for case in ("last_fused_run=1@1", "T=4095"):
        N = geo[case]
        eng = pkg.Engine(targets, H, N, tracks=3)
        try:
            waves = [_audio(pkg, N, 300), None, None]
            stems = _run(pkg, eng, waves, pkg.FLAG_WIENER_ITERS(2))
            check_front_back(rep, eng, 0, waves[0], stems[0], False, f"{case}, 2 EM iterations",
                             sf.fused_run_split(sf.n_frames(N), 1, n_cus)[0], n_iter=2)
        finally:
            eng.close()
    _finish(rep, "wiener_iters")


def test_ragged_lanes_and_lane_subsets(pkg, model_small, n_cus):
    """T = 4095, three lanes: n = N, N - 1023, 2049 (less than half a window); then a call with lane 1 absent (two active lanes: a
    different run split) and n = 1 on lane 0.  And a 48-lane context at T = 201 whose split differs from the one-lane split."""
    _, _, targets = model_small
    rep = sf.Report()
    N = sf.N_MAX
    T = sf.n_frames(N)
    assert sf.fused_run_split(T, 3, n_cus) != sf.fused_run_split(T, 2, n_cus)
    eng = pkg.Engine(targets, H, N, tracks=3)
    try:
        for call, ns in enumerate(((N, N - 1023, 2049), (1, None, N - 5))):
            waves = [None if n is None else _audio(pkg, n, 400 + 10 * call + b) for b, n in enumerate(ns)]
            stems = _run(pkg, eng, waves, 0)
            lanes = sum(w is not None for w in waves)
            for b, w in enumerate(waves):
                if w is not None:
                    check_front_back(rep, eng, b, w, stems[b], False, f"ragged call {call}", sf.fused_run_split(T, lanes, n_cus)[0])
    finally:
        eng.close()
    N = sf._N(201, 77)
    T = sf.n_frames(N)
    assert sf.fused_run_split(T, 48, n_cus) != sf.fused_run_split(T, 1, n_cus)
    eng = pkg.Engine(targets, H, N, tracks=48)
    try:
        waves = [_audio(pkg, N - 3 * b, 500 + b) for b in range(48)]
        stems = _run(pkg, eng, waves, 0)
        for b in (0, 47):
            check_front_back(rep, eng, b, waves[b], stems[b], False, "48 lanes", sf.fused_run_split(T, 48, n_cus)[0])
    finally:
        eng.close()
    _finish(rep, "ragged")


def _edge_inputs(pkg, n):
    """name -> (2, n) float32."""
    k = np.arange(n)
    base = _audio(pkg, n, 600)
    dc_nyq = (0.2 * base + np.array([[0.25], [-0.4]]) + 0.2 * np.where(k % 2 == 0, 1.0, -1.0)).astype(np.float32)
    click = (1e-3 * base).astype(np.float32)
    click[:, -1] = 1.0  # full scale in the last sample: max |X| in the last run
    quiet = (1e-5 * _audio(pkg, n, 601)).astype(np.float32)
    mono = np.repeat(_audio(pkg, n, 602)[:1], 2, axis=0)  # R == L exactly, as umx-cli gives a mono file
    assert np.array_equal(mono[0], mono[1])
    return {"dc_offsets_nyquist_tone": dc_nyq, "click_in_last_sample": click, "zero": np.zeros((2, n), np.float32),
            "gain_1e-5": quiet, "mono": mono}


@pytest.mark.parametrize("tracks", [1, 3], ids=["single_track_unfused", "three_lanes_fused"])
def test_edge_inputs(pkg, model_small, geo, n_cus, tracks):
    """DC offsets and a Nyquist tone, a click in the last sample, a zero lane beside loud ones, 1e-5 gain and mono (R == L) at a last
    fused run of one frame and at a partial last STFT run (T % 4 = 2, N % 1024 = 1023)."""
    _, _, targets = model_small
    rep = sf.Report()
    for case in ("last_fused_run=1@3", "T%4=2,N%1024=1023"):
        N = geo[case]
        T = sf.n_frames(N)
        ins = _edge_inputs(pkg, N)
        names = list(ins)
        eng = pkg.Engine(targets, H, N, tracks=tracks)
        try:
            if tracks == 1:
                calls = [[nm] for nm in names]
            else:
                calls = [names[:3], names[3:] + [None]]  # the zero lane beside loud ones
            for call in calls:
                waves = [None if nm is None else ins[nm] for nm in call]
                stems = _run(pkg, eng, waves, 0)
                lanes = sum(w is not None for w in waves)
                run_len = sf.fused_run_split(T, lanes, n_cus)[0] if tracks > 1 else None
                for b, nm in enumerate(call):
                    if nm is not None:
                        check_front_back(rep, eng, b, waves[b], stems[b], False, f"{nm}, {case}", run_len)
                        if nm == "click_in_last_sample":
                            spec = np.abs(eng.tap("spec" + _sfx(eng, b)))
                            assert spec.max(axis=(0, 2)).argmax() >= T - 3
        finally:
            eng.close()
    _finish(rep, f"edge_{tracks}")


@pytest.mark.parametrize("tracks", [1, 3], ids=["single_track", "three_lanes"])
def test_network_stages_at_odd_geometries(pkg, model_small, geo, tracks):
    """fc1, lstm, fc2, mask, target_mag at hidden 128, two odd lengths, on the second call (a carried LSTM state)."""
    _, _, targets = model_small
    rep = sf.Report()
    for case in ("T%4=3,N%1024=other", "last_fused_run=2@3"):
        N = geo[case]
        eng = pkg.Engine(targets, H, N, tracks=tracks)
        try:
            lanes = range(tracks)
            _run(pkg, eng, [_audio(pkg, N - 5 * b, 700 + b) for b in lanes], 0)
            states = [eng.stream_get() if tracks == 1 else eng.track_stream_get(b) for b in lanes]
            assert all(np.abs(s).max() > 0 for s in states)
            _run(pkg, eng, [_audio(pkg, N - 11 * b, 710 + b) for b in lanes], 0)
            for b in (0, tracks - 1):
                check_network(rep, eng, b, targets, states[b], case)
        finally:
            eng.close()
    _finish(rep, f"network_{tracks}")


def test_network_stages_hidden_512_nine_lanes(pkg, tmp_path):
    """hidden 512, 9 lanes, T = 915: two octets and one lane of lstm_batch8_kernel, 8235 rows ragged against the 256-row tiles, enough
    tiles for the persistent plane GEMM.  Lanes 0 and 8, targets 0 and 3."""
    Hh, B, N = 512, 9, sf._N(915, 301)
    path = str(tmp_path / "m512.bin")
    pkg.ggml.write_model(path, pkg.ggml.synth_weights(Hh, seed=81), Hh, compress=False)
    _, targets = pkg.ggml.read_model(path)
    rep = sf.Report()
    eng = pkg.Engine(targets, Hh, N, tracks=B)
    try:
        waves = [_audio(pkg, N - 13 * b, 800 + b) for b in range(B)]
        _run(pkg, eng, waves, 0)
        assert eng.lstm_kernel_name() == "lstm_batch8_kernel"
        assert eng.gemm_kernel_name(1) == "gemm_planes_ps_kernel"
        assert B * sf.n_frames(N) == 8235 and 8235 % 256
        for b in (0, 8):
            check_network(rep, eng, b, targets, np.zeros(eng.lib.umx_hip_stream_floats(eng.h), np.float32), "9 lanes", which=(0, 3))
    finally:
        eng.close()
    _finish(rep, "network_512")


def test_plane_gemm_address_limit(pkg, model_small, n_cus):
    """hidden 128, 64 lanes: the largest N the 32-bit guard of the plane GEMMs accepts runs correctly in lanes 0 and 63, every stage;
    N + 1024 is refused.  Every lane has audio, so each plane GEMM is ONE launch over all 64 lanes with its buffer resources based at
    lane 0 (engine_stages.h launch_gemm_lanes: one launch per run of consecutive active lanes): lane 63's rows of the second plane
    are then within 0.1% of 2^31 bytes from that base.  Lanes 1 .. 62 carry short audio (the GEMMs' M is lanes x Tp whatever n is)."""
    _, _, targets = model_small
    T = sf.plane_gemm_max_T(64, H)
    N = sf._N(T, 1023)
    assert 0.999 * 2 ** 31 < sf.plane_gemm_bytes(64, T, H) < 2 ** 31  # the largest plane offset of the one 64-lane launch
    with pytest.raises(pkg.UmxError, match="32-bit"):
        pkg.Engine(targets, H, N + 1024, tracks=64)
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=64)
    try:
        waves = [_audio(pkg, 4096, 902 + b) for b in range(64)]
        waves[0], waves[63] = _audio(pkg, N, 900), _audio(pkg, N - 777, 901)
        state = np.zeros(eng.lib.umx_hip_stream_floats(eng.h), np.float32)
        stems = _run(pkg, eng, waves, 0)
        assert eng.gemm_kernel_name(0).startswith("gemm_planes")
        for b in (0, 63):
            check_network(rep, eng, b, targets, state, "64 lanes at the address limit")
            check_front_back(rep, eng, b, waves[b], stems[b], False, "64 lanes at the address limit", sf.fused_run_split(T, 64, n_cus)[0])
    finally:
        eng.close()
    _finish(rep, "address_limit")


def test_segment_bounds(pkg, model_small):
    """N = 4095 and N = 4,193,280 are refused, 4096 and 4,193,279 (T = 4095) accepted; the message names the accepted range."""
    _, _, targets = model_small
    for N in (sf.N_MIN - 1, sf.N_MAX + 1):
        with pytest.raises(pkg.UmxError, match=r"\[4096, 4,193,279\] \(at most 4095 STFT frames"):
            pkg.Engine(targets, H, N)
    for N in (sf.N_MIN, sf.N_MAX):
        eng = pkg.Engine(targets, H, N)
        assert eng.T == sf.n_frames(N) == (5 if N == sf.N_MIN else 4095)
        eng.close()
