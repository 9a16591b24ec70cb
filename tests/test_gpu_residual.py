"""The residual source on the GPU (UMX_FLAG_RESIDUAL; csrc/residual_mask.h): the residual slot's mask plane is the fp32 rule
bit for bit, the four slots' filtered spectrograms follow the float64 restatement (tests/residual_ref.py over tests/wiener_em_ref.py) fed
with the engine's own taps, the mixture-phase estimates add up to the input, and every entry point, driver and CLI carries the flag."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import rel_l2

sys.path.insert(0, str(Path(__file__).parent))
import guarded as gd  # noqa: E402
import residual_ref as rr  # noqa: E402
import stage_f64 as sf  # noqa: E402

pytestmark = pytest.mark.gpu

NB = 2049
N41, N6 = 40 * 1024, 5 * 1024  # 41 frames (five runs of the fused kernel) and 6 frames (one run, no interior frame)
SKIP_SETS = [(0, 1, 2), (1,), (0, 2), (2, 3)]
GOLD = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engines' streams exist
    return t


def _flags(pkg, skip, residual=True):
    f = pkg.FLAG_RESIDUAL if residual else 0
    for t in skip:
        f |= pkg.FLAG_SKIP_TARGET(t)
    return f


def _planes(mask):
    """The mask tap (T, 4098) as [2][T][2049]."""
    return np.stack([mask[:, :NB], mask[:, NB:]])


def _one(pkg, targets, N, wave, flags, tracks=1, lane=0):
    """One segment on a fresh context: stems, and the spec / mix_mag / mask / target_mag / y taps of all four slots."""
    eng = pkg.Engine(targets, 128, N, tracks=tracks)
    try:
        if tracks == 1:
            stems = eng.infer_segment(wave, flags | pkg.FLAG_DEBUG_TAPS)
            sfx = ""
        else:
            batch = [None] * tracks
            batch[lane] = wave
            stems = eng.infer_batch(batch, flags | pkg.FLAG_DEBUG_TAPS)[lane]
            sfx = f"#{lane}"
        taps = {"spec": eng.tap("spec" + sfx), "mix_mag": eng.tap("mix_mag" + sfx),
                "mask": [_planes(eng.tap("mask" + sfx, t)) for t in range(4)],
                "target_mag": [eng.tap("target_mag" + sfx, t) for t in range(4)],
                "y": [eng.tap("y" + sfx, t) for t in range(4)]}
    finally:
        eng.close()
    return stems, taps


def _assert_rho_taps(flags, stems, taps, where):
    r = rr.residual_slot(flags)
    want = rr.rho_f32(taps["mask"], flags)
    assert np.array_equal(taps["mask"][r].view(np.uint32), want.view(np.uint32)), (where, "mask of the residual slot")
    tm = (taps["mask"][r] * taps["mix_mag"]).astype(np.float32)
    assert np.array_equal(taps["target_mag"][r].view(np.uint32), tm.view(np.uint32)), (where, "target_mag of the residual slot")
    assert stems[r].any() and taps["y"][r].any(), (where, "the residual is silent")
    for t in rr.skipped(flags):
        if t != r:
            assert not taps["mask"][t].any() and not taps["y"][t].any() and not stems[t].any(), (where, "silent slot", t)
    for t in rr.active(flags):
        assert stems[t].any(), (where, t)


@pytest.mark.parametrize("skip", SKIP_SETS, ids=lambda s: "skip" + "".join(map(str, s)))
def test_rho_taps_are_the_fp32_rule_bitwise(pkg, model_small, skip):
    _, _, targets = model_small
    flags = _flags(pkg, skip)
    for N, tracks in ((N41, 1), (N6, 1), (N41, 2)):
        wave = pkg.ggml.synth_audio(N, 81)
        stems, taps = _one(pkg, targets, N, wave, flags, tracks, lane=tracks - 1)
        _assert_rho_taps(flags, stems, taps, (skip, N, tracks))


def _f64_report(rep, taps, n_iter, where):
    """y of all four slots against float64 fed with the engine's own spec and target_mag taps; the float32 evaluation of the same loop
    is the yardstick (tests/stage_f64.py: 4 x its distance + 2e-7)."""
    ref64 = sf.wiener(taps["spec"], taps["target_mag"], n_iter, "float64")
    ref32 = sf.wiener(taps["spec"], taps["target_mag"], n_iter, "float32")
    for t in range(4):
        r = rep.add(sf.check(f"y[{t}] n={n_iter}", taps["y"][t], ref64[t], ref32[t], "spectrum", where=where))
        print(f"residual f64 {where} iters {n_iter} slot {t}: rel {r['rel']:.3e} (float32 {r['rel32']:.3e}, ratio {r['ratio_rel']:.2f}), "
              f"worst block {r['blk']:.3e} (float32 {r['blk32']:.3e}, ratio {r['ratio_blk']:.2f}), excess {r['excess']:.3f}")


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_all_four_slots_follow_the_float64_restatement(pkg, model_small, tracks):
    _, _, targets = model_small
    rep = sf.Report()
    for skip in ((0, 1, 2), (1,)):
        for N in (N41, N6):
            wave = pkg.ggml.synth_audio(N, 82)
            for n in (1, 2, 3):
                _, taps = _one(pkg, targets, N, wave, _flags(pkg, skip) | pkg.FLAG_WIENER_ITERS(n), tracks)
                _f64_report(rep, taps, n, f"skip {skip} N {N} tracks {tracks}")
    rep.assert_ok()


def test_full_size_segment_on_a_two_lane_context(pkg, model_small):
    """T = 2584: 646 workgroups of eight rows per lane in the residual kernel, thirteen R batches, the fused kernel's full run layout."""
    _, _, targets = model_small
    N = pkg.SEGMENT_SAMPLES
    flags = _flags(pkg, (0, 1, 2))
    stems, taps = _one(pkg, targets, N, pkg.ggml.synth_audio(N, 83), flags, tracks=2, lane=1)
    assert taps["spec"].shape[1] == 2584
    _assert_rho_taps(flags, stems, taps, "T=2584")
    rep = sf.Report()
    _f64_report(rep, taps, 1, "T=2584 lane 1")
    rep.assert_ok()


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_mixture_phase_stems_sum_to_the_input(pkg, model_small, tracks):
    """UMX_FLAG_NO_WIENER | RESIDUAL: sum_j m_j |X| e^{i arg X} + rho |X| e^{i arg X} = X, so the four stems add up to
    iSTFT(STFT(input)) = the input, within the 1e-4 of the identity-mask round trip (tests/test_gpu_parity.py), every sample."""
    _, _, targets = model_small
    for skip in SKIP_SETS:
        for N, n in ((16 * 1024, 16 * 1024), (16 * 1024, 9000)):
            wave = pkg.ggml.synth_audio(n, 84)
            eng = pkg.Engine(targets, 128, N, tracks=tracks)
            flags = _flags(pkg, skip) | pkg.FLAG_NO_WIENER
            stems = eng.infer_segment(wave, flags) if tracks == 1 else eng.infer_batch([None, wave], flags)[1]
            eng.close()
            err = float(np.abs(sum(s.astype(np.float64) for s in stems) - wave).max())
            print(f"mixture-phase conservation skip {skip} n {n} tracks {tracks}: max |sum - input| = {err:.3e}")
            assert err < 1e-4, (skip, n, err)


def test_the_flag_is_read(pkg, model_small):
    _, _, targets = model_small
    wave = pkg.ggml.synth_audio(N41, 85)
    for skip in ((0, 1, 2), (1,)):
        plain, _ = _one(pkg, targets, N41, wave, _flags(pkg, skip, residual=False))
        res, _ = _one(pkg, targets, N41, wave, _flags(pkg, skip))
        r = min(skip)
        assert not plain[r].any() and res[r].any()
        for t in rr.active(_flags(pkg, skip)):
            assert rel_l2(res[t], plain[t]) > 1e-4, (skip, t, rel_l2(res[t], plain[t]))


def test_fused_and_unfused_filters_agree_bitwise(pkg, model_small, monkeypatch):
    _, _, targets = model_small
    for N in (N41, N6):
        wave = pkg.ggml.synth_audio(N, 86)
        for n in (1, 2):
            flags = _flags(pkg, (0, 2)) | pkg.FLAG_WIENER_ITERS(n)
            res = {}
            for mode in ("stats4", "fused"):
                monkeypatch.setenv("UMX_WIENER", mode)
                res[mode] = _one(pkg, targets, N, wave, flags)
            for t in range(4):
                assert np.array_equal(res["fused"][0][t], res["stats4"][0][t]), (N, n, t)
                assert np.array_equal(res["fused"][1]["y"][t], res["stats4"][1]["y"][t]), (N, n, t)


def test_a_lane_among_three_equals_the_lane_alone(pkg, model_small):
    """Three lanes, one short and one idle: one launch of the residual kernel covers the call's lanes, each on its own planes."""
    _, _, targets = model_small
    N = N41
    flags = _flags(pkg, (0, 1, 2))
    waves = [pkg.ggml.synth_audio(N, 87), None, pkg.ggml.synth_audio(N, 88)[:, : 9 * 1024 + 123]]
    eng = pkg.Engine(targets, 128, N, tracks=3)
    together = eng.infer_batch(waves, flags)
    eng.close()
    assert together[1] is None
    for k in (0, 2):
        eng = pkg.Engine(targets, 128, N, tracks=3)
        batch = [None] * 3
        batch[k] = waves[k]
        alone = eng.infer_batch(batch, flags)[k]
        eng.close()
        for t in range(4):
            assert together[k][t].shape == waves[k].shape
            assert np.array_equal(together[k][t], alone[t]), (k, t)


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_no_stale_rho_plane_is_left_in_a_slot(pkg, model_small, tracks):
    """A residual call, then as many calls as bring the pipeline back to the same slot, the last a plain-skip call: its bits are those of
    the same call sequence without the residual ever having run (the skipped slot is zero-filled again)."""
    _, _, targets = model_small
    N = N41
    skip = (0, 2)
    waves = [pkg.ggml.synth_audio(N, 89 + k) for k in range(4)]

    def run(first_flags):
        eng = pkg.Engine(targets, 128, N, tracks=tracks)
        depth = eng.pipeline_depth()
        call = (lambda w, f: eng.infer_segment(w, f)) if tracks == 1 else (lambda w, f: eng.infer_batch([w, None], f)[0])
        try:
            call(waves[0], first_flags)
            for k in range(1, depth):
                call(waves[k], _flags(pkg, skip, residual=False))
            return call(waves[depth], _flags(pkg, skip, residual=False))  # the slot of the first call
        finally:
            eng.close()

    after_residual, fresh = run(_flags(pkg, skip)), run(_flags(pkg, skip, residual=False))
    for t in range(4):
        assert np.array_equal(after_residual[t], fresh[t]), t
    assert not after_residual[0].any() and not after_residual[2].any()


class _Buf:
    """One guarded device buffer (tests/guarded.py)."""

    def __init__(self, torch, layout, data=None):
        self.layout = layout
        self.before = gd.make(layout, data)
        self.t = torch.from_numpy(self.before).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.layout.pre

    def words(self):
        return self.t.cpu().numpy()


@pytest.mark.parametrize("tracks", [1, 3], ids=["single_track", "track_batched"])
def test_device_pointer_call_writes_exactly_n(pkg, model_small, torch, tracks):
    _, _, targets = model_small
    N = gd.SINGLE_N
    n = N - 2 * gd.HOP - 77
    flags = _flags(pkg, (0, 1, 2))
    wave = pkg.ggml.synth_audio(N, 93)[:, :n]
    inter = np.ascontiguousarray(wave.T).ravel()
    eng, twin = pkg.Engine(targets, 128, N, tracks=tracks), pkg.Engine(targets, 128, N, tracks=tracks)
    try:
        a = _Buf(torch, gd.stem_layout(n, N, 8), inter)
        outs = [_Buf(torch, gd.stem_layout(n, N, 8 * (t % 2))) for t in range(4)]
        torch.cuda.synchronize()
        if tracks == 1:
            eng.infer_segment_device(a.ptr, n, [o.ptr for o in outs], flags)
            ref = twin.infer_segment(wave, flags)
        else:
            ptrs, ns, op = [0] * tracks, [0] * tracks, [0] * (4 * tracks)
            idle = [_Buf(torch, gd.stem_layout(gd.HOP, N)) for _ in range(4 * (tracks - 1))]
            ptrs[1], ns[1] = a.ptr, n
            op[4:8] = [o.ptr for o in outs]
            op[0:4] = [o.ptr for o in idle[:4]]
            op[8:12] = [o.ptr for o in idle[4:]]
            eng.infer_batch_ptrs(ptrs, ns, op, flags)
            ref = twin.infer_batch([None, wave, None], flags)[1]
        eng.sync()
        torch.cuda.synchronize()
        r = gd.check(a.words(), a.layout, a.before)
        assert r.ok, ("audio", str(r))
        for t in range(4):
            w = outs[t].words()
            r = gd.check(w, outs[t].layout)
            assert r.ok, ("stem", t, str(r))
            got = gd.payload(w, outs[t].layout).view(np.int32)
            assert np.array_equal(got, np.ascontiguousarray(ref[t].T).ravel().view(np.int32)), t
        if tracks > 1:
            for o in idle:
                assert gd.untouched(o.words(), o.before) is None
    finally:
        eng.close()
        twin.close()


def test_drivers_carry_the_residual(pkg, model_small):
    """A two-segment track: the host driver over umx_hip_infer_segment, the device-resident track driver and the multi-GPU driver in
    by-segment mode (loopback) give the same bits; by-target mode refuses the flag."""
    path, _, targets = model_small
    N = 24 * 1024
    flags = _flags(pkg, (0, 1, 2))
    wave = pkg.ggml.synth_audio(int(N * 1.7), 94)
    eng = pkg.Engine.from_file(path, N)
    host = pkg.shift_inference(pkg.engine_backend(eng, flags), wave, N, offset=4033)
    dev = eng.separate(wave, flags=flags, shift_offset=4033)
    plain = eng.separate(wave, flags=_flags(pkg, (0, 1, 2), residual=False), shift_offset=4033)
    for t in range(4):
        assert np.array_equal(host[t], dev[t]), t
    assert dev[0].any() and not dev[1].any() and not dev[2].any() and not plain[0].any()
    assert rel_l2(dev[3], plain[3]) > 1e-4
    mg = pkg.MultiGpuTrack(eng, loopback=True, by_target=False)
    got = mg.separate(wave, shift_offset=4033, flags=flags)
    mg.close()
    for t in range(4):
        assert np.array_equal(got[t], dev[t]), t
    mg = pkg.MultiGpuTrack(eng, loopback=True, by_target=True)
    with pytest.raises(Exception) as e:
        mg.separate(wave, shift_offset=4033, flags=flags)
    assert getattr(e.value, "code", None) == pkg.ERR_ARG and "UMX_FLAG_RESIDUAL" in str(e.value), e.value
    mg.close()
    # the phased host form zero-fills too: segment_begin / lstm_layer x 3 / segment_end on one segment equals infer_segment
    seg = wave[:, :N]
    eng.stream_reset()
    want = eng.infer_segment(seg, flags)
    eng.stream_reset()
    eng.segment_begin(seg, flags)
    for layer in range(3):
        eng.segment_lstm_layer(layer)
    got = eng.segment_end()
    for t in range(4):
        assert np.array_equal(got[t], want[t]), t
    eng.close()


def test_reset_mode_and_48k_carry_the_residual(pkg, model_small, torch):
    path, _, _ = model_small
    flags = _flags(pkg, (0, 1, 2))
    rng = np.random.default_rng(95)
    n48 = 70 * 48000
    x = (0.1 * rng.standard_normal((2, n48))).astype(np.float32)
    eng = pkg.Engine.from_file(path, tracks=2)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T).ravel()).cuda()

    def resample(xs, rin, rout, n_out):
        ins = [dev(a) for a in xs]
        outs = [torch.empty(2 * n_out, dtype=torch.float32, device="cuda") for _ in xs]
        eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.data_ptr() for o in outs], n_out)
        torch.cuda.synchronize()
        return [o.cpu().numpy().reshape(n_out, 2).T.copy() for o in outs]

    for f in (flags, flags | pkg.FLAG_RESET_SEGMENTS):
        got = eng.separate(x, flags=f, shift_offset=4033, rate=48000)
        n44 = pkg.resampled_length(n48, 48000, 44100)
        (x44,) = resample([x], 48000, 44100, n44)
        stems44 = eng.separate(x44, flags=f, shift_offset=4033)
        comp = resample(stems44, 44100, 48000, n48)
        for t in range(4):
            assert np.array_equal(got[t], comp[t]), (f, t)
        assert got[0].any() and got[3].any() and not got[1].any() and not got[2].any()
    # reset mode carries the flag: it differs from the plain skip in reset mode
    x44 = pkg.ggml.synth_audio(70 * 44100, 96)
    a = eng.separate(x44, flags=flags | pkg.FLAG_RESET_SEGMENTS, shift_offset=4033)
    b = eng.separate(x44, flags=_flags(pkg, (0, 1, 2), residual=False) | pkg.FLAG_RESET_SEGMENTS, shift_offset=4033)
    assert a[0].any() and not b[0].any() and rel_l2(a[3], b[3]) > 1e-4
    eng.close()


def test_invalid_combinations_are_refused(pkg, model_small):
    _, _, targets = model_small
    N = N6
    wave = pkg.ggml.synth_audio(N, 97)
    eng = pkg.Engine(targets, 128, N, tracks=2)
    try:
        for skip in ((), (0, 1, 2, 3)):
            flags = _flags(pkg, skip)
            calls = {"infer_segment": lambda: eng.infer_segment(wave, flags),
                     "infer_batch": lambda: eng.infer_batch([wave, wave], flags),
                     "segment_begin": lambda: eng.segment_begin(wave, flags),
                     "separate": lambda: eng.separate(wave, flags=flags),
                     "separate_rate": lambda: eng.separate(wave, flags=flags, rate=48000),
                     "reset_mode": lambda: eng.separate(wave, flags=flags | pkg.FLAG_RESET_SEGMENTS)}
            for name, call in calls.items():
                with pytest.raises(pkg.UmxError) as e:
                    call()
                assert e.value.code == pkg.ERR_ARG and "UMX_FLAG_RESIDUAL" in str(e.value), (skip, name, e.value)
        # nothing was left open or queued by the refused calls
        ok = eng.infer_segment(wave, _flags(pkg, (1,)))
        assert ok[1].any()
    finally:
        eng.close()


def test_clis_write_the_chosen_targets_and_the_residual(pkg, model_small, tmp_path):
    path, _, _ = model_small
    wav = GOLD / "gspi_stereo.wav"
    wave, _ = pkg.wav_load(wav)
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_TARGETS": "vocals", "UMX_RESIDUAL": "1"}
    cli, batch = Path(pkg.HERE) / "umx-cli", Path(pkg.HERE) / "umx-batch"
    flags = pkg.flags_for_targets(["vocals"], residual=True)
    assert pkg.residual_slot(flags) == 0
    r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["residual.wav", "target_3.wav"]
    eng = pkg.Engine.from_file(path)
    ref = eng.separate(wave, flags=flags, shift_offset=4033)
    eng.close()
    for name, t in (("target_3.wav", 3), ("residual.wav", 0)):
        got, ch = pkg.wav_load(tmp_path / "out" / name)
        assert ch == 2 and np.array_equal(got, ref[t]), name
    # umx-batch: two files (the second a stretch of the first)
    wav2 = tmp_path / "second.wav"
    wave2 = np.ascontiguousarray(wave[:, : wave.shape[1] * 2 // 3])
    pkg.wav_write(wav2, wave2)
    r = subprocess.run([str(batch), path, str(tmp_path / "bout"), str(wav), str(wav2)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    eng2 = pkg.Engine.from_file(path, tracks=2)
    refs = eng2.separate_many([wave, wave2], flags=flags, shift_offsets=[4033, 4033])
    eng2.close()
    for i, name in enumerate(("gspi_stereo", "second")):
        assert sorted(p.name for p in (tmp_path / "bout" / name).iterdir()) == ["residual.wav", "target_3.wav"]
        for fn, t in (("target_3.wav", 3), ("residual.wav", 0)):
            got, _ = pkg.wav_load(tmp_path / "bout" / name / fn)
            assert np.array_equal(got, refs[i][t]), (name, fn)
    # two targets without a residual: exactly their two files
    r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "two")], capture_output=True, text=True,
                       env={**env, "UMX_TARGETS": "drums,vocals", "UMX_RESIDUAL": "0"}, timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in (tmp_path / "two").iterdir()) == ["target_1.wav", "target_3.wav"]
    # refused settings: status 1 and the variable's name
    for bad, var in (({"UMX_TARGETS": "voice"}, "UMX_TARGETS"), ({"UMX_TARGETS": ""}, "UMX_TARGETS"),
                     ({"UMX_TARGETS": "bass,drums,other,vocals"}, "UMX_RESIDUAL")):
        for exe, args in ((cli, [path, str(wav), str(tmp_path / "bad")]), (batch, [path, str(tmp_path / "bad"), str(wav)])):
            r = subprocess.run([str(exe)] + args, capture_output=True, text=True, env={**env, **bad}, timeout=600)
            assert r.returncode == 1 and var in r.stderr, (exe.name, bad, r.stderr)
    no_targets = {k: v for k, v in env.items() if k != "UMX_TARGETS"}
    r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "bad")], capture_output=True, text=True, env=no_targets, timeout=600)
    assert r.returncode == 1 and "UMX_RESIDUAL" in r.stderr, r.stderr
    assert not (tmp_path / "bad").exists()
