"""The soft mask on the GPU (UMX_FLAG_SOFTMASK; csrc/softmask.h): the rewritten mask planes follow the fp32 rule to its
rounding bound, the residual is formed from the normalised planes, the filtered spectrograms follow the float64 restatement
(tests/softmask_ref.py), the mixture-phase stems add up to the input -- which they do not without the flag --, and every entry point,
driver and CLI carries the flag.

Segments of 41 and 6 frames: 82 and 12 plane rows, i.e. ten full groups of eight rows plus a partial one / one full and one partial
group, even and odd rows of the spectrogram (the two alignments of its 2049 x 8 byte rows) and the bin-2048 tail of every row."""
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
import softmask_ref as sr  # noqa: E402
import stage_f64 as sf  # noqa: E402
import wiener_em_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NB = 2049
N41, N6 = 40 * 1024, 5 * 1024
ACTIVE_SETS = [(0, 1, 2, 3), (0, 2, 3), (3,), (0, 1)]
CONFIGS = [(N41, 1, 0), (N6, 1, 0), (N41, 2, 1), (N6, 2, 0)]  # (segment samples, track lanes of the context, the lane used)
GOLD = Path(__file__).parent / "golden"
SEED = 181


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engines' streams exist
    return t


def _flags(pkg, active=(0, 1, 2, 3), softmask=True, residual=False):
    f = (pkg.FLAG_SOFTMASK if softmask else 0) | (pkg.FLAG_RESIDUAL if residual else 0)
    for t in range(4):
        if t not in active:
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


@pytest.fixture(scope="module")
def seg(pkg, model_small):
    """(N, tracks, lane, flags) -> (stems, taps) of the one test segment of that length, computed once per module and left unchanged."""
    _, _, targets = model_small
    cache = {}

    def run(N, tracks, lane, flags):
        key = (N, tracks, lane, flags)
        if key not in cache:
            cache[key] = _one(pkg, targets, N, pkg.ggml.synth_audio(N, SEED), flags, tracks, lane)
        return cache[key]
    return run


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---------------------------------------------------------------- 1: the rule
@pytest.mark.parametrize("active", ACTIVE_SETS, ids=lambda s: "active" + "".join(map(str, s)))
def test_mask_taps_follow_the_rule(pkg, seg, active):
    """Every element of the rewritten planes within relative 1e-6 (+ 1e-37 absolute for subnormal quotients) of the rule evaluated in
    float64 from the fp32 mask and mix_mag taps of the same segment without the flag.  In units of u = 2^-24: a carries <= 2.5 u, g + 1 u,
    three adds of non-negative terms + 3 u, the eps add + 1 u, the quotient + 1 u: numerator and denominator together <= 12 u = 7.2e-7,
    also where eps dominates the denominator and the error of a does not cancel."""
    for N, tracks, lane in CONFIGS:
        _, plain = seg(N, tracks, lane, _flags(pkg, active, softmask=False))
        flags = _flags(pkg, active)
        stems, soft = seg(N, tracks, lane, flags)
        assert _same_bits(plain["mix_mag"], soft["mix_mag"]) and plain["mix_mag"].shape == (2, N // 1024 + 1, NB)
        for j in active:
            assert (plain["mask"][j] >= 0).all(), "masks are ReLU outputs"
            assert plain["mask"][j].any() and not _same_bits(plain["mask"][j], soft["mask"][j]), (active, j, "the planes were not rewritten")
            assert np.isfinite(soft["mask"][j]).all()
        worst = sr.rule_errors(soft["mask"], plain["mix_mag"], plain["mask"], flags)
        print(f"softmask rule active {active} N {N} tracks {tracks}: worst error / bound per target {worst}")
        assert max(worst.values()) <= 1.0, (active, N, tracks, worst)
        silent = plain["mix_mag"] == 0
        for j in active:
            assert not soft["mask"][j][silent].any(), "a silent bin gives m' = 0"
        for t in range(4):
            if t not in active:  # skipped, no residual: exactly zero
                assert not soft["mask"][t].any() and not soft["y"][t].any() and not stems[t].any(), (active, t)


# ---------------------------------------------------------------- 2: the magnitude tap
def test_target_mag_tap_is_mask_times_mix_mag_bitwise(pkg, seg):
    for active in ((0, 1, 2, 3), (0, 1)):
        for N, tracks, lane in CONFIGS:
            _, soft = seg(N, tracks, lane, _flags(pkg, active))
            for t in range(4):
                want = (soft["mask"][t] * soft["mix_mag"]).astype(np.float32)
                assert _same_bits(soft["target_mag"][t], want), (active, N, tracks, t)


# ---------------------------------------------------------------- 3: with the residual
@pytest.mark.parametrize("skip", [(0, 1, 2), (1,)], ids=lambda s: "skip" + "".join(map(str, s)))
def test_residual_is_formed_from_the_normalised_planes(pkg, seg, skip):
    active = tuple(t for t in range(4) if t not in skip)
    for N, tracks, lane in CONFIGS:
        flags = _flags(pkg, active, residual=True)
        r = rr.residual_slot(flags)
        stems, both = seg(N, tracks, lane, flags)
        _, soft = seg(N, tracks, lane, _flags(pkg, active))
        for j in active:  # the residual changes nothing about the normalisation
            assert _same_bits(both["mask"][j], soft["mask"][j]), (skip, N, tracks, j)
        assert _same_bits(both["mask"][r], rr.rho_f32(both["mask"], flags)), (skip, N, tracks, "rho of the softmask taps")
        assert _same_bits(both["target_mag"][r], (both["mask"][r] * both["mix_mag"]).astype(np.float32))
        # rho = 1 - sum m' and sum m' = s / (eps + s), s = sum g of the plain masks: where s > 1e-3 that is eps / (eps + s) <= 1e-7 plus the
        # fp32 error of the m' (12 u together, test_mask_taps_follow_the_rule) and of at most three additions (3 u), u = 2^-24
        _, plain = seg(N, tracks, lane, _flags(pkg, active, softmask=False))
        s = sum(plain["target_mag"][j].astype(np.float64) for j in active)
        assert (s > 1e-3).any()
        assert np.abs(both["mask"][r][s > 1e-3]).max() <= 1e-7 + 15 * 2.0 ** -24, "the residual's first estimate is nearly empty"
        for t in skip:
            if t != r:
                assert not both["mask"][t].any() and not stems[t].any()


# ---------------------------------------------------------------- 4: float64 end to end
def _f64_report(rep, got, plain, flags, n_iter, where, slots):
    """y against tests/softmask_ref.wiener (softmask, residual, EM) fed with the spec and mix_mag taps and the masks of the same segment
    WITHOUT the flag; the float32 evaluation of the same restatement is the yardstick (tests/stage_f64.py: 4 x its distance + 2e-7, the
    bounds tests/test_gpu_residual.py holds its float64 comparison to)."""
    ma = wiener_em_ref.find_max_abs(np.asarray(got["spec"], np.complex128))
    ref64 = sr.wiener(got["spec"], plain["mix_mag"], plain["mask"], flags, n_iter, "float64", max_abs=ma)
    ref32 = sr.wiener(got["spec"], plain["mix_mag"], plain["mask"], flags, n_iter, "float32", max_abs=ma)
    for t in slots:
        r = rep.add(sf.check(f"y[{t}] n={n_iter}", got["y"][t], ref64[t], ref32[t], "spectrum", where=where))
        print(f"softmask f64 {where} iters {n_iter} slot {t}: rel {r['rel']:.3e} (float32 {r['rel32']:.3e}, ratio {r['ratio_rel']:.2f}), "
              f"worst block {r['blk']:.3e} (float32 {r['blk32']:.3e}, ratio {r['ratio_blk']:.2f}), excess {r['excess']:.3f}")


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_all_four_slots_follow_the_float64_restatement(pkg, model_small, seg, tracks, monkeypatch):
    """Four targets, and three targets with a silent slot: all four slots.  Three targets plus the residual: the three targets' slots --
    the residual's own magnitude is then the fp32 rounding of 1 - sum m' (a few 2^-24, either sign) where float64 has 1e-10 / sum g, so no
    float32 evaluation follows float64 in that slot; its plane is pinned bit for bit by
    test_residual_is_formed_from_the_normalised_planes instead."""
    _, _, targets = model_small
    rep = sf.Report()
    for active, residual in (((0, 1, 2, 3), False), ((0, 2, 3), False), ((0, 2, 3), True)):
        for N in (N41, N6):
            wave = pkg.ggml.synth_audio(N, SEED)
            _, plain = seg(N, tracks, 0, _flags(pkg, active, softmask=False))
            for n in (1, 2):
                for mode in ("fused", "stats4"):
                    monkeypatch.setenv("UMX_WIENER", mode)
                    flags = _flags(pkg, active, residual=residual)
                    _, got = _one(pkg, targets, N, wave, flags | pkg.FLAG_WIENER_ITERS(n), tracks)
                    assert _same_bits(got["spec"], plain["spec"])
                    _f64_report(rep, got, plain, flags, n, f"active {active} residual {residual} N {N} tracks {tracks} {mode}",
                                active if residual else range(4))
    rep.assert_ok()


# ---------------------------------------------------------------- 5: the stems sum to the mixture
@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_mixture_phase_stems_sum_to_the_input_only_with_the_flag(pkg, model_small, tracks):
    """UMX_FLAG_NO_WIENER | SOFTMASK, four targets: sum_j X g_j / (eps + sum g) = X wherever sum g >> eps, so the four stems add up to
    iSTFT(STFT(input)) = the input within the 1e-4 of tests/test_gpu_residual.py::test_mixture_phase_stems_sum_to_the_input.  Without
    the flag the masks sum to whatever the networks say and the same call misses that bound."""
    _, _, targets = model_small
    for N, n in ((16 * 1024, 16 * 1024), (16 * 1024, 9000)):
        wave = pkg.ggml.synth_audio(n, 184)
        err = {}
        for softmask in (True, False):
            eng = pkg.Engine(targets, 128, N, tracks=tracks)
            flags = _flags(pkg, softmask=softmask) | pkg.FLAG_NO_WIENER
            stems = eng.infer_segment(wave, flags) if tracks == 1 else eng.infer_batch([None, wave], flags)[1]
            eng.close()
            err[softmask] = float(np.abs(sum(s.astype(np.float64) for s in stems) - wave).max())
        print(f"softmask mixture-phase conservation n {n} tracks {tracks}: max |sum - input| = {err[True]:.3e} with the flag, "
              f"{err[False]:.3e} without")
        assert err[True] < 1e-4, (n, err)
        assert err[False] >= 1e-4, (n, err, "the plain masks happen to sum to one here: another segment is needed")


# ---------------------------------------------------------------- 6: bitwise invariants
def test_a_lane_among_three_equals_the_lane_alone(pkg, model_small):
    """Three lanes, one short and one idle: one launch of the softmask kernel covers the call's lanes, each on its own planes."""
    _, _, targets = model_small
    N = N41
    flags = _flags(pkg)
    waves = [pkg.ggml.synth_audio(N, 187), None, pkg.ggml.synth_audio(N, 188)[:, : 9 * 1024 + 123]]
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


def test_fused_and_unfused_filters_agree_bitwise(pkg, model_small, monkeypatch):
    _, _, targets = model_small
    for N in (N41, N6):
        wave = pkg.ggml.synth_audio(N, 186)
        for extra in (0, pkg.FLAG_WIENER_ITERS(2), pkg.FLAG_NO_WIENER):
            flags = _flags(pkg, (0, 2, 3)) | extra
            res = {}
            for mode in ("stats4", "fused"):
                monkeypatch.setenv("UMX_WIENER", mode)
                res[mode] = _one(pkg, targets, N, wave, flags)
            for t in range(4):
                assert np.array_equal(res["fused"][0][t], res["stats4"][0][t]), (N, extra, t)
                assert np.array_equal(res["fused"][1]["y"][t], res["stats4"][1]["y"][t]), (N, extra, t)


def test_the_flag_is_read(pkg, seg):
    for active in ((0, 1, 2, 3), (3,)):
        for N, tracks, lane in CONFIGS:
            plain, _ = seg(N, tracks, lane, _flags(pkg, active, softmask=False))
            soft, _ = seg(N, tracks, lane, _flags(pkg, active))
            for t in active:
                assert soft[t].any() and not np.array_equal(soft[t], plain[t]), (active, N, tracks, t)
                print(f"softmask against plain, active {active} N {N} tracks {tracks} target {t}: rel L2 {rel_l2(soft[t], plain[t]):.3e}")


# ---------------------------------------------------------------- 7: the drivers
def test_drivers_carry_the_flag(pkg, model_small):
    """A two-segment track: umx_hip_shift_inference, umx_hip_separate_tracks, the multi-GPU driver by segment (loopback) and the phased
    host form give the bits of the segment-wise composition (the host driver over one-segment calls); by-target mode refuses the flag."""
    path, _, targets = model_small
    N = 24 * 1024
    flags = _flags(pkg, (0, 3), residual=True)
    wave = pkg.ggml.synth_audio(int(N * 1.7), 194)
    eng = pkg.Engine.from_file(path, N)
    host = pkg.shift_inference(pkg.engine_backend(eng, flags), wave, N, offset=4033)
    dev = eng.separate(wave, flags=flags, shift_offset=4033)
    plain = eng.separate(wave, flags=flags & ~pkg.FLAG_SOFTMASK, shift_offset=4033)
    for t in range(4):
        assert np.array_equal(host[t], dev[t]), t
    assert dev[0].any() and dev[3].any() and not dev[2].any()
    assert not np.array_equal(dev[3], plain[3]) and not np.array_equal(dev[1], plain[1])
    mg = pkg.MultiGpuTrack(eng, loopback=True, by_target=False)
    got = mg.separate(wave, shift_offset=4033, flags=flags)
    mg.close()
    for t in range(4):
        assert np.array_equal(got[t], dev[t]), t
    # 9: the refusal, reached in loopback on one GPU
    mg = pkg.MultiGpuTrack(eng, loopback=True, by_target=True)
    with pytest.raises(Exception) as e:
        mg.separate(wave, shift_offset=4033, flags=_flags(pkg))
    assert getattr(e.value, "code", None) == pkg.ERR_ARG and "UMX_FLAG_SOFTMASK" in str(e.value), e.value
    mg.close()
    seg0 = wave[:, :N]
    eng.stream_reset()
    want = eng.infer_segment(seg0, flags)
    eng.stream_reset()
    eng.segment_begin(seg0, flags)
    for layer in range(3):
        eng.segment_lstm_layer(layer)
    got = eng.segment_end()
    for t in range(4):
        assert np.array_equal(got[t], want[t]), t
    eng.close()
    # umx_hip_separate_tracks: two tracks side by side, each the composition of its own segments on a track-batched context
    wave2 = pkg.ggml.synth_audio(int(N * 1.2), 195)
    eng2 = pkg.Engine(targets, 128, N, tracks=2)
    many = eng2.separate_many([wave, wave2], flags=flags, shift_offsets=[4033, 4033])
    be = pkg.make_backend(lambda w: eng2.infer_batch([w, None], flags)[0], lambda: eng2.track_stream_reset(-1))
    for i, w in enumerate((wave, wave2)):
        comp = pkg.shift_inference(be, w, N, offset=4033)
        for t in range(4):
            assert np.array_equal(many[i][t], comp[t]), (i, t)
    eng2.close()


def test_reset_mode_and_48k_carry_the_flag(pkg, model_small, torch):
    _, _, targets = model_small
    N = 16 * 1024
    flags = _flags(pkg)
    eng = pkg.Engine(targets, 128, N, tracks=2)

    def segment_from_zero(w):
        eng.track_stream_reset(-1)
        return eng.infer_batch([w], flags)[0]
    wave = pkg.ggml.synth_audio(int(N * 2.3), 196)
    got = eng.separate(wave, flags=flags | pkg.FLAG_RESET_SEGMENTS, shift_offset=4033)
    comp = pkg.shift_inference(pkg.make_backend(segment_from_zero), wave, N, offset=4033)
    plain = eng.separate(wave, flags=pkg.FLAG_RESET_SEGMENTS, shift_offset=4033)
    for t in range(4):
        assert np.array_equal(got[t], comp[t]), t
        assert not np.array_equal(got[t], plain[t]), t

    # 48 kHz: resampled in, separated segment by segment at 44.1 kHz, resampled back
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T).ravel()).cuda()

    def resample(xs, rin, rout, n_out):
        ins = [dev(a) for a in xs]
        outs = [torch.empty(2 * n_out, dtype=torch.float32, device="cuda") for _ in xs]
        eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.data_ptr() for o in outs], n_out)
        torch.cuda.synchronize()
        return [o.cpu().numpy().reshape(n_out, 2).T.copy() for o in outs]

    rng = np.random.default_rng(197)
    n48 = int(N * 1.6 * 48000 / 44100)
    x = (0.1 * rng.standard_normal((2, n48))).astype(np.float32)
    got = eng.separate(x, flags=flags, shift_offset=4033, rate=48000)
    n44 = pkg.resampled_length(n48, 48000, 44100)
    (x44,) = resample([x], 48000, 44100, n44)
    be = pkg.make_backend(lambda w: eng.infer_batch([w, None], flags)[0], lambda: eng.track_stream_reset(-1))
    stems44 = pkg.shift_inference(be, x44, N, offset=4033)
    comp = resample(stems44, 44100, 48000, n48)
    for t in range(4):
        assert got[t].any() and np.array_equal(got[t], comp[t]), t
    eng.close()


# ---------------------------------------------------------------- 8: the device-pointer call
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
    flags = _flags(pkg, (0, 1, 3))
    wave = pkg.ggml.synth_audio(N, 193)[:, :n]
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


# ---------------------------------------------------------------- 10: the CLIs
def test_clis_carry_umx_softmask(pkg, model_small, tmp_path):
    path, _, _ = model_small
    wav = GOLD / "gspi_stereo.wav"
    wave, _ = pkg.wav_load(wav)
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_SOFTMASK": "1"}
    for k in ("UMX_TARGETS", "UMX_RESIDUAL"):
        env.pop(k, None)
    cli, batch = Path(pkg.HERE) / "umx-cli", Path(pkg.HERE) / "umx-batch"
    flags = pkg.flags_for_targets(pkg.TARGET_NAMES, softmask=True)
    names = [f"target_{t}.wav" for t in range(4)]
    r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == names
    eng = pkg.Engine.from_file(path)
    ref = eng.separate(wave, flags=flags, shift_offset=4033)
    plain = eng.separate(wave, shift_offset=4033)
    eng.close()
    for t in range(4):
        got, ch = pkg.wav_load(tmp_path / "out" / names[t])
        assert ch == 2 and np.array_equal(got, ref[t]) and not np.array_equal(got, plain[t]), t
    # umx-batch: two files (the second a stretch of the first), vocals and the rest
    wav2 = tmp_path / "second.wav"
    wave2 = np.ascontiguousarray(wave[:, : wave.shape[1] * 2 // 3])
    pkg.wav_write(wav2, wave2)
    env2 = {**env, "UMX_TARGETS": "vocals", "UMX_RESIDUAL": "1"}
    flags2 = pkg.flags_for_targets(["vocals"], residual=True, softmask=True)
    r = subprocess.run([str(batch), path, str(tmp_path / "bout"), str(wav), str(wav2)], capture_output=True, text=True, env=env2, timeout=600)
    assert r.returncode == 0, r.stderr
    eng2 = pkg.Engine.from_file(path, tracks=2)
    refs = eng2.separate_many([wave, wave2], flags=flags2, shift_offsets=[4033, 4033])
    eng2.close()
    for i, name in enumerate(("gspi_stereo", "second")):
        assert sorted(p.name for p in (tmp_path / "bout" / name).iterdir()) == ["residual.wav", "target_3.wav"]
        for fn, t in (("target_3.wav", 3), ("residual.wav", 0)):
            got, _ = pkg.wav_load(tmp_path / "bout" / name / fn)
            assert np.array_equal(got, refs[i][t]), (name, fn)
    # UMX_SOFTMASK=0 is the plain call
    r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "off")], capture_output=True, text=True, env={**env, "UMX_SOFTMASK": "0"}, timeout=600)
    assert r.returncode == 0, r.stderr
    got, _ = pkg.wav_load(tmp_path / "off" / "target_3.wav")
    assert np.array_equal(got, plain[3])
