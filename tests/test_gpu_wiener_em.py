"""Wiener EM iterations on the GPU (UMX_FLAG_WIENER_ITERS; csrc/wiener_em.h): n = 1 keeps today's bits, n >= 2 follows the float64
restatement of the reference loop (tests/wiener_em_ref.py) fed with the engine's own mixture spectrogram and target magnitudes, the fused
and unfused filter paths agree bit for bit, lanes stay independent, and every driver carries the flag."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import rel_l2
import wiener_em_ref

pytestmark = pytest.mark.gpu

N41, N6 = 40 * 1024, 5 * 1024  # 41 frames (five runs of the fused kernel) and 6 frames (one run, no interior frame)
TOL_Y, TOL_WAVE = 1e-4, 1e-4
# Three iterations: the EM steps amplify rounding, and the reference loop evaluated in float32 -- its own precision, its own order
# (tests/wiener_em_ref.py, precision="float32") -- is itself 0.5e-4 .. 7e-4 (rel L2 per target) from float64 on these segments'
# taps, 7e-4 on the 6-frame one.  No float32 implementation meets 1e-4 there; this bound is twice the largest such distance.
TOL_3 = 1.5e-3


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.zeros(1).cuda()  # a current device for the debug entry points


def _taps(eng, lane=None):
    sfx = "" if lane is None else f"#{lane}"
    spec = eng.tap("spec" + sfx)
    mags = [eng.tap("target_mag" + sfx, t) for t in range(4)]
    y = [eng.tap("y" + sfx, t) for t in range(4)]
    return spec, mags, y


def _one(pkg, targets, N, wave, flags, tracks=1):
    """One segment on a fresh context (zero stream state): stems and the y tap (and spec / target_mag)."""
    eng = pkg.Engine(targets, 128, N, tracks=tracks)
    try:
        if tracks == 1:
            stems = eng.infer_segment(wave, flags | pkg.FLAG_DEBUG_TAPS)
            spec, mags, y = _taps(eng)
        else:
            stems = eng.infer_batch([wave] + [None] * (tracks - 1), flags | pkg.FLAG_DEBUG_TAPS)[0]
            spec, mags, y = _taps(eng, 0)
    finally:
        eng.close()
    return stems, y, spec, mags


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_one_iteration_flag_gives_the_bits_of_flags_zero(pkg, model_small, tracks):
    _, _, targets = model_small
    for N in (N41, N6):
        wave = pkg.ggml.synth_audio(N, 61)
        a = _one(pkg, targets, N, wave, 0, tracks)
        b = _one(pkg, targets, N, wave, pkg.FLAG_WIENER_ITERS(1), tracks)
        for t in range(4):
            assert np.array_equal(a[0][t], b[0][t]), (N, t)
            assert np.array_equal(a[1][t], b[1][t]), (N, t)


@pytest.mark.parametrize("tracks", [1, 2], ids=["single_track", "track_batched"])
def test_iterations_follow_the_float64_restatement(pkg, model_small, tracks):
    _, _, targets = model_small
    for N in (N41, N6):
        wave = pkg.ggml.synth_audio(N, 62)
        _, y1, _, _ = _one(pkg, targets, N, wave, 0, tracks)
        for n in (2, 3):
            _, y, spec, mags = _one(pkg, targets, N, wave, pkg.FLAG_WIENER_ITERS(n), tracks)
            ref = wiener_em_ref.wiener_em(spec, mags, n_iter=n)
            tol = TOL_Y if n == 2 else TOL_3
            for t in range(4):
                assert np.isfinite(y[t]).all()
                assert rel_l2(y[t], ref[t]) <= tol, (N, n, t, rel_l2(y[t], ref[t]))
                if n == 2:  # the bits of the flag are read: a second iteration moves the estimate
                    assert rel_l2(y[t], y1[t]) > 1e-3, (N, t)


def test_two_iterations_at_full_size_on_a_track_context(pkg, model_small):
    """T = 2584 (a 60 s segment): thirteen 200-frame batches per EM step, the fused kernel's full run layout."""
    _, _, targets = model_small
    N = pkg.SEGMENT_SAMPLES
    wave = pkg.ggml.synth_audio(N, 63)
    eng = pkg.Engine(targets, 128, N, tracks=2)
    try:
        eng.infer_batch([None, wave], pkg.FLAG_WIENER_ITERS(2) | pkg.FLAG_DEBUG_TAPS)
        spec, mags, y = _taps(eng, 1)
    finally:
        eng.close()
    assert spec.shape[1] == 2584
    ref = wiener_em_ref.wiener_em(spec, mags, n_iter=2)
    for t in range(4):
        assert rel_l2(y[t], ref[t]) <= TOL_Y, (t, rel_l2(y[t], ref[t]))


def test_fused_and_unfused_filters_agree_bitwise_over_iterations(pkg, model_small, monkeypatch):
    """The v-reading fused kernel (wiener_istft_v_kernel) against wiener_apply_kernel<true> + the separate inverse STFT."""
    _, _, targets = model_small
    for N in (N41, N6):
        wave = pkg.ggml.synth_audio(N, 64)
        for n in (2, 3):
            flags = pkg.FLAG_DEBUG_TAPS | pkg.FLAG_WIENER_ITERS(n)
            res = {}
            for mode in ("stats4", "fused"):
                monkeypatch.setenv("UMX_WIENER", mode)
                eng = pkg.Engine(targets, 128, N)
                res[mode] = (eng.infer_segment(wave, flags), [eng.tap("y", t) for t in range(4)])
                eng.close()
            for t in range(4):
                assert np.array_equal(res["fused"][0][t], res["stats4"][0][t]), (N, n, t)
                assert np.array_equal(res["fused"][1][t], res["stats4"][1][t]), (N, n, t)


def test_lanes_stay_independent_over_iterations(pkg, model_small):
    """Three lanes, one of them short: each equals the same audio alone in a one-lane call, bit for bit (the EM step's grid
    covers the lanes of a call, v and R are a lane's own)."""
    _, _, targets = model_small
    N = N41
    waves = [pkg.ggml.synth_audio(N, 65), pkg.ggml.synth_audio(N, 66)[:, : 9 * 1024 + 123], pkg.ggml.synth_audio(N, 67)]
    flags = pkg.FLAG_WIENER_ITERS(2)
    eng = pkg.Engine(targets, 128, N, tracks=3)
    together = eng.infer_batch(waves, flags)
    eng.close()
    for k in range(3):
        eng = pkg.Engine(targets, 128, N, tracks=3)
        batch = [None] * 3
        batch[k] = waves[k]
        alone = eng.infer_batch(batch, flags)[k]
        eng.close()
        for t in range(4):
            assert together[k][t].shape == waves[k].shape
            assert np.array_equal(together[k][t], alone[t]), (k, t)


def test_edge_cases_at_three_iterations(pkg, po, model_small):
    _, _, targets = model_small
    N = N41
    n3 = pkg.FLAG_WIENER_ITERS(3)
    wave = pkg.ggml.synth_audio(N, 68)
    # a skipped target has an all-zero magnitude: v = 0 in every iteration, its stem and y stay exactly zero
    stems, y, _, _ = _one(pkg, targets, N, wave, n3 | pkg.FLAG_SKIP_TARGET(1))
    assert not stems[1].any() and not y[1].any()
    assert all(stems[t].any() for t in (0, 2, 3))
    # silence: max_abs = 1, v = 0, R = 0 / eps, Cxx = 4 sqrt(eps) I -- zeros, no NaN
    stems, y, _, _ = _one(pkg, targets, N, np.zeros((2, N), np.float32), n3)
    for t in range(4):
        assert np.isfinite(stems[t]).all() and not stems[t].any()
        assert np.isfinite(y[t]).all()
    # the stems are the inverse STFT of the iterated estimates
    stems, _, spec, mags = _one(pkg, targets, N, wave, n3)
    ref = wiener_em_ref.wiener_em(spec, mags, n_iter=3)
    for t in range(4):
        want = po.istft(ref[t].astype(np.complex64), N)
        assert rel_l2(stems[t], want) <= TOL_3, (t, rel_l2(stems[t], want))


def test_drivers_carry_the_iteration_count(pkg, model_small):
    """Two-segment tracks at two iterations: the device-resident track driver equals the host driver over umx_hip_infer_segment;
    the multi-GPU driver (loopback, by segment and by target: the phased segment_end / segment_finish_device paths) equals both."""
    path, _, targets = model_small
    N = 24 * 1024
    flags = pkg.FLAG_WIENER_ITERS(2)
    wave = pkg.ggml.synth_audio(int(N * 1.7), 69)
    eng = pkg.Engine.from_file(path, N)
    host = pkg.shift_inference(pkg.engine_backend(eng, flags), wave, N, offset=4033)
    dev = eng.separate(wave, flags=flags, shift_offset=4033)
    one = eng.separate(wave, shift_offset=4033)
    for t in range(4):
        assert np.array_equal(host[t], dev[t]), t
        assert rel_l2(dev[t], one[t]) > 1e-4, t
    for by_target in (False, True):
        mg = pkg.MultiGpuTrack(eng, loopback=True, by_target=by_target)
        got = mg.separate(wave, shift_offset=4033, flags=flags)
        mg.close()
        for t in range(4):
            assert np.array_equal(got[t], dev[t]), (by_target, t)
    eng.close()


def test_cli_reads_the_iteration_switch(pkg, model_small, tmp_path):
    """umx-cli with UMX_WIENER_ITERS=2 on a track of two 60 s segments writes the stems of umx_hip_shift_inference at two
    iterations; values outside 1 .. 15 are refused."""
    path, _, _ = model_small
    L = 70 * 44100
    wave = pkg.ggml.synth_audio(L, 70)
    wav = tmp_path / "in.wav"
    pkg.wav_write(wav, wave)
    cli = Path(pkg.HERE) / "umx-cli"
    out = tmp_path / "out"
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_WIENER_ITERS": "2"}
    r = subprocess.run([str(cli), path, str(wav), str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    eng = pkg.Engine.from_file(path)
    ref = eng.separate(wave, flags=pkg.FLAG_WIENER_ITERS(2), shift_offset=4033)
    eng.close()
    for t in range(4):
        got, ch = pkg.wav_load(out / f"target_{t}.wav")
        assert ch == 2 and got.shape == wave.shape
        assert np.array_equal(got, ref[t]), t
    for bad in ("0", "16"):
        r = subprocess.run([str(cli), path, str(wav), str(tmp_path / "bad")], capture_output=True, text=True,
                           env={**env, "UMX_WIENER_ITERS": bad}, timeout=600)
        assert r.returncode == 1 and "UMX_WIENER_ITERS" in r.stderr, bad
