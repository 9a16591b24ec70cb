"""Shift ensemble (csrc/shift_mean.h): umx_hip_shift_ensemble separates ONE track at K shift offsets as K track lanes
of one pass and averages them on the device.  Held against its definition -- the fp32 mean, left to right, of what
umx_hip_separate_tracks returns for the K lanes (tests/shift_ensemble_ref.py) -- bit for bit: for lanes that disagree about the
segment count, more shifts than one octet, flags, another sample rate, through the C entry point with guarded buffers and
through umx-cli; against the float64 mean of the oracle's single-shift results within the waveform parity bound."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import shift_ensemble_ref as ser

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
TOL_WAVE = 1e-4  # the waveform parity bound (test_gpu_batch.py); a mean of values each within it stays within it
OFFSETS = [0, 11025, 22049]
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wave(pkg):
    return pkg.ggml.synth_audio(25739, 71)


def _bits_equal(got, want, what):
    for t in range(4):
        assert got[t].shape == want[t].shape, (what, t)
        assert np.array_equal(got[t].view(np.uint32), want[t].view(np.uint32)), (what, t, float(np.abs(got[t] - want[t]).max()))


def _todays_call(pkg, eng, x):
    _bits_equal(eng.separate_ensemble(x, offsets=[700]), eng.separate(x, shift_offset=700), "K = 1")


def test_one_shift_is_todays_call(pkg, model_small, eng3, wave):
    one = pkg.Engine.from_file(model_small[0], N)
    for eng in (one, eng3):
        _todays_call(pkg, eng, wave)
        ref = eng.separate(wave, shift_offset=4033)
        _bits_equal(eng.separate_ensemble(wave), ref, "default offset")
        _bits_equal(eng.separate_ensemble(wave, shifts=1), ref, "shifts=1")
    one.close()


def test_mean_of_lanes_that_disagree_about_the_segment_count(pkg, po, model_small, eng3, wave):
    _, om, _ = model_small
    padded = [wave.shape[1] + max(22050 - o, o) for o in OFFSETS]
    assert padded == [47789, 36764, 47788]
    assert [len(pkg.segment_plan(p, N)[0]) for p in padded] == [4, 3, 4]  # lane 1 idles in the last call
    for length in (25739, 1, N // 2):
        x = np.ascontiguousarray(wave[:, :length])
        cache = {}
        for offsets in (OFFSETS, [22049, 0, 11025]):
            got = eng3.separate_ensemble(x, offsets=offsets)
            lanes = eng3.separate_many([x, x, x], shift_offsets=offsets)
            _bits_equal(got, ser.mean_of_lanes(lanes), (length, offsets))
            ref = ser.oracle_mean_f64(po, om, x, N, offsets, cache=cache)
            for t in range(4):
                err = float(np.abs(got[t] - ref[t]).max())
                print(f"length {length} offsets {offsets} stem {t}: max |gpu - oracle float64 mean| = {err:.3e}")
                assert err <= TOL_WAVE, (length, offsets, t, err)
        _bits_equal(eng3.separate_ensemble(x, offsets=OFFSETS, rate=44100), ser.mean_of_lanes(eng3.separate_many([x, x, x], shift_offsets=OFFSETS)),
                    (length, "rate=44100"))


def test_two_equal_shifts_are_that_shift(pkg, model_small, wave):
    eng = pkg.Engine.from_file(model_small[0], N, tracks=2, lstm_batched=True)
    assert eng.lstm_is_batched()
    _bits_equal(eng.separate_ensemble(wave, offsets=[700, 700]), eng.separate(wave, shift_offset=700), "[700, 700]")
    eng.close()


def test_ten_shifts_span_more_than_one_octet(pkg, model_small):
    x = pkg.ggml.synth_audio(int(N * 1.9), 72)
    eng = pkg.Engine.from_file(model_small[0], N, tracks=10)
    offsets = pkg.ensemble_offsets(10)
    got = eng.separate_ensemble(x, shifts=10)
    lanes = eng.separate_many([x] * 10, shift_offsets=offsets)
    eng.close()
    _bits_equal(got, ser.mean_of_lanes(lanes), "K = 10")
    assert any(not np.array_equal(lanes[0][t], lanes[1][t]) for t in range(4))  # (the shifts do give different stems)


def test_flags_reach_every_lane(pkg, model_small, wave):
    flags = pkg.flags_for_targets(["vocals"], residual=True, softmask=True) | pkg.FLAG_WIENER_ITERS(2)
    eng = pkg.Engine.from_file(model_small[0], N, tracks=2)
    offsets = [4033, 15058]
    got = eng.separate_ensemble(wave, offsets=offsets, flags=flags)
    lanes = eng.separate_many([wave, wave], flags=flags, shift_offsets=offsets)
    plain = eng.separate_ensemble(wave, offsets=offsets)
    eng.close()
    _bits_equal(got, ser.mean_of_lanes(lanes), "flags")
    used = {3, pkg.residual_slot(flags)}
    for t in range(4):
        if t in used:
            assert np.abs(got[t]).max() > 0 and not np.array_equal(got[t], plain[t]), t
        else:
            assert np.abs(got[t]).max() == 0.0, t  # a silent slot stays exactly zero


def test_c_entry_point_writes_exactly_length_frames_and_leaves_the_input(pkg, eng3, wave):
    length = wave.shape[1]
    lay = gd.track_layout(2 * length, misalign=8)
    audio = gd.make(lay, np.ascontiguousarray(wave.T))
    before = audio.copy()
    outs = [gd.make(lay) for _ in range(4)]

    def body_ptr(w):
        return C.cast(w.ctypes.data + 4 * lay.pre, FP)

    off = (C.c_int * 3)(*OFFSETS)
    rc = eng3.lib.umx_hip_shift_ensemble(eng3.h, body_ptr(audio), length, 44100, 3, off, (FP * 4)(*[body_ptr(o) for o in outs]), 0, None, None)
    assert rc == 0, eng3.last_error()
    assert gd.check(audio, lay, expect=before).ok, str(gd.check(audio, lay, expect=before))
    want = eng3.separate_ensemble(wave, offsets=OFFSETS)
    for t in range(4):
        rep = gd.check(outs[t], lay)
        assert rep.ok, (t, str(rep))
        assert np.array_equal(gd.payload(outs[t], lay).reshape(length, 2).T, want[t]), t


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()).cuda()


def _resample(torch, eng, xs, rin, rout, n_out):
    ins = [_dev(torch, x) for x in xs]
    outs = [torch.empty(2 * n_out, dtype=torch.float32, device="cuda") for _ in xs]
    eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.data_ptr() for o in outs], n_out)
    torch.cuda.synchronize()
    return [o.cpu().numpy().reshape(n_out, 2).T.copy() for o in outs]


def test_48k_ensemble_is_the_composition(pkg, model_small):
    import torch
    torch.zeros(1).cuda()
    x = pkg.ggml.synth_audio(3 * 48000, 73)
    offsets = [4033, 15058]
    eng = pkg.Engine.from_file(model_small[0], N, tracks=2)
    got = eng.separate_ensemble(x, offsets=offsets, rate=48000)
    n44 = pkg.resampled_length(x.shape[1], 48000, 44100)
    (x44,) = _resample(torch, eng, [x], 48000, 44100, n44)
    comp = _resample(torch, eng, eng.separate_ensemble(x44, offsets=offsets), 44100, 48000, x.shape[1])
    eng.close()
    _bits_equal(got, comp, "48 kHz")
    assert all(g.shape == x.shape and np.isfinite(g).all() and np.abs(g).max() > 0 for g in got)


def test_refusals_leave_the_context_usable(pkg, eng3, wave):
    for what, kwargs in (("K = 4 on three lanes", dict(shifts=4)), ("K = 0", dict(shifts=0)), ("offset 22050", dict(offsets=[0, 22050])),
                         ("offset -1 in an array", dict(offsets=[100, -1])), ("reset mode", dict(shifts=2, flags=pkg.FLAG_RESET_SEGMENTS)),
                         ("reset mode, one shift", dict(flags=pkg.FLAG_RESET_SEGMENTS)), ("rate 7000", dict(shifts=2, rate=7000)),
                         ("rate 7000, one shift", dict(rate=7000))):
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_ensemble(wave, **kwargs)
        assert e.value.code == pkg.ERR_ARG, what
        assert str(e.value), what
        _todays_call(pkg, eng3, wave[:, :5000])
    a = np.ascontiguousarray(wave.T).ravel()
    outs = [np.empty(a.size, np.float32) for _ in range(4)]
    arr = (FP * 4)(*[o.ctypes.data_as(FP) for o in outs])
    holed = (FP * 4)(arr[0], arr[1], None, arr[3])
    call = eng3.lib.umx_hip_shift_ensemble
    assert call(eng3.h, None, wave.shape[1], 44100, 2, None, arr, 0, None, None) == pkg.ERR_ARG
    assert call(eng3.h, a.ctypes.data_as(FP), wave.shape[1], 44100, 2, None, None, 0, None, None) == pkg.ERR_ARG
    assert call(eng3.h, a.ctypes.data_as(FP), wave.shape[1], 44100, 2, None, holed, 0, None, None) == pkg.ERR_ARG
    assert call(eng3.h, a.ctypes.data_as(FP), 0, 44100, 2, None, arr, 0, None, None) == pkg.ERR_ARG
    assert call(None, a.ctypes.data_as(FP), wave.shape[1], 44100, 2, None, arr, 0, None, None) == pkg.ERR_ARG
    _todays_call(pkg, eng3, wave[:, :5000])


def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def test_cli_shifts_switch(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    x, _ = pkg.wav_load(wav)
    cli, batch = Path(pkg.HERE) / "umx-cli", Path(pkg.HERE) / "umx-batch"
    env = {"UMX_SHIFT_OFFSET": "4033"}
    r = _run(cli, [path, wav, tmp_path / "two"], env, UMX_SHIFTS="2")
    assert r.returncode == 0, r.stderr
    eng = pkg.Engine.from_file(path, tracks=2)  # (the CLI's segment size)
    ref = eng.separate_ensemble(x, offsets=pkg.ensemble_offsets(2, 4033))
    eng.close()
    for t in range(4):
        got, ch = pkg.wav_load(tmp_path / "two" / f"target_{t}.wav")
        assert ch == 2 and np.array_equal(got.view(np.uint32), ref[t].view(np.uint32)), t
    r0 = _run(cli, [path, wav, tmp_path / "plain"], env)
    r1 = _run(cli, [path, wav, tmp_path / "one"], env, UMX_SHIFTS="1")
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    for t in range(4):
        assert (tmp_path / "one" / f"target_{t}.wav").read_bytes() == (tmp_path / "plain" / f"target_{t}.wav").read_bytes(), t
        assert (tmp_path / "one" / f"target_{t}.wav").read_bytes() != (tmp_path / "two" / f"target_{t}.wav").read_bytes(), t
    for bad in ("abc", "65", "0", "2x"):
        r = _run(cli, [path, wav, tmp_path / "bad"], env, UMX_SHIFTS=bad)
        assert r.returncode == 1 and "UMX_SHIFTS" in r.stderr, (bad, r.stderr)
    r = _run(batch, [path, tmp_path / "bout", wav], env, UMX_SHIFTS="2")
    assert r.returncode == 1 and "UMX_SHIFTS" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not (tmp_path / "bad").exists() and not (tmp_path / "bout").exists()
