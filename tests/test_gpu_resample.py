"""Resampling on the device (csrc/resample.h): the kernel against the float64 definition (tests/resample_ref.py),
batched launches against single ones bit for bit, exactly n_out frames written, and the any-rate track entry points
(umx_hip_shift_inference_rate / _separate_tracks_rate): bitwise today's entry points at 44.1 kHz, bitwise the composition
resample -> separate -> resample elsewhere, and the same through umx-cli / umx-batch with UMX_RESAMPLE=1."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import resample_ref as rr

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
PAIRS = [(48000, 44100), (96000, 44100), (22050, 44100), (8000, 44100), (32000, 44100), (44056, 44100)]
PAIRS = PAIRS + [(b, a) for a, b in PAIRS]
TOL_MAX, TOL_L2 = 4e-6, 1e-6
CANARY = 1024  # floats of NaN pattern in front of and behind every output buffer


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()
    return t


@pytest.fixture(scope="module")
def eng(pkg, model_small, torch):
    _, _, targets = model_small
    e = pkg.Engine(targets, 128, 16 * 1024)
    yield e
    e.close()


def _inputs(n, rin, kind, seed, rout=44100):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = rng.uniform(-1, 1, (2, n))
    elif kind == "tones":  # just below and just above the cutoff 0.99 min(r_in, r_out) / 2
        cut = 0.99 * min(rin, rout) / 2
        i = np.arange(n)
        x = np.stack([np.sin(2 * np.pi * 0.97 * cut * i / rin), np.sin(2 * np.pi * 1.03 * cut * i / rin + 0.3)])
    else:  # impulses in the first and the last sample
        x = np.zeros((2, n))
        x[0, 0], x[1, -1] = 1.0, -1.0
        x[1, 0], x[0, -1] = 0.5, 0.75
    return x.astype(np.float32)


class Out:
    """A device buffer of n frames with NaN-pattern canaries around it."""

    def __init__(self, torch, n):
        self.n, self.i32 = n, torch.int32
        self.t = torch.empty((2 * n + 2 * CANARY,), dtype=torch.float32, device="cuda")
        self.t.view(torch.int32)[:] = 0x7FC0DEAD

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * CANARY

    def read(self):
        a = self.t.view(self.i32).cpu().numpy()
        assert (a[:CANARY] == 0x7FC0DEAD).all() and (a[-CANARY:] == 0x7FC0DEAD).all(), "write outside [0, n_out)"
        return self.t[CANARY:CANARY + 2 * self.n].cpu().numpy().reshape(self.n, 2).T.copy()


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()).cuda()


def _resample(torch, eng, x_list, rin, rout, n_out):
    ins = [_dev(torch, x) for x in x_list]
    outs = [Out(torch, n_out) for _ in x_list]
    eng.resample_device(rin, rout, [t.data_ptr() for t in ins], x_list[0].shape[1], [o.ptr for o in outs], n_out)
    torch.cuda.synchronize()
    return [o.read() for o in outs]


def _check(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    rel = np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30)
    assert err.max() <= TOL_MAX and (rel <= TOL_L2 or np.linalg.norm(ref) < 1e-3), (what, float(err.max()), float(rel))


@pytest.mark.parametrize("rin,rout", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_kernel_follows_the_float64_definition(pkg, torch, eng, rin, rout):
    K = rr.geometry(rin, rout)[4]
    for n in (1, 2, K - 1, K + 1, 4099):
        for kind in ("noise", "tones", "impulses"):
            x = _inputs(n, rin, kind, n, rout)
            n_out = pkg.resampled_length(n, rin, rout)
            (got,) = _resample(torch, eng, [x], rin, rout, n_out)
            _check(got, rr.resample(x, rin, rout, n_out), (n, kind))
    x = _inputs(1_000_003, rin, "noise", 9)
    (got,) = _resample(torch, eng, [x], rin, rout, pkg.resampled_length(x.shape[1], rin, rout))
    _check(got, rr.resample(x, rin, rout), "1000003")


@pytest.mark.parametrize("rin,rout", [(48000, 44100), (44100, 8000), (44056, 44100)])
def test_four_buffer_launch_equals_four_single_launches_and_n_out_follows_the_formula(pkg, torch, eng, rin, rout):
    n = 50_001
    xs = [_inputs(n, rin, "noise", 20 + b) for b in range(4)]
    n_out = pkg.resampled_length(n, rin, rout) + 3 * rr.geometry(rin, rout)[4] + 5  # zeros in, a decaying tail out
    four = _resample(torch, eng, xs, rin, rout, n_out)
    for b in range(4):
        (one,) = _resample(torch, eng, [xs[b]], rin, rout, n_out)
        assert np.array_equal(four[b].view(np.uint32), one.view(np.uint32)), b
        _check(four[b], rr.resample(xs[b], rin, rout, n_out), b)
    assert np.abs(four[0][:, -5:]).max() == 0.0  # far past the input every tap reads zeros
    short = _resample(torch, eng, xs[:1], rin, rout, 7)[0]  # fewer frames than natural: a prefix of the same outputs
    assert np.array_equal(short, four[0][:, :7])
    eng.resample_device(rin, rout, [_dev(torch, xs[0]).data_ptr()], n, [Out(torch, 1).ptr], 0)  # n_out = 0 writes nothing
    with pytest.raises(pkg.UmxError):
        eng.resample_device(7999, rout, [_dev(torch, xs[0]).data_ptr()], n, [Out(torch, 8).ptr], 8)


def _wave(pkg, seconds, rate, seed):
    return pkg.ggml.synth_audio(int(seconds * rate), seed)


def _shift_rate(pkg, eng, x, rate, offset):
    """umx_hip_shift_inference_rate itself (Engine.separate takes today's entry point at 44.1 kHz)."""
    import ctypes as C
    fp = C.POINTER(C.c_float)
    L = x.shape[1]
    a = np.ascontiguousarray(x.T).ravel()
    outs = [np.empty(2 * L, np.float32) for _ in range(4)]
    rc = eng.lib.umx_hip_shift_inference_rate(eng.h, a.ctypes.data_as(fp), L, rate, offset, (fp * 4)(*[o.ctypes.data_as(fp) for o in outs]),
                                              0, None, None)
    assert rc == 0, eng.last_error()
    return [o.reshape(L, 2).T for o in outs]


def test_rate_entry_points_at_44100_are_todays_entry_points(pkg, model_small):
    path, _, _ = model_small
    x = _wave(pkg, 70, 44100, 31)
    eng = pkg.Engine.from_file(path)
    a = eng.separate(x, shift_offset=4033)
    b = _shift_rate(pkg, eng, x, 44100, 4033)
    c = _shift_rate(pkg, eng, x, 44100, -1)  # < 0 = the reference's 4033
    eng.close()
    for t in range(4):
        assert np.array_equal(a[t], b[t]) and np.array_equal(a[t], c[t]), t
    eng2 = pkg.Engine.from_file(path, tracks=2)
    ys = [_wave(pkg, 9, 44100, 32), _wave(pkg, 13, 44100, 33)]
    p = eng2.separate_many(ys, shift_offsets=[4033, None])
    q = eng2.separate_many(ys, shift_offsets=[4033, None], rates=[44100, 44100])
    eng2.close()
    for i in range(2):
        for t in range(4):
            assert np.array_equal(p[i][t], q[i][t]), (i, t)


def _composition(torch, pkg, eng, x, rate, offset, flags=0):
    """resample(rate <- 44100) of the n44 frames that shift_inference returns for resample(44100 <- rate) of x, on the device."""
    n44 = pkg.resampled_length(x.shape[1], rate, 44100)
    (x44,) = _resample(torch, eng, [x], rate, 44100, n44)
    stems44 = eng.separate(x44, flags=flags, shift_offset=offset)
    return _resample(torch, eng, stems44, 44100, rate, x.shape[1]), x44


def test_48k_track_is_the_composition_bitwise_and_near_float64_resampling(pkg, model_small, torch):
    path, _, _ = model_small
    x = _wave(pkg, 70, 48000, 41)
    eng = pkg.Engine.from_file(path)
    got = eng.separate(x, shift_offset=4033, rate=48000)
    comp, _ = _composition(torch, pkg, eng, x, 48000, 4033)
    for t in range(4):
        assert got[t].shape == x.shape
        assert np.array_equal(got[t].view(np.uint32), comp[t].view(np.uint32)), t
    # the same separation around a float64 resampler: within the waveform parity bound
    s44 = eng.separate(rr.resample(x, 48000, 44100).astype(np.float32), shift_offset=4033)
    eng.close()
    for t in range(4):
        ref = rr.resample(s44[t], 44100, 48000, x.shape[1])
        assert np.abs(got[t] - ref).max() <= 1e-4, (t, float(np.abs(got[t] - ref).max()))


def test_mixed_rates_in_one_pass_are_each_their_own_one_track_call(pkg, model_small):
    path, _, _ = model_small
    rates = [44100, 48000, 32000]
    xs = [_wave(pkg, s, r, 50 + i) for i, (s, r) in enumerate(zip((11, 9, 13), rates))]
    eng = pkg.Engine.from_file(path, tracks=3)
    many = eng.separate_many(xs, shift_offsets=[4033, 100, None], rates=rates)
    for i in range(3):
        one = eng.separate_many([xs[i]], shift_offsets=[[4033, 100, None][i]], rates=[rates[i]])[0]
        for t in range(4):
            assert many[i][t].shape == xs[i].shape
            assert np.array_equal(many[i][t], one[t]), (i, t)
    with pytest.raises(pkg.UmxError) as e:
        eng.separate_many(xs[:1], rates=[7000])
    assert e.value.code == pkg.ERR_ARG
    eng.close()


def test_reset_mode_and_wiener_iterations_at_48k(pkg, model_small, torch):
    path, _, _ = model_small
    x = _wave(pkg, 70, 48000, 61)
    eng = pkg.Engine.from_file(path, tracks=2)
    for flags in (pkg.FLAG_RESET_SEGMENTS, pkg.FLAG_WIENER_ITERS(2)):
        got = eng.separate(x, flags=flags, shift_offset=4033, rate=48000)
        comp, _ = _composition(torch, pkg, eng, x, 48000, 4033, flags)
        for t in range(4):
            assert np.isfinite(got[t]).all()
            assert np.array_equal(got[t], comp[t]), (flags, t)
    eng.close()


def _gspi_48k(pkg):
    wave, _ = pkg.wav_load(GOLD / "gspi_stereo.wav")
    return rr.resample(wave, 44100, 48000).astype(np.float32)


def test_cli_and_batch_resample_switch(pkg, model_small, tmp_path):
    path, _, _ = model_small
    x48 = _gspi_48k(pkg)
    wav48 = tmp_path / "gspi48.wav"
    pkg.wav_write(wav48, x48, rate=48000)
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033"}
    cli = Path(pkg.HERE) / "umx-cli"
    r = subprocess.run([str(cli), path, str(wav48), str(tmp_path / "out")], capture_output=True, text=True,
                       env={**env, "UMX_RESAMPLE": "1"}, timeout=600)
    assert r.returncode == 0, r.stderr
    eng = pkg.Engine.from_file(path)
    ref = eng.separate(x48, shift_offset=4033, rate=48000)
    eng.close()
    for t in range(4):
        got, ch, rate = pkg.wav_load_rate(tmp_path / "out" / f"target_{t}.wav")
        assert ch == 2 and rate == 48000 and got.shape == x48.shape
        assert np.array_equal(got, ref[t]), t
    r = subprocess.run([str(cli), path, str(wav48), str(tmp_path / "plain")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 1 and "only supports the following sample rate (Hz): 44100" in r.stderr
    # umx-batch: a 48 kHz file and a 44.1 kHz file in one pass
    batch = Path(pkg.HERE) / "umx-batch"
    r = subprocess.run([str(batch), path, str(tmp_path / "bout"), str(wav48), str(GOLD / "gspi_stereo.wav")], capture_output=True,
                       text=True, env={**env, "UMX_RESAMPLE": "1"}, timeout=600)
    assert r.returncode == 0, r.stderr
    x44, _ = pkg.wav_load(GOLD / "gspi_stereo.wav")
    eng2 = pkg.Engine.from_file(path, tracks=2)
    refs = eng2.separate_many([x48, x44], shift_offsets=[4033, 4033], rates=[48000, 44100])
    eng2.close()
    for name, want_rate, want in (("gspi48", 48000, refs[0]), ("gspi_stereo", 44100, refs[1])):
        for t in range(4):
            got, ch, rate = pkg.wav_load_rate(tmp_path / "bout" / name / f"target_{t}.wav")
            assert rate == want_rate and got.shape == want[t].shape
            assert np.array_equal(got, want[t]), (name, t)
    r = subprocess.run([str(batch), path, str(tmp_path / "bplain"), str(wav48)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 1 and "only supports the following sample rate (Hz): 44100" in r.stderr
