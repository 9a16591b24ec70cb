"""Resampled tracks by range (csrc/resample.h, csrc/engine_tracks.h, csrc/engine_queue.h).

The kernel: a range of the outputs (umx_hip_resample_range_device) is bit for bit that range of the whole launch and writes nothing
else; ranges in any order tile the whole launch; umx_hip_resample_needs / _ready name exactly what a range reads (every other input
frame may be NaN -- a zero tap times NaN is NaN, so a read beyond the rule shows).
The drivers: a resampled track goes in and out by region (umx_hip_debug_resample_launches counts the launches) with the bits of
the composition resample -> separate -> resample; the track queue takes jobs at any rate, each bit for bit the one-track call on
the same engine, in the calls umx_hip_queue_plan predicts, with int16 buffers, levels, loudness and a mix; umx-batch with
UMX_RESAMPLE=1 goes through the queue.  Hidden 128, at most three lanes."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import resample_ref as rr

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
PAIRS = [(48000, 44100), (8000, 44100), (96000, 44100), (22050, 44100), (44056, 44100)]
PAIRS = PAIRS + [(b, a) for a, b in PAIRS]
IDS = [f"{a}-{b}" for a, b in PAIRS]
N_IN = 10007
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()
    return t


@pytest.fixture(scope="module")
def eng(pkg, model_small, torch):
    e = pkg.Engine(model_small[2], 128, 16 * 1024)
    yield e
    e.close()


def _block(rin, rout):
    """ResampleGeom.block by its documented rule: the largest even count of outputs, at most 2048, whose input span
    floor((B - 1) M / L) + 1 + K fits the 4096 frames a workgroup stages."""
    M, L, _, _, K = rr.geometry(rin, rout)
    b = 2048
    while b > 2 and (b - 1) * M // L + 1 + K > 4096:
        b -= 2
    return b


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (2, n)).astype(np.float32)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()).cuda()


class Guarded:
    """n_out frames on the device between guards (tests/guarded.py), FILL before every call."""

    def __init__(self, torch, n_out):
        self.lay = gd.track_layout(2 * n_out)
        self.before = gd.make(self.lay)
        self.pristine = torch.from_numpy(self.before).cuda()
        self.t = self.pristine.clone()
        self.n = n_out

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lay.pre

    def reset(self):
        self.t.copy_(self.pristine)

    def words(self):
        return self.t.cpu().numpy()

    def frames(self):
        """the payload as (n, 2) uint32 words, guards checked"""
        w = self.words()
        rep = gd.check(w, self.lay, w)
        assert rep.pre is None and rep.post is None, str(rep)
        return w[self.lay.body].view(np.uint32).reshape(self.n, 2)


FILL = np.uint32(np.int32(gd.FILL))


def _whole(torch, eng, xs, rin, rout, n_out):
    ins = [_dev(torch, x) for x in xs]
    outs = [Guarded(torch, n_out) for _ in xs]
    eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.ptr for o in outs], n_out)
    torch.cuda.synchronize()
    got = [o.frames() for o in outs]
    for g in got:
        assert not (g == FILL).any()
    return got


def _check_range(outs, whole, first, count, what):
    for b, o in enumerate(outs):
        g = o.frames()
        assert np.array_equal(g[first:first + count], whole[b][first:first + count]), (what, b)
        assert (g[:first] == FILL).all() and (g[first + count:] == FILL).all(), (what, b, "a frame outside the range was written")


@pytest.mark.parametrize("rin,rout", PAIRS, ids=IDS)
def test_ranges_equal_the_whole_launch_and_write_nothing_else(pkg, torch, eng, rin, rout):
    n_out = pkg.resampled_length(N_IN, rin, rout)
    block = _block(rin, rout)
    firsts = sorted({f for f in (0, 2, block - 2, block, block + 2, (n_out - 1) & ~1) if 0 <= f < n_out})
    for nb in (1, 4):
        xs = [_noise(N_IN, 100 + b) for b in range(nb)]
        whole = _whole(torch, eng, xs, rin, rout, n_out)
        ins = [_dev(torch, x) for x in xs]
        outs = [Guarded(torch, n_out) for _ in xs]
        for first in firsts:
            counts = sorted({min(c, n_out - first) for c in (1, 2, 3, block - 1, block + 1, 4099, n_out - first)})
            for count in counts:
                for o in outs:
                    o.reset()
                eng.resample_range_device(rin, rout, [t.data_ptr() for t in ins], N_IN, [o.ptr for o in outs], n_out, first, count)
                torch.cuda.synchronize()
                _check_range(outs, whole, first, count, (nb, first, count))
        # count == 0 launches nothing
        for o in outs:
            o.reset()
        eng.resample_range_device(rin, rout, [t.data_ptr() for t in ins], N_IN, [o.ptr for o in outs], n_out, firsts[-1], 0)
        torch.cuda.synchronize()
        assert all(gd.untouched(o.words(), o.before) is None for o in outs)


@pytest.mark.parametrize("rin,rout", PAIRS, ids=IDS)
def test_five_uneven_ranges_in_shuffled_order_tile_the_whole_launch(pkg, torch, eng, rin, rout):
    n_out = pkg.resampled_length(N_IN, rin, rout)
    xs = [_noise(N_IN, 200 + b) for b in range(4)]
    whole = _whole(torch, eng, xs, rin, rout, n_out)
    cuts = [0] + [int(n_out * f) & ~1 for f in (0.07, 0.31, 0.33, 0.8)] + [n_out]
    assert len(set(cuts)) == 6
    ins = [_dev(torch, x) for x in xs]
    outs = [Guarded(torch, n_out) for _ in xs]
    for k in (3, 0, 4, 2, 1):
        eng.resample_range_device(rin, rout, [t.data_ptr() for t in ins], N_IN, [o.ptr for o in outs], n_out, cuts[k], cuts[k + 1] - cuts[k])
    torch.cuda.synchronize()
    for b in range(4):
        assert np.array_equal(outs[b].frames(), whole[b]), b


@pytest.mark.parametrize("rin,rout", PAIRS, ids=IDS)
def test_needs_and_ready_name_everything_a_range_reads(pkg, torch, eng, rin, rout):
    n_out = pkg.resampled_length(N_IN, rin, rout)
    block = _block(rin, rout)
    D = rr.geometry(rin, rout)[3]
    x = _noise(N_IN, 300)
    (whole,) = _whole(torch, eng, [x], rin, rout, n_out)
    out = Guarded(torch, n_out)
    # needs: every input frame from needs(first + count) on is NaN
    for first, count in ((0, 1), (0, min(block + 1, n_out)), ((n_out // 2) & ~1, min(777, n_out - ((n_out // 2) & ~1))), (min(block, (n_out - 1) & ~1), 1)):
        need = pkg.resample_needs(first + count, rin, rout, N_IN)
        z = x.copy()
        z[:, need:] = np.nan
        out.reset()
        zd = _dev(torch, z)
        eng.resample_range_device(rin, rout, [zd.data_ptr()], N_IN, [out.ptr], n_out, first, count)
        torch.cuda.synchronize()
        _check_range([out], [whole], first, count, ("needs", first, count, need))
    # ready: every input frame from f on is NaN; outputs [0, ready(f)) are those of the clean launch
    for f in (D + 2, D + 3, 1000, N_IN // 2, N_IN - 1):
        r = pkg.resample_ready(f, rin, rout, N_IN, n_out)
        assert 0 < r < n_out, (f, r)
        z = x.copy()
        z[:, f:] = np.nan
        out.reset()
        zd = _dev(torch, z)
        eng.resample_range_device(rin, rout, [zd.data_ptr()], N_IN, [out.ptr], n_out, 0, r)
        torch.cuda.synchronize()
        _check_range([out], [whole], 0, r, ("ready", f, r))


def test_range_refusals_leave_the_outputs_untouched(pkg, torch, eng):
    rin, rout = 48000, 44100
    n_out = pkg.resampled_length(N_IN, rin, rout)
    x = _dev(torch, _noise(N_IN, 400))
    out = Guarded(torch, n_out)
    for r_in, first, count in ((rin, 1, 2), (rin, 3, 0), (rin, 0, n_out + 1), (rin, n_out & ~1, 3), (rin, -2, 4), (rin, 0, -1), (7000, 0, 4)):
        with pytest.raises(pkg.UmxError) as e:
            eng.resample_range_device(r_in, rout, [x.data_ptr()], N_IN, [out.ptr], n_out, first, count)
        assert e.value.code == pkg.ERR_ARG, (r_in, first, count)
    torch.cuda.synchronize()
    assert gd.untouched(out.words(), out.before) is None
    eng.resample_range_device(rin, rout, [x.data_ptr()], N_IN, [out.ptr], n_out, 0, 2)  # the context stays usable
    torch.cuda.synchronize()
    assert not (out.frames()[:2] == FILL).any()


# ---------------------------------------------------------------- the drivers
RATES = [44100, 48000, 8000, 44100, 48000]
SECONDS = [11, 100, 100, 50, 9]
SHIFTS = [4033, None, 100, 0, 22049]


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def waves(pkg):
    return [pkg.ggml.synth_audio(s * r, 500 + i) for i, (s, r) in enumerate(zip(SECONDS, RATES))]


@pytest.fixture(scope="module")
def alone(eng3, waves):
    """Every job alone on the three-lane engine at its rate and shift: computed once, never changed."""
    return [eng3.separate_many([x], rates=[r], shift_offsets=[s])[0] for x, r, s in zip(waves, RATES, SHIFTS)]


def _bits_equal(got, want, what):
    assert len(got) == len(want), what
    for t in range(len(want)):
        assert got[t].shape == want[t].shape and got[t].dtype == want[t].dtype, (what, t)
        assert np.ascontiguousarray(got[t]).tobytes() == np.ascontiguousarray(want[t]).tobytes(), (what, t)


def _segments(pkg, length, rate, shift):
    n44 = pkg.resampled_length(length, rate, 44100)
    return len(pkg.segment_plan(n44 if shift is None else n44 + max(22050 - shift, shift))[0])


def test_queue_at_mixed_rates(pkg, eng3, waves, alone):
    counts = [_segments(pkg, x.shape[1], r, s) for x, r, s in zip(waves, RATES, SHIFTS)]
    assert counts[1] == 3 and counts[2] == 3 and counts[0] == 1
    got = eng3.separate_queue(waves, shift_offsets=SHIFTS, rates=RATES)
    assert eng3.queue_calls() == pkg.queue_plan(3, counts)[2]
    for j in range(5):
        _bits_equal(got[j], alone[j], j)
    fwd, back = eng3.resample_launches()
    assert back == 3 + 3 + 1 and 3 < fwd <= 3 + 3 + 1, (fwd, back)  # the three resampled jobs, region by region
    assert all(np.abs(alone[2][t]).max() > 0 for t in range(4))  # (the stems are not silence)
    _bits_equal(eng3.separate_queue(waves[:2], shift_offsets=SHIFTS[:2])[0], alone[0], "no rates: 44.1 kHz jobs as before")


def test_queue_options_at_48k(pkg, eng3, waves):
    idx = [1, 4, 0, 4]  # four jobs on three lanes: one refill; 48 kHz / 100 s, 48 kHz / 9 s, 44.1 kHz / 11 s, 48 kHz / 9 s
    jobs, rates, shifts = [waves[i] for i in idx], [RATES[i] for i in idx], [4033, None, 7, 4033]
    nj = len(jobs)
    # int16 in and out, dithered
    io = pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16, dither_seed=5)
    jobs16 = [np.round(x * 30000).astype(np.int16) for x in jobs]
    got = eng3.separate_queue(jobs16, shift_offsets=shifts, io=io, rates=rates)
    for j in range(nj):
        want = eng3.separate_many_io([jobs16[j]], io=io, shift_offsets=[shifts[j]], rates=[rates[j]])[0]
        assert want[0].dtype == np.int16
        _bits_equal(got[j], want, ("s16", j))
    # levels and loudness
    got, lv, ld, env = eng3.separate_queue(jobs, shift_offsets=shifts, levels=True, loudness=True, rates=rates)
    for j in range(nj):
        want, wlv, wld, wenv = eng3.separate_many_loudness([jobs[j]], shift_offsets=[shifts[j]], rates=[rates[j]])
        _bits_equal(got[j], want[0], ("loudness", j))
        assert bytes(lv[j]) == bytes(wlv[0]) and bytes(ld[j]) == bytes(wld[0]), j
        assert env[j].shape == wenv[0].shape and np.array_equal(env[j].view(np.uint64), wenv[0].view(np.uint64)), j
    # a two-row mix
    gains = [[0, 0, 0, 1, 0], [0.5, 0.5, 0.5, 0, -0.25]]
    got = eng3.separate_queue(jobs, shift_offsets=shifts, mix=gains, rates=rates)
    for j in range(nj):
        assert len(got[j]) == 2
        _bits_equal(got[j], eng3.separate_many_mix([jobs[j]], gains, shift_offsets=[shifts[j]], rates=[rates[j]])[0], ("mix", j))
    # rescale: a job leaves whole, in one launch back
    got, lv = eng3.separate_queue(jobs[:2], shift_offsets=shifts[:2], clip=pkg.CLIP_RESCALE, rates=rates[:2])
    assert eng3.resample_launches()[1] == 2
    for j in range(2):
        want, wlv = eng3.separate_many_levels([jobs[j]], clip=pkg.CLIP_RESCALE, shift_offsets=[shifts[j]], rates=[rates[j]])
        _bits_equal(got[j], want[0], ("rescale", j))
        assert bytes(lv[j]) == bytes(wlv[0]), j


def _resample(torch, eng, xs, rin, rout, n_out):
    ins = [_dev(torch, x) for x in xs]
    outs = [torch.empty(2 * n_out, dtype=torch.float32, device="cuda") for _ in xs]
    eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.data_ptr() for o in outs], n_out)
    torch.cuda.synchronize()
    return [o.cpu().numpy().reshape(n_out, 2).T.copy() for o in outs]


def _composition(torch, pkg, eng, x, rate, offset, flags=0):
    """resample(rate <- 44100) of the n44 frames that shift_inference returns for resample(44100 <- rate) of x, on the device
    (tests/test_gpu_resample.py's helper, restated)."""
    n44 = pkg.resampled_length(x.shape[1], rate, 44100)
    (x44,) = _resample(torch, eng, [x], rate, 44100, n44)
    stems44 = eng.separate(x44, flags=flags, shift_offset=offset)
    return _resample(torch, eng, stems44, 44100, rate, x.shape[1])


def test_a_48k_track_leaves_by_region(pkg, model_small, torch, waves):
    x = waves[1]  # 48 kHz, 100 s: three segments
    e1 = pkg.Engine.from_file(model_small[0])
    assert e1.resample_launches() is None
    got = e1.separate(x, shift_offset=4033, rate=48000)
    fwd, back = e1.resample_launches()
    assert back == 3 and 1 < fwd <= 3, (fwd, back)
    _bits_equal(got, _composition(torch, pkg, e1, x, 48000, 4033), "composition")
    assert e1.resample_launches() == (0, 0)  # (the composition's whole-track call was at 44.1 kHz)
    res, _ = e1.separate_many_levels([x], clip=pkg.CLIP_RESCALE, shift_offsets=[4033], rates=[48000])
    assert e1.resample_launches()[1] == 1  # a rescaled track leaves whole: its divisor needs every peak
    assert res[0][0].shape == x.shape
    e1.separate(waves[0], shift_offset=4033)
    assert e1.resample_launches() == (0, 0)
    e1.close()
    e2 = pkg.Engine.from_file(model_small[0], tracks=2)
    y = waves[4]  # 48 kHz, 9 s
    ens = e2.separate_ensemble(y, offsets=[4033, 100], rate=48000)
    assert e2.resample_launches() == (1, 1)
    assert ens[0].shape == y.shape
    e2.close()


def test_reset_mode_at_48k_on_two_lanes(pkg, model_small, torch, waves):
    x = waves[1]
    e2 = pkg.Engine.from_file(model_small[0], tracks=2)
    got = e2.separate(x, flags=pkg.FLAG_RESET_SEGMENTS, shift_offset=4033, rate=48000)
    fwd, back = e2.resample_launches()
    assert back == 3 and 1 < fwd <= 3, (fwd, back)  # three segments over two calls
    _bits_equal(got, _composition(torch, pkg, e2, x, 48000, 4033, pkg.FLAG_RESET_SEGMENTS), "reset mode")
    e2.close()


def test_queue_refuses_a_rate_outside_the_range(pkg, eng3, waves, alone):
    order = [0, 1, 2, 4, 0]  # the fifth job is asked for before call 2: job 0 (one segment, call 0) is complete by then
    rates = [RATES[i] for i in order[:4]] + [7000]
    outs = [[np.full(2 * waves[i].shape[1], np.nan, np.float32) for _ in range(4)] for i in order]
    ins = [np.ascontiguousarray(waves[i].T).ravel() for i in order]
    taken, done = [], []

    def _next(_user, job):
        j = len(taken)
        if j >= len(order):
            return 0
        taken.append(j)
        job[0].audio = C.cast(ins[j].ctypes.data, FP)
        job[0].length = waves[order[j]].shape[1]
        job[0].shift_offset = -1 if SHIFTS[order[j]] is None else SHIFTS[order[j]]
        job[0].rate = rates[j]
        for t in range(4):
            job[0].out[t] = C.cast(outs[j][t].ctypes.data, FP)
        job[0].tag = j + 1
        return 1

    def _done(_user, job):
        done.append(int(job[0].tag) - 1)

    rc = eng3.lib.umx_hip_separate_queue(eng3.h, pkg.QUEUE_NEXT_FN(_next), pkg.QUEUE_DONE_FN(_done), None, 4, None, 0)
    assert rc == pkg.ERR_ARG
    assert "8000 .. 192000" in eng3.last_error(), eng3.last_error()
    assert taken == [0, 1, 2, 3, 4] and done == [0], (taken, done)
    L = waves[0].shape[1]
    _bits_equal([o.reshape(L, 2).T for o in outs[0]], alone[0], "the job that was complete")
    _bits_equal(eng3.separate_many([waves[4]], rates=[48000], shift_offsets=[SHIFTS[4]])[0], alone[4], "a track after the refusal")
    _bits_equal(eng3.separate_queue(waves[:2], shift_offsets=SHIFTS[:2], rates=RATES[:2])[1], alone[1], "a queue run after the refusal")


def test_umx_batch_with_resample_goes_through_the_queue(pkg, model_small, tmp_path):
    path = model_small[0]
    x44, _ = pkg.wav_load(GOLD / "gspi_stereo.wav")
    x48 = rr.resample(x44, 44100, 48000).astype(np.float32)
    files = [("a48", x48, 48000), ("b44", x44, 44100), ("c48", np.ascontiguousarray(x48[:, : x48.shape[1] // 2]), 48000)]
    for name, x, rate in files:
        pkg.wav_write(tmp_path / f"{name}.wav", x, rate=rate)
    batch = Path(pkg.HERE) / "umx-batch"
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_RESAMPLE": "1", "UMX_BATCH_LANES": "2"}
    outs = {}
    for mode, extra in (("queue", {}), ("loop", {"UMX_BATCH_QUEUE": "0"})):
        outs[mode] = tmp_path / mode
        r = subprocess.run([str(batch), path, str(outs[mode])] + [str(tmp_path / f"{n}.wav") for n, _, _ in files], capture_output=True,
                           text=True, env={**env, **extra}, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Separated 3 file(s)" in r.stdout and "2 track lanes" in r.stdout, r.stdout
    e2 = pkg.Engine.from_file(path, tracks=2)
    for name, x, rate in files:
        want = e2.separate(x, shift_offset=4033, rate=rate)
        for t in range(4):
            got, ch, got_rate = pkg.wav_load_rate(outs["queue"] / name / f"target_{t}.wav")
            assert ch == 2 and got_rate == rate and got.shape == x.shape, (name, t)
            assert np.array_equal(got.view(np.uint32), want[t].view(np.uint32)), (name, t)
            assert (outs["queue"] / name / f"target_{t}.wav").read_bytes() == (outs["loop"] / name / f"target_{t}.wav").read_bytes(), (name, t)
    e2.close()
