"""Track queue (csrc/engine_queue.h): umx_hip_separate_queue runs more tracks than the context has lanes through one
segment loop, a lane refilled with the next track the moment one ends.  Its definition is hard: every job's output is, bit for bit,
what the context returns for that job alone (Engine.separate / separate_mix on the SAME engine, with the same flags), and the run
makes exactly the calls umx_hip_queue_plan predicts.  Held to that here for a refill pattern with an exact stride multiple and one
sample more, mixed shift offsets, a one-sample job in a lane a long job just left, flags, a mix, the C entry point on guarded
buffers with the callback contract, the refusals, and umx-batch against its pass-by-pass loop.

Not tested: the recovery from a persistent-kernel timeout (the jobs in flight run again from their first segment).  Nothing here
provokes a timeout."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: stride 12288
STRIDE = 12288
LENGTHS = [9000, 55000, 20000, 24576, 24577, 1, 40000]
COUNTS = [1, 5, 2, 2, 3, 1, 4]
SHIFTS = [4033, None, 0, 22049, 700, None, 11025]
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def waves(pkg):
    return [pkg.ggml.synth_audio(L, 180 + i) for i, L in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def alone(eng3, waves):
    """Every job alone on the 3-lane engine, split mode: computed once, never changed."""
    return [eng3.separate(x) for x in waves]


def _bits_equal(got, want, what):
    assert len(got) == len(want), what
    for t in range(len(want)):
        assert got[t].shape == want[t].shape, (what, t)
        assert np.array_equal(got[t].view(np.uint32), want[t].view(np.uint32)), (what, t, float(np.abs(got[t] - want[t]).max()))


def _padded(length, shift):
    return length if shift is None else length + max(22050 - shift, shift)


def test_refill_seven_jobs_on_three_lanes(pkg, eng3, waves, alone):
    assert [len(pkg.segment_plan(L, N)[0]) for L in LENGTHS] == COUNTS  # 24576 = 2 strides exactly, 24577 one sample more
    assert pkg.queue_plan(3, COUNTS)[2] == 8
    runs = []
    for run in range(2):  # the second run meets the state and the accumulators the first one left behind
        got = eng3.separate_queue(waves)
        assert eng3.queue_calls() == 8
        for j in range(7):
            _bits_equal(got[j], alone[j], (run, j))
        runs.append(got)
    for j in range(7):
        _bits_equal(runs[1][j], runs[0][j], ("second run", j))
    assert all(np.abs(alone[1][t]).max() > 0 for t in range(4))  # (the stems are not silence)


def test_mixed_shifts(pkg, eng3, waves):
    counts = [len(pkg.segment_plan(_padded(L, s), N)[0]) for L, s in zip(LENGTHS, SHIFTS)]
    assert counts != COUNTS  # (the shift padding changes the segment counts)
    got = eng3.separate_queue(waves, shift_offsets=SHIFTS)
    assert eng3.queue_calls() == pkg.queue_plan(3, counts)[2]
    for j, (x, s) in enumerate(zip(waves, SHIFTS)):
        _bits_equal(got[j], eng3.separate(x, shift_offset=s), (j, s))


def test_one_sample_job_in_the_lane_a_long_job_left(pkg, model_small, waves):
    eng = pkg.Engine.from_file(model_small[0], N, tracks=1, lstm_batched=True)
    assert eng.lstm_is_batched()
    jobs = [waves[1], waves[5], waves[5]]  # 5 segments, then 1 sample (split), then 1 sample behind a shift: all on the one lane
    shifts = [None, None, 700]
    got = eng.separate_queue(jobs, shift_offsets=shifts)
    assert eng.queue_calls() == 5 + 1 + len(pkg.segment_plan(_padded(1, 700), N)[0])
    for j in range(3):
        _bits_equal(got[j], eng.separate(jobs[j], shift_offset=shifts[j]), j)
    eng.close()


def test_flags_and_mix(pkg, eng3, waves):
    idx = [0, 4, 5, 2]  # four jobs on three lanes: one refill
    jobs = [waves[i] for i in idx]
    shifts = [None, 4033, None, 0]
    for flags in (pkg.flags_for_targets(["vocals"], residual=True, softmask=True) | pkg.FLAG_WIENER_ITERS(2), pkg.FLAG_NO_WIENER):
        got = eng3.separate_queue(jobs, shift_offsets=shifts, flags=flags)
        for j in range(4):
            _bits_equal(got[j], eng3.separate(jobs[j], flags=flags, shift_offset=shifts[j]), (hex(flags), j))
    gains = [[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]]  # vocals, mix - vocals
    got = eng3.separate_queue(jobs, shift_offsets=shifts, mix=gains)
    for j in range(4):
        assert len(got[j]) == 2
        _bits_equal(got[j], eng3.separate_mix(jobs[j], gains, shift_offset=shifts[j]), ("mix", j))
    plain = eng3.separate_queue(jobs, shift_offsets=shifts)
    for j in range(4):  # (row 0 is 1 x vocals: the unmixed run's fourth stem, exactly)
        _bits_equal([got[j][0]], [plain[j][3]], ("vocals row", j))


class _CRun:
    """The C entry point on guarded host buffers: jobs handed out in order (`stop_at`: the request that answers -1)."""

    def __init__(self, pkg, waves, want, stop_at=None):
        self.pkg, self.want, self.stop_at = pkg, want, stop_at
        self.lay = [gd.track_layout(2 * w.shape[1]) for w in waves]
        self.ins = [gd.make(l, np.ascontiguousarray(w.T)) for l, w in zip(self.lay, waves)]
        self.ins_before = [a.copy() for a in self.ins]
        self.outs = [[gd.make(l) for _ in range(4)] for l in self.lay]
        self.requests, self.after_zero, self.taken, self.done, self.done_ok = 0, 0, [], [], []
        self.zero_seen = False

    def _ptr(self, words, lay):
        return C.cast(words.ctypes.data + 4 * lay.pre, FP)

    def next(self, _user, job):
        if self.zero_seen:
            self.after_zero += 1
            return 0
        j = self.requests
        self.requests += 1
        if self.stop_at is not None and j == self.stop_at:
            return -1
        if j >= len(self.lay):
            self.zero_seen = True
            return 0
        job[0].audio = self._ptr(self.ins[j], self.lay[j])
        job[0].length, job[0].shift_offset = self.lay[j].payload // 2, -1
        for t in range(4):
            job[0].out[t] = self._ptr(self.outs[j][t], self.lay[j])
        job[0].tag = j + 1
        self.taken.append(j)
        return 1

    def done_cb(self, _user, job):
        j = int(job[0].tag) - 1
        self.done.append(j)
        L = self.lay[j].payload // 2
        ok = job[0].length == L and job[0].shift_offset == -1
        for t in range(4):  # the data is complete NOW, not merely by the time the call returns
            got = gd.payload(self.outs[j][t], self.lay[j]).reshape(L, 2).T
            ok = ok and np.array_equal(got.view(np.uint32), self.want[j][t].view(np.uint32))
        self.done_ok.append(bool(ok))

    def run(self, eng, flags=0):
        return eng.lib.umx_hip_separate_queue(eng.h, self.pkg.QUEUE_NEXT_FN(self.next), self.pkg.QUEUE_DONE_FN(self.done_cb), None, 4, None, flags)

    def check_buffers(self, jobs):
        for j in jobs:
            assert gd.check(self.ins[j], self.lay[j], self.ins_before[j]).ok, j
            for t in range(4):
                rep = gd.check(self.outs[j][t], self.lay[j])
                assert rep.ok, (j, t, str(rep))  # exactly 2 * length floats written, none outside


def test_c_entry_point_on_guarded_buffers(pkg, eng3, waves, alone):
    r = _CRun(pkg, waves, alone)
    assert r.run(eng3) == 0, eng3.last_error()
    assert eng3.queue_calls() == 8
    assert r.taken == list(range(7)) and sorted(r.done) == list(range(7)) and len(r.done) == 7  # once per job
    assert all(r.done_ok), r.done_ok
    assert r.after_zero == 0  # next is not called again once it has returned 0
    assert r.requests == 8  # seven jobs and the one request that was answered 0
    r.check_buffers(range(7))


def test_refusals_leave_the_context_usable(pkg, model_small, eng3, waves, alone):
    x = waves[0]

    def refused(fn, word):
        with pytest.raises(pkg.UmxError) as e:
            fn()
        assert e.value.code == pkg.ERR_ARG and word in str(e.value), str(e.value)

    refused(lambda: eng3.separate_queue([x], flags=pkg.FLAG_RESET_SEGMENTS), "RESET_SEGMENTS")
    refused(lambda: eng3.separate_queue([x, np.zeros((2, 0), np.float32)]), "length >= 1")
    refused(lambda: eng3.separate_queue([x], shift_offsets=[22050]), "shift offset < 22050")
    one = pkg.Engine.from_file(model_small[0], N)
    assert not one.lstm_is_batched()
    refused(lambda: one.separate_queue([x]), "track-batched")
    _bits_equal(one.separate(x), one.separate(x), "unbatched context after the refusal")
    one.close()
    _bits_equal(eng3.separate(x), alone[0], "after the refusals")
    # next answers -1 at its fifth request (before call 2): job 0 (one segment, call 0) is complete by then and stays so
    r = _CRun(pkg, waves, alone, stop_at=4)
    assert r.run(eng3) == pkg.ERR_ARG
    assert "next" in eng3.last_error()
    assert r.taken == [0, 1, 2, 3] and r.done == [0] and r.done_ok == [True], (r.taken, r.done, r.done_ok)
    r.check_buffers([0])
    for j in (1, 2, 3):  # abandoned jobs: whatever was written stayed inside the buffers
        for t in range(4):
            rep = gd.check(r.outs[j][t], r.lay[j], r.outs[j][t])
            assert rep.pre is None and rep.post is None, (j, t, str(rep))
    _bits_equal(eng3.separate(waves[4]), alone[4], "a plain track after the stopped run")
    _bits_equal(eng3.separate_queue(waves[:4])[1], alone[1], "a queue run after the stopped run")


def test_umx_batch_queue_equals_its_pass_by_pass_loop(pkg, model_small, tmp_path):
    files = []
    for i, (secs, name) in enumerate(((20, "a/x.wav"), (100, "long.wav"), (50, "b/x.wav"), (20, "short.wav"))):
        p = tmp_path / name
        p.parent.mkdir(exist_ok=True)
        pkg.wav_write(p, pkg.ggml.synth_audio(secs * 44100, 300 + i))
        files.append(str(p))
    batch = Path(pkg.HERE) / "umx-batch"
    outs = {}
    for mode, env in (("queue", {}), ("loop", {"UMX_BATCH_QUEUE": "0"})):
        out = tmp_path / mode
        r = subprocess.run([str(batch), model_small[0], str(out)] + files, capture_output=True, text=True, timeout=600,
                           env={**os.environ, "UMX_BATCH_LANES": "2", **env})
        assert r.returncode == 0, r.stderr
        assert "Separated 4 file(s), 190.00 s of audio" in r.stdout and "2 track lanes" in r.stdout, r.stdout
        outs[mode] = out
    names = sorted(p.name for p in outs["loop"].iterdir())
    assert names == ["long", "short", "x", "x_2"] and sorted(p.name for p in outs["queue"].iterdir()) == names
    for name in names:
        for t in range(4):
            a, b = outs["queue"] / name / f"target_{t}.wav", outs["loop"] / name / f"target_{t}.wav"
            assert a.read_bytes() == b.read_bytes(), (name, t)
    # argument order names the directories: a/x.wav (20 s) is "x", b/x.wav (50 s) is "x_2"
    assert 20 * 44100 * 8 <= (outs["queue"] / "x" / "target_0.wav").stat().st_size < 50 * 44100 * 8 <= (outs["queue"] / "x_2" / "target_0.wav").stat().st_size
