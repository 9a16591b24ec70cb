"""The progress callback of the device whole-track entry points (csrc/engine_tracks.h, include/umx_hip.h: "once per QUEUED
segment", umx.cpp:208,229): how often it runs and the float32 values it reports, for the one-lane context, several track lanes,
reset mode (UMX_FLAG_RESET_SEGMENTS: a call queues up to B segments of the one track, and reports each) and the shift ensemble.
The expected sequence is the reference's own arithmetic in float32: total = ceil(L2 / stride), done += 1 / total per segment of the
longest lane.  A callback must not change a stem bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: stride 12288
STRIDE = 12288
L = int(4.3 * N)
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def eng1(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wave(pkg):
    return np.ascontiguousarray(pkg.ggml.synth_audio(L, 77).T).ravel()


def _padded(length, shift):
    return length if shift is None else length + max(22050 - shift, shift)


def _expected(segments):
    """done after each of `segments` queued segments, as umx.cpp:208,229 form it in float32"""
    total = np.float32(segments)
    done, seq = np.float32(0), []
    for _ in range(segments):
        done = np.float32(done + np.float32(1) / total)
        seq.append(done)
    return np.array(seq, np.float32)


def _segments(length, shift):
    return -(-_padded(length, shift) // STRIDE)


class Progress:
    """A PROGRESS_FN that records what it is handed; .arg is what the C entry points take."""

    def __init__(self, pkg):
        self.seen = []
        self.fn = pkg.PROGRESS_FN(lambda p, _user: self.seen.append(p))
        self.arg = C.cast(self.fn, C.c_void_p)

    def check(self, expected, what):
        got = np.array(self.seen, np.float32)
        print(what, "callbacks", len(got), "expected", len(expected), "last", got[-1] if len(got) else None, "expected last", expected[-1])
        assert len(got) == len(expected), (what, len(got), len(expected), got)
        assert np.array_equal(got.view(np.uint32), expected.view(np.uint32)), (what, got, expected)


def _one_track(eng, a, length, shift, flags, progress):
    outs = [np.empty(2 * length, np.float32) for _ in range(4)]
    arr = (FP * 4)(*[o.ctypes.data_as(FP) for o in outs])
    cb = progress.arg if progress else None
    if shift is None:
        rc = eng.lib.umx_hip_split_inference(eng.h, a.ctypes.data_as(FP), length, arr, flags, cb, None)
    else:
        rc = eng.lib.umx_hip_shift_inference(eng.h, a.ctypes.data_as(FP), length, shift, arr, flags, cb, None)
    assert rc == 0, eng.last_error()
    return outs


@pytest.mark.parametrize("shift,segments", [(None, 6), (4033, 8)])
def test_carry_mode_reports_once_per_segment(pkg, eng1, wave, shift, segments):
    assert _segments(L, shift) == segments and (shift is None or _padded(L, shift) == 88468)
    p = Progress(pkg)
    got = _one_track(eng1, wave, L, shift, 0, p)
    p.check(_expected(segments), ("carry", shift))
    plain = _one_track(eng1, wave, L, shift, 0, None)
    for t in range(4):
        assert np.array_equal(got[t].view(np.uint32), plain[t].view(np.uint32)), (shift, t)


def test_three_lanes_report_once_per_call_of_the_longest_lane(pkg, eng3):
    lengths = [int(3.4 * N), N // 2, int(1.9 * N)]
    shifts = [4033, None, 700]
    ins = [np.ascontiguousarray(pkg.ggml.synth_audio(n, 300 + i).T).ravel() for i, n in enumerate(lengths)]
    outs = [[np.empty(2 * n, np.float32) for _ in range(4)] for n in lengths]
    a = (FP * 3)(*[x.ctypes.data_as(FP) for x in ins])
    o = (FP * 12)(*[x.ctypes.data_as(FP) for t4 in outs for x in t4])
    sh = (C.c_int * 3)(*[(-1 if s is None else s) for s in shifts])
    p = Progress(pkg)
    rc = eng3.lib.umx_hip_separate_tracks(eng3.h, 3, a, (C.c_int * 3)(*lengths), sh, o, 0, p.arg, None)
    assert rc == 0, eng3.last_error()
    calls = max(_segments(n, s) for n, s in zip(lengths, shifts))
    assert calls == 6
    p.check(_expected(calls), "three lanes")


@pytest.mark.parametrize("shift,segments", [(None, 6), (4033, 8)])
def test_reset_mode_reports_every_segment_of_a_call(pkg, eng3, wave, shift, segments):
    """3 lanes: the 8 segments go in passes of 3 + 3 + 2 (the 6 in 3 + 3); the sequence is carry mode's, count and bits."""
    p = Progress(pkg)
    _one_track(eng3, wave, L, shift, pkg.FLAG_RESET_SEGMENTS, p)
    p.check(_expected(segments), ("reset", shift))


def test_ensemble_reports_once_per_call_of_the_longer_lane(pkg, eng3, wave):
    offsets = [4033, 15058]
    outs = [np.empty(2 * L, np.float32) for _ in range(4)]
    arr = (FP * 4)(*[x.ctypes.data_as(FP) for x in outs])
    p = Progress(pkg)
    rc = eng3.lib.umx_hip_shift_ensemble(eng3.h, wave.ctypes.data_as(FP), L, pkg.MODEL_RATE, 2, (C.c_int * 2)(*offsets), arr, 0, p.arg,
                                         None)
    assert rc == 0, eng3.last_error()
    calls = max(_segments(L, s) for s in offsets)
    assert calls == 8
    p.check(_expected(calls), "ensemble")
