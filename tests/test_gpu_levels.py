"""Output levels and clip handling of the whole-track drivers (csrc/levels.h), bit for bit and without tolerances against
the rules of tests/levels_ref.py composed with what the fp32 calls return: the measuring kernel alone on guarded device buffers (the
record itself guarded), the rescaled encode and the in-place division, the drivers -- clamp with levels and rescale, int16 and fp32
outputs, dithered or not, over split and shifted tracks of one to three segments, lanes of unequal length, reset mode, flags, another
sample rate --, the queue, the no-op form, the refusals, and the CLIs."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import levels_ref as ref
import pcm16_ref as pcm

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
STRIDE = 12288
SEED = 7
ACC_WORDS = 28  # umx_levels_acc: 4 peak words, 3 x 4 64-bit counts
GRID_FRAMES = 1024 * 256  # frames the measuring kernel's largest grid covers in one pass (levels_blocks)
# synth_audio peaks at 0.5: the first row (3 mix, peak 1.5) clips, the second (0.25 mix) stays quiet, the third is a stem (vocals' slot)
GAINS = np.array([[0, 0, 0, 0, 3], [0, 0, 0, 0, 0.25], [0, 0, 0, 1, 0]], np.float32)
QUIET = np.ascontiguousarray(GAINS[1:])


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engines' streams exist
    return t


@pytest.fixture(scope="module")
def eng1(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wave(pkg):
    return pkg.ggml.synth_audio(25739, 71)


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = np.uint32 if g.dtype == np.float32 else np.uint16
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


def _frames(words):
    """n frame words -> (2, n) int16"""
    return np.ascontiguousarray(np.asarray(words, np.int32).view(np.int16).reshape(-1, 2).T)


KEYS = ("peak_bits", "over_unity", "clipped", "nonfinite")


def _acc_words(recs):
    """per-buffer records (dicts of levels_ref) -> the 28 words of a umx_levels_acc"""
    a = np.zeros(ACC_WORDS, np.uint32)
    for m, r in enumerate(recs):
        a[m] = r["peak_bits"]
        for q, k in enumerate(KEYS[1:]):
            a[4 + 8 * q + 2 * m] = r[k] & 0xFFFFFFFF
            a[4 + 8 * q + 2 * m + 1] = r[k] >> 32
    return a.view(np.int32)


def _same_levels(lv, recs, g, what):
    """a Levels of a call against the per-buffer records and the gain of the reference"""
    assert lv.n_out == len(recs), (what, lv.n_out)
    got = [{"peak_bits": int(np.float32(lv.peak[m]).view(np.uint32)), "over_unity": int(lv.over_unity[m]), "clipped": int(lv.clipped[m]),
            "nonfinite": int(lv.nonfinite[m])} for m in range(len(recs))]
    assert got == [{k: r[k] for k in KEYS} for r in recs], (what, got, recs)
    assert np.float32(lv.gain).view(np.uint32) == np.float32(g).view(np.uint32), (what, lv.gain, g)
    for m in range(len(recs), 4):
        assert (lv.peak[m], lv.over_unity[m], lv.clipped[m], lv.nonfinite[m]) == (0, 0, 0, 0), (what, m)


# ---------------------------------------------------------------- the kernels alone
class Buf:
    """A guarded device buffer of `words` 32-bit words (tests/guarded.py): the words given, or FILL."""

    def __init__(self, torch, words, data=None, misalign=0):
        self.lay = gd.track_layout(words, misalign)
        self.before = gd.make(self.lay)
        if data is not None:
            self.before[self.lay.body] = np.asarray(data).view(np.int32).ravel()
        self.t = torch.from_numpy(self.before).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lay.pre

    def result(self):
        """guards intact -> the payload's words"""
        words = self.t.cpu().numpy()
        rep = gd.check(words, self.lay, expect=words)
        assert rep.pre is None and rep.post is None, str(rep)
        return np.array(words[self.lay.body])

    def unchanged(self):
        return gd.untouched(self.t.cpu().numpy(), self.before) is None


def _record(torch, words=None):
    return Buf(torch, ACC_WORDS, np.zeros(ACC_WORDS, np.int32) if words is None else words)


def _floats(seed, n, awkward=True):
    """(2, n) fp32: audio-like noise, some of it beyond full scale, and the awkward values of the CPU test where they fit"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2, n)) * 0.4).astype(np.float32)
    x[:, ::5] *= 4
    if awkward:
        a = ref.awkward_floats()
        k = min(a.shape[1], n)
        pos = rng.permutation(n)[:k]
        x[:, pos] = a[:, rng.permutation(a.shape[1])[:k]]
    return x


def _inputs(torch, xs, off):
    return [Buf(torch, 2 * x.shape[1], np.ascontiguousarray(x.T), misalign=8 * (1 - off)) for x in xs]


FORMS = [(False, None, 0), (True, None, 0), (True, 5, 12345), (True, 5, 0), (True, None, 12345)]  # s16, dither seed, first_frame


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4099, GRID_FRAMES + 77])
def test_levels_kernel_alone(pkg, torch, eng1, n):
    forms = FORMS if n < 100000 else FORMS[2:3]
    for off in (0, 1):  # pointers offset by one frame: 8-byte aligned
        for nb in (1, 4):
            xs = [_floats(1000 * n + 10 * b + off, n + off) for b in range(nb)]
            ins = _inputs(torch, xs, off)
            for s16, seed, first in forms:
                acc = _record(torch)
                io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16 if s16 else pkg.SAMPLE_F32, seed)
                eng1.levels_device([b.ptr + 8 * off for b in ins], n, acc.ptr, first, io)
                torch.cuda.synchronize()
                want = [ref.levels(x[:, off:], b, first, s16, seed) for b, x in enumerate(xs)]
                assert np.array_equal(acc.result(), _acc_words(want)), (n, off, nb, s16, seed, first, acc.result(), want)
            assert all(b.unchanged() for b in ins)


def test_peak_position_sign_channel_and_buffer(pkg, torch, eng1):
    n = 700  # three workgroups
    for nb in (1, 4):
        for b in range(nb):
            for frame in (0, n - 1, 255, 256):
                for ch in (0, 1):
                    for sign in (1.0, -1.0):
                        xs = [np.full((2, n), 0.125, np.float32) for _ in range(nb)]
                        xs[b][ch, frame] = sign * 1.75
                        ins = _inputs(torch, xs, 1)
                        acc = _record(torch)
                        eng1.levels_device([i.ptr for i in ins], n, acc.ptr, 0, pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16))
                        torch.cuda.synchronize()
                        got = acc.result().view(np.uint32)
                        want = [ref.levels(x, m, 0, True) for m, x in enumerate(xs)]
                        assert np.array_equal(got.view(np.int32), _acc_words(want)), (nb, b, frame, ch, sign)
                        assert got[b] == np.float32(1.75).view(np.uint32) and want[b]["over_unity"] == want[b]["clipped"] == 1


def test_record_accumulates_over_three_launches(pkg, torch, eng1):
    n = 3000
    xs = [_floats(50 + b, n) for b in range(4)]
    ins = _inputs(torch, xs, 1)
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)
    acc = _record(torch)
    cuts = [0, 1, 1234, n]
    for a, b in zip(cuts[:-1], cuts[1:]):  # consecutive spans of the track, each at its frame number
        eng1.levels_device([i.ptr + 8 * a for i in ins], b - a, acc.ptr, 100 + a, io)
    torch.cuda.synchronize()
    want = [ref.levels(x, m, 100, True, SEED) for m, x in enumerate(xs)]
    assert np.array_equal(acc.result(), _acc_words(want))
    # a record that is not zero is added to, not overwritten
    again = _record(torch, _acc_words(want))
    eng1.levels_device([ins[0].ptr], n, again.ptr, 100, io)
    torch.cuda.synchronize()
    twice = [ref.add(want[0], want[0])] + want[1:]
    assert np.array_equal(again.result(), _acc_words(twice))


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_rescale_kernels(pkg, torch, eng1, n):
    for nb in (1, 4):
        for kind in ("loud", "quiet", "inf"):
            xs = [_floats(7 * n + b, n + 1, awkward=False) for b in range(nb)]
            xs[0][0, 1 + n // 3] = -1.625  # (beyond full scale whatever the noise)
            if kind == "quiet":
                xs = [np.clip(x, -0.99, 0.99) for x in xs]
            if kind == "inf":
                xs[-1][1, 1 + n // 2] = -np.inf
            measured = [ref.levels(x[:, 1:], b) for b, x in enumerate(xs)]
            g = ref.gain([r["peak"] for r in measured])
            assert (g > 1) == (kind == "loud")
            for seed, first in ((None, 0), (SEED, 12345)):
                ins = _inputs(torch, xs, 1)
                acc = _record(torch)
                eng1.levels_device([b.ptr + 8 for b in ins], n, acc.ptr, first)  # (an fp32 measurement: clipped is the encode's)
                outs = [Buf(torch, n + 1) for _ in range(nb)]
                eng1.pcm16_encode_rescaled_device([b.ptr + 8 for b in ins], n, [o.ptr + 4 for o in outs], acc.ptr, first, seed)
                torch.cuda.synchronize()
                res = [o.result() for o in outs]
                assert all(r[0] == gd.FILL for r in res), "the encode wrote in front of its n frames"
                want = [pcm.encode(ref.rescaled(x[:, 1:], g), b, first, seed) for b, x in enumerate(xs)]
                _same([_frames(r[1:]) for r in res], want, (n, nb, kind, seed))
                if kind != "loud":  # divisor 1: the plain encode's bits
                    plain = [Buf(torch, n + 1) for _ in range(nb)]
                    eng1.pcm16_encode_device([b.ptr + 8 for b in ins], n, [o.ptr + 4 for o in plain], first, seed)
                    torch.cuda.synchronize()
                    _same([_frames(o.result()[1:]) for o in plain], want, (n, nb, kind, seed, "plain"))
                recs = [ref.levels(x[:, 1:], b, first, True, seed, g) for b, x in enumerate(xs)]
                assert np.array_equal(acc.result(), _acc_words(recs)), (n, nb, kind, seed)
                assert (sum(r["clipped"] for r in recs) > 0) == (kind == "inf"), (n, nb, kind)  # only a divisor of 1 lets a sample clamp
                assert all(b.unchanged() for b in ins)
                # the division in place
                before = acc.result()
                eng1.rescale_device([b.ptr + 8 for b in ins], n, acc.ptr)
                torch.cuda.synchronize()
                for b, x in zip(ins, xs):
                    words = b.result()
                    assert np.array_equal(words[:2], np.ascontiguousarray(x.T).view(np.int32).ravel()[:2]), "the division wrote in front"
                    _same([np.ascontiguousarray(words[2:].view(np.float32).reshape(n, 2).T)], [ref.rescaled(x[:, 1:], g)], (n, nb, kind, "in place"))
                assert np.array_equal(acc.result(), before)


def test_device_form_refusals_write_nothing(pkg, torch, eng1):
    src, dst, acc = Buf(torch, 128, np.zeros(128, np.float32)), Buf(torch, 64), _record(torch)
    for what, call in (("levels n 0", lambda: eng1.levels_device([src.ptr], 0, acc.ptr)),
                       ("levels null in", lambda: eng1.levels_device([0], 8, acc.ptr)),
                       ("levels null record", lambda: eng1.levels_device([src.ptr], 8, 0)),
                       ("levels 5 buffers", lambda: eng1.levels_device([src.ptr] * 5, 8, acc.ptr)),
                       ("levels first_frame < 0", lambda: eng1.levels_device([src.ptr], 8, acc.ptr, -1)),
                       ("encode null out", lambda: eng1.pcm16_encode_rescaled_device([src.ptr], 8, [0], acc.ptr)),
                       ("encode null record", lambda: eng1.pcm16_encode_rescaled_device([src.ptr], 8, [dst.ptr], 0)),
                       ("encode n 0", lambda: eng1.pcm16_encode_rescaled_device([src.ptr], 0, [dst.ptr], acc.ptr)),
                       ("rescale null", lambda: eng1.rescale_device([0], 8, acc.ptr)),
                       ("rescale null record", lambda: eng1.rescale_device([src.ptr], 8, 0)),
                       ("rescale no buffers", lambda: eng1.rescale_device([], 8, acc.ptr))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
    torch.cuda.synchronize()
    assert src.unchanged() and dst.unchanged() and acc.unchanged()


# ---------------------------------------------------------------- whole tracks
def _plain(eng, waves, gains, **kw):
    return eng.separate_many_mix(waves, gains, **kw) if gains is not None else eng.separate_many(waves, **kw)


def _drive(pkg, eng, waves, what, gains=GAINS, loud=True, **kw):
    """Every form of the levels call for the fp32 tracks `waves` against the rules applied to what the fp32 call returns for the same
    arguments: clamp with levels and rescale; fp32 and int16 outputs, the latter plain and dithered.  Returns the fp32 call's result."""
    plain = _plain(eng, waves, gains, **kw)
    for clip in (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE):
        for s16, seed in ((False, None), (True, None), (True, SEED)):
            io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16 if s16 else pkg.SAMPLE_F32, seed)
            outs, lvs = eng.separate_many_levels(waves, clip, io, gains=gains, **kw)
            for ln, stems in enumerate(plain):
                recs, g, left = ref.track(stems, s16, seed, clip == pkg.CLIP_RESCALE)
                tag = (what, "rescale" if clip else "clamp", s16, seed, ln)
                _same_levels(lvs[ln], recs, g, tag)
                _same(outs[ln], left, tag)
                if loud and gains is GAINS:  # conditions: the first row clips, the quiet one does not
                    assert recs[0]["over_unity"] > 0 and recs[1]["over_unity"] == 0 and recs[1]["clipped"] == 0, tag
                    assert (recs[0]["clipped"] > 0) == (s16 and not clip) and (g > 1) == bool(clip), tag
    return plain


def test_the_inputs_clip_in_two_regions(pkg, eng1, wave):
    """the condition of every driver test below, on the fp32 call's own result: the 3 x mix row passes full scale -- and its int16
    encode clamps -- in at least two regions of the three-segment track; the quiet row never does"""
    plain = eng1.separate_many_mix([wave], GAINS, shift_offsets=[None])[0]
    loud = [ref.levels(plain[0][:, a:a + STRIDE], 0, a, True) for a in range(0, wave.shape[1], STRIDE)]
    assert len(loud) == 3 and sum(1 for r in loud if r["over_unity"] > 0 and r["clipped"] > 0) >= 2, loud
    quiet = ref.levels(plain[1], 1, 0, True)
    assert quiet["over_unity"] == 0 and quiet["clipped"] == 0 and quiet["peak"] > 0
    assert np.abs(plain[2]).max() > 0


@pytest.mark.parametrize("length", [12288, 12289, 25739])
def test_split_and_shifted_tracks(pkg, eng1, wave, length):
    x = np.ascontiguousarray(wave[:, 300:300 + length] if length < 25739 else wave)
    for shift in (None, 0, 11025, 22049):
        _drive(pkg, eng1, [x], (length, shift), shift_offsets=[shift])


def test_three_lanes_of_unequal_length(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 3000:3000 + 9000]), np.ascontiguousarray(wave[:, 500:500 + 20000])]
    _drive(pkg, eng3, xs, "lanes", shift_offsets=[11025, None, 0])
    _drive(pkg, eng3, xs[1:], "two of three lanes", shift_offsets=[22049, None])


def test_reset_mode(pkg, eng3, wave):
    for shift in (None, 11025):
        _drive(pkg, eng3, [wave], ("reset", shift), flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])
    long = np.ascontiguousarray(np.concatenate([wave, wave[:, ::-1]], axis=1))  # more segments than lanes: two calls of the segment loop
    assert len(pkg.segment_plan(long.shape[1] + 22050, N)[0]) > 3
    _drive(pkg, eng3, [long], "reset, two calls", flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[0])


def test_flags_and_another_rate(pkg, eng1, wave):
    _drive(pkg, eng1, [wave], "no wiener", flags=pkg.FLAG_NO_WIENER, shift_offsets=[4033])
    _drive(pkg, eng1, [wave], "vocals + residual", flags=pkg.flags_for_targets(["vocals"], residual=True), shift_offsets=[4033])
    x48 = pkg.ggml.synth_audio(48000, 73)  # one second at 48 kHz
    plain = _drive(pkg, eng1, [x48], "48 kHz", shift_offsets=[4033], rates=[48000])
    assert all(s.shape == x48.shape for s in plain[0])
    _drive(pkg, eng1, [wave], "four stems", gains=None, loud=False, shift_offsets=[4033])  # no mix: four records


def test_a_quiet_track_rescales_to_the_clamp_bits(pkg, eng1, wave):
    plain = _drive(pkg, eng1, [wave], "quiet", gains=QUIET, loud=False, shift_offsets=[4033])
    assert max(float(np.abs(s).max()) for s in plain[0]) < 1 / 1.01
    for s16 in (False, True):
        io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16 if s16 else pkg.SAMPLE_F32, SEED if s16 else None)
        a, la = eng1.separate_many_levels([wave], pkg.CLIP_CLAMP, io, gains=QUIET, shift_offsets=[4033])
        b, lb = eng1.separate_many_levels([wave], pkg.CLIP_RESCALE, io, gains=QUIET, shift_offsets=[4033])
        _same(b[0], a[0], ("quiet", s16))
        assert la[0].gain == lb[0].gain == 1.0 and bytes(la[0]) == bytes(lb[0])


def test_queue_jobs_equal_the_single_track_call(pkg, eng2, wave):
    lengths, shifts = [5000, 12289, 25739, 1, 20000], [None, None, None, None, 11025]
    xs = [np.ascontiguousarray(wave[:, 40 * i:40 * i + n]) for i, n in enumerate(lengths)]
    segs = [len(pkg.segment_plan(n + (0 if s is None else max(22050 - s, s)), N)[0]) for n, s in zip(lengths, shifts)]
    assert segs == [1, 2, 3, 1, 3], segs
    plain = eng2.separate_queue(xs, shift_offsets=shifts, mix=GAINS)
    for clip in (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE):
        for s16, seed in ((True, SEED), (False, None)):
            io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16 if s16 else pkg.SAMPLE_F32, seed)
            got, lvs = eng2.separate_queue(xs, shift_offsets=shifts, mix=GAINS, io=io, clip=clip, levels=True)  # (done once per job: asserted there)
            assert eng2.queue_calls() == pkg.queue_plan(2, segs)[2]
            for j, (x, s) in enumerate(zip(xs, shifts)):
                one, lv1 = eng2.separate_many_levels([x], clip, io, gains=GAINS, shift_offsets=[s])
                _same(got[j], one[0], ("queue job", clip, s16, j))
                assert bytes(lvs[j]) == bytes(lv1[0]), ("queue job's levels", clip, s16, j)
                recs, g, left = ref.track(plain[j], s16, seed, clip == pkg.CLIP_RESCALE)
                _same(got[j], left, ("queue job against the rule", clip, s16, j))
                _same_levels(lvs[j], recs, g, ("queue", clip, s16, j))
    again = eng2.separate_queue(xs, shift_offsets=shifts, mix=GAINS)  # the plain queue afterwards is what it was
    for j in range(len(xs)):
        _same(again[j], plain[j], ("queue afterwards", j))


# ---------------------------------------------------------------- no-ops and refusals
def _c_call(pkg, eng, audio_ptrs, lengths, shifts, out_ptrs, io, clip, levels, n_out=4, gains=None):
    nt = len(lengths)
    a = None if audio_ptrs is None else (C.c_void_p * nt)(*audio_ptrs)
    o = None if out_ptrs is None else (C.c_void_p * len(out_ptrs))(*out_ptrs)
    return eng.lib.umx_hip_separate_tracks_levels(eng.h, nt, a, (C.c_int * nt)(*lengths), None, (C.c_int * nt)(*shifts), n_out,
                                                  None if gains is None else gains.ctypes.data_as(pkg._fp), o, 0,
                                                  None if io is None else C.byref(io), clip, levels, None, None)


def test_clamp_without_levels_is_the_io_call(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 1000:14000])]
    shifts = [4033, None]
    for io in (pkg.sample_io(), pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)):
        for gains in (None, GAINS):
            want = eng3.separate_many_io(xs, io=io, shift_offsets=shifts, gains=gains)
            got, lv = eng3.separate_many_levels(xs, pkg.CLIP_CLAMP, io, shift_offsets=shifts, gains=gains, levels=False)
            assert lv is None
            for ln in range(2):
                _same(got[ln], want[ln], ("no-op", ln))
            got, lv = eng3.separate_many_levels(xs, pkg.CLIP_CLAMP, io, shift_offsets=shifts, gains=gains)  # measuring changes no bit
            for ln in range(2):
                _same(got[ln], want[ln], ("clamp with levels", ln))
    # io == NULL
    ins = [np.ascontiguousarray(x.T) for x in xs]
    outs = [[np.empty((x.shape[1], 2), np.float32) for _ in range(4)] for x in xs]
    assert _c_call(pkg, eng3, [a.ctypes.data for a in ins], [x.shape[1] for x in xs], [4033, -1], [o.ctypes.data for t4 in outs for o in t4], None,
                   pkg.CLIP_CLAMP, None) == 0, eng3.last_error()
    usual = eng3.separate_many(xs, shift_offsets=shifts)
    for ln in range(2):
        _same([np.ascontiguousarray(o.T) for o in outs[ln]], usual[ln], ("io NULL", ln))


def test_refusals_leave_the_context_usable(pkg, eng3, wave):
    usual = eng3.separate_many([wave], shift_offsets=[4033])[0]
    n = wave.shape[1]
    a = np.ascontiguousarray(wave.T)
    outs = [np.full(2 * n, 0x5A5A, np.int16) for _ in range(4)]
    op = [o.ctypes.data for o in outs]
    S16, F32 = pkg.SAMPLE_S16, pkg.SAMPLE_F32
    lv = (pkg.Levels * 1)()
    cases = [("clip mode 2", [a.ctypes.data], op, pkg.SampleIO(F32, S16, 0, 0), 2, "clip mode"),
             ("clip mode -1", [a.ctypes.data], op, None, -1, "clip mode"),
             ("unknown output format", [a.ctypes.data], op, pkg.SampleIO(F32, 7, 0, 0), pkg.CLIP_RESCALE, "format"),
             ("dither with an fp32 output", [a.ctypes.data], op, pkg.SampleIO(F32, F32, 1, 3), pkg.CLIP_RESCALE, "dither"),
             ("null audio", [None], op, pkg.SampleIO(F32, S16, 0, 0), pkg.CLIP_RESCALE, "audio"),
             ("a null output", [a.ctypes.data], [op[0], None, op[2], op[3]], pkg.SampleIO(F32, S16, 0, 0), pkg.CLIP_CLAMP, "outputs")]
    for what, ap, outp, io, clip, word in cases:
        assert _c_call(pkg, eng3, ap, [n], [4033], outp, io, clip, lv) == pkg.ERR_ARG, what
        assert word in eng3.last_error(), (what, eng3.last_error())
        assert all(np.all(o == 0x5A5A) for o in outs) and bytes(lv[0]) == bytes(C.sizeof(pkg.Levels)), what
        _same(eng3.separate_many([wave], shift_offsets=[4033])[0], usual, ("fp32 after", what))
    bad_gains = np.full((1, 5), np.nan, np.float32)
    assert _c_call(pkg, eng3, [a.ctypes.data], [n], [4033], op, None, pkg.CLIP_RESCALE, lv, 1, bad_gains) == pkg.ERR_ARG and "mix" in eng3.last_error()
    nxt = pkg.QUEUE_NEXT_FN(lambda u, j: 0)
    done = pkg.QUEUE_LEVELS_FN(lambda u, j, l: None)
    for io, clip, word in ((None, 3, "clip mode"), (pkg.SampleIO(F32, 9, 0, 0), 0, "format")):
        assert eng3.lib.umx_hip_separate_queue_levels(eng3.h, nxt, done, None, 4, None, 0, None if io is None else C.byref(io), clip) == pkg.ERR_ARG
        assert word in eng3.last_error()
    assert eng3.lib.umx_hip_separate_queue_levels(eng3.h, nxt, pkg.QUEUE_LEVELS_FN(), None, 4, None, 0, None, 0) == pkg.ERR_ARG
    assert eng3.lib.umx_hip_separate_tracks_levels(None, 1, None, None, None, None, 4, None, None, 0, None, 0, None, None, None) == pkg.ERR_ARG
    _same(eng3.separate_many([wave], shift_offsets=[4033])[0], usual, "fp32 after the refusals")


def test_refusal_precedence(pkg, eng1, wave):
    """Several bad options in ONE call: every whole-track and queue entry point refuses the sample formats first, then the clip mode, then
    the gains, in the words each check has always used (recorded from the library before the entry points shared their checks).  Nothing
    is written, no callback runs, and the next plain call gives the usual bits."""
    FORMAT, CLIP, MIX = "sample io: unknown sample format", "clip mode: unknown", "mix: need 1 <= n_out <= 4 rows of five finite gains"
    usual = eng1.separate_many([wave], shift_offsets=[4033])[0]
    n = wave.shape[1]
    a = np.ascontiguousarray(wave.T)
    outs = [np.full(2 * n, 0x5A5A, np.int16) for _ in range(4)]
    ap, op = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 4)(*[o.ctypes.data for o in outs])
    ln, sh = (C.c_int * 1)(n), (C.c_int * 1)(4033)
    lv, ld = (pkg.Levels * 1)(), (pkg.Loudness * 1)()
    hop = np.full(4 * 2 * (n // 4410 + 1), 7.0)
    hp = (C.c_void_p * 1)(hop.ctypes.data)
    nan = np.full((1, 5), np.nan, np.float32)
    gp = nan.ctypes.data_as(pkg._fp)
    bad_io, good_io = pkg.SampleIO(pkg.SAMPLE_F32, 7, 0, 0), pkg.SampleIO(pkg.SAMPLE_F32, pkg.SAMPLE_S16, 0, 0)
    called = []
    nxt = pkg.QUEUE_NEXT_FN(lambda u, j: called.append("next") or 0)
    done = {"io": pkg.QUEUE_DONE_FN(lambda u, j: called.append("done")), "levels": pkg.QUEUE_LEVELS_FN(lambda u, j, l: called.append("done")),
            "loudness": pkg.QUEUE_LOUDNESS_FN(lambda u, j, l, d, e: called.append("done"))}
    lib, h = eng1.lib, eng1.h

    def tracks(rung, io, clip):
        head = (h, 1, ap, ln, None, sh, 1, gp, op, 0, C.byref(io))
        tail = {"io": (), "levels": (clip, lv), "loudness": (clip, lv, ld, hp)}[rung]
        return getattr(lib, "umx_hip_separate_tracks_" + rung)(*head, *tail, None, None)

    def queue(rung, io, clip):
        return getattr(lib, "umx_hip_separate_queue_" + rung)(h, nxt, done[rung], None, 1, gp, 0, C.byref(io), *(() if rung == "io" else (clip,)))

    cases = [(call, rung, *c) for call in (tracks, queue) for rung in ("levels", "loudness")
             for c in ((bad_io, 2, FORMAT), (good_io, 2, CLIP), (good_io, pkg.CLIP_RESCALE, MIX))]
    cases += [(call, "io", bad_io, None, FORMAT) for call in (tracks, queue)]
    for call, rung, io, clip, words in cases:
        what = (call.__name__, rung, words)
        assert call(rung, io, clip) == pkg.ERR_ARG, what
        assert eng1.last_error().startswith(words), (what, eng1.last_error())
        assert all(np.all(o == 0x5A5A) for o in outs) and np.all(hop == 7.0) and not called, what
        assert bytes(lv[0]) == bytes(C.sizeof(pkg.Levels)) and bytes(ld[0]) == bytes(C.sizeof(pkg.Loudness)), what
        _same(eng1.separate_many([wave], shift_offsets=[4033])[0], usual, ("fp32 after", what))


# ---------------------------------------------------------------- the CLIs
MIX_SPEC = "loud=3*mix;quiet=0.25*mix;vocals=vocals"  # GAINS as UMX_MIX
MIX_FILES = ["loud.wav", "quiet.wav", "vocals.wav"]
LINE = re.compile(r"^levels (\S+) peak=(\S+) over_unity=(\d+) clipped=(\d+) nonfinite=(\d+) gain=(\S+)$", re.M)


def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def _check_dir(pkg, stdout, dfloat, dgot, s16, seed, rescale, want_lines=True):
    """the directory dgot of one input file against the rules applied to the files of the clamp fp32 run in dfloat, and the printed
    lines of its files against the levels of those"""
    outs = [pkg.wav_load_rate(Path(dfloat) / f)[0] for f in MIX_FILES]
    recs, g, left = ref.track(outs, s16, seed, rescale)
    assert recs[0]["over_unity"] > 0 and recs[1]["over_unity"] == 0 and (g > 1) == rescale, (recs, g)  # conditions: the input clips
    lines = {m[0]: m[1:] for m in LINE.findall(stdout)}
    for m, f in enumerate(MIX_FILES):
        got = pkg.wav_load_pcm16(Path(dgot) / f)[0] if s16 else pkg.wav_load_rate(Path(dgot) / f)[0]
        _same([got], [left[m]], (str(dgot), f))
        if want_lines:
            want = ("%.9g" % recs[m]["peak"], str(recs[m]["over_unity"]), str(recs[m]["clipped"]), str(recs[m]["nonfinite"]), "%.9g" % g)
            assert lines.get(str(Path(dgot) / f)) == want, (f, lines, want)
    return recs


def test_cli_clip_and_levels(pkg, model_small, tmp_path):
    path, wav, cli = model_small[0], GOLD / "gspi_stereo.wav", Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": MIX_SPEC}
    r = _run(cli, [path, wav, tmp_path / "f"], env)
    assert r.returncode == 0 and "levels " not in r.stdout, r.stderr
    for name, extra, s16, seed, rescale in (("r16", {"UMX_PCM16": "1", "UMX_CLIP": "rescale", "UMX_LEVELS": "1"}, True, None, True),
                                            ("c16", {"UMX_PCM16": "1", "UMX_PCM16_DITHER": "7", "UMX_CLIP": "clamp", "UMX_LEVELS": "1"}, True, 7, False),
                                            ("rf", {"UMX_CLIP": "rescale", "UMX_LEVELS": "1"}, False, None, True),
                                            ("cf", {"UMX_LEVELS": "1"}, False, None, False)):
        r = _run(cli, [path, wav, tmp_path / name], env, **extra)
        assert r.returncode == 0, r.stderr
        assert len(LINE.findall(r.stdout)) == 3, r.stdout
        recs = _check_dir(pkg, r.stdout, tmp_path / "f", tmp_path / name, s16, seed, rescale)
        assert (recs[0]["clipped"] > 0) == (s16 and not rescale)
    r = _run(cli, [path, wav, tmp_path / "quietly"], env, UMX_CLIP="rescale")  # rescale without the lines
    assert r.returncode == 0 and "levels " not in r.stdout, r.stderr
    _check_dir(pkg, "", tmp_path / "f", tmp_path / "quietly", False, None, True, want_lines=False)
    for extra, word in (({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"), ({"UMX_CLI_PER_SEGMENT": "1", "UMX_MIX": ""}, "UMX_CLI_PER_SEGMENT")):
        for knob in ({"UMX_CLIP": "rescale"}, {"UMX_LEVELS": "1"}):
            r = _run(cli, [path, wav, tmp_path / "no"], env, **knob, **extra)
            assert r.returncode == 1 and "UMX_CLIP / UMX_LEVELS" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(cli, [path, wav, tmp_path / "f2"], env, UMX_CLIP="clamp", UMX_LEVELS="0")  # today's files byte for byte
    assert r.returncode == 0 and all(open(tmp_path / "f2" / f, "rb").read() == open(tmp_path / "f" / f, "rb").read() for f in MIX_FILES), r.stderr


def test_batch_clip_and_levels(pkg, model_small, tmp_path):
    path, wav, batch = model_small[0], GOLD / "gspi_stereo.wav", Path(pkg.HERE) / "umx-batch"
    q = pkg.wav_load_pcm16(wav)[0]
    files = [wav]
    for i, (a, b) in enumerate(((10000, 90000), (0, 50000), (30000, 31000))):
        files.append(tmp_path / f"part{i}.wav")
        pkg.wav_write_pcm16(files[-1], q[:, a:b])
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_BATCH_LANES": "2", "UMX_MIX": MIX_SPEC}  # four files on two lanes: the queue runs
    r = _run(batch, [path, tmp_path / "f"] + files, env)
    assert r.returncode == 0 and "levels " not in r.stdout, r.stderr
    for name, extra, s16, seed, rescale in (("r16", {"UMX_PCM16": "1", "UMX_CLIP": "rescale", "UMX_LEVELS": "1"}, True, None, True),
                                            ("loop", {"UMX_PCM16": "1", "UMX_CLIP": "rescale", "UMX_LEVELS": "1", "UMX_BATCH_QUEUE": "0"}, True, None, True),
                                            ("cf", {"UMX_LEVELS": "1"}, False, None, False)):
        r = _run(batch, [path, tmp_path / name] + files, env, **extra)
        assert r.returncode == 0, r.stderr
        assert len(LINE.findall(r.stdout)) == 12, r.stdout
        for f in files[:3]:  # (the 1000-frame part is too short to clip: the others carry the conditions)
            _check_dir(pkg, r.stdout, tmp_path / "f" / Path(f).stem, tmp_path / name / Path(f).stem, s16, seed, rescale)
    r = _run(batch, [path, tmp_path / "no"] + files, env, UMX_CLIP="limit")
    assert r.returncode == 1 and "UMX_CLIP" in r.stderr and not (tmp_path / "no").exists(), r.stderr
