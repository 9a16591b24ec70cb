"""16-bit PCM in and out of the whole-track drivers (csrc/pcm16.h), bit for bit and without tolerances against the rules
of tests/pcm16_ref.py composed with what the fp32 calls return: the two kernels alone on guarded device buffers, int16 in, int16
out (dithered or not, the dither counted in the caller's track), both at once -- over split and shifted tracks of one to three
segments, lanes of unequal length, reset mode, flags, a mix, other sample rates --, the queue, the C entry point on guarded host
buffers, the refusals, the fp32 forms of the new calls, and the CLIs."""
import ctypes as C
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import pcm16_ref as ref

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
OFFSETS = [None, 0, 11025, 22049]
LENGTHS = [1, 12288, 12289, 25739]  # one to three segments: region boundaries fall inside the track
SEED = 7


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
def qwave(pkg):
    """int16 audio (2, 25739): the synthetic track at 16 bits"""
    return ref.encode(pkg.ggml.synth_audio(25739, 71))


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = np.uint32 if g.dtype == np.float32 else np.uint16
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


def _words(q):
    """(2, n) int16 -> n frame words"""
    return np.ascontiguousarray(np.asarray(q, np.int16).T).view(np.int32).ravel()


def _frames(words):
    """n frame words -> (2, n) int16"""
    return np.ascontiguousarray(np.asarray(words, np.int32).view(np.int16).reshape(-1, 2).T)


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
        rep = gd.check(words, self.lay, expect=words)  # (guards only: int16 frames are not floats)
        assert rep.pre is None and rep.post is None, str(rep)
        return np.array(words[self.lay.body])

    def unchanged(self):
        return gd.untouched(self.t.cpu().numpy(), self.before) is None


def _floats(seed, n):
    """(2, n) fp32: audio-like noise, some of it clipping, and the awkward values of the CPU test where they fit"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2, n)) * 0.4).astype(np.float32)
    x[:, ::5] *= 4
    a = ref.awkward_floats()
    k = min(a.shape[1], n)
    pos = rng.permutation(n)[:k]
    x[:, pos] = a[:, rng.permutation(a.shape[1])[:k]]
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4099])
def test_kernels_alone(pkg, torch, eng1, n):
    rng = np.random.default_rng(n)
    for off in (0, 1):  # pointers offset by one frame: 4-byte aligned int16, 8-byte aligned fp32
        q = rng.integers(-32768, 32768, (2, n + off)).astype(np.int16)
        src = Buf(torch, n + off, _words(q))
        dst = Buf(torch, 2 * (n + off), misalign=8 * (1 - off))  # (either way the pointer passed is 8 mod 16)
        eng1.pcm16_decode_device(src.ptr + 4 * off, n, dst.ptr + 8 * off)
        torch.cuda.synchronize()
        got = dst.result()
        assert np.all(got[:2 * off] == gd.FILL), (n, off, "decode wrote in front of its n frames")
        _same([got[2 * off:].view(np.float32).reshape(n, 2).T], [ref.decode(q[:, off:])], (n, off, "decode"))
        assert src.unchanged()
        for nb in (1, 4):
            for first in (0, 12345):
                for seed in (None, 5):
                    xs = [_floats(1000 * n + 10 * b + off, n + off) for b in range(nb)]
                    ins = [Buf(torch, 2 * (n + off), np.ascontiguousarray(x.T), misalign=8 * (1 - off)) for x in xs]
                    outs = [Buf(torch, n + off) for _ in range(nb)]
                    eng1.pcm16_encode_device([b.ptr + 8 * off for b in ins], n, [o.ptr + 4 * off for o in outs], first, seed)
                    torch.cuda.synchronize()
                    res = [o.result() for o in outs]
                    assert all(np.all(r[:off] == gd.FILL) for r in res), (n, off, "encode wrote in front of its n frames")
                    _same([_frames(r[off:]) for r in res], [ref.encode(x[:, off:], b, first, seed) for b, x in enumerate(xs)],
                          (n, off, nb, first, seed))
                    assert all(b.unchanged() for b in ins)


def test_decode_kernel_on_every_code(pkg, torch, eng1):
    codes = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    q = np.stack([codes[:32768], codes[32768:]])
    src, dst = Buf(torch, 32768, _words(q)), Buf(torch, 65536)
    eng1.pcm16_decode_device(src.ptr, 32768, dst.ptr)
    torch.cuda.synchronize()
    x = dst.result().view(np.float32).reshape(32768, 2).T
    _same([np.ascontiguousarray(x)], [ref.decode(q)], "all codes")
    # ... and back through the encode kernel: the round trip is exact
    back = Buf(torch, 32768)
    eng1.pcm16_encode_device([dst.ptr], 32768, [back.ptr])
    torch.cuda.synchronize()
    _same([_frames(back.result())], [q], "round trip")


def test_device_form_refusals_write_nothing(pkg, torch, eng1):
    src, dst = Buf(torch, 64, np.arange(64, dtype=np.int32)), Buf(torch, 128)
    for what, call in (("decode n 0", lambda: eng1.pcm16_decode_device(src.ptr, 0, dst.ptr)),
                       ("decode null in", lambda: eng1.pcm16_decode_device(0, 8, dst.ptr)),
                       ("decode null out", lambda: eng1.pcm16_decode_device(src.ptr, 8, 0)),
                       ("encode n 0", lambda: eng1.pcm16_encode_device([dst.ptr], 0, [src.ptr])),
                       ("encode null in", lambda: eng1.pcm16_encode_device([0], 8, [src.ptr])),
                       ("encode null out", lambda: eng1.pcm16_encode_device([dst.ptr, dst.ptr], 8, [src.ptr, 0])),
                       ("encode 5 buffers", lambda: eng1.pcm16_encode_device([dst.ptr] * 5, 8, [src.ptr] * 5)),
                       ("encode first_frame < 0", lambda: eng1.pcm16_encode_device([dst.ptr], 8, [src.ptr], first_frame=-1))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
    torch.cuda.synchronize()
    assert src.unchanged() and dst.unchanged()


# ---------------------------------------------------------------- whole tracks
def _compose(pkg, eng, qs, what, **kw):
    """Every form of the _io call for the int16 tracks qs against the fp32 call on decode(qs): int16 in; int16 out, plain and
    dithered; both.  kw: flags, shift_offsets, rates, gains as separate_many_io takes them."""
    xs = [ref.decode(q) for q in qs]
    plain_kw = {k: v for k, v in kw.items() if k != "gains"}
    plain = eng.separate_many_mix(xs, kw["gains"], **plain_kw) if kw.get("gains") is not None else eng.separate_many(xs, **plain_kw)
    S16, F32 = pkg.SAMPLE_S16, pkg.SAMPLE_F32
    for ln, (g, w) in enumerate(zip(eng.separate_many_io(qs, S16, F32, **kw), plain)):
        _same(g, w, (what, "S16 in", ln))
    for seed in (None, SEED):
        want = [[ref.encode(s, m, 0, seed) for m, s in enumerate(stems)] for stems in plain]  # k from the track's first frame
        for fin, ins in ((F32, xs), (S16, qs)):
            for ln, (g, w) in enumerate(zip(eng.separate_many_io(ins, fin, S16, seed, **kw), want)):
                _same(g, w, (what, "S16 out", "S16 in" if fin == S16 else "F32 in", seed, ln))
    return plain


@pytest.mark.parametrize("length", LENGTHS)
def test_split_and_shifted_tracks(pkg, eng1, qwave, length):
    q = np.ascontiguousarray(qwave[:, 300:300 + length])
    for shift in OFFSETS:
        plain = _compose(pkg, eng1, [q], (length, shift), shift_offsets=[shift])
        assert length < 1000 or all(np.abs(s).max() > 0 for s in plain[0])
    segs = [len(pkg.segment_plan(n, N)[0]) for n in LENGTHS]
    assert segs == [1, 1, 2, 3], segs


def test_three_lanes_of_unequal_length(pkg, eng3, qwave):
    qs = [qwave, np.ascontiguousarray(qwave[:, 3000:3000 + 9000]), np.ascontiguousarray(qwave[:, 500:500 + 20000])]
    _compose(pkg, eng3, qs, "lanes", shift_offsets=[11025, None, 0])
    _compose(pkg, eng3, qs[1:], "two of three lanes", shift_offsets=[22049, None])


def test_reset_mode(pkg, eng3, qwave):
    for shift in (None, 11025):
        _compose(pkg, eng3, [qwave], ("reset", shift), flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])
    # more segments than lanes: a second call of the segment loop, with its upload ahead of the first one's end
    long = np.ascontiguousarray(np.concatenate([qwave, qwave[:, ::-1]], axis=1))
    assert len(pkg.segment_plan(long.shape[1] + 22050, N)[0]) > 3
    _compose(pkg, eng3, [long], "reset, two calls", flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[0])


def test_flags_and_the_mix(pkg, eng1, eng3, qwave):
    _compose(pkg, eng1, [qwave], "no wiener", flags=pkg.FLAG_NO_WIENER, shift_offsets=[4033])
    flags = pkg.flags_for_targets(["vocals"], residual=True)
    _compose(pkg, eng1, [qwave], "vocals + residual", flags=flags, shift_offsets=[4033])
    two_rows = np.array([[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]], np.float32)  # vocals, mixture minus vocals
    _compose(pkg, eng1, [qwave], "two-row mix", gains=two_rows, shift_offsets=[4033])
    qs = [qwave, np.ascontiguousarray(qwave[:, 100:100 + 13000])]
    _compose(pkg, eng3, qs, "two-row mix, lanes", gains=two_rows, shift_offsets=[None, 22049])


@pytest.mark.parametrize("rate", [48000, 22050])
def test_another_rate_dithers_at_the_callers_rate(pkg, eng1, eng3, rate):
    q = ref.encode(pkg.ggml.synth_audio(rate, 73))  # one second
    plain = _compose(pkg, eng1, [q], rate, shift_offsets=[4033], rates=[rate])
    assert all(s.shape == q.shape for s in plain[0])
    q2 = ref.encode(pkg.ggml.synth_audio(30000, 74))
    _compose(pkg, eng3, [q, q2], (rate, "beside a 44.1 kHz lane"), shift_offsets=[4033, 0], rates=[rate, 44100])
    _compose(pkg, eng1, [q], (rate, "mix"), gains=np.array([[1, 1, 1, 0, 0], [0, 0, 0, -1, 1]], np.float32), shift_offsets=[4033], rates=[rate])


def test_queue_jobs_equal_the_single_track_call(pkg, eng2, qwave):
    lengths, shifts = [5000, 12289, 25739, 1, 20000], [None, None, None, None, 11025]
    qs = [np.ascontiguousarray(qwave[:, 40 * i:40 * i + n]) for i, n in enumerate(lengths)]
    segs = [len(pkg.segment_plan(n + (0 if s is None else max(22050 - s, s)), N)[0]) for n, s in zip(lengths, shifts)]
    assert segs == [1, 2, 3, 1, 3], segs
    io = pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED)
    got = eng2.separate_queue(qs, shift_offsets=shifts, io=io)
    assert eng2.queue_calls() == pkg.queue_plan(2, segs)[2]
    for j, (q, s) in enumerate(zip(qs, shifts)):
        want = eng2.separate_many_io([q], pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED, shift_offsets=[s])[0]
        _same(got[j], want, ("queue job", j))
        stems = eng2.separate_many([ref.decode(q)], shift_offsets=[s])[0]
        _same(got[j], [ref.encode(x, m, 0, SEED) for m, x in enumerate(stems)], ("queue job against the rule", j))
    # int16 out alone, with a mix; and the fp32 queue afterwards is what it was
    two_rows = np.array([[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]], np.float32)
    xs = [ref.decode(q) for q in qs]
    plain = eng2.separate_queue(xs, shift_offsets=shifts, mix=two_rows)
    got = eng2.separate_queue(xs, shift_offsets=shifts, mix=two_rows, io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16))
    for j in range(len(qs)):
        _same(got[j], [ref.encode(x, m) for m, x in enumerate(plain[j])], ("queue, mix", j))
    again = eng2.separate_queue(xs, shift_offsets=shifts, mix=two_rows, io=pkg.sample_io())
    for j in range(len(qs)):
        _same(again[j], plain[j], ("queue, fp32 io", j))


# ---------------------------------------------------------------- C entry points
def _c_call(pkg, eng, audio_ptrs, lengths, shifts, out_ptrs, io, n_out=4, gains=None, flags=0, rates=None):
    nt = len(lengths)
    a = None if audio_ptrs is None else (C.c_void_p * nt)(*audio_ptrs)
    o = None if out_ptrs is None else (C.c_void_p * len(out_ptrs))(*out_ptrs)
    return eng.lib.umx_hip_separate_tracks_io(eng.h, nt, a, (C.c_int * nt)(*lengths), None if rates is None else (C.c_int * nt)(*rates),
                                              (C.c_int * nt)(*shifts), n_out, None if gains is None else gains.ctypes.data_as(pkg._fp), o,
                                              flags, None if io is None else C.byref(io), None, None)


def test_entry_point_writes_exactly_the_tracks_int16s(pkg, eng3, qwave):
    lengths = [25739, 9001]
    qs = [qwave, np.ascontiguousarray(qwave[:, 77:77 + 9001])]
    lays = [gd.track_layout(n) for n in lengths]  # a frame is one word: exactly 2 * length int16s
    audio = [gd.make(lay) for lay in lays]
    for a, lay, q in zip(audio, lays, qs):
        a[lay.body] = _words(q)
    audio_before = [a.copy() for a in audio]
    outs = [[gd.make(lay) for _ in range(4)] for lay in lays]
    io = pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED)
    rc = _c_call(pkg, eng3, [a.ctypes.data + 4 * lay.pre for a, lay in zip(audio, lays)], lengths, [4033, -1],
                 [o.ctypes.data + 4 * lay.pre for t4, lay in zip(outs, lays) for o in t4], io)
    assert rc == 0, eng3.last_error()
    want = eng3.separate_many_io(qs, pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED, shift_offsets=[4033, None])
    for ln, lay in enumerate(lays):
        assert gd.untouched(audio[ln], audio_before[ln]) is None
        for t in range(4):
            rep = gd.check(outs[ln][t], lay, expect=outs[ln][t])
            assert rep.pre is None and rep.post is None, (ln, t, str(rep))
            _same([_frames(outs[ln][t][lay.body])], [want[ln][t]], (ln, t))
    # a mix of two rows writes two buffers per track and nothing of a third
    two_rows = np.ascontiguousarray(np.array([[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]], np.float32))
    outs = [gd.make(lays[0]) for _ in range(3)]
    before = outs[2].copy()
    rc = _c_call(pkg, eng3, [audio[0].ctypes.data + 4 * lays[0].pre], lengths[:1], [0], [o.ctypes.data + 4 * lays[0].pre for o in outs], io, 2,
                 two_rows.ravel())
    assert rc == 0, eng3.last_error()
    want = eng3.separate_many_io(qs[:1], pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED, shift_offsets=[0], gains=two_rows)[0]
    for m in range(2):
        rep = gd.check(outs[m], lays[0], expect=outs[m])
        assert rep.pre is None and rep.post is None, (m, str(rep))
        _same([_frames(outs[m][lays[0].body])], [want[m]], ("mix", m))
    assert gd.untouched(outs[2], before) is None


def test_refusals_leave_the_context_usable(pkg, eng3, qwave):
    x = ref.decode(qwave)
    usual = eng3.separate_many([x], shift_offsets=[4033])[0]
    n = qwave.shape[1]
    a16 = np.ascontiguousarray(qwave.T)
    outs = [np.full(2 * n, 0x5A5A, np.int16) for _ in range(4)]
    op = [o.ctypes.data for o in outs]
    S16, F32 = pkg.SAMPLE_S16, pkg.SAMPLE_F32
    cases = [("unknown input format", [a16.ctypes.data], op, pkg.SampleIO(2, S16, 0, 0), "format"),
             ("unknown output format", [a16.ctypes.data], op, pkg.SampleIO(S16, 7, 0, 0), "format"),
             ("negative format", [a16.ctypes.data], op, pkg.SampleIO(-1, F32, 0, 0), "format"),
             ("dither with an fp32 output", [a16.ctypes.data], op, pkg.SampleIO(S16, F32, 1, 3), "dither"),
             ("null audio", [None], op, pkg.SampleIO(S16, S16, 0, 0), "audio"),
             ("null audio array", None, op, pkg.SampleIO(S16, S16, 0, 0), "null"),
             ("a null output", [a16.ctypes.data], [op[0], None, op[2], op[3]], pkg.SampleIO(S16, S16, 0, 0), "outputs"),
             ("null output array", [a16.ctypes.data], None, pkg.SampleIO(S16, S16, 0, 0), "outputs")]
    for what, ap, outp, io, word in cases:
        assert _c_call(pkg, eng3, ap, [n], [4033], outp, io) == pkg.ERR_ARG, what
        assert word in eng3.last_error(), (what, eng3.last_error())
        assert all(np.all(o == 0x5A5A) for o in outs), what
        _same(eng3.separate_many([x], shift_offsets=[4033])[0], usual, ("fp32 after", what))
    nxt = pkg.QUEUE_NEXT_FN(lambda u, j: 0)
    done = pkg.QUEUE_DONE_FN(lambda u, j: None)
    for io, word in ((pkg.SampleIO(S16, 9, 0, 0), "format"), (pkg.SampleIO(F32, F32, 1, 0), "dither")):
        assert eng3.lib.umx_hip_separate_queue_io(eng3.h, nxt, done, None, 4, None, 0, C.byref(io)) == pkg.ERR_ARG
        assert word in eng3.last_error()
    assert eng3.lib.umx_hip_separate_tracks_io(None, 1, None, None, None, None, 4, None, None, 0, None, None, None) == pkg.ERR_ARG
    # a good int16 call after all that, and the fp32 call after it
    got = eng3.separate_many_io([qwave], S16, S16, shift_offsets=[4033])[0]
    _same(got, [ref.encode(s, m) for m, s in enumerate(usual)], "int16 after the refusals")
    _same(eng3.separate_many([x], shift_offsets=[4033])[0], usual, "fp32 after int16")


def test_fp32_forms_are_todays_calls(pkg, eng3, qwave):
    xs = [ref.decode(qwave), ref.decode(qwave[:, 1000:14000])]
    shifts = [4033, None]
    usual = eng3.separate_many(xs, shift_offsets=shifts)
    for ln, stems in enumerate(eng3.separate_many_io(xs, shift_offsets=shifts)):  # F32 / F32
        _same(stems, usual[ln], ("F32 / F32", ln))
    # io == NULL
    ins = [np.ascontiguousarray(x.T) for x in xs]
    outs = [[np.empty((x.shape[1], 2), np.float32) for _ in range(4)] for x in xs]
    rc = _c_call(pkg, eng3, [a.ctypes.data for a in ins], [x.shape[1] for x in xs], [4033, -1], [o.ctypes.data for t4 in outs for o in t4], None)
    assert rc == 0, eng3.last_error()
    for ln in range(2):
        _same([np.ascontiguousarray(o.T) for o in outs[ln]], usual[ln], ("io NULL", ln))
    g = np.array([[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]], np.float32)
    for a, b in zip(eng3.separate_many_io(xs, shift_offsets=shifts, gains=g), eng3.separate_many_mix(xs, g, shift_offsets=shifts)):
        _same(a, b, "F32 / F32 with a mix")
    for a, b in zip(eng3.separate_many_io(xs[:1], shift_offsets=[4033], rates=[48000]), eng3.separate_many(xs[:1], shift_offsets=[4033], rates=[48000])):
        _same(a, b, "F32 / F32 at 48 kHz")


# ---------------------------------------------------------------- the CLIs
def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def _tree(d):
    return sorted(str(p.relative_to(d)) for p in Path(d).rglob("*.wav"))


def _check_pcm16_tree(pkg, d16, dfloat, seed, slot_of):
    """every file of the float run, as a 16-bit PCM WAV of the same name, rate and length whose samples are encode() of the float
    file's (m: the file's index in the call's list of outputs)"""
    assert _tree(d16) == _tree(dfloat) and _tree(d16), (_tree(d16), _tree(dfloat))
    for rel in _tree(d16):
        b = open(Path(d16) / rel, "rb").read(44)
        tag, ch, rate, _, align, bits = struct.unpack("<HHIIHH", b[20:36])
        x, _, frate = pkg.wav_load_rate(Path(dfloat) / rel)
        assert (tag, ch, align, bits, rate) == (1, 2, 4, 16, frate), rel
        q = pkg.wav_load_pcm16(Path(d16) / rel)[0]
        _same([q], [ref.encode(x, slot_of(Path(rel).name), 0, seed)], rel)


def _bytes(d):
    return {rel: open(Path(d) / rel, "rb").read() for rel in _tree(d)}


STEM_SLOT = {f"target_{t}.wav": t for t in range(4)}


def test_cli_pcm16_switch(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"  # 16-bit PCM: goes up as int16
    cli = Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033"}
    r = _run(cli, [path, wav, tmp_path / "f"], env)
    assert r.returncode == 0, r.stderr
    for name, extra, seed in (("q", {"UMX_PCM16": "1"}, None), ("qd", {"UMX_PCM16": "1", "UMX_PCM16_DITHER": "7"}, 7)):
        r = _run(cli, [path, wav, tmp_path / name], env, **extra)
        assert r.returncode == 0, r.stderr
        _check_pcm16_tree(pkg, tmp_path / name, tmp_path / "f", seed, STEM_SLOT.get)
    assert _bytes(tmp_path / "q") != _bytes(tmp_path / "qd")
    # a float input file goes up as fp32 and comes back as int16; with the mix, the targets and the resampler
    x, _ = pkg.wav_load(wav)
    pkg.wav_write(tmp_path / "in48.wav", x[:, :60000], rate=48000)
    spec = "vocals=vocals;karaoke=mix-vocals"
    env2 = {**env, "UMX_RESAMPLE": "1", "UMX_MIX": spec, "UMX_TARGETS": "vocals,drums"}
    r = _run(cli, [path, tmp_path / "in48.wav", tmp_path / "mf"], env2)
    assert r.returncode == 0, r.stderr
    r = _run(cli, [path, tmp_path / "in48.wav", tmp_path / "mq"], env2, UMX_PCM16="1", UMX_PCM16_DITHER="7")
    assert r.returncode == 0, r.stderr
    _check_pcm16_tree(pkg, tmp_path / "mq", tmp_path / "mf", 7, {"vocals.wav": 0, "karaoke.wav": 1}.get)
    # the two refusals, and without the variable today's files byte for byte
    for extra, word in (({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"), ({"UMX_CLI_PER_SEGMENT": "1"}, "UMX_CLI_PER_SEGMENT")):
        r = _run(cli, [path, wav, tmp_path / "no"], env, UMX_PCM16="1", **extra)
        assert r.returncode == 1 and "UMX_PCM16" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(cli, [path, wav, tmp_path / "f2"], env, UMX_PCM16="0")
    assert r.returncode == 0 and _bytes(tmp_path / "f2") == _bytes(tmp_path / "f"), r.stderr


def test_batch_pcm16_switch(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    q = pkg.wav_load_pcm16(wav)[0]
    files = [wav]
    for i, (a, b) in enumerate(((10000, 90000), (0, 50000), (30000, 31000))):
        files.append(tmp_path / f"part{i}.wav")
        pkg.wav_write_pcm16(files[-1], q[:, a:b])
    batch = Path(pkg.HERE) / "umx-batch"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_BATCH_LANES": "2"}  # four files on two lanes: the queue runs
    r = _run(batch, [path, tmp_path / "f"] + files, env)
    assert r.returncode == 0, r.stderr
    for name, extra, seed in (("q", {"UMX_PCM16": "1"}, None), ("qd", {"UMX_PCM16": "1", "UMX_PCM16_DITHER": "7"}, 7),
                              ("loop", {"UMX_PCM16": "1", "UMX_PCM16_DITHER": "7", "UMX_BATCH_QUEUE": "0"}, 7)):
        r = _run(batch, [path, tmp_path / name] + files, env, **extra)
        assert r.returncode == 0, r.stderr
        _check_pcm16_tree(pkg, tmp_path / name, tmp_path / "f", seed, STEM_SLOT.get)
    assert len(_tree(tmp_path / "q")) == 16
    # one float file among them: the run's inputs go up as fp32, the outputs are the same files
    x, _ = pkg.wav_load(files[1])
    pkg.wav_write(tmp_path / "part0.wav", x)
    r = _run(batch, [path, tmp_path / "mixed"] + files, env, UMX_PCM16="1", UMX_PCM16_DITHER="7", UMX_TARGETS="vocals", UMX_RESIDUAL="1")
    assert r.returncode == 0, r.stderr
    r = _run(batch, [path, tmp_path / "mixedf"] + files, env, UMX_TARGETS="vocals", UMX_RESIDUAL="1")
    assert r.returncode == 0, r.stderr
    _check_pcm16_tree(pkg, tmp_path / "mixed", tmp_path / "mixedf", 7, {"target_3.wav": 3, "residual.wav": 0}.get)
    r = _run(batch, [path, tmp_path / "f2"] + files[:1] + [files[2], files[3]], env, UMX_PCM16="0")
    assert r.returncode == 0, r.stderr
    want = {k: v for k, v in _bytes(tmp_path / "f").items() if not k.startswith("part0")}
    assert _bytes(tmp_path / "f2") == want
    r = _run(batch, [path, tmp_path / "no"] + files, env, UMX_PCM16_DITHER="7")
    assert r.returncode == 1 and "UMX_PCM16" in r.stderr and not (tmp_path / "no").exists(), r.stderr
