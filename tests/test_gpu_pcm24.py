"""Packed 24-bit PCM in and out of the whole-track drivers (csrc/pcm24.h), bit for bit and without tolerances against the
rules of tests/pcm24_ref.py composed with what the fp32 calls return: the kernels alone on guarded device buffers (byte-granular
guards on the packed side: exactly 6 n bytes are written), S24 on either side of the drivers -- one lane split and shifted, lanes of
unequal length, reset mode, the queue, the mix, another sample rate, mixed with int16 --, levels, rescale and loudness of an S24
output, the fp32 and int16 forms afterwards, the refusals, and the CLIs."""
import ctypes as C
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import levels_ref as lev
import pcm16_ref as ref16
import pcm24_ref as ref

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
LENGTH = 61440  # five segments
SEED = 7
ACC_WORDS = 28  # umx_levels_acc: 4 peak words, 3 x 4 64-bit counts
PASS_FRAMES = 2 * 2048 * 256  # frames one pass of the kernels' largest grid covers (pcm24_blocks: a thread per pair of frames)
ODD_N = 7 * 4410 + 123
# synth_audio peaks at 0.5: the first row (3 mix) passes full scale, the second stays quiet, the third is a stem (vocals' slot)
GAINS = np.array([[0, 0, 0, 0, 3], [0, 0, 0, 0, 0.25], [0, 0, 0, 1, 0]], np.float32)
TWO_ROWS = np.array([[0, 0, 0, 1, 0], [0, 0, 0, -1, 1]], np.float32)  # vocals, mixture minus vocals


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
    """24-bit audio (2, LENGTH) int32 codes: the synthetic track at 24 bits"""
    return ref.encode(pkg.ggml.synth_audio(LENGTH, 71))


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[g.dtype.itemsize]
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


# ---------------------------------------------------------------- the kernels alone
class Buf:
    """A guarded device buffer of `words` 32-bit words (tests/guarded.py): the words given, or FILL; its payload at 0 or 8 mod 256."""

    def __init__(self, torch, words, data=None, misalign=0):
        self.lay = gd.track_layout(words, misalign)
        self.before = gd.make(self.lay)
        if data is not None:
            self.before[self.lay.body] = np.ascontiguousarray(data).view(np.int32).ravel()
        self.t = torch.from_numpy(self.before).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lay.pre

    def result(self):
        words = self.t.cpu().numpy()
        rep = gd.check(words, self.lay, expect=words)
        assert rep.pre is None and rep.post is None, str(rep)
        return np.array(words[self.lay.body])

    def floats(self, n):
        return np.ascontiguousarray(self.result().view(np.float32).reshape(n, 2).T)

    def unchanged(self):
        return gd.untouched(self.t.cpu().numpy(), self.before) is None


class Bytes:
    """A device buffer of `nbytes` payload bytes with byte-granular guards: 4 KiB (+ misalign: 0 or 2, the payload's address mod 4) of
    0xA5 in front, the payload (the bytes given, or 0x5A), 4 KiB of 0xA5 behind it, which starts at the payload's very last byte + 1."""
    PRE = 4096

    def __init__(self, torch, nbytes, data=None, misalign=0):
        assert misalign in (0, 2)
        self.pre, self.n = self.PRE + misalign, nbytes
        self.before = np.full(self.pre + nbytes + self.PRE, 0xA5, np.uint8)
        self.before[self.pre:self.pre + nbytes] = 0x5A if data is None else np.asarray(data, np.uint8)
        self.t = torch.from_numpy(self.before).cuda()
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.pre

    def result(self):
        """guards intact, byte for byte -> the payload"""
        b = self.t.cpu().numpy()
        bad = np.flatnonzero(np.concatenate([b[:self.pre], b[self.pre + self.n:]]) != 0xA5)
        assert bad.size == 0, ("a guard byte changed", bad[:8] - self.pre)
        return np.array(b[self.pre:self.pre + self.n])

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before)


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


def _codes(seed, n):
    q = np.random.default_rng(seed).integers(ref.QMIN, ref.QMAX + 1, (2, n)).astype(np.int32)
    q[:, :1] = [[ref.QMIN], [ref.QMAX]]
    return q


FIRSTS = [(0, None), (12345, 5), ((1 << 32) + 7, 5)]  # first_frame (0, odd, beyond 2^32), dither seed


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, ODD_N])
def test_kernels_alone(pkg, torch, eng1, n):
    for pmis in (0, 2):  # the packed address mod 4: 2 has a head frame
        for fmis in (0, 8):  # the fp32 address mod 256
            q = _codes(n + pmis + fmis, n)
            src = Bytes(torch, 6 * n, ref.pack(q), pmis)
            dst = Buf(torch, 2 * n, misalign=fmis)
            eng1.pcm24_decode_device(src.ptr, n, dst.ptr)
            torch.cuda.synchronize()
            _same([dst.floats(n)], [ref.decode(q)], (n, pmis, fmis, "decode"))
            assert src.unchanged()
            for nb in (1, 4):
                for first, seed in FIRSTS:
                    xs = [_floats(1000 * n + 10 * b + pmis, n) for b in range(nb)]
                    ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T), misalign=fmis) for x in xs]
                    outs = [Bytes(torch, 6 * n, misalign=(pmis + 2 * b) % 4) for b in range(nb)]  # (every buffer its own head)
                    eng1.pcm24_encode_device([b.ptr for b in ins], n, [o.ptr for o in outs], first, seed)
                    torch.cuda.synchronize()
                    _same([o.result() for o in outs], [ref.pack(ref.encode(x, b, first, seed)) for b, x in enumerate(xs)],
                          (n, pmis, fmis, nb, first, seed))
                    assert all(b.unchanged() for b in ins)


def test_three_launches_cut_at_odd_frames_give_the_same_bytes(pkg, torch, eng1):
    n, first = ODD_N, 1001
    xs = [_floats(40 + b, n) for b in range(2)]
    ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T)) for x in xs]
    whole = [Bytes(torch, 6 * n) for _ in xs]
    parts = [Bytes(torch, 6 * n) for _ in xs]
    eng1.pcm24_encode_device([b.ptr for b in ins], n, [o.ptr for o in whole], first, SEED)
    cuts = [0, 4411, 20001, n]  # the second and third launch start at odd frames: packed addresses 2 mod 4, fp32 addresses 8 mod 16
    for a, b in zip(cuts, cuts[1:]):
        eng1.pcm24_encode_device([i.ptr + 8 * a for i in ins], b - a, [o.ptr + 6 * a for o in parts], first + a, SEED)
    torch.cuda.synchronize()
    want = [ref.pack(ref.encode(x, m, first, SEED)) for m, x in enumerate(xs)]
    _same([o.result() for o in whole], want, "one launch")
    _same([o.result() for o in parts], want, "three launches")
    # ... and the decode of the middle part alone writes its own frames only
    back = Buf(torch, 2 * n)
    eng1.pcm24_decode_device(parts[0].ptr + 6 * cuts[1], cuts[2] - cuts[1], back.ptr + 8 * cuts[1])
    torch.cuda.synchronize()
    got = back.result()
    assert np.all(got[:2 * cuts[1]] == gd.FILL) and np.all(got[2 * cuts[2]:] == gd.FILL)
    _same([got[2 * cuts[1]:2 * cuts[2]].view(np.float32).reshape(-1, 2).T.copy()], [ref.decode(ref.unpack(want[0]))[:, cuts[1]:cuts[2]].copy()], "part")


def test_every_code_and_a_launch_longer_than_one_pass_of_its_grid(pkg, torch, eng1):
    codes = np.arange(ref.QMIN, ref.QMAX + 1, dtype=np.int32)
    n = 1 << 23
    assert PASS_FRAMES < n and PASS_FRAMES + 77 <= 2 * 1024 * 1024
    q = np.stack([codes[:n], codes[n:]])
    src, dst = Bytes(torch, 6 * n, ref.pack(q)), Buf(torch, 2 * n)
    eng1.pcm24_decode_device(src.ptr, n, dst.ptr)
    torch.cuda.synchronize()
    _same([dst.floats(n)], [ref.decode(q)], "all codes")
    back = Bytes(torch, 6 * n)  # ... and back through the encode kernel: the round trip is exact
    eng1.pcm24_encode_device([dst.ptr], n, [back.ptr])
    torch.cuda.synchronize()
    _same([back.result()], [ref.pack(q)], "round trip")
    # with dither, from an odd address and a first frame beyond 2^32, one pass and a little: within 1 LSB, and the reference's bytes
    m = PASS_FRAMES + 77
    first = (1 << 32) + 12345
    out = Bytes(torch, 6 * m, misalign=2)
    eng1.pcm24_encode_device([dst.ptr], m, [out.ptr], first, SEED)
    torch.cuda.synchronize()
    got = out.result()
    _same([got], [ref.pack(ref.encode(ref.decode(q[:, :m]), 0, first, SEED))], "dithered, two passes")
    assert np.abs(ref.unpack(got).astype(np.int64) - q[:, :m]).max() <= 1


def _clipped(words):
    return [int(words.view(np.uint32)[12 + 2 * m]) | (int(words.view(np.uint32)[13 + 2 * m]) << 32) for m in range(4)]


@pytest.mark.parametrize("n", [1, 258, 4099])
def test_levels_and_rescaled_encode_kernels(pkg, torch, eng1, n):
    for finite in (True, False):
        xs = [_floats(7 * n + b, n) for b in range(3)]
        if finite:  # (and of an audio-like size: the divisor is then a few units, and x / g is not all zeros)
            xs = [np.where(np.isfinite(x) & (np.abs(x) < 100), x, np.float32(0.5)).astype(np.float32) for x in xs]
        ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T), misalign=8) for x in xs]
        for first, seed in FIRSTS[:2]:
            # the measuring kernel counts what the plain S24 encode clamps
            rec = Buf(torch, ACC_WORDS, np.zeros(ACC_WORDS, np.int32))
            eng1.levels_device([b.ptr for b in ins], n, rec.ptr, first, pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S24, seed))
            torch.cuda.synchronize()
            want = [ref.clipped(x, m, first, seed) for m, x in enumerate(xs)] + [0]
            assert _clipped(rec.result()) == want and (n == 1 or want[0] > 0), (n, finite, first, seed)
            # the rescaled encode: the divisor of the peaks an fp32 measurement left in the record, its own count of what clamps
            rec = Buf(torch, ACC_WORDS, np.zeros(ACC_WORDS, np.int32))
            eng1.levels_device([b.ptr for b in ins], n, rec.ptr, first)
            outs = [Bytes(torch, 6 * n, misalign=2 * (b & 1)) for b in range(3)]
            eng1.pcm24_encode_rescaled_device([b.ptr for b in ins], n, [o.ptr for o in outs], rec.ptr, first, seed)
            torch.cuda.synchronize()
            g = lev.gain([lev.levels(x)["peak"] for x in xs])
            assert n == 1 or (g > 1) == finite, (g, finite)
            left = [lev.rescaled(x, g) for x in xs]
            _same([o.result() for o in outs], [ref.pack(ref.encode(x, m, first, seed)) for m, x in enumerate(left)], (n, finite, first, seed))
            want = [ref.clipped(x, m, first, seed) for m, x in enumerate(left)] + [0]
            assert _clipped(rec.result()) == want and (g == 1 or want == [0, 0, 0, 0]), (n, finite, want)
        assert all(b.unchanged() for b in ins)


def test_device_form_refusals_write_nothing(pkg, torch, eng1):
    src, dst, rec = Bytes(torch, 96), Buf(torch, 32), Buf(torch, ACC_WORDS, np.zeros(ACC_WORDS, np.int32))
    for what, call in (("decode n 0", lambda: eng1.pcm24_decode_device(src.ptr, 0, dst.ptr)),
                       ("decode null in", lambda: eng1.pcm24_decode_device(0, 8, dst.ptr)),
                       ("decode null out", lambda: eng1.pcm24_decode_device(src.ptr, 8, 0)),
                       ("decode odd address", lambda: eng1.pcm24_decode_device(src.ptr + 1, 8, dst.ptr)),
                       ("encode n 0", lambda: eng1.pcm24_encode_device([dst.ptr], 0, [src.ptr])),
                       ("encode null in", lambda: eng1.pcm24_encode_device([0], 8, [src.ptr])),
                       ("encode null out", lambda: eng1.pcm24_encode_device([dst.ptr, dst.ptr], 8, [src.ptr, 0])),
                       ("encode odd address", lambda: eng1.pcm24_encode_device([dst.ptr, dst.ptr], 8, [src.ptr, src.ptr + 3])),
                       ("encode 5 buffers", lambda: eng1.pcm24_encode_device([dst.ptr] * 5, 8, [src.ptr] * 5)),
                       ("encode first_frame < 0", lambda: eng1.pcm24_encode_device([dst.ptr], 8, [src.ptr], first_frame=-1)),
                       ("rescaled null record", lambda: eng1.pcm24_encode_rescaled_device([dst.ptr], 8, [src.ptr], 0)),
                       ("rescaled null out", lambda: eng1.pcm24_encode_rescaled_device([dst.ptr], 8, [0], rec.ptr)),
                       ("rescaled odd address", lambda: eng1.pcm24_encode_rescaled_device([dst.ptr], 8, [src.ptr + 1], rec.ptr))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
        assert ("aligned" in str(e.value)) == ("odd" in what), (what, str(e.value))
    torch.cuda.synchronize()
    assert src.unchanged() and dst.unchanged() and rec.unchanged()


# ---------------------------------------------------------------- whole tracks
def _plain(eng, xs, **kw):
    plain_kw = {k: v for k, v in kw.items() if k != "gains"}
    return eng.separate_many_mix(xs, kw["gains"], **plain_kw) if kw.get("gains") is not None else eng.separate_many(xs, **plain_kw)


def _compose(pkg, eng, qs, what, seeds=(None, SEED), **kw):
    """Every form of the _io call for the 24-bit tracks qs against the fp32 call on decode(qs): S24 in; S24 out, plain and dithered;
    both.  kw: flags, shift_offsets, rates, gains as separate_many_io takes them.  Returns the fp32 call's result."""
    xs = [ref.decode(q) for q in qs]
    plain = _plain(eng, xs, **kw)
    S24, F32 = pkg.SAMPLE_S24, pkg.SAMPLE_F32
    for ln, (g, w) in enumerate(zip(eng.separate_many_io(qs, S24, F32, **kw), plain)):
        _same(g, w, (what, "S24 in", ln))
    for seed in seeds:
        want = [[ref.encode(s, m, 0, seed) for m, s in enumerate(stems)] for stems in plain]  # k from the track's first frame, at its rate
        for fin, ins in ((F32, xs), (S24, qs)):
            for ln, (g, w) in enumerate(zip(eng.separate_many_io(ins, fin, S24, seed, **kw), want)):
                _same(g, w, (what, "S24 out", "S24 in" if fin == S24 else "F32 in", seed, ln))
    return plain


def test_one_lane_split_and_shifted(pkg, eng1, qwave):
    assert len(pkg.segment_plan(LENGTH, N)[0]) == 5
    for shift in (None, 4033):  # (4033: every region starts at an odd frame of the track)
        plain = _compose(pkg, eng1, [qwave], ("one lane", shift), shift_offsets=[shift])
        assert all(np.abs(s).max() > 0 for s in plain[0])
    for length in (1, 12289):
        _compose(pkg, eng1, [np.ascontiguousarray(qwave[:, 301:301 + length])], ("short", length), seeds=(SEED,), shift_offsets=[0])


def test_three_lanes_of_unequal_length(pkg, eng3, qwave):
    qs = [qwave, np.ascontiguousarray(qwave[:, 3000:3000 + 9001]), np.ascontiguousarray(qwave[:, 500:500 + 20000])]
    _compose(pkg, eng3, qs, "lanes", seeds=(SEED,), shift_offsets=[11025, None, 0])


def test_reset_mode(pkg, eng3, qwave):
    assert len(pkg.segment_plan(LENGTH + 22050, N)[0]) > 3  # more segments than lanes: a second call of the segment loop
    _compose(pkg, eng3, [qwave], "reset", seeds=(SEED,), flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[11025])


def test_four_queue_jobs_on_two_lanes(pkg, eng2, qwave):
    lengths, shifts = [5000, 12289, 25739, 20001], [None, None, 4033, 11025]
    qs = [np.ascontiguousarray(qwave[:, 41 * i:41 * i + n]) for i, n in enumerate(lengths)]
    io = pkg.sample_io(pkg.SAMPLE_S24, pkg.SAMPLE_S24, SEED)
    got = eng2.separate_queue(qs, shift_offsets=shifts, io=io)
    for j, (q, s) in enumerate(zip(qs, shifts)):
        stems = eng2.separate_many([ref.decode(q)], shift_offsets=[s])[0]
        _same(got[j], [ref.encode(x, m, 0, SEED) for m, x in enumerate(stems)], ("queue job against the rule", j))
    # with levels and rescale through the queue: the record and the bytes of the single-track call
    xs = [ref.decode(q) for q in qs]
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S24, SEED)
    got, lvs = eng2.separate_queue(xs, shift_offsets=shifts, mix=GAINS, io=io, clip=pkg.CLIP_RESCALE, levels=True)
    for j, (x, s) in enumerate(zip(xs, shifts)):
        one, lv1 = eng2.separate_many_levels([x], pkg.CLIP_RESCALE, io, gains=GAINS, shift_offsets=[s])
        _same(got[j], one[0], ("queue job, rescaled", j))
        assert bytes(lvs[j]) == bytes(lv1[0]), j


def test_the_mix_and_another_rate(pkg, eng1, eng3, qwave):
    _compose(pkg, eng1, [qwave], "two-row mix", seeds=(SEED,), gains=TWO_ROWS, shift_offsets=[4033])
    q48 = ref.encode(pkg.ggml.synth_audio(48000, 73))  # one second at 48 kHz: the dither is indexed at 48 kHz
    plain = _compose(pkg, eng1, [q48], "48 kHz", shift_offsets=[4033], rates=[48000])
    assert all(s.shape == q48.shape for s in plain[0])
    _compose(pkg, eng3, [q48, np.ascontiguousarray(qwave[:, :30001])], "48 kHz beside a 44.1 kHz lane", seeds=(SEED,), shift_offsets=[4033, 0],
             rates=[48000, 44100])


def test_s24_with_s16_on_the_other_side(pkg, eng1, qwave):
    S16, S24 = pkg.SAMPLE_S16, pkg.SAMPLE_S24
    x24 = ref.decode(qwave)
    plain = eng1.separate_many([x24], shift_offsets=[4033])[0]
    got = eng1.separate_many_io([qwave], S24, S16, SEED, shift_offsets=[4033])[0]
    _same(got, [ref16.encode(s, m, 0, SEED) for m, s in enumerate(plain)], "S24 in, S16 out")
    q16 = ref16.encode(x24)
    plain = eng1.separate_many([ref16.decode(q16)], shift_offsets=[4033])[0]
    got = eng1.separate_many_io([q16], S16, S24, SEED, shift_offsets=[4033])[0]
    _same(got, [ref.encode(s, m, 0, SEED) for m, s in enumerate(plain)], "S16 in, S24 out")


def _records(lv, n):
    return [{"peak_bits": int(np.float32(lv.peak[m]).view(np.uint32)), "over_unity": int(lv.over_unity[m]), "clipped": int(lv.clipped[m]),
             "nonfinite": int(lv.nonfinite[m])} for m in range(n)]


def test_levels_rescale_and_loudness_of_an_s24_output(pkg, eng1, eng3, qwave):
    for eng, qs, kw in ((eng1, [qwave], {"shift_offsets": [4033]}),
                        (eng3, [qwave, np.ascontiguousarray(qwave[:, 77:77 + 30001])], {"shift_offsets": [None, 11025]})):
        xs = [ref.decode(q) for q in qs]
        plain = eng.separate_many_mix(xs, GAINS, **kw)
        _, _, _, env32 = eng.separate_many_loudness(xs, gains=GAINS, **kw)
        for seed in (None, SEED):
            io = pkg.sample_io(pkg.SAMPLE_S24, pkg.SAMPLE_S24, seed)
            # clamp: the 3 x mix row passes full scale, and clipped says how many samples the S24 encode clamped
            outs, lvs, lds, env = eng.separate_many_loudness(qs, pkg.CLIP_CLAMP, io, gains=GAINS, **kw)
            for ln, stems in enumerate(plain):
                want = [{**{k: lev.levels(s, m)[k] for k in ("peak_bits", "over_unity", "nonfinite")}, "clipped": ref.clipped(s, m, 0, seed)}
                        for m, s in enumerate(stems)]
                assert _records(lvs[ln], 3) == want and lvs[ln].gain == 1.0, (ln, seed, _records(lvs[ln], 3), want)
                assert want[0]["clipped"] > 100 and want[1]["clipped"] == 0, want
                _same(outs[ln], [ref.encode(s, m, 0, seed) for m, s in enumerate(stems)], ("clamp", ln, seed))
                _same([env[ln]], [env32[ln]], ("loudness: the fp32 call's E bits", ln, seed))  # measured before the encode
            # rescale: one divisor per track, nothing clamps, the bytes are the encode of x / g
            outs, lvs, lds, env = eng.separate_many_loudness(qs, pkg.CLIP_RESCALE, io, gains=GAINS, **kw)
            for ln, stems in enumerate(plain):
                g = lev.gain([lev.levels(s, m)["peak"] for m, s in enumerate(stems)])
                assert g > 1 and np.float32(lvs[ln].gain) == g and [r["clipped"] for r in _records(lvs[ln], 3)] == [0, 0, 0], (ln, seed, g)
                _same(outs[ln], [ref.encode(lev.rescaled(s, g), m, 0, seed) for m, s in enumerate(stems)], ("rescale", ln, seed))
                _same([env[ln]], [env32[ln]], ("loudness under rescale", ln, seed))  # ... and before any divisor


def test_dispatch_matrix_every_format_pair_clip_mode_and_dither(pkg, eng1, qwave):
    """Every (in, out) format pair x clip mode x dither seed through umx_hip_separate_tracks_levels, on one track whose regions all
    start at odd frames (shift offset 4033: the 24-bit head / tail path, byte offsets of 6 x an odd frame) and whose first mix row
    passes full scale: the bytes and the levels record of each call are the fp32 call's composed with pcm16_ref / pcm24_ref /
    levels_ref, bit for bit.  36 cases; the 6 that ask for dither with an fp32 output are the documented refusal (sample io: dither
    goes with an integer output only), and it is that refusal they are held to."""
    F32, S16, S24 = pkg.SAMPLE_F32, pkg.SAMPLE_S16, pkg.SAMPLE_S24
    kw = {"gains": GAINS, "shift_offsets": [4033]}
    q24 = np.ascontiguousarray(qwave[:, :25739])
    x = ref.decode(q24)
    q16 = ref16.encode(x)
    plain_x = eng1.separate_many_mix([x], GAINS, shift_offsets=[4033])[0]
    plain_16 = eng1.separate_many_mix([ref16.decode(q16)], GAINS, shift_offsets=[4033])[0]
    cases = 0
    for fin, given, stems in ((F32, x, plain_x), (S16, q16, plain_16), (S24, q24, plain_x)):
        base = [lev.levels(s, m) for m, s in enumerate(stems)]
        g_track = lev.gain([b["peak"] for b in base])
        assert g_track > 1 and base[0]["over_unity"] > 100 and base[1]["over_unity"] == 0, base
        for fout in (F32, S16, S24):
            for clip in (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE):
                for seed in (None, SEED):
                    cases += 1
                    what = (fin, fout, clip, seed)
                    io = pkg.sample_io(fin, fout, seed)
                    if fout == F32 and seed is not None:
                        with pytest.raises(pkg.UmxError) as e:
                            eng1.separate_many_levels([given], clip, io, **kw)
                        assert e.value.code == pkg.ERR_ARG and "dither" in str(e.value), (what, str(e.value))
                        continue
                    outs, lvs = eng1.separate_many_levels([given], clip, io, **kw)
                    g = g_track if clip == pkg.CLIP_RESCALE else np.float32(1.0)
                    left = [lev.rescaled(s, g) for s in stems]
                    if fout == S16:
                        want = [ref16.encode(s, m, 0, seed) for m, s in enumerate(left)]
                        clipped = [lev.levels(s, m, 0, True, seed, g)["clipped"] for m, s in enumerate(stems)]
                    elif fout == S24:
                        want = [ref.encode(s, m, 0, seed) for m, s in enumerate(left)]
                        clipped = [ref.clipped(s, m, 0, seed) for m, s in enumerate(left)]
                    else:
                        want, clipped = left, [0, 0, 0]
                    _same(outs[0], want, what)
                    recs = [{**{k: base[m][k] for k in ("peak_bits", "over_unity", "nonfinite")}, "clipped": clipped[m]} for m in range(3)]
                    assert _records(lvs[0], 3) == recs and np.float32(lvs[0].gain) == g and lvs[0].n_out == 3, (what, _records(lvs[0], 3), recs)
                    assert (clipped[0] > 100) == (fout != F32 and clip == pkg.CLIP_CLAMP) and clipped[1] == 0, (what, clipped)
    assert cases == 36


def _c_call(pkg, eng, audio_ptrs, lengths, shifts, out_ptrs, io):
    nt = len(lengths)
    a = None if audio_ptrs is None else (C.c_void_p * nt)(*audio_ptrs)
    o = None if out_ptrs is None else (C.c_void_p * len(out_ptrs))(*out_ptrs)
    return eng.lib.umx_hip_separate_tracks_io(eng.h, nt, a, (C.c_int * nt)(*lengths), None, (C.c_int * nt)(*shifts), 4, None, o, 0,
                                              None if io is None else C.byref(io), None, None)


def test_refusals_and_todays_bits_afterwards(pkg, eng3, qwave):
    q = np.ascontiguousarray(qwave[:, :25739])
    x = ref.decode(q)
    q16 = ref16.encode(x)
    usual = eng3.separate_many([x], shift_offsets=[4033])[0]
    usual16 = eng3.separate_many_io([q16], pkg.SAMPLE_S16, pkg.SAMPLE_S16, SEED, shift_offsets=[4033])[0]
    n = q.shape[1]
    packed = ref.pack(q)
    # the entry point on guarded host buffers: exactly 6 n bytes of every output, the input untouched
    outs = [np.full(6 * n + 64, 0xA5, np.uint8) for _ in range(4)]
    S24, S16, F32 = pkg.SAMPLE_S24, pkg.SAMPLE_S16, pkg.SAMPLE_F32
    assert _c_call(pkg, eng3, [packed.ctypes.data], [n], [4033], [o.ctypes.data + 32 for o in outs], pkg.SampleIO(S24, S24, 1, SEED)) == 0, eng3.last_error()
    assert all(np.all(o[:32] == 0xA5) and np.all(o[-32:] == 0xA5) for o in outs) and np.array_equal(packed, ref.pack(q))
    _same([ref.unpack(o[32:-32]) for o in outs], [ref.encode(s, m, 0, SEED) for m, s in enumerate(usual)], "C entry point")
    outs = [np.full(6 * n, 0x5A, np.uint8) for _ in range(4)]
    op = [o.ctypes.data for o in outs]
    cases = [("format 2", pkg.SampleIO(2, S24, 0, 0), "sample io: unknown sample format"),
             ("format 7", pkg.SampleIO(S24, 7, 0, 0), "sample io: unknown sample format"),
             ("format 9", pkg.SampleIO(9, S24, 0, 0), "sample io: unknown sample format"),
             ("format -1", pkg.SampleIO(S24, -1, 0, 0), "sample io: unknown sample format"),
             ("dither with an fp32 output", pkg.SampleIO(S24, F32, 1, 3), "dither")]
    for what, io, word in cases:
        assert _c_call(pkg, eng3, [packed.ctypes.data], [n], [4033], op, io) == pkg.ERR_ARG, what
        assert word in eng3.last_error(), (what, eng3.last_error())
        assert all(np.all(o == 0x5A) for o in outs), what
    assert _c_call(pkg, eng3, [None], [n], [4033], op, pkg.SampleIO(S24, S24, 0, 0)) == pkg.ERR_ARG
    assert _c_call(pkg, eng3, [packed.ctypes.data], [n], [4033], [op[0], None, op[2], op[3]], pkg.SampleIO(S24, S24, 0, 0)) == pkg.ERR_ARG
    assert all(np.all(o == 0x5A) for o in outs)
    # the context is usable: an S24 call, and after it the fp32 and the int16 forms are today's bits
    got = eng3.separate_many_io([q], S24, S24, shift_offsets=[4033])[0]
    _same(got, [ref.encode(s, m) for m, s in enumerate(usual)], "S24 after the refusals")
    _same(eng3.separate_many([x], shift_offsets=[4033])[0], usual, "fp32 after S24")
    _same(eng3.separate_many_io([x], F32, F32, shift_offsets=[4033])[0], usual, "F32 / F32 after S24")
    _same(eng3.separate_many_io([q16], S16, S16, SEED, shift_offsets=[4033])[0], usual16, "S16 / S16 after S24")


# ---------------------------------------------------------------- the CLIs
def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def _tree(d):
    return sorted(str(p.relative_to(d)) for p in Path(d).rglob("*.wav"))


def _check_tree(pkg, d, want, rate=44100):
    """the files of a run: 24-bit PCM WAVs whose data chunk is, byte for byte, the Python path's codes; want: {relative name: (2, n) codes}"""
    assert _tree(d) == sorted(want), (_tree(d), sorted(want))
    for rel, q in want.items():
        b = open(Path(d) / rel, "rb").read()
        tag, ch, r, _, align, bits = struct.unpack("<HHIIHH", b[20:36])
        assert (tag, ch, align, bits, r) == (1, 2, 6, 24, rate), rel
        assert b[44:] == ref.pack(q).tobytes(), rel


STEMS = [f"target_{t}.wav" for t in range(4)]


@pytest.fixture(scope="module")
def cli_files(pkg, tmp_path_factory):
    """a 24-bit and a 16-bit input file of 60000 frames, and their codes"""
    d = tmp_path_factory.mktemp("pcm24_in")
    q16 = np.ascontiguousarray(pkg.wav_load_pcm16(GOLD / "gspi_stereo.wav")[0][:, 20000:80000])
    q24 = ref.encode(ref16.decode(q16) * np.float32(0.75))
    pkg.wav_write_pcm24(d / "in24.wav", q24)
    pkg.wav_write_pcm16(d / "in16.wav", q16)
    return d, q24, q16


def test_cli_pcm24_switch(pkg, model_small, cli_files, tmp_path):
    d, q24, q16 = cli_files
    path = model_small[0]
    cli = Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033"}
    eng = pkg.Engine.from_file(path, pkg.SEGMENT_SAMPLES)
    try:
        S24, S16 = pkg.SAMPLE_S24, pkg.SAMPLE_S16
        want24 = eng.separate_many_io([q24], S24, S24, 7, shift_offsets=[4033])[0]
        want16 = eng.separate_many_io([q16], S16, S24, None, shift_offsets=[4033])[0]
        io = pkg.sample_io(S24, S24, 7)
        names, gains = pkg.mix_parse("vocals=vocals;karaoke=mix-vocals")
        wantmix, _ = eng.separate_many_levels([q24], pkg.CLIP_RESCALE, io, gains=gains, shift_offsets=[4033])
    finally:
        eng.close()
    r = _run(cli, [path, d / "in24.wav", tmp_path / "a"], env, UMX_PCM24="1", UMX_PCM24_DITHER="7")
    assert r.returncode == 0, r.stderr
    _check_tree(pkg, tmp_path / "a", dict(zip(STEMS, want24)))
    r = _run(cli, [path, d / "in16.wav", tmp_path / "b"], env, UMX_PCM24="1")
    assert r.returncode == 0, r.stderr
    _check_tree(pkg, tmp_path / "b", dict(zip(STEMS, want16)))
    r = _run(cli, [path, d / "in24.wav", tmp_path / "c"], env, UMX_PCM24="1", UMX_PCM24_DITHER="7", UMX_MIX="vocals=vocals;karaoke=mix-vocals",
             UMX_CLIP="rescale", UMX_LEVELS="1")
    assert r.returncode == 0 and r.stdout.count("levels ") == 2, (r.stdout, r.stderr)
    _check_tree(pkg, tmp_path / "c", {"vocals.wav": wantmix[0][0], "karaoke.wav": wantmix[0][1]})
    for extra, word in (({"UMX_PCM24": "1", "UMX_PCM16": "1"}, "UMX_PCM16"), ({"UMX_PCM24": "1", "UMX_SHIFTS": "2"}, "UMX_SHIFTS"),
                        ({"UMX_PCM24": "1", "UMX_CLI_PER_SEGMENT": "1"}, "UMX_CLI_PER_SEGMENT"), ({"UMX_PCM24_DITHER": "7"}, "UMX_PCM24=1")):
        r = _run(cli, [path, d / "in24.wav", tmp_path / "no"], env, **extra)
        assert r.returncode == 1 and "UMX_PCM24" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), (extra, r.stderr)


def test_batch_pcm24_switch(pkg, model_small, cli_files, tmp_path):
    d, q24, q16 = cli_files
    path = model_small[0]
    batch = Path(pkg.HERE) / "umx-batch"
    parts24 = {"in24": q24, "p0": np.ascontiguousarray(q24[:, 10001:50000]), "p1": np.ascontiguousarray(q24[:, :30001])}
    parts16 = {"in16": q16, "s0": np.ascontiguousarray(q16[:, 5000:45001])}
    for name, q in parts24.items():
        pkg.wav_write_pcm24(tmp_path / f"{name}.wav", q)
    for name, q in parts16.items():
        pkg.wav_write_pcm16(tmp_path / f"{name}.wav", q)
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_BATCH_LANES": "2", "UMX_PCM24": "1", "UMX_PCM24_DITHER": "7"}
    eng = pkg.Engine.from_file(path, pkg.SEGMENT_SAMPLES, tracks=2)
    try:
        S24, S16, F32 = pkg.SAMPLE_S24, pkg.SAMPLE_S16, pkg.SAMPLE_F32
        want24 = {n: eng.separate_many_io([q], S24, S24, 7, shift_offsets=[4033])[0] for n, q in parts24.items()}
        want16 = {n: eng.separate_many_io([q], S16, S24, 7, shift_offsets=[4033])[0] for n, q in parts16.items()}
        wantf = {"in24": eng.separate_many_io([ref.decode(q24)], F32, S24, 7, shift_offsets=[4033])[0],
                 "in16": eng.separate_many_io([ref16.decode(q16)], F32, S24, 7, shift_offsets=[4033])[0]}
    finally:
        eng.close()

    def tree(want):
        return {f"{n}/{s}": q for n, stems in want.items() for s, q in zip(STEMS, stems)}

    # three 24-bit files on two lanes: the queue runs, the files go up packed; and the pass-by-pass loop
    files = [tmp_path / f"{n}.wav" for n in parts24]
    for out, extra in (("q", {}), ("loop", {"UMX_BATCH_QUEUE": "0"})):
        r = _run(batch, [path, tmp_path / out] + files, env, **extra)
        assert r.returncode == 0, r.stderr
        _check_tree(pkg, tmp_path / out, tree(want24))
    # 16-bit files go up as int16; a 24-bit and a 16-bit file in one run go up as fp32
    r = _run(batch, [path, tmp_path / "s"] + [tmp_path / f"{n}.wav" for n in parts16], env)
    assert r.returncode == 0, r.stderr
    _check_tree(pkg, tmp_path / "s", tree(want16))
    r = _run(batch, [path, tmp_path / "m", tmp_path / "in24.wav", tmp_path / "in16.wav"], env)
    assert r.returncode == 0, r.stderr
    _check_tree(pkg, tmp_path / "m", tree(wantf))
    for extra, word in (({"UMX_PCM16": "1"}, "UMX_PCM16"),):
        r = _run(batch, [path, tmp_path / "no"] + files, env, **extra)
        assert r.returncode == 1 and "UMX_PCM24" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(batch, [path, tmp_path / "no"] + files, {"UMX_PCM24_DITHER": "7"})
    assert r.returncode == 1 and "UMX_PCM24" in r.stderr and not (tmp_path / "no").exists(), r.stderr
