"""True peak of every output (csrc/true_peak.h) on the GPU: the kernel alone on guarded device buffers (the record itself
guarded), bit for bit the host statement of the rule (umx_hip_true_peak_host), and the whole-track drivers -- one lane, lanes of
unequal length, reset mode, the queue, a mix, integer outputs, another sample rate, both rescales -- each record bit for bit the host
function over that job's own fp32 outputs."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import true_peak_ref as ref

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
STRIDE = 12288
SEED = 7
LENGTH = 5 * STRIDE  # 61440 frames: five segments
TILE = 1024  # TP_TILE of csrc/true_peak.h: frames of a workgroup
GAINS = np.array([[0, 0, 0, 0, 3], [0, 0, 0, 0, 0.25], [0, 0, 0, 1, 0]], np.float32)  # as tests/test_gpu_levels.py
INF_BITS = 0x7f800000


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
    x = pkg.ggml.synth_audio(LENGTH, 71)
    assert x.shape == (2, LENGTH)
    return x


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = {4: np.uint32, 2: np.uint16, 8: np.uint64}[g.dtype.itemsize]
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


def _bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------- the kernel alone
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


def _record(torch):
    return Buf(torch, 4, np.zeros(4, np.uint32))


def _signals(rate, n, nb, seed):
    """noise with a 40 dB step, and the 45 degree tone over a stretch of it: inter-sample peaks above the sample peak"""
    xs = []
    for b in range(nb):
        x = ref.stepped(rate, n, seed + b)
        a = n // 3
        x[:, a:a + min(40, n - a)] += (0.6 * ref.tone(rate, 45.0, min(40, n - a) / rate)[:, :min(40, n - a)]).astype(np.float32)
        xs.append(x * np.float32(1.0 + 0.5 * b))
    return xs


def _device(torch, eng, xs, rate, spans=None, off=0):
    """the kernel over `spans` of guarded copies of xs (one launch each; None: the whole) -> the four words; the inputs stay as they were"""
    n = xs[0].shape[1] - off
    ins = [Buf(torch, 2 * (n + off), np.ascontiguousarray(x.T), misalign=8 * (1 - off) if off else 0) for x in xs]
    rec = _record(torch)
    for first, count in (spans or [(0, n)]):
        eng.true_peak_device([b.ptr + 8 * off for b in ins], n, rate, rec.ptr, first, count)
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in ins)
    return rec.result().view(np.uint32)


def _host(pkg, xs, rate, spans=None, off=0):
    out = np.zeros(4, np.uint32)
    for b, x in enumerate(xs):
        x = x[:, off:]
        for first, count in (spans or [(0, x.shape[1])]):
            out[b] = pkg.true_peak_host(x, rate, first, count, out[b])
    return out


@pytest.mark.parametrize("rate", [8000, 44100, 96000, 192000])
def test_kernel_alone(pkg, torch, eng1, rate):
    for n in (1, 5, 23, 255, 256, 257, 7 * 256 + 123):
        for nb in (1, 4):
            xs = _signals(rate, n, nb, 10 * n + nb)
            got, want = _device(torch, eng1, xs, rate), _host(pkg, xs, rate)
            assert np.array_equal(got, want), (rate, n, nb, got, want)
            assert (got[nb:] == 0).all() and (got[:nb] > 0).all()
    # the buffers one frame into their allocation: 8-byte aligned, not 16
    xs = _signals(rate, 7 * 256 + 124, 4, 3)
    assert np.array_equal(_device(torch, eng1, xs, rate, off=1), _host(pkg, xs, rate, off=1))


@pytest.mark.parametrize("rate", [44100, 96000])
def test_spans_and_more_than_one_workgroup(pkg, torch, eng1, rate):
    """3 tiles and a half: a span that starts and ends mid-tile, and the same frames in three launches cut off the tile edges"""
    n = 3 * TILE + 500
    xs = _signals(rate, n, 2, 5)
    whole = _device(torch, eng1, xs, rate)
    assert np.array_equal(whole, _host(pkg, xs, rate))
    span = [(300, 2500)]
    got = _device(torch, eng1, xs, rate, span)
    assert np.array_equal(got, _host(pkg, xs, rate, span))
    cut = [(1000, 1800), (300, 1), (301, 699)]
    assert np.array_equal(_device(torch, eng1, xs, rate, cut), got)
    assert np.array_equal(_device(torch, eng1, xs, rate, [(0, 0), (n, 0)]), np.zeros(4, np.uint32))  # an empty span: no launch
    # the largest value sits in one tile only: a span beside it does not see it
    x = np.zeros((2, n), np.float32)
    x[0, 2 * TILE + 100] = 0.5
    assert _device(torch, eng1, [x], rate, [(0, 2 * TILE)])[0] == 0
    assert _device(torch, eng1, [x], rate, [(2 * TILE, TILE)])[0] >= _bits(0.5)


@pytest.mark.parametrize("rate", [44100, 96000])
def test_an_inter_sample_peak_across_a_tile_edge(pkg, torch, eng1, rate):
    n = 2 * TILE + 77
    burst = (0.9 * ref.tone(rate, 45.0, 10 / rate)[:, :10]).astype(np.float32)
    for at in (TILE - 5, TILE - 1, TILE, 2 * TILE - 9):
        x = np.zeros((2, n), np.float32)
        x[:, at:at + 10] = burst
        got, want = _device(torch, eng1, [x], rate), _host(pkg, [x], rate)
        assert np.array_equal(got, want), (rate, at, got, want)
        assert pkg.true_peak_float(got[0]) > 1.05 * ref.sample_peak(x), (rate, at)
        # and with the launch's tiles anchored elsewhere: the same bits
        assert np.array_equal(_device(torch, eng1, [x], rate, [(0, 7), (7, n - 7)]), want)


MAX_BLOCKS = 2048  # TP_MAX_BLOCKS of csrc/true_peak.h: a launch has at most MAX_BLOCKS // buffers workgroups per buffer


@pytest.mark.parametrize("rate,nb,tiles", [(44100, 4, 2 * 512 + 76), (96000, 1, 2048 + 700), (96000, 2, 1024 + 1)])
def test_workgroups_walk_several_tiles(pkg, torch, eng1, rate, nb, tiles):
    """More tiles than a launch has workgroups per buffer, and no multiple of them: a workgroup takes its next tile from the registers
    it prefetched into while the tile before was measured, over the same LDS.  The largest value of every buffer is an inter-sample
    peak in a tile of the LAST pass; the second buffer has it across the edge of a tile of the second pass."""
    grid = MAX_BLOCKS // nb
    assert tiles > grid and tiles % grid != 0
    n = tiles * TILE + 77
    burst = ref.tone(rate, 45.0, 10 / rate, amplitude=2.0)[:, :10].astype(np.float32)  # samples of 1.41, an inter-sample peak near 2
    xs = []
    for b in range(nb):
        x = ref.stepped(rate, n, 40 + b) * np.float32(0.5)  # below 0.3 in size
        at = (tiles - 1 - 3 * b) * TILE + 500 + 11 * b if b != 1 else min(grid + 7, tiles - 1) * TILE - 4  # (b == 1: across the edge of a second-pass tile)
        x[:, at:at + 10] = np.float32(0.9 + 0.02 * b) * burst
        xs.append(x)
    got, want = _device(torch, eng1, xs, rate), _host(pkg, xs, rate)
    assert np.array_equal(got, want), (rate, nb, tiles, got, want)
    for b in range(nb):  # (the condition: the burst's inter-sample peak is the buffer's largest value, above every sample)
        assert pkg.true_peak_float(got[b]) > 1.05 * ref.sample_peak(xs[b]) > 1.0, b
    # without the bursts the maxima sit elsewhere, in tiles of any pass: the walk meets every tile once
    quiet = [ref.stepped(rate, n, 60 + b) for b in range(nb)]
    assert np.array_equal(_device(torch, eng1, quiet, rate), _host(pkg, quiet, rate))
    # a span off the tile grid whose tiles outnumber the workgroups too: the same rule
    span = [(333, n - 1000)]
    assert np.array_equal(_device(torch, eng1, xs[:1], rate, span), _host(pkg, xs[:1], rate, span))


def test_a_nan_and_an_inf_mid_tile(pkg, torch, eng1):
    rate, n = 44100, TILE + 300
    xs = _signals(rate, n, 2, 9)
    xs[0][0, 100] = 0.95  # the peak of buffer 0, far from the NaN
    clean = _host(pkg, xs, rate)
    xs[0][1, 500] = np.nan
    xs[1][0, 600] = -np.inf
    got = _device(torch, eng1, xs, rate)
    assert np.array_equal(got, _host(pkg, xs, rate))
    assert got[0] == clean[0] and got[1] == INF_BITS
    assert _device(torch, eng1, [np.full((2, 40), np.nan, np.float32)], rate)[0] == 0


def test_refusals_write_nothing(pkg, torch, eng1):
    rate, n = 44100, 300
    x = _signals(rate, n, 1, 1)[0]
    src = Buf(torch, 2 * n, np.ascontiguousarray(x.T))
    rec = _record(torch)
    for what, call in (("rate 7999", lambda: eng1.true_peak_device([src.ptr], n, 7999, rec.ptr)),
                       ("rate 192001", lambda: eng1.true_peak_device([src.ptr], n, 192001, rec.ptr)),
                       ("n 2^30", lambda: eng1.true_peak_device([src.ptr], 1 << 30, rate, rec.ptr, 0, 1)),
                       ("frames beyond n", lambda: eng1.true_peak_device([src.ptr], n, rate, rec.ptr, 1, n)),
                       ("first beyond n", lambda: eng1.true_peak_device([src.ptr], n, rate, rec.ptr, n + 1, 0)),
                       ("first_frame < 0", lambda: eng1.true_peak_device([src.ptr], n, rate, rec.ptr, -1, 1)),
                       ("n_frames < 0", lambda: eng1.true_peak_device([src.ptr], n, rate, rec.ptr, 0, -1)),
                       ("null record", lambda: eng1.true_peak_device([src.ptr], n, rate, 0)),
                       ("null buffer", lambda: eng1.true_peak_device([0], n, rate, rec.ptr)),
                       ("five buffers", lambda: eng1.true_peak_device([src.ptr] * 5, n, rate, rec.ptr)),
                       ("n 0", lambda: eng1.true_peak_device([src.ptr], 0, rate, rec.ptr))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
    torch.cuda.synchronize()
    assert rec.unchanged() and src.unchanged()
    eng1.true_peak_device([src.ptr], n, rate, rec.ptr)  # the context works
    torch.cuda.synchronize()
    assert rec.result().view(np.uint32)[0] == pkg.true_peak_host(x, rate)


# ---------------------------------------------------------------- whole tracks
def _held(pkg, outs, tp, rate, what):
    """one track of a true-peak call: its record bit for bit the host function over its own fp32 outputs `outs`"""
    assert (tp.n_out, tp.factor) == (len(outs), ref.factor_of(rate)), (what, tp.n_out, tp.factor)
    for m in range(4):
        want = int(pkg.true_peak_host(outs[m], rate)) if m < len(outs) else 0
        assert _bits(tp.true_peak[m]) == want, (what, m, tp.true_peak[m], pkg.true_peak_float(want))
    return tp


def test_one_lane_and_its_forms(pkg, eng1, wave):
    outs, lv, _, _, tp = eng1.separate_many_true_peak([wave], shift_offsets=[None])
    _same(outs[0], eng1.separate_many([wave], shift_offsets=[None])[0], "stems")
    _held(pkg, outs[0], tp[0], 44100, "one lane, split")
    assert all(_bits(tp[0].true_peak[m]) >= _bits(lv[0].peak[m]) > 0 for m in range(4))
    for shift in (4033, 22049):
        o, _, _, _, t = eng1.separate_many_true_peak([wave], shift_offsets=[shift])
        _held(pkg, o[0], t[0], 44100, ("one lane, shift", shift))
    mixed, lvm, _, _, tpm = eng1.separate_many_true_peak([wave], gains=GAINS, shift_offsets=[4033])
    _same(mixed[0], eng1.separate_many_mix([wave], GAINS, shift_offsets=[4033])[0], "mix")
    _held(pkg, mixed[0], tpm[0], 44100, "mix")
    assert _bits(tpm[0].true_peak[1]) == int(pkg.true_peak_host((0.25 * wave).astype(np.float32), 44100))  # 0.25 x the input itself
    # integer outputs: what is measured is the fp32 sample before the encode
    for fmt, seed in ((pkg.SAMPLE_S16, SEED), (pkg.SAMPLE_S24, None)):
        io = pkg.sample_io(pkg.SAMPLE_F32, fmt, seed)
        q, lvq, _, _, tpq = eng1.separate_many_true_peak([wave], io=io, gains=GAINS, shift_offsets=[4033])
        _same(q[0], eng1.separate_many_io([wave], io=io, gains=GAINS, shift_offsets=[4033])[0], ("integer output", fmt))
        assert bytes(tpq[0]) == bytes(tpm[0]), fmt
    # with the loudness of the same call: neither changes the other
    o, lv2, ld, env, t = eng1.separate_many_true_peak([wave], gains=GAINS, shift_offsets=[4033], loudness=True, envelopes=True)
    want = eng1.separate_many_loudness([wave], gains=GAINS, shift_offsets=[4033])
    assert bytes(t[0]) == bytes(tpm[0]) and bytes(ld[0]) == bytes(want[2][0]) and bytes(lv2[0]) == bytes(want[1][0])
    _same([env[0]], [want[3][0]], "hop energies beside the true peak")


def test_three_lanes_of_unequal_length(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 3000:3000 + 9000]), np.ascontiguousarray(wave[:, 500:500 + 20000])]
    shifts = [11025, None, 0]
    outs, _, _, _, tp = eng3.separate_many_true_peak(xs, shift_offsets=shifts)
    plain = eng3.separate_many(xs, shift_offsets=shifts)
    for ln in range(3):
        _same(outs[ln], plain[ln], ("lanes", ln))
        _held(pkg, outs[ln], tp[ln], 44100, ("lanes", ln))


def test_reset_mode(pkg, eng3, wave):
    for shift in (None, 11025):
        outs, _, _, _, tp = eng3.separate_many_true_peak([wave], flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])
        _same(outs[0], eng3.separate_many([wave], flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])[0], ("reset", shift))
        _held(pkg, outs[0], tp[0], 44100, ("reset", shift))


def test_queue_jobs_equal_the_single_track_call(pkg, eng2, wave):
    lengths, shifts = [LENGTH, 12289, 30000, 4], [None, None, 11025, None]
    xs = [np.ascontiguousarray(wave[:, 40 * i:40 * i + n]) for i, n in enumerate(lengths)]
    got, lvs, lds, envs, tps = eng2.separate_queue(xs, shift_offsets=shifts, true_peak=pkg.TRUE_PEAK_MEASURE)
    calls = eng2.queue_calls()
    plain = eng2.separate_queue(xs, shift_offsets=shifts)
    assert eng2.queue_calls() == calls
    for j, (x, s) in enumerate(zip(xs, shifts)):
        _same(got[j], plain[j], ("queue job", j))
        _held(pkg, got[j], tps[j], 44100, ("queue job", j))
        one = eng2.separate_many_true_peak([x], shift_offsets=[s], loudness=True)
        _same(one[0][0], got[j], ("the job alone", j))
        assert bytes(tps[j]) == bytes(one[4][0]) and bytes(lvs[j]) == bytes(one[1][0]) and bytes(lds[j]) == bytes(one[2][0]), j
    # the queue's other callbacks still get what they got
    _, lv0, ld0, env0 = eng2.separate_queue(xs, shift_offsets=shifts, loudness=True)
    for j in range(4):
        assert bytes(lv0[j]) == bytes(lvs[j]) and bytes(ld0[j]) == bytes(lds[j])
        _same([env0[j]], [envs[j]], ("queue energies", j))
    # mode OFF through the new entry point: the loudness run, and a record of zeros
    off = eng2.separate_queue(xs[:2], shift_offsets=shifts[:2], true_peak=pkg.TRUE_PEAK_OFF)
    for j in range(2):
        _same(off[0][j], plain[j], ("queue, mode off", j))
        assert bytes(off[4][j]) == bytes(pkg.TruePeak()) and bytes(off[1][j]) == bytes(lvs[j])


def test_another_rate(pkg, eng1):
    x48 = pkg.ggml.synth_audio(48000, 73)  # one second at 48 kHz: it leaves by ranges through the resampler
    outs, _, _, _, tp = eng1.separate_many_true_peak([x48], shift_offsets=[4033], rates=[48000])
    _same(outs[0], eng1.separate_many([x48], shift_offsets=[4033], rates=[48000])[0], "48 kHz")
    _held(pkg, outs[0], tp[0], 48000, "48 kHz")
    assert eng1.resample_launches()[1] > 1  # (the condition: more than one range left)
    r, lvr, _, _, tpr = eng1.separate_many_true_peak([x48], clip=pkg.CLIP_RESCALE, gains=GAINS, shift_offsets=[4033], rates=[48000])
    c, lvc, _, _, tpc = eng1.separate_many_true_peak([x48], gains=GAINS, shift_offsets=[4033], rates=[48000])
    assert lvr[0].gain > 1 and bytes(tpr[0]) == bytes(tpc[0])  # measured before the divisor, whole or by ranges
    _held(pkg, c[0], tpc[0], 48000, "48 kHz, mix")


# ---------------------------------------------------------------- the two rescales
def _tone_track(rate=44100):
    """the 45 degree tone at fs/4, amplitude 0.5: sample peak 0.354, true peak about 0.506"""
    return np.ascontiguousarray(ref.tone(rate, 45.0, LENGTH / rate)[:, :LENGTH].astype(np.float32))


TONE_GAINS = np.array([[0, 0, 0, 0, 2.5], [0, 0, 0, 1, 0]], np.float32)  # 2.5 x the tone: sample peak 0.88, true peak about 1.26


def test_measuring_leaves_the_sample_peak_rescale_as_it_is(pkg, eng1, wave):
    for io in (pkg.sample_io(), pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)):
        want, lvw = eng1.separate_many_levels([wave], pkg.CLIP_RESCALE, io, gains=GAINS, shift_offsets=[4033])
        got, lv, _, _, tp = eng1.separate_many_true_peak([wave], pkg.TRUE_PEAK_MEASURE, pkg.CLIP_RESCALE, io, gains=GAINS, shift_offsets=[4033])
        assert lv[0].gain > 1 and lv[0].gain == np.float32(1.01) * max(lv[0].peak[:3])
        _same(got[0], want[0], "sample-peak rescale with the true peak measured")
        assert bytes(lv[0]) == bytes(lvw[0])
    clamp = eng1.separate_many_true_peak([wave], gains=GAINS, shift_offsets=[4033])
    assert bytes(tp[0]) == bytes(clamp[4][0])  # measured before the divisor


def test_true_peak_rescale(pkg, eng1, eng2):
    x = _tone_track()
    clamp, lvc, _, _, tpc = eng1.separate_many_true_peak([x], gains=TONE_GAINS, shift_offsets=[4033])
    _held(pkg, clamp[0], tpc[0], 44100, "tone, clamp")
    peak, tpk = max(lvc[0].peak[:2]), max(tpc[0].true_peak[:2])
    print("tone: sample peak", peak, "true peak", tpk, "dB apart", 20 * np.log10(tpk / peak))
    assert 2.5 < 20 * np.log10(tpk / peak) < 3.5 and np.float32(1.01) * np.float32(peak) <= 1 < tpk  # (the condition)
    # on the sample peak nothing is divided, and what leaves overshoots between the samples
    s, lvs = eng1.separate_many_levels([x], pkg.CLIP_RESCALE, gains=TONE_GAINS, shift_offsets=[4033])
    assert lvs[0].gain == 1 and pkg.true_peak_float(pkg.true_peak_host(s[0][0], 44100)) > 1
    g = np.float32(1.01) * np.float32(tpk)
    for io in (None, pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED), pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S24, None)):
        r, lvr, _, _, tpr = eng1.separate_many_true_peak([x], pkg.TRUE_PEAK_RESCALE, pkg.CLIP_RESCALE, io, gains=TONE_GAINS, shift_offsets=[4033])
        assert lvr[0].gain == g and bytes(tpr[0]) == bytes(tpc[0]), (lvr[0].gain, g)
        assert list(lvr[0].clipped) == [0] * 4 and list(lvr[0].peak) == list(lvc[0].peak)
        if io is None:
            want = [(o / g).astype(np.float32) for o in clamp[0]]  # numpy's float32 quotient is the correctly rounded one
            _same(r[0], want, "x / gain")
            for m in range(2):
                left = pkg.true_peak_float(pkg.true_peak_host(r[0][m], 44100))
                print("true peak of what left", m, left)
                assert left <= 1.0
        elif io.out_format == pkg.SAMPLE_S16:
            want = [pkg.pcm16_encode_host((o / g).astype(np.float32), m, 0, SEED) for m, o in enumerate(clamp[0])]
            _same(r[0], want, "int16 of x / gain")
        else:
            want = [pkg.pcm24_encode_host((o / g).astype(np.float32), m, 0, None) for m, o in enumerate(clamp[0])]
            _same(r[0], want, "24-bit of x / gain")
    # through the queue: the same job
    q = eng2.separate_queue([x, x[:, :20000]], shift_offsets=[4033, None], mix=TONE_GAINS, clip=pkg.CLIP_RESCALE, true_peak=pkg.TRUE_PEAK_RESCALE)
    one = eng2.separate_many_true_peak([x], pkg.TRUE_PEAK_RESCALE, pkg.CLIP_RESCALE, gains=TONE_GAINS, shift_offsets=[4033])
    _same(q[0][0], one[0][0], "queue, true-peak rescale")
    assert bytes(q[1][0]) == bytes(one[1][0]) and bytes(q[4][0]) == bytes(one[4][0]) and q[1][0].gain > 1 and q[1][1].gain > 1


# ---------------------------------------------------------------- the no-op form and the refusals
def test_mode_off_is_the_loudness_call(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 1000:14000])]
    shifts = [4033, None]
    for io in (pkg.sample_io(), pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)):
        for clip in (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE):
            want = eng3.separate_many_loudness(xs, clip, io, gains=GAINS, shift_offsets=shifts)
            launches = eng3.resample_launches()
            got = eng3.separate_many_true_peak(xs, pkg.TRUE_PEAK_OFF, clip, io, gains=GAINS, shift_offsets=shifts, loudness=True, envelopes=True,
                                               records=False)
            assert got[4] is None and eng3.resample_launches() == launches
            for ln in range(2):
                _same(got[0][ln], want[0][ln], ("no-op", ln))
                assert bytes(got[1][ln]) == bytes(want[1][ln]) and bytes(got[2][ln]) == bytes(want[2][ln])
                _same([got[3][ln]], [want[3][ln]], ("no-op: E", ln))
            on = eng3.separate_many_true_peak(xs, pkg.TRUE_PEAK_MEASURE, clip, io, gains=GAINS, shift_offsets=shifts)  # measuring changes no bit
            for ln in range(2):
                _same(on[0][ln], want[0][ln], ("measured", ln))
                assert bytes(on[1][ln]) == bytes(want[1][ln])
    # nothing wanted at all: the plain call
    bare = eng3.separate_many_true_peak(xs, pkg.TRUE_PEAK_OFF, shift_offsets=shifts, levels=False, records=False)
    plain = eng3.separate_many(xs, shift_offsets=shifts)
    for ln in range(2):
        _same(bare[0][ln], plain[ln], ("bare", ln))


def test_refusals_leave_the_context_usable(pkg, eng3, wave, model_small, tmp_path):
    usual = eng3.separate_many([wave], shift_offsets=[4033])[0]
    m = pkg._TrackArgs([wave], pkg.sample_io(), 4, [4033], None)
    for o in m.outs[0]:
        o[:] = 123.0
    io = pkg.sample_io()
    for mode, clip, word in ((3, pkg.CLIP_CLAMP, "unknown"), (-1, pkg.CLIP_RESCALE, "unknown"), (pkg.TRUE_PEAK_RESCALE, pkg.CLIP_CLAMP, "UMX_CLIP_RESCALE")):
        tp = (pkg.TruePeak * 1)()
        rc = eng3.lib.umx_hip_separate_tracks_true_peak(eng3.h, 1, m.a, m.n, m.rt, m.sh, 4, None, m.o, 0, C.byref(io), clip, None, None, None, mode, tp,
                                                        None, None)
        assert rc == pkg.ERR_ARG and "true peak mode" in eng3.last_error() and word in eng3.last_error(), eng3.last_error()
        assert all((o == 123.0).all() for o in m.outs[0]) and bytes(tp[0]) == bytes(pkg.TruePeak())
    # the pinned precedence: formats, clip mode and gains are named first
    rc = eng3.lib.umx_hip_separate_tracks_true_peak(eng3.h, 1, m.a, m.n, m.rt, m.sh, 4, None, m.o, 0, C.byref(io), 2, None, None, None, 3, None, None, None)
    assert rc == pkg.ERR_ARG and "clip mode" in eng3.last_error()
    for rate in (7999, 192001):
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_many_true_peak([wave], shift_offsets=[4033], rates=[rate])
        assert e.value.code == pkg.ERR_ARG and "rate" in eng3.last_error(), eng3.last_error()
    ran = []
    nxt = pkg.QUEUE_NEXT_FN(lambda u, j: ran.append("next") or 0)
    done = pkg.QUEUE_TRUE_PEAK_FN(lambda *a: ran.append("done"))
    assert eng3.lib.umx_hip_separate_queue_true_peak(eng3.h, nxt, pkg.QUEUE_TRUE_PEAK_FN(), None, 4, None, 0, None, 0, 1) == pkg.ERR_ARG
    assert eng3.lib.umx_hip_separate_queue_true_peak(eng3.h, nxt, done, None, 4, None, 0, None, 0, 3) == pkg.ERR_ARG
    assert "true peak mode" in eng3.last_error()
    assert eng3.lib.umx_hip_separate_queue_true_peak(eng3.h, nxt, done, None, 4, None, 0, None, pkg.CLIP_CLAMP, pkg.TRUE_PEAK_RESCALE) == pkg.ERR_ARG
    assert "UMX_CLIP_RESCALE" in eng3.last_error() and ran == []
    _same(eng3.separate_many([wave], shift_offsets=[4033])[0], usual, "fp32 after the refusals")
    # the shift ensemble and the per-segment driver do not offer it: the CLI says so before it opens a file
    cli, wav = Path(pkg.HERE) / "umx-cli", GOLD / "gspi_stereo.wav"
    for extra, word in (({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"), ({"UMX_CLI_PER_SEGMENT": "1"}, "UMX_CLI_PER_SEGMENT")):
        r = _run(cli, [model_small[0], wav, tmp_path / "no"], {"UMX_TRUE_PEAK": "1"}, **extra)
        assert r.returncode == 1 and "UMX_TRUE_PEAK" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(cli, [model_small[0], wav, tmp_path / "no"], {"UMX_TRUE_PEAK": "peak"})
    assert r.returncode == 1 and "UMX_TRUE_PEAK: need 0, 1 or rescale" in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(cli, [model_small[0], wav, tmp_path / "no"], {"UMX_TRUE_PEAK": "rescale"})
    assert r.returncode == 1 and "UMX_CLIP=rescale" in r.stderr and not (tmp_path / "no").exists(), r.stderr


# ---------------------------------------------------------------- the CLI
LINE = re.compile(r"^true_peak (\S+) dbtp=(\S+) linear=(\S+) factor=(\d+)$", re.M)


def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def test_cli_prints_the_true_peak_of_every_file(pkg, model_small, tmp_path):
    path, wav, cli = model_small[0], GOLD / "gspi_stereo.wav", Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": "m=mix;loud=8*mix;hush=0*mix"}
    r = _run(cli, [path, wav, tmp_path / "on"], env, UMX_TRUE_PEAK="1")
    assert r.returncode == 0, r.stderr
    lines = {m[0]: m[1:] for m in LINE.findall(r.stdout)}
    assert len(lines) == 3 and "levels " not in r.stdout and "loudness " not in r.stdout, r.stdout
    for f in ("m.wav", "loud.wav", "hush.wav"):
        p = tmp_path / "on" / f
        out = pkg.wav_load_rate(p)[0]  # the fp32 file IS what left
        want = float(pkg.true_peak_float(pkg.true_peak_host(out, 44100)))
        dbtp, linear, factor = lines[str(p)]
        print("true_peak", f, lines[str(p)], want)
        assert factor == "4" and np.float32(float(linear)) == np.float32(want)
        assert dbtp == "-inf" if want == 0 else abs(float(dbtp) - 20 * np.log10(want)) <= 1e-5
    assert lines[str(tmp_path / "on" / "hush.wav")][0] == "-inf"
    # unset: today's output, and the same files
    r0 = _run(cli, [path, wav, tmp_path / "off"], env)
    assert r0.returncode == 0 and "true_peak " not in r0.stdout, r0.stderr
    for f in ("m.wav", "loud.wav", "hush.wav"):
        assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "on" / f, "rb").read(), f
    # rescale on the true peak: the file's true peak is at most 1 / 1.01 up to rounding
    r1 = _run(cli, [path, wav, tmp_path / "tp"], env, UMX_TRUE_PEAK="rescale", UMX_CLIP="rescale", UMX_LEVELS="1")
    assert r1.returncode == 0, r1.stderr
    tps = {m[0]: float(m[2]) for m in LINE.findall(r1.stdout)}
    gain = float(re.search(r"gain=(\S+)", r1.stdout).group(1))
    assert np.float32(gain) == np.float32(1.01) * np.float32(max(tps.values())) and gain > 1
    left = pkg.wav_load_rate(tmp_path / "tp" / "loud.wav")[0]
    assert pkg.true_peak_float(pkg.true_peak_host(left, 44100)) <= 1.0


def test_batch_prints_the_true_peak_through_the_queue_and_the_loop(pkg, model_small, tmp_path):
    """umx-batch: three files on two lanes (the queue: umx_hip_separate_queue_true_peak) and the pass-by-pass loop
    (umx_hip_separate_tracks_true_peak) print the same line per file written, the host function's over the fp32 file"""
    path, wav, batch = model_small[0], GOLD / "gspi_stereo.wav", Path(pkg.HERE) / "umx-batch"
    q = pkg.wav_load_pcm16(wav)[0]
    files = [wav]
    for i, (a, b) in enumerate(((10000, 90000), (30000, 31000))):
        files.append(tmp_path / f"part{i}.wav")
        pkg.wav_write_pcm16(files[-1], q[:, a:b])
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_BATCH_LANES": "2", "UMX_MIX": "m=mix;loud=8*mix"}
    r0 = _run(batch, [path, tmp_path / "off"] + files, env)
    assert r0.returncode == 0 and "true_peak " not in r0.stdout, r0.stderr
    seen = {}
    for name, extra in (("queue", {}), ("loop", {"UMX_BATCH_QUEUE": "0"})):
        r = _run(batch, [path, tmp_path / name] + files, env, UMX_TRUE_PEAK="1", **extra)
        assert r.returncode == 0 and "loudness " not in r.stdout and "levels " not in r.stdout, r.stderr
        lines = {m[0]: m[1:] for m in LINE.findall(r.stdout)}
        assert len(lines) == 6, r.stdout
        for f in files:
            for out in ("m.wav", "loud.wav"):
                p = tmp_path / name / Path(f).stem / out
                assert open(p, "rb").read() == open(tmp_path / "off" / Path(f).stem / out, "rb").read(), p
                want = float(pkg.true_peak_float(pkg.true_peak_host(pkg.wav_load_rate(p)[0], 44100)))
                dbtp, linear, factor = lines[str(p)]
                assert factor == "4" and np.float32(float(linear)) == np.float32(want) and want > 0, (p, linear, want)
                assert abs(float(dbtp) - 20 * np.log10(want)) <= 1e-5
                seen.setdefault((Path(f).stem, out), []).append(linear)
    assert all(a == b for a, b in seen.values()), seen  # the queue and the loop: the same bits
    # rescale on the true peak through the queue: every file's outputs stay at or below 1 / 1.01 between the samples too
    r = _run(batch, [path, tmp_path / "tp"] + files, env, UMX_TRUE_PEAK="rescale", UMX_CLIP="rescale")
    assert r.returncode == 0, r.stderr
    for f in files:
        left = pkg.wav_load_rate(tmp_path / "tp" / Path(f).stem / "loud.wav")[0]
        assert pkg.true_peak_float(pkg.true_peak_host(left, 44100)) <= 1.0, f
    r = _run(batch, [path, tmp_path / "no"] + files, env, UMX_TRUE_PEAK="rescale")
    assert r.returncode == 1 and "UMX_CLIP=rescale" in r.stderr and not (tmp_path / "no").exists(), r.stderr
