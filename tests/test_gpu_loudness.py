"""Loudness of every output (csrc/loudness.h) on the GPU: the hop kernel alone on guarded device buffers (E itself guarded)
against the rule of tests/loudness_ref.py, and the whole-track drivers -- one lane, lanes of unequal length, reset mode, the queue, a
mix, a dithered int16 output, rescale, another sample rate -- each held to the reference evaluated on that path's own fp32 outputs,
its records to the gate of its own energies, and paths that return the same stems to the same bits of E."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import loudness_ref as ref

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
STRIDE = 12288
SEED = 7
LENGTH = 5 * STRIDE  # 61440 frames: five segments; at 44100 Hz 13 hops and 10 blocks
GAINS = np.array([[0, 0, 0, 0, 3], [0, 0, 0, 0, 0.25], [0, 0, 0, 1, 0]], np.float32)  # as tests/test_gpu_levels.py
WORST = {"relative": 0.0}  # the largest relative deviation of a device hop energy from the reference's rule, over this module


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
    assert x.shape == (2, LENGTH) and LENGTH // ref.hop_of(44100) == 13
    return x


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = {4: np.uint32, 2: np.uint16, 8: np.uint64}[g.dtype.itemsize]
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


def _within(got, want, what):
    """device hop energies (..., hops) against the reference's rule: 1e-9 E + 1e-9 E_prev"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, tol = np.abs(got - want), ref.tolerance(want)
    rel = float(np.max(err / np.maximum(np.abs(want), 1e-300))) if want.size else 0.0
    WORST["relative"] = max(WORST["relative"], rel)
    print("hop energies", what, "largest deviation / tolerance", float(np.max(err / np.maximum(tol, 1e-300))) if want.size else 0.0, "relative", rel,
          "largest so far", WORST["relative"])
    assert (err <= tol).all(), (what, np.argwhere(err > tol)[:4], got[err > tol][:4], want[err > tol][:4])


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


FILL64 = np.array([gd.FILL, gd.FILL], np.int32).view(np.float64)[0]  # (a NaN pattern: what an entry nobody wrote holds)


def _E(torch, nb, hops):
    return Buf(torch, 2 * max(1, nb * 2 * hops))


def _E_result(buf, nb, hops):
    """-> (nb, 2, hops) float64 and the mask of the entries that still hold the fill"""
    w = buf.result()[:2 * nb * 2 * hops].view(np.float64).reshape(nb, 2, hops)
    return w, w.view(np.uint64) == np.array([FILL64]).view(np.uint64)[0]


def _signals(rate, n, nb, seed):
    xs = [ref.stepped_noise(rate, n, seed + b) for b in range(nb)]
    for b, x in enumerate(xs):
        x *= np.float32(1.0 + 0.5 * b)
    return xs


@pytest.mark.parametrize("rate", [8000, 44100, 192000])
def test_hop_kernel_alone(pkg, torch, eng1, rate):
    hop = ref.hop_of(rate)
    n, hops = 7 * hop + 123, 7
    for nb in (1, 4):
        for off in (0, 1):  # the buffers start one frame into their allocation: 8-byte aligned, not 16
            xs = _signals(rate, n + off, nb, 100 * nb + off)
            ins = [Buf(torch, 2 * (n + off), np.ascontiguousarray(x.T), misalign=8 * (1 - off)) for x in xs]
            ptrs = [b.ptr + 8 * off for b in ins]
            want = np.stack([ref.hop_energies(x[:, off:], rate) for x in xs])
            # all hops in one launch
            E = _E(torch, nb, hops)
            eng1.kweight_hops_device(ptrs, n, rate, E.ptr)
            torch.cuda.synchronize()
            whole, fill = _E_result(E, nb, hops)
            assert not fill.any()
            _within(whole, want, (rate, nb, off))
            # a span: exactly the asked entries are written
            E = _E(torch, nb, hops)
            eng1.kweight_hops_device(ptrs, n, rate, E.ptr, 2, 3)
            torch.cuda.synchronize()
            part, fill = _E_result(E, nb, hops)
            assert fill[:, :, :2].all() and fill[:, :, 5:].all() and not fill[:, :, 2:5].any()
            _same([part[:, :, 2:5].copy()], [whole[:, :, 2:5].copy()], (rate, nb, off, "a span's bits"))
            # the same span in three launches cut at arbitrary hops: the same bits
            E = _E(torch, nb, hops)
            for a, b in ((5, 7), (0, 1), (1, 5)):
                eng1.kweight_hops_device(ptrs, n, rate, E.ptr, a, b - a)
            torch.cuda.synchronize()
            cut, fill = _E_result(E, nb, hops)
            assert not fill.any()
            _same([cut], [whole], (rate, nb, off, "three launches"))
            assert all(b.unchanged() for b in ins)


def test_hop_kernel_more_than_one_workgroup(pkg, torch, eng1):
    """131 hops at 8000 Hz: three workgroups per buffer, the last with three rows; cut at the workgroup edge and off it"""
    rate, hop = 8000, 800
    n, hops = 131 * hop + 799, 131
    xs = _signals(rate, n, 2, 9)
    ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T)) for x in xs]
    E = _E(torch, 2, hops)
    eng1.kweight_hops_device([b.ptr for b in ins], n, rate, E.ptr)
    torch.cuda.synchronize()
    whole, fill = _E_result(E, 2, hops)
    assert not fill.any()
    _within(whole, np.stack([ref.hop_energies(x, rate) for x in xs]), "131 hops")
    E = _E(torch, 2, hops)
    for a, b in ((0, 64), (64, 65), (65, 131)):
        eng1.kweight_hops_device([b_.ptr for b_ in ins], n, rate, E.ptr, a, b - a)
    torch.cuda.synchronize()
    _same([_E_result(E, 2, hops)[0]], [whole], "131 hops in three launches")


def test_a_nan_and_an_inf_reach_two_hops(pkg, torch, eng1):
    rate, hop = 44100, 4410
    n, hops = 7 * hop + 123, 7
    clean = _signals(rate, n, 2, 3)
    want = np.stack([ref.hop_energies(x, rate) for x in clean])
    xs = [x.copy() for x in clean]
    xs[0][1, 2 * hop + hop // 2] = np.nan   # buffer 0, right channel, mid hop 2: hops 2 and 3
    xs[1][0, 4 * hop + hop // 3] = -np.inf  # buffer 1, left channel, mid hop 4: hops 4 and 5
    ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T)) for x in xs]
    E = _E(torch, 2, hops)
    eng1.kweight_hops_device([b.ptr for b in ins], n, rate, E.ptr)
    torch.cuda.synchronize()
    got, fill = _E_result(E, 2, hops)
    assert not fill.any()
    hit = np.zeros((2, 2, hops), bool)
    hit[0, 1, 2:4] = hit[1, 0, 4:6] = True
    assert np.array_equal(~np.isfinite(got), hit), np.argwhere(~np.isfinite(got))
    assert np.isnan(got[0, 1, 2:4]).all() and not np.isfinite(got[1, 0, 4]) and not np.isfinite(got[1, 0, 5])
    _within(np.where(hit, 0.0, got), np.where(hit, 0.0, want), "beside the NaN and the inf")
    host = np.stack([pkg.kweight_hops_host(x, rate) for x in xs])  # the host statement of the rule: the same two hops
    assert np.array_equal(~np.isfinite(host), hit)


def test_short_inputs_and_refusals_write_nothing(pkg, torch, eng1):
    rate, hop = 44100, 4410
    src = Buf(torch, 2 * (hop + 5), np.zeros(2 * (hop + 5), np.float32))
    E = _E(torch, 1, 1)
    eng1.kweight_hops_device([src.ptr], hop - 1, rate, E.ptr)  # n < hop: no hop, nothing launched
    eng1.kweight_hops_device([src.ptr], hop + 5, rate, E.ptr, 1, 0)  # no hop asked
    torch.cuda.synchronize()
    assert E.unchanged() and src.unchanged()
    for what, call in (("rate 7999", lambda: eng1.kweight_hops_device([src.ptr], hop, 7999, E.ptr)),
                       ("rate 192001", lambda: eng1.kweight_hops_device([src.ptr], hop, 192001, E.ptr)),
                       ("hops beyond n / hop", lambda: eng1.kweight_hops_device([src.ptr], hop + 5, rate, E.ptr, 0, 2)),
                       ("first_hop < 0", lambda: eng1.kweight_hops_device([src.ptr], hop + 5, rate, E.ptr, -1, 1)),
                       ("null E", lambda: eng1.kweight_hops_device([src.ptr], hop + 5, rate, 0)),
                       ("null buffer", lambda: eng1.kweight_hops_device([0], hop + 5, rate, E.ptr)),
                       ("five buffers", lambda: eng1.kweight_hops_device([src.ptr] * 5, hop + 5, rate, E.ptr)),
                       ("n 0", lambda: eng1.kweight_hops_device([src.ptr], 0, rate, E.ptr))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
    torch.cuda.synchronize()
    assert E.unchanged() and src.unchanged()
    eng1.kweight_hops_device([src.ptr], hop + 5, rate, E.ptr)  # the context works: one hop of silence
    torch.cuda.synchronize()
    assert np.array_equal(_E_result(E, 1, 1)[0], np.zeros((1, 2, 1)))


# ---------------------------------------------------------------- whole tracks
def _held(pkg, outs, ld, env, rate, what):
    """one track of a loudness call: its energies against the reference on its own fp32 outputs `outs`, its record against the gate
    of its own energies"""
    hop = ref.hop_of(rate)
    hops = outs[0].shape[1] // hop
    assert env.shape == (len(outs), 2, hops) and (ld.n_out, ld.hop, ld.hops) == (len(outs), hop, hops), (what, env.shape, ld.n_out, ld.hop, ld.hops)
    _within(env, np.stack([ref.hop_energies(o, rate) for o in outs]), what)
    for m in range(4):
        want = pkg.loudness_gate(env[m], hop) if m < len(outs) else (-np.inf, -np.inf, 0, 0)
        assert (ld.integrated[m], ld.momentary_max[m], ld.blocks[m], ld.gated[m]) == want, (what, m, want)
    return env


def test_one_lane_and_its_forms(pkg, eng1, wave):
    """fp32 stems, the mix, the dithered int16 output and rescale of ONE track: the energies are those of the fp32 samples that leave
    before any encode or divisor, so the int16 and the rescaled call carry the fp32 clamp call's bits of E"""
    outs, lv, ld, env = eng1.separate_many_loudness([wave], shift_offsets=[None])
    _same(outs[0], eng1.separate_many([wave], shift_offsets=[None])[0], "stems")
    assert ld[0].hops == 13 and list(ld[0].blocks) == [10] * 4
    _held(pkg, outs[0], ld[0], env[0], 44100, "one lane")
    assert all(np.isfinite(ld[0].integrated[m]) and ld[0].gated[m] > 0 for m in range(4))  # (the condition: the stems are not silent)
    for shift in (4033, 22049):  # the track behind a shift's padding: frame 0 of the caller's track is still hop 0's first
        o, _, l, e = eng1.separate_many_loudness([wave], shift_offsets=[shift])
        _held(pkg, o[0], l[0], e[0], 44100, ("one lane, shift", shift))
    mixed, _, ldm, envm = eng1.separate_many_loudness([wave], gains=GAINS, shift_offsets=[4033])
    _same(mixed[0], eng1.separate_many_mix([wave], GAINS, shift_offsets=[4033])[0], "mix")
    _held(pkg, mixed[0], ldm[0], envm[0], 44100, "mix")
    # 3 x mix and 0.25 x mix: 20 log10(12) apart, whatever the track
    assert abs((ldm[0].integrated[0] - ldm[0].integrated[1]) - 20 * np.log10(12.0)) < 1e-3
    # the input's own loudness is the host rule's on the input
    assert abs(ldm[0].integrated[1] - (pkg.loudness_gate(pkg.kweight_hops_host(wave, 44100), 4410)[0] + 20 * np.log10(0.25))) < 1e-3
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)
    q, _, ldq, envq = eng1.separate_many_loudness([wave], io=io, gains=GAINS, shift_offsets=[4033])
    assert q[0][0].dtype == np.int16
    _same([envq[0]], [envm[0]], "int16 with dither: E")
    assert bytes(ldq[0]) == bytes(ldm[0])
    for io_ in (None, io):
        r, lvr, ldr, envr = eng1.separate_many_loudness([wave], clip=pkg.CLIP_RESCALE, io=io_, gains=GAINS, shift_offsets=[4033])
        assert lvr[0].gain > 1  # (the condition: the 3 x mix row passes full scale, the track is divided)
        _same([envr[0]], [envm[0]], "rescale: E is measured before the divisor")
        assert bytes(ldr[0]) == bytes(ldm[0])
    _same(r[0], eng1.separate_many_levels([wave], pkg.CLIP_RESCALE, io, gains=GAINS, shift_offsets=[4033])[0][0], "rescaled outputs")


def test_three_lanes_of_unequal_length(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 3000:3000 + 9000]), np.ascontiguousarray(wave[:, 500:500 + 20000]), ]
    shifts = [11025, None, 0]
    outs, lv, ld, env = eng3.separate_many_loudness(xs, shift_offsets=shifts)
    plain = eng3.separate_many(xs, shift_offsets=shifts)
    assert [l.hops for l in ld] == [13, 2, 4]
    for ln in range(3):
        _same(outs[ln], plain[ln], ("lanes", ln))
        _held(pkg, outs[ln], ld[ln], env[ln], 44100, ("lanes", ln))
    assert list(ld[1].blocks) == [0] * 4 and ld[1].integrated[0] == -np.inf  # two hops: no block


def test_reset_mode(pkg, eng3, wave):
    for shift in (None, 11025):
        outs, lv, ld, env = eng3.separate_many_loudness([wave], flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])
        _same(outs[0], eng3.separate_many([wave], flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[shift])[0], ("reset", shift))
        _held(pkg, outs[0], ld[0], env[0], 44100, ("reset", shift))


def test_queue_jobs_equal_the_single_track_call(pkg, eng2, wave):
    lengths, shifts = [LENGTH, 12289, 30000, 4409], [None, None, 11025, None]
    xs = [np.ascontiguousarray(wave[:, 40 * i:40 * i + n]) for i, n in enumerate(lengths)]
    got, lvs, lds, envs = eng2.separate_queue(xs, shift_offsets=shifts, loudness=True)
    plain = eng2.separate_queue(xs, shift_offsets=shifts)
    assert [l.hops for l in lds] == [13, 2, 6, 0]
    for j, (x, s) in enumerate(zip(xs, shifts)):
        _same(got[j], plain[j], ("queue job", j))
        _held(pkg, got[j], lds[j], envs[j], 44100, ("queue job", j))
        one, lv1, ld1, env1 = eng2.separate_many_loudness([x], shift_offsets=[s])
        _same(one[0], got[j], ("the job alone", j))  # bit-identical stems ...
        _same([envs[j]], [env1[0]], ("the job alone: E", j))  # ... so bit-identical energies
        assert bytes(lds[j]) == bytes(ld1[0]) and bytes(lvs[j]) == bytes(lv1[0]), j
    mixed, _, ldm, envm = eng2.separate_queue(xs[:2], shift_offsets=shifts[:2], mix=GAINS, clip=pkg.CLIP_RESCALE, loudness=True)
    for j in range(2):
        clamp = eng2.separate_many_loudness([xs[j]], gains=GAINS, shift_offsets=[shifts[j]])
        _same([envm[j]], [clamp[3][0]], ("a rescaled queue job: E before the divisor", j))
        _held(pkg, clamp[0][0], ldm[j], envm[j], 44100, ("a rescaled queue job", j))


def test_another_rate(pkg, eng1):
    x48 = pkg.ggml.synth_audio(48000, 73)  # one second at 48 kHz: ten hops of 4800
    outs, lv, ld, env = eng1.separate_many_loudness([x48], shift_offsets=[4033], rates=[48000])
    _same(outs[0], eng1.separate_many([x48], shift_offsets=[4033], rates=[48000])[0], "48 kHz")
    assert (ld[0].hop, ld[0].hops) == (4800, 10)
    _held(pkg, outs[0], ld[0], env[0], 48000, "48 kHz")
    r, lvr, ldr, envr = eng1.separate_many_loudness([x48], clip=pkg.CLIP_RESCALE, gains=GAINS, shift_offsets=[4033], rates=[48000])
    c, lvc, ldc, envc = eng1.separate_many_loudness([x48], gains=GAINS, shift_offsets=[4033], rates=[48000])
    assert lvr[0].gain > 1
    _same([envr[0]], [envc[0]], "48 kHz, rescale: E before the divisor")
    _held(pkg, c[0], ldr[0], envr[0], 48000, "48 kHz, rescale")


# ---------------------------------------------------------------- the no-op form and the refusals
def test_without_loudness_it_is_the_levels_call(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 1000:14000])]
    shifts = [4033, None]
    for io in (pkg.sample_io(), pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED)):
        for clip in (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE):
            want, lvw = eng3.separate_many_levels(xs, clip, io, gains=GAINS, shift_offsets=shifts)
            got, lv, ld, env = eng3.separate_many_loudness(xs, clip, io, gains=GAINS, shift_offsets=shifts, loudness=False, envelopes=False)
            assert ld is None and env is None
            for ln in range(2):
                _same(got[ln], want[ln], ("no-op", ln))
                assert bytes(lv[ln]) == bytes(lvw[ln])
            got, lv, ld, env = eng3.separate_many_loudness(xs, clip, io, gains=GAINS, shift_offsets=shifts)  # measuring changes no bit
            for ln in range(2):
                _same(got[ln], want[ln], ("with loudness", ln))
                assert bytes(lv[ln]) == bytes(lvw[ln])
    # the records alone, and the energies alone, measure the same
    a = eng3.separate_many_loudness(xs, gains=GAINS, shift_offsets=shifts, envelopes=False)
    b = eng3.separate_many_loudness(xs, gains=GAINS, shift_offsets=shifts, loudness=False)
    for ln in range(2):
        assert bytes(a[2][ln]) == bytes(ld[ln])
        _same([b[3][ln]], [env[ln]], ("energies alone", ln))


def test_refusals_leave_the_context_usable(pkg, eng3, wave, model_small, tmp_path):
    usual = eng3.separate_many([wave], shift_offsets=[4033])[0]
    for rate in (7999, 192001):
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_many_loudness([wave], shift_offsets=[4033], rates=[rate])
        assert e.value.code == pkg.ERR_ARG and "rate" in eng3.last_error(), eng3.last_error()
    with pytest.raises(pkg.UmxError) as e:
        eng3.separate_many_loudness([wave], clip=2, shift_offsets=[4033])
    assert "clip mode" in eng3.last_error()
    nxt = pkg.QUEUE_NEXT_FN(lambda u, j: 0)
    assert eng3.lib.umx_hip_separate_queue_loudness(eng3.h, nxt, pkg.QUEUE_LOUDNESS_FN(), None, 4, None, 0, None, 0) == pkg.ERR_ARG
    assert eng3.lib.umx_hip_separate_queue_loudness(eng3.h, nxt, pkg.QUEUE_LOUDNESS_FN(lambda *a: None), None, 4, None, 0, None, 3) == pkg.ERR_ARG
    assert "clip mode" in eng3.last_error()
    _same(eng3.separate_many([wave], shift_offsets=[4033])[0], usual, "fp32 after the refusals")
    # the shift ensemble and the per-segment driver do not offer it: the CLI says so before it opens a file
    cli, wav = Path(pkg.HERE) / "umx-cli", GOLD / "gspi_stereo.wav"
    for extra, word in (({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"), ({"UMX_CLI_PER_SEGMENT": "1"}, "UMX_CLI_PER_SEGMENT")):
        r = _run(cli, [model_small[0], wav, tmp_path / "no"], {"UMX_LOUDNESS": "1"}, **extra)
        assert r.returncode == 1 and "UMX_LOUDNESS" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = _run(cli, [model_small[0], wav, tmp_path / "no"], {"UMX_LOUDNESS": "loud"})
    assert r.returncode == 1 and "UMX_LOUDNESS: need 0 or 1" in r.stderr and not (tmp_path / "no").exists(), r.stderr


# ---------------------------------------------------------------- the CLI
LINE = re.compile(r"^loudness (\S+) integrated=(\S+) momentary_max=(\S+) blocks=(\d+) gated=(\d+)$", re.M)


def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def test_cli_prints_the_loudness_of_every_file(pkg, model_small, tmp_path):
    path, wav, cli = model_small[0], GOLD / "gspi_stereo.wav", Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": "m=mix;vocals=vocals;hush=0*mix"}
    r = _run(cli, [path, wav, tmp_path / "on"], env, UMX_LOUDNESS="1")
    assert r.returncode == 0, r.stderr
    lines = {m[0]: m[1:] for m in LINE.findall(r.stdout)}
    assert len(lines) == 3 and "levels " not in r.stdout, r.stdout
    x = pkg.wav_load_rate(wav)[0]
    for f in ("m.wav", "vocals.wav", "hush.wav"):
        p = tmp_path / "on" / f
        out = pkg.wav_load_rate(p)[0]  # the fp32 file IS what left
        i, m, b, g = pkg.loudness_gate(pkg.kweight_hops_host(out, 44100), 4410)
        got = lines[str(p)]
        print("loudness", f, got, (i, m, b, g))
        assert (int(got[2]), int(got[3])) == (b, g) and b == x.shape[1] // 4410 - 3
        for text, want in ((got[0], i), (got[1], m)):
            assert text == "-inf" if want == -np.inf else abs(float(text) - want) <= 1e-6, (f, text, want)
    assert lines[str(tmp_path / "on" / "hush.wav")][:2] == ("-inf", "-inf")
    # UMX_MIX="m=mix": the loudness of the input itself
    want = pkg.loudness_gate(pkg.kweight_hops_host(x, 44100), 4410)[0]
    assert np.isfinite(want) and abs(float(lines[str(tmp_path / "on" / "m.wav")][0]) - want) <= 1e-5
    # unset: today's output, and the same files
    r0 = _run(cli, [path, wav, tmp_path / "off"], env)
    assert r0.returncode == 0 and "loudness " not in r0.stdout, r0.stderr
    for f in ("m.wav", "vocals.wav", "hush.wav"):
        assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "on" / f, "rb").read(), f
