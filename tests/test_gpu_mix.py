"""Stem mix matrix (csrc/stem_mix.h): weighted sums of the four stem slots and of the input mixture, formed on the
device behind the overlap-add.  Held bit for bit against its definition (tests/mix_ref.py) applied to what the unmixed calls
return: the kernel alone on guarded device buffers (out of place and in place, awkward values, unused columns full of inf / NaN
or absent), whole tracks (split and shifted, one and several segments, several lanes, reset mode, flags with a residual slot,
other sample rates, the shift ensemble), the CLIs, the refusals; and within the waveform parity bound of the oracle."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as gd
import mix_ref as mr

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
N = 16 * 1024  # segment_samples: stride 12288
TOL_WAVE = 1e-4  # the project's waveform parity bound (test_gpu_batch.py)
OFFSETS = [0, 11025, 22049]
FP = C.POINTER(C.c_float)
MATRICES = {"identity": mr.IDENTITY, "aggregate": mr.AGGREGATE, "karaoke": mr.KARAOKE}
# every column, gains that round: rows of three and two terms, one whose products overflow, and an empty row
BUSY = np.array([[0.7, -1.3, 1, 0, 0], [0, 0, 0, 1, -0.5], [2, 0, 0, 0, 2], [0, -0.0, 0, 0, 0]], np.float32)


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
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wave(pkg):
    return pkg.ggml.synth_audio(25739, 71)


def _same(got, want, what):
    """Bit for bit; where the definition itself gives a NaN (inf - inf of overflowed products) the positions, not the payloads."""
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float32, (what, m)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, m, "NaN positions")
        assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), (what, m, float(np.nanmax(np.abs(g - w))))


def _inter(x):
    return np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()


# ---------------------------------------------------------------- the kernel alone
class Buf:
    """A guarded device buffer of `frames` frames (tests/guarded.py): the data, or FILL; `lead` extra frames in front of the
    payload's use (a pointer offset by one frame is only 8-byte aligned)."""

    def __init__(self, torch, frames, data=None, misalign=0):
        self.lay = gd.track_layout(2 * frames, misalign)
        self.before = gd.make(self.lay, data)
        self.t = torch.from_numpy(self.before).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lay.pre

    def result(self):
        """guards intact -> the payload"""
        words = self.t.cpu().numpy()
        rep = gd.check(words, self.lay)
        assert rep.pre is None and rep.post is None and rep.holes is None, str(rep)
        return gd.payload(words, self.lay)

    def unchanged(self):
        return gd.untouched(self.t.cpu().numpy(), self.before) is None


def _awkward(seed, n):
    """2n interleaved floats: noise, subnormals, signed zeros and values whose products and sums overflow"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(2 * n).astype(np.float32)
    special = np.concatenate([np.array([1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 0x80000001, 0x807FFFFF], np.uint32).view(np.float32),
                              np.array([0.0, -0.0, 3e38, -3e38, 2.9e38, 1e-38], np.float32)])
    k = min(special.size, 2 * n)
    pos = rng.permutation(2 * n)[:k]
    a[pos] = rng.permutation(special)[:k]
    return a


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_kernel_alone(pkg, torch, eng1, n):
    cols = [_awkward(100 * n + c, n + 1) for c in range(5)]  # one frame more: the call starts at frame 1
    if n >= 3:  # 2 * 3e38 + 2 * -3e38 = inf - inf: a NaN the nonzero gains produce themselves
        cols[0][7], cols[4][7] = 3e38, -3e38
    poison = np.full(2 * (n + 1), np.nan, np.float32)
    poison[::3] = np.inf
    poison[1::3] = -np.inf
    part = BUSY.copy()
    part[:, [1, 4]] = 0  # columns 1 and 4 unused
    for what, gains, data, absent in (("every column", BUSY, cols, ()), ("aggregate", mr.AGGREGATE, cols, ()),
                                     ("poisoned unused columns", part, [cols[0], poison, cols[2], cols[3], poison], ()),
                                     ("absent unused columns", part, cols, (1, 4)), ("identity", mr.IDENTITY, cols, (4,))):
        n_out = gains.shape[0]
        want = mr.mix_fp32([d[2:] for d in data[:4]], data[4][2:], gains)
        ins = [Buf(torch, n + 1, d) for d in data]
        ptrs = [0 if c in absent else ins[c].ptr + 8 for c in range(5)]
        outs = [Buf(torch, n, None, misalign=8 * (m % 2)) for m in range(n_out)]
        eng1.mix_stems_device(gains, ptrs[:4], ptrs[4], n, [o.ptr for o in outs])
        torch.cuda.synchronize()
        _same([o.result() for o in outs], want, (n, what, "out of place"))
        assert all(b.unchanged() for b in ins), (n, what)
        # in place: output m over stem m (exactly n frames each, guards on both sides)
        stems = [Buf(torch, n, d[2:], misalign=8 * (c % 2)) for c, d in enumerate(data[:4])]
        sp = [0 if c in absent else stems[c].ptr for c in range(4)]
        eng1.mix_stems_device(gains, sp, ptrs[4], n, [stems[m].ptr for m in range(n_out)])
        torch.cuda.synchronize()
        _same([stems[m].result() for m in range(n_out)], want, (n, what, "in place"))
        assert all(stems[c].unchanged() for c in range(n_out, 4)), (n, what)
    assert n < 3 or np.isnan(mr.mix_fp32([d[2:] for d in cols[:4]], cols[4][2:], BUSY)[2][5])  # (the NaN rule is exercised)


def test_device_form_refusals_write_nothing(pkg, torch, eng1):
    n = 300
    cols = [Buf(torch, n, _awkward(c, n)) for c in range(5)]
    outs = [Buf(torch, n) for _ in range(4)]
    sp, op = [b.ptr for b in cols[:4]], [o.ptr for o in outs]
    bad = mr.IDENTITY.copy()
    bad[1, 1] = np.inf
    nan = mr.IDENTITY.copy()
    nan[0, 4] = np.nan
    for what, args in (("n_out 0", (np.zeros((0, 5), np.float32), sp, cols[4].ptr, n, op)),
                       ("n_out 5", (np.zeros((5, 5), np.float32), sp, cols[4].ptr, n, op + [op[0]])),
                       ("inf gain", (bad, sp, cols[4].ptr, n, op)), ("NaN gain", (nan, sp, cols[4].ptr, n, op)),
                       ("null output", (mr.IDENTITY, sp, cols[4].ptr, n, [op[0], 0, op[2], op[3]])),
                       ("used stem column without a pointer", (mr.AGGREGATE, [sp[0], 0, sp[2], sp[3]], cols[4].ptr, n, op[:2])),
                       ("used mixture column without a pointer", (mr.KARAOKE, sp, 0, n, op[:1])),
                       ("n = 0", (mr.KARAOKE, sp, cols[4].ptr, 0, op[:1]))):
        with pytest.raises(pkg.UmxError) as e:
            eng1.mix_stems_device(*args)
        assert e.value.code == pkg.ERR_ARG and str(e.value), what
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in cols + outs)
    lib = eng1.lib
    g = np.ascontiguousarray(mr.KARAOKE).ravel()
    assert lib.umx_hip_mix_stems_device(None, 1, g.ctypes.data_as(FP), (C.c_void_p * 4)(*sp), cols[4].ptr, n, (C.c_void_p * 1)(op[0]), None) == pkg.ERR_ARG
    assert lib.umx_hip_mix_stems_device(eng1.h, 1, None, (C.c_void_p * 4)(*sp), cols[4].ptr, n, (C.c_void_p * 1)(op[0]), None) == pkg.ERR_ARG
    assert lib.umx_hip_mix_stems_device(eng1.h, 1, g.ctypes.data_as(FP), (C.c_void_p * 4)(*sp), cols[4].ptr, n, None, None) == pkg.ERR_ARG
    # the mixture alone needs no stems at all
    assert lib.umx_hip_mix_stems_device(eng1.h, 1, np.array([0, 0, 0, 0, 2], np.float32).ctypes.data_as(FP), None, cols[4].ptr, n,
                                        (C.c_void_p * 1)(op[0]), None) == 0
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = np.float32(2) * gd.payload(cols[4].before, cols[4].lay)
    assert np.array_equal(outs[0].result().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- whole tracks
@pytest.mark.parametrize("length", [1, N // 2, 25739])
def test_whole_track_is_the_mix_of_the_unmixed_call(pkg, eng1, wave, length):
    x = np.ascontiguousarray(wave[:, :length])
    for shift in (None, 0, 4033, 22049):
        stems = eng1.separate(x, shift_offset=shift)
        for name, G in MATRICES.items():
            got = eng1.separate_mix(x, G, shift_offset=shift)
            _same(got, mr.mix_fp32(stems, x, G), (length, shift, name))
            if name == "identity":
                _same(got, stems, (length, shift, "identity == separate"))
    assert len(pkg.segment_plan(25739 + 22050, N)[0]) == 4  # several segments, a ragged last one


def test_lanes_of_different_lengths(pkg, eng3, wave):
    xs = [wave, np.ascontiguousarray(wave[:, 3000:3000 + 9000]), np.ascontiguousarray(wave[:, 500:500 + 20000])]
    shifts = [4033, None, 0]
    counts = [len(pkg.segment_plan(x.shape[1] + (0 if s is None else max(22050 - s, s)), N)[0]) for x, s in zip(xs, shifts)]
    assert counts == [4, 1, 4]  # lane 1 idles from the second call on
    plain = eng3.separate_many(xs, shift_offsets=shifts)
    G = np.concatenate([mr.AGGREGATE, mr.KARAOKE])
    got = eng3.separate_many_mix(xs, G, shift_offsets=shifts)
    for ln in range(3):
        _same(got[ln], mr.mix_fp32(plain[ln], xs[ln], G), ("lane", ln))
    # two tracks on three lanes, and no state left behind: the plain call again
    got2 = eng3.separate_many_mix(xs[:2], mr.KARAOKE, shift_offsets=shifts[:2])
    for ln in range(2):
        _same(got2[ln], mr.mix_fp32(plain[ln], xs[ln], mr.KARAOKE), ("two lanes", ln))
    again = eng3.separate_many(xs, shift_offsets=shifts)
    for ln in range(3):
        _same(again[ln], plain[ln], ("plain after mixed", ln))


def test_reset_mode(pkg, eng3, wave):
    flags = pkg.FLAG_RESET_SEGMENTS
    for shift in (None, 4033):
        stems = eng3.separate(wave, flags=flags, shift_offset=shift)
        for name, G in MATRICES.items():
            _same(eng3.separate_mix(wave, G, flags=flags, shift_offset=shift), mr.mix_fp32(stems, wave, G), ("reset", shift, name))
    assert any(not np.array_equal(a, b) for a, b in zip(stems, eng3.separate(wave, shift_offset=4033)))  # (reset mode is another result)


def test_flags_and_the_residual_slot(pkg, eng1, wave):
    flags = pkg.flags_for_targets(["vocals"], residual=True, softmask=True) | pkg.FLAG_WIENER_ITERS(2)
    r = pkg.residual_slot(flags)
    assert r == 0
    names, G = pkg.mix_parse("lead=vocals+0.5*residual;backing=mix-vocals;rest=residual;silent=drums", residual_slot=r)
    assert G[0].tolist() == [0.5, 0, 0, 1, 0]
    stems = eng1.separate(wave, flags=flags, shift_offset=4033)
    got = eng1.separate_mix(wave, G, flags=flags, shift_offset=4033)
    _same(got, mr.mix_fp32(stems, wave, G), "residual flags")
    assert np.abs(got[2]).max() > 0 and np.array_equal(got[2], stems[r])
    assert np.abs(got[3]).max() == 0.0  # a skipped target's slot of zeros is a column like any other
    assert not np.array_equal(got[1], eng1.separate_mix(wave, G, shift_offset=4033)[1])  # (the flags do reach the call)


def _resample(torch, eng, xs, rin, rout, n_out):
    ins = [torch.from_numpy(_inter(x)).cuda() for x in xs]
    outs = [torch.empty(2 * n_out, dtype=torch.float32, device="cuda") for _ in xs]
    eng.resample_device(rin, rout, [t.data_ptr() for t in ins], xs[0].shape[1], [o.data_ptr() for o in outs], n_out)
    torch.cuda.synchronize()
    return [o.cpu().numpy().reshape(n_out, 2).T.copy() for o in outs]


@pytest.mark.parametrize("rate", [48000, 22050])
def test_another_rate_is_mixed_at_44k(pkg, torch, eng1, rate):
    x = pkg.ggml.synth_audio(rate, 73)  # one second
    G = np.concatenate([mr.AGGREGATE, mr.KARAOKE])
    got = eng1.separate_mix(x, G, rate=rate)
    n44 = pkg.resampled_length(x.shape[1], rate, 44100)
    (x44,) = _resample(torch, eng1, [x], rate, 44100, n44)
    mixed44 = mr.mix_fp32(eng1.separate(x44, shift_offset=4033), x44, G)  # column 4: the track's 44.1 kHz version
    _same(got, _resample(torch, eng1, mixed44, 44100, rate, x.shape[1]), rate)
    _same(eng1.separate_mix(x, mr.IDENTITY, rate=rate), eng1.separate(x, rate=rate), (rate, "identity"))
    assert all(g.shape == x.shape and np.isfinite(g).all() and np.abs(g).max() > 0 for g in got)


def test_ensemble_mixes_the_mean(pkg, torch, eng3, wave):
    G = np.concatenate([mr.AGGREGATE, mr.KARAOKE])
    mean = eng3.separate_ensemble(wave, offsets=OFFSETS)
    _same(eng3.separate_ensemble(wave, offsets=OFFSETS, gains=G), mr.mix_fp32(mean, wave, G), "ensemble")
    _same(eng3.separate_ensemble(wave, offsets=OFFSETS, gains=mr.IDENTITY), mean, "ensemble, identity")
    _same(eng3.separate_ensemble(wave, offsets=[700], gains=G), mr.mix_fp32(eng3.separate(wave, shift_offset=700), wave, G), "K = 1")
    # at 48 kHz the mean is mixed at 44.1 kHz (column 4: the resampled track) and the outputs are resampled back
    x = pkg.ggml.synth_audio(48000, 74)
    n44 = pkg.resampled_length(x.shape[1], 48000, 44100)
    (x44,) = _resample(torch, eng3, [x], 48000, 44100, n44)
    mixed44 = mr.mix_fp32(eng3.separate_ensemble(x44, offsets=OFFSETS), x44, G)
    _same(eng3.separate_ensemble(x, offsets=OFFSETS, rate=48000, gains=G), _resample(torch, eng3, mixed44, 44100, 48000, x.shape[1]), "48 kHz")
    _same(eng3.separate_ensemble(x, offsets=OFFSETS, rate=48000, gains=mr.IDENTITY), eng3.separate_ensemble(x, offsets=OFFSETS, rate=48000),
          "48 kHz, identity")
    _same(eng3.separate_ensemble(wave, offsets=OFFSETS), mean, "plain ensemble after mixed ones")


def test_no_state_leaks_into_the_plain_call(pkg, eng1, wave):
    before = eng1.separate(wave, shift_offset=4033)
    eng1.separate_mix(wave, BUSY, shift_offset=4033)
    eng1.separate_mix(wave[:, :5000], mr.KARAOKE)
    _same(eng1.separate(wave, shift_offset=4033), before, "plain after mixed")


def test_accompaniment_against_the_oracle(pkg, po, model_small, eng1, wave):
    _, om, _ = model_small
    G = mr.AGGREGATE[1:]
    bound = TOL_WAVE * float(np.abs(G[0, :4]).sum())  # every stem within TOL_WAVE of the oracle's: the sum within the sum of |gains|
    for shift, ref in ((None, po.split_inference(om, wave, N)), (4033, po.shift_inference(om, wave, N, 4033))):
        want = sum(np.asarray(ref[t], np.float64) for t in range(3))
        got = eng1.separate_mix(wave, G, shift_offset=shift)[0]
        err = float(np.abs(got - want).max())
        print(f"shift {shift}: max |gpu accompaniment - float64 sum of the oracle's stems| = {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (shift, err)


# ---------------------------------------------------------------- C entry points
def test_track_entry_point_refusals_write_nothing(pkg, eng3, wave):
    length = wave.shape[1]
    lay = gd.track_layout(2 * length, misalign=8)
    audio = gd.make(lay, _inter(wave))
    outs = [gd.make(lay) for _ in range(5)]
    before = [o.copy() for o in outs]

    def body(w):
        return C.cast(w.ctypes.data + 4 * lay.pre, FP)

    a = (FP * 1)(body(audio))
    ln, sh = (C.c_int * 1)(length), (C.c_int * 1)(4033)
    arr = (FP * 5)(*[body(o) for o in outs])
    holed = (FP * 4)(arr[0], None, arr[2], arr[3])
    ident = np.ascontiguousarray(mr.IDENTITY).ravel()
    inf, nan = ident.copy(), ident.copy()
    inf[7], nan[19] = -np.inf, np.nan
    g = lambda v: v.ctypes.data_as(FP)  # noqa: E731
    tracks, ens = eng3.lib.umx_hip_separate_tracks_mix, eng3.lib.umx_hip_shift_ensemble_mix
    for what, rc in (("n_out 0", tracks(eng3.h, 1, a, ln, None, sh, 0, g(ident), arr, 0, None, None)),
                     ("n_out 5", tracks(eng3.h, 1, a, ln, None, sh, 5, g(np.zeros(25, np.float32)), arr, 0, None, None)),
                     ("inf", tracks(eng3.h, 1, a, ln, None, sh, 4, g(inf), arr, 0, None, None)),
                     ("NaN", tracks(eng3.h, 1, a, ln, None, sh, 4, g(nan), arr, 0, None, None)),
                     ("no gains", tracks(eng3.h, 1, a, ln, None, sh, 4, None, arr, 0, None, None)),
                     ("no outputs", tracks(eng3.h, 1, a, ln, None, sh, 4, g(ident), None, 0, None, None)),
                     ("a null output", tracks(eng3.h, 1, a, ln, None, sh, 4, g(ident), holed, 0, None, None)),
                     ("no context", tracks(None, 1, a, ln, None, sh, 4, g(ident), arr, 0, None, None)),
                     ("ensemble n_out 0", ens(eng3.h, body(audio), length, 44100, 3, None, 0, g(ident), arr, 0, None, None)),
                     ("ensemble n_out 5", ens(eng3.h, body(audio), length, 44100, 3, None, 5, g(np.zeros(25, np.float32)), arr, 0, None, None)),
                     ("ensemble inf", ens(eng3.h, body(audio), length, 44100, 3, None, 4, g(inf), arr, 0, None, None)),
                     ("ensemble NaN", ens(eng3.h, body(audio), length, 44100, 3, None, 4, g(nan), arr, 0, None, None)),
                     ("ensemble no outputs", ens(eng3.h, body(audio), length, 44100, 3, None, 4, g(ident), None, 0, None, None)),
                     ("ensemble a null output", ens(eng3.h, body(audio), length, 44100, 3, None, 4, g(ident), holed, 0, None, None)),
                     ("ensemble no context", ens(None, body(audio), length, 44100, 3, None, 4, g(ident), arr, 0, None, None))):
        assert rc == pkg.ERR_ARG, what
    assert all(gd.untouched(o, b) is None for o, b in zip(outs, before))
    # and a good call writes exactly `length` frames of n_out buffers, nothing of the others, and leaves the input
    kar = np.ascontiguousarray(np.concatenate([mr.KARAOKE, mr.AGGREGATE])).ravel()
    assert tracks(eng3.h, 1, a, ln, None, sh, 3, g(kar), arr, 0, None, None) == 0, eng3.last_error()
    want = eng3.separate_mix(wave, kar.reshape(3, 5), shift_offset=4033)
    assert gd.check(audio, lay, expect=gd.make(lay, _inter(wave))).ok
    for m in range(3):
        rep = gd.check(outs[m], lay)
        assert rep.ok, (m, str(rep))
        assert np.array_equal(gd.payload(outs[m], lay).reshape(length, 2).T, want[m]), m
    assert gd.untouched(outs[3], before[3]) is None and gd.untouched(outs[4], before[4]) is None


# ---------------------------------------------------------------- the CLIs
SPEC = "vocals=vocals;accompaniment=bass+drums+other;karaoke=mix-vocals;quiet=mix-0.5*vocals"


def _run(tool, args, env, **extra):
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**os.environ, **env, **extra}, timeout=600)


def _files(d):
    return sorted(p.name for p in Path(d).iterdir())


def _check_dir(pkg, d, names, ref):
    assert _files(d) == sorted(f"{n}.wav" for n in names), _files(d)  # the named files, and no target_*.wav
    for m, name in enumerate(names):
        got, ch = pkg.wav_load_rate(d / f"{name}.wav")[:2]
        assert ch == 2 and np.array_equal(got.view(np.uint32), ref[m].view(np.uint32)), name


def test_cli_mix_switch(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    x, _ = pkg.wav_load(wav)
    cli = Path(pkg.HERE) / "umx-cli"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": SPEC}
    names, G = pkg.mix_parse(SPEC)
    eng = pkg.Engine.from_file(path)  # (the CLI's segment size)
    r = _run(cli, [path, wav, tmp_path / "plain"], env)
    assert r.returncode == 0, r.stderr
    _check_dir(pkg, tmp_path / "plain", names, eng.separate_mix(x, G, shift_offset=4033))
    wav48 = tmp_path / "gspi48.wav"
    pkg.wav_write(wav48, x, rate=48000)  # (the same samples, declared 48 kHz)
    r = _run(cli, [path, wav48, tmp_path / "r48"], env, UMX_RESAMPLE="1")
    assert r.returncode == 0, r.stderr
    _check_dir(pkg, tmp_path / "r48", names, eng.separate_mix(x, G, shift_offset=4033, rate=48000))
    eng.close()
    r = _run(cli, [path, wav, tmp_path / "two"], env, UMX_SHIFTS="2")
    assert r.returncode == 0, r.stderr
    eng2 = pkg.Engine.from_file(path, tracks=2)
    _check_dir(pkg, tmp_path / "two", names, eng2.separate_ensemble(x, offsets=pkg.ensemble_offsets(2, 4033), gains=G))
    eng2.close()


def test_batch_mix_switch(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    x, _ = pkg.wav_load(wav)
    y = np.ascontiguousarray(x[:, 10000:90000])
    pkg.wav_write(tmp_path / "short.wav", y)
    spec = "vocals=vocals;karaoke=mix-vocals"
    names, G = pkg.mix_parse(spec)
    r = _run(Path(pkg.HERE) / "umx-batch", [path, tmp_path / "out", wav, tmp_path / "short.wav"], {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": spec})
    assert r.returncode == 0, r.stderr
    eng2 = pkg.Engine.from_file(path, tracks=2)
    refs = eng2.separate_many_mix([x, y], G, shift_offsets=[4033, 4033])
    eng2.close()
    assert _files(tmp_path / "out") == ["gspi_stereo", "short"]
    _check_dir(pkg, tmp_path / "out" / "gspi_stereo", names, refs[0])
    _check_dir(pkg, tmp_path / "out" / "short", names, refs[1])


def test_batch_mix_switch_with_mixed_rates(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    x, _ = pkg.wav_load(wav)
    y = np.ascontiguousarray(x[:, 10000:90000])
    pkg.wav_write(tmp_path / "short48.wav", y, rate=48000)  # (the same samples, declared 48 kHz)
    spec = "acc=bass+drums+other;karaoke=mix-vocals"
    names, G = pkg.mix_parse(spec)
    batch = Path(pkg.HERE) / "umx-batch"
    env = {"UMX_SHIFT_OFFSET": "4033", "UMX_MIX": spec, "UMX_RESAMPLE": "1"}
    r = _run(batch, [path, tmp_path / "out", tmp_path / "short48.wav", wav], env)
    assert r.returncode == 0, r.stderr
    eng2 = pkg.Engine.from_file(path, tracks=2)
    refs = eng2.separate_many_mix([y, x], G, shift_offsets=[4033, 4033], rates=[48000, 44100])
    eng2.close()
    assert _files(tmp_path / "out") == ["gspi_stereo", "short48"]
    _check_dir(pkg, tmp_path / "out" / "short48", names, refs[0])
    _check_dir(pkg, tmp_path / "out" / "gspi_stereo", names, refs[1])
    assert pkg.wav_load_rate(tmp_path / "out" / "short48" / "acc.wav")[2] == 48000
    # its lanes are files: more than one shift is refused with the mix as without it
    r = _run(batch, [path, tmp_path / "no", wav], env, UMX_SHIFTS="2")
    assert r.returncode == 1 and "UMX_SHIFTS" in r.stderr and not (tmp_path / "no").exists(), r.stderr


def test_cli_refusals(pkg, model_small, tmp_path):
    path = model_small[0]
    wav = GOLD / "gspi_stereo.wav"
    cli, batch = Path(pkg.HERE) / "umx-cli", Path(pkg.HERE) / "umx-batch"
    cases = [({"UMX_MIX": "x=guitar"}, "guitar"), ({"UMX_MIX": "x=vocals+vocals"}, "vocals"), ({"UMX_MIX": "x=mix;x=bass"}, "x"),
             ({"UMX_MIX": "a=mix;b=mix;c=mix;d=mix;e=mix"}, "e=mix"), ({"UMX_MIX": "x="}, "x="), ({"UMX_MIX": "x=1e99*mix"}, "1e99"),
             ({"UMX_MIX": "bad name!=mix"}, "badname!"), ({"UMX_MIX": "rest=residual"}, "residual"),
             ({"UMX_MIX": "x=drums+vocals", "UMX_TARGETS": "vocals"}, "drums"),                      # a source that does not run
             ({"UMX_MIX": "x=bass+vocals", "UMX_TARGETS": "vocals,drums", "UMX_RESIDUAL": "1"}, None)]  # bass's slot IS the residual's: fine
    for env, piece in cases[:-1]:
        for tool, args in ((cli, [path, wav, tmp_path / "bad"]), (batch, [path, tmp_path / "bad", wav])):
            r = _run(tool, args, env)
            assert r.returncode == 1 and "UMX_MIX" in r.stderr and piece in r.stderr, (env, r.stderr)
    r = _run(cli, [path, wav, tmp_path / "bad"], {"UMX_MIX": "x=mix", "UMX_CLI_PER_SEGMENT": "1"})
    assert r.returncode == 1 and "UMX_MIX" in r.stderr and "UMX_CLI_PER_SEGMENT" in r.stderr, r.stderr
    assert not (tmp_path / "bad").exists()
    r = _run(cli, [path, wav, tmp_path / "ok"], cases[-1][0])
    assert r.returncode == 0 and _files(tmp_path / "ok") == ["x.wav"], r.stderr
