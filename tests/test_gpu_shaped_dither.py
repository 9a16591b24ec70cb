"""Noise-shaped dither for 16-bit outputs on the device (csrc/pcm16_shaped.h), bit for bit against the host rule
(umx_hip_pcm16_encode_host with UMX_DITHER_SHAPED, itself held to tests/shaped_ref.py by the CPU test): the kernel alone on guarded
buffers, the whole-track calls and the queue against the host rule on the fp32 outputs of the same call, and the refusals."""
import numpy as np
import pytest

import levels_ref
import shaped_ref
from test_gpu_pcm16 import Buf, _frames

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: stride 12288, so regions cut the blocks of 4096 frames
SEED = 7


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()
    return t


@pytest.fixture(scope="module")
def eng(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=2)
    yield e
    e.close()


def _floats(seed, n):
    x = (np.random.default_rng(seed).standard_normal((2, n)) * 0.4).astype(np.float32)
    x[:, ::5] *= 4  # beyond full scale
    if n > 40:
        x[0, 17], x[1, 23], x[0, 31] = np.nan, np.inf, -np.inf
    return x


@pytest.mark.parametrize("first", [0, 4096])
@pytest.mark.parametrize("n", [1, 5, 4095, 4096, 4097, 2 * 4096 + 17])
def test_kernel_equals_the_host_rule(pkg, torch, eng, n, first):
    for nb in (1, 4):
        xs = [_floats(100 * n + b, n) for b in range(nb)]
        ins = [Buf(torch, 2 * n, np.ascontiguousarray(x.T)) for x in xs]
        outs = [Buf(torch, n) for _ in range(nb)]
        eng.pcm16_encode_device([b.ptr for b in ins], n, [o.ptr for o in outs], first, SEED, shaped=True)
        torch.cuda.synchronize()
        for b, (x, o) in enumerate(zip(xs, outs)):  # (result(): guards intact -- exactly n frames were written)
            assert np.array_equal(_frames(o.result()), pkg.pcm16_encode_host(x, b, first, SEED, shaped=True)), (n, first, nb, b)
        # over the divisor of a record's peak words, counting what clamps: a record that divides, and one whose divisor is 1
        for peaks in ([float(np.nanmax(np.abs(x[np.isfinite(x)]))) for x in xs], [0.5] * nb):
            g = levels_ref.gain(np.array(peaks, np.float32))
            words = np.zeros(28, np.int32)
            words[:nb] = np.array(peaks, np.float32).view(np.int32)
            acc, outs = Buf(torch, 28, words), [Buf(torch, n) for _ in range(nb)]
            eng.pcm16_encode_rescaled_device([b.ptr for b in ins], n, [o.ptr for o in outs], acc.ptr, first, SEED, shaped=True)
            torch.cuda.synchronize()
            counts = acc.result()[12:20].view(np.uint64)
            for b, (x, o) in enumerate(zip(xs, outs)):
                want, clipped = shaped_ref.encode(x, b, first, SEED, None if g == 1 else g)
                assert np.array_equal(pkg.pcm16_encode_host(levels_ref.rescaled(x, g), b, first, SEED, shaped=True), want)
                assert np.array_equal(_frames(o.result()), want) and counts[b] == clipped, (n, first, nb, b, g, counts, clipped)
                assert g != 1 or n < 40 or clipped > 0
        assert all(b.unchanged() for b in ins)


def _host(pkg, stems):
    return [pkg.pcm16_encode_host(s, m, 0, SEED, shaped=True) for m, s in enumerate(stems)]


@pytest.fixture(scope="module")
def waves(pkg):
    return [pkg.ggml.synth_audio(25739, 71), pkg.ggml.synth_audio(9001, 72)]  # three segments and one: two lanes of different lengths


@pytest.mark.parametrize("case", ["carry", "reset", "48k", "queue"])
def test_whole_tracks_equal_the_host_rule_on_the_fp32_outputs(pkg, eng, waves, case):
    S16, F32 = pkg.SAMPLE_S16, pkg.SAMPLE_F32
    if case == "reset":  # the segments of ONE track as the lanes
        kw = dict(flags=pkg.FLAG_RESET_SEGMENTS, shift_offsets=[11025])
        xs = waves[:1]
    else:
        kw = dict(shift_offsets=[4033, None], rates=[48000, 44100] if case == "48k" else None)
        xs = waves
    if case == "queue":
        plain = eng.separate_queue(xs, shift_offsets=kw["shift_offsets"])
        got = eng.separate_queue(xs, shift_offsets=kw["shift_offsets"], io=pkg.sample_io(F32, S16, SEED), shaped=True)
    else:
        plain = eng.separate_many(xs, **kw)
        got = eng.separate_many_io(xs, F32, S16, SEED, shaped=True, **kw)
    for ln, (g, p) in enumerate(zip(got, plain)):
        for m, (a, b) in enumerate(zip(g, _host(pkg, p))):
            assert a.dtype == np.int16 and np.array_equal(a, b), (case, ln, m, np.flatnonzero((a != b).any(axis=0))[:4])


def test_clamp_mode_levels_count_what_the_shaped_encode_clamps(pkg, eng, waves):
    gains = np.array([[60, 0, 0, 0, 0], [0, 0, 0, -1, 1]], np.float32)  # a row far beyond full scale, and one that is not
    plain = eng.separate_many_mix(waves, gains, shift_offsets=[4033, None])
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED, shaped=True)
    got, levels = eng.separate_many_levels(waves, io=io, gains=gains, shift_offsets=[4033, None])
    for ln, (g, p) in enumerate(zip(got, plain)):
        for m, s in enumerate(p):
            want, clipped = shaped_ref.encode(s, m, 0, SEED)
            assert np.array_equal(g[m], want) and levels[ln].clipped[m] == clipped, (ln, m, levels[ln].clipped[m], clipped)
        assert levels[ln].clipped[0] > 0


def test_refusals_leave_the_context_usable(pkg, torch, eng, waves):
    S16, S24, F32 = pkg.SAMPLE_S16, pkg.SAMPLE_S24, pkg.SAMPLE_F32
    src, dst, acc = Buf(torch, 128, np.zeros(128, np.float32)), Buf(torch, 128), Buf(torch, 28, np.zeros(28, np.int32))
    x = waves[1:]
    shaped = lambda out: pkg.sample_io(F32, out, SEED, shaped=True)
    for word, call in (("4096", lambda: eng.pcm16_encode_device([src.ptr], 8, [dst.ptr], 5, SEED, shaped=True)),
                       ("4096", lambda: eng.pcm16_encode_rescaled_device([src.ptr], 8, [dst.ptr], acc.ptr, 4095, SEED, shaped=True)),
                       ("16-bit", lambda: eng._encode_device(24, [src.ptr], 8, [dst.ptr], 0, SEED, None, shaped=True)),
                       ("16-bit", lambda: eng.levels_device([src.ptr], 8, acc.ptr, io=shaped(S16))),
                       ("16-bit", lambda: eng.separate_many_io(x, io=shaped(S24))),
                       ("16-bit", lambda: eng.separate_many_io(x, io=shaped(F32))),
                       ("16-bit", lambda: eng.separate_many_flac(x, 16, io=shaped(F32))),
                       ("44100 or 48000", lambda: eng.separate_many_io(x, io=shaped(S16), rates=[22050])),
                       ("44100 or 48000", lambda: eng.separate_queue(x, io=shaped(S16), rates=[96000])),
                       ("unknown dither mode", lambda: eng.separate_many_io(x, io=pkg.SampleIO(F32, S16, 3, SEED)))):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and word in str(e.value), (word, str(e.value))
    torch.cuda.synchronize()
    assert dst.unchanged() and acc.unchanged()
    got = eng.separate_many_io(x, F32, S16, SEED, shaped=True)[0]
    assert all(np.array_equal(a, b) for a, b in zip(got, _host(pkg, eng.separate_many(x)[0])))
