"""The look-ahead peak limiter on the device (csrc/limiter.h), without tolerances: the gain and apply kernels against the
host call on guarded buffers around the gain kernel's tile, ranges against the whole call, the whole-track call against the call
without a limiter with the host rule applied, the rescale refusal, and umx-cli's UMX_LIMIT against the Python path."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded
import limit_ref
from limit_ref import T, same_bits

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: the small context of tests/test_gpu_pcm24.py
CEILING = np.float32(10 ** (-1 / 20))
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engine's streams exist
    return t


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


def on_device(torch, xs, misalign):
    """the track's buffers, guarded, on the device -> (tensors, pointers of their payloads, layout, words before the call)"""
    lay = guarded.track_layout(2 * xs[0].shape[1], misalign)
    before = [guarded.make(lay, np.ascontiguousarray(x.T)) for x in xs]
    dev = [torch.from_numpy(w).cuda() for w in before]
    return dev, [d.data_ptr() + 4 * lay.pre for d in dev], lay, before


def report_of(words):
    return (float(np.float32((1 << 21) - int(words[1])) * np.float32(2.0 ** -21)), int(words[2]))


@pytest.mark.parametrize("nb, misalign", [(1, 8), (4, 0)])
@pytest.mark.parametrize("name", ["quiet", "spike_first", "spike_last", "sustained", "two_w", "nonfinite"])
@pytest.mark.parametrize("rate", [44100, 96000, 192000])
def test_device_calls_are_the_host_call(pkg, torch, eng3, rate, name, nb, misalign):
    W = limit_ref.window(rate)
    for n in (T - 1, T, T + 1, T + W, 2 * T + 17):
        xs = limit_ref.make(name, n, nb, W, seed=n, extra=(T - 1, T, T + W - 1))  # every halo path decides a value
        g_ref, ys_ref, rep_ref = pkg.limit_host(xs, rate, CEILING)
        dev, ptrs, lay, before = on_device(torch, xs, misalign)
        glay = guarded.track_layout(n)
        gain = torch.from_numpy(guarded.make(glay)).cuda()
        rep = torch.tensor([SENTINEL, 0, 0, SENTINEL], dtype=torch.int32).cuda()
        eng3.limit_gain_device(ptrs, n, rate, CEILING, gain.data_ptr() + 4 * glay.pre, rep.data_ptr() + 4)
        torch.cuda.synchronize()
        gw, rw = gain.cpu().numpy(), rep.cpu().numpy()
        assert all(guarded.check(d.cpu().numpy(), lay, b).ok for d, b in zip(dev, before))  # the track is only read
        assert guarded.check(gw, glay).ok, str(guarded.check(gw, glay))
        assert same_bits(guarded.payload(gw, glay), g_ref), (n, np.flatnonzero(guarded.payload(gw, glay) != g_ref)[:8])
        assert rw[0] == rw[3] == SENTINEL and report_of(rw) == rep_ref, (n, rw, rep_ref)
        eng3.limit_apply_device(ptrs, n, gain.data_ptr() + 4 * glay.pre)
        torch.cuda.synchronize()
        for d, y in zip(dev, ys_ref):
            want = guarded.make(lay, np.ascontiguousarray(y.T))
            r = guarded.check(d.cpu().numpy(), lay, want)
            assert r.ok, (n, str(r))


@pytest.mark.parametrize("rate", [44100, 192000])
def test_ranges_give_the_whole_call(pkg, torch, eng3, rate):
    W, n = limit_ref.window(rate), 2 * T + 17
    cuts = [0, T - W // 2 - 1, T + W + 3, n]  # two odd frames
    xs = limit_ref.make("sustained", n, 4, W, seed=5, extra=(T - 1, T, T + W - 1, cuts[1], cuts[2] - 1))
    g_ref, _, rep_ref = pkg.limit_host(xs, rate, CEILING)
    dev, ptrs, lay, before = on_device(torch, xs, 0)
    glay = guarded.track_layout(n)
    gain = torch.from_numpy(guarded.make(glay)).cuda()
    rep = torch.zeros(2, dtype=torch.int32).cuda()
    for k in (1, 0, 2):
        first, count = cuts[k], cuts[k + 1] - cuts[k]
        eng3.limit_gain_device(ptrs, n, rate, CEILING, gain.data_ptr() + 4 * (glay.pre + first), rep.data_ptr(), first=first, n=count)
        torch.cuda.synchronize()
        if k == 1:  # nothing outside gain[0 .. n) of the range
            w = gain.cpu().numpy()
            want = guarded.make(glay)
            want[glay.pre + first:glay.pre + first + count] = g_ref[first:first + count].view(np.int32)
            assert guarded.untouched(w, want) is None
    assert same_bits(guarded.payload(gain.cpu().numpy(), glay), g_ref) and guarded.check(gain.cpu().numpy(), glay).ok
    assert report_of(np.concatenate([[0], rep.cpu().numpy()])) == rep_ref


GAINS = [[0, 0, 0, 0, 3.0], [0, 0, 0, 1.0, 0]]  # the mixture three times over, and the vocals


@pytest.fixture(scope="module")
def two_tracks(pkg, eng3):
    """a loud and a quiet track as two lanes, and the call without a limiter: (waves, keywords, plain outputs)"""
    waves = [pkg.ggml.synth_audio(30001, 61), (0.02 * pkg.ggml.synth_audio(12345, 62)).astype(np.float32)]
    kw = dict(gains=GAINS, shift_offsets=[4033, 4033])
    return waves, kw, eng3.separate_many_flac(waves, 0, **kw)[0]


def test_whole_track_call_is_the_plain_call_limited_on_the_host(pkg, eng3, two_tracks):
    waves, kw, plain = two_tracks
    want = [pkg.limit_host(outs, 44100, CEILING) for outs in plain]
    assert want[0][2][1] > 0 and want[1][2] == (1.0, 0)  # the loud track is limited, the quiet one is not
    got, lv, _, _, _, reps = eng3.separate_many_limit(waves, CEILING, **kw)
    plain_lv = eng3.separate_many_flac(waves, 0, **kw)[1]
    for i in range(2):
        assert all(same_bits(a, b) for a, b in zip(got[i], want[i][1])) and reps[i].as_tuple() == want[i][2]
        assert list(lv[i].peak) == list(plain_lv[i].peak) and list(lv[i].over_unity) == list(plain_lv[i].over_unity)  # measured in front
    assert all(same_bits(a, b) for a, b in zip(got[1], plain[1]))
    # int16 and FLAC-16 out: the host encode of the limited floats, nothing clamps
    s16, lv16, _, _, _, reps16 = eng3.separate_many_limit(waves, CEILING, io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16), **kw)
    flac, lvf, _, _, _, repsf = eng3.separate_many_limit(waves, CEILING, flac_bits=16, **kw)
    plain16 = eng3.separate_many_io(waves, out_format=pkg.SAMPLE_S16, **kw)
    for i in range(2):
        for b, y in enumerate(want[i][1]):
            assert np.array_equal(s16[i][b], pkg.pcm16_encode_host(y, buffer=b))
            assert bytes(flac[i][b]) == bytes(pkg.flac_encode_host(y, 44100, 16, buffer=b))
        assert list(lv16[i].clipped) == [0] * 4 == list(lvf[i].clipped)
        assert reps16[i].as_tuple() == repsf[i].as_tuple() == want[i][2]
    assert all(np.array_equal(a, b) for a, b in zip(s16[1], plain16[1]))
    # ... in reset mode too: the segments of the loud track as lanes
    reset = dict(gains=GAINS, shift_offsets=[4033], flags=pkg.FLAG_RESET_SEGMENTS)
    want_r = pkg.limit_host(eng3.separate_many_flac(waves[:1], 0, **reset)[0][0], 44100, CEILING)
    got_r = eng3.separate_many_limit(waves[:1], CEILING, **reset)
    assert all(same_bits(a, b) for a, b in zip(got_r[0][0], want_r[1])) and got_r[5][0].as_tuple() == want_r[2]


def test_no_limiter_is_the_flac_call_and_rescale_is_refused(pkg, eng3, two_tracks):
    waves, kw, plain = two_tracks
    got = eng3.separate_many_limit(waves, None, **kw)
    assert got[5] is None and all(same_bits(a, b) for g, p in zip(got[0], plain) for a, b in zip(g, p))
    for ceiling, clip, reason in [(CEILING, pkg.CLIP_RESCALE, "limiter: not with UMX_CLIP_RESCALE"), (0.0, pkg.CLIP_CLAMP, "ceiling"),
                                  (1.5, pkg.CLIP_CLAMP, "ceiling"), (float("nan"), pkg.CLIP_CLAMP, "ceiling"), (CEILING, 2, "clip mode")]:
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_many_limit(waves, ceiling, clip=clip, **kw)
        assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
    again = eng3.separate_many_flac(waves, 0, **kw)[0]  # the context goes on, with its usual bits
    assert all(same_bits(a, b) for g, p in zip(again, plain) for a, b in zip(g, p))


def test_cli_limit_is_the_python_path(pkg, model_small, tmp_path):
    wav, cli = Path(__file__).resolve().parent / "golden" / "gspi_stereo.wav", Path(pkg.HERE) / "umx-cli"
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_MIX": "loud=3*mix;vocals=vocals"}

    def run(out, tool=cli, **extra):
        return subprocess.run([str(tool), model_small[0]] + ([str(out), str(wav)] if tool != cli else [str(wav), str(out)]), capture_output=True,
                              text=True, env={**env, **extra}, timeout=600)
    r = run(tmp_path / "lim", UMX_LIMIT="-1")
    assert r.returncode == 0, r.stderr
    hm = pkg.HostModel(model_small[0])
    eng = pkg.engine_from_host_model(hm, pkg.SEGMENT_SAMPLES)  # the context umx-cli makes
    try:
        outs, _, _, _, _, reps = eng.separate_many_limit([pkg.wav_load(wav)[0]], CEILING, gains=GAINS, shift_offsets=[4033])
    finally:
        eng.close()
    min_gain, limited = reps[0].as_tuple()
    assert limited > 0
    for name, y in zip(("loud", "vocals"), outs[0]):
        assert same_bits(pkg.wav_load(tmp_path / "lim" / f"{name}.wav")[0], y)
        assert f"limit {tmp_path / 'lim' / name}.wav min_gain_db={20 * np.log10(np.float64(min_gain)):.6f} limited_frames={limited}\n" in r.stdout
    for extra, word in [({"UMX_CLIP": "rescale"}, "UMX_CLIP=rescale"), ({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"),
                        ({"UMX_CLI_PER_SEGMENT": "1", "UMX_MIX": ""}, "UMX_CLI_PER_SEGMENT"), ({"UMX_LIMIT": "3"}, "<= 0")]:
        r = run(tmp_path / "no", **{"UMX_LIMIT": "-1", **extra})
        assert r.returncode == 1 and "UMX_LIMIT" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
    r = run(tmp_path / "b", tool=Path(pkg.HERE) / "umx-batch", UMX_LIMIT="-1")
    assert r.returncode == 1 and "UMX_LIMIT" in r.stderr and "queue" in r.stderr and not (tmp_path / "b").exists(), r.stderr
