"""The limiter's true-peak detector on the device (csrc/limiter.h), without tolerances: its kernels against the host twin on
guarded buffers, ranges, the whole-track call against the plain call limited by the host twin, umx-cli against the Python path."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded
import limit_ref
import limit_tp_ref
from limit_ref import T, same_bits
from test_gpu_limit import CEILING, GAINS, SENTINEL, eng3, on_device, report_of, torch  # noqa: F401 (eng3, torch: its fixtures)

pytestmark = pytest.mark.gpu


def track(n, nb, W, seed):
    """noise with inter-sample peaks at the edges of the gain kernel's tile and halo, of the track and of the detector's tiles; a spike at T"""
    xs = limit_tp_ref.bursts(limit_ref.make("quiet", n, nb, W, seed=seed), [T - 1, T + W - 2, 0, n - 2, 1022, 2045])
    if T < n:
        xs[nb - 1][1, T] = np.float32(-4.0)
    return xs


@pytest.mark.parametrize("nb, misalign", [(1, 8), (4, 0)])
@pytest.mark.parametrize("rate", [44100, 96000])
def test_device_calls_are_the_host_twin(pkg, torch, eng3, rate, nb, misalign):
    W = limit_ref.window(rate)
    for n in (T - 1, T, T + 1, T + W, 2 * T + 17):
        xs = track(n, nb, W, n)
        g_ref, ys_ref, rep_ref = pkg.limit_host(xs, rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
        assert rep_ref[1] > pkg.limit_host(xs, rate, CEILING)[2][1]  # the bursts are seen between the samples only
        dev, ptrs, lay, before = on_device(torch, xs, misalign)
        glay = guarded.track_layout(n)
        gain = torch.from_numpy(guarded.make(glay)).cuda()
        rep = torch.tensor([SENTINEL, 0, 0, SENTINEL], dtype=torch.int32).cuda()
        eng3.limit_gain_device(ptrs, n, rate, CEILING, gain.data_ptr() + 4 * glay.pre, rep.data_ptr() + 4, detector=pkg.LIMIT_TRUE_PEAK)
        torch.cuda.synchronize()
        gw, rw = gain.cpu().numpy(), rep.cpu().numpy()
        assert all(guarded.check(d.cpu().numpy(), lay, b).ok for d, b in zip(dev, before))  # the track is only read
        assert guarded.check(gw, glay).ok, str(guarded.check(gw, glay))
        assert same_bits(guarded.payload(gw, glay), g_ref), (n, np.flatnonzero(guarded.payload(gw, glay) != g_ref)[:8])
        assert rw[0] == rw[3] == SENTINEL and report_of(rw) == rep_ref, (n, rw, rep_ref)
        eng3.limit_apply_device(ptrs, n, gain.data_ptr() + 4 * glay.pre)
        torch.cuda.synchronize()
        for d, y in zip(dev, ys_ref):
            r = guarded.check(d.cpu().numpy(), lay, guarded.make(lay, np.ascontiguousarray(y.T)))
            assert r.ok, (n, str(r))


def test_ranges_give_the_whole_call(pkg, torch, eng3):
    rate, W, n = 44100, 256, 2 * T + 17
    cuts = [0, T - W // 2 - 1, T + W + 3, n]  # two odd frames
    xs = limit_tp_ref.bursts(track(n, 4, W, 5), [cuts[1] - 1, cuts[2] - 1])  # a peak between a range's last frame and the next one's first
    g_ref, _, rep_ref = pkg.limit_host(xs, rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
    dev, ptrs, lay, before = on_device(torch, xs, 0)
    glay = guarded.track_layout(n)
    gain = torch.from_numpy(guarded.make(glay)).cuda()
    rep = torch.zeros(2, dtype=torch.int32).cuda()
    for k in (1, 0, 2):
        first, count = cuts[k], cuts[k + 1] - cuts[k]
        eng3.limit_gain_device(ptrs, n, rate, CEILING, gain.data_ptr() + 4 * (glay.pre + first), rep.data_ptr(), first=first, n=count,
                               detector=pkg.LIMIT_TRUE_PEAK)
        torch.cuda.synchronize()
    assert same_bits(guarded.payload(gain.cpu().numpy(), glay), g_ref) and guarded.check(gain.cpu().numpy(), glay).ok
    assert report_of(np.concatenate([[0], rep.cpu().numpy()])) == rep_ref


def test_whole_track_call_is_the_plain_call_limited_by_the_host_twin(pkg, eng3):
    waves = [pkg.ggml.synth_audio(30001, 61), (0.02 * pkg.ggml.synth_audio(12345, 62)).astype(np.float32)]
    kw = dict(gains=GAINS, shift_offsets=[4033, 4033])
    plain = eng3.separate_many_flac(waves, 0, **kw)[0]
    want = [pkg.limit_host(outs, 44100, CEILING, detector=pkg.LIMIT_TRUE_PEAK) for outs in plain]
    assert want[0][2][1] > 0 and want[1][2] == (1.0, 0)  # the loud track is limited, the quiet one is not
    got, _, _, _, _, reps = eng3.separate_many_limit(waves, CEILING, detector=pkg.LIMIT_TRUE_PEAK, **kw)
    s16, _, _, _, _, reps16 = eng3.separate_many_limit(waves, CEILING, detector=pkg.LIMIT_TRUE_PEAK, io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16), **kw)
    for i in range(2):
        after = max(pkg.true_peak_float(pkg.true_peak_host(y, 44100)) for y in want[i][1])
        assert all(same_bits(a, b) for a, b in zip(got[i], want[i][1]))
        assert reps[i].as_tuple() == reps16[i].as_tuple() == want[i][2] and reps[i].true_peak_after == reps16[i].true_peak_after == after
        assert all(np.array_equal(s16[i][b], pkg.pcm16_encode_host(y, buffer=b)) for b, y in enumerate(want[i][1]))
    assert all(same_bits(a, b) for a, b in zip(got[1], plain[1]))  # the quiet lane leaves bit for bit
    assert eng3.separate_many_limit(waves, CEILING, **kw)[5][0].true_peak_after == 0  # the sample detector does not fill it
    for rates, detector, reason in [([7000, 44100], pkg.LIMIT_TRUE_PEAK, "sample rate"), (None, 2, "unknown detector")]:
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_many_limit(waves, CEILING, detector=detector, rates=rates, **kw)
        assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
    again = eng3.separate_many_flac(waves, 0, **kw)[0]  # the context goes on, with its usual bits
    assert all(same_bits(a, b) for g, p in zip(again, plain) for a, b in zip(g, p))


def test_cli_detector_is_the_python_path(pkg, model_small, tmp_path):
    wav, cli = Path(__file__).resolve().parent / "golden" / "gspi_stereo.wav", Path(pkg.HERE) / "umx-cli"
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_MIX": "loud=3*mix;vocals=vocals", "UMX_LIMIT": "-1"}

    def run(out, **extra):
        return subprocess.run([str(cli), model_small[0], str(wav), str(out)], capture_output=True, text=True, env={**env, **extra}, timeout=600)
    r = run(tmp_path / "tp", UMX_LIMIT_DETECTOR="true_peak")
    assert r.returncode == 0, r.stderr
    eng = pkg.engine_from_host_model(pkg.HostModel(model_small[0]), pkg.SEGMENT_SAMPLES)  # the context umx-cli makes
    try:
        outs, _, _, _, _, reps = eng.separate_many_limit([pkg.wav_load(wav)[0]], CEILING, gains=GAINS, shift_offsets=[4033],
                                                         detector=pkg.LIMIT_TRUE_PEAK)
    finally:
        eng.close()
    (min_gain, limited), after = reps[0].as_tuple(), reps[0].true_peak_after
    assert limited > 0
    for name, y in zip(("loud", "vocals"), outs[0]):
        assert same_bits(pkg.wav_load(tmp_path / "tp" / f"{name}.wav")[0], y)
        assert (f"limit {tmp_path / 'tp' / name}.wav min_gain_db={20 * np.log10(np.float64(min_gain)):.6f} limited_frames={limited} "
                f"true_peak_after_db={20 * np.log10(np.float64(after)):.6f}\n") in r.stdout
    for extra, word in [({"UMX_LIMIT_DETECTOR": "peak"}, "sample or true_peak"), ({"UMX_LIMIT_DETECTOR": "true_peak", "UMX_LIMIT": ""}, "needs UMX_LIMIT")]:
        r = run(tmp_path / "no", **extra)
        assert r.returncode == 1 and "UMX_LIMIT_DETECTOR" in r.stderr and word in r.stderr and not (tmp_path / "no").exists(), r.stderr
