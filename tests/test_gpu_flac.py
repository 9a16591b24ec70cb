"""FLAC out of the whole-track driver (csrc/flac.h), without tolerances: the three kernels on guarded device buffers
against the host restatement byte for byte, and the whole-track call decoded by the independent decoder of tests/flac_ref.py against
the codes and levels that separate_many_levels returns for the PCM format of the same width."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flac_ref
from flac_ref import RATE, SIZES, signal

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: stride 12288
LENGTH = 30001  # three segments
SEED = 7
GUARD = 4096
# the signals of tests/test_flac_cpu.py, every one at both widths here (noise24: full-range noise, the 25-bit side channel and the
# VERBATIM-against-RICE2 decision; noise24_quiet: RICE2 itself)
SIGNALS = ["silence", "equal", "opposite", "sine", "noise", "alternating", "noise24", "noise24_quiet", "nonfinite"]
TWO_ROWS = np.array([[0, 0, 0, 1, 0], [0, 0, 0, 0, 3]], np.float32)  # vocals; three times the mixture, which passes full scale
IDENTITY = np.eye(4, 5, dtype=np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engines' streams exist
    return t


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.mark.parametrize("seed", [None, SEED], ids=["plain", "dithered"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("bits", [16, 24])
def test_device_streams_are_the_host_streams(pkg, torch, eng3, bits, nb, n, seed):
    """every signal of the CPU matrix at this size, with and without dither: one launch per signal (nb 1), or four signals per launch
    (nb 4: three launches cover the nine, the last wrapping round)"""
    cap = pkg.flac_bound(n, bits) + 64
    for g in range(0, len(SIGNALS), nb):
        names = [SIGNALS[(g + b) % len(SIGNALS)] for b in range(nb)]
        xs = [signal(s, n) for s in names]
        ins = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in xs]
        # guarded outputs at byte addresses of every residue mod 16: guard | capacity (0x5A) | guard
        outs = [torch.full((2 * GUARD + cap,), 0xA5, dtype=torch.uint8).cuda() for _ in range(nb)]
        starts = [GUARD - 16 + (5 * b + n + g) % 16 for b in range(nb)]
        for o, s in zip(outs, starts):
            o[s:s + cap] = 0x5A
        got_bytes = torch.zeros(nb, dtype=torch.int64).cuda()
        first = 4 - nb  # (buffer b is output first + b of the dither rule)
        eng3.flac_encode_device([i.data_ptr() for i in ins], n, RATE, bits, [o.data_ptr() + s for o, s in zip(outs, starts)], [cap] * nb,
                                got_bytes.data_ptr(), first_buffer=first, dither_seed=seed)
        torch.cuda.synchronize()
        for b in range(nb):
            want = pkg.flac_encode_host(xs[b], RATE, bits, buffer=first + b, dither_seed=seed)
            o, k = outs[b].cpu().numpy(), int(got_bytes[b])
            what = (bits, nb, n, names[b], seed)
            assert k == want.size, (what, k, want.size)
            assert np.array_equal(o[starts[b]:starts[b] + k], want), what
            assert np.all(o[:starts[b]] == 0xA5) and np.all(o[starts[b] + cap:] == 0xA5) and np.all(o[starts[b] + k:starts[b] + cap] == 0x5A), what


@pytest.mark.parametrize("clip", ["clamp", "rescale"])
@pytest.mark.parametrize("gains", [IDENTITY, TWO_ROWS], ids=["identity", "two_rows"])
@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("reset", [False, True], ids=["carry", "reset"])
def test_whole_track_streams_decode_to_the_pcm_call(pkg, eng3, reset, rate, gains, clip):
    x = pkg.ggml.synth_audio(LENGTH, 71)
    kw = dict(flags=pkg.FLAG_RESET_SEGMENTS if reset else 0, shift_offsets=[4033], rates=[rate], gains=gains)
    mode = pkg.CLIP_RESCALE if clip == "rescale" else pkg.CLIP_CLAMP
    for bits, fmt, seed in ((16, pkg.SAMPLE_S16, SEED), (24, pkg.SAMPLE_S24, None)):
        want, lvw = eng3.separate_many_levels([x], mode, pkg.sample_io(pkg.SAMPLE_F32, fmt, seed), **kw)
        streams, lv = eng3.separate_many_flac([x], bits, clip=mode, io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_F32, seed), **kw)[:2]
        assert len(streams[0]) == gains.shape[0]
        for m, s in enumerate(streams[0]):
            info, codes = flac_ref.decode(s)
            assert (info["rate"], info["bits"], info["total"]) == (rate, bits, LENGTH)
            assert np.array_equal(codes, want[0][m].astype(np.int32)), (bits, m)
            assert s.size <= pkg.flac_bound(LENGTH, bits)
        assert bytes(lv[0]) == bytes(lvw[0]), (bits, lv[0].as_dict(), lvw[0].as_dict())
        if clip == "clamp" and gains is TWO_ROWS:
            assert lv[0].clipped[1] > 0  # counted as for the PCM format of that width


def test_flac_bits_zero_is_the_true_peak_call_and_the_refusals(pkg, eng3):
    x = pkg.ggml.synth_audio(LENGTH, 73)
    kw = dict(shift_offsets=[4033], gains=TWO_ROWS, records=True, true_peak=pkg.TRUE_PEAK_MEASURE)
    want = eng3.separate_many_true_peak([x], **kw)
    got = eng3.separate_many_flac([x], 0, **kw)
    assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got[0][0], want[0][0]))
    assert bytes(got[1][0]) == bytes(want[1][0]) and bytes(got[4][0]) == bytes(want[4][0])
    for what, call in (("capacity", lambda: eng3.separate_many_flac([x], 16, caps=pkg.flac_bound(LENGTH, 16) - 1)),
                       ("out_format", lambda: eng3.separate_many_flac([x], 16, io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16))),
                       ("flac_bits", lambda: eng3.separate_many_flac([x], 12)),
                       ("queue", lambda: eng3.separate_queue([x], flac_bits=16))):  # (refused by the Python wrapper: the C queue has no such argument)
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and ("flac" in str(e.value).lower()), (what, str(e.value))
    again = eng3.separate_many_true_peak([x], **kw)  # the context works afterwards
    assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(again[0][0], want[0][0]))
    streams = eng3.separate_many_flac([x], 24)[0]
    assert all(flac_ref.decode(s)[0]["total"] == LENGTH for s in streams[0])


def test_cli_flac_decodes_to_the_pcm16_wav(pkg, model_small, tmp_path):
    q = np.ascontiguousarray(pkg.wav_load_pcm16(Path(__file__).resolve().parent / "golden" / "gspi_stereo.wav")[0][:, 20000:50000])
    pkg.wav_write_pcm16(tmp_path / "in.wav", q)
    runs = {}
    for name, env in (("wav", {"UMX_PCM16": "1"}), ("flac", {"UMX_FLAC": "16"}), ("both", {"UMX_FLAC": "16", "UMX_PCM16": "1"})):
        runs[name] = subprocess.run([str(Path(pkg.HERE) / "umx-cli"), model_small[0], str(tmp_path / "in.wav"), str(tmp_path / name)],
                                    capture_output=True, text=True, env={**os.environ, "UMX_SHIFT_OFFSET": "4033", **env}, timeout=600)
    assert runs["wav"].returncode == 0 and runs["flac"].returncode == 0, (runs["wav"].stderr, runs["flac"].stderr)
    assert runs["both"].returncode == 1 and "UMX_FLAC" in runs["both"].stderr and not (tmp_path / "both").exists()
    assert sorted(f.name for f in (tmp_path / "flac").iterdir()) == [f"target_{t}.flac" for t in range(4)]
    for t in range(4):
        info, codes = flac_ref.decode((tmp_path / "flac" / f"target_{t}.flac").read_bytes())
        assert np.array_equal(codes, pkg.wav_load_pcm16(tmp_path / "wav" / f"target_{t}.wav")[0].astype(np.int32)) and info["rate"] == 44100
    r = subprocess.run([str(Path(pkg.HERE) / "umx-batch"), model_small[0], str(tmp_path / "b"), str(tmp_path / "in.wav")], capture_output=True,
                       text=True, env={**os.environ, "UMX_FLAC": "16"}, timeout=600)
    assert r.returncode == 1 and "UMX_FLAC" in r.stderr and not (tmp_path / "b").exists()
