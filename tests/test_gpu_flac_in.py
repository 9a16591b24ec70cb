"""FLAC in (csrc/flac_decode.h) on the device, without tolerances: umx_hip_flac_decode_device against the host decoder bit for
bit on guarded buffers, a false candidate that the scan alone would trust, damaged streams, and the whole-track call with SAMPLE_FLAC in
against the same call with SAMPLE_S16 / SAMPLE_S24 in on the same codes."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flac_ref
import guarded
from flac_lpc_ref import signal
from flac_ref import RATE
from test_flac_in_cpu import FOREIGN, SIGNALS, SIZES, same_bits

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: the small context of tests/test_gpu_pcm24.py
PAD = 64       # guard bytes around a stream


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


@pytest.fixture(scope="module")
def foreign():
    return np.load(Path(__file__).parent / "golden" / "flac_foreign.npz")


def decode_on_device(pkg, torch, eng, stream, offset=1):
    """the stream at an odd byte of a guarded byte buffer -> (status, the guarded output's words, its layout)"""
    info = pkg.flac_probe(stream)
    held = np.full(PAD + offset + stream.size + PAD, 0xA5, np.uint8)
    held[PAD + offset:PAD + offset + stream.size] = stream
    dev = torch.from_numpy(held).cuda()
    lay = guarded.track_layout(2 * info.n_frames, misalign=8 * (offset & 1))
    out = torch.from_numpy(guarded.make(lay)).cuda()
    status = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32).cuda()
    eng.flac_decode_device(dev.data_ptr() + PAD + offset, stream.size, info, out.data_ptr() + 4 * lay.pre, status.data_ptr() + 4)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), held)
    st = status.cpu().numpy()
    assert st[0] == st[2] == 0x5A5A5A5A
    return int(st[1]), out.cpu().numpy(), lay


def assert_device_is_host(pkg, torch, eng, stream, offset=1):
    status, words, lay = decode_on_device(pkg, torch, eng, stream, offset)
    assert status == 0
    assert guarded.check(words, lay).ok, str(guarded.check(words, lay))
    want = np.ascontiguousarray(pkg.flac_decode_host(stream).T).ravel()
    assert same_bits(guarded.payload(words, lay), want)


@pytest.mark.parametrize("lpc", [0, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", SIZES)
def test_device_decode_is_the_host_decode(pkg, torch, eng3, n, bits, lpc):
    for k, name in enumerate(SIGNALS):
        assert_device_is_host(pkg, torch, eng3, pkg.flac_encode_host(signal(name, n), RATE, bits, dither_seed=7 if k & 1 else None, lpc=lpc),
                              offset=1 + 2 * (k & 3))


@pytest.mark.parametrize("name", FOREIGN)  # (tiny_2050_frames: 33 waves of candidates)
def test_foreign_streams_on_the_device(pkg, torch, eng3, foreign, name):
    assert_device_is_host(pkg, torch, eng3, foreign[name + "_bytes"], offset=3)


def test_a_planted_frame_header_is_no_frame(pkg, torch, eng3):
    """frame 1's whole header, byte for byte, inside frame 0's VERBATIM samples: a candidate with a valid CRC-8 and a fitting number"""
    stream = pkg.flac_encode_host(signal("noise24", 2 * 4096), RATE, 24)
    info, _ = flac_ref.decode(stream)
    assert info["stats"]["verbatim"] == 4
    size0 = info["stats"]["frames"][0][1]
    header = stream[42 + size0:42 + size0 + 6].copy()  # sync, codes, number 1, CRC-8
    assert flac_ref.crc8(bytes(header[:5])) == header[5]
    stream[42 + 7 + 3 * 500:42 + 7 + 3 * 500 + 6] = header  # (6 header bytes and the subframe's byte, then 3 bytes a sample)
    stream[42 + size0 - 2:42 + size0] = np.frombuffer(flac_ref.crc16(bytes(stream[42:42 + size0 - 2])).to_bytes(2, "big"), np.uint8)
    assert_device_is_host(pkg, torch, eng3, stream)


@pytest.mark.parametrize("damage", ["flipped", "cut"])
def test_damaged_streams_name_their_frame(pkg, torch, eng3, damage):
    x = signal("two_tones", 3 * 4096 + 17)
    good = pkg.flac_encode_host(x, RATE, 16)
    sizes = [s for _, s in flac_ref.decode(good)[0]["stats"]["frames"]]
    if damage == "flipped":
        frame, bad = 2, good.copy()
        bad[42 + sizes[0] + sizes[1] + sizes[2] // 2] ^= 0x04
    else:
        frame, bad = 3, good[:-(sizes[3] // 2)]
    with pytest.raises(pkg.UmxError) as e:
        pkg.flac_decode_host(bad)
    assert f"frame {frame}:" in str(e.value)
    status, words, lay = decode_on_device(pkg, torch, eng3, bad)
    assert status == 1 + frame
    assert guarded.untouched(words, guarded.make(lay)) is None  # nothing but the status word
    io = pkg.sample_io(pkg.SAMPLE_FLAC)
    with pytest.raises(pkg.UmxError) as e:
        eng3.separate_many_io([bad], io=io)
    assert e.value.code == pkg.ERR_ARG and f"track 0: frame {frame} " in str(e.value), str(e.value)
    got = eng3.separate_many_io([good], io=io)  # the context goes on
    want = eng3.separate_many_io([pkg.pcm16_encode_host(x)], in_format=pkg.SAMPLE_S16)
    assert all(same_bits(a, b) for a, b in zip(got[0], want[0]))


@pytest.mark.parametrize("rate", [RATE, 48000])
@pytest.mark.parametrize("reset", [False, True], ids=["carry", "reset"])
def test_whole_track_flac_in_is_the_pcm_in_call(pkg, eng3, reset, rate):
    lengths = [30001] if reset else [30001, 12345]  # (reset mode takes one track)
    xs = [pkg.ggml.synth_audio(L, 81 + i) for i, L in enumerate(lengths)]
    kw = dict(flags=pkg.FLAG_RESET_SEGMENTS if reset else 0, shift_offsets=[4033] * len(xs), rates=[rate] * len(xs))
    for bits, fmt, encode in [(16, pkg.SAMPLE_S16, pkg.pcm16_encode_host), (24, pkg.SAMPLE_S24, pkg.pcm24_encode_host)]:
        streams = [pkg.flac_encode_host(x, rate, bits, lpc=4) for x in xs]
        codes = [encode(x) for x in xs]
        for out_format in (pkg.SAMPLE_F32, pkg.SAMPLE_S16):
            got = eng3.separate_many_io(streams, in_format=pkg.SAMPLE_FLAC, out_format=out_format, dither_seed=None, **kw)
            want = eng3.separate_many_io(codes, in_format=fmt, out_format=out_format, dither_seed=None, **kw)
            for g, w in zip(got, want):
                assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g, w)), (bits, out_format)


def test_flac_in_and_flac_out(pkg, eng3):
    x = pkg.ggml.synth_audio(30001, 91)
    got = eng3.separate_many_flac([pkg.flac_encode_host(x, RATE, 16)], 16, io=pkg.sample_io(pkg.SAMPLE_FLAC, pkg.SAMPLE_F32, 7))
    want = eng3.separate_many_flac([pkg.pcm16_encode_host(x)], 16, io=pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_F32, 7))
    assert all(np.array_equal(a, b) for a, b in zip(got[0][0], want[0][0])) and bytes(got[1][0]) == bytes(want[1][0])


def test_the_refusals(pkg, eng3):
    x = pkg.ggml.synth_audio(30001, 93)
    stream = pkg.flac_encode_host(x, RATE, 16)
    for call, reason in [(lambda: eng3.separate_queue([stream], io=pkg.sample_io(pkg.SAMPLE_FLAC)), "queue"),
                         (lambda: eng3.separate_many_io([x], io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_FLAC)), "input format"),
                         (lambda: eng3.separate_many_io([stream], io=pkg.sample_io(pkg.SAMPLE_FLAC), rates=[48000]), "rate disagrees")]:
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
    # ... and the library's own queue refusal, behind the Python one: it comes before the first `next` call
    io = pkg.sample_io(pkg.SAMPLE_FLAC)
    rc = eng3.lib.umx_hip_separate_queue_io(eng3.h, pkg.QUEUE_NEXT_FN(lambda user, job: 0), pkg.QUEUE_DONE_FN(lambda user, job: None), None, 4, None, 0, io)
    assert rc == pkg.ERR_ARG and "queue" in eng3.last_error() and "UMX_SAMPLE_FLAC" in eng3.last_error()


def test_cli_on_a_flac_file_writes_what_it_writes_for_the_wav(pkg, model_small, tmp_path):
    q = np.ascontiguousarray(pkg.wav_load_pcm16(Path(__file__).resolve().parent / "golden" / "gspi_stereo.wav")[0][:, 20000:50000])
    pkg.wav_write_pcm16(tmp_path / "in.wav", q)
    stream = pkg.flac_encode_host(pkg.pcm16_decode_host(q), RATE, 16)  # (decode and encode are inverse on the codes)
    assert np.array_equal(flac_ref.decode(stream)[1], q.astype(np.int32))
    (tmp_path / "in.flac").write_bytes(b"ID3\x04\x00\x00\x00\x00\x00\x05tag!!" + stream.tobytes())  # recognised by content, behind a tag
    env = {**os.environ, "UMX_SHIFT_OFFSET": "4033", "UMX_PCM16": "1"}
    for name in ("wav", "flac"):
        r = subprocess.run([str(Path(pkg.HERE) / "umx-cli"), model_small[0], str(tmp_path / f"in.{name}"), str(tmp_path / name)], capture_output=True,
                           text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
    for t in range(4):
        assert (tmp_path / "flac" / f"target_{t}.wav").read_bytes() == (tmp_path / "wav" / f"target_{t}.wav").read_bytes()
    r = subprocess.run([str(Path(pkg.HERE) / "umx-batch"), model_small[0], str(tmp_path / "b"), str(tmp_path / "in.flac")], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 1 and "queue" in r.stderr and not (tmp_path / "b").exists()
