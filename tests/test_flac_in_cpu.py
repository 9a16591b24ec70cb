"""FLAC in (csrc/flac_decode.h), host side, without tolerances: the host decoder returns, bit for bit, the floats the int16 /
packed 24-bit decode gives for the codes a stream holds -- over this project's own streams and over the foreign ones of
tests/golden/flac_foreign.npz -- the probe returns what was encoded, and every refusal gives its reason."""
from pathlib import Path

import numpy as np
import pytest

import flac_ref
from flac_lpc_ref import signal
from flac_ref import RATE

SIZES = [1, 15, 4096, 4097, 2 * 4096 + 17]
SIGNALS = ["two_tones", "resonance", "noise24_quiet", "nonfinite", "silence", "noise24"]  # (silence: CONSTANT; full-range noise: VERBATIM)
FOREIGN = ["rice_escape", "rice2_escape_wasted_side", "lpc32_metadata_id3", "tiny_2050_frames"]


@pytest.fixture(scope="module")
def foreign():
    return np.load(Path(__file__).parent / "golden" / "flac_foreign.npz")


def pcm_floats(pkg, codes, bits):
    return pkg.pcm16_decode_host(codes.astype(np.int16)) if bits == 16 else pkg.pcm24_decode_host(codes.astype(np.int32))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("seed", [None, 7], ids=["plain", "dithered"])
@pytest.mark.parametrize("lpc", [0, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", SIGNALS)
@pytest.mark.parametrize("n", SIZES)
def test_own_streams_decode_to_the_pcm_floats(pkg, n, name, bits, lpc, seed):
    x = signal(name, n)
    stream = pkg.flac_encode_host(x, RATE, bits, dither_seed=seed, lpc=lpc)
    info = pkg.flac_probe(stream)
    assert (info.n_frames, info.rate, info.bits, info.channels, info.max_block, info.audio_offset) == (n, RATE, bits, 2, 4096, 42)
    codes = (pkg.pcm16_encode_host if bits == 16 else pkg.pcm24_encode_host)(x, dither_seed=seed)
    assert same_bits(pkg.flac_decode_host(stream), pcm_floats(pkg, codes, bits))


@pytest.mark.parametrize("name", FOREIGN)
def test_foreign_streams_decode_to_their_samples(pkg, foreign, name):
    data, samples = foreign[name + "_bytes"], foreign[name + "_samples"]
    info = pkg.flac_probe(data)
    assert info.n_frames == samples.shape[1] and info.channels == 2
    assert same_bits(pkg.flac_decode_host(data), pcm_floats(pkg, samples, info.bits))


def _streaminfo(stream, **put):
    """the 64 bits behind the frame sizes: rate 20, channels - 1 3, bits - 1 5, total 36"""
    s = stream.copy()
    v = int.from_bytes(bytes(s[18:26]), "big")
    for (shift, width), value in [((44, 20), put.get("rate")), ((41, 3), put.get("channels")), ((36, 5), put.get("bits")), ((0, 36), put.get("total"))]:
        if value is not None:
            v = (v & ~(((1 << width) - 1) << shift)) | (value << shift)
    s[18:26] = np.frombuffer(v.to_bytes(8, "big"), np.uint8)
    return s


@pytest.mark.parametrize("case,reason", [("marker", "no fLaC marker"), ("variable", "variable-blocksize"), ("mono", "2-channel"),
                                         ("bits8", "16 and 24 bits"), ("total0", "total sample count is unknown"), ("length", "n_frames equal to"),
                                         ("flipped", "frame 1:"), ("cut", "frame 2:")])
def test_the_refusals_give_their_reason(pkg, case, reason):
    good = pkg.flac_encode_host(signal("two_tones", 2 * 4096 + 17), RATE, 16)
    sizes = [size for _, size in flac_ref.decode(good)[0]["stats"]["frames"]]  # three frames
    n_frames = None
    if case == "marker":
        bad = good.copy()
        bad[0] = ord("F")
    elif case == "variable":
        bad = good.copy()
        bad[43] = 0xF9
    elif case == "flipped":  # a byte inside frame 1
        bad = good.copy()
        bad[42 + sizes[0] + sizes[1] // 2] ^= 0x10
    elif case == "cut":
        bad = good[:-(sizes[2] // 2)]
    else:
        bad = _streaminfo(good, **{"mono": dict(channels=0), "bits8": dict(bits=7), "total0": dict(total=0), "length": {}}[case])
        n_frames = 5 if case == "length" else None
    with pytest.raises(pkg.UmxError) as e:
        pkg.flac_decode_host(bad, n_frames)
    assert e.value.code == pkg.ERR_ARG and reason in str(e.value), str(e.value)
