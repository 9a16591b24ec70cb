"""Packed 24-bit PCM in and out, the host side: the library's restatement of the decode / encode rules
(umx_hip_pcm24_decode_host / _encode_host, csrc/pcm24.h -- the functions the kernels call) against tests/pcm24_ref.py bit for bit,
the round trip of all 2^24 codes through the library, the S24 clip count of umx_hip_levels_host, and the 24-bit PCM WAV functions of
the host library.  No GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

import pcm24_ref as ref

F32 = np.float32


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    raw = {np.dtype(np.float32): np.uint32, np.dtype(np.int32): np.uint32, np.dtype(np.uint8): np.uint8}[a.dtype]
    bad = np.flatnonzero(a.view(raw).ravel() != b.view(raw).ravel())
    assert bad.size == 0, (bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


@pytest.fixture(scope="module")
def all_codes():
    c = np.arange(ref.QMIN, ref.QMAX + 1, dtype=np.int32)
    return np.stack([c, c[::-1]])  # (2, 2^24)


def test_the_format_constant_and_the_packing(pkg):
    assert (pkg.SAMPLE_F32, pkg.SAMPLE_S16, pkg.SAMPLE_S24) == (0, 1, 3)
    q = np.array([[0, 1, -1, ref.QMAX, ref.QMIN, 0x123456], [-0x123456, 256, -256, 65536, -65536, 2]], np.int32)
    b = pkg.pcm24_pack(q)
    assert b.dtype == np.uint8 and b.size == 36
    _same(b, ref.pack(q))
    assert b[:6].tolist() == [0, 0, 0, 0xAA, 0xCB, 0xED] and b[30:36].tolist() == [0x56, 0x34, 0x12, 2, 0, 0]  # L then R, little-endian
    _same(pkg.pcm24_unpack(b), q)
    _same(ref.unpack(b), q)
    with pytest.raises(ValueError):
        pkg.pcm24_pack(np.array([[ref.QMAX + 1], [0]]))
    with pytest.raises(ValueError):
        pkg.pcm24_unpack(np.zeros(7, np.uint8))


def test_all_codes_round_trip_through_the_library(pkg, all_codes):
    x = pkg.pcm24_decode_host(all_codes)
    _same(x, ref.decode(all_codes))
    assert np.array_equal(x.astype(np.float64) * 8388608.0, all_codes.astype(np.float64))  # exact: the loader's q / 8388608.f
    _same(pkg.pcm24_encode_host(x), all_codes)
    q = pkg.pcm24_encode_host(x, buffer=2, first_frame=5, dither_seed=7)
    assert np.abs(q.astype(np.int64) - all_codes).max() <= 1
    n = 1 << 16  # (the reference's dither over a part of them, at both ends of the scale and in the middle)
    for lo in (0, (1 << 23) - n // 2, (1 << 24) - n):
        _same(q[:, lo:lo + n], ref.encode(x[:, lo:lo + n], 2, 5 + lo, 7))


def test_the_sum_is_formed_in_double(pkg):
    """At |v| >= 2^22 an fp32 v + d falls on a 0.5 grid before the rounding; the rule rounds the exact sum once."""
    k = np.arange(4096, dtype=np.int64)
    q0 = (1 << 22) + 2 * k + 1  # odd codes above 2^22
    x = ref.decode(np.stack([q0, -q0]).astype(np.int32))
    got = pkg.pcm24_encode_host(x, 1, 100, 3)
    _same(got, ref.encode(x, 1, 100, 3))
    dd = np.stack([ref.d(3, 1, ch, 100 + k) for ch in range(2)])
    fp32_form = np.rint((x * ref.SCALE + dd).astype(F32)).astype(np.int32)
    assert np.count_nonzero(fp32_form != got) > 100  # the two forms do differ here, so the test above tells them apart


def test_ties_go_to_even_and_the_awkward_values(pkg):
    for k, even in ((0, 0), (1, 2), (2, 2), (100, 100), (8388606, 8388606)):
        x = np.array([[(k + 0.5) / 8388608.0], [-(k + 0.5) / 8388608.0]], F32)
        assert pkg.pcm24_encode_host(x).ravel().tolist() == [even, -even]
    x = ref.awkward_floats()
    _same(pkg.pcm24_encode_host(x), ref.encode(x))
    for m in range(4):
        _same(pkg.pcm24_encode_host(x, m, 3, 11), ref.encode(x, m, 3, 11))
    fixed = np.array([[1.0, 2.0, np.inf, np.nan, -0.0, 8388607.5 / 8388608.0], [-1.0, -2.0, -np.inf, -np.nan, 1e-45, -8388609.0 / 8388608.0]], F32)
    assert pkg.pcm24_encode_host(fixed).tolist() == [[8388607, 8388607, 8388607, 0, 0, 8388607], [-8388608, -8388608, -8388608, 0, 0, -8388608]]


@pytest.mark.parametrize("seed", [None, 0, 12345])
def test_host_encode_equals_the_reference_on_random_values(pkg, seed):
    rng = np.random.default_rng(19)
    x = (rng.standard_normal((2, 1 << 15)) * 0.4).astype(F32)
    x[:, ::97] *= 4  # some clip
    for first in (0, 12345, (1 << 31) - 70000, (1 << 32) + 5):
        for m in (0, 3):
            _same(pkg.pcm24_encode_host(x, m, first, seed), ref.encode(x, m, first, seed))
    # a nonzero first_frame is the same as the tail of a longer array
    _same(pkg.pcm24_encode_host(x[:, 1001:], 1, 1001, seed), pkg.pcm24_encode_host(x, 1, 0, seed)[:, 1001:])


def test_levels_host_counts_what_the_s24_encode_clamps(pkg):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 20000)) * 0.5).astype(F32)
    x[0, :6] = [1.0, -1.0, np.nextafter(F32(1), F32(0)), np.inf, -np.inf, np.nan]
    for seed in (None, 9):
        for m, first in ((0, 0), (2, 4321)):
            io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S24, seed)
            acc = pkg.levels_host(x, m, first, io)
            want = ref.clipped(x, m, first, seed)
            assert int(acc.clipped[m]) == want and want > 100, (seed, m, int(acc.clipped[m]), want)
            assert all(int(acc.clipped[o]) == 0 for o in range(4) if o != m)
            # the same samples, by the code: the clamp changed the value
            r = ref.rounded(x, m, first, seed)
            assert want == int(np.count_nonzero(~np.isnan(r) & (r != ref.encode(x, m, first, seed))))
            # over a divisor: x / g is what is encoded; with the track's own divisor nothing clamps
            fin = np.where(np.isfinite(x), x, F32(0))
            g = pkg.rescale_gain([np.abs(fin).max()])
            assert g > 1
            acc = pkg.levels_host(fin, m, first, io, clip_divisor=g)
            assert int(acc.clipped[m]) == ref.clipped(fin / F32(g), m, first, seed) == 0
            g2 = F32(1.5)
            acc = pkg.levels_host(fin, m, first, io, clip_divisor=g2)
            want2 = ref.clipped(fin / g2, m, first, seed)
            assert int(acc.clipped[m]) == want2 and 0 < want2 < want, (want2, want)
    # +1.0f is clipped (code 8388607), -1.0f is not (code -8388608); an fp32 and an int16 output count by their own rules
    one = np.array([[1.0, -1.0], [0.0, 0.0]], F32)
    assert int(pkg.levels_host(one, 0, 0, pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S24)).clipped[0]) == 1
    assert int(pkg.levels_host(one, 0, 0, pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16)).clipped[0]) == 0
    assert int(pkg.levels_host(one, 0, 0, pkg.sample_io()).clipped[0]) == 0


def test_host_entry_points_refuse_bad_arguments(pkg):
    lib = pkg.hip_lib()
    b = np.zeros(12, np.uint8)
    x = np.zeros(4, F32)
    fp, bp = x.ctypes.data_as(pkg._fp), b.ctypes.data_as(pkg._u8p)
    assert lib.umx_hip_pcm24_decode_host(None, 4, fp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_decode_host(bp, 4, None) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_decode_host(bp, -1, fp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_encode_host(None, 2, 0, 0, None, bp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_encode_host(fp, 2, 0, 0, None, None) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_encode_host(fp, -1, 0, 0, None, bp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_encode_host(fp, 2, 4, 0, None, bp) == pkg.ERR_ARG  # buffers are 0 .. 3
    assert lib.umx_hip_pcm24_encode_host(fp, 2, 0, -1, None, bp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm24_encode_host(fp, 2, 0, 0, None, bp) == 0  # io NULL: no dither
    assert lib.umx_hip_pcm24_decode_host(bp, 4, fp) == 0


# ---------------------------------------------------------------- WAV
def _fmt(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    tag, ch, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", b[20:36])
    return tag, ch, rate, byte_rate, align, bits, struct.unpack("<I", b[40:44])[0], len(b)


def _write_wav(path, tag, bits, channels, rate, payload):
    hdr = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, channels, rate,
                                                                                      rate * channels * bits // 8, channels * bits // 8, bits)
    open(path, "wb").write(hdr + b"data" + struct.pack("<I", len(payload)) + payload)


def test_pcm24_wav_round_trip_and_the_float_loader_decodes_it(pkg, tmp_path):
    rng = np.random.default_rng(2)
    q = rng.integers(ref.QMIN, ref.QMAX + 1, (2, 1001)).astype(np.int32)
    q[:, :4] = [[ref.QMIN, ref.QMAX, 0, -1], [1, -ref.QMAX, ref.QMAX, ref.QMIN]]
    for rate in (44100, 48000):
        p = tmp_path / f"a{rate}.wav"
        pkg.wav_write_pcm24(p, q, rate)
        assert _fmt(p) == (1, 2, rate, rate * 6, 6, 24, 6006, 6050)
        assert open(p, "rb").read()[44:] == ref.pack(q).tobytes()
        back, ch, r = pkg.wav_load_pcm24(p)
        assert (ch, r) == (2, rate)
        _same(back, q)
        assert pkg.wav_load_pcm24(p, probe=True) == (1001, 2, rate)
        f, ch, r = pkg.wav_load_rate(p)
        _same(f, ref.decode(q))
    f, _ = pkg.wav_load(tmp_path / "a44100.wav")
    _same(f, pkg.pcm24_decode_host(q))


def test_pcm24_loader_duplicates_mono_and_refuses_other_encodings(pkg, tmp_path):
    q = np.array([1, -2, 300, ref.QMIN, ref.QMAX], np.int32)
    mono = ref.pack(np.stack([q, q]))[np.arange(30).reshape(5, 6)[:, :3].ravel()]
    _write_wav(tmp_path / "mono.wav", 1, 24, 1, 44100, mono.tobytes())
    back, ch, rate = pkg.wav_load_pcm24(tmp_path / "mono.wav")
    assert (ch, rate) == (1, 44100)
    _same(back, np.stack([q, q]))
    _same(pkg.wav_load(tmp_path / "mono.wav")[0], ref.decode(np.stack([q, q])))
    pkg.wav_write_pcm16(tmp_path / "p16.wav", np.zeros((2, 8), np.int16))
    _write_wav(tmp_path / "f32.wav", 3, 32, 2, 44100, np.zeros(16, F32).tobytes())
    _write_wav(tmp_path / "p32.wav", 1, 32, 2, 44100, np.zeros(16, np.int32).tobytes())
    for name in ("p16.wav", "f32.wav", "p32.wav"):
        with pytest.raises(pkg.HostError) as e:
            pkg.wav_load_pcm24(tmp_path / name)
        assert e.value.code == pkg.HOST_ERR_AUDIO and "24-bit" in str(e.value), name
        with pytest.raises(pkg.HostError):
            pkg.wav_load_pcm24(tmp_path / name, probe=True)
        pkg.wav_load(tmp_path / name)  # the float loader takes all three
    # the probe: the head alone, data that is not there is not counted
    pkg.wav_write_pcm24(tmp_path / "big.wav", np.zeros((2, 100000), np.int32))
    open(tmp_path / "cut.wav", "wb").write(open(tmp_path / "big.wav", "rb").read()[:70000])
    assert pkg.wav_load_pcm24(tmp_path / "big.wav", probe=True) == (100000, 2, 44100)
    assert pkg.wav_load_pcm24(tmp_path / "cut.wav", probe=True)[0] == (70000 - 44) // 6
    assert pkg.wav_load_pcm24(tmp_path / "mono.wav", probe=True) == (5, 1, 44100)
    # rate_out == NULL: 44100 Hz only, as umx_wav_load; null arguments
    pkg.wav_write_pcm24(tmp_path / "r48.wav", np.zeros((2, 8), np.int32), 48000)
    host = pkg.host_lib()
    p, n, ch = pkg._u8p(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    assert host.umx_wav_load_pcm24(str(tmp_path / "r48.wav").encode(), C.byref(p), C.byref(n), C.byref(ch), None, err) == pkg.HOST_ERR_AUDIO
    assert host.umx_wav_load_pcm24(None, C.byref(p), C.byref(n), C.byref(ch), None, err) == pkg.ERR_ARG
    assert host.umx_wav_write_pcm24_rate(str(tmp_path / "x.wav").encode(), None, 4, 44100, err) == pkg.ERR_ARG
    host.umx_wav_free_pcm24(None)
