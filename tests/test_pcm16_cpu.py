"""16-bit PCM in and out, the host side: the library's restatement of the decode / encode / dither rules
(umx_hip_pcm16_decode_host / _encode_host, csrc/pcm16.h -- the functions the kernels call) against tests/pcm16_ref.py bit for bit,
the properties of the rules themselves, and the 16-bit PCM WAV functions of the host library.  No GPU."""
import struct

import numpy as np
import pytest

import pcm16_ref as ref

ALL_CODES = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
# the issue's vectors of the dither word w
W_VECTORS = [((0, 0, 0), [0, 1, 2, 3], [0xAE6F80F1, 0xA07C7A97, 0x0E77CEB6, 0x7E1BD18E]),
             ((1, 3, 1), [0, 1, 2 ** 31 - 1], [0x03172956, 0x1597C993, 0x194856F0])]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    raw = {np.dtype(np.float32): np.uint32, np.dtype(np.int16): np.uint16}[a.dtype]
    bad = np.flatnonzero(a.view(raw).ravel() != b.view(raw).ravel())
    assert bad.size == 0, (bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


def test_reference_dither_words_are_the_issues_vectors():
    for (seed, m, ch), ks, want in W_VECTORS:
        assert [int(x) for x in ref.w(seed, m, ch, ks)] == want


def test_host_decode_equals_the_reference_on_every_code(pkg):
    _same(pkg.pcm16_decode_host(ALL_CODES), ref.decode(ALL_CODES))
    # and it is the float loader's expression, (float)q / 32767.f
    assert pkg.pcm16_decode_host(np.array([32767, -32767, -32768, 1], np.int16)).tolist() == [1.0, -1.0, np.float32(-32768) / np.float32(32767),
                                                                                              np.float32(1) / np.float32(32767)]


def test_round_trip_is_exact_without_dither_and_within_one_lsb_with_it(pkg):
    x = pkg.pcm16_decode_host(np.stack([ALL_CODES, ALL_CODES[::-1]]))
    _same(pkg.pcm16_encode_host(x), np.stack([ALL_CODES, ALL_CODES[::-1]]))
    _same(ref.encode(x), np.stack([ALL_CODES, ALL_CODES[::-1]]))
    for seed in (0, 7, 0xFFFFFFFF):
        q = pkg.pcm16_encode_host(x, buffer=2, first_frame=5, dither_seed=seed)
        _same(q, ref.encode(x, 2, 5, seed))
        assert np.abs(q.astype(np.int32) - np.stack([ALL_CODES, ALL_CODES[::-1]]).astype(np.int32)).max() <= 1


def test_host_dither_words_through_the_encoder(pkg):
    """x = 0 with dither encodes rint(d): the library's w is pinned through d for the issue's vectors (|d| > 0.5 <=> q != 0, its sign)."""
    for (seed, m, ch), ks, want in W_VECTORS:
        for k, wv in zip(ks, want):
            dd = ((wv & 0xFFFF) + (wv >> 16) - 65535) / 65536.0
            q = pkg.pcm16_encode_host(np.zeros((2, 1), np.float32), buffer=m, first_frame=k, dither_seed=seed)[ch, 0]
            assert q == int(np.rint(np.float32(dd))), (seed, m, ch, k, dd, q)
            # and exactly: x chosen so that x * 32767 + d crosses 0.5 only for this d
            _same(pkg.pcm16_encode_host(np.full((2, 1), 0.25, np.float32), m, k, seed), ref.encode(np.full((2, 1), 0.25, np.float32), m, k, seed))


def test_ties_go_to_even_and_the_awkward_values(pkg):
    for half, even in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (100.5, 100), (32766.5, 32766)):
        x = np.array([[ref.preimage(half)], [-ref.preimage(half)]], np.float32)
        assert np.float32(x[0, 0] * np.float32(32767.0)) == np.float32(half)
        assert pkg.pcm16_encode_host(x).ravel().tolist() == [even, -even]
    x = ref.awkward_floats()
    _same(pkg.pcm16_encode_host(x), ref.encode(x))
    for m in range(4):
        _same(pkg.pcm16_encode_host(x, m, 3, 11), ref.encode(x, m, 3, 11))
    fixed = np.array([[1.0, 2.0, np.inf, np.nan, -0.0], [-1.0, -2.0, -np.inf, -np.nan, 1e-45]], np.float32)
    assert pkg.pcm16_encode_host(fixed).tolist() == [[32767, 32767, 32767, 0, 0], [-32767, -32768, -32768, 0, 0]]


@pytest.mark.parametrize("seed", [None, 0, 12345])
def test_host_encode_equals_the_reference_on_random_values(pkg, seed):
    rng = np.random.default_rng(19)
    x = (rng.standard_normal((2, 1 << 16)) * 0.4).astype(np.float32)
    x[:, ::97] *= 4  # some clip
    for first in (0, (1 << 30) - 1000, (1 << 31) - 70000):
        for m in range(4):
            _same(pkg.pcm16_encode_host(x, m, first, seed), ref.encode(x, m, first, seed))


def test_dither_is_tpdf():
    k = np.arange(1 << 20)
    d0, d1 = ref.d(0, 0, 0, k).astype(np.float64), ref.d(0, 0, 1, k).astype(np.float64)
    for dd in (d0, d1, ref.d(9, 3, 1, k + (1 << 30)).astype(np.float64)):
        assert dd.min() > -1.0 and dd.max() < 1.0
        assert abs(dd.mean()) < 0.005 and abs(dd.var() - 1.0 / 6.0) < 0.005, (dd.mean(), dd.var())
    assert abs(np.corrcoef(d0, d1)[0, 1]) < 0.005
    assert abs(np.corrcoef(d0[1:], d0[:-1])[0, 1]) < 0.005


def test_host_entry_points_refuse_bad_arguments(pkg):
    lib = pkg.hip_lib()
    q = np.zeros(4, np.int16)
    x = np.zeros(4, np.float32)
    fp, ip = x.ctypes.data_as(pkg._fp), q.ctypes.data_as(pkg._i16p)
    assert lib.umx_hip_pcm16_decode_host(None, 4, fp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm16_decode_host(ip, -1, fp) == pkg.ERR_ARG
    assert lib.umx_hip_pcm16_encode_host(fp, 2, 4, 0, None, ip) == pkg.ERR_ARG  # buffers are 0 .. 3
    assert lib.umx_hip_pcm16_encode_host(fp, 2, 0, -1, None, ip) == pkg.ERR_ARG
    assert lib.umx_hip_pcm16_encode_host(fp, 2, 0, 0, None, ip) == 0  # io NULL: no dither


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


def test_pcm16_wav_round_trip_and_the_float_loader_decodes_it(pkg, tmp_path):
    rng = np.random.default_rng(2)
    q = rng.integers(-32768, 32768, (2, 1000)).astype(np.int16)
    q[:, :4] = [[-32768, 32767, 0, -1], [1, -32767, 32767, -32768]]
    for rate in (44100, 48000):
        p = tmp_path / f"a{rate}.wav"
        pkg.wav_write_pcm16(p, q, rate)
        assert _fmt(p) == (1, 2, rate, rate * 4, 4, 16, 4000, 4044)
        back, ch, r = pkg.wav_load_pcm16(p)
        assert (ch, r) == (2, rate)
        _same(back, q)
        f, ch, r = pkg.wav_load_rate(p)
        _same(f, ref.decode(q))
    f, _ = pkg.wav_load(tmp_path / "a44100.wav")
    _same(f, pkg.pcm16_decode_host(q))


def test_pcm16_loader_duplicates_mono_and_refuses_other_encodings(pkg, tmp_path):
    q = np.array([1, -2, 300, -32768, 32767], np.int16)
    _write_wav(tmp_path / "mono.wav", 1, 16, 1, 44100, q.tobytes())
    back, ch, rate = pkg.wav_load_pcm16(tmp_path / "mono.wav")
    assert (ch, rate) == (1, 44100)
    _same(back, np.stack([q, q]))
    _write_wav(tmp_path / "p24.wav", 1, 24, 2, 44100, bytes(range(48)))
    _write_wav(tmp_path / "f32.wav", 3, 32, 2, 44100, np.zeros(16, np.float32).tobytes())
    pkg.wav_write(tmp_path / "f32b.wav", np.zeros((2, 8), np.float32))
    for name in ("p24.wav", "f32.wav", "f32b.wav"):
        with pytest.raises(pkg.HostError) as e:
            pkg.wav_load_pcm16(tmp_path / name)
        assert e.value.code == pkg.HOST_ERR_AUDIO, name
        pkg.wav_load(tmp_path / name)  # the float loader takes all three
    # audio_out == NULL: the head alone says the same, data that is not there is not counted (a long file cut short behind its head)
    import ctypes as C
    host = pkg.host_lib()
    big = np.zeros((2, 100000), np.int16)
    pkg.wav_write_pcm16(tmp_path / "big.wav", big)
    open(tmp_path / "cut.wav", "wb").write(open(tmp_path / "big.wav", "rb").read()[:70000])
    for name, rc_want, n_want, ch_want in (("mono.wav", 0, 5, 1), ("big.wav", 0, 100000, 2), ("cut.wav", 0, (70000 - 44) // 4, 2),
                                           ("p24.wav", pkg.HOST_ERR_AUDIO, 0, 2), ("f32.wav", pkg.HOST_ERR_AUDIO, 0, 2)):
        n, ch, rate = C.c_int(), C.c_int(), C.c_int()
        err = C.create_string_buffer(256)
        assert host.umx_wav_load_pcm16(str(tmp_path / name).encode(), None, C.byref(n), C.byref(ch), C.byref(rate), err) == rc_want, name
        assert (n.value, ch.value) == (n_want, ch_want), name
    # rate_out == NULL: 44100 Hz only, as umx_wav_load
    pkg.wav_write_pcm16(tmp_path / "r48.wav", np.zeros((2, 8), np.int16), 48000)
    p, n, ch = pkg._i16p(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    assert pkg.host_lib().umx_wav_load_pcm16(str(tmp_path / "r48.wav").encode(), C.byref(p), C.byref(n), C.byref(ch), None, err) == pkg.HOST_ERR_AUDIO
