"""Resampling to 44.1 kHz and back, the host half: the fp32 tap table the device kernel reads against the float64
definition (tests/resample_ref.py), the natural output length, that definition against an independent formulation (scipy's
upfirdn with the continuous kernel sampled on the 1/L grid) and against physics (DC gain, a tone's amplitude and phase, no delay),
and the rate-aware WAV reader / writer.  No GPU."""
import math
import struct
import wave as wavemod

import numpy as np
import pytest

import resample_ref as rr

PAIRS = [(48000, 44100), (44100, 48000), (96000, 44100), (44100, 96000), (22050, 44100), (44100, 22050), (8000, 44100),
         (44100, 8000), (32000, 44100), (44056, 44100)]


@pytest.mark.parametrize("rin,rout", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_tap_table_is_the_float64_definition_rounded_once(pkg, rin, rout):
    taps, first = pkg.resample_taps(rin, rout)
    M, L, b, D, K = rr.geometry(rin, rout)
    assert taps.shape == (L, K) and first == -D
    ref = rr.taps(rin, rout)
    err = np.abs(taps.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-15
    assert (err <= bound).all(), float((err / np.maximum(np.abs(ref), 1e-30)).max())
    # the taps of each phase sum to ~1 (unit DC gain within the passband ripple)
    assert np.abs(ref.sum(axis=1) - 1.0).max() < 2e-3


def test_known_table_shapes(pkg):
    for (rin, rout), (L, K) in {(48000, 44100): (147, 16), (44100, 48000): (160, 16), (44100, 8000): (80, 70)}.items():
        taps, first = pkg.resample_taps(rin, rout)
        assert taps.shape == (L, K) and first == -(K - 2) // 2


def test_resampled_length_is_ceil_n_l_over_m(pkg):
    for rin, rout in PAIRS:
        M, L, _, _, _ = rr.geometry(rin, rout)
        for n in (1, 2, 13, 2_646_000, 26_460_001):
            assert pkg.resampled_length(n, rin, rout) == -(-n * L // M), (rin, rout, n)
    for bad in ((7999, 44100), (44100, 192001), (0, 44100), (-48000, 44100)):
        assert pkg.resampled_length(100, *bad) < 0, bad
    assert pkg.resampled_length(100, 192000, 8000) == 5 and pkg.resampled_length(100, 8000, 192000) == 2400


def _upfirdn_ref(x, rin, rout):
    """y[j] = sum_i x[i] h(j M - i L), h the continuous kernel sampled on the 1/(M L) grid, via scipy's polyphase FIR."""
    from scipy.signal import upfirdn
    M, L, b, _, _ = rr.geometry(rin, rout)
    m0 = M * math.ceil(rr.W * L / b)  # half-length, a multiple of M so that the output grid lines up
    m = np.arange(-m0, m0 + 1, dtype=np.float64)
    h = b / M * rr.kernel(b * m / (M * L))
    n_out = rr.natural_length(x.shape[1], rin, rout)
    y = np.stack([upfirdn(h, ch, up=L, down=M) for ch in x])
    return y[:, m0 // M: m0 // M + n_out]


@pytest.mark.parametrize("rin,rout", [(48000, 44100), (44100, 48000), (96000, 44100), (44100, 8000), (22050, 44100)])
def test_restatement_equals_an_independent_upfirdn_formulation(rin, rout):
    x = np.random.default_rng(3).standard_normal((2, 3001))
    y = rr.resample(x, rin, rout)
    z = _upfirdn_ref(x, rin, rout)
    assert y.shape == z.shape
    assert np.abs(y - z).max() < 1e-12


@pytest.mark.parametrize("rin,rout", [(48000, 44100), (44100, 48000), (96000, 44100), (32000, 44100), (44100, 22050)])
def test_dc_gain_tone_amplitude_phase_and_no_delay(rin, rout):
    n = rin // 5  # 0.2 s
    y = rr.resample(np.ones((2, n)), rin, rout)
    edge = 200  # away from the zero padding at both ends
    assert np.abs(y[:, edge:-edge] - 1.0).max() < 2e-3
    f = 1000.0
    x = np.sin(2 * np.pi * f * np.arange(n) / rin)
    y = rr.resample(np.stack([x, -x]), rin, rout)
    want = np.sin(2 * np.pi * f * np.arange(y.shape[1]) / rout)  # same amplitude, same phase: no delay
    assert np.abs(y[0, edge:-edge] - want[edge:-edge]).max() < 3e-3
    assert np.abs(y[1, edge:-edge] + want[edge:-edge]).max() < 3e-3


def _write_wav(path, data_frames, rate, pcm16):
    """(n, 2) float -> a stereo WAV at `rate`, PCM16 or IEEE float."""
    if pcm16:
        q = np.round(np.clip(data_frames, -1, 1) * 32767).astype("<i2")
        with wavemod.open(str(path), "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(q.tobytes())
        return
    body = np.asarray(data_frames, "<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 2, rate, rate * 8, 8, 32)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(body)) + body)


@pytest.mark.parametrize("pcm16", [True, False], ids=["pcm16", "float"])
def test_wav_load_rate_reads_any_rate_and_the_plain_loader_still_refuses(pkg, tmp_path, pcm16):
    frames = np.random.default_rng(4).uniform(-0.9, 0.9, (4801, 2))
    _write_wav(tmp_path / "a48.wav", frames, 48000, pcm16)
    _write_wav(tmp_path / "a44.wav", frames, 44100, pcm16)
    got, ch, rate = pkg.wav_load_rate(tmp_path / "a48.wav")
    ref, ch44 = pkg.wav_load(tmp_path / "a44.wav")
    assert rate == 48000 and ch == ch44 == 2
    assert np.array_equal(got, ref)
    _, _, r44 = pkg.wav_load_rate(tmp_path / "a44.wav")
    assert r44 == 44100
    with pytest.raises(pkg.HostError) as e:
        pkg.wav_load(tmp_path / "a48.wav")
    assert "only supports the following sample rate (Hz): 44100" in str(e.value)
    _write_wav(tmp_path / "a4k.wav", frames, 4000, pcm16)
    with pytest.raises(pkg.HostError):
        pkg.wav_load_rate(tmp_path / "a4k.wav")


def test_wav_write_rate_puts_the_rate_in_the_header(pkg, tmp_path):
    x = np.random.default_rng(5).standard_normal((2, 777)).astype(np.float32)
    pkg.wav_write(tmp_path / "o.wav", x, rate=48000)
    b = (tmp_path / "o.wav").read_bytes()
    assert struct.unpack("<II", b[24:32]) == (48000, 48000 * 8)
    got, ch, rate = pkg.wav_load_rate(tmp_path / "o.wav")
    assert rate == 48000 and np.array_equal(got, x)
    pkg.wav_write(tmp_path / "p.wav", x)  # the default stays 44.1 kHz
    assert struct.unpack("<I", (tmp_path / "p.wav").read_bytes()[24:28])[0] == 44100
