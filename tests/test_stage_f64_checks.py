"""The float64 stage checker of tests/stage_f64.py has teeth (CPU only): the float64 reference cast to float32 passes every stage, and
each plausible kernel fault, planted into that cast, fails its stage by at least ten times the bound.  Also pins the geometry helper's
restatement of the host's run split."""
import numpy as np
import pytest

import stage_f64 as sf
import wiener_em_ref

HOP, NB = sf.HOP, sf.NB


def _wave(n, seed):
    return np.random.default_rng(seed).uniform(-0.8, 0.8, (2, n)).astype(np.float32)


def _stft64_faulty(wave, N, right_pad_shift=0):
    """stft_f64 with the right reflect padding taken one sample too far left (a pad built from N instead of N - 1)."""
    n, T = wave.shape[1], sf.n_frames(N)
    w = sf._hann(np.float64)
    out = np.zeros((2, T, NB), np.complex128)
    for c in range(2):
        buf = np.zeros(N + 4096)
        buf[2048:2048 + n] = wave[c]
        buf[:2048] = buf[2048:4096][::-1].copy()
        buf[-2048:] = buf[-4096 - right_pad_shift:-2048 - right_pad_shift][::-1].copy()
        for f in range(T):
            out[c, f] = np.fft.rfft(buf[f * HOP:f * HOP + 4096] * w)
    return out


def _irfft_packed(s):
    """A real inverse FFT through one complex FFT of half the length (even samples real, odd imaginary): with the imaginary parts at
    DC and Nyquist left in, they leak into every sample as an even / odd offset."""
    n = 4096
    k = np.arange(n // 2)
    a, b = s[k], np.conj(s[n // 2 - k])
    z = np.fft.ifft(0.5 * (a + b) + 0.5j * np.exp(2j * np.pi * k / n) * (a - b))
    x = np.empty(n)
    x[0::2], x[1::2] = z.real, z.imag
    return x


def _istft64_faulty(y, n, N, keep_edge_imag=False, interior_nw_block=None, drop_run_edges=None):
    """istft_f64 with one planted fault: the imaginary parts at DC / Nyquist kept; the interior window sum-square (1.5) on overlap-add
    buffer block `interior_nw_block`; run `drop_run_edges = (r, run_len)`'s first three blocks without the previous run's frames."""
    T = sf.n_frames(N)
    w = sf._hann(np.float64)
    nw = np.zeros((T + 3) * HOP)
    for f in range(T):
        nw[f * HOP:f * HOP + 4096] += w * w
    if interior_nw_block is not None:
        nw[interior_nw_block * HOP:(interior_nw_block + 1) * HOP] = 1.5
    out = np.zeros((2, n))
    for c in range(2):
        buf = np.zeros((T + 3) * HOP)
        for f in range(T):
            s = y[c, f].copy()
            if not keep_edge_imag:
                s[0], s[-1] = s[0].real, s[-1].real
            fr = _irfft_packed(s)
            contrib = fr * w / (nw[f * HOP:f * HOP + 4096] + 1e-8)
            if drop_run_edges is not None:
                r, run_len = drop_run_edges
                r0 = r * run_len
                if f < r0:
                    for b in range(4):
                        if r0 <= f + b < r0 + 3:
                            contrib[b * HOP:(b + 1) * HOP] = 0
            buf[f * HOP:f * HOP + 4096] += contrib
        out[c] = buf[2048:2048 + n]
    return out


@pytest.fixture(scope="module")
def front():
    """T = 23 (last STFT run of 3 frames), N % 1024 = 517."""
    N = (23 - 1) * HOP + 517
    wave = _wave(N, 5)
    return N, wave, sf.stft(wave, N, "float64"), sf.stft(wave, N, "float32")


@pytest.fixture(scope="module")
def back():
    """Stems of a lane with n % 1024 != 0 from a spectrum whose DC / Nyquist bins have imaginary parts (a filter's output can)."""
    N = (23 - 1) * HOP + 517
    n = N - 300
    rng = np.random.default_rng(6)
    y = (rng.standard_normal((2, sf.n_frames(N), NB)) + 1j * rng.standard_normal((2, sf.n_frames(N), NB))).astype(np.complex64)
    return N, n, y, sf.istft(y, n, N, "float64"), sf.istft(y, n, N, "float32")


def _fails_by_10x(r):
    assert r["failure"] is not None and r["excess"] >= 10, r


def test_float64_cast_to_float32_passes_every_stage(front, back):
    N, wave, s64, s32 = front
    assert sf.check("spec", s64.astype(np.complex64), s64, s32, "spectrum")["failure"] is None
    m64, m32 = sf.magnitude(s32, "float64"), sf.magnitude(s32, "float32")
    assert sf.check("mix_mag", m64.astype(np.float32), m64, m32, "spectrum")["failure"] is None
    Nb, n, y, o64, o32 = back
    r = sf.check("stems", o64.astype(np.float32), o64, o32, "stems")
    assert r["failure"] is None, r
    mags = [np.abs(s32) * (0.2 + 0.2 * j) for j in range(4)]
    for it in (1, 2):
        y64, y32 = sf.wiener(s32, mags, it, "float64"), sf.wiener(s32, mags, it, "float32")
        for j in range(4):
            r = sf.check("y", y64[j].astype(np.complex64), y64[j], y32[j], "spectrum")
            assert r["failure"] is None, r


def test_checker_fails_reflect_padding_off_by_one(front):
    N, wave, s64, s32 = front
    _fails_by_10x(sf.check("spec", _stft64_faulty(wave.astype(np.float64), N, 1).astype(np.complex64), s64, s32, "spectrum"))


def test_checker_fails_last_frame_of_partial_stft_run_zeroed(front):
    N, wave, s64, s32 = front
    T = s64.shape[1]
    assert sf.last_stft_run(T) == 3
    got = s64.astype(np.complex64)
    got[:, T - 1] = 0
    r = sf.check("spec", got, s64, s32, "spectrum")
    _fails_by_10x(r)
    assert f"frame {T - 1} of {T}" in r["failure"] and "partial run" in r["failure"]


def test_checker_fails_bins_2047_2048_swapped(front):
    N, wave, s64, s32 = front
    got = s64.astype(np.complex64)
    got[:, :, [2047, 2048]] = got[:, :, [2048, 2047]]
    _fails_by_10x(sf.check("spec", got, s64, s32, "spectrum"))


def test_checker_fails_dc_nyquist_imaginary_parts_kept(back):
    N, n, y, o64, o32 = back
    got = _istft64_faulty(np.asarray(y, np.complex128), n, N, keep_edge_imag=True).astype(np.float32)
    _fails_by_10x(sf.check("stems", got, o64, o32, "stems"))


def test_checker_fails_interior_window_normalisation_on_an_edge_block(back):
    N, n, y, o64, o32 = back
    got = _istft64_faulty(np.asarray(y, np.complex128), n, N, interior_nw_block=2).astype(np.float32)  # output block 0
    r = sf.check("stems", got, o64, o32, "stems", T=sf.n_frames(N))
    _fails_by_10x(r)
    assert "hop block 0 " in r["failure"] and "segment edge" in r["failure"]


def test_checker_fails_one_runs_edge_blocks_not_added(back):
    N, n, y, o64, o32 = back
    T, run_len = sf.n_frames(N), 6
    got = _istft64_faulty(np.asarray(y, np.complex128), n, N, drop_run_edges=(2, run_len)).astype(np.float32)
    r = sf.check("stems", got, o64, o32, "stems", T=T, run_len=run_len)
    _fails_by_10x(r)
    assert "first three blocks of fused run 2" in r["failure"]


def test_checker_fails_lane_tail_zeroed(back):
    N, n, y, o64, o32 = back
    assert n % HOP
    got = o64.astype(np.float32)
    got[:, n - n % HOP:] = 0
    _fails_by_10x(sf.check("stems", got, o64, o32, "stems"))


def test_checker_fails_last_r_batch_dropped(monkeypatch):
    T = 201
    assert sf.last_r_batch(T) == 1
    N = (T - 1) * HOP
    bins = np.arange(0, NB, 64)
    spec = sf.stft(_wave(N, 9), N, "float32")
    mags = [np.abs(spec) * (0.1 + 0.3 * j) for j in range(4)]
    y64 = sf.wiener(spec, mags, 1, "float64", bins=bins)
    y32 = sf.wiener(spec, mags, 1, "float32", bins=bins)
    cov = wiener_em_ref._covariance

    def without_last_batch(y, v):
        last = (y.shape[1] - 1) // sf.WIENER_BATCH * sf.WIENER_BATCH
        return cov(y[:, :last], v[:last])
    monkeypatch.setattr(wiener_em_ref, "_covariance", without_last_batch)
    bad = sf.wiener(spec, mags, 1, "float64", bins=bins)
    for j in range(4):
        _fails_by_10x(sf.check("y", bad[j].astype(np.complex64), y64[j], y32[j], "spectrum"))


def test_checker_refuses_an_ill_conditioned_yardstick():
    """Mono (R == L) with target magnitudes proportional to |X| in both channels: Cxx is rank one plus the regulariser, and the
    float32 evaluation of the closed-form inverse is about 2e-2 from float64 -- a bound of 4x that would pass nearly anything, so
    the check fails on the yardstick itself, even for the float64 result cast to float32."""
    N = 30 * HOP
    w = _wave(N, 16)
    w[1] = w[0]
    spec = sf.stft(w, N, "float32")
    mags = [np.abs(spec) * (0.1 + 0.3 * j) for j in range(4)]
    y64, y32 = sf.wiener(spec, mags, 1, "float64"), sf.wiener(spec, mags, 1, "float32")
    r = sf.check("y", y64[0].astype(np.complex64), y64[0], y32[0], "spectrum")
    assert r["rel32"] > 10 * sf.YARDSTICK_CAP_REL and r["failure"] and "no yardstick" in r["failure"], r
    # masks that differ per channel, frame and bin, as the network's do: well conditioned again
    rng = np.random.default_rng(17)
    mags = [np.abs(spec) * rng.uniform(0.05, 1.0, spec.shape) for j in range(4)]
    y64, y32 = sf.wiener(spec, mags, 1, "float64"), sf.wiener(spec, mags, 1, "float32")
    assert sf.check("y", y64[0].astype(np.complex64), y64[0], y32[0], "spectrum")["failure"] is None


def test_bin_subset_of_the_filter_matches_the_whole_filter():
    """sf.wiener(bins=...) is the whole filter's output at those bins (max_abs still over the whole spectrogram)."""
    N = 9 * HOP
    spec = sf.stft(_wave(N, 12) * 40, N, "float32")
    mags = [np.abs(spec) * (0.1 + 0.3 * j) for j in range(4)]
    assert sf.max_abs(spec) > 1
    bins = np.array([0, 1, 700, 2047, 2048])
    whole, part = sf.wiener(spec, mags, 2, "float64"), sf.wiener(spec, mags, 2, "float64", bins=bins)
    for j in range(4):
        np.testing.assert_allclose(part[j], whole[j][:, :, bins], rtol=1e-12, atol=1e-12)


def test_float32_yardsticks_follow_float64():
    """The packed inverse FFT of the planted fault is exact once DC / Nyquist are real; the float32 evaluations are the same formulas: within float32 rounding of the float64 ones."""
    s = np.random.default_rng(14).standard_normal(NB) + 1j * np.random.default_rng(15).standard_normal(NB)
    s[0], s[-1] = s[0].real, s[-1].real
    np.testing.assert_allclose(_irfft_packed(s), np.fft.irfft(s, 4096), atol=1e-13)
    N = 7 * HOP + 5
    wave = _wave(N, 13)
    s64, s32 = sf.stft(wave, N, "float64"), sf.stft(wave, N, "float32")
    assert sf.distances(s32, s64, "spectrum")[0] < 1e-6
    o64, o32 = sf.istft(s64, N - 9, N, "float64"), sf.istft(s64, N - 9, N, "float32")
    assert sf.distances(o32, o64, "stems")[0] < 1e-6
    np.testing.assert_allclose(sf.istft(s64, N, N, "float64"), wave, atol=1e-6)


def test_geometry_cases_are_hit_at_256_and_other_cu_counts():
    g = sf.geometries(256)
    assert sf.n_frames(g["last_fused_run=1@1"]) == 73 and sf.n_frames(g["last_fused_run=2@1"]) == 65
    assert sf.fused_run_split(73, 1, 256) == (9, 9) and sf.fused_run_split(65, 1, 256) == (9, 8)
    for cus in (32, 80, 304):
        assert set(sf.geometries(cus)) == set(sf.GEOMETRY_CASES)
    assert len(sf.GEOMETRY_CASES) == 13


def test_run_split_depends_on_active_lanes():
    # 3 lanes against 2 at T = 4095 (a call with one lane absent), and 48 lanes against one at T = 915
    assert sf.fused_run_split(4095, 3, 256) != sf.fused_run_split(4095, 2, 256)
    assert sf.fused_run_split(915, 48, 256) != sf.fused_run_split(915, 1, 256)


def test_plane_gemm_limit_restatement():
    T = sf.plane_gemm_max_T(64, 128)
    assert 2 * (64 * T + 256) * 2976 * 2 < 2 ** 31 <= 2 * (64 * (T + 1) + 256) * 2976 * 2
