"""tests/stage_f64.py -- per-stage float64 references, their float32 yardsticks, the checker that compares a kernel's tap with both,
and the segment geometries where the kernels' tiles have edges.  Test infrastructure for tests/test_stage_f64_checks.py (CPU) and
tests/test_gpu_geometry_f64.py (GPU); nothing here needs a GPU except `device_cu_count`.

Every reference is computed from the engine's own tap of that stage's INPUT, so each stage's error is its own.  Each stage is
evaluated twice: in float64 (the reference) and as a plain float32 evaluation of the same formula from the same inputs (numpy float32
FFTs, torch float32, wiener_em_ref at precision="float32").  How far the float32 evaluation is from float64 is the yardstick: a kernel
passes a stage when its distance to float64 is at most C times the yardstick's, plus a small floor, both over the whole segment and in
its worst block (a frame for spectra and activations, a 1024-sample hop block for stems).  A block's error is normalised by the RMS
block norm of the reference, not by its own norm, so that near-silent blocks do not dominate.
"""
import ctypes
import importlib.util
import os
from pathlib import Path

import numpy as np
import torch

import wiener_em_ref

HERE = Path(__file__).resolve().parent
NB, CROP, NFFT, HOP = 2049, 1487, 4096, 1024
STFT_RUN = 4                 # csrc/stft_kernels.h: frames per workgroup of stft_kernel
WIENER_BATCH = wiener_em_ref.WIENER_BATCH  # frames per batch of the R sums (wiener.cpp:204-269)
N_MIN, N_MAX = 4096, 4094 * HOP + HOP - 1  # engine_init.h: segment_samples >= NFFT and N / HOP + 2 <= 4096 (T <= 4095)
C_DEFAULT = 4.0              # a kernel may be this many times as far from float64 as the float32 evaluation of its formula ...
FLOOR = 2e-7                 # ... plus this (about two float32 ulps, relative), for stages the float32 evaluation gets nearly exact
# Measured on an MI355X over tests/test_gpu_geometry_f64.py: the worst ratio to the float32 evaluation is 5.1 (spec, a near-silent
# lane with a full-scale click: rel L2 1.5e-7 against numpy float32's 3.0e-8, inside the floor), 3.1 (y, worst frame), 2.6 (fc1,
# worst frame); every other stage stays below 2.4.
# The bound scales with the float32 evaluation's own error, so a formula that float32 evaluates badly would make the check toothless:
# where the float32 evaluation is itself further than this from float64 (whole segment / worst block), the check fails instead.
# Measured on the GPU tests: at most 2.1e-4 / 5.3e-4 (the Wiener filter, on the mono and the click lanes).  About 2e-2 / 5e-2 on a
# mono input whose target magnitudes are proportional to |X| in both channels (tests/test_stage_f64_checks.py).
YARDSTICK_CAP_REL, YARDSTICK_CAP_BLK = 1e-3, 3e-3


def _load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", HERE / "golden" / "make_golden.py")
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


mg = _load_make_golden()


def n_frames(N):
    return N // HOP + 1


# ---------------------------------------------------------------- geometry (restated from the host code)
def fused_run_split(T, lanes, n_cus):
    """engine_stages.h (fused Wiener + inverse STFT): (run_len, nruns) for a call with `lanes` active track lanes."""
    runs = max(1, min(T // 8, (4 * n_cus + lanes - 1) // lanes))
    run_len = max(3, (T + runs - 1) // runs)
    return run_len, (T + run_len - 1) // run_len


def last_fused_run(T, lanes, n_cus):
    run_len, nruns = fused_run_split(T, lanes, n_cus)
    return T - (nruns - 1) * run_len


def last_stft_run(T):
    """Frames in stft_kernel's last run of STFT_RUN."""
    return T - (T - 1) // STFT_RUN * STFT_RUN


def last_r_batch(T):
    """Frames in the last 200-frame batch of the Wiener R sums."""
    return T - (T - 1) // WIENER_BATCH * WIENER_BATCH


def plane_gemm_bytes(lanes, T, hidden):
    """engine_init.h: the bytes behind one plane-GEMM operand base when all `lanes` lanes form one launch -- both fp16 planes of
    rows = lanes x Tp + 256 rows of max(KX, 2 x hidden) columns; the guard refuses contexts where this reaches 2^31."""
    rows = lanes * max(T, 256) + 256
    return 2 * rows * max(2976, 2 * hidden) * 2


def plane_gemm_max_T(lanes, hidden):
    """engine_init.h: the largest T a context of `lanes` track lanes accepts under the plane GEMMs' 32-bit addressing."""
    T = 4095
    while T > 0:
        if plane_gemm_bytes(lanes, T, hidden) < 2 ** 31 and lanes * 2 * T * 2176 * 4 < 2 ** 32:
            return T
        T -= 1
    raise AssertionError("no T fits")


def device_cu_count(device=0):
    """hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount) through the HIP runtime torch has loaded (its bundled copy, else
    the one on the loader's path)."""
    import torch as _t  # noqa: F401  (brings in the HIP runtime the engine uses)
    bundled = os.path.join(os.path.dirname(_t.__file__), "lib", "libamdhip64.so")
    try:
        lib = ctypes.CDLL(bundled if os.path.exists(bundled) else "libamdhip64.so")
    except OSError as e:
        raise RuntimeError(f"device_cu_count: no HIP runtime library to ask for the CU count ({e})") from e
    v = ctypes.c_int(0)
    HIP_ATTR_MULTIPROCESSOR_COUNT = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h); callers cross-check with torch
    rc = lib.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, device)
    assert rc == 0 and v.value > 0, (rc, v.value)
    return v.value


def _first_T(pred, lo=9, hi=4095):
    for T in range(lo, hi + 1):
        if pred(T):
            return T
    raise AssertionError("no segment length has this geometry")


def _N(T, rem):
    return (T - 1) * HOP + rem


GEOMETRY_CASES = ("T%4=0,N%1024=0", "T%4=1,N%1024=1", "T%4=2,N%1024=1023", "T%4=3,N%1024=other", "N=4096", "T=4095",
                  "last_fused_run=1@1", "last_fused_run=1@3", "last_fused_run=2@1", "last_fused_run=2@3", "T=200", "T=201", "T=401")


def geometries(n_cus):
    """{case: N} for every case of GEOMETRY_CASES; each case is asserted to hold for its N.  `@k`: k active lanes of a fused call."""
    g = {
        "T%4=0,N%1024=0": _N(20, 0),
        "T%4=1,N%1024=1": _N(29, 1),
        "T%4=2,N%1024=1023": _N(22, 1023),
        "T%4=3,N%1024=other": _N(23, 517),
        "N=4096": N_MIN,
        "T=4095": N_MAX,
        "T=200": _N(200, 333),
        "T=201": _N(201, 0),
        "T=401": _N(401, 1023),
    }
    for k in (1, 2):
        for lanes in (1, 3):
            T = _first_T(lambda T: last_fused_run(T, lanes, n_cus) == k)
            g[f"last_fused_run={k}@{lanes}"] = _N(T, 0 if lanes == 1 else 700)
    assert tuple(sorted(g)) == tuple(sorted(GEOMETRY_CASES)), sorted(g)
    for case, N in g.items():
        T, r = n_frames(N), N % HOP
        assert N_MIN <= N <= N_MAX, case
        if case.startswith("T%4="):
            assert T % 4 == int(case[4]), case
            want = case.split("N%1024=")[1]
            assert (r not in (0, 1, 1023)) if want == "other" else r == int(want), case
        elif case == "N=4096":
            assert T == 5 and fused_run_split(T, 3, n_cus)[1] == 1, case
        elif case.startswith("T="):
            assert T == int(case[2:]), case
        else:
            k, lanes = int(case.split("=")[1].split("@")[0]), int(case.split("@")[1])
            assert last_fused_run(T, lanes, n_cus) == k, case
    assert last_r_batch(n_frames(g["T=201"])) == 1 and last_r_batch(n_frames(g["T=200"])) == WIENER_BATCH
    assert {last_stft_run(n_frames(N)) for N in g.values()} == {1, 2, 3, 4}
    return g


# ---------------------------------------------------------------- references: float64 and the float32 yardstick
def _hann(dt):
    return (0.5 * (1 - np.cos(2 * np.pi * np.arange(NFFT) / NFFT))).astype(dt)


def stft(wave, N, precision):
    """(2, n) waves of one lane -> (2, T, 2049): the reference's STFT of a segment buffer of N samples (dsp.cpp:109-176)."""
    if precision == "float64":
        return mg.stft_f64(np.asarray(wave, np.float64), N)
    wave = np.asarray(wave, np.float32)
    n, T = wave.shape[1], n_frames(N)
    out = np.empty((2, T, NB), np.complex64)
    w = _hann(np.float32)
    for c in range(2):
        buf = np.zeros(N + NFFT, np.float32)
        buf[2048:2048 + n] = wave[c]
        buf[:2048] = buf[2048:4096][::-1]
        buf[-2048:] = buf[-4096:-2048][::-1].copy()
        fr = np.lib.stride_tricks.sliding_window_view(buf, NFFT)[::HOP][:T]
        out[c] = np.fft.rfft(fr * w, axis=-1)
    return out


def istft(y, n, N, precision):
    """(2, T, 2049) -> (2, n): the reference's inverse STFT and window-normalised overlap-add, cropped to the lane's n."""
    if precision == "float64":
        return mg.istft_f64(np.asarray(y, np.complex128), n, N)
    y = np.array(y, np.complex64)
    T = y.shape[1]
    w = _hann(np.float32)
    nw = np.zeros((T + 3) * HOP, np.float32)
    for f in range(T):
        nw[f * HOP:f * HOP + NFFT] += w * w
    out = np.empty((2, n), np.float32)
    for c in range(2):
        s = y[c]
        s[:, 0] = s[:, 0].real
        s[:, -1] = s[:, -1].real
        fr = np.fft.irfft(s, NFFT, axis=-1).astype(np.float32) * np.float32(NFFT) * w / np.float32(NFFT)
        buf = np.zeros((T + 3) * HOP, np.float32)
        for f in range(T):
            buf[f * HOP:f * HOP + NFFT] += fr[f] / (nw[f * HOP:f * HOP + NFFT] + np.float32(1e-8))
        out[c] = buf[2048:2048 + n]
    return out


def max_abs(spec):
    """wiener.cpp:31-52 rounded to float32, from the spec tap."""
    return np.float32(max(1.0, float(np.abs(np.asarray(spec, np.complex128)).max()) / 10.0))


def magnitude(spec, precision):
    if precision == "float64":
        return np.abs(np.asarray(spec, np.complex128))
    s = np.asarray(spec, np.complex64)
    return np.sqrt(s.real * s.real + s.imag * s.imag)


def crop_x(mix_mag):
    """(2, T, 2049) -> (T, 2974): the network input, channel after channel (inference.cpp:41-56)."""
    return np.concatenate([mix_mag[0, :, :CROP], mix_mag[1, :, :CROP]], axis=1)


def wiener(spec, mags, n_iter, precision, bins=None):
    """The filter's output y (4 x (2, T, 2049)) from the spec and target_mag taps; `bins`: only those bins (the filter is per bin
    but for max_abs, which is taken over the whole spectrogram first)."""
    ma = wiener_em_ref.find_max_abs(np.asarray(spec, np.complex128))
    if bins is not None:
        spec = np.asarray(spec)[:, :, bins]
        mags = [np.asarray(m)[:, :, bins] for m in mags]
    return wiener_em_ref.wiener_em(spec, mags, n_iter=n_iter, precision=precision, max_abs=ma)


def mixture_phase(spec, mags, precision, bins=None):
    """FLAG_NO_WIENER: y_j = |y_j| e^{i arg X}."""
    ct, rt = (np.complex128, np.float64) if precision == "float64" else (np.complex64, np.float32)
    X = np.asarray(spec, ct) if bins is None else np.asarray(spec, ct)[:, :, bins]
    ph = np.angle(X)
    out = []
    for m in mags:
        m = np.asarray(m, rt) if bins is None else np.asarray(m, rt)[:, :, bins]
        out.append((m * np.cos(ph) + 1j * (m * np.sin(ph))).astype(ct))
    return out


def target_weights(file_target):
    """One target of ggml.read_model -> name -> the file's dequantised float32 tensor."""
    return {k: v["f32"] for k, v in file_target.items()}


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dt)


def _bn(wt, y, name, dt):
    return (y - _t(wt[name + ".running_mean"], dt)) / torch.sqrt(_t(wt[name + ".running_var"], dt) + 1e-5) * \
        _t(wt[name + ".weight"], dt) + _t(wt[name + ".bias"], dt)


def _dt(precision):
    return torch.float64 if precision == "float64" else torch.float32


def fc1(wt, x, precision):
    """x tap (T, 2974) -> tanh(bn1(fc1(x * scale + mean)))  (inference.cpp:78-97)."""
    dt = _dt(precision)
    with torch.no_grad():
        xs = _t(x, dt) * _t(np.tile(wt["input_scale"], 2), dt) + _t(np.tile(wt["input_mean"], 2), dt)
        return torch.tanh(_bn(wt, xs @ _t(wt["fc1.weight"], dt).T, "bn1", dt)).numpy()


def lstm(wt, H, a1, state, precision):
    """fc1 tap (T, H) and one target's carried state [3][2][2][H/2] -> the 3-layer BiLSTM's output (T, H)."""
    dt = _dt(precision)
    with torch.no_grad():
        m = torch.nn.LSTM(H, H // 2, num_layers=3, bidirectional=True).to(dt)
        m.load_state_dict({f"{wn}_l{l}{sfx}": _t(wt[f"lstm.{wn}_l{l}{sfx}"], dt) for l in range(3) for sfx in ("", "_reverse")
                           for wn in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")})
        st = _t(state, dt).reshape(3, 2, 2, H // 2)
        h0, c0 = st[:, :, 0].reshape(6, 1, H // 2).contiguous(), st[:, :, 1].reshape(6, 1, H // 2).contiguous()
        out, _ = m(_t(a1, dt)[:, None, :], (h0, c0))
        return out[:, 0].numpy()


def fc2(wt, a1, lo, precision):
    """[fc1 | lstm] taps -> relu(bn2(fc2(.)))  (inference.cpp:118-140)."""
    dt = _dt(precision)
    with torch.no_grad():
        return torch.relu(_bn(wt, torch.cat([_t(a1, dt), _t(lo, dt)], dim=1) @ _t(wt["fc2.weight"], dt).T, "bn2", dt)).numpy()


def mask(wt, a2, precision):
    """fc2 tap -> relu(bn3(fc3(.)) * output_scale + output_mean)  (inference.cpp:143-166), (T, 4098)."""
    dt = _dt(precision)
    with torch.no_grad():
        a3 = _bn(wt, _t(a2, dt) @ _t(wt["fc3.weight"], dt).T, "bn3", dt)
        return torch.relu(a3 * _t(np.tile(wt["output_scale"], 2), dt) + _t(np.tile(wt["output_mean"], 2), dt)).numpy()


def target_mag(mk, mix_mag, precision):
    """mask (T, 4098) x mix_mag (2, T, 2049) -> (2, T, 2049)  (inference.cpp:173-183)."""
    rt = np.float64 if precision == "float64" else np.float32
    mk, mm = np.asarray(mk, rt), np.asarray(mix_mag, rt)
    return np.stack([mk[:, :NB] * mm[0], mk[:, NB:] * mm[1]])


# ---------------------------------------------------------------- the checker
def blocks(a, kind):
    """(blocks, -1): kind "spectrum" (2, T, F) -> frames; "rows" (T, F) -> frames; "stems" (2, n) -> 1024-sample hop blocks."""
    a = np.asarray(a)
    if kind == "spectrum":
        return a.transpose(1, 0, 2).reshape(a.shape[1], -1)
    if kind == "rows":
        return a.reshape(a.shape[0], -1)
    if kind == "stems":
        n = a.shape[1]
        nb = (n + HOP - 1) // HOP
        p = np.zeros((2, nb * HOP), a.dtype)
        p[:, :n] = a
        return p.reshape(2, nb, HOP).transpose(1, 0, 2).reshape(nb, -1)
    raise ValueError(kind)


def distances(got, ref, kind):
    """(whole-segment relative L2, worst block's error / RMS block norm of ref, index of that block)."""
    ct = np.complex128 if (np.iscomplexobj(got) or np.iscomplexobj(ref)) else np.float64
    d = blocks(np.asarray(got, ct) - np.asarray(ref, ct), kind)
    r = blocks(np.asarray(ref, ct), kind)
    dn = np.sqrt((np.abs(d) ** 2).sum(axis=1))
    rn2 = (np.abs(r) ** 2).sum(axis=1)
    tot = float(np.sqrt(rn2.sum()))
    if tot == 0.0:  # a silent reference: absolute distances
        return float(np.sqrt((dn ** 2).sum())), float(dn.max()), int(dn.argmax())
    rms = tot / np.sqrt(len(rn2))
    k = int(dn.argmax())
    return float(np.sqrt((dn ** 2).sum())) / tot, float(dn[k]) / rms, k


def describe_block(k, kind, T, run_len=None):
    """Where block k sits in the kernels' tiling: STFT runs (frames), fused-kernel runs (frames and hop blocks)."""
    tags = []
    if kind in ("spectrum", "rows"):
        if k % STFT_RUN in (0, STFT_RUN - 1) or k >= (T - 1) // STFT_RUN * STFT_RUN:
            tags.append("STFT run edge" + (" (last, partial run)" if k >= (T - 1) // STFT_RUN * STFT_RUN and last_stft_run(T) < 4 else ""))
        if run_len and k % run_len in (0, run_len - 1):
            tags.append(f"fused run seam (run {k // run_len})")
        if k >= (T - 1) // WIENER_BATCH * WIENER_BATCH:
            tags.append("last R batch")
        return f"frame {k} of {T}" + (": " + ", ".join(tags) if tags else "")
    b = k + 2  # hop block k of the output is block k + 2 of the overlap-add buffer (the first 2048 samples are padding)
    if b < 4 or b > T - 1:
        tags.append("segment edge (window normalisation)")
    if run_len and b % run_len < 3 and b < T + 3:
        tags.append(f"one of the first three blocks of fused run {b // run_len}")
    return f"hop block {k} (samples {k * HOP}..{(k + 1) * HOP - 1})" + (": " + ", ".join(tags) if tags else "")


def check(stage, got, ref64, ref32, kind, *, C=C_DEFAULT, floor=FLOOR, where="", T=None, run_len=None):
    """-> dict with the kernel's and the yardstick's distances to float64 and how far past its bound each is ("excess" <= 1 passes).
    `failure` is None or a message naming the stage, the place (`where`: geometry and lane) and the worst block -- or saying that the
    float32 evaluation is too far from float64 here to measure the kernel by (YARDSTICK_CAP_*)."""
    rel, blk, k = distances(got, ref64, kind)
    rel32, blk32, k32 = distances(ref32, ref64, kind)
    b_rel, b_blk = C * rel32 + floor, C * blk32 + floor
    r = {"stage": stage, "where": where, "rel": rel, "rel32": rel32, "blk": blk, "blk32": blk32, "block": k,
         "ratio_rel": rel / max(rel32, 1e-30), "ratio_blk": blk / max(blk32, 1e-30),
         "excess": max(rel / b_rel, blk / b_blk), "failure": None}
    if not (np.isfinite(np.asarray(got)).all() and r["excess"] <= 1.0):
        T = T if T is not None else (np.asarray(ref64).shape[1] if kind == "spectrum" else np.asarray(ref64).shape[0])
        r["failure"] = (f"{stage} {where}: rel L2 {rel:.3e} (bound {b_rel:.3e} = {C} x float32's {rel32:.3e} + {floor:g}); worst "
                        f"block {blk:.3e} (bound {b_blk:.3e}) at {describe_block(k, kind, T, run_len)}"
                        + ("" if np.isfinite(np.asarray(got)).all() else "; NON-FINITE values"))
    elif not (rel32 <= YARDSTICK_CAP_REL and blk32 <= YARDSTICK_CAP_BLK):
        r["failure"] = (f"{stage} {where}: the float32 evaluation is itself {rel32:.3e} (worst block {blk32:.3e}) from float64, past "
                        f"{YARDSTICK_CAP_REL:g} / {YARDSTICK_CAP_BLK:g}: an ill-conditioned formula here, no yardstick for the kernel")
    return r


class Report:
    """Collects the checks of one test, so that a failure lists every stage that failed, not only the first."""

    def __init__(self):
        self.rows = []

    def add(self, r):
        self.rows.append(r)
        return r

    def exact(self, stage, ok, where, msg):
        self.rows.append({"stage": stage, "where": where, "excess": 0.0 if ok else float("inf"),
                          "failure": None if ok else f"{stage} {where}: {msg}"})

    def failures(self):
        return [r["failure"] for r in self.rows if r["failure"]]

    def assert_ok(self):
        f = self.failures()
        assert not f, f"{len(f)} of {len(self.rows)} checks failed:\n  " + "\n  ".join(f)
