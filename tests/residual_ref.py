"""tests/residual_ref.py -- the residual source of UMX_FLAG_RESIDUAL (Open-Unmix's Separator(residual=True)) restated in numpy:
test infrastructure for tests/test_residual_cpu.py and tests/test_gpu_residual.py.

  * residual_slot: the flag arithmetic of umx_hip_residual_slot;
  * rho_f32: the engine's rule bit for bit -- rho = 1.0f - ((m_j1 + m_j2) + m_j3) in float32 over the active targets in ascending order;
  * magnitudes / wiener: the float64 (or float32) restatement on top of the unchanged tests/wiener_em_ref.wiener_em, which takes signed
    magnitudes as they are: slot r is fed rho |X|, the other skipped slots 0.
"""
import numpy as np

import wiener_em_ref

FLAG_RESIDUAL = 0x8000


def skipped(flags):
    return [t for t in range(4) if flags & (0x100 << t)]


def active(flags):
    return [t for t in range(4) if not flags & (0x100 << t)]


def residual_slot(flags):
    """The lowest skipped target; -1 without the flag; -2 when no target or every target is skipped."""
    if not flags & FLAG_RESIDUAL:
        return -1
    s = skipped(flags)
    if len(s) in (0, 4):
        return -2
    return s[0]


def rho_f32(masks, flags):
    """masks: per target an array of any shape (entries of skipped targets are ignored) -> float32 rho of that shape."""
    act = active(flags)
    s = np.asarray(masks[act[0]], np.float32)
    for j in act[1:]:
        s = (s + np.asarray(masks[j], np.float32)).astype(np.float32)
    return (np.float32(1.0) - s).astype(np.float32)


def rho(masks, flags, precision="float64"):
    if precision == "float32":
        return rho_f32(masks, flags)
    act = active(flags)
    s = np.asarray(masks[act[0]], np.float64)
    for j in act[1:]:
        s = s + np.asarray(masks[j], np.float64)
    return 1.0 - s


def magnitudes(mix_mag, masks, flags, precision="float64"):
    """The four slots' magnitudes [2, T, B]: mask x |X| for an active target, rho |X| for the residual slot, 0 for a silent one."""
    rt = np.float64 if precision == "float64" else np.float32
    mm = np.asarray(mix_mag, rt)
    r = residual_slot(flags)
    assert r >= 0, flags
    out = []
    for t in range(4):
        if t == r:
            out.append((rho(masks, flags, precision).astype(rt) * mm).astype(rt))
        elif t in active(flags):
            out.append((np.asarray(masks[t], rt) * mm).astype(rt))
        else:
            out.append(np.zeros_like(mm))
    return out


def mixture_phase(spec, mags):
    """Zero iterations (UMX_FLAG_NO_WIENER): y_j = mag_j e^{i arg X}, float64."""
    X = np.asarray(spec, np.complex128)
    ph = np.angle(X)
    return [np.asarray(m, np.float64) * np.cos(ph) + 1j * (np.asarray(m, np.float64) * np.sin(ph)) for m in mags]


def wiener(spec, mix_mag, masks, flags, n_iter=1, precision="float64"):
    """The filter's output for all four slots with the residual in slot r."""
    return wiener_em_ref.wiener_em(spec, magnitudes(mix_mag, masks, flags, precision), n_iter=n_iter, precision=precision)


def cxx_inverse(spec, mags):
    """Cxx^-1 [T, B, 2, 2] of the FIRST iteration in float64, from wiener_em_ref's own pieces (on the scaled-down estimates)."""
    X = np.asarray(spec, np.complex128)
    ma = wiener_em_ref.find_max_abs(X)
    y = [yj / ma for yj in mixture_phase(X, mags)]
    v = [wiener_em_ref._psd(yj) for yj in y]
    R = [wiener_em_ref._covariance(y[j], v[j]) for j in range(4)]
    reg = np.sqrt(wiener_em_ref.WIENER_EPS) * np.eye(2)
    Cxx = np.zeros(X.shape[1:] + (2, 2), np.complex128)
    for j in range(4):
        Cxx = Cxx + (reg + v[j][:, :, None, None] * R[j][None])
    return wiener_em_ref._invert(Cxx)
