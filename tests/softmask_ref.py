"""tests/softmask_ref.py -- the soft mask of UMX_FLAG_SOFTMASK (Open-Unmix's Separator(softmask=True)) restated in numpy:
test infrastructure for tests/test_softmask_cpu.py and tests/test_gpu_softmask.py, on top of tests/residual_ref.py and
tests/wiener_em_ref.py.

  * masks: the engine's rule -- over the active targets in ascending order, a = |X|, g_j = m_j a, d = eps + (((g_j1 + g_j2) + g_j3) + g_j4),
    m'_j = g_j / d -- with every step rounded to `precision`; a skipped target's entry is returned as it came;
  * direct: Open-Unmix's own form X[..., None] * g / (eps + sum g) (the softmask branch of filtering.wiener, before max_abs), float64;
  * magnitudes / wiener: softmask, then the residual (rho from the NORMALISED masks, residual_ref), then wiener_em_ref.wiener_em;
  * rule_errors: how far a float32 result is from the rule evaluated in float64 from the same float32 inputs, against the bound of
    DESIGN 15 (relative 1e-6 plus an absolute 1e-37).
"""
import numpy as np

import residual_ref as rr
import wiener_em_ref

FLAG_SOFTMASK = 0x2
EPS = wiener_em_ref.WIENER_EPS  # 1e-10: Open-Unmix's eps and the engine's WIENER_EPS
RULE_REL, RULE_ABS = 1e-6, 1e-37


def _rt(precision):
    return np.float64 if precision == "float64" else np.float32


def masks(mix_mag, masks_in, flags, precision="float64"):
    """The four mask planes after the rule (entries of skipped targets: as given)."""
    rt = _rt(precision)
    a = np.asarray(mix_mag, rt)
    act = rr.active(flags)
    out = list(masks_in)
    if not act:
        return out
    g = {j: (np.asarray(masks_in[j], rt) * a).astype(rt) for j in act}
    s = g[act[0]]
    for j in act[1:]:
        s = (s + g[j]).astype(rt)
    d = (rt(EPS) + s).astype(rt)
    for j in act:
        out[j] = (g[j] / d).astype(rt)
    return out


def direct(spec, mix_mag, masks_in, flags):
    """Open-Unmix: y = X[..., None] * g / (eps + sum(g, -1, keepdim)); float64, the active targets' estimates by target index."""
    X = np.asarray(spec, np.complex128)
    act = rr.active(flags)
    g = np.stack([np.asarray(masks_in[j], np.float64) * np.asarray(mix_mag, np.float64) for j in act], axis=-1)
    y = X[..., None] * g / (EPS + g.sum(axis=-1, keepdims=True))
    return {j: y[..., i] for i, j in enumerate(act)}


def magnitudes(mix_mag, masks_in, flags, precision="float64"):
    """The four slots' magnitudes [2, T, B] as the filter sees them: softmask (if flagged), then the residual (if flagged)."""
    rt = _rt(precision)
    mm = np.asarray(mix_mag, rt)
    m = masks(mix_mag, masks_in, flags, precision) if flags & FLAG_SOFTMASK else list(masks_in)
    if rr.residual_slot(flags) >= 0:
        return rr.magnitudes(mm, m, flags, precision)
    act = rr.active(flags)
    return [(np.asarray(m[t], rt) * mm).astype(rt) if t in act else np.zeros_like(mm) for t in range(4)]


def wiener(spec, mix_mag, masks_in, flags, n_iter=1, precision="float64", max_abs=None):
    """The filter's output for all four slots: softmask, then residual, then the EM."""
    return wiener_em_ref.wiener_em(spec, magnitudes(mix_mag, masks_in, flags, precision), n_iter=n_iter, precision=precision,
                                   max_abs=max_abs)


def rule_errors(got, mix_mag, masks_in, flags):
    """Per active target: the largest |got - want| / (RULE_REL |want| + RULE_ABS) over the plane (<= 1 passes), `want` the rule in float64
    from the float32 inputs."""
    want = masks(np.asarray(mix_mag, np.float32), [None if m is None else np.asarray(m, np.float32) for m in masks_in], flags, "float64")
    out = {}
    for j in rr.active(flags):
        w = np.asarray(want[j], np.float64)
        out[j] = float((np.abs(np.asarray(got[j], np.float64) - w) / (RULE_REL * np.abs(w) + RULE_ABS)).max())
    return out
