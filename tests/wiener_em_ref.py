"""tests/wiener_em_ref.py -- the reference's multichannel Wiener filter (wiener.cpp:92-425) with `n_iter` EM iterations, restated in
numpy float64 in the reference's operation order: test infrastructure for tests/test_wiener_em_cpu.py and tests/test_gpu_wiener_em.py.

What it keeps of the reference:
  * the initial estimates y_j = polar(|y_j|, arg X) (wiener.cpp:96-109);
  * max_abs = max(1, max |X| / 10) (wiener.cpp:31-52), the mixture divided by it IN PLACE and the estimates divided by it once, before
    the loop (:115-146); y multiplied by it once, after the loop (:408-422);
  * per iteration: v = sum_c (Re y + Im y)^2 / 2 (:187-202, quirk F5), R_j = (sum of the 200-frame batch sums of y y^H) / (eps + sum v)
    (:204-269), Cxx = sum_j (sqrt(eps) I + v_j R_j) (:301-325: the regularisation once per source, quirk F6), its closed-form inverse
    (:54-84), the gains G_j = v_j (R_j Cxx^-1) (:339-376) applied to the scaled-down MIXTURE (:381-400), not to the previous y.

precision="float32" evaluates the same loop in the reference's own precision: how far THAT is from float64 is the yardstick for a
float32 implementation (the EM iterations amplify rounding: ~2e-5 at one iteration, up to ~7e-4 at three on synthetic segments).
"""
import numpy as np

WIENER_EPS = 1e-10
WIENER_SCALE = 10.0
WIENER_BATCH = 200


def find_max_abs(X):
    """wiener.cpp:31-52: max(1, max over both channels of |X| / scale)."""
    return max(1.0, float(np.abs(X).max()) / WIENER_SCALE)  # (the caller rounds it to its precision)


def _psd(y):
    """wiener.cpp:187-202 for one source: y [2, T, B] -> v [T, B] (F5: (Re + Im)^2, not |y|^2)."""
    s = np.zeros(y.shape[1:], y.real.dtype)
    for c in range(y.shape[0]):
        re = 0.0 + y[c].real + y[c].imag
        s = s + (re * re + 0.0 * 0.0)
    return s / y.shape[0]


def _covariance(y, v):
    """wiener.cpp:204-269 for one source: R [B, 2, 2] from the batches of 200 frames, in batch order."""
    T, B = y.shape[1], y.shape[2]
    R = np.zeros((B, 2, 2), y.dtype)
    weight = np.full(B, WIENER_EPS, v.dtype)
    for pos in range(0, T, WIENER_BATCH):
        end = min(T, pos + WIENER_BATCH)
        yb = y[:, pos:end, :]                                    # [c, t, b]
        tempR = np.einsum("itb,ktb->tbik", yb, np.conj(yb))      # calculateCovariance (:435-478): a conj(b) per frame
        R += tempR.sum(axis=0)                                   # :229-243
        weight += v[pos:end].sum(axis=0)                         # :247-253
    return R / weight[:, None, None]                             # :259-269


def _invert(C):
    """invert4D (wiener.cpp:54-84): closed-form 2x2 inverse per (frame, bin)."""
    a, b, c, d = C[..., 0, 0], C[..., 0, 1], C[..., 1, 0], C[..., 1, 1]
    det = a * d - b * c
    inv_det = 1.0 / det
    out = np.empty_like(C)
    out[..., 0, 0] = inv_det * d
    out[..., 0, 1] = -inv_det * b
    out[..., 1, 0] = -inv_det * c
    out[..., 1, 1] = inv_det * a
    return out


def wiener_em(spec, target_mags, n_iter=1, precision="float64", max_abs=None):
    """spec: complex [2, T, B] mixture; target_mags: 4 x [2, T, B] magnitudes -> 4 x complex [2, T, B] (complex128; complex64 at float32) (the reference's
    wiener_filter with WIENER_ITERATIONS = n_iter).  The caller's arrays are not changed (the reference divides its mixture in place:
    here a copy is).  max_abs: the scale of the whole spectrogram when `spec` holds only some of its bins (the filter is per bin but for
    this scale)."""
    rt, ct = {"float64": (np.float64, np.complex128), "float32": (np.float32, np.complex64)}[precision]
    X = np.array(spec, dtype=ct)                                 # the copy the in-place division below works on
    phase = np.angle(X)
    y = [(np.asarray(m, rt) * np.cos(phase) + 1j * (np.asarray(m, rt) * np.sin(phase))).astype(ct) for m in target_mags]
    max_abs = rt(find_max_abs(X) if max_abs is None else max_abs)
    X /= max_abs                                                 # :118-130, in place
    y = [yj / max_abs for yj in y]                               # :133-146
    T, B = X.shape[1], X.shape[2]
    reg = np.sqrt(rt(WIENER_EPS)) * np.eye(2, dtype=rt)
    for _ in range(n_iter):                                      # :175
        v = [_psd(yj) for yj in y]
        R = [_covariance(y[j], v[j]) for j in range(4)]
        Cxx = np.zeros((T, B, 2, 2), ct)
        for j in range(4):
            Cxx = Cxx + (reg + v[j][:, :, None, None] * R[j][None])
        inv = _invert(Cxx)
        new = []
        for j in range(4):
            gain = np.einsum("bik,tbkl->tbil", R[j], inv)        # R_j Cxx^-1 (:339-361)
            gain = gain * v[j][:, :, None, None]                 # :363-376
            new.append(np.einsum("tbkl,ltb->ktb", gain, X))      # y(c2) = sum_c1 G(c2, c1) x(c1) (:381-400)
        y = new
    return [yj * max_abs for yj in y]                            # :408-422
