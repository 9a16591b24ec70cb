"""tests/planes_f32_emu.py -- a numpy emulation of the plane GEMMs on float32 weights ("form 2": csrc/engine_init.h load_weight,
csrc/gemm_planes.h with NBP = 2), in the order the kernels have it, and the fc1 and lstm stages built on it
(tests/test_fp32_weights_cpu.py; the GPU side is tests/test_gpu_fp32_weights_f64.py).  The rounding of the matrix instruction and the
epilogues are tests/bf16x3_emu.py's.

  * weight planes: one power of two per SOURCE tensor, 2^e bringing its largest finite |w| into [2^14, 2^15) (an all-zero tensor keeps
    the scale 1); P_hi = fp16(w 2^e), P_lo = fp16(w 2^e - P_hi), round to nearest even.  W_ih is two source tensors, forward rows then
    reverse rows, each with its own e.
  * activation planes as split_planes_kernel forms them: the row times 2^e_m, its largest |a| into [2^14, 2^15) (adaptive: fc1's
    x scale + mean), or the constant 2^14 (tanh / LSTM outputs: W_ih); a1 = fp16(a'), a2 = fp16(a' - a1).
  * per 32-k tile and 16-k half the three matrix instructions of GP_COMPUTE in its order -- a2 P_hi, a1 P_lo, a1 P_hi --, each adding
    its 16 exact products to the fp32 accumulator (bf16x3_emu._mfma: one rounding per 4 products); a2 P_lo is not formed.
  * the unscale per source tensor: columns below bsplit take 2^-e of the forward tensor, the others the reverse tensor's, times the
    row's 2^-e_m: powers of two, exact.  The offset term is zero (o2 = 0).

`fault` plants one of FAULTS:
    "drop_lo"        the low weight plane dropped (a1 P_lo not formed);
    "unscale_fwd"    the forward tensor's unscale applied to the reverse tensor's columns (bsplit ignored);
    "common_scale"   the planes of both tensors formed under ONE scale, from the maximum over both, but unscaled with each tensor's own.
"""
import numpy as np

import bf16x3_emu as emu
import fp32_weights as fw
import stage_f64 as sf

f32 = np.float32
BK = 32                       # GP_BK
FAULTS = ("drop_lo", "unscale_fwd", "common_scale")
ORDER = ((1, 0), (0, 1), (0, 0))  # GP_COMPUTE: (plane of A, plane of B), smallest terms first


def f16(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def split2(v):
    """float32 (already scaled) -> the two fp16 planes, as float32."""
    v = np.asarray(v, f32)
    hi = f16(v)
    return hi, f16((v - hi).astype(f32))


def weight_planes(w, e):
    """One source tensor under the scale 2^e (None: 1) -> (P_hi, P_lo)."""
    return split2((np.asarray(w, f32) * f32(2.0 ** (e or 0))).astype(f32))


def activation_planes(a, fixed_exp=None):
    """(M, K) float32 -> (a1, a2, the per-row unscale 2^-e_m as float64)."""
    a = np.asarray(a, f32)
    if fixed_exp is None:
        e = np.array([fw.load_exponent(r) or 0 for r in a], np.float64)  # the same rule as the weights': frexp of the row maximum
    else:
        e = np.full(a.shape[0], float(fixed_exp))
    a1, a2 = split2((a * np.exp2(e).astype(f32)[:, None]).astype(f32))
    return a1, a2, np.exp2(-e)


def _pad_k(a):
    K = a.shape[1]
    Kp = -(-K // BK) * BK
    if Kp == K:
        return a
    out = np.zeros((a.shape[0], Kp), a.dtype)
    out[:, :K] = a
    return out


def product(a, tensors, fixed_exp=None, fault=None):
    """a (M, K) float32 times the source tensors (each (N_s, K) float32, stacked along N: W_ih's forward and reverse) -> (M, sum N_s)
    float32, as gemm_planes_kernel<MODE, 2> and its _pp / _ps flavours form it."""
    assert fault is None or fault in FAULTS, fault
    own = [fw.load_exponent(w) for w in tensors]
    used = own
    if fault == "common_scale":
        used = [fw.load_exponent(np.concatenate([np.ravel(w) for w in tensors]))] * len(tensors)
    planes = [weight_planes(w, e) for w, e in zip(tensors, used)]
    hi = np.concatenate([p[0] for p in planes])
    lo = np.concatenate([p[1] for p in planes])
    unscale_w = np.concatenate([np.full(len(w), 2.0 ** -((own[0] if fault == "unscale_fwd" else e) or 0)) for w, e in zip(tensors, own)])
    a1, a2, unscale_a = activation_planes(a, fixed_exp)
    ap = emu._k_major([_pad_k(a1), _pad_k(a2)])
    bp = emu._k_major([_pad_k(hi), _pad_k(lo)])
    acc = np.zeros((a.shape[0], hi.shape[0]), f32)
    for k0 in range(0, ap[0].shape[0], emu.BK):  # 16 k per matrix instruction; both halves of a 32-k tile run the same three terms
        for pa, pb in ORDER:
            if not (fault == "drop_lo" and pb == 1):
                acc = emu._mfma(acc, ap[pa][k0:k0 + emu.BK], bp[pb][k0:k0 + emu.BK])
    out = (acc.astype(np.float64) * unscale_a[:, None] * unscale_w[None, :]).astype(f32)  # powers of two: exact
    return out


def fc1_stage(wt, x, fault=None):
    """x tap (T, 2974) -> tanh(bn1(fc1(x scale + mean))): the adaptive row scale of xs, fc1.weight one source tensor."""
    xs = (np.asarray(x, f32) * np.tile(wt["input_scale"], 2).astype(f32)).astype(f32) + np.tile(wt["input_mean"], 2).astype(f32)
    assert xs.dtype == f32
    return np.tanh(emu._bn32(wt, product(xs, [wt["fc1.weight"]], None, fault), "bn1")).astype(f32)


def lstm_stage(wt, H, a1, state, fault=None):
    """fc1 tap (T, H) -> the BiLSTM's output: W_ih x + b_ih of every layer through the plane GEMM (both directions one product, the
    constant scale 2^14 on the activations, fp32 bias add), the recurrence in float64 on W_hh (stage_f64.bilstm_f64's loop), so that
    the lstm stage shows what the W_ih products feed into it and nothing else."""
    Hl = H // 2
    G = 4 * Hl
    st = np.asarray(state, np.float64).reshape(3, 2, 2, Hl)
    inp = np.asarray(a1, f32)
    T = inp.shape[0]
    for layer in range(3):
        names = [f"_l{layer}", f"_l{layer}_reverse"]
        Pall = product(inp, [wt["lstm.weight_ih" + n] for n in names], fw.SPLIT_FIXED_EXP, fault)
        nxt = np.empty((T, H), f32)
        for d, n in enumerate(names):
            P = (Pall[:, d * G:(d + 1) * G] + np.asarray(wt["lstm.bias_ih" + n], f32)).astype(np.float64)
            whh, bhh = np.asarray(wt["lstm.weight_hh" + n], np.float64), np.asarray(wt["lstm.bias_hh" + n], np.float64)
            h, c = st[layer, d, 0].copy(), st[layer, d, 1].copy()
            for step in range(T):
                t = step if d == 0 else T - 1 - step
                g = (P[t] + whh @ h) + bhh
                c = sf.gate_ref("sigmoid", g[Hl:2 * Hl]) * c + sf.gate_ref("sigmoid", g[:Hl]) * np.tanh(g[2 * Hl:3 * Hl])
                h = sf.gate_ref("sigmoid", g[3 * Hl:]) * np.tanh(c)
                nxt[t, d * Hl:(d + 1) * Hl] = h
        inp = nxt
    return inp
