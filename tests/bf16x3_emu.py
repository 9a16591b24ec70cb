"""tests/bf16x3_emu.py -- a numpy emulation of the arithmetic of csrc/gemm_bf16x3.h, in the order the kernel has it, and the stages of
a one-track context built on it (tests/test_one_track_checks_cpu.py; the GPU side is tests/test_gpu_one_track_f64.py).

  * split3: x = x1 + x2 + x3, x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), round to nearest even (v_cvt_pk_bf16_f32,
    bf16_rne_bits); the subtractions are exact in fp32.
  * product_six (BQ_F32, BQ_U16; fc2 and fc3 of a one-track context): per 16-k tile the six matrix instructions of BX_COMPUTE in its
    order -- a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1 --, each adding its 16 exact products to the fp32 accumulator, which is rounded to
    nearest after every MFMA_ROUND_K = 4 of them.  How the matrix core rounds inside an instruction is not documented.  With one
    rounding per instruction (16) the emulation is half as far from float64 as gemm_bf16x3_kernel measures on an MI355X; with one per
    4 k it reproduces the kernel's ratios to the float32 evaluation at hidden 1024 -- fc1 1.9 / 2.1 against the kernel's 2.1 / 2.2, fc2
    (K = 2048) 2.7 / 2.8 against 2.8 / 2.9 --; with one per 2 k or per product it overshoots them (fc2 3.6, 4.7), and a truncating
    accumulator is 30 - 250 times off.  That fixes how the emulation rounds, not any bound.
    The u16 weights are dequantised as the staging code does, fl(fl(q s) + o): the file's float32 tensor.
  * product_u8x (BQ_U8X; fc1 and W_ih): the three instructions a3 p, a2 p, a1 p with p = q - c exact in bf16, c and o2 = o + c s from
    skewed_weights.centre_and_o2(..., "recentred_f64") (quant_centre's rule, held to it bit for bit by tests/test_affine_offset_cpu.py);
    the fp32 row sum as the staging threads form it -- a thread owns one row and one 8-k half of every tile and adds
    ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) to its running sum tile after tile; the two halves meet at the end --; then
    fl(fl(s acc) + fl(o2 rowsum)), without contraction (the library is built with -ffp-contract=off).
  * one_track_stages: fc1, lstm, fc2 and mask of one target with these products and the epilogues of gemm_common.h in float32 (batch
    norm through div_by, which gives the correctly rounded quotient); the recurrence itself in float64 on the dequantised W_hh, so that
    the lstm stage shows what the W_ih products feed into it and nothing else.

`fault` plants one of FAULTS into every product it applies to:
    "drop_a2b2", "drop_a3b1"  a second-order term left out (a3 p in the one-plane form; a2 b2 has no counterpart there);
    "centre_128"              the one-plane form centred at 128 whatever the tensor's range;
    "rowsum_a1"               the row sum taken over the bf16-rounded a1 instead of a.
"""
import numpy as np

import skewed_weights as sw
import stage_f64 as sf

f32 = np.float32
BK = 16                                              # BX_BK
MFMA_ROUND_K = 4                                     # products added per rounding of the accumulator inside a matrix instruction
FAULTS = ("drop_a2b2", "drop_a3b1", "centre_128", "rowsum_a1")
SIX_ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # BX_COMPUTE: (plane of A, plane of B), smallest terms first
U8X_ORDER = (2, 1, 0)


def bf16(x):
    """float32 -> the nearest bf16 (ties to even) as float32; finite inputs."""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(f32)


def split3(x):
    x = np.asarray(x, f32)
    x1 = bf16(x)
    r1 = (x - x1).astype(f32)
    x2 = bf16(r1)
    return x1, x2, bf16((r1 - x2).astype(f32))


def _pad_k(a):
    K = a.shape[1]
    Kp = -(-K // BK) * BK
    if Kp == K:
        return a
    out = np.zeros((a.shape[0], Kp), a.dtype)
    out[:, :K] = a
    return out


def _mfma(acc, xT, yT):
    """One matrix instruction: acc (M, N) fp32 += x (M, 16) y (N, 16)^T, the products exact, the accumulator rounded to nearest after
    every MFMA_ROUND_K of them.  xT (16, M), yT (16, N): the operands k-major in float64 (bf16 values: every product is exact)."""
    for k in range(0, BK, MFMA_ROUND_K):
        acc = (acc + xT[k:k + MFMA_ROUND_K].T @ yT[k:k + MFMA_ROUND_K]).astype(f32)  # (float32 + float64 -> float64, then one rounding)
    return acc


def _k_major(planes):
    return [np.ascontiguousarray(p.T, np.float64) for p in planes]


def product_six(a, w, fault=None):
    """a (M, K) float32 times w (N, K) float32 -> (M, N) float32: the six-term form."""
    ap, wp = _k_major(split3(_pad_k(np.asarray(a, f32)))), _k_major(split3(_pad_k(np.asarray(w, f32))))
    skip = {"drop_a2b2": (1, 1), "drop_a3b1": (2, 0)}.get(fault)
    acc = np.zeros((ap[0].shape[1], wp[0].shape[1]), f32)
    for k0 in range(0, ap[0].shape[0], BK):
        for pa, pb in SIX_ORDER:
            if (pa, pb) != skip:
                acc = _mfma(acc, ap[pa][k0:k0 + BK], wp[pb][k0:k0 + BK])
    return acc


def staging_rowsum(a):
    """(M, K) float32, K a multiple of 16 -> the fp32 row sums of the u8 one-plane form."""
    a = np.asarray(a, f32)
    M, K = a.shape
    x = a.reshape(M, K // BK, 2, 8)
    part = ((x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])) + ((x[..., 4] + x[..., 5]) + (x[..., 6] + x[..., 7]))
    rs = np.zeros((M, 2), f32)
    for t in range(K // BK):
        rs = rs + part[:, t]
    assert rs.dtype == f32 and part.dtype == f32
    return rs[:, 0] + rs[:, 1]


def product_u8x(a, q, s, o, fault=None):
    """a (M, K) float32 times the u8 file tensor (q (N, K), s, o) -> (M, N) float32: the one-plane form."""
    assert q.dtype == np.uint8
    a = _pad_k(np.asarray(a, f32))
    c, o2 = sw.centre_and_o2(s, o, False, "fixed" if fault == "centre_128" else "recentred_f64")
    if fault == "centre_128":  # the fault is the centre, not the rounding of o + 128 s (exact in fp32: 128 is a power of two)
        assert c == sw.U8_CENTRE
    a1 = bf16(a)
    ap = _k_major(split3(a))
    p = _k_major([_pad_k(q.astype(f32) - f32(c))])[0]
    acc = np.zeros((a.shape[0], q.shape[0]), f32)
    for k0 in range(0, a.shape[1], BK):
        for pa in U8X_ORDER:
            if not (fault == "drop_a3b1" and pa == 2):
                acc = _mfma(acc, ap[pa][k0:k0 + BK], p[k0:k0 + BK])
    rs = staging_rowsum(a1 if fault == "rowsum_a1" else a)
    add = f32(o2) * rs
    out = f32(s) * acc + add[:, None]
    assert out.dtype == f32
    return out


def _div_by(a, b):
    """gemm_common.h div_by: q = a rcp(b) corrected by one fma step -- the correctly rounded quotient."""
    return (a.astype(np.float64) / b.astype(np.float64)).astype(f32)


def _bn32(wd, y, name):
    g = lambda k: np.asarray(wd[name + "." + k], f32)
    sd = np.sqrt(g("running_var") + f32(1e-5)).astype(f32)
    out = _div_by((y - g("running_mean")).astype(f32), np.broadcast_to(sd, y.shape)) * g("weight") + g("bias")
    assert out.dtype == f32
    return out


def fc1_stage(ft, x, fault=None):
    """x tap (T, 2974) -> tanh(bn1(fc1(x scale + mean))) as gemm_bf16x3_kernel<G_FC1, BQ_U8X> forms it."""
    wd = sf.target_weights(ft)
    xs = np.asarray(x, f32) * np.tile(wd["input_scale"], 2).astype(f32) + np.tile(wd["input_mean"], 2).astype(f32)
    r = ft["fc1.weight"]
    return np.tanh(_bn32(wd, product_u8x(xs, r["q"], r["scale"], r["offset"], fault), "bn1")).astype(f32)


def lstm_stage(ft, H, a1, state, fault=None):
    """fc1 tap (T, H) -> the BiLSTM's output: W_ih x + b_ih of every layer and direction through the one-plane form (fp32 bias add),
    the recurrence in float64 on the dequantised W_hh (stage_f64.bilstm_f64's loop)."""
    wd = sf.target_weights(ft)
    Hl = H // 2
    st = np.asarray(state, np.float64).reshape(3, 2, 2, Hl)
    inp = np.asarray(a1, f32)
    T = inp.shape[0]
    for layer in range(3):
        nxt = np.empty((T, H), f32)
        for d, sfx in enumerate(("", "_reverse")):
            n = f"_l{layer}{sfx}"
            r = ft["lstm.weight_ih" + n]
            P = (product_u8x(inp, r["q"], r["scale"], r["offset"], fault) + np.asarray(wd["lstm.bias_ih" + n], f32)).astype(np.float64)
            whh, bhh = np.asarray(wd["lstm.weight_hh" + n], np.float64), np.asarray(wd["lstm.bias_hh" + n], np.float64)
            h, c = st[layer, d, 0].copy(), st[layer, d, 1].copy()
            for step in range(T):
                t = step if d == 0 else T - 1 - step
                g = (P[t] + whh @ h) + bhh
                c = sf.gate_ref("sigmoid", g[Hl:2 * Hl]) * c + sf.gate_ref("sigmoid", g[:Hl]) * np.tanh(g[2 * Hl:3 * Hl])
                h = sf.gate_ref("sigmoid", g[3 * Hl:]) * np.tanh(c)
                nxt[t, d * Hl:(d + 1) * Hl] = h
        inp = nxt
    return inp


def fc2_stage(ft, a1, lo, fault=None):
    wd = sf.target_weights(ft)
    cat = np.concatenate([np.asarray(a1, f32), np.asarray(lo, f32)], axis=1)
    return np.maximum(_bn32(wd, product_six(cat, wd["fc2.weight"], fault), "bn2"), f32(0))


def mask_stage(ft, a2, fault=None):
    wd = sf.target_weights(ft)
    y = _bn32(wd, product_six(a2, wd["fc3.weight"], fault), "bn3")
    out = np.maximum(y * np.tile(wd["output_scale"], 2).astype(f32) + np.tile(wd["output_mean"], 2).astype(f32), f32(0))
    assert out.dtype == f32
    return out


def one_track_stages(ft, H, x, a1, lo, a2, state, fault=None, stages=("fc1", "lstm", "fc2", "mask")):
    """name -> the stage of one target (ggml.read_model record `ft`) from the inputs of each stage (skewed_weights.cpu_activations)."""
    fns = {"fc1": lambda: fc1_stage(ft, x, fault), "lstm": lambda: lstm_stage(ft, H, a1, state, fault),
           "fc2": lambda: fc2_stage(ft, a1, lo, fault), "mask": lambda: mask_stage(ft, a2, fault)}
    return {k: fns[k]() for k in stages}
