"""tests/fp32_weights.py -- raw float32 weights for the fp32-resident family of the engine (csrc/engine_init.h load_weight: plane GEMMs
on two fp16 planes of w 2^e with ONE power-of-two scale per source tensor, "form 2"; lstm_batch_kernel<WQ = false>; the one-track
context's gemm_bf16x3_kernel<BQ_F32> and fp32 W_hh).  A target is a dict name -> np.float32 array: views_from_file_tensors hands a bare
array over as DTYPE_F32 and stage_f64.target_weights takes it as it is.

Every float32 weight the suite ran before was a dequantised u8 / u16 value of a U(-k, k) draw: 256 or 65536 distinct values per tensor,
all within a few binades of the tensor's maximum.  Here:

  plain(ggml, H, seed)   ggml.synth_weights as float32, never quantised: full mantissas.
  wide(ggml, H, seed)    plain with row r of fc1 / fc2 / fc3 times 2^-g_r, g_r = r mod 13, the matching BatchNorm running_mean times
                         2^-g_r and BatchNorm weight times 2^g_r: every value stays exact, in exact arithmetic the stage outputs are
                         plain's, and the rows of one tensor now span 2^12 under the tensor's one scale (inside the 2^17 that
                         csrc/gemm_planes.h documents as loss-free).  Every lstm.weight_ih_l*_reverse times 2^-3, so that the two
                         directions of W_ih carry different load-time exponents (bs[0] != bs[1] across bsplit) -- asserted.  Target 3's
                         fc3.weight is zero: load_weight's mx == 0 branch, where the scale stays at its default.
  mixed(file_targets)    the quantised tensors of ggml.read_model with target 1's lstm.weight_hh_l1 and fc2.weight replaced by their
                         float32 arrays: W_hh and fc2 are then expanded for all four targets, fc1, W_ih and fc3 stay integer, and both
                         families run in one context.
"""
import math

import numpy as np

import stage_f64 as sf

ROW_SPREAD = 13               # g_r cycles through 0 .. 12
REVERSE_IH_SHIFT = 3          # lstm.weight_ih_l*_reverse times 2^-3
ZERO_TARGET = 3               # its fc3.weight is zero
SPLIT_FIXED_EXP = 14          # csrc/gemm_planes.h GP_SPLIT_FIXED_EXP
DENSE = (("fc1", "bn1"), ("fc2", "bn2"), ("fc3", "bn3"))
MIXED_TARGET, MIXED_NAMES = 1, ("lstm.weight_hh_l1", "fc2.weight")


def plain(ggml, H, seed):
    return [{k: np.ascontiguousarray(v, np.float32) for k, v in d.items()} for d in ggml.synth_weights(H, seed)]


def row_shifts(rows):
    return np.arange(rows) % ROW_SPREAD


def wide(ggml, H, seed):
    out = plain(ggml, H, seed)
    for t, d in enumerate(out):
        for fc, bn in DENSE:
            g = row_shifts(d[fc + ".weight"].shape[0]).astype(np.float32)
            d[fc + ".weight"] = (d[fc + ".weight"] * np.exp2(-g)[:, None]).astype(np.float32)
            d[bn + ".running_mean"] = (d[bn + ".running_mean"] * np.exp2(-g)).astype(np.float32)
            d[bn + ".weight"] = (d[bn + ".weight"] * np.exp2(g)).astype(np.float32)
        for layer in range(3):
            n = f"lstm.weight_ih_l{layer}_reverse"
            d[n] = (d[n] * np.float32(2.0 ** -REVERSE_IH_SHIFT)).astype(np.float32)
            assert load_exponent(d[n]) != load_exponent(d[n[:-len("_reverse")]]), (t, n)
        if t == ZERO_TARGET:
            d["fc3.weight"] = np.zeros_like(d["fc3.weight"])
    return out


def mixed(file_targets):
    out = [dict(d) for d in file_targets]
    for n in MIXED_NAMES:
        out[MIXED_TARGET][n] = np.ascontiguousarray(file_targets[MIXED_TARGET][n]["f32"], np.float32)
    return out


def dequantised(file_targets):
    """ggml.read_model's targets -> the same as bare float32 arrays."""
    return [{k: np.ascontiguousarray(v, np.float32) for k, v in sf.target_weights(d).items()} for d in file_targets]


def load_exponent(w):
    """load_weight's e of one source tensor: 2^e brings the largest finite |w| into [2^14, 2^15); None for an all-zero tensor (the
    scale stays 1)."""
    w = np.asarray(w, np.float32)
    fin = np.abs(w[np.isfinite(w)])
    mx = float(fin.max()) if fin.size else 0.0
    if mx == 0.0:
        return None
    return min(max(SPLIT_FIXED_EXP + 1 - math.frexp(mx)[1], -100), 100)


def row_spread(w):
    """log2 of (largest row maximum / smallest row maximum) of a matrix with no zero row."""
    m = np.abs(np.asarray(w, np.float64)).max(axis=1)
    return float(np.log2(m.max() / m.min()))


def zero_mask_reference(wt, T, precision="float64"):
    """The mask of a target whose fc3.weight is zero: relu(bn3(0) x output_scale + output_mean) in every frame."""
    return sf.mask(wt, np.zeros((T, wt["fc3.weight"].shape[1]), np.float32), precision)


def cpu_activations(ggml, wt, H, T=24, seed=11):
    """The inputs of every stage of one target (name -> float32 array) without a GPU, as skewed_weights.cpu_activations forms them
    for file tensors: x from the float32 STFT of T frames of ggml.synth_audio, then each stage's float64 evaluation rounded to
    float32.  -> (x, a1, lo, a2, state)."""
    N = (T - 1) * sf.HOP
    wave = ggml.synth_audio(N, seed)
    x = sf.crop_x(sf.magnitude(sf.stft(wave, N, "float32"), "float32")).astype(np.float32)
    state = np.zeros(12 * (H // 2), np.float32)
    a1 = sf.fc1(wt, x, "float64").astype(np.float32)
    lo = sf.lstm(wt, H, a1, state, "float64").astype(np.float32)
    a2 = sf.fc2(wt, a1, lo, "float64").astype(np.float32)
    return x, a1, lo, a2, state
