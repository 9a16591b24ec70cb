"""tests/skewed_weights.py -- weight fixtures whose quantised range is ASYMMETRIC, the two float64 references of a stage on them, and
a numpy emulation of the quantised matrix products (tests/test_affine_offset_cpu.py on the CPU, tests/test_gpu_affine_offset.py on
the GPU).

Every quantised product applies the file's affine map w = q s + o to the accumulated sum,
    sum_k a_k (q_k s + o) = s sum_k a_k (q_k - c) + (o + c s) sum_k a_k,
and the second term is a constant times the fp32 row sum of the activations.  The rounding of that row sum (and of the first sum,
which cancels against it) is multiplied by |o + c s|: how far the code that stands for a zero weight lies from the centre c.
ggml.synth_weights draws every matrix from U(-k, k): the zero-weight code is 127 of 254 and |o + 128 s| is about one code, so no
other fixture of the suite makes that factor matter.  Trained tensors have outliers; here a matrix is redrawn as a zero-mean Laplace
body at its usual standard deviation sigma, clipped to the variant's range, with one planted minimum and one planted maximum:
    "high": -4 sigma .. +25 sigma        "low": -14 sigma .. +4 sigma
so that the zero-weight code lies 35 / 198 of 254 (u8) and 9039 / 50971 of 65534 (u16).  "low" began at -25 sigma and was narrowed for
the definition gap below: near-zero weights are then fl(q s) of about 25 sigma plus o, rounded in the binade of 0.25 .. 0.5 for fc1,
and on a lane at 30 times the level fc1's gap came to 3.0e-6 / 4.1e-6; at -14 sigma (the binade below) it is half that.  (skew_matrix
also moves the outlier by up to 4 % where the file scale it gives makes the definition's per-weight rounding biased.)

Two conditions make a fixture count (assert_sharp, definition_gaps; asserted on the CPU for every fixture the GPU tests use):
  * sharpness: |o + 128 s| / s >= 64 (u8), |o + 32896 s| / s >= 16384 (u16) for every skewed tensor, read back from the file;
  * definition gap: the reference defines a weight as fl(fl(q s) + o) in fp32, the kernels apply the exact affine map.
    Per stage, the distance (stage_f64.distances) between two float64 evaluations on the same activations, one with the dequantised
    fp32 weights and one with float64(q) float64(s) + float64(o), stays below half of test_gpu_batch.REG_STAGE (2.5e-6), over the
    whole segment and in the worst frame.
Measured on the CPU (fixture "h128_all", 64 frames of ggml.synth_audio, the worst of targets 0 .. 2; whole segment / worst frame):
    fc1 4.0e-7 / 4.8e-7, lstm 2.2e-7 / 2.3e-7, fc2 3.2e-7 / 3.4e-7, mask 3.8e-8 / 3.9e-8; with the audio at 30 times the level
    fc1 9.1e-7 / 1.20e-6 (on an MI355X, the lane at that level: 1.04e-6);
the control target (plain U(-k, k)) 5.6e-8 / 5.7e-8 at fc1 and below 4e-8 elsewhere.
On the same fixture the emulation below (plane_product) is, against the float64 evaluation with exact-affine matrices and as a
multiple of the float32 evaluation's distance: with the fixed centres 45 - 113 (fc1), 4 - 11 (fc2), 8 - 25 (mask), 2 - 4 (lstm);
with a per-tensor centre and o + c s formed in fp32 5 - 19 (fc1); with the per-tensor centre and the sum formed in double at most
1.0 everywhere.
"""
import numpy as np

import stage_f64 as sf

FAMILIES = ("fc1", "ih", "hh", "fc2", "fc3")
ALL = frozenset(FAMILIES)
HIGH, LOW = (-4.0, 25.0), (-14.0, 4.0)
RANGES = {"high": HIGH, "low": LOW}
U8_CENTRE, U16_CENTRE = 128, 32896           # the centres of every tensor before the per-tensor centre (W_hh in the batched recurrences: still)
SHARP_U8, SHARP_U16 = 64.0, 16384.0          # codes between the zero-weight code and those centres: a quarter of the code range
GAP_BOUND = 0.5 * 5e-6                       # half of tests/test_gpu_batch.py REG_STAGE (asserted equal in test_affine_offset_cpu.py)
CONTROL_TARGET = 3                           # stays as ggml.synth_weights drew it


def family(name):
    """Tensor name -> its matrix family, or None (biases, batch norm, input / output vectors)."""
    if name in ("fc1.weight", "fc2.weight", "fc3.weight"):
        return name[:3]
    if name.startswith("lstm.weight_ih"):
        return "ih"
    if name.startswith("lstm.weight_hh"):
        return "hh"
    return None


def variant(target, name):
    """The variant of matrix `name` in target `target`, or None for the control target.  Target 0: fc high, forward chains high,
    reverse chains low.  Target 1: the opposite.  Target 2: fc1 low, fc2 high, fc3 low, the directions swapping with the layer."""
    if target == CONTROL_TARGET or family(name) is None:
        return None
    flip = {0: 0, 1: 1}.get(target)
    if name.startswith("lstm."):
        rev = int(name.endswith("_reverse"))
        layer = int(name.split("_l")[1][0])
        k = rev ^ (flip if flip is not None else layer & 1)
        return ("high", "low")[k]
    if flip is not None:
        return ("high", "low")[flip]
    return {"fc1": "low", "fc2": "high", "fc3": "low"}[name[:3]]


NARROW = tuple(round(1.0 - 0.002 * i, 3) for i in range(21))  # the outlier at 1.0, 0.998 .. 0.96 of its place (13.4 sigma: still sharp)
BIAS_MAX = 1e-7  # |mean over the tensor of fl(fl(q s) + o) - (q s + o)|, in units of sigma


def skew_matrix(ggml, name, a, which, rng):
    """A matrix of a's shape and standard deviation: Laplace body, clipped to the variant's range, one planted minimum and maximum.
    The per-weight rounding of the definition is usually unbiased (its mean over a tensor is 1e-8 sigma or less), but a file scale s
    with few significant bits makes q s round one way: a mean error of 5e-7 sigma, which positive activations (fc1's, fc3's) add up
    into a definition gap of 6e-6.  The outlier is then moved in, 0.2 % at a time (another scale), until the mean is below BIAS_MAX."""
    sigma = float(np.std(np.asarray(a, np.float64)))
    lo, hi = (r * sigma for r in RANGES[which])
    body = np.clip(rng.laplace(0.0, sigma / np.sqrt(2.0), a.shape), lo, hi)
    i, j = rng.choice(body.size, 2, replace=False)
    for f in NARROW:
        out = body.copy()
        out.flat[i], out.flat[j] = (lo * f, hi) if which == "low" else (lo, hi * f)
        out = np.clip(out, out.flat[i], out.flat[j]).astype(np.float32)
        q, s, o = ggml.quantize(out, np.uint16 if ggml.is_u16(name) else np.uint8)
        bias = np.mean(ggml.dequantize(q, s, o).astype(np.float64) - (q.astype(np.float64) * float(s) + float(o)))
        if abs(bias) <= BIAS_MAX * sigma:
            return out
    raise AssertionError(f"{name}: no outlier within {NARROW[-1]} .. 1 of its place leaves the definition's rounding unbiased")


def skewed_weights(ggml, weights, families=ALL, seed=0):
    """ggml.synth_weights -> the same with the matrices of `families` (a subset of FAMILIES) rewritten per variant(); everything else,
    and every tensor of CONTROL_TARGET, keeps its synthetic values.  ggml: the package's file module (its quantiser, unchanged)."""
    families = frozenset(families)
    assert families <= ALL, families
    rng = np.random.default_rng(seed)
    out = []
    for t, d in enumerate(weights):
        e = dict(d)
        for name, a in d.items():
            v = variant(t, name)
            if v is not None and family(name) in families:
                e[name] = skew_matrix(ggml, name, a, v, rng)
        out.append(e)
    return out


# name -> (hidden, seed of ggml.synth_weights, skewed families, seed of the redraw): every model of tests/test_gpu_affine_offset.py
FIXTURES = {
    "h128_all": (128, 3, ALL, 5),
    "h128_hh": (128, 3, frozenset({"hh"}), 6),
    "h512_all": (512, 81, ALL, 9),  # 256 x 256 tiles (W_ih, fc3) and lstm_batch8_kernel at K = 256; also the bitwise comparison of the flavours
    "h1024_all": (1024, 81, ALL, 9),  # UMX-L's width: lstm_batch8_kernel at K = 512
    "h512_hh": (512, 81, frozenset({"hh"}), 9),  # only W_hh skewed: the batched recurrences' own offset term (centre 128) at its real K
    "h1024_hh": (1024, 81, frozenset({"hh"}), 9),
}


def make_fixture(ggml, name, directory):
    """Write fixture `name` in the reference's file format under `directory`, read it back, assert its sharpness.
    -> (hidden, skewed families, ggml.read_model's targets)."""
    H, seed, fams, seed_skew = FIXTURES[name]
    path = str(directory / f"skewed_{name}.bin")
    ggml.write_model(path, skewed_weights(ggml, ggml.synth_weights(H, seed=seed), fams, seed_skew), H, compress=False)
    hidden, targets = ggml.read_model(path)
    assert hidden == H
    assert_sharp(targets, fams)
    return H, fams, targets


def zero_code_distance(rec):
    """Codes between the zero-weight code -o / s of a file tensor (ggml.read_model record) and the fixed centre of its type."""
    s, o = float(rec["scale"]), float(rec["offset"])
    c = U16_CENTRE if rec["q"].dtype == np.uint16 else U8_CENTRE
    return abs(o + c * s) / s


def assert_sharp(targets, families=ALL):
    """Every skewed tensor of the file (ggml.read_model's targets) has its zero-weight code a quarter of the code range from the fixed
    centre; the control target's matrices stay within two codes of it (which is why the plain fixtures are blind).  The two LSTM
    directions of every layer carry different variants."""
    for t, d in enumerate(targets):
        for name, rec in d.items():
            fam = family(name)
            if fam is None:
                continue
            dist = zero_code_distance(rec)
            u16 = rec["q"].dtype == np.uint16
            if t != CONTROL_TARGET and fam in families:
                assert dist >= (SHARP_U16 if u16 else SHARP_U8), (t, name, dist)
                if name.startswith("lstm.") and not name.endswith("_reverse"):
                    assert variant(t, name) != variant(t, name + "_reverse"), (t, name)
            else:
                assert dist <= (2.0 * 257 if u16 else 2.0), (t, name, dist)


def target_weights_exact(file_target):
    """One target of ggml.read_model -> name -> float64 q s + o for the five matrix families (the map the kernels apply to the sum),
    the file's dequantised float32 tensor for everything else."""
    out = {}
    for k, v in file_target.items():
        if family(k) is None:
            out[k] = v["f32"]
        else:
            out[k] = v["q"].astype(np.float64) * float(v["scale"]) + float(v["offset"])
    return out


# ---------------------------------------------------------------- one stage: both float64 references, the yardstick, the gap
STAGE_KIND = "rows"


def stage_refs(file_target, stage_fn):
    """stage_fn(weights, precision) -> (float64 with exact-affine matrices, the definition's float64, the definition's float32)."""
    wd, we = sf.target_weights(file_target), target_weights_exact(file_target)
    return stage_fn(we, "float64"), stage_fn(wd, "float64"), stage_fn(wd, "float32")


def check_both(stage, got, exact64, def64, def32, *, where="", T=None, no_gap=False):
    """The two comparisons of one stage -> two rows of stage_f64.check (its C_DEFAULT, FLOOR and yardstick caps, unchanged).
    "<stage> arithmetic": `got` against the float64 evaluation with exact-affine matrices.
    "<stage> parity": `got` against the definition's float64, the bound raised by the definition gap of this stage on these
    activations (no_gap: no allowance -- the per-weight form of UMX_CREATE_U8_DEQUANT).
    The yardstick of both is the definition's float32 evaluation against the definition's float64.  Each row also carries the gap
    and fails if the gap itself is past GAP_BOUND."""
    gap_rel, gap_blk, _ = sf.distances(exact64, def64, STAGE_KIND)
    rows = [sf.check(f"{stage} arithmetic", got, exact64, def32, STAGE_KIND, where=where, T=T, yard64=def64),
            sf.check(f"{stage} parity", got, def64, def32, STAGE_KIND, where=where, T=T, gap=(0.0, 0.0) if no_gap else (gap_rel, gap_blk))]
    for r in rows:  # the fixture's own condition on these activations, in the same row
        r["gap_rel"], r["gap_blk"], r["gap_ok"] = gap_rel, gap_blk, bool(gap_rel < GAP_BOUND and gap_blk < GAP_BOUND)
        if not r["gap_ok"] and r["failure"] is None:
            r["failure"] = f"{r['stage']} {where}: definition gap {gap_rel:.3e} / {gap_blk:.3e} past {GAP_BOUND:g}: the fixture is not one here"
    return rows


def stage_functions(H, x, a1, lo, a2, state):
    """name -> (weights, precision) -> stage output, from the inputs of each stage (engine taps, or cpu_activations)."""
    return {"fc1": lambda w, p: sf.fc1(w, x, p), "lstm": lambda w, p: sf.lstm(w, H, a1, state, p),
            "fc2": lambda w, p: sf.fc2(w, a1, lo, p), "mask": lambda w, p: sf.mask(w, a2, p)}


def cpu_activations(ggml, file_target, H, T=64, seed=11, level=1.0):
    """The inputs of every stage of one target without a GPU: x from the float32 STFT of T frames of ggml.synth_audio, then each
    stage's float64 evaluation (exact-affine matrices) rounded to float32, as the engine's taps are.  -> (x, a1, lo, a2, state)."""
    N = (T - 1) * sf.HOP
    wave = ggml.synth_audio(N, seed) * np.float32(level)
    x = sf.crop_x(sf.magnitude(sf.stft(wave, N, "float32"), "float32")).astype(np.float32)
    we = target_weights_exact(file_target)
    state = np.zeros(12 * (H // 2), np.float32)
    a1 = sf.fc1(we, x, "float64").astype(np.float32)
    lo = sf.lstm(we, H, a1, state, "float64").astype(np.float32)
    a2 = sf.fc2(we, a1, lo, "float64").astype(np.float32)
    return x, a1, lo, a2, state


def definition_gaps(file_target, fns):
    """stage -> (whole segment, worst block): the distance between the float64 evaluations with dequantised fp32 and with exact-affine
    matrices."""
    wd, we = sf.target_weights(file_target), target_weights_exact(file_target)
    return {k: sf.distances(f(we, "float64"), f(wd, "float64"), STAGE_KIND)[:2] for k, f in fns.items()}


def assert_gaps(gaps, where=""):
    for k, (rel, blk) in gaps.items():
        assert rel < GAP_BOUND and blk < GAP_BOUND, (where, k, rel, blk)


# ---------------------------------------------------------------- the products as the kernels form them, in numpy
FORMS = ("fixed", "recentred_f32", "recentred_f64")


def centre_and_o2(s, o, u16, form):
    """(c, o2 = o + c s as float32) of one file tensor.  "fixed": c = 128 / 32896, fp32.  "recentred_f32": c = the code nearest -o / s
    (0 .. 255, or 31 .. 65504 so that |q - c| <= 65504), the sum formed in fp32.  "recentred_f64": that c, the sum formed in double."""
    s32, o32 = np.float32(s), np.float32(o)
    fixed = U16_CENTRE if u16 else U8_CENTRE
    if form == "fixed" or not (np.isfinite(s32) and s32 != 0):
        return fixed, np.float32(o32 + np.float32(np.float32(fixed) * s32))
    c = int(np.clip(np.rint(-float(o32) / float(s32)), *((31, 65504) if u16 else (0, 255))))
    if form == "recentred_f32":
        return c, np.float32(o32 + np.float32(np.float32(c) * s32))
    assert form == "recentred_f64", form
    return c, np.float32(float(o32) + float(c) * float(s32))


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _lane_rowsum(a):
    """fp32 row sums the way a wave forms them: 64 lanes add every 64th element in turn, then a butterfly over the lanes."""
    M, K = a.shape
    p = np.zeros((M, -(-K // 64) * 64), np.float32)
    p[:, :K] = a
    p = p.reshape(M, -1, 64)
    acc = np.zeros((M, 64), np.float32)
    for i in range(p.shape[1]):
        acc = (acc + p[:, i]).astype(np.float32)
    n = 64
    while n > 1:
        n //= 2
        acc = (acc[:, :n] + acc[:, n:2 * n]).astype(np.float32)
    return acc[:, 0]


def plane_product(a, q, s, o, form, *, fixed_exp=None, kstep=16, ones_rowsum=False, a_parts=None):
    """a (M, K) float32 times the file tensor (q (N, K) u8 / u16, s, o) -> (M, N) float32, as the plane kernels form it:
    the row scaled by a power of two (its maximum into [2^14, 2^15), or 2^fixed_exp), two fp16 planes a1 + a2; q - c exact in one
    fp16 plane (u8) or two (u16: fp16(q - c) and the remainder; a2 x remainder is not formed); every product exact, each matrix
    instruction's `kstep` products added to an fp32 accumulator with one rounding; then s 2^-e acc + o2 rowsum with one rounding.
    The row sum is fp32 (a_parts: the sums of these column ranges added in turn, a concatenated A), or with ones_rowsum the
    accumulated products of a1 + a2 with a plane of ones (the recurrences)."""
    a = np.asarray(a, np.float32)
    u16 = q.dtype == np.uint16
    c, o2 = centre_and_o2(s, o, u16, form)
    M, K = a.shape
    if fixed_exp is None:
        mx = np.abs(a).max(axis=1)
        e = np.where(mx > 0, 14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 0.0)
    else:
        e = np.full(M, float(fixed_exp))
    ap = (a.astype(np.float64) * np.exp2(e)[:, None]).astype(np.float32)  # exact
    a1 = _f16(ap)
    a2 = _f16(ap - a1)
    P = q.astype(np.float64) - c
    if u16:
        Phi = _f16(P).astype(np.float64)
        terms = ((a2, Phi), (a1, P - Phi), (a1, Phi))
        assert np.abs(P - Phi).max() <= 16
    else:
        terms = ((a1, P), (a2, P))
    acc = np.zeros((M, q.shape[0]), np.float32)
    ones = np.zeros((M, 1), np.float32)
    for k0 in range(0, K, kstep):
        for x, p in terms:
            acc = (acc.astype(np.float64) + x[:, k0:k0 + kstep].astype(np.float64) @ p[:, k0:k0 + kstep].T).astype(np.float32)
        if ones_rowsum:
            for x in (a1, a2):
                ones = (ones.astype(np.float64) + x[:, k0:k0 + kstep].astype(np.float64).sum(axis=1, keepdims=True)).astype(np.float32)
    unscale = np.exp2(-e)
    if ones_rowsum:
        rs = ones[:, 0].astype(np.float64) * unscale  # the power of two comes back out with the offset term
    else:
        parts = a_parts or ((0, K),)
        rs = _lane_rowsum(a[:, parts[0][0]:parts[0][1]])
        for lo_, hi_ in parts[1:]:
            rs = (rs + _lane_rowsum(a[:, lo_:hi_])).astype(np.float32)
        rs = rs.astype(np.float64)
    add = (float(o2) * rs).astype(np.float32).astype(np.float64)
    mul = float(np.float32(s)) * unscale
    return (mul[:, None] * acc.astype(np.float64) + add[:, None]).astype(np.float32)


def _bn64(wt, y, name):
    f = lambda k: np.asarray(wt[name + "." + k], np.float64)
    return (y - f("running_mean")) / np.sqrt(f("running_var") + 1e-5) * f("weight") + f("bias")


def emulated_stages(file_target, H, x, a1, lo, a2, state, form):
    """fc1, lstm, fc2 and mask of one target with every quantised product formed by plane_product under `form`, everything around
    the products in float64, each output rounded to float32."""
    ft = file_target
    wd = sf.target_weights(ft)
    rec = lambda n: (ft[n]["q"], ft[n]["scale"], ft[n]["offset"])
    out = {}
    xs = (np.asarray(x, np.float32) * np.tile(wd["input_scale"], 2) + np.tile(wd["input_mean"], 2)).astype(np.float32)
    out["fc1"] = np.tanh(_bn64(wd, plane_product(xs, *rec("fc1.weight"), form).astype(np.float64), "bn1")).astype(np.float32)
    # the BiLSTM: W_ih through the plane GEMM (inputs bounded by 1: the constant scale 2^14), W_hh per step against the two planes of
    # h 2^14, the row sum out of a tile of ones
    Hl = H // 2
    st = np.asarray(state, np.float64).reshape(3, 2, 2, Hl)
    inp = np.asarray(a1, np.float32)
    T = inp.shape[0]
    for layer in range(3):
        nxt = np.empty((T, H), np.float32)
        for d, sfx in enumerate(("", "_reverse")):
            n = f"_l{layer}{sfx}"
            P = plane_product(inp, *rec("lstm.weight_ih" + n), form, fixed_exp=14,
                              a_parts=None if layer == 0 else ((0, Hl), (Hl, H))).astype(np.float64) + np.asarray(wd["lstm.bias_ih" + n], np.float64)
            bhh = np.asarray(wd["lstm.bias_hh" + n], np.float64)
            h, c = st[layer, d, 0].astype(np.float32), st[layer, d, 1].copy()
            for step in range(T):
                t = step if d == 0 else T - 1 - step
                g = P[t] + plane_product(h[None, :], *rec("lstm.weight_hh" + n), form, fixed_exp=14, kstep=32, ones_rowsum=True)[0] + bhh
                c = sf.gate_ref("sigmoid", g[Hl:2 * Hl]) * c + sf.gate_ref("sigmoid", g[:Hl]) * np.tanh(g[2 * Hl:3 * Hl])
                h = (sf.gate_ref("sigmoid", g[3 * Hl:]) * np.tanh(c)).astype(np.float32)
                nxt[t, d * Hl:(d + 1) * Hl] = h
        inp = nxt
    out["lstm"] = inp
    cat = np.concatenate([np.asarray(a1, np.float32), np.asarray(lo, np.float32)], axis=1)
    y = plane_product(cat, *rec("fc2.weight"), form, fixed_exp=14, a_parts=((0, H), (H, 2 * H))).astype(np.float64)
    out["fc2"] = np.maximum(_bn64(wd, y, "bn2"), 0.0).astype(np.float32)
    y = _bn64(wd, plane_product(a2, *rec("fc3.weight"), form).astype(np.float64), "bn3")
    out["mask"] = np.maximum(y * np.tile(np.asarray(wd["output_scale"], np.float64), 2) + np.tile(np.asarray(wd["output_mean"], np.float64), 2), 0.0).astype(np.float32)
    return out
