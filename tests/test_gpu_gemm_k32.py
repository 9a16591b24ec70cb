"""The plane GEMMs on v_mfma_f32_16x16x32_f16 (csrc/gemm_planes.h, gemm_planes_pp.h, gemm_planes_ps.h; GP_MFMA_K32): every lane, register
and block of the new fragment reads, products and lane swaps lands where the 32x32x16 form put it.

  * Position.  A model whose fc1 is a SELECTION: output column n has one nonzero weight code, 2^(n % 8), at input k_n (all k_n
    different, spread over every K tile and every 16-byte chunk of a tile), scale 1 and offset 0, so that the affine map's second term is
    0 x rowsum; input_scale 2^-40, input_mean 0, bn1 the identity (running_var + 1e-5 == 1 in float32).  Then every step from the x tap
    to the fc1 tap is exact in float32 and numpy restates it bit for bit: the row's power-of-two scale, the split into two fp16 planes
    a1 + a2 (csrc/gemm_planes.h split2_f16), the products a2 w and a1 w and their sum (w a power of two: no rounding), the scale back,
    and tanh_epi, which returns x itself below |x| = 2^-13 (its polynomial's correction is below half an ulp of 1).  Rows are spectra of
    different audio, columns differ in k and in weight: a wrong lane, register, block or k chunk is a wrong value, not noise.  The
    fc1 tap must EQUAL the restatement, element for element, on each kernel at the smallest shape that reaches it (engine_stages.h:
    256 x 256 tiles from 224 tiles per launch on, the persistent kernel from more tiles than workgroups on):
      - hidden 128, one lane, T = 5 and T = 130: gemm_planes_kernel, 128 x 128 tiles (two row tiles, the second with 2 valid rows);
      - hidden 256, 56 lanes, T = 300 (lanes follow each other every 300 rows, so the 66 row tiles of 256 straddle them; 264 tiles for
        fc1's four targets): gemm_planes_kernel at 256 x 256 (UMX_GEMM_PP=0), gemm_planes_pp_kernel (UMX_GEMM_PS=0) and
        gemm_planes_ps_kernel, where 264 tiles on 256 workgroups make eight workgroups run a second tile: the first trip with the
        previous tile's epilogue beside the first term.
  * One u16 stage on the three-product form (a2 P_hi, a1 P_lo, a1 P_hi): hidden 256, four lanes, T = 300 -- fc2 on gemm_planes_kernel
    (128 x 128) and the mask on gemm_planes_ps_kernel / gemm_planes_pp_kernel (340 tiles) -- against the float64 evaluation within the
    bounds of tests/stage_f64.py, unchanged, on a lane whose rows share tiles with both neighbours.
"""
import numpy as np
import pytest

import stage_f64 as sf
import test_gpu_affine_offset as aff
import test_gpu_geometry_f64 as geo

pytestmark = pytest.mark.gpu

NIN = 2 * sf.CROP
X_SCALE = np.float32(2.0 ** -40)
LOCK, PP, PS = "gemm_planes_kernel", "gemm_planes_pp_kernel", "gemm_planes_ps_kernel"


def _const(n, value, like):
    """A file tensor whose every element dequantises to `value` exactly: code 0, offset = value."""
    return dict(q=np.zeros(n, like.dtype), scale=np.float32(1.0), offset=np.float32(value), f32=np.full(n, value, np.float32))


def selection_columns(hidden):
    n = np.arange(hidden)
    k = (37 * n + 5) % NIN  # 37 and 2974 = 2 x 1487 are coprime: all different
    assert len(set(k.tolist())) == hidden and set((k % 32 // 8).tolist()) == {0, 1, 2, 3} and k.max() >= NIN - 32
    return k, (1 << (n % 8)).astype(np.uint8)


def selection_model(pkg, tmp_path, hidden):
    """File tensors of ggml.synth_weights with fc1 turned into the selection of the module docstring (all four targets)."""
    path = str(tmp_path / f"sel{hidden}.bin")
    pkg.ggml.write_model(path, pkg.ggml.synth_weights(hidden, seed=61), hidden, compress=False)
    _, targets = pkg.ggml.read_model(path)
    k, w = selection_columns(hidden)
    codes = np.zeros((hidden, NIN), np.uint8)
    codes[np.arange(hidden), k] = w
    var = np.float32(1.0) - np.float32(1e-5)
    while np.float32(var + np.float32(1e-5)) != np.float32(1.0):
        var = np.nextafter(var, np.float32(2.0), dtype=np.float32)
    out = []
    for d in targets:
        d = dict(d)
        d["fc1.weight"] = dict(q=codes, scale=np.float32(1.0), offset=np.float32(0.0), f32=codes.astype(np.float32))
        d["input_scale"] = _const(sf.CROP, X_SCALE, d["input_scale"]["q"])
        d["input_mean"] = _const(sf.CROP, 0.0, d["input_mean"]["q"])
        d["bn1.running_mean"] = _const(hidden, 0.0, d["bn1.running_mean"]["q"])
        d["bn1.running_var"] = _const(hidden, var, d["bn1.running_var"]["q"])
        d["bn1.weight"] = _const(hidden, 1.0, d["bn1.weight"]["q"])
        d["bn1.bias"] = _const(hidden, 0.0, d["bn1.bias"]["q"])
        out.append(d)
    return out


def fc1_restated(x, hidden):
    """x tap (T, >= 2974) -> what fc1 of the selection model holds, every step exact in float32 (asserted in float64)."""
    k, w = selection_columns(hidden)
    xs = x[:, :NIN].astype(np.float32) * X_SCALE
    mx = np.abs(xs).max(axis=1)
    assert (mx > 0).all()
    e = 15 - np.frexp(mx)[1]  # split_planes_shared_kernel: the row's largest element into [2^14, 2^15)
    v = np.ldexp(xs, e[:, None]).astype(np.float32)
    assert (np.ldexp(v.astype(np.float64), -e[:, None]) == xs).all() and 2.0 ** 14 <= np.abs(v).max() < 2.0 ** 15
    a1 = v.astype(np.float16)
    a2 = (v - a1.astype(np.float32)).astype(np.float16)
    s = a1.astype(np.float64) + a2.astype(np.float64)
    y = np.ldexp(s[:, k] * w[None, :].astype(np.float64), -e[:, None])
    y32 = y.astype(np.float32)
    assert (y32.astype(np.float64) == y).all() and (np.abs(y32) < 2.0 ** -13).all()  # exact, and tanh_epi(y) == y
    assert (s == (a1.astype(np.float32) + a2.astype(np.float32)).astype(np.float64)).all()  # w (a1 + a2) is one float32: no rounding in the accumulator
    return y32


@pytest.fixture(scope="module")
def lane_audio(pkg):
    """56 lanes of different audio from four draws (rolled by a lane's own offset), 300 frames."""
    N = sf._N(300, 517)
    base = [pkg.ggml.synth_audio(N, 4100 + i) for i in range(4)]
    return N, [np.ascontiguousarray(np.roll(base[b % 4], 4099 * b, axis=1)[:, :N - 7 * b]) for b in range(56)]


def _assert_positions(eng, hidden, lanes):
    T = eng.T
    for b in lanes:
        sfx = geo._sfx(eng, b)
        want = fc1_restated(eng.tap("x" + sfx), hidden)
        assert want.shape == (T, hidden)
        for t in range(4):
            got = eng.tap("fc1" + sfx, t)
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (f"lane {b}, target {t}: {len(bad)} of {got.size} elements differ, first at (frame, column) "
                                   f"{bad[0].tolist()}: {got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("T", [5, 130])
def test_positions_on_the_128_wide_lock_step_kernel(pkg, tmp_path, monkeypatch, T):
    for name in ("UMX_GEMM_PP", "UMX_GEMM_PS"):
        monkeypatch.delenv(name, raising=False)
    H, N = 128, sf.N_MIN if T == 5 else sf._N(T, 517)
    eng = pkg.Engine(selection_model(pkg, tmp_path, H), H, N, tracks=1, lstm_batched=True, gemm="planes")
    try:
        assert eng.T == T
        geo._run(pkg, eng, [geo._audio(pkg, N, 4000)], 0)
        assert eng.gemm_kernel_name(0) == LOCK, eng.gemm_kernel_name(0)
        _assert_positions(eng, H, [0])
    finally:
        eng.close()


@pytest.fixture(scope="module")
def selection_256(pkg, tmp_path_factory):
    return selection_model(pkg, tmp_path_factory.mktemp("k32_selection"), 256)


@pytest.mark.parametrize("env,kernel", [({"UMX_GEMM_PP": "0"}, LOCK), ({"UMX_GEMM_PS": "0"}, PP), ({}, PS)],
                         ids=["lock_step_256", "ping_pong", "persistent"])
def test_positions_on_the_256_wide_kernels(pkg, selection_256, lane_audio, monkeypatch, env, kernel):
    for name in ("UMX_GEMM_PP", "UMX_GEMM_PS"):
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)
    H, B = 256, 56
    N, waves = lane_audio
    eng = pkg.Engine(selection_256, H, N, tracks=B)
    try:
        assert eng.T == 300 and -(-B * eng.T // 256) * 4 > 256  # 66 row tiles x 4 targets: more tiles than workgroups
        geo._run(pkg, eng, waves, 0)
        assert eng.gemm_kernel_name(0) == kernel, eng.gemm_kernel_name(0)
        # lane 0 (rows 0 .. 299), lanes whose rows share 256-row tiles with both neighbours, the last lane (the M padding behind it)
        _assert_positions(eng, H, [0, 1, 27, 54, 55])
    finally:
        eng.close()


@pytest.mark.parametrize("env,fc3_kernel", [({}, PS), ({"UMX_GEMM_PS": "0"}, PP)], ids=["persistent", "ping_pong"])
def test_u16_stages_on_the_three_product_form_against_float64(pkg, tmp_path, lane_audio, monkeypatch, env, fc3_kernel):
    for name in ("UMX_GEMM_PP", "UMX_GEMM_PS"):
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)
    H, B = 256, 4
    N, waves = lane_audio
    path = str(tmp_path / "m256.bin")
    pkg.ggml.write_model(path, pkg.ggml.synth_weights(H, seed=67), H, compress=False)
    _, targets = pkg.ggml.read_model(path)
    rep = sf.Report()
    eng = pkg.Engine(targets, H, N, tracks=B)
    try:
        state = aff._zero_state(eng)
        geo._run(pkg, eng, waves[:B], 0)
        names = [eng.gemm_kernel_name(m) for m in range(4)]
        assert names[2] == LOCK and names[3] == fc3_kernel, names
        for lane in (1, 3):
            geo.check_network(rep, eng, lane, targets, state, f"k32 u16 stages, fc3 on {fc3_kernel}", which=(0, 3))
    finally:
        eng.close()
    for r in rep.rows:
        if r["stage"].split("[")[0] in ("fc2", "mask"):
            print({k: r[k] for k in ("stage", "ratio_rel", "ratio_blk") if k in r})
    geo._finish(rep, f"k32_u16_{fc3_kernel}")
