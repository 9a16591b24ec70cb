"""The write contract of the device entry points (include/umx_hip.h): a call with n samples writes exactly out[t][0 .. 2n) of the
caller's buffers and reads exactly audio[0 .. 2n).  Every caller buffer is a guarded allocation of tests/guarded.py -- NaN guards on
both sides of a payload of exactly the contract's size, the post-guard past the furthest store any kernel could issue -- and every
result is compared bit for bit with a twin engine (same weights, the same sequence of calls) through the host form, whose stems go
to the engine's own full-length buffers.  A store past n lands in a guard; a read past n brings a NaN into the twin comparison.

  (a) umx_hip_infer_batch_device on track contexts (the fused Wiener / inverse STFT kernel), n at run boundaries, in a run's first
      blocks, whole hop blocks short, an idle lane; every flag that reaches a different writer; once more under UMX_WIENER=stats4
  (b) umx_hip_infer_segment_device, (c) the phased _device calls, both under stats4 and fused
  (d) the host-async form on guarded pinned host buffers (the copy stream's download)
  (e) in all of them the audio is guarded as well and must come back unchanged
  (f) the track kernels (umx_hip_weight_stems_device, _track_accumulate_device, _track_normalise_device) against a float32 numpy
      restatement of csrc/track_kernels.h
  (g) the multi-GPU driver at world 1 under UMX_WIENER=fused: its last segment's stems are exact-size neighbours in one arena"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import guarded as gd  # noqa: E402
import stage_f64 as sf  # noqa: E402

pytestmark = pytest.mark.gpu
HOP = gd.HOP


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engines' streams exist
    return t


@pytest.fixture(scope="module")
def n_cus(torch):
    n = sf.device_cu_count()
    assert n == torch.cuda.get_device_properties(0).multi_processor_count
    return n


_AUDIO = {}


def _audio(n, k):
    """(2,n) of seeded music-like audio, a different stretch for every k."""
    if "a" not in _AUDIO:
        import __graft_entry__ as ge
        _AUDIO["a"] = ge.load_package().ggml.synth_audio(3 * 200 * HOP, 4242)
    a = _AUDIO["a"]
    s = (k * 7919 * 37) % (a.shape[1] - n + 1)
    return np.ascontiguousarray(a[:, s:s + n])


def _inter(x):
    """(2,n) -> the interleaved float32 words of the C-ABI."""
    return np.ascontiguousarray(np.asarray(x, np.float32).T).ravel()


class Buf:
    """One guarded buffer in its own allocation: device memory, or pinned host memory (pinned=True)."""

    def __init__(self, torch, layout, data=None, pinned=False):
        self.layout = layout
        self.before = gd.make(layout, data)
        src = torch.from_numpy(self.before)
        if pinned:
            self.t = torch.empty(layout.total, dtype=torch.int32, pin_memory=True)
            self.t.copy_(src)
        else:
            self.t = src.cuda()
        assert self.t.data_ptr() % 256 == 0
        self.words = None

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.layout.pre

    def read(self):
        self.words = self.t.cpu().numpy()
        return self.words

    def report(self, expect=None):
        return gd.check(self.read(), self.layout, expect)

    def values(self):
        return gd.payload(self.words, self.layout)


def _lane(torch, wave, N, misalign, pinned=False):
    """Guarded audio (the wave) and four guarded outputs of 2n floats; the outputs alternate between the two alignments."""
    n = wave.shape[1]
    a = Buf(torch, gd.stem_layout(n, N, misalign), _inter(wave), pinned)
    outs = [Buf(torch, gd.stem_layout(n, N, 8 * ((misalign // 8 + t) % 2)), None, pinned) for t in range(4)]
    return a, outs


def _assert_lane(what, a, outs, ref):
    """The audio untouched, every output guard untouched and every payload word written with the twin's bits."""
    r = a.report(a.before)
    assert r.ok, (what, "audio", str(r))
    for t in range(4):
        r = outs[t].report()
        assert r.ok, (what, "stem", t, str(r))
        got, want = outs[t].values().view(np.int32), _inter(ref[t]).view(np.int32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, "stem", t, "differs from the host form at words", bad[:4], bad.size)


def _sync(torch, *engines):
    for e in engines:
        e.sync()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- (a) the batched device form on track contexts
FLAG_SETS = {"wiener": 0, "no_wiener": 0x1, "em3": 3 << 16, "skip12": (0x100 << 1) | (0x100 << 2)}


def _batch_calls(N, lanes, n_cus):
    """Per call, the n of every lane (None: the lane sits out): ragged_ns dealt over the lanes, then a call whose middle lane sits
    out while the others are one sample long and one short of N."""
    ns = gd.ragged_ns(N, *sf.fused_run_split(gd.n_frames(N), lanes, n_cus))
    calls = gd.lanes_of(ns, lanes)
    idle = [N - 1] * lanes
    idle[0], idle[lanes // 2] = 1, None
    calls.append(idle)
    assert any(c[i] is not None and c[i] <= N - 2 * HOP for c in calls for i in range(lanes))  # whole hop blocks past n
    return calls


def _run_batch_calls(torch, pkg, eng, twin, N, lanes, calls, flags, what):
    for ci, ns in enumerate(calls):
        waves = [None if n is None else _audio(n, 1000 * ci + i) for i, n in enumerate(ns)]
        bufs = [None if w is None else _lane(torch, w, N, 8 * ((i + ci) % 2)) for i, w in enumerate(waves)]
        # a lane that sits out gets guarded outputs too: nothing of them may change
        idle = {i: [Buf(torch, gd.stem_layout(HOP, N)) for _ in range(4)] for i, w in enumerate(waves) if w is None}
        out_ptrs = []
        for i in range(lanes):
            out_ptrs += [o.ptr for o in (idle[i] if i in idle else bufs[i][1])]
        torch.cuda.synchronize()
        eng.infer_batch_ptrs([0 if b is None else b[0].ptr for b in bufs], [0 if n is None else n for n in ns], out_ptrs, flags)
        _sync(torch, eng)
        ref = twin.infer_batch(waves, flags)
        for i in range(lanes):
            if i in idle:
                for t, o in enumerate(idle[i]):
                    assert gd.untouched(o.read(), o.before) is None, (what, ci, "idle lane", i, t)
            else:
                _assert_lane((what, ci, "lane", i, "n", ns[i]), bufs[i][0], bufs[i][1], ref[i])


@pytest.mark.parametrize("ctx", list(gd.BATCH_CONTEXTS))
def test_batched_device_form_writes_exactly_n_per_lane(pkg, model_small, torch, n_cus, ctx, monkeypatch):
    """Track contexts run the fused Wiener / inverse STFT kernel by default: wiener_istft_kernel<true> (flags 0), <false>
    (FLAG_NO_WIENER), wiener_istft_v_kernel (three EM iterations), the skipped targets' zero-filled magnitudes; each with
    wiener_ola_edges_kernel behind it."""
    monkeypatch.delenv("UMX_WIENER", raising=False)
    _, _, targets = model_small
    N, lanes = gd.BATCH_CONTEXTS[ctx]
    calls = _batch_calls(N, lanes, n_cus)
    eng, twin = pkg.Engine(targets, 128, N, tracks=lanes), pkg.Engine(targets, 128, N, tracks=lanes)
    try:
        for name, flags in FLAG_SETS.items():
            _run_batch_calls(torch, pkg, eng, twin, N, lanes, calls, flags, (ctx, name))
    finally:
        eng.close()
        twin.close()


def test_batched_device_form_under_the_unfused_kernels(pkg, model_small, torch, n_cus, monkeypatch):
    """The same calls with UMX_WIENER=stats4 on a track context: wiener_apply_kernel, istft_frames_kernel and istft_ola_kernel on
    batched lanes (and mixphase_kernel for FLAG_NO_WIENER)."""
    monkeypatch.setenv("UMX_WIENER", "stats4")
    _, _, targets = model_small
    N, lanes = gd.BATCH_CONTEXTS["T201x3"]
    calls = _batch_calls(N, lanes, n_cus)
    eng, twin = pkg.Engine(targets, 128, N, tracks=lanes), pkg.Engine(targets, 128, N, tracks=lanes)
    try:
        for name in ("wiener", "no_wiener"):
            _run_batch_calls(torch, pkg, eng, twin, N, lanes, calls, FLAG_SETS[name], ("stats4", name))
    finally:
        eng.close()
        twin.close()


# ---------------------------------------------------------------- (b) one track, (c) phase by phase, (d) host-async
def _single_ns(n_cus):
    N = gd.SINGLE_N
    return N, gd.ragged_ns(N, *sf.fused_run_split(gd.n_frames(N), 1, n_cus))


@pytest.mark.parametrize("mode", ["stats4", "fused"])
def test_single_track_device_form_writes_exactly_n(pkg, model_small, torch, n_cus, mode, monkeypatch):
    monkeypatch.setenv("UMX_WIENER", mode)
    _, _, targets = model_small
    N, ns = _single_ns(n_cus)
    eng, twin = pkg.Engine(targets, 128, N), pkg.Engine(targets, 128, N)
    try:
        for k, n in enumerate(ns):
            wave = _audio(n, 50 + k)
            a, outs = _lane(torch, wave, N, 8 * (k % 2))
            torch.cuda.synchronize()
            eng.infer_segment_device(a.ptr, n, [o.ptr for o in outs])
            _sync(torch, eng)
            _assert_lane((mode, "n", n), a, outs, twin.infer_segment(wave))
    finally:
        eng.close()
        twin.close()


@pytest.mark.parametrize("mode", ["stats4", "fused"])
@pytest.mark.parametrize("back", ["end", "masks_finish"])
def test_phased_device_calls_write_exactly_n(pkg, model_small, torch, n_cus, mode, back, monkeypatch):
    """segment_begin_device -> segment_lstm_layer x 3 -> segment_end_device, or segment_masks_device + segment_finish_device, against
    the host phased form."""
    monkeypatch.setenv("UMX_WIENER", mode)
    _, _, targets = model_small
    N = gd.SINGLE_N
    run_len = sf.fused_run_split(gd.n_frames(N), 1, n_cus)[0]
    # the last sample short, an end at run 1's first block and one past it, inside run 2's first blocks, whole hop blocks short
    pick = [N - 1, run_len * HOP - 2048, run_len * HOP - 2047, 2 * run_len * HOP - 2048 + HOP + 517, 1025, 1]
    eng, twin = pkg.Engine(targets, 128, N), pkg.Engine(targets, 128, N)
    try:
        for k, n in enumerate(pick):
            wave = _audio(n, 80 + k)
            a, outs = _lane(torch, wave, N, 8 * (k % 2))
            torch.cuda.synchronize()
            eng.segment_begin_device(a.ptr, n)
            for layer in range(3):
                eng.segment_lstm_layer(layer)
            if back == "end":
                eng.segment_end_device([o.ptr for o in outs])
            else:
                eng.segment_masks_device()
                eng.segment_finish_device([o.ptr for o in outs])
            _sync(torch, eng)
            twin.segment_begin(wave)
            for layer in range(3):
                twin.segment_lstm_layer(layer)
            _assert_lane((mode, back, "n", n), a, outs, twin.segment_end())
    finally:
        eng.close()
        twin.close()


@pytest.mark.parametrize("lanes", [1, 3])
def test_host_async_form_on_pinned_buffers_writes_exactly_n(pkg, model_small, torch, n_cus, lanes, monkeypatch):
    """umx_hip_infer_batch_async: the upload from and the copy stream's download into guarded pinned host buffers of 2n floats."""
    monkeypatch.delenv("UMX_WIENER", raising=False)
    _, _, targets = model_small
    N = gd.SINGLE_N
    ns = gd.ragged_ns(N, *sf.fused_run_split(gd.n_frames(N), lanes, n_cus))
    eng, twin = pkg.Engine(targets, 128, N, tracks=lanes), pkg.Engine(targets, 128, N, tracks=lanes)
    try:
        for ci, cn in enumerate(gd.lanes_of(ns, lanes)):
            waves = [_audio(n, 300 + 10 * ci + i) for i, n in enumerate(cn)]
            bufs = [_lane(torch, w, N, 8 * ((i + ci) % 2), pinned=True) for i, w in enumerate(waves)]
            eng.infer_batch_ptrs([b[0].ptr for b in bufs], cn, [o.ptr for b in bufs for o in b[1]], 0, where="host_async")
            _sync(torch, eng)
            ref = twin.infer_batch(waves)
            for i in range(lanes):
                _assert_lane(("host_async", ci, i, "n", cn[i]), bufs[i][0], bufs[i][1], ref[i])
    finally:
        eng.close()
        twin.close()


# ---------------------------------------------------------------- (f) the track kernels
def _transition_weight(k, N):
    """csrc/track_kernels.h transition_weight in float32: (float)(k + 1 or N - k) / (float)(N / 2), one IEEE division."""
    raw = np.where(k < N // 2, k + 1, N - k).astype(np.float32)
    return raw / np.float32(N // 2)


def test_track_kernels_write_exactly_their_samples(pkg, model_small, torch):
    """weight_stems (w * s in place, k < n), track_accumulate (track[offset + k] += weighted[k], sum_weight[offset + k] += w) and
    track_normalise (track /= sum_weight over the length): each a single float32 operation per value, so bit for bit."""
    _, _, targets = model_small
    N = gd.SINGLE_N
    L, offset, n = int(2.7 * N) + 3, 12345, N - 1023
    rng = np.random.default_rng(7)
    eng = pkg.Engine(targets, 128, N)
    try:
        k = np.arange(n)
        w = _transition_weight(k, N)
        stems = [rng.uniform(-1, 1, 2 * n).astype(np.float32) for _ in range(4)]
        sb = [Buf(torch, gd.stem_layout(n, N, 8 * (t % 2)), stems[t]) for t in range(4)]
        torch.cuda.synchronize()
        eng.weight_stems_device([b.ptr for b in sb], n)
        torch.cuda.synchronize()
        weighted = [(w[:, None] * s.reshape(n, 2)).ravel() for s in stems]
        for t in range(4):
            r = sb[t].report(gd.make(sb[t].layout, weighted[t]))
            assert r.ok, ("weight_stems", t, str(r))
        track0 = [rng.uniform(-1, 1, 2 * L).astype(np.float32) for _ in range(4)]
        sumw0 = rng.uniform(0.25, 2, L).astype(np.float32)
        tb = [Buf(torch, gd.track_layout(2 * L, 8 * ((t + 1) % 2)), track0[t]) for t in range(4)]
        swb = Buf(torch, gd.track_layout(L, 8), sumw0)
        torch.cuda.synchronize()
        eng.track_accumulate_device([b.ptr for b in tb], swb.ptr, [b.ptr for b in sb], offset, n)
        torch.cuda.synchronize()
        track1 = [x.copy() for x in track0]
        for t in range(4):
            track1[t][2 * offset:2 * (offset + n)] += weighted[t]
        sumw1 = sumw0.copy()
        sumw1[offset:offset + n] += w
        for t in range(4):
            r = tb[t].report(gd.make(tb[t].layout, track1[t]))
            assert r.ok, ("track_accumulate", t, str(r))
            r = sb[t].report(gd.make(sb[t].layout, weighted[t]))
            assert r.ok, ("track_accumulate reads the weighted stems only", t, str(r))
        r = swb.report(gd.make(swb.layout, sumw1))
        assert r.ok, ("track_accumulate sum_weight", str(r))
        eng.track_normalise_device([b.ptr for b in tb], swb.ptr, L)
        torch.cuda.synchronize()
        for t in range(4):
            want = (track1[t].reshape(L, 2) / sumw1[:, None]).ravel()
            r = tb[t].report(gd.make(tb[t].layout, want))
            assert r.ok, ("track_normalise", t, str(r))
        r = swb.report(gd.make(swb.layout, sumw1))
        assert r.ok, ("track_normalise reads sum_weight only", str(r))
    finally:
        eng.close()


# ---------------------------------------------------------------- (g) the multi-GPU driver's exact-size arena stems
def test_world1_driver_under_the_fused_kernel_equals_the_whole_track_driver(pkg, model_small, torch, monkeypatch):
    """host/mgpu.cpp gives each stem of a segment exactly 2n floats, back to back in one arena: a store past n of the short last
    segment would land in the next stem."""
    monkeypatch.setenv("UMX_WIENER", "fused")
    _, _, targets = model_small
    N = 24 * HOP
    eng = pkg.Engine(targets, 128, N)
    mg = pkg.MultiGpuTrack(eng)
    try:
        for L, off in ((int(N * 3.3), None), (int(N * 2.1) + 7, 4033)):
            wave = _audio(L, 900 + L % 7)
            ref = eng.separate(wave, shift_offset=off)
            got = mg.separate(wave, shift_offset=off)
            for t in range(4):
                assert np.isfinite(got[t]).all(), (L, off, t)
                assert np.array_equal(got[t].view(np.int32), ref[t].view(np.int32)), (L, off, t)
    finally:
        mg.close()
        eng.close()
