"""tests/poison.py -- non-finite audio for the containment contract of include/umx_hip.h ("Non-finite input"): the poison patterns,
applied to a copy of a clean wave, the STFT frames a set of samples reaches, and a small builder of schedules -- which lane is
poisoned in which call, and where the reset of that lane falls.  Test infrastructure for tests/test_poison_cpu.py (the patterns
through the oracle, no GPU) and tests/test_gpu_poisoned_lanes.py.  Nothing here needs a GPU.

The patterns, on a (2, n) float32 wave:
  nan_mid    (a) one NaN sample mid-segment, in channel 0
  inf_pair   (b) one +inf sample in channel 0 and one -inf sample in channel 1, a few hops apart
  nan_lane   (c) every sample NaN
  huge       (d) every sample of both channels +-3e38 (seeded signs): all finite, and the windowed sums of the STFT overflow in every
                 frame -- a run of a few samples would leave the frames that touch it with the tail of their window finite in some bins
  nan_last   (e) the last valid sample NaN, both channels (with n < N: the edge of the zero-padded tail of the segment buffer)
"""
from collections import namedtuple

import numpy as np

HOP, NFFT = 1024, 4096
PATTERNS = ("nan_mid", "inf_pair", "nan_lane", "huge", "nan_last")
HUGE = np.float32(3e38)


def poisoned_samples(pattern, n):
    """{channel: sorted sample indices} the pattern replaces in a wave of n samples."""
    if pattern == "nan_mid":
        return {0: [n // 2 + 7]}
    if pattern == "inf_pair":
        return {0: [n // 3 + 5], 1: [(2 * n) // 3 + 11]}
    if pattern in ("nan_lane", "huge"):
        return {0: list(range(n)), 1: list(range(n))}
    if pattern == "nan_last":
        return {0: [n - 1], 1: [n - 1]}
    raise ValueError(f"unknown poison pattern {pattern!r}: one of {', '.join(PATTERNS)}")


def apply(pattern, wave, seed=0):
    """A poisoned COPY of the (2, n) float32 wave; the wave itself is left as it is."""
    wave = np.asarray(wave)
    assert wave.dtype == np.float32 and wave.ndim == 2 and wave.shape[0] == 2 and wave.shape[1] >= 8, (wave.dtype, wave.shape)
    out = wave.copy()
    n = wave.shape[1]
    where = poisoned_samples(pattern, n)
    if pattern == "inf_pair":
        out[0, where[0][0]] = np.inf
        out[1, where[1][0]] = -np.inf
    elif pattern == "huge":
        signs = np.random.default_rng(4200 + seed).integers(0, 2, size=(2, n)) * 2 - 1
        out[:] = (signs * HUGE).astype(np.float32)
    else:
        for c, idx in where.items():
            out[c, idx] = np.nan
    return out


def n_frames(N):
    return N // HOP + 1


def covering_frames(N, samples):
    """The frames of the STFT of a segment buffer of N samples that read any of `samples` (dsp.cpp:109-176: the buffer mirrored by
    NFFT / 2 at both ends, edge sample included; frame f reads padded positions [f HOP, f HOP + NFFT))."""
    half, T = NFFT // 2, n_frames(N)
    frames = set()
    for s in samples:
        assert 0 <= s < N, (s, N)
        places = [s + half]
        if s < half:
            places.append(half - 1 - s)
        if N - 1 - s < half:
            places.append(N + half + (N - 1 - s))
        for p in places:
            frames.update(f for f in range(max(0, (p - NFFT) // HOP + 1), min(T - 1, p // HOP) + 1))
    return sorted(frames)


def poisoned_frames(pattern, n, N):
    """The frames a pattern on a wave of n samples reaches in a segment buffer of N samples, over both channels."""
    where = poisoned_samples(pattern, n)
    if pattern in ("nan_lane", "huge"):  # (every valid sample: the union is that of the two ends and of every hop between them)
        picks = sorted(set(range(0, n, HOP)) | {n - 1})
        return covering_frames(N, picks)
    return covering_frames(N, sorted({s for idx in where.values() for s in idx}))


def nonfinite_frames(spec):
    """(2, T, bins) complex -> (frames with any non-finite bin in a channel, frames with EVERY bin non-finite in a channel), as sets."""
    spec = np.asarray(spec)
    bad = ~(np.isfinite(spec.real) & np.isfinite(spec.imag))
    return set(np.flatnonzero(bad.any(axis=(0, 2)))), set(np.flatnonzero(bad.all(axis=2).any(axis=0)))


# ---------------------------------------------------------------- schedules
Call = namedtuple("Call", "active poison flags short")
Call.__doc__ = """One call of a schedule.  active: frozenset of lanes with audio; poison: {lane: pattern} (a subset of active); flags:
the call's flag word; short: True = every lane's wave cut to the smallest n the entry point accepts (one sample)."""
Reset = namedtuple("Reset", "lane")
Reset.__doc__ = "track_stream_reset(lane) between two calls."


class PoisonSchedule:
    """Calls and resets in order.  A lane's history is a list of EPOCHS: a reset (or the start) opens one, and the k-th clean call of a
    lane consumes the lane's k-th clean segment counted over all its epochs, so that no clean wave is used twice.  A poisoned call
    consumes a segment as well (the clean wave the pattern is applied to)."""

    def __init__(self, steps, depth):
        self.steps, self.depth = list(steps), int(depth)
        assert self.depth >= 1
        seen, dirty = {}, set()
        self.segment, self.history = [], {}  # per step: {lane: segment} (None for a reset); lane -> [[(step, segment), ...] per epoch]
        for i, st in enumerate(self.steps):
            if isinstance(st, Reset):
                assert st.lane in dirty, ("a reset of a lane that is not poisoned", i, st.lane)
                dirty.discard(st.lane)
                self.history.setdefault(st.lane, [[]]).append([])
                self.segment.append(None)
                continue
            assert st.active and set(st.poison) <= set(st.active), i
            assert not (dirty & set(st.active) - set(st.poison)), ("a poisoned lane runs again before its reset", i, sorted(dirty))
            assert all(p in PATTERNS for p in st.poison.values()), i
            seg = {}
            for ln in sorted(st.active):
                seg[ln] = seen.get(ln, 0)
                seen[ln] = seg[ln] + 1
                if ln not in st.poison:
                    self.history.setdefault(ln, [[]])[-1].append((i, seg[ln]))
            dirty |= set(st.poison)
            self.segment.append(seg)
        assert not dirty, ("a schedule ends with a poisoned lane not reset", sorted(dirty))
        self.counts = seen
        for i in self.poisoned_calls():
            assert self.clean_calls_behind(i) >= self.depth + 1, ("too few clean calls behind a poisoned one", i)

    def poisoned_calls(self):
        return [i for i, st in enumerate(self.steps) if isinstance(st, Call) and st.poison]

    def clean_calls_behind(self, i):
        """Calls without poison behind step i (every pipeline slot is revisited once there are depth of them, and once more)."""
        return sum(1 for st in self.steps[i + 1:] if isinstance(st, Call) and not st.poison)

    def lanes(self):
        return sorted(self.counts)

    def clean_sequence(self, lane):
        """The lane's clean calls as its one-lane reference runs them: a tuple of epochs, each a tuple of (segment, flags, short)."""
        return tuple(tuple((seg, self.steps[i].flags, self.steps[i].short) for i, seg in ep) for ep in self.history.get(lane, [[]]))

    def reference_index(self, i, lane):
        """(epoch, position in it) of the clean call of `lane` in step i."""
        for e, ep in enumerate(self.history[lane]):
            for k, (step, _) in enumerate(ep):
                if step == i:
                    return e, k
        raise KeyError((i, lane))


def build(lanes, poison, depth, *, flags=0, before=1, behind=None, behind_active=None, behind_flags=None, behind_short=False):
    """The common shape: `before` clean calls of all `lanes`, the poisoned call (poison: {lane: pattern}) with `flags`, the reset of
    every poisoned lane, then the clean calls behind it -- depth + 1 of them unless `behind` says more.  behind_active[k] / behind_flags[k]:
    the lane set / flag word of the k-th clean call behind (None, or past the end of the list: all lanes / `flags`); behind_short: those
    calls run at the smallest n."""
    lanes = frozenset(lanes)
    n_behind = depth + 1 if behind is None else int(behind)
    steps = [Call(lanes, {}, flags, False) for _ in range(before)]
    steps.append(Call(lanes, dict(poison), flags, False))
    steps += [Reset(ln) for ln in sorted(poison)]
    for k in range(n_behind):
        act = lanes if not behind_active or k >= len(behind_active) or behind_active[k] is None else frozenset(behind_active[k])
        fl = flags if not behind_flags or k >= len(behind_flags) or behind_flags[k] is None else behind_flags[k]
        steps.append(Call(act, {}, fl, bool(behind_short)))
    return PoisonSchedule(steps, depth)


# ---------------------------------------------------------------- the schedules of tests/test_gpu_poisoned_lanes.py
PIPELINE_DEPTH = 2  # umx_hip_pipeline_depth of every context (csrc/engine_init.h: two slots); the GPU file asserts it
FLAG_SOFTMASK, FLAG_LSTM_STEPWISE, FLAG_RESIDUAL = 0x2, 0x10, 0x8000  # include/umx_hip.h; tests/test_poison_cpu.py holds them to the package


def SKIP(*targets):
    return sum(0x100 << t for t in targets)


def ITERS(n):
    return n << 16


Entry = namedtuple("Entry", "hidden tracks kernel schedule env")
Entry.__doc__ = """One schedule and where it runs.  tracks: lanes of the context (1: the one-track context, gemm_bf16x3_kernel and
lstm_persistent_kernel); kernel: what lstm_kernel_name reports for a persistent call; env: environment the context is created under."""
B8, BG, P1 = "lstm_batch8_kernel", "lstm_batch_kernel", "lstm_persistent_kernel"
R = lambda a, b: range(a, b + 1)  # noqa: E731  (lanes a .. b)


# the schedules whose poisoned call tests/test_gpu_poisoned_lanes.py takes with FLAG_DEBUG_TAPS: one per recurrence (lstm_batch_kernel,
# lstm_batch8_kernel with one octet and with two in turn, lstm_persistent_kernel, the per-step driver), together every pattern
NOT_VACUOUS = ("h256_17_huge", "h256_17_two_in_a_group", "h512_8_inf_pair_last", "h1024_33_nan_last_32", "h128_1_nan_mid", "h512_1_nan_lane_stepwise")
AGAINST_F64 = "h512_9_huge_second_octet"  # the one whose first clean call behind the poison is held to float64


def clean_wave(pkg, N, lane, k):
    """The k-th clean segment of a lane (the waves of tests/test_gpu_sparse_lanes.py: Lab.audio)."""
    return pkg.ggml.synth_audio(N - 31 * ((lane + 2 * k) % 5), 9000 + 8 * lane + k)


def catalogue(depth=PIPELINE_DEPTH):
    """name -> Entry.  The lane sets are those of the table in DESIGN 28: hidden 128 / 256 at 3 and 17 lanes (lstm_batch_kernel, one
    and two groups, lane 16 the first of the second group), hidden 512 at 8 and 9 (one octet full, a second of one lane), hidden 1024
    at 33 and 64 (two octets per workgroup in turn; 31 | 32 is the pair boundary), and the one-track context at 128 and 512.  The 3-,
    8- and 33-lane calls run on the 17-, 9- and 64-lane context: everything a call launches follows from its lane set (lane_masks.py)."""
    d = depth
    vocals = SKIP(0, 1, 2)
    c = {
        # containment and recovery on the same geometry: every pattern in both recurrence families
        "h128_3_nan_mid": Entry(128, 17, BG, build(R(0, 2), {1: "nan_mid"}, d), {}),
        "h128_17_inf_pair": Entry(128, 17, BG, build(R(0, 16), {16: "inf_pair"}, d), {}),
        "h256_3_nan_last": Entry(256, 17, BG, build(R(0, 2), {0: "nan_last"}, d), {}),
        "h256_17_huge": Entry(256, 17, BG, build(R(0, 16), {16: "huge"}, d), {}),
        "h256_17_two_in_a_group": Entry(256, 17, BG, build(R(0, 16), {3: "nan_mid", 9: "nan_lane"}, d), {}),
        "h512_8_nan_lane_first": Entry(512, 9, B8, build(R(0, 7), {0: "nan_lane"}, d), {}),
        "h512_8_inf_pair_last": Entry(512, 9, B8, build(R(0, 7), {7: "inf_pair"}, d), {}),
        "h512_9_huge_second_octet": Entry(512, 9, B8, build(R(0, 8), {8: "huge"}, d), {}),
        "h512_9_two_in_an_octet": Entry(512, 9, B8, build(R(0, 8), {2: "nan_mid", 5: "nan_lane"}, d), {}),
        "h1024_33_nan_mid_31": Entry(1024, 64, B8, build(R(0, 32), {31: "nan_mid"}, d), {}),
        "h1024_33_nan_last_32": Entry(1024, 64, B8, build(R(0, 32), {32: "nan_last"}, d), {}),
        "h1024_64_pair_boundary_and_last": Entry(1024, 64, B8, build(R(0, 63), {31: "inf_pair", 32: "nan_lane", 63: "huge"}, d), {}),
        "h1024_64_two_in_an_octet": Entry(1024, 64, B8, build(R(0, 63), {41: "nan_mid", 46: "nan_lane"}, d), {}),
        "h128_1_nan_mid": Entry(128, 1, P1, build([0], {0: "nan_mid"}, d), {}),
        "h128_1_huge_stepwise": Entry(128, 1, P1, build([0], {0: "huge"}, d, flags=FLAG_LSTM_STEPWISE), {}),
        "h512_1_inf_pair": Entry(512, 1, P1, build([0], {0: "inf_pair"}, d), {}),
        "h512_1_nan_lane_stepwise": Entry(512, 1, P1, build([0], {0: "nan_lane"}, d, flags=FLAG_LSTM_STEPWISE), {}),
        # recovery after a change of shape
        "short_h512_9": Entry(512, 9, B8, build(R(0, 8), {8: "nan_lane"}, d, behind_short=True), {}),
        "short_h128_1": Entry(128, 1, P1, build([0], {0: "nan_lane"}, d, behind_short=True), {}),
        "short_h128_3_stats4": Entry(128, 3, BG, build(R(0, 2), {1: "nan_lane"}, d, behind_short=True), {"UMX_WIENER": "stats4"}),
        "sparse_h256_17": Entry(256, 17, BG, build(R(0, 16), {16: "nan_lane"}, d, behind_active=[R(0, 15)]), {}),
        "sparse_h1024_64": Entry(1024, 64, B8, build(R(0, 63), {32: "huge"}, d, behind_active=[{3, 63}]), {}),
        "skip_h512_9": Entry(512, 9, B8, build(R(0, 8), {4: "nan_mid"}, d, behind=d + 2,
                                                behind_flags=[vocals, vocals | FLAG_RESIDUAL | FLAG_SOFTMASK, SKIP(1) | FLAG_RESIDUAL]), {}),
        "em_h256_17": Entry(256, 17, BG, build(R(0, 16), {5: "inf_pair"}, d, flags=ITERS(3), behind_flags=[ITERS(1), ITERS(3)]), {}),
        "em_h512_9": Entry(512, 9, B8, build(R(0, 8), {8: "huge"}, d, flags=ITERS(3), behind_flags=[ITERS(1), ITERS(3)]), {}),
    }
    return c
