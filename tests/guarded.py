"""tests/guarded.py -- caller buffers with NaN guards on both sides, for the write contract of the device entry points
(include/umx_hip.h): a call with n samples writes out[t][0 .. 2n) and nothing else, and reads audio[0 .. 2n) and nothing else.

Every buffer is its own allocation, [pre-guard | payload | post-guard], held as int32 words so that bit patterns survive:
  * the payload has exactly the size the contract names (2n floats, or a track's length) and starts at 0 or 8 mod 256 bytes
    (the header asks for float2 alignment, no more);
  * the pre-guard is at least 4 KiB; the post-guard reaches past the furthest store ANY kernel could issue for the context
    without its n predicate (furthest_stem_sample), plus a margin -- an overrun lands in the test's own allocation;
  * guards hold GUARD, an output payload holds FILL before the call (a word the call did not write shows as a hole), an input
    payload holds the real audio.  Both are quiet NaNs no kernel computes; a NaN read past an input poisons the outputs.
Host logic only: numpy arrays stand in for device memory (tests/test_guarded_cpu.py); the GPU module copies these words to and
from torch tensors (tests/test_gpu_device_buffers.py).
"""
from dataclasses import dataclass, field

import numpy as np

HOP, NFFT = 1024, 4096
GUARD = np.int32(0x7FC0DEAD)
FILL = np.int32(0x7FC0F111)
PRE_BYTES = 4096
ALIGN_BYTES = 256
MARGIN_SAMPLES = 2048  # beyond the furthest possible store


def n_frames(N):
    return N // HOP + 1


def furthest_stem_sample(N):
    """The largest stem sample index a segment kernel of a context with segment_samples N could store to if it dropped its
    `s < n` predicate (csrc/wiener_istft.h, csrc/stft_kernels.h), for any n and any run split.  Stem sample s is padded sample
    s + NFFT/2 of hop block h = (s + NFFT/2) / HOP:
      wiener_istft_kernel, in-loop store of frame f <= T - 1: block f                 -> (T - 2) HOP - 1
      wiener_ola_edges_kernel, blocks f0 .. f0 + 2 of a run that starts at f0 <= T - 1 -> (T + 2) HOP - NFFT/2 - 1 = T HOP - 1
      wiener_istft_kernel, run-end flush of blocks f1 .. f1 + 2, f1 <= T             -> (T + 3) HOP - NFFT/2 - 1 = (T + 1) HOP - 1
      istft_ola_kernel, threads up to ceil(n / 256) 256 - 1                          -> N + 255"""
    T = n_frames(N)
    return max((T - 2) * HOP - 1, T * HOP - 1, (T + 1) * HOP - 1, (N + 255) // 256 * 256 - 1)


def _round_up(x, m):
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class Layout:
    """Word offsets of one guarded buffer.  payload: words of the contract; reach: words from the payload start that a kernel
    could touch at most; misalign: the payload's start mod 256 bytes (0 or 8), given a 256-byte aligned allocation."""
    payload: int
    reach: int
    misalign: int = 0
    pre: int = field(init=False)
    post: int = field(init=False)

    def __post_init__(self):
        assert self.misalign in (0, 8) and self.payload >= 0 and self.reach >= self.payload
        object.__setattr__(self, "pre", (PRE_BYTES + self.misalign) // 4)
        end = _round_up(self.pre + self.reach + 2 * MARGIN_SAMPLES, ALIGN_BYTES // 4)
        object.__setattr__(self, "post", end - self.pre - self.payload)

    @property
    def total(self):
        return self.pre + self.payload + self.post

    @property
    def body(self):
        return slice(self.pre, self.pre + self.payload)


def stem_layout(n, N, misalign=0):
    """A (2,n) stem or audio buffer of a context with segment_samples N."""
    return Layout(2 * n, 2 * max(n, furthest_stem_sample(N) + 1), misalign)


def track_layout(words, misalign=0):
    """A track-sized buffer (4 stems x (2,length) or the weight sum (length)) for the track kernels: threads past the length
    reach at most 255 samples (256-thread blocks) -- 2 x 256 words covers a stem."""
    return Layout(words, words + 2 * 256, misalign)


def make(layout, payload=None):
    """The buffer's words before the call: guards, and FILL or the float32 payload given."""
    w = np.full(layout.total, GUARD, np.int32)
    if payload is None:
        w[layout.body] = FILL
    else:
        p = np.ascontiguousarray(payload, np.float32).ravel()
        assert p.size == layout.payload, (p.size, layout.payload)
        w[layout.body] = p.view(np.int32)
    return w


def payload(words, layout):
    """The payload as float32 (a copy)."""
    return np.array(words[layout.body]).view(np.float32)


def _span(idx, base):
    return None if idx.size == 0 else (int(idx[0]) - base, int(idx[-1]) - base, int(idx.size))


@dataclass
class Report:
    """Offsets are words from the payload start (negative: in front of it); a span is (first, last, count) or None."""
    pre: tuple = None        # guard words in front of the payload that changed
    post: tuple = None       # guard words behind it that changed
    holes: tuple = None      # payload words still holding FILL
    nonfinite: tuple = None  # payload words that are not finite floats (holes included)
    changed: tuple = None    # payload words that differ from the expected ones (inputs, in-place updates)

    @property
    def ok(self):
        return self.pre is None and self.post is None and self.holes is None and self.nonfinite is None and self.changed is None

    def __str__(self):
        return "clean" if self.ok else ", ".join(f"{k} {v}" for k, v in vars(self).items() if v is not None)


def check(words, layout, expect=None):
    """An output buffer after the call (expect=None): guards unchanged, every payload word written and finite.  Otherwise (an
    input, or a buffer updated in place) guards unchanged and the payload exactly the words of `expect` (a whole buffer's words)."""
    w = np.asarray(words, np.int32)
    assert w.shape == (layout.total,), (w.shape, layout.total)
    r = Report()
    r.pre = _span(np.flatnonzero(w[:layout.pre] != GUARD), layout.pre)
    r.post = _span(np.flatnonzero(w[layout.pre + layout.payload:] != GUARD) + layout.payload, 0)
    body = w[layout.body]
    if expect is None:
        r.holes = _span(np.flatnonzero(body == FILL), 0)
        r.nonfinite = _span(np.flatnonzero(~np.isfinite(body.view(np.float32))), 0)
    else:
        r.changed = _span(np.flatnonzero(body != np.asarray(expect, np.int32)[layout.body]), 0)
    return r


def untouched(words, before):
    """A buffer the call must not have touched at all (an idle lane's outputs): the span of words that changed, or None."""
    w, b = np.asarray(words, np.int32), np.asarray(before, np.int32)
    return _span(np.flatnonzero(w != b), 0)


# ---------------------------------------------------------------- the n of the device-buffer tests
def ragged_ns(N, run_len, nruns):
    """Segment lengths 1 <= n <= N at the edges of the kernels' tiles for a context with segment_samples N whose fused Wiener /
    inverse STFT call splits T frames into nruns runs of run_len (tests/stage_f64.fused_run_split): the last samples, the
    first hop blocks, a multiple of HOP and one past it, an end at the first block of runs 1, 2, the middle and the last (stem
    sample k run_len HOP - NFFT/2, and one either side), and an end inside a run's first three blocks (wiener_ola_edges_kernel)."""
    mid = max(1, N // HOP // 2) * HOP
    ns = {N, N - 1, N - 1023, 2049, 2048, 1025, 1024, 1, mid, mid + 1}
    runs = sorted({k for k in (1, 2, nruns // 2, nruns - 1) if 1 <= k < nruns})
    for k in runs:
        b = k * run_len * HOP - NFFT // 2
        ns |= {b - 1, b, b + 1}
    # inside the second of run k's first three blocks (stem samples [k run_len HOP - NFFT/2, + 3 HOP)); run 0's start before sample 0
    ns.add(runs[-1] * run_len * HOP - NFFT // 2 + HOP + 517 if runs else 517)
    return sorted(n for n in ns if 1 <= n <= N)


def lanes_of(ns, lanes):
    """ns dealt into calls of `lanes` lanes each: a list of per-call n lists (the last call padded with N = ns[-1])."""
    calls = [list(ns[i:i + lanes]) for i in range(0, len(ns), lanes)]
    calls[-1] += [max(ns)] * (lanes - len(calls[-1]))
    return calls


# the contexts of tests/test_gpu_device_buffers.py: segment_samples and track lanes of the batched device form, segment_samples of
# the single-track forms (T = 41: five runs of nine frames in a fused call of one lane)
BATCH_CONTEXTS = {"T201x3": (200 * HOP, 3), "N4096x3": (4096, 3), "T201x64": (200 * HOP, 64)}
SINGLE_N = 40 * HOP
