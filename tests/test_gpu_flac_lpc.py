"""FLAC with LPC subframes (csrc/flac.h), without tolerances: the LPC variant of the encode kernel on guarded device buffers
against the host restatement byte for byte, and the whole-track call against its flac_lpc = 0 form: the same codes and levels, no more
bytes."""
import numpy as np
import pytest

import flac_lpc_ref
import flac_ref
from flac_lpc_ref import SIZES, signal
from flac_ref import RATE
import guarded

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: the smallest context of tests/test_gpu_flac.py
LENGTH = 30001
SEED = 7
SIGNALS = ["two_tones", "resonance", "noise24_quiet", "nonfinite"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    t.zeros(1).cuda()  # let torch initialise HIP before the engine's streams exist
    return t


@pytest.fixture(scope="module")
def eng3(pkg, model_small):
    e = pkg.Engine.from_file(model_small[0], N, tracks=3)
    yield e
    e.close()


@pytest.mark.parametrize("seed", [None, SEED], ids=["plain", "dithered"])
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("lpc", [1, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("n", SIZES)
def test_device_streams_are_the_host_streams(pkg, torch, eng3, n, bits, lpc, nb, seed):
    cap = (pkg.flac_bound(n, bits) + 3) // 4 * 4  # whole words of a guarded buffer (tests/guarded.py): guard | capacity (FILL) | guard
    for g in range(0, len(SIGNALS), nb):
        names = SIGNALS[g:g + nb]
        xs = [signal(s, n) for s in names]
        ins = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in xs]
        lays = [guarded.track_layout(cap // 4, misalign=8 * ((b + g) & 1)) for b in range(nb)]
        before = [guarded.make(lay) for lay in lays]
        outs = [torch.from_numpy(w).cuda() for w in before]
        got_bytes = torch.zeros(nb, dtype=torch.int64).cuda()
        first = 4 - nb  # (buffer b is output first + b of the dither rule)
        eng3.flac_encode_device([i.data_ptr() for i in ins], n, RATE, bits, [o.data_ptr() + 4 * lay.pre for o, lay in zip(outs, lays)], [cap] * nb, got_bytes.data_ptr(),
                                first_buffer=first, dither_seed=seed, lpc=lpc)
        torch.cuda.synchronize()
        for b in range(nb):
            want = pkg.flac_encode_host(xs[b], RATE, bits, buffer=first + b, dither_seed=seed, lpc=lpc)
            k, what = int(got_bytes[b]), (n, bits, lpc, nb, names[b], seed)
            assert k == want.size, (what, k, want.size)
            expect = before[b].copy()  # the stream's bytes and not a byte more, in front of it, behind it or beyond the capacity
            expect.view(np.uint8)[4 * lays[b].pre:4 * lays[b].pre + k] = want
            assert guarded.untouched(outs[b].cpu().numpy(), expect) is None, what


@pytest.mark.parametrize("reset", [False, True], ids=["carry", "reset"])
def test_whole_track_lpc_streams_decode_to_the_fixed_streams_codes(pkg, eng3, reset):
    x = pkg.ggml.synth_audio(LENGTH, 71)
    kw = dict(flags=pkg.FLAG_RESET_SEGMENTS if reset else 0, shift_offsets=[4033], io=pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_F32, SEED))
    for bits in (16, 24):
        base, lv0 = eng3.separate_many_flac([x], bits, lpc=None, **kw)[:2]  # umx_hip_separate_tracks_flac
        same, lvs = eng3.separate_many_flac([x], bits, lpc=0, **kw)[:2]  # 0 through umx_hip_separate_tracks_flac_lpc: that call
        streams, lv = eng3.separate_many_flac([x], bits, lpc=12, **kw)[:2]
        assert bytes(lv[0]) == bytes(lv0[0]) == bytes(lvs[0])
        for s, s0, ss in zip(streams[0], base[0], same[0]):
            assert np.array_equal(ss, s0)
            assert np.array_equal(flac_lpc_ref.decode(s)[1], flac_ref.decode(s0)[1]) and s.size <= s0.size, bits


def test_the_refusals(pkg, eng3):
    x = pkg.ggml.synth_audio(LENGTH, 73)
    for bits, lpc in [(16, 13), (24, -1), (0, 4)]:
        with pytest.raises(pkg.UmxError) as e:
            eng3.separate_many_flac([x], bits, lpc=lpc)
        assert e.value.code == pkg.ERR_ARG and "flac_lpc" in str(e.value), str(e.value)
