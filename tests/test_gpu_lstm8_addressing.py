"""The addressing of lstm_batch8_kernel's step loop (csrc/lstm_batch8.h): every stream behind a buffer resource, a per-lane offset formed
once (beyond the range for lanes with nothing to load or store) and a scalar offset that a step advances by an add.

The smallest shapes at which that can go wrong, each compared BITWISE with the same kernel one step per launch (FLAG_LSTM_STEPWISE),
where every launch forms its offsets afresh from the step number:
  * segments of 5 and 6 frames -- odd and even T, so the end rows of the forward and the backward chains differ;
  * 9 lanes (a second octet with one lane, one octet per workgroup), 33 lanes (two octets per workgroup in turn, a one-lane partner
    octet), 40 lanes (workgroups with one octet and with two);
  * a call with two lanes idle and one lane shorter than the segment; state carried over two consecutive calls;
  * stems and carried state of a plain call (the rows leave as fused planes only), the `lstm` and `fc2` taps of a call with
    FLAG_DEBUG_TAPS (the fp32 rows of every step as well, and the planes' consumer);
  * hidden 512 with 64 lanes: the side-by-side form (eight octets, one per workgroup).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("lstm8_addr")
    paths = {}
    for hidden in (1024, 512):
        paths[hidden] = str(d / f"m{hidden}.bin")
        pkg.ggml.write_model(paths[hidden], pkg.ggml.synth_weights(hidden, seed=71), hidden, compress=False)
    return paths


def _run(pkg, path, N, B, lstm_flags):
    """Two consecutive calls: all lanes with a plain call, then two lanes idle and one short with the debug taps."""
    idle, short = (1, B - 2), B - 1
    eng = pkg.Engine.from_file(path, N, tracks=B, quantised=True)
    first = [pkg.ggml.synth_audio(N, 7100 + b) for b in range(B)]
    second = [None if b in idle else pkg.ggml.synth_audio(N - 1500 if b == short else N, 7300 + b) for b in range(B)]
    out = {"stems1": eng.infer_batch(first, lstm_flags)}
    assert eng.lstm_kernel_name() == "lstm_batch8_kernel"
    out["state1"] = [eng.track_stream_get(b) for b in range(B)]
    out["stems2"] = eng.infer_batch(second, pkg.FLAG_DEBUG_TAPS | lstm_flags)
    out["taps"] = {(name, b, t): eng.tap(f"{name}#{b}", t) for name in ("lstm", "fc2") for b in range(B) if b not in idle for t in range(4)}
    out["state2"] = [eng.track_stream_get(b) for b in range(B)]
    persistent = eng.lstm_was_persistent()
    eng.close()
    return out, persistent, idle


@pytest.mark.parametrize("hidden,frames,B", [(1024, 5, 9), (1024, 6, 9), (1024, 5, 33), (1024, 6, 33), (1024, 5, 40), (1024, 6, 40), (512, 5, 64)])
def test_default_call_has_the_bits_of_the_per_step_driver(pkg, models, hidden, frames, B):
    N = frames * 1024
    got, persistent, idle = _run(pkg, models[hidden], N, B, 0)
    ref, ref_persistent, _ = _run(pkg, models[hidden], N, B, pkg.FLAG_LSTM_STEPWISE)
    assert persistent and not ref_persistent
    for call in ("stems1", "stems2"):
        for b in range(B):
            if call == "stems2" and b in idle:
                assert got[call][b] is None and ref[call][b] is None
                continue
            for t in range(4):
                assert (got[call][b][t] == ref[call][b][t]).all(), (call, b, t)
    for call in ("state1", "state2"):
        for b in range(B):
            assert (got[call][b] == ref[call][b]).all(), (call, b)
    for b in idle:  # a lane that sat the call out keeps its state
        assert (got["state2"][b] == got["state1"][b]).all(), b
    for key, tap in got["taps"].items():
        assert np.abs(tap).max() > 0, key
        assert (tap == ref["taps"][key]).all(), key
