"""bench.py --dump-outputs: the stems of the last timed step, as they are (small runs) or as a fixed seeded sample
(the full-size workload), within the size bound; on the GPU, what the timed path computed, the same from run to run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
import bench  # noqa: E402


def test_dump_positions_are_bounded_and_fixed():
    n = 60 * 44100
    assert bench.dump_positions(16 * 1024, 2) is None  # small runs keep every sample
    for tracks in (1, 2, 64):
        pos = bench.dump_positions(n, tracks)
        assert pos is not None and tracks * 4 * len(pos) * 2 * 4 <= bench.DUMP_BYTES <= 64 * 10 ** 6
        assert (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < n
        assert (pos == bench.dump_positions(n, tracks)).all()  # seeded: the same positions in every run
    track = bench.dump_positions(600 * 44100, 1)
    assert 4 * len(track) * 2 * 4 <= bench.DUMP_BYTES


def test_dump_stems_writes_float32_at_the_positions(tmp_path):
    rng = np.random.default_rng(5)
    for n in (1000, 1_000_000):
        stems = [[rng.standard_normal(2 * n).astype(np.float32) for _ in range(4)] for _ in range(2)]
        bench.dump_stems(str(tmp_path / str(n)), stems, n)
        got = np.load(tmp_path / str(n) / "stems.npy")
        pos = bench.dump_positions(n, 2)
        idx = np.arange(n) if pos is None else pos
        assert got.dtype == np.float32 and got.shape == (2, 4, len(idx), 2)
        for b in range(2):
            for t in range(4):
                assert (got[b, t] == stems[b][t].reshape(n, 2)[idx]).all()


def _bench_dump(out_dir):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--tracks", "2", "--hidden", "128",
           "--segment-samples", str(16 * 1024), "--no-cpu-baseline", "--no-pcie", "--no-single-track", "--track-seconds", "0",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][-1])
    assert line["steps"] == 2
    return np.load(os.path.join(out_dir, "stems.npy"))


@pytest.mark.gpu
def test_bench_dump_is_the_timed_path_output_and_reproducible(pkg, po, tmp_path):
    """Two tracks, three consecutive segments each (1 warm-up + 2 timed steps, LSTM state carried): the dump is the third
    segment's stems of every track, within the parity tolerance of the oracle, and bit for bit the same in a second run."""
    H, N = 128, 16 * 1024
    a = _bench_dump(tmp_path / "a")
    assert a.dtype == np.float32 and a.shape == (2, 4, N, 2)
    path = str(tmp_path / "m.bin")
    pkg.ggml.write_model(path, pkg.ggml.synth_weights(H, seed=0), H, compress=False)  # bench.py's weights
    om = po.Model.load(path)
    for b in range(2):
        wave = pkg.ggml.synth_audio(N, seed=b)  # bench.py's audio of lane b on rank 0
        st = po.stream_state(H)
        for _ in range(3):
            ref, _ = po.umx_inference(om, wave, n_buf=N, state=st)
        for t in range(4):
            err = float(np.abs(a[b, t].T - ref[t]).max())
            assert err < 1e-4, (b, t, err)
    b_ = _bench_dump(tmp_path / "b")
    assert np.array_equal(a, b_)
