"""Times of the residual source (UMX_FLAG_RESIDUAL; csrc/residual_mask.h) on a track-batched context.

    python tools/residual_timing.py calls     one segment of every lane per call, device buffers in / out: calls with flags 0 (four
                                              targets) alternated with calls for vocals + residual; medians of the call time (host
                                              clock around call + sync) and of umx_hip_stage_times.  The flags-0 figures are the ones
                                              to hold against the parent commit: run the same tool there (it needs nothing of the
                                              residual for them: --plain-only)
    python tools/residual_timing.py kernel    a few vocals + residual calls and nothing else: run it under
                                              rocprofv3 --kernel-trace --stats for residual_mask_kernel's own time

Default: 64 lanes x 60 s, hidden 1024.  The bytes the residual kernel must move are printed with the shapes."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

MAGP = 2176  # csrc/common.h: row pitch of a mask plane [2][T][MAGP]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["calls", "kernel"])
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="flags 0 only (a tree without the residual)")
    a = ap.parse_args()
    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    N = int(a.seconds * 44100)
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
    T = eng.T
    plane = 2 * T * MAGP * 4
    print(f"{a.lanes} lanes x {a.seconds:.0f} s (T = {T}), hidden {a.hidden}: one mask plane of all lanes {a.lanes * plane / 1e9:.3f} GB; "
          f"residual kernel with one active target reads 1 + writes 1 = {2 * a.lanes * plane / 1e9:.3f} GB, with three {4 * a.lanes * plane / 1e9:.3f} GB")
    base = pkg.ggml.synth_audio(N + 64 * a.lanes, 5)
    audio = [torch.from_numpy(np.ascontiguousarray(base[:, 64 * i:64 * i + N].T).ravel()).cuda() for i in range(a.lanes)]
    # two sets of stems: consecutive calls must be given distinct output buffers (umx_hip.h, ordering contract)
    outs = [[torch.empty(2 * N, device="cuda") for _ in range(4 * a.lanes)] for _ in range(2)]
    ap_, ns = [t.data_ptr() for t in audio], [N] * a.lanes
    plain = 0
    resid = 0 if a.plain_only else pkg.flags_for_targets(["vocals"], residual=True)
    ncall = [0]

    def call(flags):
        o = outs[ncall[0] % 2]
        ncall[0] += 1
        t0 = time.perf_counter()
        eng.infer_batch_ptrs(ap_, ns, [t.data_ptr() for t in o], flags)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3, eng.stage_times()

    if a.what == "kernel":
        for _ in range(a.reps + 1):
            call(resid)
        eng.close()
        return
    for f in (plain, resid):  # warm-up of both paths
        call(f)
    res = {"plain": ([], []), "residual": ([], [])}
    for _ in range(a.reps):
        for name, f in (("plain", plain), ("residual", resid)):
            if name == "residual" and a.plain_only:
                continue
            ms, st = call(f)
            res[name][0].append(ms)
            res[name][1].append(st)
    out = {"lanes": a.lanes, "seconds": a.seconds, "hidden": a.hidden, "T": T}
    for name, (ms, st) in res.items():
        if not ms:
            continue
        out[name] = {"call_ms_median": round(statistics.median(ms), 3), "call_ms": [round(x, 3) for x in ms],
                     "stage_ms_median": {k: round(statistics.median(s[k] for s in st), 3) for k in st[0]}}
        print(f"{name}: call median {out[name]['call_ms_median']} ms, min {min(ms):.3f}, max {max(ms):.3f}  {out[name]['call_ms']}")
        print("   stages (median ms): " + "  ".join(f"{k} {v}" for k, v in out[name]["stage_ms_median"].items()))
    if "residual" in out:
        print(f"plain / residual call time: {out['plain']['call_ms_median'] / out['residual']['call_ms_median']:.2f}x")
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
