"""Times of the soft mask (UMX_FLAG_SOFTMASK; csrc/softmask.h) on a track-batched context.

    python tools/softmask_timing.py calls     one segment of every lane per call, device buffers in / out: calls with flags 0 (four
                                              targets) alternated with the same calls with the flag; medians of the call time (host
                                              clock around call + sync) and of umx_hip_stage_times (the kernel runs inside fc3's
                                              interval).  The flags-0 figures are the ones to hold against the parent commit: run the
                                              same tool there (it needs nothing of the soft mask for them: --plain-only)
    python tools/softmask_timing.py kernel    a few calls with the flag and nothing else: run it under
                                              rocprofv3 --kernel-trace --stats for softmask_kernel's own time; --targets vocals is
                                              the one-target kernel (NA = 1), the default all four (NA = 4)

Default: 64 lanes x 60 s, hidden 1024.  The bytes the kernel must move are printed with the shapes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["calls", "kernel"])
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--targets", default="bass,drums,other,vocals", help="the active targets of the flagged calls")
    ap.add_argument("--plain-only", action="store_true", help="flags 0 only (a tree without the soft mask)")
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
    names = a.targets.split(",")
    bins = a.lanes * 2 * T * 2049  # channel-bin-frames of a call: 8 B of mixture and 4 + 4 B per active mask each
    print(f"{a.lanes} lanes x {a.seconds:.0f} s (T = {T}), hidden {a.hidden}: softmask kernel with {len(names)} active target(s) moves "
          f"{bins * (8 + 8 * len(names)) / 1e9:.3f} GB ({bins * 8 / 1e9:.3f} GB of mixture, {bins * 8 * len(names) / 1e9:.3f} GB of masks in and out)")
    base = pkg.ggml.synth_audio(N + 64 * a.lanes, 5)
    audio = [torch.from_numpy(np.ascontiguousarray(base[:, 64 * i:64 * i + N].T).ravel()).cuda() for i in range(a.lanes)]
    # two sets of stems: consecutive calls must be given distinct output buffers (umx_hip.h, ordering contract)
    outs = [[torch.empty(2 * N, device="cuda") for _ in range(4 * a.lanes)] for _ in range(2)]
    ap_, ns = [t.data_ptr() for t in audio], [N] * a.lanes
    resid = 0 if a.plain_only else pkg.flags_for_targets(names, softmask=True)
    plain = 0 if a.plain_only else pkg.flags_for_targets(names)
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
    res = {"plain": ([], []), "softmask": ([], [])}
    for _ in range(a.reps):
        for name, f in (("plain", plain), ("softmask", resid)):
            if name == "softmask" and a.plain_only:
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
    if "softmask" in out:
        print(f"plain / softmask call time: {out['plain']['call_ms_median'] / out['softmask']['call_ms_median']:.2f}x")
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
