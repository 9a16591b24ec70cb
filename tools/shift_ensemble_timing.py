"""Times of the shift ensemble (umx_hip_shift_ensemble; csrc/shift_mean.h) against what a caller could do before it.

    python tools/shift_ensemble_timing.py [--shifts 1,2,4,10,16] [--seconds 600] [--hidden 1024] [--reps 5] [--out FILE]

Per K: the wall time of umx_hip_shift_ensemble (K shifts as the K lanes of one pass, one upload, the mean on the device, one
download) on a K-lane context, against K sequential umx_hip_shift_inference calls at the same offsets on a single-track context
with their fp32 mean taken on the host in numpy -- both on this tree, same weights, same track, host buffers in and out, the bare C
calls.  One warm-up call of each, then `reps` timed ones; medians.  One context is alive at a time.  K = 1 through the new entry
point is the same call as umx_hip_shift_inference: the two are alternated on the same context.  shift_mean_kernel's own time comes from device events around
its launch (umx_hip_debug_shift_mean_ms); its bytes are 4 stems x (K + 1) x 8 B per frame."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

FP = C.POINTER(C.c_float)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shifts", default="1,2,4,10,16")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--segment", type=int, default=None, help="segment_samples (default: the production 60 s)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    N = a.segment or pkg.SEGMENT_SAMPLES
    L = int(a.seconds * 44100)
    xi = np.ascontiguousarray(pkg.ggml.synth_audio(L, 5).T).ravel()  # (2,L) interleaved
    res_e, res_s, tmp = ([np.empty(2 * L, np.float32) for _ in range(4)] for _ in range(3))

    def ptrs(bufs):
        return (FP * 4)(*[b.ctypes.data_as(FP) for b in bufs])

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        box = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = sorted({ln.split(":", 1)[1].strip() for ln in box.splitlines() if "Marketing Name" in ln and "Instinct" in ln})
    except Exception:  # noqa: BLE001 - the identity line is a courtesy
        names = []
    say(f"# {', '.join(names) or torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# track {a.seconds:.0f} s ({L} frames), segment_samples {N}, hidden {a.hidden}, synthetic weights; 1 warm-up, median of {a.reps}")
    say("# ensemble: umx_hip_shift_ensemble on a K-lane context; sequential: K x umx_hip_shift_inference on a 1-lane context + numpy fp32 mean")
    out = {"seconds": a.seconds, "frames": L, "segment_samples": N, "hidden": a.hidden, "rows": []}
    shifts = [int(k) for k in a.shifts.split(",")]

    def shift_inference(eng, offset, bufs):  # the bare C calls, interleaved host buffers in and out
        t0 = time.perf_counter()
        rc = eng.lib.umx_hip_shift_inference(eng.h, xi.ctypes.data_as(FP), L, offset, ptrs(bufs), 0, None, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, eng.last_error()
        return dt

    def shift_ensemble(eng, offsets, bufs):
        K = len(offsets)
        t0 = time.perf_counter()
        rc = eng.lib.umx_hip_shift_ensemble(eng.h, xi.ctypes.data_as(FP), L, 44100, K, (C.c_int * K)(*offsets), ptrs(bufs), 0, None, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, eng.last_error()
        return dt

    def sequential(eng, offsets):  # K single-shift calls, the running fp32 sum and the division in numpy
        t0 = time.perf_counter()
        for k, o in enumerate(offsets):
            shift_inference(eng, o, res_s if k == 0 else tmp)
            for t in range(4 if k else 0):
                np.add(res_s[t], tmp[t], out=res_s[t])
        for t in range(4 if len(offsets) > 1 else 0):
            np.divide(res_s[t], np.float32(len(offsets)), out=res_s[t])
        return (time.perf_counter() - t0) * 1e3

    def med(v):
        return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"

    # One context is alive at a time, as in a caller's process: a second live context in the process was seen to slow the whole-track
    # calls (the last line measures umx_hip_shift_inference on one, and on a context created after all others were closed).
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        one = pkg.Engine.from_file(path, segment_samples=N)
        seq = {}
        for K in shifts:
            offsets = pkg.ensemble_offsets(K)
            sequential(one, offsets)
            seq[K] = [sequential(one, offsets) for _ in range(a.reps)]
        # K = 1 is the same call: both entry points on the SAME context, alternated
        shift_inference(one, 4033, res_s)
        shift_ensemble(one, [4033], res_e)
        same1 = all(np.array_equal(res_e[t], res_s[t]) for t in range(4))
        t_old, t_new = [], []
        for _ in range(a.reps):
            t_old.append(shift_inference(one, 4033, res_s))
            t_new.append(shift_ensemble(one, [4033], res_e))
        say(f"# K = 1 on one context, alternated: umx_hip_shift_inference {med(t_old)} ms, umx_hip_shift_ensemble {med(t_new)} ms, "
            f"results {'bit-identical' if same1 else 'DIFFER'}")
        out["k1_shift_inference_ms"], out["k1_shift_ensemble_ms"] = t_old, t_new
        ref10 = None
        if 10 in shifts:  # the sequential result, for the distance of the ensemble's (the one-lane context runs another LSTM kernel)
            sequential(one, pkg.ensemble_offsets(10))
            ref10 = [r.copy() for r in res_s]
        two = pkg.Engine.from_file(path, segment_samples=N)  # a second live context: the same entry point on it
        shift_inference(two, 4033, res_s)
        t_two = [shift_inference(two, 4033, res_s) for _ in range(a.reps)]
        two.close()
        one.close()
        say(f"{'K':>3} {'ensemble ms (min .. max)':>30} {'sequential ms (min .. max)':>32} {'seq / ens':>10} {'ens ms per shift':>17} "
            f"{'mean kernel ms':>15} {'GB':>7} {'TB/s':>6}")
        for K in shifts:
            offsets = pkg.ensemble_offsets(K)
            eng = pkg.Engine.from_file(path, segment_samples=N, tracks=K)
            shift_ensemble(eng, offsets, res_e)
            te, tk = [], []
            for _ in range(a.reps):
                te.append(shift_ensemble(eng, offsets, res_e))
                if K > 1:
                    tk.append(eng.shift_mean_ms())
            eng.close()
            me, ms = statistics.median(te), statistics.median(seq[K])
            gb = 4 * (K + 1) * 8 * L / 1e9
            mk = statistics.median(tk) if tk else None
            note = ""
            if K == 10 and ref10 is not None:
                note = f"   # ensemble against sequential result: max difference {max(float(np.abs(res_e[t] - ref10[t]).max()) for t in range(4)):.2e}"
            say(f"{K:>3} {med(te):>30} {med(seq[K]):>32} {ms / me:>10.2f} {me / K:>17.1f} "
                f"{(f'{mk:.3f}' if mk else '-'):>15} {(f'{gb:.2f}' if mk else '-'):>7} {(f'{gb / mk:.2f}' if mk else '-'):>6}{note}")
            out["rows"].append({"K": K, "ensemble_ms": te, "sequential_ms": seq[K], "mean_kernel_ms": tk, "mean_kernel_gb": gb})
        last = pkg.Engine.from_file(path, segment_samples=N)  # alone again: umx_hip_shift_inference as in the first line
        shift_inference(last, 4033, res_s)
        t_last = [shift_inference(last, 4033, res_s) for _ in range(a.reps)]
        last.close()
        say(f"# umx_hip_shift_inference on a second one-lane context while the first is alive: {med(t_two)} ms; on a one-lane context created "
            f"after all others were closed: {med(t_last)} ms")
        out["second_live_context_ms"], out["last_context_ms"] = t_two, t_last
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
