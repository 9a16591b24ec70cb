"""Times of the device resampler (csrc/resample.h) on a 600 s track.

    python tools/resample_timing.py kernels   the two launches of a 48 kHz track, a few times each (run it under
                                              rocprofv3 --kernel-trace --stats for the kernel times): 48k -> 44.1k of the
                                              track, 44.1k -> 48k of its four stems in one launch
    python tools/resample_timing.py wall      umx_hip_shift_inference at 44.1 kHz against umx_hip_shift_inference_rate at
                                              48 kHz on the same audio, alternated, host buffers in / out; --reset adds both
                                              in reset mode on a two-lane context.  One `wall ...` line of medians and
                                              min .. max per mode: run it in fresh processes (DESIGN 23 alternates two trees)

Bytes each launch must move (the floor the kernel time is held against) are printed with the shapes."""
import argparse
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
    ap.add_argument("what", choices=["kernels", "wall"])
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reset", action="store_true", help="wall: also UMX_FLAG_RESET_SEGMENTS on a two-lane context")
    a = ap.parse_args()
    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    n48 = int(a.seconds * 48000)
    n44 = pkg.resampled_length(n48, 48000, 44100)
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden if a.what == "wall" else 128, seed=7), a.hidden if a.what == "wall" else 128)
        eng = pkg.Engine.from_file(path)
        eng2 = pkg.Engine.from_file(path, tracks=2) if a.what == "wall" and a.reset else None
    x48 = pkg.ggml.synth_audio(n48, 5)
    if a.what == "kernels":
        src = torch.from_numpy(np.ascontiguousarray(x48.T).ravel()).cuda()
        t44 = [torch.empty(2 * n44, device="cuda") for _ in range(4)]
        back = [torch.empty(2 * n48, device="cuda") for _ in range(4)]
        print(f"track 48k -> 44.1k: {n48} -> {n44} frames, {(n48 + n44) * 8 / 1e9:.3f} GB; "
              f"stems 44.1k -> 48k: 4 x {n44} -> {n48}, {4 * (n48 + n44) * 8 / 1e9:.3f} GB")
        for _ in range(a.reps + 1):  # the first of each is the warm-up
            eng.resample_device(48000, 44100, [src.data_ptr()], n48, [t44[0].data_ptr()], n44)
            torch.cuda.synchronize()
            eng.resample_device(44100, 48000, [t.data_ptr() for t in t44], n44, [b.data_ptr() for b in back], n48)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            eng.resample_device(44100, 48000, [t.data_ptr() for t in t44], n44, [b.data_ptr() for b in back], n48)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.reps * 1e3
        print(f"stems launch, host clock around {a.reps} back-to-back launches: {ms:.3f} ms each")
    else:
        src = torch.from_numpy(np.ascontiguousarray(x48.T).ravel()).cuda()
        dst = torch.empty(2 * n44, device="cuda")
        eng.resample_device(48000, 44100, [src.data_ptr()], n48, [dst.data_ptr()], n44)
        torch.cuda.synchronize()
        x44 = dst.cpu().numpy().reshape(n44, 2).T.copy()  # the same audio at 44.1 kHz
        import ctypes as C
        fp = C.POINTER(C.c_float)
        out44 = [np.empty(2 * n44, np.float32) for _ in range(4)]
        out48 = [np.empty(2 * n48, np.float32) for _ in range(4)]
        a44, a48 = np.ascontiguousarray(x44.T).ravel(), np.ascontiguousarray(x48.T).ravel()
        o48 = (fp * 4)(*[o.ctypes.data_as(fp) for o in out48])

        def run48(e, flags):
            t0 = time.perf_counter()
            rc = e.lib.umx_hip_shift_inference_rate(e.h, a48.ctypes.data_as(fp), n48, 48000, 4033, o48, flags, None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        for mode, e, flags in (("carry", eng, 0), ("reset", eng2, pkg.FLAG_RESET_SEGMENTS)):
            if e is None:
                continue
            run48(e, flags)  # warm-up of both paths
            e.separate_interleaved(a44, n44, out44, flags, 4033)
            t_44, t_48 = [], []
            for _ in range(a.reps):
                t_44.append(e.separate_interleaved(a44, n44, out44, flags, 4033))
                t_48.append(run48(e, flags))
            launches = e.resample_launches() if hasattr(e, "resample_launches") else None
            print(f"wall {mode} {a.seconds:.0f} s hidden {a.hidden}: 44.1 kHz median {statistics.median(t_44) * 1e3:.2f} ms "
                  f"({min(t_44) * 1e3:.2f} .. {max(t_44) * 1e3:.2f}); 48 kHz median {statistics.median(t_48) * 1e3:.2f} ms "
                  f"({min(t_48) * 1e3:.2f} .. {max(t_48) * 1e3:.2f}); resampler launches of the 48 kHz call {launches}", flush=True)
        if eng2 is not None:
            eng2.close()
    eng.close()


if __name__ == "__main__":
    main()
