"""What the limiter's true-peak detector costs, with the inputs and method of tools/limit_timing.py: one 600 s stereo track.

    python tools/limit_tp_timing.py --kernel
        umx_hip_limit_gain_tp_device (the detector launch and the word-input gain launch) and umx_hip_limit_gain_device (the sample
        detector's one launch) on four outputs of 600 s at 44.1 kHz (F = 4) and at 96 kHz (F = 2): noise at 0.5 with a 4.0 spike and an
        fs/4 burst of amplitude 1 every second.  ms between two events on one stream, median [min .. max] of 9 calls after a warm-up;
        whether gains and count are the host twin's (on the first 2 s, where the host twin is quick).  Run it under a kernel trace for
        the split between the two launches.
    python tools/limit_tp_timing.py --walls [--parent-root <built checkout of the parent commit>]
        limit_timing.py's walls -- hidden 1024, carry mode on one lane and reset mode on 14, gspi_stereo.wav tiled and tripled, the bare
        C entry points -- for the plain fp32 call, the int16 call and the sample-peak limiter, which the parent has too, and in this
        tree the true-peak limiter; four fresh processes in the order parent1, pr1, parent2, pr2."""
import argparse
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import limit_timing as lt  # noqa: E402  (its ROOT: the tree UMX_TIMING_ROOT names, or this one)

ge, med, CEILING = lt.ge, lt.med, lt.CEILING


def kernel_main(seconds):
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=3), 128)
        eng = pkg.Engine.from_file(path, 16 * 1024, tracks=1)
    stream = torch.cuda.current_stream().cuda_stream
    for rate in (44100, 96000):
        n = seconds * rate
        rng = np.random.default_rng(5)
        xs = [(0.5 * rng.uniform(-1, 1, (2, n))).astype(np.float32) for _ in range(4)]
        k = np.arange(-7, 9)
        for b, x in enumerate(xs):
            x[b & 1, b * 1000 + rate // 2::rate] = 4.0
            for f in range(b * 1000 + rate // 4, n - 16, rate):
                x[:, f + k] = np.sin(2.0 * np.pi * k / 4.0 + np.pi / 4.0).astype(np.float32)
        src = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in xs]
        ptrs = [s.data_ptr() for s in src]
        gain, rep = torch.zeros(n, dtype=torch.float32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
        for label, detector in (("sample gain", pkg.LIMIT_SAMPLE_PEAK), ("detector + word gain", pkg.LIMIT_TRUE_PEAK)):
            ms = []
            for it in range(10):
                rep.zero_()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                eng.limit_gain_device(ptrs, n, rate, CEILING, gain.data_ptr(), rep.data_ptr(), hip_stream=stream, detector=detector)
                ev[1].record()
                torch.cuda.synchronize()
                if it:
                    ms.append(ev[0].elapsed_time(ev[1]))
            print(f"{label:<20} | {rate} Hz | 4 outputs x {seconds} s | {med(ms)} ms | {int(rep.cpu()[1])} frames limited", flush=True)
        head = 2 * rate
        g_ref, _, _ = pkg.limit_host([x[:, :head + 2048] for x in xs], rate, CEILING, detector=pkg.LIMIT_TRUE_PEAK)
        same = np.array_equal(gain[:head].cpu().numpy().view(np.uint32), g_ref[:head].view(np.uint32))
        print(f"{rate} Hz: gains of the first {head} frames equal to the host twin's: {same}", flush=True)
    eng.close()


def walls_child(tag, seconds):
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = seconds * lt.RATE
    q = pkg.wav_load_pcm16(lt.HERE / "tests" / "golden" / "gspi_stereo.wav")[0].astype(np.float32) / 32768.0
    x = 3.0 * np.tile(q, (1, n // q.shape[1] + 1))[:, :n]
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(1024, seed=7), 1024)
        engines = [("carry, 1 lane  ", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES), 0),
                   ("reset, 14 lanes", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES, tracks=lt.RESET_LANES), pkg.FLAG_RESET_SEGMENTS)]
    top = "umx_hip_separate_tracks_limit"
    cases = [("fp32", "umx_hip_separate_tracks_io", None, {}), ("int16 out", "umx_hip_separate_tracks_io", pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16), {}),
             ("fp32 limit", top, None, {"ceiling": CEILING})]
    if hasattr(pkg, "LIMIT_TRUE_PEAK"):
        cases.append(("fp32 limit tp", top, None, {"ceiling": CEILING, "detector": pkg.LIMIT_TRUE_PEAK}))
    for mode, eng, flags in engines:
        for label, entry, io, more in cases:
            call = pkg._MeasuredCall(entry, eng.h, [x], io, flags, [lt.SHIFT], None, None, **more)
            ms = []
            for it in range(9):
                t0 = time.perf_counter()
                rc = getattr(eng.lib, entry)(*call.args)
                dt = 1e3 * (time.perf_counter() - t0)
                assert rc == 0, eng.last_error()
                if it >= 2:
                    ms.append(dt)
            lr = call.lr
            note = "" if lr is None else f" | min gain {lr[0].min_gain:.4f}, {lr[0].limited_frames} frames limited"
            if "detector" in more:
                note += f", true_peak_after / c {lr[0].true_peak_after / float(CEILING):.6f}"
            print(f"{tag:<7} | {mode} | {label:<13} {med(ms)} ms{note}", flush=True)
    for _, eng, _ in engines:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--seconds", type=int, default=lt.SECONDS, help="the track's length (600: 14 segments, one call in reset mode)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", default=None, help="(the fresh processes) the tag of the tree UMX_TIMING_ROOT names")
    a = ap.parse_args()
    if a.child:
        return walls_child(a.child, a.seconds)
    if a.kernel:
        kernel_main(a.seconds)
    if a.walls:
        for tag, root in [("parent1", a.parent_root), ("pr1", None), ("parent2", a.parent_root), ("pr2", None)]:
            if tag.startswith("parent") and not root:
                continue
            env = {k: v for k, v in os.environ.items() if k not in ("UMX_HIP_LIB", "UMX_TIMING_ROOT")}
            if root:
                env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
            subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", tag, "--seconds", str(a.seconds)], env=env, check=True, timeout=500)


if __name__ == "__main__":
    main()
