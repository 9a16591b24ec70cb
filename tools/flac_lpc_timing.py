"""What LPC subframes cost and save in the FLAC encode, with the inputs and method of profiles/flac_timing.txt: one 600 s
stereo track at 44.1 kHz, "music" = tests/golden/gspi_stereo.wav tiled to length, "noise" = white noise at 0.5.

    python tools/flac_lpc_timing.py --kernel
        umx_hip_flac_encode_device_lpc on four 600 s buffers (the INPUT audio rolled by 1000 frames per buffer) at flac_lpc 0 / 4 / 8 /
        12 and both widths: the call's three launches between two events on one stream, ms as median [min .. max] of 5 calls after a
        warm-up, and the four streams' bytes against flac_lpc = 0 and against PCM
    python tools/flac_lpc_timing.py --walls [--parent-root <built checkout of the parent commit>]
        hidden 1024, host buffers in and out, the bare C entry point (buffers marshalled once, outside the timing): carry mode on one
        lane and reset mode on 14 lanes; the plain call (_flac, bits 0), FLAC16 / FLAC24 through the _flac call, which the parent has
        too, and in this tree through the _flac_lpc call at flac_lpc 4 and 12.  ms: median [min .. max] of 7 calls after 2 warm-ups;
        four fresh processes in the order parent1, pr1, parent2, pr2 (UMX_TIMING_ROOT tells a child which tree to load)."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
ROOT = Path(os.environ.get("UMX_TIMING_ROOT") or HERE).resolve()
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SECONDS, RATE, NB = 600, 44100, 4
SHIFT, RESET_LANES, FLAG_RESET = 4033, 14, 0x4000  # a 600 s track is 14 segments: one call in reset mode


def inputs(pkg, n):
    q = pkg.wav_load_pcm16(HERE / "tests" / "golden" / "gspi_stereo.wav")[0].astype(np.float32) / 32768.0
    return {"music": np.tile(q, (1, n // q.shape[1] + 1))[:, :n],
            "noise": (0.5 * np.random.default_rng(5).uniform(-1, 1, (2, n))).astype(np.float32)}


def med(v):
    return f"{statistics.median(v):7.2f} [{min(v):7.2f} .. {max(v):7.2f}]"


def kernel_main():
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = SECONDS * RATE
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=3), 128)
        eng = pkg.Engine.from_file(path, 16 * 1024, tracks=1)
    stream = torch.cuda.current_stream().cuda_stream
    for name, x in inputs(pkg, n).items():
        ins = [torch.from_numpy(np.ascontiguousarray(np.roll(x, 1000 * b, axis=1).T)).cuda() for b in range(NB)]
        for bits in (16, 24):
            cap = pkg.flac_bound(n, bits)
            outs = [torch.empty(cap, dtype=torch.uint8).cuda() for _ in range(NB)]
            got = torch.zeros(NB, dtype=torch.int64).cuda()
            base = None
            for lpc in (0, 4, 8, 12):
                ms = []
                for it in range(6):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.flac_encode_device([i.data_ptr() for i in ins], n, RATE, bits, [o.data_ptr() for o in outs], [cap] * NB, got.data_ptr(),
                                           hip_stream=stream, lpc=lpc)
                    e1.record()
                    torch.cuda.synchronize()
                    if it:
                        ms.append(e0.elapsed_time(e1))
                total = int(got.sum())
                base = total if lpc == 0 else base
                print(f"{name} | {bits} bits | flac_lpc {lpc:2d} | {med(ms)} ms | bytes {total}"
                      f" = {total / base:.3f} of flac_lpc 0 = {total / (NB * n * 2 * bits // 8):.3f} of PCM", flush=True)
            del outs
    eng.close()


def walls_child(tag):
    pkg = ge.load_package()
    n = SECONDS * RATE
    has_lpc = hasattr(pkg.hip_lib(), "umx_hip_separate_tracks_flac_lpc")
    forms = [("plain fp32 (_flac call, bits 0)", 0, None), ("FLAC16 (_flac call)", 16, None), ("FLAC24 (_flac call)", 24, None)]
    if has_lpc:
        forms += [(f"FLAC{b} flac_lpc {l:2d} (_flac_lpc call)", b, l) for b in (16, 24) for l in (4, 12)]
    outs = {0: [np.zeros(2 * n, np.float32) for _ in range(4)]}
    for b in (16, 24):
        outs[b] = [np.zeros(pkg.flac_bound(n, b), np.uint8) for _ in range(4)]
    io = pkg.sample_io()
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(1024, seed=7), 1024)
        engines = [("carry, 1 lane  ", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES), 0),
                   ("reset, 14 lanes", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES, tracks=RESET_LANES), FLAG_RESET)]
    for name, x in inputs(pkg, n).items():
        track = np.ascontiguousarray(x.T)
        for mode, e, flags in engines:
            for what, bits, lpc in forms:
                au, out = (C.c_void_p * 1)(track.ctypes.data), (C.c_void_p * 4)(*[o.ctypes.data for o in outs[bits]])
                ln, sh = (C.c_int * 1)(n), (C.c_int * 1)(SHIFT)
                cap, got = (C.c_size_t * 4)(*[o.nbytes for o in outs[bits]]), (C.c_size_t * 4)()
                head = (e.h, 1, au, ln, None, sh, 4, None, out, flags, C.byref(io), pkg.CLIP_CLAMP, None, None, None, pkg.TRUE_PEAK_OFF, None, bits, cap, got)
                ms = []
                for it in range(9):
                    t0 = time.perf_counter()
                    rc = e.lib.umx_hip_separate_tracks_flac(*head, None, None) if lpc is None else e.lib.umx_hip_separate_tracks_flac_lpc(*head, lpc, None, None)
                    dt = time.perf_counter() - t0
                    assert rc == 0, e.last_error()
                    if it >= 2:
                        ms.append(dt * 1e3)
                total = sum(got)
                tail = f"  bytes {total} = {total / (4 * n * 2 * bits // 8):.3f} of PCM" if bits else ""
                print(f"{tag:<7} | {name} | {mode} | {what:<36} {med(ms)}{tail}", flush=True)
    for _, e, _ in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", default=None, help="(the fresh processes) the tag of the tree UMX_TIMING_ROOT names")
    a = ap.parse_args()
    if a.child:
        return walls_child(a.child)
    if a.kernel:
        kernel_main()
    if a.walls:
        for tag, root in [("parent1", a.parent_root), ("pr1", None), ("parent2", a.parent_root), ("pr2", None)]:
            if tag.startswith("parent") and not root:
                continue
            env = {k: v for k, v in os.environ.items() if k not in ("UMX_HIP_LIB", "UMX_TIMING_ROOT")}
            if root:
                env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
            subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", tag], env=env, check=True, timeout=500)


if __name__ == "__main__":
    main()
