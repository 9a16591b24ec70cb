"""umx.cpp_amd -- MI355X-native Open-Unmix (UMX-L) segment inference, drop-in for sevagh/umx.cpp's
src/inference.cpp hot path.

Python is plumbing only: this module is a ctypes view of the C-ABI in include/umx_hip.h (HIP
kernels, gfx950) and include/umx_host.h (C++17 host: ggml loader, wav I/O, segment drivers).
There is NO CPU fallback: if libumx_hip.so is missing or no GPU is present, construction fails
loudly.  The directory name has a dot, so import it with `__graft_entry__.load_package()`.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from . import ggml  # noqa: F401  (weight-file format + synthetic inputs)

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
NB, CROP, KX, NOUT, NFFT, HOP = 2049, 1487, 2976, 4098, 4096, 1024
SEGMENT_SAMPLES = 60 * 44100  # inference.hpp:13 x dsp.hpp:16

UMX_OK, ERR_ARG, ERR_HIP, ERR_MODEL, ERR_TIMEOUT, ERR_NODEVICE = 0, 1, 2, 3, 4, 5
HOST_ERR_AUDIO = 12  # include/umx_host.h: unsupported sample rate / channel count / encoding
DTYPE_F32, DTYPE_U8, DTYPE_U16 = 0, 1, 2
FLAG_NO_WIENER = 0x1
FLAG_SOFTMASK = 0x2  # first estimates X g_j / (eps + sum g), g = mask |X| (Open-Unmix's softmask=True)
FLAG_LSTM_STEPWISE = 0x10
FLAG_DEBUG_TAPS = 0x20
FLAG_LSTM_FORCE_SAFE = 0x40
FLAG_LSTM_PROFILE = 0x80
FLAG_PRECISE_ACT = 0x1000
FLAG_DEBUG_LSTM_ABORT = 0x2000
FLAG_RESIDUAL = 0x8000  # the lowest skipped target's slot carries "everything else" (Open-Unmix's residual=True)
FLAG_RESET_SEGMENTS = 0x4000  # whole-track calls: every segment from a zero LSTM state, segments as lanes of one call (declared deviation)


def FLAG_SKIP_TARGET(t):
    return 0x100 << t


FLAG_WIENER_ITERS_MASK = 0xF0000
TARGET_NAMES = ("bass", "drums", "other", "vocals")  # convert-umx-pth-to-ggml.py:104


def flags_for_targets(names, residual=False, softmask=False):
    """The flag word of Open-Unmix's Separator(targets=names, residual=residual, softmask=softmask): every target not named is
    skipped; with `residual` the lowest skipped slot (residual_slot) carries the rest of the mix; with `softmask` the first estimates
    are the soft-masked ones (FLAG_SOFTMASK).  ValueError for what the engine refuses."""
    names = list(names)
    for nm in names:
        if nm not in TARGET_NAMES:
            raise ValueError(f"unknown target {nm!r}: one of {', '.join(TARGET_NAMES)}")
    if not names:
        raise ValueError("no targets")
    flags = 0
    for t, nm in enumerate(TARGET_NAMES):
        if nm not in names:
            flags |= FLAG_SKIP_TARGET(t)
    if residual:
        flags |= FLAG_RESIDUAL
        if residual_slot(flags) < 0:
            raise ValueError("a residual needs one to three of the four targets: it takes the slot of a target that does not run")
    if softmask:
        flags |= FLAG_SOFTMASK
    return flags


def residual_slot(flags):
    """umx_hip_residual_slot: the slot that carries the residual source; -1 without FLAG_RESIDUAL, -2 for a refused combination."""
    return int(hip_lib().umx_hip_residual_slot(int(flags)))


def FLAG_WIENER_ITERS(n):
    """Wiener EM iterations per call (wiener.cpp:175; Open-Unmix's niter): 1 .. 15, flag bits 16-19."""
    if not 1 <= int(n) <= 15:
        raise ValueError(f"Wiener EM iterations must be 1 .. 15, not {n}")
    return int(n) << 16


_fp = C.POINTER(C.c_float)


class QueueJob(C.Structure):
    """include/umx_hip.h: umx_queue_job's members up to `tag` (the whole record: QueueJobRate)"""
    _fields_ = [("audio", _fp), ("length", C.c_int), ("shift_offset", C.c_int), ("out", _fp * 4), ("tag", C.c_void_p)]


class QueueJobRate(QueueJob):
    """umx_queue_job as it is since DESIGN 23: QueueJob's members (its layout up to `tag`: tests/test_queue_cpu.py pins that part) and
    `rate` behind them.  The callbacks receive this record; the engine zeroes it before `next`, so rate stays 0 = 44.1 kHz unless set."""
    _fields_ = [("rate", C.c_int)]


class SampleIO(C.Structure):
    """include/umx_hip.h: umx_sample_io"""
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int), ("dither", C.c_int), ("dither_seed", C.c_uint)]


SAMPLE_F32, SAMPLE_S16 = 0, 1  # UMX_SAMPLE_*: the formats of the host buffers of the whole-track calls
SAMPLE_S24 = 3  # packed 24-bit PCM, 6 bytes per stereo frame; 2 stays an unknown format
_i16p = C.POINTER(C.c_int16)
_u8p = C.POINTER(C.c_uint8)

QUEUE_NEXT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(QueueJobRate))
QUEUE_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(QueueJobRate))

CLIP_CLAMP, CLIP_RESCALE = 0, 1  # UMX_CLIP_*: what a whole-track call does with outputs beyond full scale


class LevelsAcc(C.Structure):
    """include/umx_hip.h: umx_levels_acc, the record the measuring launches accumulate into"""
    _fields_ = [("peak_bits", C.c_uint * 4), ("over_unity", C.c_ulonglong * 4), ("clipped", C.c_ulonglong * 4),
                ("nonfinite", C.c_ulonglong * 4)]


class Levels(C.Structure):
    """include/umx_hip.h: umx_levels, what a whole-track call reports per track"""
    _fields_ = [("peak", C.c_float * 4), ("gain", C.c_float), ("n_out", C.c_int), ("over_unity", C.c_ulonglong * 4),
                ("clipped", C.c_ulonglong * 4), ("nonfinite", C.c_ulonglong * 4)]

    def as_dict(self):
        n = self.n_out
        return {"peak": np.array(self.peak[:n], np.float32), "gain": np.float32(self.gain), "over_unity": list(self.over_unity[:n]),
                "clipped": list(self.clipped[:n]), "nonfinite": list(self.nonfinite[:n])}


QUEUE_LEVELS_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(QueueJobRate), C.POINTER(Levels))


class Loudness(C.Structure):
    """include/umx_hip.h: umx_loudness, the BS.1770-4 / R128 loudness of a track's outputs"""
    _fields_ = [("integrated", C.c_double * 4), ("momentary_max", C.c_double * 4), ("blocks", C.c_longlong * 4),
                ("gated", C.c_longlong * 4), ("hops", C.c_longlong), ("n_out", C.c_int), ("hop", C.c_int)]

    def as_dict(self):
        n = self.n_out
        return {"integrated": np.array(self.integrated[:n]), "momentary_max": np.array(self.momentary_max[:n]),
                "blocks": list(self.blocks[:n]), "gated": list(self.gated[:n]), "hops": int(self.hops), "hop": int(self.hop)}


_dp = C.POINTER(C.c_double)
QUEUE_LOUDNESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(QueueJobRate), C.POINTER(Levels), C.POINTER(Loudness), _dp)


TRUE_PEAK_OFF, TRUE_PEAK_MEASURE, TRUE_PEAK_RESCALE = 0, 1, 2  # UMX_TRUE_PEAK_*: whether the true peak of what leaves is measured
_up = C.POINTER(C.c_uint)


class TruePeak(C.Structure):
    """include/umx_hip.h: umx_true_peak, the true peak (linear; dBTP = 20 log10) of a track's outputs"""
    _fields_ = [("true_peak", C.c_float * 4), ("n_out", C.c_int), ("factor", C.c_int)]

    def as_dict(self):
        return {"true_peak": np.array(self.true_peak[:self.n_out], np.float32), "factor": int(self.factor)}


QUEUE_TRUE_PEAK_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(QueueJobRate), C.POINTER(Levels), C.POINTER(Loudness), _dp, C.POINTER(TruePeak))


class TensorView(C.Structure):
    """include/umx_hip.h: umx_tensor_view"""
    _fields_ = [("name", C.c_char_p), ("target", C.c_int), ("dtype", C.c_int), ("n_dims", C.c_int),
                ("ne", C.c_int * 2), ("scale", C.c_float), ("offset", C.c_float), ("data", C.c_void_p)]


class UmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"umx_hip error {code}: {msg}")
        self.code = code


def build(verbose=False):
    """Compile every native library in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", str(HERE), "all"], stdout=out)


_hip = None


def hip_lib():
    """Load libumx_hip.so (fails loudly: the product has no other compute path)."""
    global _hip
    if _hip is not None:
        return _hip
    try:  # if torch is going to be used in this process it must bring ITS HIP runtime in first: loading
        import torch  # the system libamdhip64 before torch's own copy makes torch report "No HIP GPUs"
        torch.cuda.is_available()
    except Exception:  # noqa: BLE001 - torch is optional plumbing
        pass
    path = Path(os.environ.get("UMX_HIP_LIB", HERE / "libumx_hip.so"))  # override = kernel-variant A/B runs
    if not path.exists():
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(str(path))
    lib.umx_hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(TensorView), C.c_int]
    lib.umx_hip_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(TensorView), C.c_int,
                                      C.c_uint]
    lib.umx_hip_create_tracks.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(TensorView), C.c_int,
                                          C.c_uint, C.c_int]
    lib.umx_hip_n_tracks.argtypes = [C.c_void_p]
    lib.umx_hip_pipeline_depth.argtypes = [C.c_void_p]
    lib.umx_hip_lstm_is_batched.argtypes = [C.c_void_p]
    lib.umx_hip_debug_f16_bits.argtypes = [C.c_float]
    lib.umx_hip_debug_f16_bits.restype = C.c_uint
    lib.umx_hip_debug_quant_centre.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    lib.umx_hip_debug_quant_centre.restype = C.c_int
    lib.umx_hip_debug_quant_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    lib.umx_hip_debug_quant_planes.restype = C.c_int
    lib.umx_hip_track_stream_reset.argtypes = [C.c_void_p, C.c_int]
    lib.umx_hip_track_stream_get.argtypes = [C.c_void_p, C.c_int, _fp]
    lib.umx_hip_track_stream_set.argtypes = [C.c_void_p, C.c_int, _fp]
    lib.umx_hip_infer_segment_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_uint]
    lib.umx_hip_infer_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_uint]
    lib.umx_hip_infer_batch_async.argtypes = lib.umx_hip_infer_batch.argtypes
    lib.umx_hip_infer_batch_device.argtypes = lib.umx_hip_infer_batch.argtypes
    lib.umx_hip_order_after.argtypes = [C.c_void_p, C.c_void_p]
    lib.umx_hip_order_before.argtypes = [C.c_void_p, C.c_void_p]
    lib.umx_hip_weight_bytes.restype = C.c_size_t
    lib.umx_hip_weight_bytes.argtypes = [C.c_void_p]
    lib.umx_hip_destroy.argtypes = [C.c_void_p]
    lib.umx_hip_last_error.restype = C.c_char_p
    lib.umx_hip_last_error.argtypes = [C.c_void_p]
    lib.umx_hip_stream_floats.restype = C.c_size_t
    lib.umx_hip_stream_floats.argtypes = [C.c_void_p]
    lib.umx_hip_stream_reset.argtypes = [C.c_void_p]
    lib.umx_hip_stream_get.argtypes = [C.c_void_p, _fp]
    lib.umx_hip_stream_set.argtypes = [C.c_void_p, _fp]
    lib.umx_hip_infer_segment.argtypes = [C.c_void_p, _fp, C.c_int, C.POINTER(_fp), C.c_uint]
    lib.umx_hip_infer_segment_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_uint]
    lib.umx_hip_sync.argtypes = [C.c_void_p]
    lib.umx_hip_stream_handle.restype = C.c_void_p
    lib.umx_hip_stream_handle.argtypes = [C.c_void_p]
    lib.umx_hip_nb_frames.argtypes = [C.c_void_p]
    lib.umx_hip_segment_samples.argtypes = [C.c_void_p]
    lib.umx_hip_hidden.argtypes = [C.c_void_p]
    lib.umx_hip_read_tap.restype = C.c_long
    lib.umx_hip_read_tap.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _fp, C.c_size_t]
    lib.umx_hip_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), _fp, C.c_int]
    lib.umx_hip_stage_times_slot.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), _fp, C.c_int]
    lib.umx_hip_stage_kernel_times_slot.argtypes = [C.c_void_p, C.c_int, _fp, C.c_int]
    lib.umx_hip_lstm_was_persistent.argtypes = [C.c_void_p]
    lib.umx_hip_lstm_mode.argtypes = [C.c_void_p]
    lib.umx_hip_debug_lstm_profile.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    lib.umx_hip_debug_wiener_bins.argtypes = [C.c_int, _fp, _fp, _fp, C.c_float, _fp]
    lib.umx_hip_debug_gate_math.argtypes = [C.c_int, _fp, _fp, C.c_int, _fp, _fp, _fp]
    lib.umx_hip_lstm_kernel_name.restype = C.c_char_p
    lib.umx_hip_lstm_kernel_name.argtypes = [C.c_void_p]
    lib.umx_hip_gemm_kernel_name.restype = C.c_char_p
    lib.umx_hip_gemm_kernel_name.argtypes = [C.c_void_p, C.c_int]
    lib.umx_hip_debug_lstm_placement.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    lib.umx_hip_stream_layer_floats.restype = C.c_size_t
    lib.umx_hip_stream_layer_floats.argtypes = [C.c_void_p]
    lib.umx_hip_stream_get_layer.argtypes = [C.c_void_p, C.c_int, _fp]
    lib.umx_hip_stream_set_layer.argtypes = [C.c_void_p, C.c_int, _fp]
    lib.umx_hip_segment_begin.argtypes = [C.c_void_p, _fp, C.c_int, C.c_uint]
    lib.umx_hip_segment_lstm_layer.argtypes = [C.c_void_p, C.c_int]
    lib.umx_hip_segment_end.argtypes = [C.c_void_p, C.POINTER(_fp)]
    lib.umx_hip_segment_begin_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
    lib.umx_hip_segment_end_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.umx_hip_segment_masks_device.argtypes = [C.c_void_p]
    lib.umx_hip_segment_residual_device.argtypes = [C.c_void_p]
    lib.umx_hip_residual_slot.argtypes = [C.c_uint]
    lib.umx_hip_segment_finish_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.umx_hip_weight_stems_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.umx_hip_track_accumulate_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_int,
                                                    C.c_int, C.c_void_p]
    lib.umx_hip_track_normalise_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p]
    lib.umx_hip_debug_lds_guard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint)]
    lib.umx_hip_split_inference.argtypes = [C.c_void_p, _fp, C.c_int, C.POINTER(_fp), C.c_uint, C.c_void_p, C.c_void_p]
    lib.umx_hip_shift_inference.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.POINTER(_fp), C.c_uint, C.c_void_p,
                                            C.c_void_p]
    lib.umx_hip_resampled_length.restype = C.c_longlong
    lib.umx_hip_resampled_length.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.umx_hip_resample_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                            C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.umx_hip_resample_needs.restype = C.c_longlong
    lib.umx_hip_resample_needs.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_longlong]
    lib.umx_hip_resample_ready.restype = C.c_longlong
    lib.umx_hip_resample_ready.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_longlong]
    lib.umx_hip_resample_range_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                                  C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.umx_hip_debug_resample_launches.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.umx_hip_shift_inference_rate.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(_fp), C.c_uint, C.c_void_p,
                                                 C.c_void_p]
    lib.umx_hip_debug_resample_taps.argtypes = [C.c_int, C.c_int, _fp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                C.POINTER(C.c_int)]
    lib.umx_hip_ensemble_offsets.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.umx_hip_shift_ensemble.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_fp), C.c_uint,
                                           C.c_void_p, C.c_void_p]
    lib.umx_hip_debug_shift_mean_ms.restype = C.c_float
    lib.umx_hip_debug_shift_mean_ms.argtypes = [C.c_void_p]
    lib.umx_hip_mix_columns.argtypes = [C.c_int, _fp]
    lib.umx_hip_shift_ensemble_mix.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _fp, C.POINTER(_fp),
                                               C.c_uint, C.c_void_p, C.c_void_p]
    lib.umx_hip_mix_stems_device.argtypes = [C.c_void_p, C.c_int, _fp, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                             C.c_void_p]
    lib.umx_hip_queue_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.umx_hip_debug_queue_calls.argtypes = [C.c_void_p]
    lib.umx_hip_pcm16_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.umx_hip_pcm16_encode_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(SampleIO),
                                                C.POINTER(C.c_void_p), C.c_void_p]
    lib.umx_hip_pcm16_decode_host.argtypes = [_i16p, C.c_longlong, _fp]
    lib.umx_hip_pcm16_encode_host.argtypes = [_fp, C.c_int, C.c_int, C.c_longlong, C.POINTER(SampleIO), _i16p]
    lib.umx_hip_pcm24_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.umx_hip_pcm24_encode_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(SampleIO),
                                                C.POINTER(C.c_void_p), C.c_void_p]
    lib.umx_hip_pcm24_encode_rescaled_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(SampleIO),
                                                         C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
    lib.umx_hip_pcm24_decode_host.argtypes = [_u8p, C.c_longlong, _fp]
    lib.umx_hip_pcm24_encode_host.argtypes = [_fp, C.c_int, C.c_int, C.c_longlong, C.POINTER(SampleIO), _u8p]
    lib.umx_hip_levels_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(SampleIO), C.c_void_p,
                                          C.c_void_p]
    lib.umx_hip_pcm16_encode_rescaled_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_longlong, C.POINTER(SampleIO),
                                                         C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
    lib.umx_hip_rescale_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
    lib.umx_hip_levels_host.argtypes = [_fp, C.c_int, C.c_int, C.c_longlong, C.POINTER(SampleIO), C.c_float, C.POINTER(LevelsAcc)]
    lib.umx_hip_rescale_gain.argtypes = [_fp, C.c_int]
    lib.umx_hip_rescale_gain.restype = C.c_float
    lib.umx_hip_kweight_hops_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_longlong, C.c_longlong,
                                                C.c_void_p, C.c_void_p]
    lib.umx_hip_kweight_coeffs.argtypes = [C.c_int, _dp, _dp, _dp, _dp]
    lib.umx_hip_kweight_hops_host.argtypes = [_fp, C.c_int, C.c_int, C.c_longlong, C.c_longlong, _dp]
    lib.umx_hip_loudness_gate.argtypes = [_dp, C.c_longlong, C.c_int, _dp, _dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.umx_hip_true_peak_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_longlong, C.c_longlong,
                                             C.c_void_p, C.c_void_p]
    lib.umx_hip_true_peak_taps.argtypes = [C.c_int, _fp, C.POINTER(C.c_int)]
    lib.umx_hip_true_peak_host.argtypes = [_fp, C.c_int, C.c_int, C.c_longlong, C.c_longlong, _up]
    # The whole-track ladder, from one prefix: context, n_tracks, audio, lengths[, rates], shift offsets[, n_out, gains], outputs,
    # flags -- then what a rung adds -- then progress and its user pointer.  The queue entry points likewise.
    def tracks_args(ptr, rate=True, mix=True):
        return ([C.c_void_p, C.c_int, C.POINTER(ptr), C.POINTER(C.c_int)] + [C.POINTER(C.c_int)] * (2 if rate else 1)
                + ([C.c_int, _fp] if mix else []) + [C.POINTER(ptr), C.c_uint])

    progress = [C.c_void_p, C.c_void_p]
    wide = tracks_args(C.c_void_p) + [C.POINTER(SampleIO)]
    lib.umx_hip_separate_tracks.argtypes = tracks_args(_fp, rate=False, mix=False) + progress
    lib.umx_hip_separate_tracks_rate.argtypes = tracks_args(_fp, mix=False) + progress
    lib.umx_hip_separate_tracks_mix.argtypes = tracks_args(_fp) + progress
    lib.umx_hip_separate_tracks_io.argtypes = wide + progress
    lib.umx_hip_separate_tracks_levels.argtypes = wide + [C.c_int, C.POINTER(Levels)] + progress
    lib.umx_hip_separate_tracks_loudness.argtypes = wide + [C.c_int, C.POINTER(Levels), C.POINTER(Loudness), C.POINTER(C.c_void_p)] + progress
    lib.umx_hip_separate_tracks_true_peak.argtypes = (wide + [C.c_int, C.POINTER(Levels), C.POINTER(Loudness), C.POINTER(C.c_void_p), C.c_int,
                                                              C.POINTER(TruePeak)] + progress)

    def queue_args(done_fn):
        return [C.c_void_p, QUEUE_NEXT_FN, done_fn, C.c_void_p, C.c_int, _fp, C.c_uint]

    lib.umx_hip_separate_queue.argtypes = queue_args(QUEUE_DONE_FN)
    lib.umx_hip_separate_queue_io.argtypes = queue_args(QUEUE_DONE_FN) + [C.POINTER(SampleIO)]
    lib.umx_hip_separate_queue_levels.argtypes = queue_args(QUEUE_LEVELS_FN) + [C.POINTER(SampleIO), C.c_int]
    lib.umx_hip_separate_queue_loudness.argtypes = queue_args(QUEUE_LOUDNESS_FN) + [C.POINTER(SampleIO), C.c_int]
    lib.umx_hip_separate_queue_true_peak.argtypes = queue_args(QUEUE_TRUE_PEAK_FN) + [C.POINTER(SampleIO), C.c_int, C.c_int]
    _hip = lib
    return lib


CREATE_QUANTISED_RESIDENT = 0x1
CREATE_GEMM_F32 = 0x4
CREATE_DEQUANTISE_AT_LOAD = 0x8
CREATE_LSTM_BATCHED = 0x10
CREATE_U8_DEQUANT = 0x20
CREATE_GEMM_STAGED = 0x40
CREATE_GEMM_PLANES = 0x80
MAX_TRACKS = 64
MAX_SHIFTS = MAX_TRACKS  # umx_hip_shift_ensemble: one shift per track lane
MAX_MIX_OUTPUTS, MIX_COLUMNS, MIX_COLUMN_MIXTURE = 4, 5, 4  # the stem mix matrix: rows of gains over 4 stem slots + the mixture
MODEL_RATE = 44100
RESAMPLE_MIN_RATE, RESAMPLE_MAX_RATE = 8000, 192000

HIP_SYMBOLS = ["umx_hip_create", "umx_hip_create_ex", "umx_hip_create_tracks", "umx_hip_n_tracks", "umx_hip_lstm_is_batched",
               "umx_hip_track_stream_reset", "umx_hip_track_stream_get", "umx_hip_track_stream_set",
               "umx_hip_infer_segment_async", "umx_hip_infer_batch", "umx_hip_infer_batch_async",
               "umx_hip_infer_batch_device", "umx_hip_order_after", "umx_hip_order_before",
               "umx_hip_separate_tracks", "umx_hip_phase_stream", "umx_hip_stream_state_device", "umx_hip_segment_begin_device", "umx_hip_segment_end_device",
               "umx_hip_weight_stems_device", "umx_hip_track_accumulate_device", "umx_hip_track_normalise_device", "umx_hip_weight_bytes", "umx_hip_destroy", "umx_hip_last_error", "umx_hip_stream_floats",
               "umx_hip_stream_reset", "umx_hip_stream_get", "umx_hip_stream_set", "umx_hip_infer_segment",
               "umx_hip_infer_segment_device", "umx_hip_sync", "umx_hip_stream_handle", "umx_hip_nb_frames",
               "umx_hip_segment_samples", "umx_hip_hidden", "umx_hip_read_tap", "umx_hip_stage_times",
               "umx_hip_stage_times_slot", "umx_hip_stage_kernel_times_slot",
               "umx_hip_lstm_was_persistent", "umx_hip_lstm_mode", "umx_hip_lstm_kernel_name", "umx_hip_gemm_kernel_name", "umx_hip_debug_wiener_bins", "umx_hip_debug_gate_math", "umx_hip_debug_lstm_profile", "umx_hip_debug_lstm_placement",
               "umx_hip_stream_layer_floats", "umx_hip_stream_get_layer", "umx_hip_stream_set_layer",
               "umx_hip_segment_begin", "umx_hip_segment_lstm_layer", "umx_hip_segment_end",
               "umx_hip_split_inference", "umx_hip_shift_inference", "umx_hip_debug_lds_guard", "umx_hip_debug_f16_bits", "umx_hip_debug_quant_centre", "umx_hip_debug_quant_planes",
               "umx_hip_segment_masks_device", "umx_hip_target_mag_device", "umx_hip_segment_finish_device", "umx_hip_gate_reserve", "umx_hip_segment_discard", "umx_hip_pipeline_depth",
               "umx_hip_resampled_length", "umx_hip_resample_device", "umx_hip_shift_inference_rate", "umx_hip_separate_tracks_rate",
               "umx_hip_debug_resample_taps", "umx_hip_residual_slot", "umx_hip_segment_residual_device",
               "umx_hip_ensemble_offsets", "umx_hip_shift_ensemble", "umx_hip_debug_shift_mean_ms",
               "umx_hip_mix_columns", "umx_hip_separate_tracks_mix", "umx_hip_shift_ensemble_mix", "umx_hip_mix_stems_device",
               "umx_hip_separate_queue", "umx_hip_queue_plan", "umx_hip_debug_queue_calls",
               "umx_hip_separate_tracks_io", "umx_hip_separate_queue_io", "umx_hip_pcm16_decode_device", "umx_hip_pcm16_encode_device",
               "umx_hip_pcm16_decode_host", "umx_hip_pcm16_encode_host",
               "umx_hip_separate_tracks_levels", "umx_hip_separate_queue_levels", "umx_hip_levels_device",
               "umx_hip_pcm16_encode_rescaled_device", "umx_hip_rescale_device", "umx_hip_levels_host", "umx_hip_rescale_gain",
               "umx_hip_separate_tracks_loudness", "umx_hip_separate_queue_loudness", "umx_hip_kweight_hops_device",
               "umx_hip_kweight_coeffs", "umx_hip_kweight_hops_host", "umx_hip_loudness_gate",
               "umx_hip_resample_needs", "umx_hip_resample_ready", "umx_hip_resample_range_device", "umx_hip_debug_resample_launches",
               "umx_hip_pcm24_decode_device", "umx_hip_pcm24_encode_device", "umx_hip_pcm24_encode_rescaled_device",
               "umx_hip_pcm24_decode_host", "umx_hip_pcm24_encode_host",
               "umx_hip_separate_tracks_true_peak", "umx_hip_separate_queue_true_peak", "umx_hip_true_peak_device",
               "umx_hip_true_peak_taps", "umx_hip_true_peak_host"]


def sample_io(in_format=SAMPLE_F32, out_format=SAMPLE_F32, dither_seed=None):
    """A umx_sample_io: dither_seed None = no dither, else TPDF dither with that seed."""
    return SampleIO(int(in_format), int(out_format), 0 if dither_seed is None else 1, 0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFF)


def pcm16_decode_host(q):
    """umx_hip_pcm16_decode_host: int16 array -> float32 array of the same shape, x = q / 32767 (no GPU)."""
    q = np.ascontiguousarray(q, np.int16)
    x = np.empty(q.shape, np.float32)
    rc = hip_lib().umx_hip_pcm16_decode_host(q.ctypes.data_as(_i16p), q.size, x.ctypes.data_as(_fp))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_pcm16_decode_host")
    return x


def _encode_host(fmt, x, buffer, first_frame, dither_seed):
    """umx_hip_pcm<fmt>_encode_host (fmt: 16 or 24) of a (2,n) float32 x -> the n frames as the format holds them: (n,2) int16, or 6 n bytes."""
    a = np.ascontiguousarray(np.asarray(x, np.float32).T)
    q, qp, out_format = {16: (np.empty(a.shape, np.int16), _i16p, SAMPLE_S16), 24: (np.empty(6 * a.shape[0], np.uint8), _u8p, SAMPLE_S24)}[fmt]
    io = sample_io(SAMPLE_F32, out_format, dither_seed)
    name = f"umx_hip_pcm{fmt}_encode_host"
    rc = getattr(hip_lib(), name)(a.ctypes.data_as(_fp), a.shape[0], int(buffer), int(first_frame), C.byref(io), q.ctypes.data_as(qp))
    if rc != UMX_OK:
        raise UmxError(rc, name)
    return q


def pcm16_encode_host(x, buffer=0, first_frame=0, dither_seed=None):
    """umx_hip_pcm16_encode_host: (2,n) float32 -> (2,n) int16 as output buffer `buffer` of a call, frame 0 of x being frame
    first_frame of the track (no GPU)."""
    return np.ascontiguousarray(_encode_host(16, x, buffer, first_frame, dither_seed).T)


def pcm24_pack(q):
    """(2,L) int32 codes of -8388608 .. 8388607 -> the 6 L bytes of L packed stereo frames (uint8): 3 bytes per sample, little-endian,
    L then R, as a 24-bit WAV data chunk holds them."""
    a = np.ascontiguousarray(np.asarray(q, np.int32).T)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("pcm24_pack: need a (2, L) array")
    if a.size and (a.min() < -8388608 or a.max() > 8388607):
        raise ValueError("pcm24_pack: codes outside -8388608 .. 8388607")
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).ravel()


def pcm24_unpack(b):
    """The bytes of L packed stereo frames (uint8, 6 L of them) -> (2,L) int32 codes."""
    b = np.ascontiguousarray(b, np.uint8).ravel()
    if b.size % 6:
        raise ValueError("pcm24_unpack: need a multiple of 6 bytes")
    w = np.zeros((b.size // 3, 4), np.uint8)
    w[:, 1:] = b.reshape(-1, 3)
    return np.ascontiguousarray((w.view("<i4").ravel().astype(np.int32) >> 8).reshape(-1, 2).T)


def pcm24_decode_host(q):
    """umx_hip_pcm24_decode_host: int32 codes (any shape) -> float32 array of the same shape, x = q / 2^23, through the packed bytes
    (no GPU)."""
    q = np.ascontiguousarray(q, np.int32)
    b = np.ascontiguousarray(q.ravel().astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).ravel()  # 3 bytes per sample
    x = np.empty(q.shape, np.float32)
    rc = hip_lib().umx_hip_pcm24_decode_host(b.ctypes.data_as(_u8p), q.size, x.ctypes.data_as(_fp))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_pcm24_decode_host")
    return x


def pcm24_encode_host(x, buffer=0, first_frame=0, dither_seed=None):
    """umx_hip_pcm24_encode_host: (2,n) float32 -> (2,n) int32 codes as output buffer `buffer` of a call, frame 0 of x being frame
    first_frame of the track (no GPU)."""
    return pcm24_unpack(_encode_host(24, x, buffer, first_frame, dither_seed))


def levels_host(x, buffer=0, first_frame=0, io=None, clip_divisor=1.0, acc=None):
    """umx_hip_levels_host: the levels of a (2,n) float32 array as output buffer `buffer` of a call, accumulated into the LevelsAcc
    `acc` (None: a fresh one), which is returned; clipped is counted for an io with a SAMPLE_S16 or SAMPLE_S24 output, on x / clip_divisor (no GPU)."""
    a = np.ascontiguousarray(np.asarray(x, np.float32).T)
    acc = LevelsAcc() if acc is None else acc
    rc = hip_lib().umx_hip_levels_host(a.ctypes.data_as(_fp), a.shape[0], int(buffer), int(first_frame), None if io is None else C.byref(io),
                                       C.c_float(clip_divisor), C.byref(acc))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_levels_host")
    return acc


def rescale_gain(peaks):
    """umx_hip_rescale_gain: the divisor of a track whose outputs peak at `peaks` (1: nothing is divided), as float32 (no GPU)."""
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(peaks, np.float32)))
    return np.float32(hip_lib().umx_hip_rescale_gain(p.ctypes.data_as(_fp), p.size))


def kweight_coeffs(rate):
    """umx_hip_kweight_coeffs: BS.1770-4's K-weighting at `rate` -> (pb, pa, rb, ra), float64 triples: b and [1, a1, a2] of the shelf
    and of the high-pass stage (no GPU)."""
    c = [(C.c_double * 3)() for _ in range(4)]
    rc = hip_lib().umx_hip_kweight_coeffs(int(rate), *c)
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_kweight_coeffs")
    return tuple(np.array(list(x), np.float64) for x in c)


def kweight_hop_count(n, rate):
    """Whole hops (a tenth of a second: kweight_hop of csrc/loudness.h) in n frames at `rate`; a rate the calls refuse gives any size."""
    return int(n) // max(1, (int(rate) + 5) // 10)


def kweight_hops_host(x, rate, first_hop=0, n_hops=None):
    """umx_hip_kweight_hops_host: the K-weighted hop energies of a (2,n) float32 array by the rule of DESIGN 21 -> (2, n // hop)
    float64; hops outside [first_hop, first_hop + n_hops) stay NaN (no GPU)."""
    a = np.ascontiguousarray(np.asarray(x, np.float32).T)
    hops = a.shape[0] // ((int(rate) + 5) // 10)
    n_hops = hops - first_hop if n_hops is None else n_hops
    E = np.full((2, hops), np.nan)
    rc = hip_lib().umx_hip_kweight_hops_host(a.ctypes.data_as(_fp), a.shape[0], int(rate), int(first_hop), int(n_hops), E.ctypes.data_as(_dp))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_kweight_hops_host")
    return E


def loudness_gate(E, hop):
    """umx_hip_loudness_gate: blocks and gates over one output's hop energies E (2, hops) -> (integrated LUFS, momentary_max LUFS,
    blocks, gated) (no GPU)."""
    E = np.ascontiguousarray(np.asarray(E, np.float64))
    assert E.ndim == 2 and E.shape[0] == 2
    i, m, b, g = C.c_double(), C.c_double(), C.c_longlong(), C.c_longlong()
    rc = hip_lib().umx_hip_loudness_gate(E.ctypes.data_as(_dp), E.shape[1], int(hop), C.byref(i), C.byref(m), C.byref(b), C.byref(g))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_loudness_gate")
    return i.value, m.value, b.value, g.value


def true_peak_taps(rate):
    """umx_hip_true_peak_taps: the 49 float32 taps of the true-peak interpolator at `rate` and its oversampling factor (no GPU)."""
    h, f = np.empty(49, np.float32), C.c_int()
    rc = hip_lib().umx_hip_true_peak_taps(int(rate), h.ctypes.data_as(_fp), C.byref(f))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_true_peak_taps")
    return h, f.value


def true_peak_host(x, rate, first_frame=0, n_frames=None, bits=0):
    """umx_hip_true_peak_host: the true peak of frames [first_frame, first_frame + n_frames) of a (2,n) float32 array by the rule of
    DESIGN 26, as the maximum with the bit pattern `bits` -> the bit pattern (np.uint32; its float: true_peak_float) (no GPU)."""
    a = np.ascontiguousarray(np.asarray(x, np.float32).T)
    n_frames = a.shape[0] - first_frame if n_frames is None else n_frames
    b = C.c_uint(int(bits))
    rc = hip_lib().umx_hip_true_peak_host(a.ctypes.data_as(_fp), a.shape[0], int(rate), int(first_frame), int(n_frames), C.byref(b))
    if rc != UMX_OK:
        raise UmxError(rc, "umx_hip_true_peak_host")
    return np.uint32(b.value)


def true_peak_float(bits):
    """The float32 whose bit pattern a true-peak word holds."""
    return np.array([bits], np.uint32).view(np.float32)[0]


def resampled_length(n, rate_in, rate_out):
    """ceil(n L / M), the natural output length of the device resampler (host arithmetic; < 0 for a bad rate)."""
    return int(hip_lib().umx_hip_resampled_length(int(n), int(rate_in), int(rate_out)))


def resample_needs(n_out_wanted, rate_in, rate_out, n_in):
    """umx_hip_resample_needs: the leading input frames that outputs [0, n_out_wanted) of the device resampler read (host
    arithmetic; < 0 for a bad rate or a negative count)."""
    return int(hip_lib().umx_hip_resample_needs(int(n_out_wanted), int(rate_in), int(rate_out), int(n_in)))


def resample_ready(n_in_final, rate_in, rate_out, n_in, n_out):
    """umx_hip_resample_ready: the leading output frames whose whole window lies inside the first n_in_final input frames (DESIGN 23;
    host arithmetic; < 0 for a bad rate or a negative count)."""
    return int(hip_lib().umx_hip_resample_ready(int(n_in_final), int(rate_in), int(rate_out), int(n_in), int(n_out)))


def ensemble_offsets(n_shifts, first=None):
    """The default offsets of an n_shifts ensemble (umx_hip_ensemble_offsets): (first + k (22050 // n_shifts)) % 22050; first None =
    the reference's 4033.  Host arithmetic."""
    if not 1 <= int(n_shifts) <= MAX_SHIFTS:
        raise UmxError(ERR_ARG, f"ensemble_offsets: n_shifts must be 1 .. {MAX_SHIFTS}")
    out = (C.c_int * int(n_shifts))()
    rc = hip_lib().umx_hip_ensemble_offsets(int(n_shifts), -1 if first is None else int(first), out)
    if rc != 0:
        raise UmxError(rc, "ensemble_offsets: first must be below 22050")
    return list(out)


def queue_plan(lanes, seg_counts):
    """umx_hip_queue_plan: the track queue's schedule for jobs of seg_counts[j] calls each on `lanes` lanes -> (lane of every job, the
    call every job's first segment runs in, number of calls).  Host arithmetic."""
    counts = [int(c) for c in seg_counts]
    n = len(counts)
    lane, first, calls = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), C.c_int(0)
    rc = hip_lib().umx_hip_queue_plan(int(lanes), n, (C.c_int * max(n, 1))(*counts), lane, first, C.byref(calls))
    if rc != 0:
        raise UmxError(rc, f"queue_plan: need 1 .. {MAX_TRACKS} lanes and at least one job, every job of at least one segment")
    return list(lane)[:n], list(first)[:n], calls.value


def _mix_gains(gains):
    """gains as the C calls take them: (n_out, float32[n_out * 5]) from an (n_out, 5) array-like (no checks: the library refuses)."""
    g = np.ascontiguousarray(np.asarray(gains, np.float32))
    if g.ndim != 2 or g.shape[1] != MIX_COLUMNS:
        raise ValueError("mix gains: need an (n_out, 5) matrix: bass, drums, other, vocals slots and the mixture")
    return g.shape[0], g.ravel()


class _TrackArgs:
    """The marshalling of every whole-track call: a list of (2, L_i) arrays as the C entry points take it.  io: the
    SampleIO of the call or None (int16 arrays where it says SAMPLE_S16, (2,L) int32 codes where it says SAMPLE_S24 -- packed to 6
    bytes a frame here and unpacked again --, else float32); n_out: host buffers per track; ptr: the pointer
    type of the C signature's arrays.  ins / outs: the contiguous (L_i, 2) inputs and the output buffers; a, o, n, sh, rt: the ctypes
    arrays of audio, outputs, lengths, shift offsets (None = -1: no shift) and rates (None: all 44.1 kHz); result(): the outputs as a
    list of [n_out x (2, L_i)]."""

    def __init__(self, waves, io=None, n_out=4, shift_offsets=None, rates=None, ptr=C.c_void_p):
        nt = len(waves)
        fin = SAMPLE_F32 if io is None else io.in_format
        self.fout = SAMPLE_F32 if io is None else io.out_format
        tin = np.int16 if fin == SAMPLE_S16 else np.float32
        tout = np.int16 if self.fout == SAMPLE_S16 else np.float32
        if fin == SAMPLE_S24:
            self.ins = [pcm24_pack(w) for w in waves]
        else:
            self.ins = [np.ascontiguousarray(np.asarray(w, tin).T).ravel() for w in waves]
        self.Ls = [np.asarray(w).shape[1] for w in waves]
        self.n_host = min(max(n_out, 0), MAX_MIX_OUTPUTS)
        if self.fout == SAMPLE_S24:
            self.outs = [[np.empty(6 * L, np.uint8) for _ in range(self.n_host)] for L in self.Ls]
        else:
            self.outs = [[np.empty(2 * L, tout) for _ in range(self.n_host)] for L in self.Ls]
        self.a = (ptr * nt)(*[C.cast(x.ctypes.data, ptr) for x in self.ins])
        self.o = (ptr * max(1, nt * self.n_host))(*[C.cast(x.ctypes.data, ptr) for t in self.outs for x in t])
        self.n = (C.c_int * nt)(*self.Ls)
        self.shifts = [(-1 if s is None else int(s)) for s in (shift_offsets or [None] * nt)]
        self.sh = (C.c_int * nt)(*self.shifts)
        self.rt = None if rates is None else (C.c_int * nt)(*[int(r) for r in rates])

    def result(self):
        if self.fout == SAMPLE_S24:
            return [[pcm24_unpack(x) for x in t] for t in self.outs]
        return [[np.ascontiguousarray(x.reshape(L, 2).T) for x in t] for t, L in zip(self.outs, self.Ls)]


# What a rung of the whole-track ladder adds behind its SampleIO, in the C signature's order: a narrower rung is the
# wider one with the fields it does not have at their neutral values.
_MEASURE_TAIL = {"umx_hip_separate_tracks_io": (),
                 "umx_hip_separate_tracks_levels": ("clip", "levels"),
                 "umx_hip_separate_tracks_loudness": ("clip", "levels", "loudness", "hop_energy"),
                 "umx_hip_separate_tracks_true_peak": ("clip", "levels", "loudness", "hop_energy", "true_peak_mode", "true_peak")}


class _MeasuredCall:
    """One call of a rung of _MEASURE_TAIL, marshalled once: the _TrackArgs `m`, the record arrays lv / ld / tp and the hop-energy
    arrays env (None: not asked for, NULL in the call), and `args`, the C argument tuple with the tail that rung has.  results(): the
    tuple the rung's wrapper returns -- outputs, then one entry per record field of its tail."""

    def __init__(self, entry_name, handle, waves, io, flags, shift_offsets, rates, gains, clip=CLIP_CLAMP, levels=False, loudness=False,
                 envelopes=False, true_peak=TRUE_PEAK_OFF, records=False):
        nt = len(waves)
        self.io = io = sample_io() if io is None else io
        n_out, self.g = (4, None) if gains is None else _mix_gains(gains)
        self.m = m = _TrackArgs(waves, io, n_out, shift_offsets, rates)
        self.lv = (Levels * nt)() if levels else None
        self.ld = (Loudness * nt)() if loudness else None
        self.tp = (TruePeak * nt)() if records else None
        self.env = ep = None
        if envelopes:  # (a rate the call will refuse: any size does)
            self.env = [np.full((m.n_host, 2, kweight_hop_count(L, r)), np.nan) for L, r in zip(m.Ls, rates or [MODEL_RATE] * nt)]
            ep = (C.c_void_p * nt)(*[e.ctypes.data if e.size else None for e in self.env])
        tail = {"clip": int(clip), "levels": self.lv, "loudness": self.ld, "hop_energy": ep, "true_peak_mode": int(true_peak), "true_peak": self.tp}
        self.tail = _MEASURE_TAIL[entry_name]
        self.args = ((handle, nt, m.a, m.n, m.rt, m.sh, n_out, None if self.g is None else self.g.ctypes.data_as(_fp), m.o, flags, C.byref(io))
                     + tuple(tail[f] for f in self.tail) + (None, None))

    def results(self):
        got = {"levels": self.lv, "loudness": self.ld, "true_peak": self.tp}
        return (self.m.result(),) + tuple(self.env if f == "hop_energy" else (None if got[f] is None else list(got[f]))
                                          for f in self.tail if f not in ("clip", "true_peak_mode"))


def mix_columns(gains):
    """umx_hip_mix_columns: the bitmask of the columns of an (n_out, 5) gain matrix with any nonzero gain (bit 4: the mixture).
    Host arithmetic."""
    n_out, g = _mix_gains(gains)
    mask = int(hip_lib().umx_hip_mix_columns(n_out, g.ctypes.data_as(_fp)))
    if mask < 0:
        raise UmxError(ERR_ARG, "mix_columns: need 1 .. 4 rows of five finite gains")
    return mask


def mix_parse(spec, residual_slot=-1):
    """umx_mix_parse: the UMX_MIX grammar ("vocals=vocals;accompaniment=bass+drums+other;karaoke=mix-vocals") ->
    (names, gains (n_out, 5) float32).  residual_slot: the column `residual` stands for (residual_slot(flags)), -1 = refuse it."""
    lib = host_lib()
    n_out = C.c_int(0)
    names = C.create_string_buffer(MAX_MIX_OUTPUTS * 64)
    gains = np.zeros(MAX_MIX_OUTPUTS * MIX_COLUMNS, np.float32)
    err = C.create_string_buffer(256)
    rc = lib.umx_mix_parse(str(spec).encode(), int(residual_slot), C.byref(n_out), names, gains.ctypes.data_as(_fp), err)
    if rc != 0:
        raise HostError(rc, err.value.decode())
    raw = names.raw
    return ([raw[64 * m:64 * (m + 1)].split(b"\0", 1)[0].decode() for m in range(n_out.value)],
            gains.reshape(MAX_MIX_OUTPUTS, MIX_COLUMNS)[:n_out.value].copy())


GATE_FUNCTIONS = ("tanh_epi", "tanh_hw", "sigmoid_hw", "tanhf", "sigmoid_ref")
CELL_FORMS = ("lstm_cell<false>", "lstm_cell_flat", "lstm_cell<true>", "lstm_cell_lane<false>")


def debug_gate_math(x=None, pre=None, c=None):
    """umx_hip_debug_gate_math: x (n,) -> {name of GATE_FUNCTIONS: (n,)}; pre (waves, 64) in the quad layout lane = 4 * unit + gate and
    c (waves, 16) -> {name of CELL_FORMS: (c, h), each (waves, 16)}.  Either half may be left out (None); returns (functions, cells)."""
    lib = hip_lib()
    n = nw = 0
    fn = cell = None
    if x is not None:
        x = np.ascontiguousarray(x, np.float32).ravel()
        n = x.size
        fn = np.empty((5, n), np.float32)
    if pre is not None:
        pre, c = np.ascontiguousarray(pre, np.float32), np.ascontiguousarray(c, np.float32)
        nw = pre.shape[0]
        assert pre.shape == (nw, 64) and c.shape == (nw, 16), (pre.shape, c.shape)
        cell = np.empty((len(CELL_FORMS), nw, 2, 16), np.float32)
    ptr = lambda a: a.ctypes.data_as(_fp) if a is not None and a.size else None  # noqa: E731
    rc = lib.umx_hip_debug_gate_math(n, ptr(x), ptr(fn), nw, ptr(pre), ptr(c), ptr(cell))
    if rc:
        raise UmxError(rc, "umx_hip_debug_gate_math")
    return ({k: fn[i] for i, k in enumerate(GATE_FUNCTIONS)} if n else {},
            {k: (cell[i, :, 0], cell[i, :, 1]) for i, k in enumerate(CELL_FORMS)} if nw else {})


def resample_taps(rate_in, rate_out):
    """The resampler's fp32 tap table of a rate pair: (taps [L][K], first offset -D).  Host only."""
    lib = hip_lib()
    L, K, d0 = C.c_int(), C.c_int(), C.c_int()
    rc = lib.umx_hip_debug_resample_taps(int(rate_in), int(rate_out), None, 0, C.byref(L), C.byref(K), C.byref(d0))
    if L.value < 1:
        raise UmxError(rc, f"bad rate pair {rate_in} -> {rate_out}")
    taps = np.empty((L.value, K.value), np.float32)
    rc = lib.umx_hip_debug_resample_taps(int(rate_in), int(rate_out), taps.ctypes.data_as(_fp), taps.size, C.byref(L), C.byref(K),
                                         C.byref(d0))
    if rc:
        raise UmxError(rc, "umx_hip_debug_resample_taps")
    return taps, d0.value


def views_from_file_tensors(targets, quantised=True):
    """Build umx_tensor_view[] from ggml.read_model() output.  quantised=True hands the u8/u16 bytes
    + scale/offset to the engine (it dequantises like model.cpp:610-616); False hands fp32."""
    keep, views = [], []
    for t, d in enumerate(targets):
        for name in ggml.tensor_names():
            rec = d[name]
            if isinstance(rec, dict) and quantised:
                arr = np.ascontiguousarray(rec["q"])
                dt = DTYPE_U16 if arr.dtype == np.uint16 else DTYPE_U8
                scale, offset = float(rec["scale"]), float(rec["offset"])
            else:
                arr = np.ascontiguousarray(rec["f32"] if isinstance(rec, dict) else rec, dtype=np.float32)
                dt, scale, offset = DTYPE_F32, 1.0, 0.0
            shp = arr.shape
            v = TensorView()
            nm = name.encode()
            keep.append((arr, nm))
            v.name, v.target, v.dtype, v.n_dims = nm, t, dt, len(shp)
            v.ne[0] = shp[-1]
            v.ne[1] = shp[0] if len(shp) == 2 else 1
            v.scale, v.offset, v.data = scale, offset, arr.ctypes.data
            views.append(v)
    return (TensorView * len(views))(*views), keep


class Engine:
    """One device context = the reference's (umx_model on device, stft_buffers, 4 x lstm_data).

    Mirrors the call shape of umx.cpp:160-227: create once per track, `infer_segment` per chunk,
    the streaming LSTM state carries over until `stream_reset`."""

    def __init__(self, targets, hidden, segment_samples=SEGMENT_SAMPLES, device=0, quantised=True,
                 quantised_resident=True, gemm=None, tracks=1, lstm_batched=False, u8_dequant=False):
        """quantised: hand the file's u8/u16 bytes (+ scale/offset) to the engine instead of fp32 arrays;
        quantised_resident: keep them that way in HBM (the default; BASELINE config 5) or expand them at load;
        gemm: "planes" (fp16 matrix cores, operands pre-split into fp16 planes, LDS-DMA staging: the default with tracks > 1
        or lstm_batched) or "bf16x3" (bf16 terms, both operands split while every tile is staged: the default of the
        single-track engine); "f32" (the fp32-MFMA flavour of rounds 1-2) is refused;
        tracks: independent track lanes (1..64) run together per call (infer_batch*);
        lstm_batched: use the batched (matrix-core) LSTM kernel also on a 1-track context."""
        self.lib = hip_lib()
        views, self._keep = views_from_file_tensors(targets, quantised)
        h = C.c_void_p()
        rc = self.lib.umx_hip_create_tracks(C.byref(h), device, hidden, segment_samples, views, len(views),
                                            (0 if quantised_resident else CREATE_DEQUANTISE_AT_LOAD) |
                                            {"f32": CREATE_GEMM_F32, "bf16x3": CREATE_GEMM_STAGED, "planes": CREATE_GEMM_PLANES}.get(
                                                gemm or os.environ.get("UMX_GEMM", ""), 0) |
                                            (CREATE_LSTM_BATCHED if lstm_batched else 0) |
                                            (CREATE_U8_DEQUANT if (u8_dequant or os.environ.get("UMX_U8") == "dequant") else 0), tracks)
        if rc != UMX_OK:
            raise UmxError(rc, self.lib.umx_hip_last_error(None).decode())
        self.h = h
        self.hidden = hidden
        self.N = segment_samples
        self.T = self.lib.umx_hip_nb_frames(h)
        self.tracks = tracks

    @classmethod
    def from_file(cls, path, segment_samples=SEGMENT_SAMPLES, device=0, quantised_resident=True, gemm=None, tracks=1,
                  lstm_batched=False, quantised=True, u8_dequant=False):
        hidden, targets = ggml.read_model(path)
        return cls(targets, hidden, segment_samples, device, quantised=quantised, quantised_resident=quantised_resident,
                   gemm=gemm, tracks=tracks, lstm_batched=lstm_batched, u8_dequant=u8_dequant)

    def lstm_is_batched(self):
        return bool(self.lib.umx_hip_lstm_is_batched(self.h))

    def pipeline_depth(self):
        """Segments in flight together: that many consecutive asynchronous calls need distinct buffers."""
        return int(self.lib.umx_hip_pipeline_depth(self.h))

    def weight_bytes(self):
        return int(self.lib.umx_hip_weight_bytes(self.h))

    def _check(self, rc):
        if rc != UMX_OK:
            raise UmxError(rc, self.lib.umx_hip_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.umx_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- stream state (lstm.hpp:10-16) ---
    def stream_reset(self):
        self._check(self.lib.umx_hip_stream_reset(self.h))

    def stream_get(self):
        a = np.empty(self.lib.umx_hip_stream_floats(self.h), np.float32)
        self._check(self.lib.umx_hip_stream_get(self.h, a.ctypes.data_as(_fp)))
        return a

    def stream_set(self, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == self.lib.umx_hip_stream_floats(self.h)
        self._check(self.lib.umx_hip_stream_set(self.h, a.ctypes.data_as(_fp)))

    def track_stream_reset(self, track=-1):
        self._check(self.lib.umx_hip_track_stream_reset(self.h, track))

    def track_stream_get(self, track):
        a = np.empty(self.lib.umx_hip_stream_floats(self.h), np.float32)
        self._check(self.lib.umx_hip_track_stream_get(self.h, track, a.ctypes.data_as(_fp)))
        return a

    def track_stream_set(self, track, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == self.lib.umx_hip_stream_floats(self.h)
        self._check(self.lib.umx_hip_track_stream_set(self.h, track, a.ctypes.data_as(_fp)))

    def stream_get_layer(self, layer):
        """(h, c) of LSTM layer `layer`, all chains: [4 targets][2 dirs][2: h, c][hidden/2]."""
        a = np.empty(self.lib.umx_hip_stream_layer_floats(self.h), np.float32)
        self._check(self.lib.umx_hip_stream_get_layer(self.h, layer, a.ctypes.data_as(_fp)))
        return a

    def stream_set_layer(self, layer, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == self.lib.umx_hip_stream_layer_floats(self.h)
        self._check(self.lib.umx_hip_stream_set_layer(self.h, layer, a.ctypes.data_as(_fp)))

    # --- one segment phase by phase (exact multi-GPU carry, multigpu.separate_track_carry_mode) ---
    def segment_begin(self, wave, flags=0):
        wave = np.asarray(wave, np.float32)
        self._phase_n = wave.shape[1]
        a = np.ascontiguousarray(wave.T).ravel()
        self._check(self.lib.umx_hip_segment_begin(self.h, a.ctypes.data_as(_fp), self._phase_n, flags))

    def segment_lstm_layer(self, layer):
        self._check(self.lib.umx_hip_segment_lstm_layer(self.h, layer))

    def segment_end(self):
        n = self._phase_n
        outs = [np.empty(2 * n, np.float32) for _ in range(4)]
        arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs])
        self._check(self.lib.umx_hip_segment_end(self.h, arr))
        return [np.ascontiguousarray(o.reshape(n, 2).T) for o in outs]

    # --- the same cut points on device pointers, all queued on one stream (host/mgpu.cpp); asynchronous, call sync() ---
    def segment_begin_device(self, audio_ptr, n, flags=0):
        self._check(self.lib.umx_hip_segment_begin_device(self.h, C.c_void_p(audio_ptr), n, flags))

    def segment_end_device(self, out_ptrs):
        self._check(self.lib.umx_hip_segment_end_device(self.h, (C.c_void_p * 4)(*out_ptrs)))

    def segment_masks_device(self):
        self._check(self.lib.umx_hip_segment_masks_device(self.h))

    def segment_residual_device(self):
        self._check(self.lib.umx_hip_segment_residual_device(self.h))

    def segment_finish_device(self, out_ptrs):
        self._check(self.lib.umx_hip_segment_finish_device(self.h, (C.c_void_p * 4)(*out_ptrs)))

    # --- split_inference's overlap-add on device pointers (umx.cpp:197-273); hip_stream None = the null stream ---
    def weight_stems_device(self, stem_ptrs, n, hip_stream=None):
        self._check(self.lib.umx_hip_weight_stems_device(self.h, (C.c_void_p * 4)(*stem_ptrs), n, hip_stream))

    def track_accumulate_device(self, track_ptrs, sum_weight_ptr, weighted_ptrs, offset, n, hip_stream=None):
        self._check(self.lib.umx_hip_track_accumulate_device(self.h, (C.c_void_p * 4)(*track_ptrs), C.c_void_p(sum_weight_ptr),
                                                             (C.c_void_p * 4)(*weighted_ptrs), offset, n, hip_stream))

    def track_normalise_device(self, track_ptrs, sum_weight_ptr, length, hip_stream=None):
        self._check(self.lib.umx_hip_track_normalise_device(self.h, (C.c_void_p * 4)(*track_ptrs), C.c_void_p(sum_weight_ptr), length,
                                                            hip_stream))

    # --- whole track on the device (umx.cpp:99-295) ---
    def separate(self, wave, flags=0, shift_offset=None, rate=MODEL_RATE):
        """(2,L) host array -> 4 x (2,L): split_inference with the track resident in HBM; shift_offset: None =
        no shift buffer, n >= 0 = shift_inference with that offset.  rate != 44100: umx_hip_shift_inference_rate (the track is
        resampled to 44.1 kHz and its stems back on the device; shift_offset None = the reference's 4033)."""
        wave = np.asarray(wave, np.float32)
        L = wave.shape[1]
        a = np.ascontiguousarray(wave.T).ravel()
        outs = [np.empty(2 * L, np.float32) for _ in range(4)]
        if rate == MODEL_RATE:
            self.separate_interleaved(a, L, outs, flags, shift_offset)
        else:
            arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs])
            self._check(self.lib.umx_hip_shift_inference_rate(self.h, a.ctypes.data_as(_fp), L, int(rate),
                                                              -1 if shift_offset is None else shift_offset, arr, flags, None, None))
        return [np.ascontiguousarray(o.reshape(L, 2).T) for o in outs]

    def separate_many(self, waves, flags=0, shift_offsets=None, rates=None):
        """Several tracks at once, one per track lane (umx_hip_separate_tracks): list of (2,L_i) -> list of [4 x (2,L_i)].
        rates: one sample rate per track (umx_hip_separate_tracks_rate), None = all 44.1 kHz."""
        m = _TrackArgs(waves, None, 4, shift_offsets, rates, _fp)
        if rates is None:
            self._check(self.lib.umx_hip_separate_tracks(self.h, len(waves), m.a, m.n, m.sh, m.o, flags, None, None))
        else:
            self._check(self.lib.umx_hip_separate_tracks_rate(self.h, len(waves), m.a, m.n, m.rt, m.sh, m.o, flags, None, None))
        return m.result()

    def separate_ensemble(self, wave, shifts=None, offsets=None, flags=0, rate=MODEL_RATE, gains=None):
        """(2,L) host array -> 4 x (2,L): umx_hip_shift_ensemble, the fp32 mean of the track separated at len(offsets) shift offsets,
        one per track lane of one pass.  offsets None: the default offsets of `shifts` shifts (None = 1: offset 4033).
        gains: an (n_out, 5) mix matrix applied to the mean on the device (umx_hip_shift_ensemble_mix) -> n_out x (2,L)."""
        wave = np.asarray(wave, np.float32)
        L = wave.shape[1]
        a = np.ascontiguousarray(wave.T).ravel()
        n_out, g = (4, None) if gains is None else _mix_gains(gains)
        outs = [np.empty(2 * L, np.float32) for _ in range(min(max(n_out, 0), MAX_MIX_OUTPUTS))]
        arr = (_fp * max(1, len(outs)))(*[o.ctypes.data_as(_fp) for o in outs])
        if offsets is None:
            k, off = (1 if shifts is None else int(shifts)), None
        else:
            k, off = len(offsets), (C.c_int * len(offsets))(*[int(o) for o in offsets])
            if shifts is not None and int(shifts) != k:
                raise ValueError("separate_ensemble: shifts and len(offsets) disagree")
        if gains is None:
            self._check(self.lib.umx_hip_shift_ensemble(self.h, a.ctypes.data_as(_fp), L, int(rate), k, off, arr, flags, None, None))
        else:
            self._check(self.lib.umx_hip_shift_ensemble_mix(self.h, a.ctypes.data_as(_fp), L, int(rate), k, off, n_out, g.ctypes.data_as(_fp),
                                                            arr, flags, None, None))
        return [np.ascontiguousarray(o.reshape(L, 2).T) for o in outs]

    # --- the stem mix matrix: weighted sums of the stems and of the input, formed on the device ---
    def separate_mix(self, wave, gains, flags=0, shift_offset=None, rate=MODEL_RATE):
        """separate() with an (n_out, 5) gain matrix behind it (umx_hip_separate_tracks_mix, one track): n_out x (2,L), output m =
        sum_c gains[m][c] * column c, columns 0 .. 3 the stems separate() returns for these arguments, column 4 the input."""
        if shift_offset is None and rate != MODEL_RATE:
            shift_offset = 4033  # as separate(): umx_hip_shift_inference_rate's default
        return self.separate_many_mix([wave], gains, flags, [shift_offset], None if rate == MODEL_RATE else [rate])[0]

    def separate_many_mix(self, waves, gains, flags=0, shift_offsets=None, rates=None):
        """separate_many() with one gain matrix for every lane: list of (2,L_i) -> list of [n_out x (2,L_i)]."""
        n_out, g = _mix_gains(gains)
        m = _TrackArgs(waves, None, n_out, shift_offsets, rates, _fp)
        self._check(self.lib.umx_hip_separate_tracks_mix(self.h, len(waves), m.a, m.n, m.rt, m.sh, n_out, g.ctypes.data_as(_fp), m.o, flags,
                                                         None, None))
        return m.result()

    # --- 16-bit PCM in and out: int16 frames across PCIe, converted on the device ---
    def separate_many_io(self, waves, in_format=SAMPLE_F32, out_format=SAMPLE_F32, dither_seed=None, flags=0, shift_offsets=None,
                         rates=None, gains=None, io=None):
        """umx_hip_separate_tracks_io: separate_many() / separate_many_mix() (gains) with the formats of the host buffers chosen:
        SAMPLE_S16 in takes (2,L_i) int16 arrays, SAMPLE_S16 out returns int16 arrays, dithered with dither_seed unless it is None.
        io: a SampleIO passed as it is instead (tests of the refusals)."""
        io = sample_io(in_format, out_format, dither_seed) if io is None else io
        return self._separate_many_measured("umx_hip_separate_tracks_io", waves, io, flags, shift_offsets, rates, gains).m.result()

    def _separate_many_measured(self, entry_name, waves, io, flags, shift_offsets, rates, gains, **asked):
        """One whole-track call through the rung `entry_name` of the ladder (_MeasuredCall: everything marshalled once, the tail
        that rung has) -> the call, with its outputs and whatever records it asked for."""
        call = _MeasuredCall(entry_name, self.h, waves, io, flags, shift_offsets, rates, gains, **asked)
        self._check(getattr(self.lib, entry_name)(*call.args))
        return call

    # --- output levels and clip handling: what leaves is measured on the device; rescale divides a track by one divisor ---
    def separate_many_levels(self, waves, clip=CLIP_CLAMP, io=None, flags=0, shift_offsets=None, rates=None, gains=None, levels=True):
        """umx_hip_separate_tracks_levels: separate_many_io() (io: a SampleIO, None = fp32 both ways) with a clip mode -> (outputs,
        [Levels per track]); levels=False passes NULL for the records and returns None for them."""
        return self._separate_many_measured("umx_hip_separate_tracks_levels", waves, io, flags, shift_offsets, rates, gains, clip=clip,
                                            levels=levels).results()

    # --- loudness of every output: K-weighted hop energies measured on the device, blocks and gates formed on the host ---
    def separate_many_loudness(self, waves, clip=CLIP_CLAMP, io=None, flags=0, shift_offsets=None, rates=None, gains=None, levels=True,
                               loudness=True, envelopes=True):
        """umx_hip_separate_tracks_loudness: separate_many_levels() -> (outputs, [Levels per track], [Loudness per track], [(n_out, 2,
        hops) float64 hop energies per track]); levels / loudness / envelopes = False pass NULL and return None for them."""
        return self._separate_many_measured("umx_hip_separate_tracks_loudness", waves, io, flags, shift_offsets, rates, gains, clip=clip,
                                            levels=levels, loudness=loudness, envelopes=envelopes).results()

    # --- true peak of every output: the oversampled peak of what leaves, measured on the device; a rescale on it ---
    def separate_many_true_peak(self, waves, true_peak=TRUE_PEAK_MEASURE, clip=CLIP_CLAMP, io=None, flags=0, shift_offsets=None, rates=None,
                                gains=None, levels=True, loudness=False, envelopes=False, records=True):
        """umx_hip_separate_tracks_true_peak: separate_many_loudness() with a true-peak mode -> (outputs, [Levels], [Loudness], [hop
        energies], [TruePeak per track]); levels / loudness / envelopes / records = False pass NULL and return None for them."""
        return self._separate_many_measured("umx_hip_separate_tracks_true_peak", waves, io, flags, shift_offsets, rates, gains, clip=clip,
                                            levels=levels, loudness=loudness, envelopes=envelopes, true_peak=true_peak, records=records).results()

    def true_peak_device(self, in_ptrs, n, rate, bits_ptr, first_frame=0, n_frames=None, hip_stream=None):
        """umx_hip_true_peak_device: frames [first_frame, first_frame + n_frames) of 1 .. 4 device buffers (2,n) interleaved fp32 into the
        four words at device address bits_ptr (unsigned maxima of bit patterns; the caller zeroes them)."""
        nb = len(in_ptrs)
        self._check(self.lib.umx_hip_true_peak_device(self.h, nb, (C.c_void_p * max(1, nb))(*in_ptrs), int(n), int(rate), int(first_frame),
                                                      int(n - first_frame if n_frames is None else n_frames), C.c_void_p(bits_ptr), hip_stream))

    def kweight_hops_device(self, in_ptrs, n, rate, E_ptr, first_hop=0, n_hops=None, hip_stream=None):
        """umx_hip_kweight_hops_device: hops [first_hop, first_hop + n_hops) of 1 .. 4 device buffers (2,n) interleaved fp32 into the
        float64 array [buffer][channel][n // hop] at device address E_ptr."""
        nb = len(in_ptrs)
        hops = kweight_hop_count(n, rate)
        self._check(self.lib.umx_hip_kweight_hops_device(self.h, nb, (C.c_void_p * max(1, nb))(*in_ptrs), int(n), int(rate), int(first_hop),
                                                         int(hops - first_hop if n_hops is None else n_hops), C.c_void_p(E_ptr), hip_stream))

    def levels_device(self, in_ptrs, n, acc_ptr, first_frame=0, io=None, hip_stream=None):
        """umx_hip_levels_device: 1 .. 4 device buffers (2,n) interleaved fp32 measured into the umx_levels_acc at device address acc_ptr."""
        nb = len(in_ptrs)
        self._check(self.lib.umx_hip_levels_device(self.h, nb, (C.c_void_p * max(1, nb))(*in_ptrs), int(n), int(first_frame),
                                                   None if io is None else C.byref(io), C.c_void_p(acc_ptr), hip_stream))

    def _encode_device(self, fmt, in_ptrs, n, out_ptrs, first_frame, dither_seed, hip_stream, acc_ptr=None):
        """umx_hip_pcm<fmt>_encode_device, or with acc_ptr umx_hip_pcm<fmt>_encode_rescaled_device (fmt: 16 or 24)."""
        nb = len(in_ptrs)
        assert len(out_ptrs) == nb
        io = sample_io(SAMPLE_F32, {16: SAMPLE_S16, 24: SAMPLE_S24}[fmt], dither_seed)
        fn = getattr(self.lib, f"umx_hip_pcm{fmt}_encode_device" if acc_ptr is None else f"umx_hip_pcm{fmt}_encode_rescaled_device")
        tail = (hip_stream,) if acc_ptr is None else (C.c_void_p(acc_ptr), hip_stream)
        self._check(fn(self.h, nb, (C.c_void_p * max(1, nb))(*in_ptrs), int(n), int(first_frame), C.byref(io), (C.c_void_p * max(1, nb))(*out_ptrs),
                       *tail))

    def _decode_device(self, fmt, in_ptr, n, out_ptr, hip_stream):
        """umx_hip_pcm<fmt>_decode_device (fmt: 16 or 24)."""
        self._check(getattr(self.lib, f"umx_hip_pcm{fmt}_decode_device")(self.h, C.c_void_p(in_ptr), int(n), C.c_void_p(out_ptr), hip_stream))

    def pcm16_encode_rescaled_device(self, in_ptrs, n, out_ptrs, acc_ptr, first_frame=0, dither_seed=None, hip_stream=None):
        """umx_hip_pcm16_encode_rescaled_device: pcm16_encode_device() on x / g, g formed on the device from the record at acc_ptr."""
        self._encode_device(16, in_ptrs, n, out_ptrs, first_frame, dither_seed, hip_stream, acc_ptr)

    def pcm24_encode_rescaled_device(self, in_ptrs, n, out_ptrs, acc_ptr, first_frame=0, dither_seed=None, hip_stream=None):
        """umx_hip_pcm24_encode_rescaled_device: pcm24_encode_device() on x / g, g formed on the device from the record at acc_ptr."""
        self._encode_device(24, in_ptrs, n, out_ptrs, first_frame, dither_seed, hip_stream, acc_ptr)

    def pcm24_decode_device(self, in_ptr, n, out_ptr, hip_stream=None):
        """umx_hip_pcm24_decode_device: n packed 24-bit stereo frames (6 n bytes, 2-byte aligned) at device address in_ptr -> (2,n)
        interleaved fp32 at out_ptr."""
        self._decode_device(24, in_ptr, n, out_ptr, hip_stream)

    def pcm24_encode_device(self, in_ptrs, n, out_ptrs, first_frame=0, dither_seed=None, hip_stream=None):
        """umx_hip_pcm24_encode_device: 1 .. 4 device buffers (2,n) interleaved fp32 -> n packed 24-bit stereo frames each (6 n bytes,
        2-byte aligned), buffer b as output b."""
        self._encode_device(24, in_ptrs, n, out_ptrs, first_frame, dither_seed, hip_stream)

    def rescale_device(self, ptrs, n, acc_ptr, hip_stream=None):
        """umx_hip_rescale_device: 1 .. 4 device buffers (2,n) interleaved fp32 divided in place by the divisor of the record at acc_ptr."""
        nb = len(ptrs)
        self._check(self.lib.umx_hip_rescale_device(self.h, nb, (C.c_void_p * max(1, nb))(*ptrs), int(n), C.c_void_p(acc_ptr), hip_stream))

    def pcm16_decode_device(self, in_ptr, n, out_ptr, hip_stream=None):
        """umx_hip_pcm16_decode_device: n int16 stereo frames at device address in_ptr -> (2,n) interleaved fp32 at out_ptr."""
        self._decode_device(16, in_ptr, n, out_ptr, hip_stream)

    def pcm16_encode_device(self, in_ptrs, n, out_ptrs, first_frame=0, dither_seed=None, hip_stream=None):
        """umx_hip_pcm16_encode_device: 1 .. 4 device buffers (2,n) interleaved fp32 -> n int16 stereo frames each, buffer b as output b."""
        self._encode_device(16, in_ptrs, n, out_ptrs, first_frame, dither_seed, hip_stream)

    # --- the track queue: more tracks than lanes, a lane refilled with the next track the moment one ends ---
    def separate_queue(self, waves, shift_offsets=None, flags=0, mix=None, io=None, clip=None, levels=False, loudness=False, rates=None,
                       true_peak=None):
        """umx_hip_separate_queue: list of (2,L_i) -> list of [4 x (2,L_i)] (mix: an (n_out, 5) gain matrix -> n_out x (2,L_i)), every
        job bit for bit what separate() / separate_mix() returns for it alone on this engine; the jobs are handed out in list order.
        rates: one sample rate per job (None: all 44.1 kHz), as separate_many() takes them.
        io: a SampleIO (sample_io()) -> umx_hip_separate_queue_io, int16 arrays in and / or out as it says.
        clip (CLIP_CLAMP / CLIP_RESCALE) or levels=True -> umx_hip_separate_queue_levels: returns (outputs, [Levels per job]).
        loudness=True -> umx_hip_separate_queue_loudness: returns (outputs, [Levels], [Loudness], [(n_out, 2, hops) float64]).
        true_peak (a TRUE_PEAK_* mode) -> umx_hip_separate_queue_true_peak: returns those four and [TruePeak per job]."""
        nj = len(waves)
        n_out, g = (4, None) if mix is None else _mix_gains(mix)
        m = _TrackArgs(waves, io, n_out, shift_offsets)
        ins, Ls, outs, shifts = m.ins, m.Ls, m.outs, m.shifts
        state = {"next": 0, "done": []}

        def _next(_user, job):
            j = state["next"]
            if j >= nj:
                return 0
            state["next"] = j + 1
            job[0].audio = C.cast(ins[j].ctypes.data, _fp)  # (read as io says: the caller casts)
            job[0].length, job[0].shift_offset = Ls[j], shifts[j]
            for m, o in enumerate(outs[j]):
                job[0].out[m] = C.cast(o.ctypes.data, _fp)
            job[0].tag = j + 1
            if rates is not None:
                job[0].rate = int(rates[j])
            return 1

        got, loud, env, tps = [None] * nj, [None] * nj, [None] * nj, [None] * nj

        def _done(_user, job, lv=None, ld=None, e=None, tp=None):  # fills whatever its entry point hands it (valid during the callback only)
            j = int(job[0].tag) - 1
            state["done"].append(j)
            if lv is not None:
                got[j] = Levels.from_buffer_copy(lv[0])
            if ld is not None:
                loud[j] = Loudness.from_buffer_copy(ld[0])
                h = int(loud[j].hops)
                env[j] = (np.ctypeslib.as_array(e, shape=(n_out * 2 * h,)).copy() if h else np.zeros(0)).reshape(n_out, 2, h)
            if tp is not None:
                tps[j] = TruePeak.from_buffer_copy(tp[0])

        # the entry point a combination chooses: its done type, what follows `flags`, and what is returned beside the outputs
        io_ref, clip_mode = None if io is None else C.byref(io), int(clip or CLIP_CLAMP)
        if true_peak is not None:
            entry, fn, tail, recs = "umx_hip_separate_queue_true_peak", QUEUE_TRUE_PEAK_FN, (io_ref, clip_mode, int(true_peak)), (got, loud, env, tps)
        elif loudness:
            entry, fn, tail, recs = "umx_hip_separate_queue_loudness", QUEUE_LOUDNESS_FN, (io_ref, clip_mode), (got, loud, env)
        elif clip is not None or levels:
            entry, fn, tail, recs = "umx_hip_separate_queue_levels", QUEUE_LEVELS_FN, (io_ref, clip_mode), (got,)
        elif io is not None:
            entry, fn, tail, recs = "umx_hip_separate_queue_io", QUEUE_DONE_FN, (io_ref,), ()
        else:
            entry, fn, tail, recs = "umx_hip_separate_queue", QUEUE_DONE_FN, (), ()
        self._check(getattr(self.lib, entry)(self.h, QUEUE_NEXT_FN(_next), fn(_done), None, n_out, None if g is None else g.ctypes.data_as(_fp),
                                             flags, *tail))
        assert sorted(state["done"]) == list(range(nj)), state
        return (m.result(),) + recs if recs else m.result()

    def queue_calls(self):
        """Calls of the segment loop the engine's last separate_queue made (umx_hip_debug_queue_calls); None: there has been none."""
        n = int(self.lib.umx_hip_debug_queue_calls(self.h))
        return None if n < 0 else n

    def mix_stems_device(self, gains, stem_ptrs, mix_ptr, n, out_ptrs, hip_stream=None):
        """umx_hip_mix_stems_device: the mix kernel on device buffers (2,n) interleaved, queued on hip_stream.  stem_ptrs: 4 device
        addresses (None / 0 where the column is unused), mix_ptr likewise; out_ptrs: n_out addresses (out_ptrs[m] may be stem_ptrs[m])."""
        n_out, g = _mix_gains(gains)
        stems = (C.c_void_p * 4)(*[p or None for p in stem_ptrs])
        outs = (C.c_void_p * max(1, len(out_ptrs)))(*[p or None for p in out_ptrs])
        self._check(self.lib.umx_hip_mix_stems_device(self.h, n_out, g.ctypes.data_as(_fp), stems, mix_ptr or None, int(n), outs, hip_stream))

    def shift_mean_ms(self):
        """shift_mean_kernel's milliseconds in the last separate_ensemble with more than one shift (None: there has been none)."""
        ms = float(self.lib.umx_hip_debug_shift_mean_ms(self.h))
        return None if ms < 0 else ms

    def resample_device(self, rate_in, rate_out, in_ptrs, n_in, out_ptrs, n_out, hip_stream=None):
        """umx_hip_resample_device: 1 .. 4 device buffers (2,n_in) interleaved -> (2,n_out), queued on hip_stream."""
        nb = len(in_ptrs)
        assert len(out_ptrs) == nb
        self._check(self.lib.umx_hip_resample_device(self.h, int(rate_in), int(rate_out), nb, (C.c_void_p * nb)(*in_ptrs), int(n_in),
                                                     (C.c_void_p * nb)(*out_ptrs), int(n_out), hip_stream))

    def resample_range_device(self, rate_in, rate_out, in_ptrs, n_in, out_ptrs, n_out, first, count, hip_stream=None):
        """umx_hip_resample_range_device: frames [first, first + count) of the n_out output frames of resample_device(), nothing else."""
        nb = len(in_ptrs)
        assert len(out_ptrs) == nb
        self._check(self.lib.umx_hip_resample_range_device(self.h, int(rate_in), int(rate_out), nb, (C.c_void_p * nb)(*in_ptrs), int(n_in),
                                                           (C.c_void_p * nb)(*out_ptrs), int(n_out), int(first), int(count), hip_stream))

    def resample_launches(self):
        """(forward, backward) resampler launches of the engine's last whole-track call or queue run (umx_hip_debug_resample_launches);
        None: there has been none."""
        f, b = C.c_int(), C.c_int()
        if self.lib.umx_hip_debug_resample_launches(self.h, C.byref(f), C.byref(b)) != UMX_OK:
            return None
        return f.value, b.value

    def separate_interleaved(self, a, L, outs, flags=0, shift_offset=None):
        """The bare C call: a = (2,L) interleaved float32, outs = 4 preallocated float32[2L]; returns seconds."""
        import time
        arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs])
        t0 = time.perf_counter()
        if shift_offset is None:
            rc = self.lib.umx_hip_split_inference(self.h, a.ctypes.data_as(_fp), L, arr, flags, None, None)
        else:
            rc = self.lib.umx_hip_shift_inference(self.h, a.ctypes.data_as(_fp), L, shift_offset, arr, flags, None, None)
        dt = time.perf_counter() - t0
        self._check(rc)
        return dt

    # --- umx_inference (inference.cpp:12-207) ---
    def infer_segment(self, wave, flags=0):
        """wave (2,n) fp32 host array -> list of 4 (2,n) host arrays (H2D + kernels + D2H)."""
        wave = np.asarray(wave, np.float32)
        n = wave.shape[1]
        a = np.ascontiguousarray(wave.T).ravel()
        outs = [np.empty(2 * n, np.float32) for _ in range(4)]
        arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs])
        self._check(self.lib.umx_hip_infer_segment(self.h, a.ctypes.data_as(_fp), n, arr, flags))
        return [np.ascontiguousarray(o.reshape(n, 2).T) for o in outs]

    def infer_batch(self, waves, flags=0):
        """waves: list (one per track lane) of (2,n_i) arrays or None (lane idle) -> list of [4 x (2,n_i)] or None."""
        nb = len(waves)
        aud, ns, outs = (C.c_void_p * nb)(), (C.c_int * nb)(), (C.c_void_p * (4 * nb))()
        keep = []
        for i, wv in enumerate(waves):
            if wv is None:
                aud[i], ns[i] = None, 0
                continue
            wv = np.asarray(wv, np.float32)
            a = np.ascontiguousarray(wv.T).ravel()
            o = [np.empty(2 * wv.shape[1], np.float32) for _ in range(4)]
            keep.append((a, o))
            aud[i], ns[i] = a.ctypes.data, wv.shape[1]
            for t in range(4):
                outs[4 * i + t] = o[t].ctypes.data
        self._check(self.lib.umx_hip_infer_batch(self.h, nb, aud, ns, outs, flags))
        res, k = [], 0
        for wv in waves:
            if wv is None:
                res.append(None)
                continue
            n = keep[k][0].size // 2
            res.append([np.ascontiguousarray(o.reshape(n, 2).T) for o in keep[k][1]])
            k += 1
        return res

    def infer_batch_ptrs(self, audio_ptrs, ns, out_ptrs, flags=0, where="device"):
        """Raw pointers: audio_ptrs[i] (0 = lane idle), ns[i], out_ptrs[4*i + t]; where = "device" (HBM buffers) or
        "host_async" (host buffers, pinned for overlap: H2D + kernels + D2H queued).  Asynchronous: call sync()."""
        nb = len(audio_ptrs)
        aud = (C.c_void_p * nb)(*[p or None for p in audio_ptrs])
        n_ = (C.c_int * nb)(*ns)
        outs = (C.c_void_p * (4 * nb))(*[p or None for p in out_ptrs])
        fn = self.lib.umx_hip_infer_batch_device if where == "device" else self.lib.umx_hip_infer_batch_async
        self._check(fn(self.h, nb, aud, n_, outs, flags))

    def infer_segment_device(self, audio_ptr, n, out_ptrs, flags=0):
        """Raw device pointers (e.g. torch tensor .data_ptr()); asynchronous, call sync()."""
        arr = (C.c_void_p * 4)(*out_ptrs)
        self._check(self.lib.umx_hip_infer_segment_device(self.h, C.c_void_p(audio_ptr), n, arr, flags))

    def sync(self):
        self._check(self.lib.umx_hip_sync(self.h))

    def last_error(self):
        return self.lib.umx_hip_last_error(self.h).decode()

    def lstm_was_persistent(self):
        return bool(self.lib.umx_hip_lstm_was_persistent(self.h))

    def lstm_mode(self):
        """0 stepwise, 1 persistent (placement-independent hand-off), 2 persistent (intra-XCD hand-off)."""
        return self.lib.umx_hip_lstm_mode(self.h)

    def lstm_profile(self):
        buf = (C.c_ulonglong * 48)()
        self._check(self.lib.umx_hip_debug_lstm_profile(self.h, buf))
        a = np.array(buf[:], dtype=np.uint64).reshape(3, 2, 8)
        return a

    def gemm_kernel_name(self, mode):
        """The GEMM kernel the last call launched for stage `mode` (0 fc1, 1 W_ih, 2 fc2, 3 fc3)."""
        return self.lib.umx_hip_gemm_kernel_name(self.h, mode).decode()

    def lstm_kernel_name(self):
        """The recurrence kernel of the last LSTM layer launch (umx_hip_lstm_kernel_name)."""
        return self.lib.umx_hip_lstm_kernel_name(self.h).decode()

    def lstm_placement(self, n=256):
        """(xcc, chain, slice, HW_ID) of every workgroup of the last profiled one-track recurrence launch."""
        buf = (C.c_ulonglong * n)()
        self._check(self.lib.umx_hip_debug_lstm_placement(self.h, buf, n))
        a = np.array(buf[:], dtype=np.uint64)
        return [(int(v >> 48) & 15, int(v >> 40) & 255, int(v >> 32) & 255, int(v) & 0xffffffff) for v in a]

    def tap(self, what, target=0):
        n = self.lib.umx_hip_read_tap(self.h, what.encode(), target, None, 0)
        if n < 0:
            raise UmxError(ERR_ARG, f"tap {what!r} unavailable ({n})")
        buf = np.empty(n, np.float32)
        got = self.lib.umx_hip_read_tap(self.h, what.encode(), target, buf.ctypes.data_as(_fp), n)
        if got != n:
            raise UmxError(ERR_HIP, f"tap {what!r} failed ({got})")
        T, H = self.T, self.hidden
        what = what.split("@")[0].split("#")[0]
        if what in ("lstm_l0", "lstm_l1"):
            return buf.reshape(T, H)
        if what == "proj":
            return buf.reshape(T, 4 * H)
        if what in ("spec", "y"):
            return buf.view(np.complex64).reshape(2, T, NB)
        if what in ("mix_mag", "target_mag"):
            return buf.reshape(2, T, NB)
        if what == "x":
            return buf.reshape(T, KX)
        if what in ("fc1", "lstm", "fc2"):
            return buf.reshape(T, H)
        if what == "mask":
            return buf.reshape(T, NOUT)
        return buf

    def stage_times(self, slot=None):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        if slot is None:
            n = self.lib.umx_hip_stage_times(self.h, names, ms, 32)
        else:
            n = self.lib.umx_hip_stage_times_slot(self.h, slot, names, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    def stage_kernel_times(self, slot=None):
        """Like stage_times, but a GEMM stage of a plane context without its split kernel (umx_hip_stage_kernel_times_slot)."""
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        n = self.lib.umx_hip_stage_times_slot(self.h, 0, names, (C.c_float * 32)(), 32)
        m = self.lib.umx_hip_stage_kernel_times_slot(self.h, -1 if slot is None else slot, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(min(n, m))}


# ------------------------------------------------------------------ C++17 host library (umx_host.h)
HOST_SYMBOLS = ["umx_model_load", "umx_model_free", "umx_model_hidden", "umx_model_n_tensors", "umx_model_views",
                "umx_model_data_bytes", "umx_model_load_progress", "umx_model_dequantize", "umx_wav_load",
                "umx_wav_free", "umx_wav_write_f32", "umx_wav_load_rate", "umx_wav_write_f32_rate",
                "umx_wav_load_pcm16", "umx_wav_free_pcm16", "umx_wav_write_pcm16_rate",
                "umx_wav_load_pcm24", "umx_wav_free_pcm24", "umx_wav_write_pcm24_rate", "umx_split_inference", "umx_shift_inference",
                "umx_segment_plan", "umx_transition_weight", "umx_split_inference_carry", "umx_split_inference_targets", "umx_mix_parse"]

SEGMENT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _fp, C.c_int, C.POINTER(_fp))
RESET_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_float, C.c_void_p)


PH_BEGIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _fp, C.c_int)
PH_LAYER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
PH_END_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_fp))
PH_STATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _fp)
P2P_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _fp, C.c_size_t, C.c_int)


class PhasedBackend(C.Structure):
    """include/umx_host.h: umx_phased_backend"""
    _fields_ = [("begin", PH_BEGIN_FN), ("layer", PH_LAYER_FN), ("end", PH_END_FN), ("get_layer", PH_STATE_FN),
                ("set_layer", PH_STATE_FN), ("layer_floats", C.c_size_t), ("user", C.c_void_p)]


TG_BEGIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _fp, C.c_int, C.c_uint)
TG_STATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, _fp)
TG_VOID_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
TG_MAG_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _fp)


class TargetBackend(C.Structure):
    """include/umx_host.h: umx_target_backend"""
    _fields_ = [("begin", TG_BEGIN_FN), ("layer", PH_LAYER_FN), ("get_state", TG_STATE_FN), ("set_state", TG_STATE_FN),
                ("masks", TG_VOID_FN), ("get_mag", TG_MAG_FN), ("set_mag", TG_MAG_FN), ("finish", PH_END_FN), ("discard", TG_VOID_FN),
                ("target_layer_floats", C.c_size_t), ("mag_floats", C.c_size_t), ("user", C.c_void_p)]


class P2P(C.Structure):
    """include/umx_host.h: umx_p2p"""
    _fields_ = [("send", P2P_FN), ("recv", P2P_FN), ("user", C.c_void_p)]


class Backend(C.Structure):
    """include/umx_host.h: umx_backend"""
    _fields_ = [("segment", SEGMENT_FN), ("reset", RESET_FN), ("user", C.c_void_p)]


_host = None


def host_lib():
    global _host
    if _host is not None:
        return _host
    path = HERE / "libumx_host.so"
    if not path.exists():
        raise ImportError(f"{path} is missing: run __graft_entry__.build()")
    lib = C.CDLL(str(path))
    lib.umx_model_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p]
    lib.umx_model_free.argtypes = [C.c_void_p]
    lib.umx_model_hidden.argtypes = [C.c_void_p]
    lib.umx_model_n_tensors.argtypes = [C.c_void_p]
    lib.umx_model_views.restype = C.POINTER(TensorView)
    lib.umx_model_views.argtypes = [C.c_void_p]
    lib.umx_model_data_bytes.restype = C.c_size_t
    lib.umx_model_data_bytes.argtypes = [C.c_void_p]
    lib.umx_model_load_progress.restype = C.c_float
    lib.umx_model_load_progress.argtypes = [C.c_void_p]
    lib.umx_model_dequantize.restype = C.c_long
    lib.umx_model_dequantize.argtypes = [C.c_void_p, C.c_int, C.c_char_p, _fp, C.c_size_t]
    lib.umx_wav_load.argtypes = [C.c_char_p, C.POINTER(_fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]
    lib.umx_wav_free.argtypes = [_fp]
    lib.umx_wav_write_f32.argtypes = [C.c_char_p, _fp, C.c_int, C.c_char_p]
    lib.umx_wav_load_rate.argtypes = [C.c_char_p, C.POINTER(_fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]
    lib.umx_wav_write_f32_rate.argtypes = [C.c_char_p, _fp, C.c_int, C.c_int, C.c_char_p]
    lib.umx_wav_load_pcm16.argtypes = [C.c_char_p, C.POINTER(_i16p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]
    lib.umx_wav_free_pcm16.argtypes = [_i16p]
    lib.umx_wav_write_pcm16_rate.argtypes = [C.c_char_p, _i16p, C.c_int, C.c_int, C.c_char_p]
    lib.umx_wav_load_pcm24.argtypes = [C.c_char_p, C.POINTER(_u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]
    lib.umx_wav_free_pcm24.argtypes = [_u8p]
    lib.umx_wav_write_pcm24_rate.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int, C.c_char_p]
    lib.umx_split_inference.argtypes = [C.POINTER(Backend), _fp, C.c_int, C.c_int, C.POINTER(_fp), PROGRESS_FN,
                                        C.c_void_p, C.c_char_p]
    lib.umx_shift_inference.argtypes = [C.POINTER(Backend), _fp, C.c_int, C.c_int, C.c_int, C.POINTER(_fp),
                                        PROGRESS_FN, C.c_void_p, C.c_char_p]
    lib.umx_split_inference_carry.argtypes = [C.POINTER(PhasedBackend), C.POINTER(P2P), C.c_int, C.c_int, _fp, C.c_int, C.c_int,
                                              C.POINTER(_fp), C.c_char_p]
    lib.umx_split_inference_targets.argtypes = [C.POINTER(TargetBackend), C.POINTER(P2P), C.c_int, C.c_int, _fp, C.c_int, C.c_int,
                                                C.POINTER(_fp), C.c_char_p]
    lib.umx_segment_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.umx_mix_parse.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, _fp, C.c_char_p]
    lib.umx_transition_weight.restype = C.c_float
    lib.umx_transition_weight.argtypes = [C.c_int, C.c_int, C.c_int]
    _host = lib
    return lib


class HostError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"umx_host error {code}: {msg}")
        self.code = code


class HostModel:
    """load_umx_model (model.cpp:42-574) through the C++ host loader; tensors stay quantised."""

    def __init__(self, path):
        self.lib = host_lib()
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        rc = self.lib.umx_model_load(str(path).encode(), C.byref(h), err)
        if rc:
            raise HostError(rc, err.value.decode())
        self.h = h
        self.hidden = self.lib.umx_model_hidden(h)
        self.n_tensors = self.lib.umx_model_n_tensors(h)

    def views(self):
        return self.lib.umx_model_views(self.h), self.n_tensors

    def dequantize(self, target, name):
        n = self.lib.umx_model_dequantize(self.h, target, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        a = np.empty(n, np.float32)
        self.lib.umx_model_dequantize(self.h, target, name.encode(), a.ctypes.data_as(_fp), n)
        return a

    def data_bytes(self):
        return self.lib.umx_model_data_bytes(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.umx_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def engine_from_host_model(hm, segment_samples=SEGMENT_SAMPLES, device=0):
    """The CLI's path: C++ loader views -> umx_hip_create (no Python copy of the weights)."""
    eng = Engine.__new__(Engine)
    eng.lib = hip_lib()
    views, n = hm.views()
    h = C.c_void_p()
    rc = eng.lib.umx_hip_create(C.byref(h), device, hm.hidden, segment_samples, views, n)
    if rc != UMX_OK:
        raise UmxError(rc, eng.lib.umx_hip_last_error(None).decode())
    eng.h, eng.hidden, eng.N, eng._keep = h, hm.hidden, segment_samples, None
    eng.T = eng.lib.umx_hip_nb_frames(h)
    return eng


def wav_load(path):
    """load_audio (dsp.cpp:18-77): -> ((2,n) float32, channels in file)."""
    lib = host_lib()
    p, n, ch = _fp(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    rc = lib.umx_wav_load(str(path).encode(), C.byref(p), C.byref(n), C.byref(ch), err)
    if rc:
        raise HostError(rc, err.value.decode())
    a = np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()
    lib.umx_wav_free(p)
    return np.ascontiguousarray(a.T), ch.value


def wav_load_rate(path):
    """umx_wav_load_rate: -> ((2,n) float32, channels in file, sample rate); any rate of 8 .. 192 kHz."""
    lib = host_lib()
    p, n, ch, rate = _fp(), C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    rc = lib.umx_wav_load_rate(str(path).encode(), C.byref(p), C.byref(n), C.byref(ch), C.byref(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())
    a = np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()
    lib.umx_wav_free(p)
    return np.ascontiguousarray(a.T), ch.value, rate.value


def wav_write(path, wave, rate=MODEL_RATE):
    """write_audio_file (dsp.cpp:80-101): (2,n) -> stereo float32 WAV (at `rate` Hz: umx_wav_write_f32_rate)."""
    a = np.ascontiguousarray(np.asarray(wave, np.float32).T)
    err = C.create_string_buffer(256)
    if rate == MODEL_RATE:
        rc = host_lib().umx_wav_write_f32(str(path).encode(), a.ctypes.data_as(_fp), a.shape[0], err)
    else:
        rc = host_lib().umx_wav_write_f32_rate(str(path).encode(), a.ctypes.data_as(_fp), a.shape[0], int(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())


def wav_load_pcm16(path):
    """umx_wav_load_pcm16: a 16-bit PCM file as it is -> ((2,n) int16, channels in file, sample rate); HostError for any other encoding."""
    lib = host_lib()
    p, n, ch, rate = _i16p(), C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    rc = lib.umx_wav_load_pcm16(str(path).encode(), C.byref(p), C.byref(n), C.byref(ch), C.byref(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())
    a = np.ctypeslib.as_array(p, shape=(max(n.value, 1), 2))[:n.value].copy()
    lib.umx_wav_free_pcm16(p)
    return np.ascontiguousarray(a.T), ch.value, rate.value


def wav_write_pcm16(path, wave, rate=MODEL_RATE):
    """umx_wav_write_pcm16_rate: (2,n) int16 -> stereo 16-bit PCM WAV at `rate` Hz."""
    a = np.ascontiguousarray(np.asarray(wave, np.int16).T)
    err = C.create_string_buffer(256)
    rc = host_lib().umx_wav_write_pcm16_rate(str(path).encode(), a.ctypes.data_as(_i16p), a.shape[0], int(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())


def wav_load_pcm24(path, probe=False):
    """umx_wav_load_pcm24: a 24-bit PCM file as it is -> ((2,n) int32 codes, channels in file, sample rate); HostError for any other
    encoding.  probe=True reads the file's head only -> (frames, channels in file, sample rate)."""
    lib = host_lib()
    p, n, ch, rate = _u8p(), C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(256)
    rc = lib.umx_wav_load_pcm24(str(path).encode(), None if probe else C.byref(p), C.byref(n), C.byref(ch), C.byref(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())
    if probe:
        return n.value, ch.value, rate.value
    b = np.ctypeslib.as_array(p, shape=(max(n.value, 1) * 6,))[:6 * n.value].copy()
    lib.umx_wav_free_pcm24(p)
    return pcm24_unpack(b), ch.value, rate.value


def wav_write_pcm24(path, wave, rate=MODEL_RATE):
    """umx_wav_write_pcm24_rate: (2,n) int32 codes -> stereo 24-bit PCM WAV at `rate` Hz."""
    b = pcm24_pack(wave)
    err = C.create_string_buffer(256)
    rc = host_lib().umx_wav_write_pcm24_rate(str(path).encode(), b.ctypes.data_as(_u8p), b.size // 6, int(rate), err)
    if rc:
        raise HostError(rc, err.value.decode())


def segment_plan(length, segment_samples=SEGMENT_SAMPLES):
    lib = host_lib()
    n = lib.umx_segment_plan(length, segment_samples, None, None, 0)
    offs, lens = (C.c_int * n)(), (C.c_int * n)()
    lib.umx_segment_plan(length, segment_samples, offs, lens, n)
    return list(offs), list(lens)


def make_backend(segment_fn, reset_fn=None):
    """Wrap Python callables as a umx_backend: segment_fn((2,n) array) -> 4 x (2,n) arrays."""
    def _seg(_user, audio, n, out):
        try:
            wave = np.ctypeslib.as_array(audio, shape=(n, 2)).T
            res = segment_fn(np.ascontiguousarray(wave))
            for t in range(4):
                dst = np.ctypeslib.as_array(out[t], shape=(n, 2))
                dst[:, :] = np.asarray(res[t], np.float32).T
            return 0
        except Exception as e:  # noqa: BLE001 - surfaced as a backend error code
            print("segment backend raised:", repr(e))
            return 13

    def _reset(_user):
        if reset_fn is not None:
            reset_fn()
        return 0
    cb_seg, cb_reset = SEGMENT_FN(_seg), RESET_FN(_reset)
    be = Backend(cb_seg, cb_reset, None)
    be._keep = (cb_seg, cb_reset)
    return be


def _run_driver(kind, backend, wave, segment_samples, offset=None, progress=None):
    lib = host_lib()
    wave = np.asarray(wave, np.float32)
    L = wave.shape[1]
    a = np.ascontiguousarray(wave.T).ravel()
    outs = [np.empty(2 * L, np.float32) for _ in range(4)]
    arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs])
    err = C.create_string_buffer(256)
    pcb = PROGRESS_FN((lambda p, _u: progress(p)) if progress else (lambda p, _u: None))
    if kind == "split":
        rc = lib.umx_split_inference(C.byref(backend), a.ctypes.data_as(_fp), L, segment_samples, arr, pcb, None, err)
    else:
        rc = lib.umx_shift_inference(C.byref(backend), a.ctypes.data_as(_fp), L, segment_samples,
                                     -1 if offset is None else offset, arr, pcb, None, err)
    if rc:
        raise HostError(rc, err.value.decode())
    return [np.ascontiguousarray(o.reshape(L, 2).T) for o in outs]


def split_inference(backend, wave, segment_samples=SEGMENT_SAMPLES, progress=None):
    """umx.cpp:152-295 through the C++ host driver."""
    return _run_driver("split", backend, wave, segment_samples, progress=progress)


def shift_inference(backend, wave, segment_samples=SEGMENT_SAMPLES, offset=None, progress=None):
    """umx.cpp:99-150 through the C++ host driver (offset None = the reference's rand()%22050)."""
    return _run_driver("shift", backend, wave, segment_samples, offset=offset, progress=progress)


def engine_backend(eng, flags=0):
    return make_backend(lambda w: eng.infer_segment(w, flags), eng.stream_reset)


# ------------------------------------------------------------------ multi-GPU track driver (umx_mgpu.h)
MGPU_SYMBOLS = ["umx_mgpu_unique_id", "umx_mgpu_create", "umx_mgpu_create_ex", "umx_mgpu_destroy", "umx_mgpu_separate_track", "umx_mgpu_stats"]
MGPU_ID_BYTES = 640
MGPU_BY_TARGET, MGPU_LOOPBACK = 0x1, 0x2
_mgpu = None


def mgpu_lib():
    """libumx_mgpu.so: C++17 host over RCCL (loads librccl; a process that never shards a track does not need it)."""
    global _mgpu
    if _mgpu is not None:
        return _mgpu
    hip_lib()
    path = HERE / "libumx_mgpu.so"
    if not path.exists():
        raise ImportError(f"{path} is missing: run __graft_entry__.build()")
    lib = C.CDLL(str(path))
    lib.umx_mgpu_unique_id.argtypes = [C.c_char_p, C.c_char_p]
    lib.umx_mgpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    lib.umx_mgpu_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_uint, C.c_char_p]
    lib.umx_mgpu_destroy.argtypes = [C.c_void_p]
    lib.umx_mgpu_separate_track.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.POINTER(_fp), C.c_uint, C.c_char_p]
    lib.umx_mgpu_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    _mgpu = lib
    return lib


def mgpu_unique_id():
    buf = C.create_string_buffer(MGPU_ID_BYTES)
    err = C.create_string_buffer(256)
    rc = mgpu_lib().umx_mgpu_unique_id(buf, err)
    if rc:
        raise UmxError(rc, err.value.decode())
    return buf.raw


class MultiGpuTrack:
    """One track over `world` GPUs, exact (include/umx_mgpu.h): world = G target groups x P segment-pipeline stages; LSTM
    layer states, target magnitudes and weighted stems travel over RCCL point to point on device pointers.  ids: the
    bytes of mgpu_unique_id() made on rank 0 and handed to every rank (None when world == 1).  by_target: shard by source
    model as well (G = gcd(world, 4)); loopback (world 1 only): every transfer through a grouped RCCL self send + receive."""

    def __init__(self, engine, rank=0, world=1, ids=None, by_target=False, loopback=False):
        self.lib, self.eng, self.rank = mgpu_lib(), engine, rank
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        rc = self.lib.umx_mgpu_create_ex(C.byref(h), engine.h, rank, world, ids, (MGPU_BY_TARGET if by_target else 0) |
                                         (MGPU_LOOPBACK if loopback else 0), err)
        if rc:
            raise UmxError(rc, err.value.decode())
        self.h = h

    def separate(self, wave, shift_offset=None, flags=0):
        """(2,L) host array on every rank -> 4 x (2,L) on rank 0 (None elsewhere); collective over the ranks."""
        wave = np.asarray(wave, np.float32)
        L = wave.shape[1]
        a = np.ascontiguousarray(wave.T).ravel()
        outs = [np.empty(2 * L, np.float32) for _ in range(4)] if self.rank == 0 else None
        arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs]) if outs else None
        err = C.create_string_buffer(256)
        rc = self.lib.umx_mgpu_separate_track(self.h, a.ctypes.data_as(_fp), L, -1 if shift_offset is None else shift_offset,
                                              arr, flags, err)
        if rc:
            raise UmxError(rc, err.value.decode())
        return [np.ascontiguousarray(o.reshape(L, 2).T) for o in outs] if outs else None

    def separate_interleaved(self, a, L, outs, shift_offset=None, flags=0):
        """The bare C call: a = (2,L) interleaved float32 on every rank, outs = 4 preallocated float32[2L] on rank 0 (None
        elsewhere); returns seconds."""
        import time
        arr = (_fp * 4)(*[o.ctypes.data_as(_fp) for o in outs]) if outs else None
        err = C.create_string_buffer(256)
        t0 = time.perf_counter()
        rc = self.lib.umx_mgpu_separate_track(self.h, a.ctypes.data_as(_fp), L, -1 if shift_offset is None else shift_offset, arr, flags, err)
        dt = time.perf_counter() - t0
        if rc:
            raise UmxError(rc, err.value.decode())
        return dt

    def stats(self):
        """{rccl_ops, state_hops, magnitude_transfers, stem_transfers, retries} of the last track."""
        buf = (C.c_longlong * 5)()
        self.lib.umx_mgpu_stats(self.h, buf)
        return dict(zip(("rccl_ops", "state_hops", "magnitude_transfers", "stem_transfers", "retries"), [int(x) for x in buf]))

    def close(self):
        if getattr(self, "h", None):
            self.lib.umx_mgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
