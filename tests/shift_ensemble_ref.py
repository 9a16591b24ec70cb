"""tests/shift_ensemble_ref.py -- the shift ensemble's definition (include/umx_hip.h) on arrays: per element, in fp32,
    out = (((s_0 + s_1) + s_2) + ... + s_{K-1}) / (float)K
summed left to right in the order given, one correctly rounded division (numpy's float32 add and divide are IEEE, subnormals
included) -- and the float64 mean of the oracle's single-shift results to hold it against."""
import numpy as np


def mean_fp32(stems):
    """stems: K float32 arrays of one shape, in ensemble order -> their fp32 mean as defined above."""
    stems = [np.asarray(s) for s in stems]
    assert stems and all(s.dtype == np.float32 and s.shape == stems[0].shape for s in stems)
    acc = stems[0].copy()
    for s in stems[1:]:
        acc = acc + s  # float32 + float32: one rounding per addition
    return acc / np.float32(len(stems))


def mean_of_lanes(lanes):
    """lanes: K lists of 4 stems (Engine.separate_many's result for the K lanes) -> 4 stems, mean_fp32 per stem."""
    return [mean_fp32([lane[t] for lane in lanes]) for t in range(4)]


def oracle_mean_f64(po, om, wave, segment_samples, offsets, flags=0, cache=None):
    """The float64 mean of the oracle's shift_inference at each offset -> 4 float64 arrays.  cache: a dict that keeps the
    single-shift results per offset (an ensemble in another order needs the same ones)."""
    cache = {} if cache is None else cache
    for o in offsets:
        if o not in cache:
            cache[o] = [np.asarray(s, np.float64) for s in po.shift_inference(om, wave, segment_samples, o, flags)]
    return [sum(cache[o][t] for o in offsets) / float(len(offsets)) for t in range(4)]
