"""tests/mix_ref.py -- the stem mix matrix's definition (include/umx_hip.h) on arrays.  gains is (n_out, 5): columns
0 .. 3 the four stem slots, column 4 the mixture.  Per output m and element, in fp32:
    out_m = ((g_c1 * s_c1 + g_c2 * s_c2) + g_c3 * s_c3) + ...   over the columns c1 < c2 < ... with gains[m][c] != 0
each product rounded on its own (numpy's float32 multiply and add are IEEE, subnormals included; there is no fused multiply-add
in numpy), the terms added left to right, the first term the product itself, a row without a nonzero gain +0.0.  A column with a
zero gain (+0 or -0) is not touched: it may be None, or hold inf / NaN."""
import numpy as np

COLUMNS = 5
MIXTURE = 4


def mix_fp32(stems4, mixture, gains):
    """stems4: 4 float32 arrays (None where no row uses the column), mixture: one more (or None), gains: (n_out, 5) ->
    list of n_out float32 arrays."""
    g = np.asarray(gains, np.float32)
    assert g.ndim == 2 and g.shape[1] == COLUMNS and 1 <= g.shape[0] <= 4 and np.isfinite(g).all()
    cols = list(stems4) + [mixture]
    assert len(cols) == COLUMNS
    shape = next(np.asarray(c).shape for c in cols if c is not None)
    outs = []
    for m in range(g.shape[0]):
        acc = None
        for c in range(COLUMNS):
            if g[m, c] == 0:  # -0.0 == 0: not a term
                continue
            s = np.asarray(cols[c])
            assert s.dtype == np.float32 and s.shape == shape, (m, c)
            with np.errstate(all="ignore"):
                p = g[m, c] * s  # float32 * float32: one rounding
                acc = p if acc is None else acc + p  # one rounding per addition
        outs.append(np.zeros(shape, np.float32) if acc is None else acc)
    return outs


IDENTITY = np.eye(4, 5, dtype=np.float32)
# vocals and accompaniment = bass + drums + other (Open-Unmix's aggregate_dict example)
AGGREGATE = np.array([[0, 0, 0, 1, 0], [1, 1, 1, 0, 0]], np.float32)
# "mixture minus vocals": not the sum of the other three
KARAOKE = np.array([[0, 0, 0, -1, 1]], np.float32)
