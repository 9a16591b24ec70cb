// gate_debug.h -- part of engine.hip: the kernels behind umx_hip_debug_gate_math (engine_cabi.h).  They only call the device functions
// the recurrence kernels and the fc1 epilogue call themselves; nothing of the arithmetic is restated here.
#pragma once
#include "gemm_common.h"
#include "lstm_kernels.h"

namespace umx
{

// The gate functions the recurrence kernels and the fc1 epilogue call -- tanh_epi (gemm_common.h), tanh_hw, sigmoid_hw and
// the PRECISE forms tanhf / sigmoid_ref (lstm_kernels.h) -- on caller-given values, and one cell step per wave through
// lstm_cell<false>, lstm_cell_flat, lstm_cell<true> and lstm_cell_lane<false>, so that a test can hold them against float64 over the whole float32 range
// (the engine's own tests keep every gate within about +-2).  fn [5][n]: tanh_epi, tanh_hw, sigmoid_hw, tanhf, sigmoid_ref.
__global__ void debug_gate_fn_kernel(int n, const float *x, float *fn)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float v = x[i];
    fn[i] = tanh_epi(v);
    fn[(size_t)n + i] = tanh_hw(v);
    fn[(size_t)2 * n + i] = sigmoid_hw(v);
    fn[(size_t)3 * n + i] = tanhf(v);
    fn[(size_t)4 * n + i] = sigmoid_ref(v);
}
// one wave per block, all 64 lanes live (the cells shuffle quads with DPP): pre [waves][64] in the quad layout lane = 4*u + g,
// c [waves][16] -> cell [waves][2: c, h][16].  FORM 0 lstm_cell<false>, 1 lstm_cell_flat, 2 lstm_cell<true>, 3 lstm_cell_lane<false>
// (the cell of the batched recurrences: the first lane of a quad reads the quad's four pre-activations): a launch each, so that
// the compiler cannot share arithmetic between the forms whose bits the test compares
template <int FORM> __global__ __launch_bounds__(64) void debug_gate_cell_kernel(const float *pre, const float *c_in, float *cell)
{
    const int w = blockIdx.x, l = threadIdx.x, u = l >> 2;
    const float *p = pre + (size_t)w * 64;
    float c = c_in[(size_t)w * 16 + u], h = 0.f;
    if constexpr (FORM == 1)
    {
        CellLane cl;
        cl.init(l);
        lstm_cell_flat(p[l], cl, c, h);
    }
    else if constexpr (FORM == 3)
    {
        if ((l & 3) == 0)
        {
            float c_t;
            h = lstm_cell_lane<false>(p[l], p[l + 1], p[l + 2], p[l + 3], c, c_t);
            c = c_t;
        }
    }
    else
        lstm_cell<FORM == 2>(p[l], l, c, h);
    if ((l & 3) == 0)
    {
        cell[((size_t)w * 2 + 0) * 16 + u] = c;
        cell[((size_t)w * 2 + 1) * 16 + u] = h;
    }
}

} // namespace umx
