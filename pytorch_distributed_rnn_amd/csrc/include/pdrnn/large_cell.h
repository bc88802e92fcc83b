// The LSTM / GRU cell of the large-H recurrence kernels (lstm_large.hip,
// lstm_rows_f32.hip): the arithmetic only, on fp32 values -- no memory access
// and no storage type.  Every kernel keeps its own loads, stores, prefetch
// registers and vector widths and calls these two functions, so the per-step,
// ping-pong, persistent and row-owning paths compute the same bits.
//
// CELL 0 = LSTM (torch gate order i, f, g, o; state = c).
// CELL 1 = GRU on the LSTM quad [r | z | n_x | n_h] (n_x = W_in x + b_in,
// n_h = W_hn h + b_hn; state = the fp32 h); the saved quad is (r, z, n, n_h).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "pdrnn/common.h"

namespace pdrnn {

// g: the four summed pre-activations in, the saved quad out.  state: c_{t-1}
// (LSTM) / h_{t-1} (GRU) in, c_t / h_t out.  Returns h_t.
template <int CELL>
PDRNN_DEVICE float cell_fwd(float (&g)[4], float& state) {
  if constexpr (CELL == 0) {
    g[0] = sigmoidf_fast(g[0]);
    g[1] = sigmoidf_fast(g[1]);
    g[2] = tanhf_fast(g[2]);
    g[3] = sigmoidf_fast(g[3]);
    state = fmaf(g[1], state, g[0] * g[2]);
    return g[3] * tanhf_fast(state);
  } else {
    // n = tanh(n_x + r n_h) takes n_x's slot in the saved quad;
    // h = n + z (h_prev - n) with the fp32 h_prev
    g[0] = sigmoidf_fast(g[0]);
    g[1] = sigmoidf_fast(g[1]);
    g[2] = tanhf_fast(fmaf(g[0], g[3], g[2]));
    state = fmaf(g[1], state - g[2], g[2]);
    return state;
  }
}

// dh: the gradient of h_t after the caller has added dout (and, for the GRU,
// the carry).  a0..a3: the saved quad; cur: c_t (LSTM only); sp: c_{t-1} /
// h_{t-1}.  dg: the four gate gradients in gate-blocked (torch row) order.
// carry: LSTM dc flowing in from step t+1, GRU the direct path dh_{t+1}
// z_{t+1}; advanced to the value step t-1 needs.
//   LSTM: dc = carry + dh o (1 - tanh(c)^2)
//         dg = [dc g i(1-i), dc c_prev f(1-f), dc i (1-g^2), dh tanh(c) o(1-o)], carry = dc f
//   GRU:  h = n + z (h_prev - n), n = tanh(n_x + r n_h):
//         dg = [dr r(1-r) | dz z(1-z) | dpre_n (x side) | dpre_n r (n_h side)], carry = dh z
template <int CELL>
PDRNN_DEVICE void cell_bwd(float dh, float a0, float a1, float a2, float a3, float cur, float sp, float& carry,
                           float (&dg)[4]) {
  if constexpr (CELL == 0) {
    const float tc = tanhf_fast(cur);
    const float dc = fmaf(dh * a3, 1.f - tc * tc, carry);
    dg[0] = dc * a2 * a0 * (1.f - a0);
    dg[1] = dc * sp * a1 * (1.f - a1);
    dg[2] = dc * a0 * (1.f - a2 * a2);
    dg[3] = dh * tc * a3 * (1.f - a3);
    carry = dc * a1;
  } else {
    const float dpn = dh * (1.f - a1) * (1.f - a2 * a2);
    dg[0] = dpn * a3 * a0 * (1.f - a0);
    dg[1] = dh * (sp - a2) * a1 * (1.f - a1);
    dg[2] = dpn;
    dg[3] = dpn * a0;
    carry = dh * a1;
  }
}

// Host dispatch on the cell id: f(std::integral_constant<int, CELL>).
template <class F>
inline hipError_t with_cell(int cell, F&& f) {
  if (cell == 0) return f(std::integral_constant<int, 0>{});
  if (cell == 1) return f(std::integral_constant<int, 1>{});
  return hipErrorInvalidValue;
}

}  // namespace pdrnn
