// Sequence-in-wave LSTM / GRU stack (H = 32, 1-2 layers), forward and lean
// BPTT, fp32, gfx950.  The motion model's recurrence (reference: nn.LSTM in
// src/motion/model.py:9,14, trained by src/motion/trainer/base.py:111,116;
// the GRU cell through the packed 4-block stack, CELL = 1, see load_fwd_w).
//
// Why a second small-H family (docs/DESIGN.md §2b): the gate-split kernels of
// lstm_small.hip spread one sequence over 4 waves (a layer = 128 lanes, one
// gate row each), so every step broadcasts the 64-float operand vector from
// LDS to all 4 waves (16 ds_read_b128 per lane, the LDS serialises the four
// waves' reads: ~276 of 966 cycles at B = 180) and crosses an s_barrier
// (~216 cycles).  Here a sequence never leaves its wave:
//
//  * lane = (unit u = lane >> 1, K half s = lane & 1).  A lane holds the four
//    gate rows q*H + u of [W_ih | W_hh] over ITS half of the operand vector
//    (layer >= 1: s = 0 the input h^{l-1}_t, s = 1 the own h_{t-1}; layer 0:
//    s = 0 x_t (12 columns, zero-padded) + h[0, 12), s = 1 h[12, 32)), as k
//    pairs for v_pk_fma_f32.  Half the operand vector per lane: 8 (layer 1) /
//    6 (layer 0) ds_read_b128 per step, the two halves' addresses on disjoint
//    banks.  One DPP swap adds the partner's partial sums.
//  * lane s = 0 activates i, g and lane s = 1 f, o (rows pre-scaled by
//    -log2 e, x2 for g: sigma = 1 / (1 + 2^z), tanh(g) = 2 sigma(2g) - 1); two
//    DPP swaps give both lanes all four gates; both update c, h.
//  * h_t goes to a per-wave LDS slot and is read back by the same wave next
//    step: LDS operations of one wave execute in order, so no barrier and no
//    waitcnt beyond the reads' own.  A two-layer stack runs each layer in
//    its own wave (one barrier per step, h^0 handed over through parity
//    slots).
//  * BPTT, per layer: lane (u, s) owns column u of W_hh (and W_ih for
//    layers >= 1: the input gradient feeding the layer below) over gate rows
//    [64 s, 64 s + 64); the row phase makes the lane's two pre-activation gate
//    gradients (s = 0: i, f; s = 1: g, o) from the saved activations, writes
//    them to LDS and over the activation slots (deferred dW, lstm_small_dw.hip),
//    and the column phase reads its 64 rows back (16 ds_read_b128) for
//    W^T dz; one DPP swap completes the sums.  Layer 1's input gradient
//    reaches layer 0's wave through LDS parity slots.
//  * How sequences and layers lie over waves is a WAVE MAP: the table kMaps
//    below holds one row per map id, and every kernel constant, launch
//    geometry and planner rule reads it.  pdrnn_lstm_sw_plan picks the maps
//    of a batch (docs/DESIGN.md §2b).
//  * Every forward body also has an inference build (INFER): the same step
//    with nothing saved, no global store in the step loop, and a head that
//    writes logits / predictions / per-sequence statistics
//    (pdrnn_lstm_sw_infer, pdrnn_lstm_sw_infer_plan).
#include "pdrnn/api.h"
#include "pdrnn/common.h"
#include "pdrnn/motion_head.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace pdrnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH = 32;
constexpr float kA = -1.4426950408889634f;  // -log2(e): rows pre-scaled so sigma(z) = 1 / (1 + 2^acc)
constexpr int kHB = 36;                     // h slot: 32 values + a zero chunk (layer 0, s = 1, chunk 5)
constexpr int kXS = 12;                     // staged x row: I <= 12 columns, zero-padded
constexpr int kDZ = 4 * kH + 4;             // dz vector, rows >= 64 shifted by 4 floats (bank spread)
constexpr uint32_t kOOR = 0x80000000u;      // buffer offset past the range: the store is dropped

// bf16 models: fp32 masters rounded to bf16 as they load (round to nearest even)
PDRNN_DEVICE float wround(float v, int w_bf16) { return w_bf16 ? (float)(__bf16)v : v; }
PDRNN_DEVICE float sig2(float z) { return fast_rcp(1.f + __builtin_amdgcn_exp2f(z)); }
PDRNN_DEVICE float tanh_c(float c) { return fmaf(sig2(c * (2.f * kA)), 2.f, -1.f); }
PDRNN_DEVICE float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
PDRNN_DEVICE pdrnn_f2 lo2(float4 v) { return pdrnn_f2{v.x, v.y}; }
PDRNN_DEVICE pdrnn_f2 hi2(float4 v) { return pdrnn_f2{v.z, v.w}; }
PDRNN_DEVICE pdrnn_f2 pfma(pdrnn_f2 a, pdrnn_f2 b, pdrnn_f2 c) { return __builtin_elementwise_fma(a, b, c); }
PDRNN_DEVICE void bstore(float v, __amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, vo, so, 0);
}
PDRNN_DEVICE int dz_slot(int r) { return r + (r >= 2 * kH ? 4 : 0); }
// sum of this lane's value and its K-half partner's (lanes 2u, 2u + 1)
PDRNN_DEVICE float pair_sum(float v) { return v + dpp_swap1(v); }

template <int NB>
PDRNN_DEVICE int pick(const int (&v)[NB], int n) {
  if constexpr (NB == 1) return v[0];
  else if constexpr (NB == 2) return n == 0 ? v[0] : v[1];
  else return n == 0 ? v[0] : n == 1 ? v[1] : v[2];
}

// ---------------------------------------------------------------------------
// Wave maps: how sequences and layers are laid over waves.  One row per map
// id (the `mode` of pdrnn_lstm_sw_fwd / _bwd, PDRNN_TUNE sw_mode /
// sw_bwd_mode); everything that is a property of the map is read from here --
// the kernels' template constants, __launch_bounds__, the launchers' grid,
// block and LDS, the planner's override check.  A map serves only the passes
// and layer counts its row lists.
//   0 / 1  one layer: a wave runs 1 / 2 whole sequences.
//   2      two layers, wave l runs layer l of one sequence; one barrier per
//          step (h^0_t / the input gradient handed over through parity slots).
//   3      backward of map 2 with two sequences per layer wave.
//   4      backward of map 2 plus two waves that accumulate the weight
//          gradients on the matrix cores (register dW: no gate-gradient
//          stores, no dW launch; an 8-slot dz ring holds a 4-step K step).
//   5      forward, four waves per sequence (lstm_sw_fwd4_kernel).
//   6      forward of map 2 capped at 168 VGPRs: three waves per SIMD.
//   8      map 6 with layer 1's input projection on the matrix cores per
//          16-step chunk (lstm_sw_fwd8_kernel), the same bits.
// (Removed, measured slower: 7, three sequences per layer wave -- forward
// +28 us, BPTT +20 us against 6 / 3 at B = 1440, profiles/r6/m7_ab.md; both
// layers of a two-layer stack in one wave, maps 0 / 1 / forward 3 at NL = 2 --
// forward 117.4 vs 68.2 us and backward 165.7 vs 53.2 us at B = 180 against
// map 2, profiles/r5/sw/sw1_probe.log.)
// ---------------------------------------------------------------------------
struct WaveMap {
  bool fwd, bwd;     // passes served
  bool nl1, nl2;     // layer counts served
  int nb;            // sequences per wave (= per workgroup)
  bool split;        // each layer in waves of its own
  int waves;         // waves per workgroup
  int eu_cap;        // amdgpu_waves_per_eu of the forward kernels (3: <= 168 VGPRs; 1: uncapped)
  bool rdw;          // register dW: two more waves on the matrix cores
  int zr;            // dz ring slots per (sequence, layer), backward
  int t_mult;        // T must be a multiple of this
};
constexpr int kNumMaps = 9;
constexpr WaveMap kMaps[kNumMaps] = {
    //       fwd    bwd    nl1    nl2    nb split  waves eu rdw    zr  t_mult
    /* 0 */ {true,  true,  true,  false, 1, false, 1,    1, false, 2,  1},
    /* 1 */ {true,  true,  true,  false, 2, false, 1,    1, false, 2,  1},
    /* 2 */ {true,  true,  false, true,  1, true,  2,    1, false, 2,  1},
    /* 3 */ {false, true,  false, true,  2, true,  2,    1, false, 2,  1},
    /* 4 */ {false, true,  false, true,  1, true,  4,    1, true,  8,  4},
    /* 5 */ {true,  false, false, true,  1, true,  4,    1, false, 0,  1},
    /* 6 */ {true,  false, false, true,  1, true,  2,    3, false, 0,  1},
    /* 7 */ {false, false, false, false, 1, false, 1,    1, false, 0,  1},  // (removed)
    /* 8 */ {true,  false, false, true,  1, true,  2,    3, false, 0,  16},
};
constexpr bool map_serves(int map, bool backward, int NL) {
  return map >= 0 && map < kNumMaps && (backward ? kMaps[map].bwd : kMaps[map].fwd) &&
         (NL == 1 ? kMaps[map].nl1 : NL == 2 && kMaps[map].nl2);
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
// This lane's four gate rows over NC float4 chunks of its operand half, k
// pairs, in the order (m0, x0, m1, x1): m0 / m1 are the gates this lane
// activates (s = 0: i, g; s = 1: f, o) and x0 / x1 the ones its partner
// activates.  After the loop the sum of w[0] is this lane's own partial of
// m0 and the sum of w[1] the partial its partner needs (and likewise for
// m1): one DPP add per gate finishes the K-split sum, with no select.  The
// biases of m0 / m1 seed their accumulators.
template <int NC>
struct FwdW {
  pdrnn_f2 w[4][2 * NC];
  float bias[2];
};

// Column of chunk c, element e (-1: zero) -- see the file comment.
PDRNN_DEVICE int fwd_col(int l, int s, int c, int e, int Iin, bool& from_ih) {
  if (l == 0) {
    if (s == 0) {
      if (c < 3) { from_ih = true; const int k = 4 * c + e; return k < Iin ? k : -1; }
      from_ih = false; return 4 * (c - 3) + e;
    }
    from_ih = false; return c < 5 ? 12 + 4 * c + e : -1;
  }
  from_ih = s == 0;
  return 4 * c + e;
}

// CELL 1 = GRU, packed by the host as a 4-row-block stack with zero blocks
// (W_ih: [W_ir; W_iz; W_in; 0], W_hh: [W_hr; W_hz; 0; W_hn], ops/gru_fused.py),
// so the products are the LSTM's: rows (r, z, n_x, n_h) with n_x / n_h scaled
// by 2 kA (tanh(n_x + r n_h) = 2 sigma(2 (n_x + r n_h)) - 1 is linear in both).
template <int NC, int CELL = 0>
PDRNN_DEVICE FwdW<NC> load_fwd_w(const PdrnnLstmSmallFwdArgs& a, int l, int u, int s) {
  FwdW<NC> W;
  const int Iin = l == 0 ? a.I : kH;
  const float* wih = a.w_ih[l];
  const float* whh = a.w_hh[l];
  const int gq[4] = {s, 1 - s, 2 + s, 3 - s};  // (m0, x0, m1, x1)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = gq[j];
    const int r = q * kH + u;
    const float sc = kA * ((CELL == 0 ? q == 2 : q >= 2) ? 2.f : 1.f);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool ih = false;
        const int k = fwd_col(l, s, c, e, Iin, ih);
        float x = 0.f;
        if (k >= 0) x = ih ? wih[(int64_t)r * Iin + k] : whh[(int64_t)r * kH + k];
        v[e] = wround(x, a.w_bf16) * sc;
      }
      W.w[j][2 * c] = pdrnn_f2{v[0], v[1]};
      W.w[j][2 * c + 1] = pdrnn_f2{v[2], v[3]};
    }
    if (!(j & 1))
      W.bias[j >> 1] = ((a.b_ih[l] ? wround(a.b_ih[l][r], a.w_bf16) : 0.f) +
                        (a.b_hh[l] ? wround(a.b_hh[l][r], a.w_bf16) : 0.f)) * sc;
  }
  return W;
}

// p[0] / p[2]: own partials of m0 / m1 (+ bias), p[1] / p[3]: the partner's
// (eight accumulators instead of four -- a gate's lo / hi halves apart, no
// back-to-back dependent v_pk_fma_f32 -- measured no faster: a wave alone on
// its SIMD issues v_pk_fma_f32 at ~8 cycles, so the products are issue-bound,
// profiles/r6/fwd_phase_stamps.md)
template <int NC>
PDRNN_DEVICE void fwd_dot(const FwdW<NC>& W, const float4 (&v)[NC], float (&p)[4]) {
  pdrnn_f2 acc[4] = {{W.bias[0], 0.f}, {0.f, 0.f}, {W.bias[1], 0.f}, {0.f, 0.f}};
#ifdef SW_PROBE_HALF_K  // timing probe only (wrong numerics): half the products
#pragma unroll
  for (int c = 0; c < NC / 2; ++c) {
#else
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#endif
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = pfma(W.w[j][2 * c], lo2(v[c]), acc[j]);
      acc[j] = pfma(W.w[j][2 * c + 1], hi2(v[c]), acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = acc[j].x + acc[j].y;
}

struct Cell {
  float a0, a1, c, h;
};
// DPP quad_perm [1, 1, 3, 3]: both lanes of a pair read the odd lane
PDRNN_DEVICE float from_odd(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xF5, 0xF, 0xF, false));
}
// The K-split sums -> this lane's two activations (s = 0: i, g; s = 1: f, o;
// `gk` = {2, -1} on even lanes: tanh(g) = 2 sigma(2g) - 1, {1, 0} on odd) and
// the unit's new c, h on both lanes: c = f c + i g is the sum of one product
// per lane (odd: f c, even: i g), h = o tanh(c) with o read from the odd lane.
PDRNN_DEVICE Cell fwd_cell_z(float z0, float z1, pdrnn_f2 gk, float c, bool odd) {
  Cell r;
  r.a0 = sig2(z0);
  r.a1 = fmaf(sig2(z1), gk.x, gk.y);
  const float term = r.a0 * (odd ? c : r.a1);
  r.c = term + dpp_swap1(term);
  r.h = from_odd(r.a1) * tanh_c(r.c);
  return r;
}
PDRNN_DEVICE Cell fwd_cell(const float (&p)[4], pdrnn_f2 gk, float c, bool odd) {
  return fwd_cell_z(p[0] + dpp_swap1(p[1]), p[2] + dpp_swap1(p[3]), gk, c, odd);
}
// GRU: lane s = 0 holds r and n_x, s = 1 z and n_h (2 kA-scaled); one DPP
// swap each gives both lanes all four, then n = tanh(n_x + r n_h) and
// h = n + z (h_prev - n) on both.  Saved slots: a0 = r | z, a1 = n_x | n_h
// (unscaled; the BPTT reads n_h), c = n.
PDRNN_DEVICE Cell fwd_cell_gru_z(float z0, float z1, float hprev, bool odd) {
  Cell r;
  r.a0 = sig2(z0);
  const float a0p = dpp_swap1(r.a0), z1p = dpp_swap1(z1);
  const float rg = odd ? a0p : r.a0, zg = odd ? r.a0 : a0p;
  const float nx = odd ? z1p : z1, nh = odd ? z1 : z1p;
  r.a1 = z1 * (1.f / (2.f * kA));
  r.c = fmaf(sig2(fmaf(rg, nh, nx)), 2.f, -1.f);
  r.h = fmaf(zg, hprev - r.c, r.c);
  return r;
}
PDRNN_DEVICE Cell fwd_cell_gru(const float (&p)[4], float hprev, bool odd) {
  return fwd_cell_gru_z(p[0] + dpp_swap1(p[1]), p[2] + dpp_swap1(p[3]), hprev, odd);
}
template <int CELL>
PDRNN_DEVICE Cell fwd_cell_any(const float (&p)[4], pdrnn_f2 gk, float c, float hprev, bool odd) {
  if constexpr (CELL == 0) return fwd_cell(p, gk, c, odd);
  else return fwd_cell_gru(p, hprev, odd);
}
// The saved rows of a step: this lane's two activations and the unit's c to
// row `rw` of act (5H floats a row), h to hseq.  `m`: kOOR drops the stores.
PDRNN_DEVICE void store_cell(const Cell& r, __amdgpu_buffer_rsrc_t r_act, __amdgpu_buffer_rsrc_t r_h, uint32_t vo_a0,
                             uint32_t vo_a1, uint32_t vo_c, uint32_t vo_h, uint32_t m, uint32_t rw) {
  bstore(r.a0, r_act, vo_a0 | m, rw * (5 * kH * 4));
  bstore(r.a1, r_act, vo_a1 | m, rw * (5 * kH * 4));
  bstore(r.c, r_act, vo_c | m, rw * (5 * kH * 4));
  bstore(r.h, r_h, vo_h | m, rw * (kH * 4));
}

// Per-workgroup stamps (PDRNN_LSTM_STAMPS), thread 0, a row of a.stamps:
// [0] / [1] the cycle counter at the loop's start / end, [2] / [3] real time
// there, [4] / [5] real time at kernel entry / exit, [6] the CU.
PDRNN_DEVICE uint64_t stamp_entry(const uint64_t* stamps, int tid) { return (stamps && tid == 0) ? stamp_real() : 0; }
PDRNN_DEVICE void stamp_loop_begin(const uint64_t* stamps, int tid, uint64_t& st0, uint64_t& sr0) {
  st0 = 0; sr0 = 0;
  if (stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }
}
PDRNN_DEVICE void stamp_loop_end(uint64_t* st, uint64_t st0, uint64_t sr0) {
  st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = stamp_real();
}
PDRNN_DEVICE void stamp_exit(uint64_t* st, uint64_t sr_in) {
  st[4] = sr_in; st[5] = stamp_real(); st[6] = stamp_cu();
}

template <int NL, int NB>
PDRNN_DEVICE constexpr int fwd_lds_floats_hb() { return NB * NL * 2 * kHB; }

// x staging (forward prologue): NB sequences' [T, I] input rows into the LDS
// rows xs[(n T + t) kXS + k] (zero-padded to kXS; the caller zeroed xs) and,
// when xg_out is set, the fp32 rows [b T + t][xg_ld] of the deferred dW (pad
// columns written as zeros).  A sequence's rows are one contiguous block of the
// motion batch: 16-byte loads of the block, all of a thread's rounds in flight
// at once (element-wise loads, one dependent round per 4 elements per thread,
// cost the single-layer forward 16 us of ~100 at B = 1440, 23 with bf16 x,
// profiles/r6/x_staging.md).  Returns false when the layout does not allow it.
// INFER: the inference builds, no xg_out copy.
template <int NB, bool INFER = false>
PDRNN_DEVICE bool stage_x_vec(const PdrnnLstmSmallFwdArgs& a, float* xs, const int (&bsrc)[NB], const int (&bidx)[NB],
                              const int (&vint)[NB], int tid, int nthr) {
  const int T = a.T, I = a.I;
  const int esz = a.x_bf16 ? 2 : 4;
  const int per = T * I;
  if (a.x_st != I || a.x_sb != (int64_t)per || (per * esz) % 16 != 0 ||
      (reinterpret_cast<uintptr_t>(a.x) & 15) != 0)
    return false;
  const int cpe = 16 / esz;  // elements per 16-byte chunk
  const int nch = per / cpe;
  const int tot = NB * nch;
  const int xg_ld = a.xg_ld;
  const char* xb = reinterpret_cast<const char*>(a.x);
  constexpr int R = 8;  // chunks per thread in flight
  for (int c0 = tid; c0 < tot; c0 += R * nthr) {
    uint4 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = min(c0 + r * nthr, tot - 1);
      const int n = c / nch, q = c - n * nch;
      v[r] = *reinterpret_cast<const uint4*>(xb + ((int64_t)pick<NB>(bsrc, n) * per + (int64_t)q * cpe) * esz);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = c0 + r * nthr;
      if (c < tot) {
        const int n = c / nch, q = c - n * nch;
        const uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
        const int e0 = q * cpe;
        int t = e0 / I, k = e0 - t * I;  // (one division per chunk, then stepped)
        float* xrow = xs + (n * T + t) * kXS;
        float* grow = nullptr;  // (stays null in the inference builds: the copies below fold away)
        if constexpr (!INFER) grow = a.xg_out ? a.xg_out + ((int64_t)pick<NB>(bidx, n) * T + t) * xg_ld : nullptr;
        const bool gv = grow != nullptr && pick<NB>(vint, n);
        for (int j = 0; j < cpe; ++j) {
          const float val = esz == 2 ? __uint_as_float((j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu) << 16)
                                     : __uint_as_float(w[j]);
          xrow[k] = val;
          if (gv && k < xg_ld) grow[k] = val;
          if (++k == I) {
            k = 0;
            xrow += kXS;
            if (grow) grow += xg_ld;
          }
        }
      }
    }
  }
  if (!INFER && a.xg_out && xg_ld > I) {  // the dW kernel reads xg_ld columns: zero pads
    const int padw = xg_ld - I;
    for (int e = tid; e < NB * T * padw; e += nthr) {
      const int n = e / (T * padw), rem = e - n * (T * padw);
      const int t = rem / padw, k = I + rem - t * padw;
      if (pick<NB>(vint, n)) a.xg_out[((int64_t)pick<NB>(bidx, n) * T + t) * xg_ld + k] = 0.f;
    }
  }
  return true;
}

// Maps 0 / 1 (one layer) and 2 / 6 (two layers, a wave per layer).  Map 6
// holds <= 168 VGPRs: three waves per SIMD, so B = 1440 (2880 layer waves on
// 1024 SIMDs) is one residency round with every SIMD loaded evenly.
// INFER (here and in fwd4_body / lstm_sw_fwd8_kernel): the inference build.
// The step is the same source, so h_n / c_n are the training build's bits,
// but nothing is saved -- no act / hseq rows, no xg_out copy, no global store
// in the step loop -- and the epilogue's head is motion_head_infer.
template <int NL, int MODE, int CELL = 0, bool INFER = false>
__global__ void __launch_bounds__(64 * kMaps[MODE].waves) __attribute__((amdgpu_waves_per_eu(kMaps[MODE].eu_cap)))
lstm_sw_fwd_kernel(PdrnnLstmSmallFwdArgs a) {
  constexpr int NB = kMaps[MODE].nb;
  constexpr bool SPLIT = kMaps[MODE].split;
  static_assert(map_serves(MODE, false, NL), "the wave map table lists no such forward");
  static_assert(SPLIT == (NL == 2), "one layer per wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x, nthr = blockDim.x;
  const uint64_t sr_in = stamp_entry(a.stamps, tid);  // (the prologue's cost)
  const int lane = tid & 63;
  const int wv = SPLIT ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int u = lane >> 1;
  const bool odd = (lane & 1) != 0;
  const int B = a.B, T = a.T, I = a.I;
  const int bbase = blockIdx.x * NB;
  float* hb = smem;
  float* xs = smem + fwd_lds_floats_hb<NL, NB>();
  auto hbuf = [&](int n, int l, int p) { return hb + ((n * NL + l) * 2 + p) * kHB; };

  int bidx[NB], bsrc[NB], vint[NB];
  bool valid[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    valid[n] = b < B;
    vint[n] = valid[n] ? 1 : 0;
    bidx[n] = valid[n] ? b : B - 1;  // an empty slot recomputes the last sequence, stores nothing
    bsrc[n] = a.idx ? (int)a.idx[bidx[n]] : bidx[n];
  }

  // ---- prologue: zero the h slots (h_{-1} = 0, pad chunks), stage x ------
  // (the vector staging writes only the I real columns: xs zeroed first; two
  // sequences per workgroup only -- with one, the zeroing pass and barrier
  // cost more than the element loads: map 6 136.2 vs 133.6 us at B = 1440)
  const bool xvec = NB == 2 && a.x_st == I && a.x_sb == (int64_t)T * I;
  for (int e = tid; e < fwd_lds_floats_hb<NL, NB>() + (xvec ? NB * T * kXS : 0); e += nthr) hb[e] = 0.f;
  if (xvec) lds_barrier();
  if (!(xvec && stage_x_vec<NB, INFER>(a, xs, bsrc, bidx, vint, tid, nthr))) {
    const int per = T * kXS, tot = NB * per;
    const int xg_ld = a.xg_ld;
    for (int e0 = tid; e0 < tot; e0 += 4 * nthr) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = min(e0 + r * nthr, tot - 1);
        const int n = e / per, rem = e - n * per;
        const int t = rem / kXS, k = rem - t * kXS;
        const float x = ldx(a.x, (int64_t)pick<NB>(bsrc, n) * a.x_sb + (int64_t)t * a.x_st + min(k, I - 1), a.x_bf16);
        v[r] = k < I ? x : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = e0 + r * nthr;
        if (e < tot) {
          const int n = e / per, rem = e - n * per;
          const int t = rem / kXS, k = rem - t * kXS;
          xs[e] = v[r];
          if (!INFER && a.xg_out && k < xg_ld && pick<NB>(vint, n))
            a.xg_out[((int64_t)pick<NB>(bidx, n) * T + t) * xg_ld + k] = v[r];
        }
      }
    }
  }
  // the LDS rows are in place; the xg_out stores (read by a later launch) need
  // not drain here -- a __syncthreads() would wait for them (~1-3 us)
  lds_barrier();

  // (the saved rows' descriptors, lane offsets, masks and row(): used by
  // store_cell alone, so the inference builds, where a.act / a.hseq are null
  // and store_cell is compiled out, form none of them)
  const __amdgpu_buffer_rsrc_t r_act = uniform_rsrc(a.act);
  const __amdgpu_buffer_rsrc_t r_h = uniform_rsrc(a.hseq);
  const uint32_t s_ = odd ? 1u : 0u;
  const uint32_t vo_a0 = (s_ * kH + u) * 4, vo_a1 = ((2 + s_) * kH + u) * 4, vo_c = (4 * kH + u) * 4, vo_h = u * 4;
  uint32_t vmask[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) vmask[n] = valid[n] ? 0u : kOOR;
  // byte offset of row (l, b, t) in act (5H floats per row) and hseq (H)
  auto row = [&](int l, int n, int t) -> uint32_t {
    return __builtin_amdgcn_readfirstlane((uint32_t)(((l * B + pick<NB>(bidx, n)) * T + t)));
  };

  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }

  // state: c and the last committed h per (layer, sequence)
  float cst[NL][NB], hst[NL][NB];
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int n = 0; n < NB; ++n) { cst[l][n] = 0.f; hst[l][n] = 0.f; }

  // Layer 0 at time t (active unless t == T) / layer 1 at time t (active
  // unless t < 0), for all NB sequences, split into the operand reads and the
  // rest (the uncapped maps pin every read ahead of the first FMA).
  auto rd0 = [&](int t, float4 (&v)[NB][6]) {
    const int tc = min(t, T - 1);
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const float* hp = hbuf(n, 0, (t - 1) & 1);
      const float* pa = odd ? hp + 12 : xs + (n * T + tc) * kXS;
      const float* pb = odd ? hp + 24 : hp;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[n][c] = ld4(pa + 4 * c);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[n][3 + c] = ld4(pb + 4 * c);
    }
  };
  auto rd1 = [&](int t, float4 (&v)[NB][8]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const float* pc = odd ? hbuf(n, 1, (t - 1) & 1) : hbuf(n, 0, t & 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) v[n][c] = ld4(pc + 4 * c);
    }
  };
  auto commit = [&](int l, int n, int t, bool act, const Cell& r) {
    cst[l][n] = act ? r.c : cst[l][n];
    hst[l][n] = act ? r.h : hst[l][n];
    hbuf(n, l, t & 1)[u] = hst[l][n];
    if constexpr (!INFER) {
      const uint32_t rw = row(l, n, min(max(t, 0), T - 1));
      store_cell(r, r_act, r_h, vo_a0, vo_a1, vo_c, vo_h, act ? vmask[n] : kOOR, rw);
    }
  };
  const pdrnn_f2 gk = odd ? pdrnn_f2{1.f, 0.f} : pdrnn_f2{2.f, -1.f};
  auto cmp0 = [&](const FwdW<6>& W, int t, const float4 (&v)[NB][6]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float p[4];
      fwd_dot<6>(W, v[n], p);
      commit(0, n, t, t < T, fwd_cell_any<CELL>(p, gk, cst[0][n], hst[0][n], odd));
    }
  };
  auto cmp1 = [&](const FwdW<8>& W, int t, const float4 (&v)[NB][8]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float p[4];
      fwd_dot<8>(W, v[n], p);
      commit(NL - 1, n, t, t >= 0, fwd_cell_any<CELL>(p, gk, cst[NL - 1][n], hst[NL - 1][n], odd));
    }
  };

  if constexpr (NL == 1) {
    const FwdW<6> W0 = load_fwd_w<6, CELL>(a, 0, u, odd ? 1 : 0);
    for (int t = 0; t < T; ++t) {
      float4 v0[NB][6];
      rd0(t, v0);
      cmp0(W0, t, v0);
    }
  } else {
    // uncapped: every operand read of the step in flight before the first
    // FMA (one LDS latency per step); under the register cap the reads are
    // left to the scheduler, which pairs them to stay within its registers
    constexpr bool PIN_READS = kMaps[MODE].eu_cap == 1;
    if (wv == 0) {
      const FwdW<6> W0 = load_fwd_w<6, CELL>(a, 0, u, odd ? 1 : 0);
      for (int it = 0; it <= T; ++it) {
        if (it < T) {
          float4 v0[NB][6];
          rd0(it, v0);
          if constexpr (PIN_READS) __builtin_amdgcn_sched_barrier(0);
          cmp0(W0, it, v0);
        }
        lds_barrier();
      }
    } else {
      const FwdW<8> W1 = load_fwd_w<8, CELL>(a, 1, u, odd ? 1 : 0);
      for (int it = 0; it <= T; ++it) {
        if (it > 0) {
          float4 v1[NB][8];
          rd1(it - 1, v1);
          if constexpr (PIN_READS) __builtin_amdgcn_sched_barrier(0);
          cmp1(W1, it - 1, v1);
        }
        lds_barrier();
      }
    }
  }
  uint64_t sr1 = 0;
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    sr1 = stamp_real();
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = sr1;
  }

  // ---- epilogue: h_n / c_n, then the fused head on the top layer's h_T ----
  // (two sequences per wave: both heads' operands loaded first, their
  // dependent loads in flight together, not behind the first head's stores;
  // one sequence loads inline -- the VGPR-capped map 6 would spill)
  const bool top_wave = !SPLIT || wv == NL - 1;
  HeadIn hin[NB];
  if constexpr (NB > 1) {
    if (a.head_w && top_wave) {
#pragma unroll
      for (int n = 0; n < NB; ++n)
        hin[n] = INFER ? head_load_infer(a, pick<NB>(bidx, n), u) : head_load(a, pick<NB>(bidx, n), u);
    }
  }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    if (!valid[n]) continue;
    const int b = bbase + n;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (SPLIT && l != wv) continue;
      if (!odd && a.hn) a.hn[((int64_t)l * B + b) * kH + u] = hst[l][n];
      if (!odd && a.cn) a.cn[((int64_t)l * B + b) * kH + u] = cst[l][n];
    }
    if (a.head_w && top_wave) {
      if constexpr (INFER) {
        if constexpr (NB > 1) motion_head_infer(a, b, hst[NL - 1][n], u, odd, hin[n]);
        else motion_head_infer(a, b, hst[NL - 1][n], u, odd);
      } else {
        if constexpr (NB > 1) motion_head(a, b, hst[NL - 1][n], u, odd, hin[n]);
        else motion_head(a, b, hst[NL - 1][n], u, odd);
      }
    }
  }
  if (a.stamps && tid == 0) stamp_exit(a.stamps + (uint64_t)blockIdx.x * 8, sr_in);
}

// ---------------------------------------------------------------------------
// Forward, four waves per sequence (map 5, two-layer stacks in the latency
// regime): wave w runs layer w >> 1, units 16 (w & 1) .. + 15.  lane =
// (unit ul = lane >> 2, K quarter q = lane & 3): a lane holds the four gate
// rows of its unit over a quarter of the operand vector (layer 0: x | h[0,12)
// | h[12,24) | h[24,32) + zero pad, 3 float4 chunks; layer 1: h^0[0,16) |
// h^0[16,32) | h^1[0,16) | h^1[16,32), 4 chunks), half of map 2's products
// per lane.  A quad reduce-scatter (xor 2, then xor 1) leaves lane q with the
// full pre-activation of gate q (i, f, g, o): one activation per lane; quad
// broadcasts give every lane of the unit i, f, g, o for c and h.  The two
// waves of a layer meet in the per-layer h slots: one barrier per step, as in
// map 2.
// ---------------------------------------------------------------------------
template <int NC>
struct Fwd4W {
  pdrnn_f2 w[4][2 * NC];
};

PDRNN_DEVICE float quad_bcast(float v, int k) {
  switch (k) {
    case 0: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x00, 0xF, 0xF, false));
    case 1: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x55, 0xF, 0xF, false));
    case 2: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xAA, 0xF, 0xF, false));
    default: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xFF, 0xF, 0xF, false));
  }
}

// column of layer l, quarter q, chunk c, element e (-1: zero)
PDRNN_DEVICE int fwd4_col(int l, int q, int c, int e, int Iin, bool& from_ih) {
  const int k = 4 * c + e;
  if (l == 0) {
    if (q == 0) { from_ih = true; return k < Iin ? k : -1; }
    from_ih = false;
    const int hk = 12 * (q - 1) + k;
    return hk < kH ? hk : -1;
  }
  from_ih = q < 2;
  return 16 * (q & 1) + k;
}

template <int NC, int CELL = 0>
PDRNN_DEVICE Fwd4W<NC> load_fwd4_w(const PdrnnLstmSmallFwdArgs& a, int l, int u, int q, float (&bias)[4]) {
  Fwd4W<NC> W;
  const int Iin = l == 0 ? a.I : kH;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = j * kH + u;
    const float sc = kA * ((CELL == 0 ? j == 2 : j >= 2) ? 2.f : 1.f);  // (GRU: see load_fwd_w)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool ih = false;
        const int k = fwd4_col(l, q, c, e, Iin, ih);
        float x = 0.f;
        if (k >= 0) x = ih ? a.w_ih[l][(int64_t)r * Iin + k] : a.w_hh[l][(int64_t)r * kH + k];
        v[e] = wround(x, a.w_bf16) * sc;
      }
      W.w[j][2 * c] = pdrnn_f2{v[0], v[1]};
      W.w[j][2 * c + 1] = pdrnn_f2{v[2], v[3]};
    }
    bias[j] = q == 0 ? ((a.b_ih[l] ? wround(a.b_ih[l][r], a.w_bf16) : 0.f) +
                        (a.b_hh[l] ? wround(a.b_hh[l][r], a.w_bf16) : 0.f)) * sc
                     : 0.f;
  }
  return W;
}

// PH: per-phase stamps (diagnostics build, PDRNN_TUNE sw_phase=1 with
// PDRNN_LSTM_STAMPS): s_memtime at the loop top (after the barrier), after the
// operand reads landed, after the products, after the quad reduce, after the
// cell and its stores; per-phase cycle sums over steps [16, T - 16) of waves 0
// (layer 0) and 2 (layer 1), written behind the loop stamps (row of 24).
template <int CELL = 0, bool PH = false, bool INFER = false>
PDRNN_DEVICE void fwd4_body(const PdrnnLstmSmallFwdArgs& a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const uint64_t sr_in = stamp_entry(a.stamps, tid);  // (the prologue's cost)
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = wv >> 1;
  const int ul = lane >> 2, q = lane & 3;
  const int u = 16 * (wv & 1) + ul;
  const int B = a.B, T = a.T, I = a.I;
  const int b = blockIdx.x;  // one sequence per workgroup
  const int bsrc = a.idx ? (int)a.idx[b] : b;
  float* hb = smem;                                  // [layer][parity][kHB]
  float* xs = smem + 2 * 2 * kHB;                    // [T][kXS]
  auto hbuf = [&](int ll, int p) { return hb + (ll * 2 + p) * kHB; };

  // (vector staging as in lstm_sw_fwd_kernel: xs zeroed first)
  const bool xvec = a.x_st == I && a.x_sb == (int64_t)T * I;
  for (int e = tid; e < 2 * 2 * kHB + (xvec ? T * kXS : 0); e += 256) hb[e] = 0.f;
  if (xvec) lds_barrier();
  const int bsrc1[1] = {bsrc}, bidx1[1] = {b}, vint1[1] = {1};
  if (!(xvec && stage_x_vec<1, INFER>(a, xs, bsrc1, bidx1, vint1, tid, 256))) {
    for (int e = tid; e < T * kXS; e += 256) {
      const int t = e / kXS, k = e - t * kXS;
      const float x = ldx(a.x, (int64_t)bsrc * a.x_sb + (int64_t)t * a.x_st + min(k, I - 1), a.x_bf16);
      const float v = k < I ? x : 0.f;
      xs[e] = v;
      if (!INFER && a.xg_out && k < a.xg_ld) a.xg_out[((int64_t)b * T + t) * a.xg_ld + k] = v;
    }
  }
  lds_barrier();  // (as in lstm_sw_fwd_kernel; the one-launch step's __syncthreads drains them before its BPTT)

  const __amdgpu_buffer_rsrc_t r_act = uniform_rsrc(a.act);
  const __amdgpu_buffer_rsrc_t r_h = uniform_rsrc(a.hseq);
  const uint32_t vo_a = (q * kH + u) * 4, vo_c = (4 * kH + u) * 4, vo_h = u * 4;
  const uint32_t lead = q == 0 ? 0u : kOOR;  // c / h stored by lane q = 0 of the unit
  const pdrnn_f2 gk = q == 2 ? pdrnn_f2{2.f, -1.f} : pdrnn_f2{1.f, 0.f};
  float cst = 0.f, hst = 0.f;

  uint64_t st0, sr0;
  stamp_loop_begin(a.stamps, tid, st0, sr0);

  // quad reduce-scatter of the four gate partials -> this lane's gate (q)
  auto gate_sum = [&](const float (&p)[4]) {
    const bool hi = q >= 2;
    const float k0 = hi ? p[2] : p[0], k1 = hi ? p[3] : p[1];
    const float s0 = hi ? p[0] : p[2], s1 = hi ? p[1] : p[3];
    const float m0 = k0 + dpp_swap2(s0), m1 = k1 + dpp_swap2(s1);
    const bool od = (q & 1) != 0;
    return (od ? m1 : m0) + dpp_swap1(od ? m0 : m1);
  };
  auto cell = [&](int t, bool act, float z) {
    float av, cn, hn;
    if constexpr (CELL == 0) {
      av = fmaf(sig2(z), gk.x, gk.y);  // i, f, tanh g or o of this lane
      const float ig = quad_bcast(av, 0), fg = quad_bcast(av, 1), gg = quad_bcast(av, 2), og = quad_bcast(av, 3);
      cn = fmaf(fg, cst, ig * gg);
      hn = og * tanh_c(cn);
    } else {  // GRU: r, z, or the 2 kA-scaled n_x / n_h of this lane; cn carries n
      const float sg = sig2(z);
      const float v = q < 2 ? sg : z;
      const float rg = quad_bcast(v, 0), zg = quad_bcast(v, 1), nx = quad_bcast(v, 2), nh = quad_bcast(v, 3);
      cn = fmaf(sig2(fmaf(rg, nh, nx)), 2.f, -1.f);
      hn = fmaf(zg, hst - cn, cn);
      av = q < 2 ? sg : z * (1.f / (2.f * kA));  // saved unscaled
    }
    cst = act ? cn : cst;
    hst = act ? hn : hst;
    if (q == 0) hbuf(l, t & 1)[u] = hst;
    if constexpr (!INFER) {
      const uint32_t rw = __builtin_amdgcn_readfirstlane((uint32_t)((l * B + b) * T + min(max(t, 0), T - 1)));
      const uint32_t m = act ? 0u : kOOR;
      bstore(av, r_act, vo_a | m, rw * (5 * kH * 4));
      bstore(cn, r_act, vo_c | m | lead, rw * (5 * kH * 4));
      bstore(hn, r_h, vo_h | m | lead, rw * (kH * 4));
    }
  };
  // phase stamps (PH only; compiled out otherwise)
  uint64_t ph_t[5] = {0, 0, 0, 0, 0}, ph_sum[5] = {0, 0, 0, 0, 0}, ph_prev = 0, ph_n = 0;
  auto ph_now = [&]() -> uint64_t {
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t v = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    return v;
  };
  auto ph_mark = [&](int k, float dep) {
    if constexpr (PH) {
      asm volatile("" ::"v"(dep));  // (the value this phase produced exists before the stamp)
      ph_t[k] = ph_now();
    }
  };
  auto ph_reads = [&]() {
    if constexpr (PH) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ph_t[1] = ph_now();
    }
  };
  auto ph_step = [&](int it) {  // after the barrier: close step it, open it + 1
    if constexpr (PH) {
      const uint64_t now = ph_now();
      if (it >= 16 && it < T - 16) {
        ph_sum[0] += ph_t[1] - ph_t[0];  // barrier -> operand reads landed
        ph_sum[1] += ph_t[2] - ph_t[1];  // products
        ph_sum[2] += ph_t[3] - ph_t[2];  // quad reduce (DPP)
        ph_sum[3] += ph_t[4] - ph_t[3];  // activations, cell, stores issued
        ph_sum[4] += now - ph_t[4];      // barrier wait
        ++ph_n;
      }
      (void)ph_prev;
      ph_t[0] = now;
    }
  };
  if constexpr (PH) ph_t[0] = ph_now();

  if (l == 0) {
    float bias[4];
    const Fwd4W<3> W = load_fwd4_w<3, CELL>(a, 0, u, q, bias);
    for (int it = 0; it <= T; ++it) {
      if (it < T) {
        const int t = it;
        const float* src = q == 0 ? xs + t * kXS : hbuf(0, (t - 1) & 1) + 12 * (q - 1);
        float4 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ld4(src + 4 * c);
        __builtin_amdgcn_sched_barrier(0);
        ph_reads();
        pdrnn_f2 acc[4] = {{bias[0], 0.f}, {bias[1], 0.f}, {bias[2], 0.f}, {bias[3], 0.f}};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = pfma(W.w[j][2 * c], lo2(v[c]), acc[j]);
            acc[j] = pfma(W.w[j][2 * c + 1], hi2(v[c]), acc[j]);
          }
        float p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = acc[j].x + acc[j].y;
        ph_mark(2, p[3]);
        const float z = gate_sum(p);
        ph_mark(3, z);
        cell(t, true, z);
        ph_mark(4, 0.f);
      }
      lds_barrier();
      ph_step(it);
    }
  } else {
    float bias[4];
    const Fwd4W<4> W = load_fwd4_w<4, CELL>(a, 1, u, q, bias);
    for (int it = 0; it <= T; ++it) {
      if (it > 0) {
        const int t = it - 1;
        const float* src = q < 2 ? hbuf(0, t & 1) + 16 * q : hbuf(1, (t - 1) & 1) + 16 * (q - 2);
        float4 v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = ld4(src + 4 * c);
        __builtin_amdgcn_sched_barrier(0);
        ph_reads();
        pdrnn_f2 acc[4] = {{bias[0], 0.f}, {bias[1], 0.f}, {bias[2], 0.f}, {bias[3], 0.f}};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = pfma(W.w[j][2 * c], lo2(v[c]), acc[j]);
            acc[j] = pfma(W.w[j][2 * c + 1], hi2(v[c]), acc[j]);
          }
        float p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = acc[j].x + acc[j].y;
        ph_mark(2, p[3]);
        const float z = gate_sum(p);
        ph_mark(3, z);
        cell(t, true, z);
        ph_mark(4, 0.f);
      }
      lds_barrier();
      ph_step(it);
    }
  }
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * (PH ? 24 : 8);
    stamp_loop_end(st, st0, sr0);
    st[4] = sr_in; st[6] = stamp_cu();  // (exit: after the head, below)
  }
  if constexpr (PH) {
    if ((wv == 0 || wv == 2) && lane == 0) {
      uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 24 + 8 + (wv == 2 ? 8 : 0);
#pragma unroll
      for (int k = 0; k < 5; ++k) st[k] = ph_sum[k];
      st[5] = ph_n;
    }
  }
  // ---- epilogue: h_n / c_n; the head reads the top layer's h_T from its slot
  if (q == 0) {
    if (a.hn) a.hn[((int64_t)l * B + b) * kH + u] = hst;
    if (a.cn) a.cn[((int64_t)l * B + b) * kH + u] = cst;
  }
  if (a.head_w) {
    // (the last barrier of the loop ordered every h_T write before this read:
    // layer 1's last step t = T-1 went to slot (T-1) & 1)
    if (wv == 2) {
      const int hu = lane >> 1;
      if constexpr (INFER) motion_head_infer(a, b, hbuf(1, (T - 1) & 1)[hu], hu, (lane & 1) != 0);
      else motion_head(a, b, hbuf(1, (T - 1) & 1)[hu], hu, (lane & 1) != 0);
    }
  }
  if (a.stamps && tid == 0) a.stamps[(uint64_t)blockIdx.x * (PH ? 24 : 8) + 5] = stamp_real();
}
template <int CELL, bool PH = false>
__global__ void __launch_bounds__(64 * kMaps[5].waves) lstm_sw_fwd4_kernel(PdrnnLstmSmallFwdArgs a) { fwd4_body<CELL, PH>(a); }
template <int CELL>
__global__ void __launch_bounds__(64 * kMaps[5].waves) lstm_sw_fwd4_infer_kernel(PdrnnLstmSmallFwdArgs a) {
  fwd4_body<CELL, false, true>(a);
}

// ---------------------------------------------------------------------------
// Forward, layer 1's input projection hoisted onto the matrix cores (map 8,
// two-layer stacks in the throughput regime, T % 16 == 0).  Map 6's waves
// (wave l = layer l of one sequence, <= 168 VGPRs: three waves per SIMD), and
// BIT FOR BIT map 6's results: every gate pre-activation is the same sum of
// the same fp32 operations, only computed elsewhere.
//  * Map 6 forms a gate of layer 1 as (in.x + in.y) + (rec.x + rec.y): `in`
//    the v_pk_fma_f32 chain over the input h^0_t (.x the even columns in
//    ascending order, .y the odd ones; seeded with the bias for i, g) and
//    `rec` the same over the own h_{t-1} (seeded with the bias for f, o).
//  * W_ih^1 h^0_t does not depend on layer 1's recurrence, so the layer-1
//    wave forms `in` for 16 steps at once with v_mfma_f32_16x16x4_f32 (M = 16
//    time steps, N = 16 gate columns per tile, 8 tiles).  An fp32 MFMA is a
//    k-ordered fma chain on its C operand, so one chain of 4 K steps over the
//    even columns (k = 8 j + 2 kk; C = the bias or 0) reproduces in.x and one
//    over the odd columns in.y: 64 MFMAs per chunk, the W_ih fragments
//    resident in 64 VGPRs.  P[16][128] = in.x + in.y goes to an LDS tile.
//  * The recurrent chains are split between the two lanes of a unit by gate,
//    not by K half: lane s runs the full 32-column chains of its own two
//    gates (s = 0: i, g from zero; s = 1: f, o from the bias) -- 8 operand
//    reads, all lanes at one address, and 32 v_pk_fma_f32 per step instead
//    of 64, no K-split DPP adds -- and adds its two P values (one ds_read_b64:
//    P column 4u + 2s + j is gate row (s + 2j) H + u; row stride kPS = 132
//    keeps the C tile's rows 4g + r on disjoint banks).
//  * Layer 0 runs map 6's step unchanged (its x columns share a chain with
//    h[0, 12), so they cannot leave it without changing the sum) and also
//    writes h^0_t into a ring of 2 chunks x 16 rows; the layer-1 wave runs one
//    chunk behind and reads a chunk of h^0 as its A fragments: one workgroup
//    barrier per chunk (T / 16 + 1 slots), none per step.
// ---------------------------------------------------------------------------
constexpr int kCT = 16;          // steps per chunk (MFMA M)
constexpr int kPS = 4 * kH + 4;  // P row stride, floats
constexpr int kF8Res = 4;        // inference: W_ih^1 column tiles (of 8) resident in VGPRs
// LDS floats of a workgroup: P[kCT][kPS] | h^0 ring [2][kCT][kHB] | h slots
// [2 layers][2 parities][kHB] | layer 1's MFMA C seeds [4H] | x rows [T][kXS]
constexpr int kF8Ring = kCT * kPS, kF8Slot = kF8Ring + 2 * kCT * kHB, kF8Bias = kF8Slot + 2 * 2 * kHB;
constexpr int kF8X = kF8Bias + 4 * kH;

template <int CELL>
PDRNN_DEVICE float gate_scale(int q) { return kA * ((CELL == 0 ? q == 2 : q >= 2) ? 2.f : 1.f); }
// gate row of P column p (see above)
PDRNN_DEVICE int p_row(int p) { return (((p >> 1) & 1) + 2 * (p & 1)) * kH + (p >> 2); }

// One MFMA B fragment element of W_ih^1: gate row r (scaled by sc), chain e
// (even / odd columns), K step j -> column 8 j + 2 kk + e.  The one place the
// resident tiles and the inference build's per-chunk tiles get their values.
PDRNN_DEVICE float bw_frag(const PdrnnLstmSmallFwdArgs& a, int r, float sc, int kk, int e, int j) {
  return wround(a.w_ih[1][(int64_t)r * kH + 8 * j + 2 * kk + e], a.w_bf16) * sc;
}

static_assert(kMaps[8].t_mult == kCT && kMaps[8].waves == 2, "map 8: whole chunks, a wave per layer");
template <int CELL, bool INFER = false>
__global__ void __launch_bounds__(64 * kMaps[8].waves) __attribute__((amdgpu_waves_per_eu(kMaps[8].eu_cap)))
lstm_sw_fwd8_kernel(PdrnnLstmSmallFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const uint64_t sr_in = stamp_entry(a.stamps, tid);  // (the prologue's cost)
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // = layer
  const int u = lane >> 1, s = lane & 1;
  const bool odd = s != 0;
  const int mi = lane & 15, kk = lane >> 4;  // MFMA fragment row / K index
  const int B = a.B, T = a.T, I = a.I;
  const int b = blockIdx.x;  // one sequence per workgroup
  const int bsrc = a.idx ? (int)a.idx[b] : b;
  const int nch = T / kCT;
  float* P = smem;
  float* ring = smem + kF8Ring;
  float* hs = smem + kF8Slot + wv * 2 * kHB;
  float* cseed = smem + kF8Bias;
  float* xs = smem + kF8X;

  // ---- prologue: h_{-1} = 0 (ring, slots and their pad chunks), layer 1's C
  // seeds (the bias of i, g; 0 for f, o) in P's column order, x staged as in
  // lstm_sw_fwd_kernel (one sequence: element loads)
  for (int e = tid; e < kF8Bias - kF8Ring; e += 128) ring[e] = 0.f;
  {
    const int r = p_row(tid);
    const float bsum = ((a.b_ih[1] ? wround(a.b_ih[1][r], a.w_bf16) : 0.f) +
                        (a.b_hh[1] ? wround(a.b_hh[1][r], a.w_bf16) : 0.f)) * gate_scale<CELL>(r / kH);
    cseed[tid] = (tid >> 1) & 1 ? 0.f : bsum;
  }
  {
    const int tot = T * kXS, xg_ld = a.xg_ld;
    for (int e0 = tid; e0 < tot; e0 += 4 * 128) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = min(e0 + r * 128, tot - 1);
        const int t = e / kXS, k = e - t * kXS;
        const float x = ldx(a.x, (int64_t)bsrc * a.x_sb + (int64_t)t * a.x_st + min(k, I - 1), a.x_bf16);
        v[r] = k < I ? x : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = e0 + r * 128;
        if (e < tot) {
          const int t = e / kXS, k = e - t * kXS;
          xs[e] = v[r];
          if (!INFER && a.xg_out && k < xg_ld) a.xg_out[((int64_t)b * T + t) * xg_ld + k] = v[r];
        }
      }
    }
  }
  lds_barrier();

  const __amdgpu_buffer_rsrc_t r_act = uniform_rsrc(a.act);
  const __amdgpu_buffer_rsrc_t r_h = uniform_rsrc(a.hseq);
  const uint32_t vo_a0 = (s * kH + u) * 4, vo_a1 = ((2 + s) * kH + u) * 4, vo_c = (4 * kH + u) * 4, vo_h = u * 4;
  const pdrnn_f2 gk = odd ? pdrnn_f2{1.f, 0.f} : pdrnn_f2{2.f, -1.f};

  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }

  float cst = 0.f, hst = 0.f;
  // h_t to the own parity slot, the saved rows to act / hseq
  auto commit = [&](int t, const Cell& r) {
    cst = r.c;
    hst = r.h;
    hs[(t & 1) * kHB + u] = r.h;
    if constexpr (!INFER) {
      const uint32_t rw = __builtin_amdgcn_readfirstlane((uint32_t)((wv * B + b) * T + t));
      store_cell(r, r_act, r_h, vo_a0, vo_a1, vo_c, vo_h, 0u, rw);
    }
  };

  if (wv == 0) {
    const FwdW<6> W0 = load_fwd_w<6, CELL>(a, 0, u, s);
    for (int c = 0; c <= nch; ++c) {
      if (c < nch) {
#pragma unroll 2
        for (int i = 0; i < kCT; ++i) {
          const int t = c * kCT + i;
          const float* hp = hs + ((t - 1) & 1) * kHB;
          const float* pa = odd ? hp + 12 : xs + t * kXS;
          const float* pb = odd ? hp + 24 : hp;
          float4 v[6];
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) v[cc] = ld4(pa + 4 * cc);
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) v[3 + cc] = ld4(pb + 4 * cc);
          float p[4];
          fwd_dot<6>(W0, v, p);
          const Cell r = fwd_cell_any<CELL>(p, gk, cst, hst, odd);
          commit(t, r);
          ring[((c & 1) * kCT + i) * kHB + u] = r.h;
        }
      }
      lds_barrier();
    }
  } else {
    // the own two gates' rows of W_hh over all 32 columns, k pairs; bias seeds (odd lanes)
    pdrnn_f2 wr[2][16];
    float seed[2];
    // B fragments of W_ih^1: column tile nt, chain e (even / odd columns), K step j -> column 8 j + 2 kk + e
    // (the inference build keeps kF8Res tiles and fetches the others from
    // memory in every chunk, the same values (bw_frag): with all eight
    // resident it spills, as the training build does)
    constexpr int NR = INFER ? kF8Res : 8;
    float bw[NR][2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int q = s + 2 * jj, r = q * kH + u;
      const float sc = gate_scale<CELL>(q);
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const float* w = a.w_hh[1] + (int64_t)r * kH + 4 * cc;
        wr[jj][2 * cc] = pdrnn_f2{wround(w[0], a.w_bf16) * sc, wround(w[1], a.w_bf16) * sc};
        wr[jj][2 * cc + 1] = pdrnn_f2{wround(w[2], a.w_bf16) * sc, wround(w[3], a.w_bf16) * sc};
      }
      const float bsum = ((a.b_ih[1] ? wround(a.b_ih[1][r], a.w_bf16) : 0.f) +
                          (a.b_hh[1] ? wround(a.b_hh[1][r], a.w_bf16) : 0.f)) * sc;
      seed[jj] = odd ? bsum : 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < NR; ++nt) {
      const int r = p_row(16 * nt + mi);
      const float sc = gate_scale<CELL>(r / kH);
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) bw[nt][e][j] = bw_frag(a, r, sc, kk, e, j);
    }
    for (int c = 0; c <= nch; ++c) {
      if (c > 0) {
        // ---- chunk c - 1: P = in.x + in.y for its 16 steps
        {
          const float* hr = ring + (((c - 1) & 1) * kCT + mi) * kHB + 2 * kk;
          pdrnn_f2 av[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) av[j] = *reinterpret_cast<const pdrnn_f2*>(hr + 8 * j);
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) {
            const float b0 = cseed[16 * nt + mi];
            f32x4 ce = {b0, b0, b0, b0}, co = {0.f, 0.f, 0.f, 0.f};
            float bf[2][4];
            if (nt >= NR) {  // (inference: this tile is not resident)
              const int r = p_row(16 * nt + mi);
              const float sc = gate_scale<CELL>(r / kH);
#pragma unroll
              for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[e][j] = bw_frag(a, r, sc, kk, e, j);
            }
            const float (&bt)[2][4] = nt < NR ? bw[nt] : bf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ce = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bt[0][j], ce, 0, 0, 0);
              co = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bt[1][j], co, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(4 * kk + r) * kPS + 16 * nt + mi] = ce[r] + co[r];
          }
        }
#pragma unroll 2
        for (int i = 0; i < kCT; ++i) {
          const int t = (c - 1) * kCT + i;
          const float* hp = hs + ((t - 1) & 1) * kHB;
          float4 v[8];
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) v[cc] = ld4(hp + 4 * cc);
          const pdrnn_f2 pin = *reinterpret_cast<const pdrnn_f2*>(P + i * kPS + 2 * lane);
          pdrnn_f2 acc[2] = {{seed[0], 0.f}, {seed[1], 0.f}};
#pragma unroll
          for (int cc = 0; cc < 8; ++cc)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              acc[jj] = pfma(wr[jj][2 * cc], lo2(v[cc]), acc[jj]);
              acc[jj] = pfma(wr[jj][2 * cc + 1], hi2(v[cc]), acc[jj]);
            }
          const float z0 = (acc[0].x + acc[0].y) + pin.x, z1 = (acc[1].x + acc[1].y) + pin.y;
          Cell r;
          if constexpr (CELL == 0) r = fwd_cell_z(z0, z1, gk, cst, odd);
          else r = fwd_cell_gru_z(z0, z1, hst, odd);
          commit(t, r);
        }
      }
      lds_barrier();
    }
  }
  if (a.stamps && tid == 0) stamp_loop_end(a.stamps + (uint64_t)blockIdx.x * 8, st0, sr0);

  // ---- epilogue: h_n / c_n, then the fused head on the top layer's h_T ----
  if (!odd && a.hn) a.hn[((int64_t)wv * B + b) * kH + u] = hst;
  if (!odd && a.cn) a.cn[((int64_t)wv * B + b) * kH + u] = cst;
  if (a.head_w && wv == 1) {
    if constexpr (INFER) motion_head_infer(a, b, hst, u, odd);
    else motion_head(a, b, hst, u, odd);
  }
  if (a.stamps && tid == 0) stamp_exit(a.stamps + (uint64_t)blockIdx.x * 8, sr_in);
}

// ---------------------------------------------------------------------------
// Backward (lean contract: zero initial state, dL/dh_T of the top layer only,
// weight gradients deferred to pdrnn_lstm_small_dw)
// ---------------------------------------------------------------------------
struct Ops {
  float i, f, g, o, c, cp;
};

// column u of W_hh (and W_ih) over rows [64 s, 64 s + 64), row pairs
struct BwdCol {
  pdrnn_f2 w[32];
};
PDRNN_DEVICE BwdCol load_bwd_col(const float* w, int ld, int col, bool live, int u, int s, int wbf) {
  BwdCol W;
  (void)u;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int r = 64 * s + 2 * j;
    const float x0 = w[(int64_t)r * ld + col], x1 = w[(int64_t)(r + 1) * ld + col];
    W.w[j] = live ? pdrnn_f2{wround(x0, wbf), wround(x1, wbf)} : pdrnn_f2{0.f, 0.f};
  }
  return W;
}

// gate gradients of this lane (d0: i | g, d1: f | o) from the saved
// activations; dc carries dL/dc_t into step t - 1
PDRNN_DEVICE void row_phase(const Ops& o, float dht, float& dc, bool odd, bool has_prev, float& d0, float& d1) {
  const float cp = has_prev ? o.cp : 0.f;
  const float tc = tanh_c(o.c);
  const float dcp = fmaf(dht * o.o, fmaf(-tc, tc, 1.f), dc);
  const float X = odd ? o.i : o.g;
  const float Y = odd ? fmaf(-o.g, o.g, 1.f) : fmaf(-o.i, o.i, o.i);
  d0 = dcp * X * Y;
  const float P = odd ? dht : dcp;
  const float Q = odd ? tc : cp;
  const float R = odd ? fmaf(-o.o, o.o, o.o) : fmaf(-o.f, o.f, o.f);
  d1 = P * Q * R;
  dc = dcp * o.f;
}

// GRU (saved r, z, n_h, n; cp = h_{t-1}): the gate-gradient vector is
// [dr r(1-r) | dz z(1-z) | dpn | dpn r] with dpn = dh (1-z) (1-n^2) (s = 0:
// the r, z blocks; s = 1: n_x, n_h), so the column phase W^T dz over the
// packed stack is the LSTM's; dc carries the direct path dh_t z_t into t - 1.
PDRNN_DEVICE void row_phase_gru(const Ops& o, float dht, float& dc, bool odd, bool has_prev, float& d0, float& d1) {
  const float hp = has_prev ? o.cp : 0.f;
  const float dh = dht + dc;
  const float n = o.c, r = o.i, z = o.f;
  const float dpn = dh * (1.f - z) * fmaf(-n, n, 1.f);
  d0 = odd ? dpn : dpn * o.o * fmaf(-r, r, r);
  d1 = odd ? dpn * r : dh * (hp - n) * fmaf(-z, z, z);
  dc = dh * z;
}

PDRNN_DEVICE float col_dot(const BwdCol& W, const float4 (&g)[16]) {
  pdrnn_f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    a0 = pfma(W.w[2 * c], lo2(g[c]), a0);
    a1 = pfma(W.w[2 * c + 1], hi2(g[c]), a1);
  }
  const pdrnn_f2 s = a0 + a1;
  return pair_sum(s.x + s.y);
}

// (no occupancy target: at 168 VGPRs the split backward spills, and it only
// runs at B <= one wave per SIMD)
template <int NL, int MODE, int CELL = 0>
PDRNN_DEVICE void bwd_body(const PdrnnLstmSmallBwdArgs& a) {
  // (A four-wave BPTT map -- two waves per layer, unit x row quarter -- was
  // correct but slower: 92.7 vs 55.3 us at B = 180, the column phase waiting
  // behind the barrier for the other wave's dz; profiles/r5/sw/bwd5_probe.log;
  // removed in round 6.)
  constexpr int NB = kMaps[MODE].nb;
  constexpr bool SPLIT = kMaps[MODE].split;
  constexpr bool DWACC = kMaps[MODE].rdw;
  constexpr int ZR = kMaps[MODE].zr;
  static_assert(map_serves(MODE, true, NL), "the wave map table lists no such backward");
  static_assert(SPLIT == (NL == 2), "one layer per wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const uint64_t sr_in = stamp_entry(a.stamps, tid);  // (the prologue's cost)
  const int lane = tid & 63;
  const int wv = SPLIT ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
  const int u = lane >> 1;
  const int s = lane & 1;
  const bool odd = s != 0;
  const int B = a.B, T = a.T;
  const int bbase = blockIdx.x * NB;
  float* dzb = smem;                          // [NB][NL][ZR][kDZ]
  float* dxb = smem + NB * NL * ZR * kDZ;     // [NB][2][32] (layer 1's input gradient -> layer 0)
  auto dzbuf = [&](int n, int l, int t) { return dzb + ((n * NL + l) * ZR + (t & (ZR - 1))) * kDZ; };

  int bidx[NB];
  bool valid[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    valid[n] = b < B;
    bidx[n] = valid[n] ? b : B - 1;
  }
  uint32_t vmask[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) vmask[n] = valid[n] ? 0u : kOOR;

  // the dW kernel streams whole stages: the PDRNN_DW_PAD_ROWS padding rows
  // behind the last layer's gate gradients must hold finite values
  if (!DWACC && blockIdx.x == 0) {
    float* pad = a.dg_out + (int64_t)NL * B * T * a.dg_st;
    for (int e = tid; e < PDRNN_DW_PAD_ROWS * a.dg_st; e += blockDim.x) pad[e] = 0.f;
  }

  const __amdgpu_buffer_rsrc_t r_act = uniform_rsrc(a.act);
  const __amdgpu_buffer_rsrc_t r_dg = uniform_rsrc(a.dg_out);
  const __amdgpu_buffer_rsrc_t r_hs = uniform_rsrc(a.hseq);  // GRU: h_{t-1}
  const uint32_t st_act = 5 * kH * 4, st_dg = (uint32_t)a.dg_st * 4;
  const uint32_t vo_i = u * 4, vo_f = (kH + u) * 4, vo_g = (2 * kH + u) * 4, vo_o = (3 * kH + u) * 4;
  const uint32_t vo_c = (4 * kH + u) * 4;
  const uint32_t vo_d0 = (2 * s * kH + u) * 4, vo_d1 = ((2 * s + 1) * kH + u) * 4;
  const int slot0 = dz_slot(2 * s * kH + u), slot1 = dz_slot((2 * s + 1) * kH + u);
  const int colbase = dz_slot(64 * s);

  auto rowidx = [&](int l, int n, int t) -> uint32_t {
    return __builtin_amdgcn_readfirstlane((uint32_t)((l * B + pick<NB>(bidx, n)) * T + t));
  };
  // branch-free operand loads of layer l, step t (clamped; masked at use)
  auto load_ops = [&](int l, int n, int t) {
    const int tc = min(max(t, 0), T - 1);
    const uint32_t ra = rowidx(l, n, tc) * st_act;
    const uint32_t rp = __builtin_amdgcn_readfirstlane(tc > 0 ? ra - st_act : ra);
    Ops o;
    o.i = bload(r_act, vo_i, ra);
    o.f = bload(r_act, vo_f, ra);
    o.o = bload(r_act, vo_o, ra);
    o.c = bload(r_act, vo_c, ra);
    if constexpr (CELL == 0) {
      o.g = bload(r_act, vo_g, ra);
      o.cp = bload(r_act, vo_c, rp);
    } else {  // GRU: n_x unused; h_{t-1} of the unit from the saved h sequence
      o.g = 0.f;
      const uint32_t rh = rowidx(l, n, tc) * (kH * 4);
      o.cp = bload(r_hs, u * 4, __builtin_amdgcn_readfirstlane(tc > 0 ? rh - kH * 4 : rh));
    }
    return o;
  };

  // per (layer, sequence) state
  float dhrec[NL][NB], dc[NL][NB];
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int n = 0; n < NB; ++n) { dhrec[l][n] = 0.f; dc[l][n] = 0.f; }
  float dhtop[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) dhtop[n] = a.dhn[(int64_t)bidx[n] * kH + u];
  if (SPLIT) {
    for (int e = tid; e < NB * 2 * 32; e += blockDim.x) dxb[e] = 0.f;
  }

  uint64_t st0, sr0;
  stamp_loop_begin(a.stamps, tid, st0, sr0);

  // Iteration `it`: the top layer at t = T-1-it, layer 0 (of a 2-layer stack)
  // at t = T-it (lag 1: its dh input is layer 1's input gradient of step t).
  // The body is branch-free (inactive steps compute on clamped operands and
  // their stores are dropped): a branch join would make the waitcnt pass wait
  // for the prefetches of the next two iterations.
  const int iters = T + NL - 1;

  // DWACC: the weight gradients on the matrix cores of two extra waves of the
  // workgroup (wave 2: layer 0, wave 3: layer 1), so the BPTT waves never
  // wait on a busy matrix core.  dW_hh / dW_ih of a layer are 16x16 C tiles
  // of v_mfma_f32_16x16x4_f32 (M = 128 gate rows in 8 tiles, N = 32 columns
  // in 2, K = 4 consecutive time steps).  A K step's A operands (the layer's
  // dz from the 8-slot LDS ring) are captured in the iteration after its
  // last step is written; its 32 MFMAs issue a quarter (two m-tiles) per
  // iteration.  The B operands (h_{t-1} and the layer input, no recurrence
  // dependency) are loaded one group ahead.  The BPTT waves keep their two
  // gate rows' bias sums in registers.
  float dbs[2] = {0.f, 0.f};
  const int xld = a.xg_ld;
  // B operands of the K step over times t .. t+3 (lane: time t + (lane >> 4),
  // column lane & 15 of each 16-column tile)
  auto dw_loadb = [&](int l, int t, float (&bv)[4]) {
    const int tk = t + (lane >> 4), c = lane & 15;
    const int64_t b = bidx[0];
    const float* hown = a.hseq + ((int64_t)(l * B + b) * T + max(tk - 1, 0)) * kH;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) bv[nt] = tk > 0 ? hown[16 * nt + c] : 0.f;
    if (l > 0) {
      const float* hin = a.hseq + ((int64_t)((l - 1) * B + b) * T + tk) * kH;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bv[2 + nt] = hin[16 * nt + c];
    } else {
      bv[2] = c < xld ? a.xg_out[((int64_t)b * T + tk) * xld + c] : 0.f;
      bv[3] = 0.f;
    }
  };
  // the dW wave of layer L (compile time); its iteration `it` is the BPTT
  // waves' iteration (one barrier each)
  auto dw_wave = [&](auto lc) {
    constexpr int L = decltype(lc)::value;
    constexpr int NI = L > 0 ? 2 : 1;  // input column tiles (layer 0: I <= 16)
    f32x4 ahh[8][2], aih[8][NI];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) ahh[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NI; ++nt) aih[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float pav[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, pb[4] = {0.f, 0.f, 0.f, 0.f}, bnext[4];
    dw_loadb(L, T - 4, bnext);
    // (branch-free: before the first K step is complete the A operands are
    // zeros; a branch would put the accumulators through copies at its joins)
    auto capture = [&](int g, bool live) {
      const float* zb = dzbuf(0, L, g + (lane >> 4));
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) {
        const float z = zb[dz_slot(16 * mt + (lane & 15))];
        pav[mt] = live ? z : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) pb[k] = bnext[k];
      dw_loadb(L, max(g - 4, 0), bnext);
    };
    auto quarter = [&](auto qc) {
      constexpr int q = decltype(qc)::value;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        constexpr int m0 = 2 * q;
        const int mt = m0 + j;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          ahh[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pav[mt], pb[nt], ahh[mt][nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < NI; ++nt)
          aih[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pav[mt], pb[2 + nt], aih[mt][nt], 0, 0, 0);
      }
    };
    using Q0 = std::integral_constant<int, 0>;
    using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>;
    using Q3 = std::integral_constant<int, 3>;
    // T % 4 == 0.  Layer 1's group g (times g .. g+3) is complete after
    // iteration T-1-g, layer 0's after T-g: capture at it = T-g (layer 1) or
    // T-g+1 (layer 0), i.e. at it % 4 == LAG, then one quarter per iteration.
    constexpr int LAG = L == 1 ? 0 : 1;
    auto pos = [&](int it, auto pc) {
      constexpr int p = decltype(pc)::value;
      constexpr int q = (p - LAG + 4) & 3;
      if constexpr (q == 0) capture(T - it + LAG, it >= 4 + LAG);
      quarter(std::integral_constant<int, q>{});
      __builtin_amdgcn_sched_barrier(0);  // (a quarter per iteration, not clumped)
      lds_barrier();
    };
    __syncthreads();
    const int iters = T + 1;
    int it = 0;
    for (; it + 3 < iters; it += 4) {
      pos(it, Q0{});
      pos(it + 1, Q1{});
      pos(it + 2, Q2{});
      pos(it + 3, Q3{});
    }
    pos(it, Q0{});  // it = T
    // (after the last barrier every dz is in the ring)
    if constexpr (L == 1) {
      quarter(Q1{}); quarter(Q2{}); quarter(Q3{});
    } else {
      capture(0, true);
      quarter(Q0{}); quarter(Q1{}); quarter(Q2{}); quarter(Q3{});
    }
    // this workgroup's slab row (an empty slot recomputed sequence B - 1: its
    // row must still be written, as zeros, since the reduction sums every row)
    const __amdgpu_buffer_rsrc_t r_slab = uniform_rsrc(a.slab);
    const uint32_t srow = (uint32_t)blockIdx.x * (uint32_t)a.P;  // (element offsets; the slab is far below 2 GiB)
    auto sst = [&](int64_t e, float v) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r_slab, (uint32_t)(srow + e) * 4u, 0, 0);
    };
    const int Iin = L == 0 ? a.I : kH;
    const int c = lane & 15, r4 = 4 * (lane >> 4);
    const float keep = valid[0] ? 1.f : 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mt + r4 + r;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) sst(a.off_whh[L] + (int64_t)row * kH + 16 * nt + c, keep * ahh[mt][nt][r]);
#pragma unroll
        for (int nt = 0; nt < NI; ++nt) {
          const int col = 16 * nt + c;
          if (col < Iin) sst(a.off_wih[L] + (int64_t)row * Iin + col, keep * aih[mt][nt][r]);
        }
      }
  };
  auto db_store = [&](int l) {
    const __amdgpu_buffer_rsrc_t r_slab = uniform_rsrc(a.slab);
    const uint32_t srow = (uint32_t)blockIdx.x * (uint32_t)a.P;
    auto sst = [&](int64_t e, float v) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r_slab, (uint32_t)(srow + e) * 4u, 0, 0);
    };
    const float d0 = valid[0] ? dbs[0] : 0.f, d1 = valid[0] ? dbs[1] : 0.f;
    const int r0 = 2 * s * kH + u, r1 = r0 + kH;
    if (a.off_bih[l] >= 0) { sst(a.off_bih[l] + r0, d0); sst(a.off_bih[l] + r1, d1); }
    if (a.off_bhh[l] >= 0) { sst(a.off_bhh[l] + r0, d0); sst(a.off_bhh[l] + r1, d1); }
  };

  // layer-generic pieces
  // (carrying c_{t-1} into the next step instead of re-loading it as that
  // step's c_t measured slower: BPTT 141 vs 128 us at B = 1440)
  auto rows = [&](int l, int n, int t, const Ops& o, float dh_in, bool act) {
    float d0, d1, dcn = dc[l][n];
    if constexpr (CELL == 0) row_phase(o, dhrec[l][n] + dh_in, dcn, odd, t > 0, d0, d1);
    else row_phase_gru(o, dhrec[l][n] + dh_in, dcn, odd, t > 0, d0, d1);
    dc[l][n] = act ? dcn : dc[l][n];
    float* zb = dzbuf(n, l, t);
    zb[slot0] = d0;
    zb[slot1] = d1;
    if constexpr (DWACC) {
      dbs[0] += act ? d0 : 0.f;
      dbs[1] += act ? d1 : 0.f;
    } else {
      const uint32_t so = rowidx(l, n, min(max(t, 0), T - 1)) * st_dg;
      const uint32_t m = act ? vmask[n] : kOOR;
      bstore(d0, r_dg, vo_d0 | m, so);
      bstore(d1, r_dg, vo_d1 | m, so);
    }
  };
  auto read_dz = [&](int l, int n, int t, float4 (&g)[16]) {
    const float* zb = dzbuf(n, l, t) + colbase;
#pragma unroll
    for (int c = 0; c < 16; ++c) g[c] = ld4(zb + 4 * c);
  };

  if constexpr (NL == 1) {
    const BwdCol Whh = load_bwd_col(a.w_hh[0], kH, u, true, u, s, a.w_bf16);
    Ops opA[NB], opB[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) opA[n] = load_ops(0, n, T - 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NB; ++n) opB[n] = load_ops(0, n, T - 2);
    __builtin_amdgcn_sched_barrier(0);
    auto body = [&](int it, Ops (&op)[NB]) {
      const int t = T - 1 - it;
      const bool act = t >= 0;
#pragma unroll
      for (int n = 0; n < NB; ++n) rows(0, n, t, op[n], it == 0 ? dhtop[n] : 0.f, act);
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float4 g[16];
        read_dz(0, n, t, g);
        const float v = col_dot(Whh, g);
        dhrec[0][n] = act ? v : dhrec[0][n];
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) op[n] = load_ops(0, n, t - 2);
    };
    int it = 0;
    for (; it + 1 < iters; it += 2) {
      body(it, opA);
      body(it + 1, opB);
    }
    if (it < iters) body(it, opA);
  } else {
    // wave 1 = layer 1 (t = T-1-it), wave 0 = layer 0 (t = T-it),
    // one barrier per iteration; layer 1's input gradient of step t reaches
    // layer 0 through dxb[n][t & 1]
    if (wv == 1) {
      const BwdCol Whh1 = load_bwd_col(a.w_hh[1], kH, u, true, u, s, a.w_bf16);
      const BwdCol Wih1 = load_bwd_col(a.w_ih[1], kH, u, true, u, s, a.w_bf16);
      Ops opA[NB], opB[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) opA[n] = load_ops(1, n, T - 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n = 0; n < NB; ++n) opB[n] = load_ops(1, n, T - 2);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      auto body = [&](int it, Ops (&op)[NB]) {
        const int t = T - 1 - it;
        const bool act = t >= 0;
#pragma unroll
        for (int n = 0; n < NB; ++n) rows(1, n, t, op[n], it == 0 ? dhtop[n] : 0.f, act);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          float4 g[16];
          read_dz(1, n, t, g);
          const float vh = col_dot(Whh1, g);
          const float vx = col_dot(Wih1, g);
          dhrec[1][n] = act ? vh : dhrec[1][n];
          if (!odd) dxb[(n * 2 + (t & 1)) * 32 + u] = act ? vx : 0.f;
          // one sequence's 64-float dz slice in registers at a time (two
          // would push the wave past 256 VGPRs: one wave per SIMD)
          if (NB > 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) op[n] = load_ops(1, n, t - 2);
        lds_barrier();
      };
      int it = 0;
      for (; it + 1 < iters; it += 2) {
        body(it, opA);
        body(it + 1, opB);
      }
      if (it < iters) body(it, opA);
      if constexpr (DWACC) db_store(1);
    } else if (wv == 0) {
      const BwdCol Whh0 = load_bwd_col(a.w_hh[0], kH, u, true, u, s, a.w_bf16);
      Ops opA[NB], opB[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) opA[n] = load_ops(0, n, T);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n = 0; n < NB; ++n) opB[n] = load_ops(0, n, T - 1);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      auto body = [&](int it, Ops (&op)[NB]) {
        const int t = T - it;
        const bool act = t < T;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float dxin = dxb[(n * 2 + (t & 1)) * 32 + u];  // layer 1's step-t input gradient
          rows(0, n, t, op[n], act ? dxin : 0.f, act);
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          float4 g[16];
          read_dz(0, n, t, g);
          const float vh = col_dot(Whh0, g);
          dhrec[0][n] = act ? vh : dhrec[0][n];
          if (NB > 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) op[n] = load_ops(0, n, t - 2);
        lds_barrier();
      };
      int it = 0;
      for (; it + 1 < iters; it += 2) {
        body(it, opA);
        body(it + 1, opB);
      }
      if (it < iters) body(it, opA);
      if constexpr (DWACC) db_store(0);
    } else if constexpr (DWACC) {
      if (wv == 2) dw_wave(std::integral_constant<int, 0>{});
      else dw_wave(std::integral_constant<int, 1>{});
    }
  }
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    const uint64_t sr1 = stamp_real();
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = sr1;
    st[4] = sr_in; st[5] = sr1; st[6] = stamp_cu();
  }
}
template <int NL, int MODE, int CELL = 0>
__global__ void __launch_bounds__(64 * kMaps[MODE].waves)
lstm_sw_bwd_kernel(PdrnnLstmSmallBwdArgs a) {
  bwd_body<NL, MODE, CELL>(a);
}

// ---------------------------------------------------------------------------
// One-launch step (latency regime: B <= two workgroups per CU, two layers).
// Workgroup b runs sequence b's four-wave forward (map 5) with the head/CE,
// then -- no grid-wide dependency between the passes -- the same sequence's
// BPTT with its two matrix-core dW waves (map 4): each sequence's backward
// starts the moment its own forward ends instead of after the slowest
// workgroup of a forward launch.  Every operand the backward reads (act,
// hseq, the staged x rows, dh_T) was written by the same workgroup: a
// __syncthreads() (which drains vmcnt on gfx950) orders them.  The slab
// reduction stays a launch of its own: inside this one (device-coherent slab
// stores, an arrival counter, every workgroup summing a column slice) it cost
// 15 us against 7 for the separate launch, and a release fence instead of
// the coherent stores 35 (profiles/r6/one_launch_step.md).
// ---------------------------------------------------------------------------
template <int CELL>
__global__ void __launch_bounds__(64 * kMaps[4].waves) lstm_sw_step_kernel(PdrnnLstmSmallFwdArgs f, PdrnnLstmSmallBwdArgs bk) {
  fwd4_body<CELL>(f);
  __syncthreads();  // the forward's outputs (act, hseq, x rows, dh_T) before the backward reads them
  bwd_body<2, 4, CELL>(bk);
}
static_assert(kMaps[5].waves == kMaps[4].waves, "the one-launch step runs both maps in one workgroup");

// ---- host side -------------------------------------------------------------
int sw_cus() {
  static thread_local int c_dev = -1, c_val = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != c_dev) {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    c_dev = dev;
    c_val = cus > 0 ? cus : 1;
  }
  return c_val;
}

// Dynamic LDS of a launch.  Forward: the h parity slots and the staged x rows
// of the workgroup's sequences (map 8: its P tile, ring, slots and seeds).
// Backward: the dz rings and the input-gradient parity slots.
size_t fwd_lds(int map, int NL, int T) {
  if (map == 8) return sizeof(float) * ((size_t)kF8X + (size_t)T * kXS);
  const size_t nb = kMaps[map].nb;
  return sizeof(float) * (nb * NL * 2 * kHB + nb * T * kXS);
}
size_t bwd_lds(int map, int NL) {
  const size_t nb = kMaps[map].nb;
  return sizeof(float) * (nb * NL * kMaps[map].zr * kDZ + nb * 2 * 32);
}
size_t step_lds(int T) { return std::max(fwd_lds(5, 2, T), bwd_lds(4, 2)); }

// The sequence lengths a map runs: whole K steps / chunks, and for map 8
// (14,144 bytes of LDS plus 48 T of x rows) six workgroups -- three waves per
// SIMD -- in a CU's 160 KiB, 26,624 bytes each in 2 KiB granules: T <= 256.
bool map_serves_T(int map, int NL, int T) {
  if (T <= 0 || T % kMaps[map].t_mult) return false;
  return map != 8 || 6 * ((fwd_lds(8, NL, T) + 2047) / 2048 * 2048) <= 160 * 1024;
}

// The instantiation of a map the table lists for the pass (a map serves one
// layer count), per cell.  `phase`: the phase-stamped build of map 5.
using FwdKernel = void (*)(PdrnnLstmSmallFwdArgs);
using BwdKernel = void (*)(PdrnnLstmSmallBwdArgs);
template <int CELL>
FwdKernel fwd_kernel(int map, bool phase) {
  switch (map) {
    case 0: return lstm_sw_fwd_kernel<1, 0, CELL>;
    case 1: return lstm_sw_fwd_kernel<1, 1, CELL>;
    case 2: return lstm_sw_fwd_kernel<2, 2, CELL>;
    case 5:
      if constexpr (CELL == 0) {
        if (phase) return lstm_sw_fwd4_kernel<0, true>;
      }
      return lstm_sw_fwd4_kernel<CELL, false>;
    case 6: return lstm_sw_fwd_kernel<2, 6, CELL>;
    case 8: return lstm_sw_fwd8_kernel<CELL>;
  }
  return nullptr;
}
template <int CELL>
FwdKernel infer_kernel(int map) {
  switch (map) {
    case 0: return lstm_sw_fwd_kernel<1, 0, CELL, true>;
    case 1: return lstm_sw_fwd_kernel<1, 1, CELL, true>;
    case 2: return lstm_sw_fwd_kernel<2, 2, CELL, true>;
    case 5: return lstm_sw_fwd4_infer_kernel<CELL>;
    case 6: return lstm_sw_fwd_kernel<2, 6, CELL, true>;
    case 8: return lstm_sw_fwd8_kernel<CELL, true>;
  }
  return nullptr;
}
template <int CELL>
BwdKernel bwd_kernel(int map) {
  switch (map) {
    case 0: return lstm_sw_bwd_kernel<1, 0, CELL>;
    case 1: return lstm_sw_bwd_kernel<1, 1, CELL>;
    case 2: return lstm_sw_bwd_kernel<2, 2, CELL>;
    case 3: return lstm_sw_bwd_kernel<2, 3, CELL>;
    case 4: return lstm_sw_bwd_kernel<2, 4, CELL>;
  }
  return nullptr;
}

hipError_t launch_fwd(const PdrnnLstmSmallFwdArgs* a, int map, hipStream_t st) {
  if (!map_serves(map, false, a->NL) || !map_serves_T(map, a->NL, a->T)) return hipErrorInvalidValue;
  const WaveMap& m = kMaps[map];
  const size_t lds = fwd_lds(map, a->NL, a->T);
  if (lds > 64 * 1024) return hipErrorInvalidConfiguration;
  const bool phase = a->phase_stamps && a->stamps;
  const FwdKernel k = a->cell == 1 ? fwd_kernel<1>(map, phase) : fwd_kernel<0>(map, phase);
  hipLaunchKernelGGL(k, dim3((a->B + m.nb - 1) / m.nb), dim3(64 * m.waves), lds, st, *a);
  return hipGetLastError();
}
hipError_t launch_infer(const PdrnnLstmSmallFwdArgs* a, int map, hipStream_t st) {
  if (!map_serves(map, false, a->NL) || !map_serves_T(map, a->NL, a->T)) return hipErrorInvalidValue;
  const WaveMap& m = kMaps[map];
  const size_t lds = fwd_lds(map, a->NL, a->T);
  if (lds > 64 * 1024) return hipErrorInvalidConfiguration;
  const FwdKernel k = a->cell == 1 ? infer_kernel<1>(map) : infer_kernel<0>(map);
  hipLaunchKernelGGL(k, dim3((a->B + m.nb - 1) / m.nb), dim3(64 * m.waves), lds, st, *a);
  return hipGetLastError();
}
hipError_t launch_bwd(const PdrnnLstmSmallBwdArgs* a, int map, hipStream_t st) {
  if (!map_serves(map, true, a->NL) || !map_serves_T(map, a->NL, a->T)) return hipErrorInvalidValue;
  const WaveMap& m = kMaps[map];
  // register dW: one slab row per workgroup; reads the x rows and the h sequence
  if (m.rdw && (!a->slab || !a->xg_out || a->xg_ld > 16 || !a->hseq)) return hipErrorInvalidValue;
  const BwdKernel k = a->cell == 1 ? bwd_kernel<1>(map) : bwd_kernel<0>(map);
  hipLaunchKernelGGL(k, dim3((a->B + m.nb - 1) / m.nb), dim3(64 * m.waves), bwd_lds(map, a->NL), st, *a);
  return hipGetLastError();
}

// The lean training contract of the family: zero initial state, the loss
// through the fused head on h_T, dL/dh_T of the top layer only.
bool fwd_args_ok(const PdrnnLstmSmallFwdArgs& a) {
  if (!pdrnn_lstm_sw_ok(kH, a.I, a.NL, a.cell) || a.h0 || a.c0) return false;
  if (!a.act || !a.hseq || a.B <= 0 || a.T <= 0) return false;
  if (!pdrnn_lstm_sw_fits(a.NL, a.B, a.T)) return false;  // 2 GiB descriptor range
  if (a.head_w && (a.C > 16 || a.C < 1 || !a.labels || !a.slab || !a.dh_top)) return false;
  return !a.xg_out || (a.xg_ld >= a.I && a.xg_ld <= kXS);
}
// Inference: no saved rows, no gradients, no initial state; the head is not
// optional (logits and pred are what the launch is for).
bool infer_args_ok(const PdrnnLstmSmallFwdArgs& a) {
  if (!pdrnn_lstm_sw_ok(kH, a.I, a.NL, a.cell) || a.B <= 0 || a.T <= 0) return false;
  if (a.act || a.hseq || a.xg_out || a.slab || a.dh_top || a.h0 || a.c0) return false;
  if (!a.head_w || a.C > 16 || a.C < 1 || !a.logits || !a.pred) return false;
  return !a.seq_stats || a.labels;
}
bool bwd_args_ok(const PdrnnLstmSmallBwdArgs& a) {
  if (!pdrnn_lstm_sw_ok(kH, a.I, a.NL, a.cell)) return false;
  if (a.h0 || a.c0 || a.dout || a.dcn || a.dx || a.dh0 || a.dc0 || !a.dhn || !a.dhn_top_only) return false;
  return a.act && a.B > 0 && a.T > 0 && pdrnn_lstm_sw_fits(a.NL, a.B, a.T);  // 2 GiB descriptor range
}

}  // namespace
}  // namespace pdrnn

using namespace pdrnn;

extern "C" int pdrnn_lstm_sw_ok(int H, int I, int NL, int cell) {
  return (H == kH && I >= 1 && I <= kXS && (NL == 1 || NL == 2) && (cell == 0 || cell == 1)) ? 1 : 0;
}

// Every (layer, sequence, step) row of `act` (5H floats) and `hseq` is
// addressed as a 32-bit byte offset under ONE buffer descriptor whose range
// is 2 GiB (uniform_rsrc): past it loads return 0 and stores are dropped.
// The launchers refuse batches whose last row (plus the deferred-dW padding
// rows) would not fit; the caller then takes the gate-split family, which
// rebases its descriptors per sequence.
extern "C" int pdrnn_lstm_sw_fits(int NL, int B, int T) {
  const int64_t rows = (int64_t)NL * B * T + PDRNN_DW_PAD_ROWS;
  return (NL >= 1 && B >= 1 && T >= 1 && rows * 5 * kH * 4 < ((int64_t)1 << 31)) ? 1 : 0;
}

// The plan: which map runs each pass of a batch.  Measured (bench/sw_probe.cpp,
// profiles/r5/sw): two-layer stacks run one wave per layer up to one wave per
// SIMD (map 2) -- the forward two waves per layer up to half a wave per SIMD
// (map 5: 56.5 vs 62.0 us at B = 180, 73.1 vs 81.8 at 512, slower above,
// profiles/r5/sw/fwd4_probe.log), where the backward forms the weight
// gradients itself (map 4: no dW launch; 55.7 us against 54.7 + 16.9 at
// B = 180, profiles/r5/sw/dw4_probe.log) and both fit one launch.  Above one
// wave per SIMD the forward keeps the layer waves at three per SIMD with layer
// 1's input projection on the matrix cores (map 8: the same bits as map 6,
// the per-step map, and 1.0-1.5 % on the headline step at B = 1440 / 1152,
// profiles/r7/fwd_chunked.md) and the backward takes two sequences per wave
// (map 3).  One layer: one wave per sequence (map 0), two above one wave per
// SIMD (map 1).  PDRNN_TUNE sw_mode / sw_bwd_mode override (sw_mode alone:
// both passes); a map the table does not list for the pass and layer count is
// ignored.  A map that does not run this T gives way last: 4 -> 2, 8 -> 6.
namespace {
// The maps by batch size, before the overrides and the rules on T.
void plan_by_batch(int NL, int B, int cus, int& f, int& b) {
  const int simds = 4 * cus;
  if (NL == 1) f = b = B <= simds ? 0 : 1;
  else if (2 * B <= simds) f = 5, b = 4;  // (four waves per workgroup, two workgroups per CU)
  else if (B <= simds) f = b = 2;
  else f = 8, b = 3;
}
// The forward map after PDRNN_TUNE sw_mode and the map's rule on T
int plan_fwd_map(int NL, int T, int f) {
  const int of = pdrnn_tune_int("sw_mode", -1);
  if (map_serves(of, false, NL)) f = of;
  if (!map_serves_T(f, NL, T)) f = 6;  // whole 16-step chunks, six workgroups per CU
  return f;
}
}  // namespace

extern "C" int pdrnn_lstm_sw_plan_cus(int NL, int B, int T, int cus, PdrnnLstmSwPlan* plan) {
  if ((NL != 1 && NL != 2) || T <= 0 || cus <= 0 || !pdrnn_lstm_sw_fits(NL, B, T)) return 0;
  int f, b;
  plan_by_batch(NL, B, cus, f, b);
  int ob = pdrnn_tune_int("sw_bwd_mode", -1);
  if (ob < 0) ob = pdrnn_tune_int("sw_mode", -1);
  if (map_serves(ob, true, NL)) b = ob;
  if (!map_serves_T(b, NL, T)) b = 2;  // register dW: whole 4-step K steps
  f = plan_fwd_map(NL, T, f);
  plan->fwd_map = f;
  plan->bwd_map = b;
  plan->fwd_nb = kMaps[f].nb;
  plan->bwd_nb = kMaps[b].nb;
  plan->register_dw = kMaps[b].rdw ? 1 : 0;
  plan->one_launch = (f == 5 && b == 4 && step_lds(T) <= 64 * 1024) ? 1 : 0;
  return 1;
}
extern "C" int pdrnn_lstm_sw_plan(int NL, int B, int T, PdrnnLstmSwPlan* plan) {
  return pdrnn_lstm_sw_plan_cus(NL, B, T, sw_cus(), plan);
}

extern "C" hipError_t pdrnn_lstm_sw_fwd(const PdrnnLstmSmallFwdArgs* a, int mode, hipStream_t st) {
  if (!fwd_args_ok(*a)) return hipErrorInvalidValue;
  return launch_fwd(a, mode, st);
}

// The forward half of the plan above (whether the store-free builds would
// rather switch maps elsewhere has not been measured), without the activation
// rows' limit pdrnn_lstm_sw_fits.
extern "C" int pdrnn_lstm_sw_infer_plan_cus(int NL, int B, int T, int cus, int* map) {
  if ((NL != 1 && NL != 2) || B <= 0 || T <= 0 || cus <= 0) return 0;
  int f, b;
  plan_by_batch(NL, B, cus, f, b);
  f = plan_fwd_map(NL, T, f);
  if (f == 1 && fwd_lds(1, NL, T) > 64 * 1024) f = 0;  // two sequences' x rows do not fit: one per wave
  if (fwd_lds(f, NL, T) > 64 * 1024) return 0;
  *map = f;
  return kMaps[f].nb;
}
extern "C" int pdrnn_lstm_sw_infer_plan(int NL, int B, int T, int* map) {
  return pdrnn_lstm_sw_infer_plan_cus(NL, B, T, sw_cus(), map);
}
extern "C" hipError_t pdrnn_lstm_sw_infer(const PdrnnLstmSmallFwdArgs* a, int mode, hipStream_t st) {
  if (!infer_args_ok(*a)) return hipErrorInvalidValue;
  return launch_infer(a, mode, st);
}

extern "C" hipError_t pdrnn_lstm_sw_bwd(const PdrnnLstmSmallBwdArgs* a, int mode, hipStream_t st) {
  if (!bwd_args_ok(*a) || !a->dg_out || a->dg_st < 4 * kH) return hipErrorInvalidValue;
  return launch_bwd(a, mode, st);
}

// Maps 5 and 4 in one workgroup: the head and the staged x rows are not
// optional, and both argument blocks describe the same batch and buffers.
extern "C" hipError_t pdrnn_lstm_sw_step(const PdrnnLstmSmallFwdArgs* f, const PdrnnLstmSmallBwdArgs* b,
                                         hipStream_t st) {
  if (!fwd_args_ok(*f) || !bwd_args_ok(*b)) return hipErrorInvalidValue;
  if (!map_serves(5, false, f->NL) || !map_serves_T(4, f->NL, f->T)) return hipErrorInvalidValue;
  if (!f->head_w || !f->xg_out || !b->slab) return hipErrorInvalidValue;
  if (b->cell != f->cell || b->B != f->B || b->T != f->T || b->NL != f->NL || b->act != f->act ||
      b->hseq != f->hseq || b->dhn != f->dh_top || b->xg_out != f->xg_out)
    return hipErrorInvalidValue;
  const size_t lds = step_lds(f->T);
  if (lds > 64 * 1024) return hipErrorInvalidConfiguration;
  const dim3 block(64 * kMaps[4].waves);
  if (f->cell == 1) hipLaunchKernelGGL(lstm_sw_step_kernel<1>, dim3(f->B), block, lds, st, *f, *b);
  else hipLaunchKernelGGL(lstm_sw_step_kernel<0>, dim3(f->B), block, lds, st, *f, *b);
  return hipGetLastError();
}
