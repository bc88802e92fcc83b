// Bidirectional LSTM stack + classifier head without gradients, ONE launch
// per batch (H = 32, input size <= 12, 1-2 layers, C <= 16), fp32, gfx950.
// The motion classifier's `--bidirectional` evaluation (docs/DESIGN.md §2b).
//
// The head reads out[:, -1, :] = [h_fwd after T steps | h_bwd after its FIRST
// step] (the reverse direction starts at position T - 1).  So the top layer's
// reverse direction is one cell step from a zero state, not T, and nothing of
// the [B, T, 2H] output sequence exists anywhere: the launch writes logits,
// pred and -- with labels -- one [loss / B, 1, correct] row per sequence.
//
//  * Work split.  A sequence is served by two waves, one per direction; a
//    workgroup holds `ns` sequences (the plan), wave w = direction w / ns of
//    sequence w % ns: the waves of one direction are adjacent, so where only
//    the forward waves are busy (below) they spread over the CU's SIMDs.
//    Each sequence's pair of waves stages its x rows into LDS once.
//  * Layer 0 runs the sequence-in-wave step of lstm_sw.hip: lane = (unit
//    u = lane >> 1, K half s = lane & 1), the four gate rows of
//    [W_ih | W_hh] over the lane's operand half in VGPRs (rows pre-scaled by
//    -log2 e: sigma(z) = 1 / (1 + 2^acc), v_exp_f32 / v_rcp_f32), DPP swaps
//    for the K-split sums and the gates; h goes through a per-wave LDS parity
//    slot, c never leaves the wave.  The directions walk time in opposite
//    orders and touch disjoint LDS.
//      - one layer: the forward wave runs T steps; the reverse wave, having
//        helped stage x, runs its single step at x[T - 1] and parks at the
//        barrier ahead of the head.
//      - two layers: both waves run T steps and write h_t into the LDS
//        sequence buffers h0[dir][t][36] (row stride 36: the MFMA A reads of
//        16 rows spread over the banks); ONE workgroup barrier, then layer 1.
//  * Layer 1 (two layers).  Its reverse direction is again one step, so the
//    reverse wave is free: it is the PRODUCER of the forward direction's
//    input projection on the matrix cores.  Per 16-step chunk it forms
//    P[16][128] = [h0_fwd | h0_bwd][16, 64] x W_ih^T[64, 128] + b with
//    v_mfma_f32_16x16x4_f32 (8 column tiles x 16 K steps, the B fragments
//    resident in 128 VGPRs, A straight out of h0) into one half of a
//    double-buffered LDS tile, one chunk ahead of the forward wave.  The
//    forward wave (CONSUMER) keeps only the h W_hh half in its step: lane s
//    runs the full 32-column chains of its own two gates (s = 0: i, g;
//    s = 1: f, o) and adds its two P values (one ds_read_b64).  One workgroup
//    barrier per chunk, none per step.  While the forward wave runs the last
//    chunk the producer does layer 1's single reverse step (its weights
//    streamed from memory once: K = 64, from a zero state, so no W_hh).
//  * Head: both waves put their final h into a 64-float LDS row; the forward
//    wave forms the C logits over the 2H columns (lane = column), argmax
//    (strict >: the lowest class on ties) and the log-sum-exp loss, with the
//    semantics of motion_head_infer.
//  * Ordering: s_waitcnt lgkmcnt(0); s_barrier only (lds_barrier).  No atomics
//    and no grid-wide wait; every sum has one fixed order, so a launch is
//    bitwise repeatable.
//
// The products are plain v_fma_f32 (this file is built with the packed fp32
// operations off).  The cell arithmetic and the lane map are copies of the few
// helpers in lstm_sw.hip; that file is unchanged.
#include "pdrnn/api.h"
#include "pdrnn/common.h"

#include <algorithm>

namespace pdrnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH = 32;
constexpr float kA = -1.4426950408889634f;  // -log2(e)
constexpr int kHB = 36;                     // h row: 32 values + a zero chunk (layer 0, s = 1) / bank spread
constexpr int kXS = 12;                     // staged x row, zero-padded
constexpr int kCT = 16;                     // steps per projection chunk (MFMA M)
constexpr int kPS = 4 * kH + 4;             // P row stride, floats
constexpr int kMaxSeq = 4;                  // sequences per workgroup, at most
constexpr size_t kLdsCap = 64 * 1024;

// LDS floats of one sequence: slots [2 dirs][2 parities][kHB] | head row [2H]
// | x rows [T][kXS] | two layers: h0 [2][T][kHB] | P [2][kCT][kPS] | C seeds [4H]
constexpr int kOffHc = 2 * 2 * kHB, kOffX = kOffHc + 2 * kH;
PDRNN_HOST_DEVICE inline int seq_floats(int NL, int T) {
  return kOffX + T * kXS + (NL == 2 ? 2 * T * kHB + 2 * kCT * kPS + 4 * kH : 0);
}

PDRNN_DEVICE float sig2(float z) { return fast_rcp(1.f + __builtin_amdgcn_exp2f(z)); }
PDRNN_DEVICE float tanh_c(float c) { return fmaf(sig2(c * (2.f * kA)), 2.f, -1.f); }
PDRNN_DEVICE float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
PDRNN_DEVICE float gate_scale(int q) { return kA * (q == 2 ? 2.f : 1.f); }  // tanh(g) = 2 sigma(2g) - 1
// DPP quad_perm [1, 1, 3, 3]: both lanes of a pair read the odd lane
PDRNN_DEVICE float from_odd(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xF5, 0xF, 0xF, false));
}
// gate row of P column p: column 4u + 2s + j is gate s + 2j of unit u
PDRNN_DEVICE int p_row(int p) { return (((p >> 1) & 1) + 2 * (p & 1)) * kH + (p >> 2); }

// The pair's pre-activations (s = 0: i, g; s = 1: f, o; scaled rows) -> the
// unit's new c and h on both lanes (lstm_sw.hip's fwd_cell_z).
PDRNN_DEVICE float cell_z(float z0, float z1, float& c, bool odd) {
  const float a0 = sig2(z0);
  const float a1 = odd ? sig2(z1) : fmaf(sig2(z1), 2.f, -1.f);
  const float term = a0 * (odd ? c : a1);
  c = term + dpp_swap1(term);
  return from_odd(a1) * tanh_c(c);
}

// Layer 0, direction d: this lane's four gate rows over the 6 float4 chunks
// of its operand half (s = 0: x (12, zero-padded) | h[0, 12); s = 1: h[12, 32)
// | zero chunk), in the order (m0, x0, m1, x1): m0 / m1 the gates this lane
// activates, x0 / x1 its partner's.  The biases seed m0 / m1.
struct W0 {
  float w[4][24];
  float bias[2];
};
PDRNN_DEVICE W0 load_w0(const PdrnnLstmBidirInferArgs& a, int d, int u, int s) {
  W0 W;
  const int I = a.I;
  const float* wih = a.w_ih[0][d];
  const float* whh = a.w_hh[0][d];
  const int gq[4] = {s, 1 - s, 2 + s, 3 - s};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = gq[j], r = q * kH + u;
    const float sc = gate_scale(q);
#pragma unroll
    for (int e = 0; e < 24; ++e) {
      float x = 0.f;
      if (s == 0) {
        if (e < kXS) { if (e < I) x = wih[(int64_t)r * I + e]; }
        else x = whh[r * kH + e - kXS];
      } else if (e < 20) {
        x = whh[r * kH + kXS + e];
      }
      W.w[j][e] = x * sc;
    }
    if (!(j & 1)) W.bias[j >> 1] = (a.b_ih[0][d][r] + a.b_hh[0][d][r]) * sc;
  }
  return W;
}
PDRNN_DEVICE float step0(const W0& W, const float4 (&v)[6], float& c, bool odd) {
  float acc[4][2] = {{W.bias[0], 0.f}, {0.f, 0.f}, {W.bias[1], 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int cc = 0; cc < 6; ++cc)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j][0] = fmaf(W.w[j][4 * cc], v[cc].x, acc[j][0]);
      acc[j][1] = fmaf(W.w[j][4 * cc + 1], v[cc].y, acc[j][1]);
      acc[j][0] = fmaf(W.w[j][4 * cc + 2], v[cc].z, acc[j][0]);
      acc[j][1] = fmaf(W.w[j][4 * cc + 3], v[cc].w, acc[j][1]);
    }
  float p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = acc[j][0] + acc[j][1];
  return cell_z(p[0] + dpp_swap1(p[1]), p[2] + dpp_swap1(p[3]), c, odd);
}

// Head on the sequence's [h_fwd | h_bwd] row (lane = column), the semantics of
// motion_head_infer: logits[b, 0..C), pred[b], seq_stats[b] with labels.
PDRNN_DEVICE void bidir_head(const PdrnnLstmBidirInferArgs& a, int b, int bsrc, const float* hc, int lane) {
  const int C = a.C;
  const float hv = hc[lane];
  const int64_t lab = a.labels ? a.labels[bsrc] : (int64_t)-1;
  float w[16], bias[16];
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    w[cc] = cc < C ? a.head_w[cc * 2 * kH + lane] : 0.f;
    bias[cc] = (cc < C && a.head_b) ? a.head_b[cc] : 0.f;
  }
  float lg[16];
  float m = -INFINITY, logit_y = 0.f, mine = 0.f;
  int amax = 0;
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    if (cc < C) {
      const float z = wave_sum(w[cc] * hv) + bias[cc];
      lg[cc] = z;
      if (z > m) { m = z; amax = cc; }
      if (cc == lab) logit_y = z;
      if (cc == lane) mine = z;
    }
  }
  if (lane < C) a.logits[(int64_t)b * C + lane] = mine;
  if (lane == 0) a.pred[b] = amax;
  if (a.seq_stats) {
    float se = 0.f;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc)
      if (cc < C) se += expf(lg[cc] - m);
    const float loss = logf(se) - (logit_y - m);  // (the difference of two logits first)
    if (lane == 0) {
      float* st = a.seq_stats + (int64_t)b * 3;
      st[0] = loss * a.inv_batch;
      st[1] = 1.f;
      st[2] = amax == lab ? 1.f : 0.f;
    }
  }
}

template <int NL>
__global__ void __launch_bounds__(128 * kMaxSeq) lstm_bidir_infer_kernel(PdrnnLstmBidirInferArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ns = (int)blockDim.x >> 7;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = wv % ns, d = wv / ns;  // sequence in the workgroup, direction
  const int u = lane >> 1, s = lane & 1;
  const bool odd = s != 0;
  const int B = a.B, T = a.T, I = a.I;
  const int b = blockIdx.x * ns + n;
  const bool valid = b < B;
  const int bc = valid ? b : B - 1;  // an empty slot recomputes the last sequence, stores nothing
  const int bsrc = a.idx ? (int)a.idx[bc] : bc;

  float* sq = smem + n * seq_floats(NL, T);
  float* slots = sq + d * 2 * kHB;
  float* hc = sq + kOffHc;
  float* xs = sq + kOffX;
  float* h0 = xs + T * kXS;
  float* P = h0 + 2 * T * kHB;
  float* cseed = P + 2 * kCT * kPS;

  // ---- prologue, by the sequence's two waves: h_{-1} = 0 (slots and their
  // pad chunks), x staged and zero-padded, layer 1's MFMA C seeds (the biases
  // in P's column order)
  const int tp = d * 64 + lane;
  for (int e = tp; e < kOffHc; e += 128) sq[e] = 0.f;
  {
    const int tot = T * kXS;
    for (int e0 = tp; e0 < tot; e0 += 4 * 128) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = min(e0 + r * 128, tot - 1);
        const int t = e / kXS, k = e - t * kXS;
        const float x = a.x[(int64_t)bsrc * a.x_sb + (int64_t)t * a.x_st + min(k, I - 1)];
        v[r] = k < I ? x : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = e0 + r * 128;
        if (e < tot) xs[e] = v[r];
      }
    }
  }
  if constexpr (NL == 2) {
    const int r = p_row(tp);
    cseed[tp] = (a.b_ih[1][0][r] + a.b_hh[1][0][r]) * gate_scale(r / kH);
  }
  lds_barrier();

  // ---- layer 0: T steps (one layer, reverse direction: its first step only)
  float h = 0.f;
  {
    const W0 W = load_w0(a, d, u, s);
    const int nsteps = (NL == 1 && d == 1) ? 1 : T;
    float c = 0.f;
    for (int k = 0; k < nsteps; ++k) {
      const int t = d ? T - 1 - k : k;
      const float* hp = slots + ((k - 1) & 1) * kHB;
      const float* pa = odd ? hp + 12 : xs + t * kXS;
      const float* pb = odd ? hp + 24 : hp;
      float4 v[6];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) v[cc] = ld4(pa + 4 * cc);
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) v[3 + cc] = ld4(pb + 4 * cc);
      h = step0(W, v, c, odd);
      slots[(k & 1) * kHB + u] = h;
      if constexpr (NL == 2) h0[(d * T + t) * kHB + u] = h;
    }
  }

  if constexpr (NL == 2) {
    lds_barrier();  // both directions' layer-0 sequences are complete
    const int nch = (T + kCT - 1) / kCT;
    if (d == 0) {
      // ---- consumer: layer 1 forward, the h W_hh half per step + P
      for (int e = lane; e < 2 * kHB; e += 64) slots[e] = 0.f;  // (own slots: a wave's LDS operations run in order)
      float wr[2][kH];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int q = s + 2 * jj, r = q * kH + u;
        const float sc = gate_scale(q);
#pragma unroll
        for (int k = 0; k < kH; ++k) wr[jj][k] = a.w_hh[1][0][r * kH + k] * sc;
      }
      float c = 0.f;
      for (int it = 0; it <= nch; ++it) {
        if (it > 0) {
          const int t0 = (it - 1) * kCT;
          const float* Pc = P + ((it - 1) & 1) * kCT * kPS;
          const int len = min(kCT, T - t0);
          for (int i = 0; i < len; ++i) {
            const int t = t0 + i;
            const float* hp = slots + ((t - 1) & 1) * kHB;
            float4 v[8];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) v[cc] = ld4(hp + 4 * cc);
            const float2 pin = *reinterpret_cast<const float2*>(Pc + i * kPS + 2 * lane);
            float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
#pragma unroll
              for (int jj = 0; jj < 2; ++jj) {
                acc[jj][0] = fmaf(wr[jj][4 * cc], v[cc].x, acc[jj][0]);
                acc[jj][1] = fmaf(wr[jj][4 * cc + 1], v[cc].y, acc[jj][1]);
                acc[jj][0] = fmaf(wr[jj][4 * cc + 2], v[cc].z, acc[jj][0]);
                acc[jj][1] = fmaf(wr[jj][4 * cc + 3], v[cc].w, acc[jj][1]);
              }
            h = cell_z((acc[0][0] + acc[0][1]) + pin.x, (acc[1][0] + acc[1][1]) + pin.y, c, odd);
            slots[(t & 1) * kHB + u] = h;
          }
        }
        lds_barrier();
      }
    } else {
      // ---- producer: P for chunk `it`, then layer 1's single reverse step
      const int mi = lane & 15, kk = lane >> 4;  // MFMA fragment row / K index
      // B fragments of the forward W_ih^1: column tile nt, K step 2 j + e -> column 8 j + 2 kk + e
      float bw[8][16];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const int r = p_row(16 * nt + mi);
        const float sc = gate_scale(r / kH);
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int e = 0; e < 2; ++e) bw[nt][2 * j + e] = a.w_ih[1][0][r * 2 * kH + 8 * j + 2 * kk + e] * sc;
      }
      for (int it = 0; it <= nch; ++it) {
        if (it < nch) {
          const int t = min(it * kCT + mi, T - 1);  // (rows past T: computed, never read)
          float* Pc = P + (it & 1) * kCT * kPS;
          float2 av[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            av[j] = *reinterpret_cast<const float2*>(h0 + ((j >> 2) * T + t) * kHB + 8 * (j & 3) + 2 * kk);
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) {
            const float b0 = cseed[16 * nt + mi];
            f32x4 acc = {b0, b0, b0, b0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bw[nt][2 * j], acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bw[nt][2 * j + 1], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Pc[(4 * kk + r) * kPS + 16 * nt + mi] = acc[r];
          }
        } else {
          // reverse direction of layer 1 at position T - 1, from a zero state:
          // z = W_ih [h0_fwd | h0_bwd][T - 1] + b_ih + b_hh, c = i g, h = o tanh(c)
          // (lane s sums K half s of all four gates; one swap completes them)
          const float* hv = h0 + (s * T + T - 1) * kHB;
          float z[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int r = q * kH + u;
            const float* wrow = a.w_ih[1][1] + r * 2 * kH + s * kH;
            float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
              const float4 hq = ld4(hv + 4 * cc);  // (the weights as scalars: a parameter may sit at any float offset)
              acc0 = fmaf(wrow[4 * cc], hq.x, acc0);
              acc1 = fmaf(wrow[4 * cc + 1], hq.y, acc1);
              acc0 = fmaf(wrow[4 * cc + 2], hq.z, acc0);
              acc1 = fmaf(wrow[4 * cc + 3], hq.w, acc1);
            }
            const float part = acc0 + acc1;
            z[q] = ((part + dpp_swap1(part)) + (a.b_ih[1][1][r] + a.b_hh[1][1][r])) * gate_scale(q);
          }
          const float cr = sig2(z[0]) * fmaf(sig2(z[2]), 2.f, -1.f);
          h = sig2(z[3]) * tanh_c(cr);
        }
        lds_barrier();
      }
    }
  }

  // ---- head on [h_fwd | h_bwd], by the forward wave
  hc[d * kH + u] = h;
  lds_barrier();
  if (d == 0 && valid) bidir_head(a, b, bsrc, hc, lane);
}

int device_cus() {
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

}  // namespace
}  // namespace pdrnn

using namespace pdrnn;

extern "C" int pdrnn_lstm_bidir_infer_ok(int H, int I, int NL, int cell) {
  return (H == kH && I >= 1 && I <= kXS && (NL == 1 || NL == 2) && cell == 0) ? 1 : 0;
}

// Sequences per workgroup: as many as the LDS cap holds (at most kMaxSeq),
// fewer while that would leave CUs without a workgroup.
extern "C" int pdrnn_lstm_bidir_infer_plan_cus(int NL, int B, int T, int cus, int* lds_bytes) {
  if ((NL != 1 && NL != 2) || B <= 0 || T <= 0 || cus <= 0) return 0;
  const int64_t fl = (int64_t)kOffX + (int64_t)T * kXS + (NL == 2 ? (int64_t)2 * T * kHB + 2 * kCT * kPS + 4 * kH : 0);
  const int64_t seq = fl * (int64_t)sizeof(float);
  if (seq > (int64_t)kLdsCap) return 0;
  int ns = (int)std::min<int64_t>(kMaxSeq, (int64_t)kLdsCap / seq);
  while (ns > 1 && (B + ns - 1) / ns < cus) --ns;
  if (lds_bytes) *lds_bytes = (int)(seq * ns);
  return ns;
}
extern "C" int pdrnn_lstm_bidir_infer_plan(int NL, int B, int T, int* lds_bytes) {
  return pdrnn_lstm_bidir_infer_plan_cus(NL, B, T, device_cus(), lds_bytes);
}

extern "C" hipError_t pdrnn_lstm_bidir_infer(const PdrnnLstmBidirInferArgs* a, int ns, hipStream_t st) {
  if (!pdrnn_lstm_bidir_infer_ok(kH, a->I, a->NL, 0) || a->B <= 0 || a->T <= 0) return hipErrorInvalidValue;
  if (!a->x || !a->head_w || a->C < 1 || a->C > 16 || !a->logits || !a->pred) return hipErrorInvalidValue;
  if (a->seq_stats && !a->labels) return hipErrorInvalidValue;
  for (int l = 0; l < a->NL; ++l)
    for (int d = 0; d < 2; ++d)
      if (!a->w_ih[l][d] || !a->w_hh[l][d] || !a->b_ih[l][d] || !a->b_hh[l][d]) return hipErrorInvalidValue;
  if (ns < 1 || ns > kMaxSeq) return hipErrorInvalidValue;
  const size_t lds = sizeof(float) * (size_t)ns * (size_t)seq_floats(a->NL, a->T);
  if ((size_t)a->T > kLdsCap || lds > kLdsCap) return hipErrorInvalidConfiguration;
  const dim3 grid((a->B + ns - 1) / ns), block(128 * ns);
  if (a->NL == 1) hipLaunchKernelGGL(lstm_bidir_infer_kernel<1>, grid, block, lds, st, *a);
  else hipLaunchKernelGGL(lstm_bidir_infer_kernel<2>, grid, block, lds, st, *a);
  return hipGetLastError();
}
