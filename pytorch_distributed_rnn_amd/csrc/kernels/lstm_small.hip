// Fused small-hidden LSTM stack, forward and BPTT backward, fp32, gfx950.
//
// Replaces the ATen CPU `_VF.lstm` the reference drives through nn.LSTM
// (reference: src/motion/model.py:9,14; per-step cell math in SURVEY.md §3.5).
//
// Design (MI355X-first, see docs/DESIGN.md):
//  * One workgroup owns NB whole sequences for all T timesteps and all NL
//    layers: the recurrence never leaves the CU, no per-timestep launches.
//  * Layers are wave-pipelined: at iteration `it` layer l processes t = it - l,
//    so the stack costs T + NL - 1 dependent steps instead of NL * T.  One
//    workgroup barrier per iteration; layer hand-offs go through double-
//    buffered LDS vectors.
//  * Forward, gate-split map (the default, lstm_small_fwd_gs_kernel): a layer
//    group is 4H lanes, lane = (unit u, gate q).  Each lane keeps ITS row of
//    [W_ih | W_hh] in VGPRs for the whole launch and reads the whole
//    [x_t | h_{t-1}] operand vector from LDS with broadcast ds_read_b128; the
//    four gates of a unit meet through DPP quad permutes (no LDS).  Above one
//    residency round (B > 1024 at H = 32) the host picks the 2-lane K-split
//    map instead (lstm_small_fwd_kernel: lane = (unit, K-slice), each lane
//    reads half the operand vector and holds all four gates of its slice).
//  * Backward, unit-group map (the default, lstm_small_bwd_gs_kernel): a layer
//    group is H*L lanes, L = 4 lanes per hidden unit (8 at H = 64).  In the
//    row phase a lane computes the gate gradients of its unit; in the column
//    phase it owns a 4H/L row slice of column k of [W_ih | W_hh] AND
//    accumulates dW of that slice in registers across all timesteps and all
//    NB sequences (the weight gradient never round-trips through HBM per
//    timestep), producing dh_{t-1} and d(input) for the layer below with the
//    same FMAs.  The grid is persistent (resident workgroups walk the batch
//    tiles); partial per-workgroup dW go to a slab that a deterministic
//    reduction sums (pdrnn_slab_reduce / pdrnn_slab_reduce_adam, adam.hip).
//    Variants on the same body: the deferred-dW backward (writes the gate
//    gradients for the matrix-core kernel lstm_small_dw.hip) and the
//    one-launch step (forward + head/CE + BPTT of one sequence per workgroup).
//    The older row/column split (lstm_small_bwd_kernel) is kept behind
//    PDRNN_TUNE split_bwd=2.
//  * Layer-0 input is zero-padded to H columns so every layer has K = 2H:
//    layers are load-balanced in the pipeline and there is one code path.
#include "pdrnn/api.h"
#include "pdrnn/common.h"

#include <cstring>
#include <type_traits>
#include <vector>

namespace pdrnn {
namespace {

// x sequence preloaded into LDS once (zero-padded to H columns) when it fits:
// layer 0 then reads its input slice straight from LDS every step -- no
// per-step global load on the recurrence's critical path.
constexpr int kXldsBytes = 48 * 1024;

// bf16 models keep fp32 master weights; the kernels use them rounded to bf16
// (round-to-nearest-even, v_cvt_pk_bf16_f32) as they load them
__device__ __forceinline__ float wround(float v, int w_bf16) { return w_bf16 ? (float)(__bf16)v : v; }


// Stage one sequence's inputs x[t][0..I) into the LDS image xs[t][0..H)
// (columns >= I zero): only the I real columns are loaded (not H), 4 loads
// in flight per thread, so the prologue is one memory round trip instead of
// T*H/blockDim dependent ones.
// xg (optional): the staged rows are also written, widened to fp32, to a
// contiguous [T][I] image (the deferred-dW kernel's layer-0 operand: no
// per-row gather or bf16 handling there).
template <int H>
__device__ __forceinline__ void stage_x(float* dst, const float* x, int64_t base, int64_t x_st, int T, int I,
                                        int bf, bool valid, float* xg = nullptr, int xg_ld = 0) {
  const int nthr = blockDim.x;
  for (int e = threadIdx.x; e < T * H; e += nthr) {
    const int k = e % H;
    if (k >= I || !valid) dst[e] = 0.f;
  }
  if (!valid) return;
  const int n = T * I;
  for (int e0 = threadIdx.x; e0 < n; e0 += 4 * nthr) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = min(e0 + r * nthr, n - 1);
      const int t = e / I, k = e - t * I;
      v[r] = ldx(x, base + (int64_t)t * x_st + k, bf);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = e0 + r * nthr;
      if (e < n) {
        const int t = e / I, k = e - t * I;
        dst[t * H + k] = v[r];
        if (xg) xg[t * xg_ld + k] = v[r];
      }
    }
  }
}

template <int H, int NB>
__device__ __forceinline__ void preload_x(float* xs, const PdrnnLstmSmallFwdArgs& a, const int* bsrc,
                                          const bool* valid) {
  for (int n = 0; n < NB; ++n)
    stage_x<H>(xs + (int64_t)n * a.T * H, a.x, (int64_t)bsrc[n] * a.x_sb, a.x_st, a.T, a.I, a.x_bf16, valid[n]);
}

// Fused classifier head + cross-entropy on the top layer's h_T (motion
// training step), shared by the gate-split and K-split forward kernels: both
// leave h_T in the top layer's hidden slot of the LDS operand buffers
// ([NB][NL][2][2H], parity T & 1).  Wave n handles sequence n of the tile.
// Label and head-weight column of this lane, loaded before the recurrence
// (the one-launch step): the epilogue's idx -> label -> logits chain then
// starts from registers instead of two dependent global round trips.
struct HeadPre {
  int64_t lab;
  float w[16];
};
template <int H, int NB>
__device__ __forceinline__ HeadPre head_prefetch(const PdrnnLstmSmallFwdArgs& a, int bbase) {
  HeadPre pre{};
  const int n = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = bbase + n;
  if (n < NB && b < a.B) {
    pre.lab = a.labels[a.idx ? a.idx[b] : b];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) pre.w[cc] = (cc < a.C && lane < H) ? a.head_w[cc * H + lane] : 0.f;
  }
  return pre;
}

template <int H, int NB>
__device__ __forceinline__ void fwd_head_epilogue(const PdrnnLstmSmallFwdArgs& a, const float* smem, int bbase,
                                                  const HeadPre* pre = nullptr, float* dh_lds = nullptr) {
  constexpr int K = 2 * H;
  const int NL = a.NL, B = a.B, T = a.T;
  const int tid = threadIdx.x;
  auto vin = [&](int n, int l, int p) -> const float* { return smem + ((n * NL + l) * 2 + p) * K; };
  static_assert(NB <= 4, "one wave per sequence of the tile");
  const int n = tid >> 6;
  const int b = bbase + n;
  if (n < NB && b < B) {
    const int lane = tid & 63;
    const float* hT = vin(n, NL - 1, T & 1) + H;
    const float hv = lane < H ? hT[lane] : 0.f;
    const int64_t lab = pre ? pre->lab : a.labels[a.idx ? a.idx[b] : b];
    const int C = a.C;
    float m = -INFINITY, logit_y = 0.f;
    int amax = 0;
    float lg_c[16];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
      if (cc < C) {
        const float wv = pre ? pre->w[cc] : (lane < H ? a.head_w[cc * H + lane] : 0.f);
        float z = wave_sum(wv * hv) + (a.head_b ? a.head_b[cc] : 0.f);
        lg_c[cc] = z;
        if (z > m) { m = z; amax = cc; }
        if (cc == lab) logit_y = z;
      }
    }
    float se = 0.f;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc)
      if (cc < C) se += expf(lg_c[cc] - m);
    const float lse = m + logf(se);
    const float inv_se = 1.f / se;
    float* srow = a.slab + (int64_t)b * a.slab_P;
    float dh = 0.f;
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
      if (cc < C) {
        const float d = (expf(lg_c[cc] - m) * inv_se - (cc == lab ? 1.f : 0.f)) * a.inv_batch;
        if (lane < H) {
          dh = fmaf(pre ? pre->w[cc] : a.head_w[cc * H + lane], d, dh);
          srow[a.head_off_w + cc * H + lane] = d * hv;
        }
        if (lane == 0 && a.head_b) srow[a.head_off_b + cc] = d;
      }
    }
    if (lane < H) {
      a.dh_top[(int64_t)b * H + lane] = dh;
      if (dh_lds) dh_lds[lane] = dh;  // one-launch step: handed to the backward half through LDS
    }
    if (lane == 0) {  // [mean-loss contribution, count, correct] -> column sums are the batch stats
      srow[a.stat_off + 0] = (lse - logit_y) * a.inv_batch;
      srow[a.stat_off + 1] = 1.f;
      srow[a.stat_off + 2] = amax == lab ? 1.f : 0.f;
    }
  }
}

constexpr float kNegLog2eK = -1.4426950408889634f;

// H <= 32: at most 168 VGPRs, three waves per SIMD -- the B = 1440 forward
// (2880 waves on 1024 SIMDs) must stay one residency round (170 VGPRs with
// the packed K loop would drop it to two: 135 -> 184 us)
template <int H, int S, int NB, bool SAVE, bool XLDS, bool HEAD = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(H <= 32 ? 3 : 1)))
lstm_small_fwd_kernel(PdrnnLstmSmallFwdArgs a) {
  constexpr int K = 2 * H;
  constexpr int KS = K / S;
  constexpr int LANES = H * S;
  static_assert(KS % 4 == 0 && H % KS == 0, "K slice must be float4 aligned and not straddle");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int NL = a.NL, B = a.B, T = a.T, I = a.I;
  const int tid = threadIdx.x;
  const uint64_t sr_in = (a.stamps && tid == 0) ? stamp_real() : 0;
  const int layer = __builtin_amdgcn_readfirstlane(tid / LANES);
  const int lg = tid - layer * LANES;
  const int u = lg / S;
  const int s = lg % S;
  const int k0 = s * KS;  // first column of this lane's K slice
  const int bbase = blockIdx.x * NB;
  const int Iin = layer == 0 ? I : H;

  // LDS: vin[n][l][p][K] (k < H layer input, k >= H own hidden) | xs[n][T][H]
  float* xs = smem + NB * NL * 2 * K;
  auto vin = [&](int n, int l, int p) -> float* { return smem + ((n * NL + l) * 2 + p) * K; };

  // ---- this lane's rows q*H+u of [W_ih | W_hh], columns k0 .. k0+KS-1 ----
  float w[4][KS];
  float bias[4];
  {
    const bool in_part = k0 < H;
    const float* src = in_part ? a.w_ih[layer] : a.w_hh[layer];
    const int ld = in_part ? Iin : H;
    const int c0 = in_part ? k0 : k0 - H;
    // float4 row loads where the slice is aligned (every h part, the input
    // part of layers >= 1): each lane reads a different row, so every load
    // instruction touches 64 cache lines -- 4x fewer instructions matter at
    // B = 1440, where all workgroups load the weights at once (the prologue
    // was ~27 us with scalar loads)
    const bool vec = (ld % 4) == 0 && (!in_part || Iin == H);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = q * H + u;
      if (vec) {
#pragma unroll
        for (int k4 = 0; k4 < KS / 4; ++k4) {
          const float4 v = *reinterpret_cast<const float4*>(src + r * ld + c0 + 4 * k4);
          w[q][4 * k4 + 0] = wround(v.x, a.w_bf16); w[q][4 * k4 + 1] = wround(v.y, a.w_bf16);
          w[q][4 * k4 + 2] = wround(v.z, a.w_bf16); w[q][4 * k4 + 3] = wround(v.w, a.w_bf16);
        }
      } else {
        // only the live columns are loaded: for the layer-0 input slice
        // (I << KS) the guard is uniform over the slice's lanes, so the
        // zero-padded tail issues no loads at all (128 -> 4 I per lane)
        const int lim = in_part ? Iin : H;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          const int c = c0 + kk;
          float v = 0.f;
          if (c < lim) v = src[r * ld + c];
          w[q][kk] = wround(v, a.w_bf16);
        }
      }
      bias[q] = (a.b_ih[layer] ? wround(a.b_ih[layer][r], a.w_bf16) : 0.f) +
                (a.b_hh[layer] ? wround(a.b_hh[layer][r], a.w_bf16) : 0.f);
    }
    if constexpr (S == 2) {
      // pre-scaled rows (as in the gate-split map): the pre-activation comes
      // out as -log2(e) z (x2 for the g gate), so sigmoid = 1 / (1 + 2^acc)
      // and tanh(g) = 2 sigmoid(2g) - 1 with no scaling in the recurrence
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float sc = kNegLog2eK * (q == 2 ? 2.f : 1.f);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) w[q][kk] *= sc;
        bias[q] *= sc;
      }
    }
  }

  pdrnn_f2 w2[4][KS / 2];  // k pairs of the slice (packed FMA operands)
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < KS / 2; ++j) w2[q][j] = pdrnn_f2{w[q][2 * j], w[q][2 * j + 1]};

  int bsrc[NB];
  bool valid[NB];
  float c[NB], hl[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    valid[n] = b < B;
    bsrc[n] = valid[n] ? (a.idx ? (int)a.idx[b] : b) : 0;
    const int bc = min(b, B - 1);
    const float h_init = (a.h0 && valid[n]) ? a.h0[((int64_t)layer * B + bc) * H + u] : 0.f;
    c[n] = (a.c0 && valid[n]) ? a.c0[((int64_t)layer * B + bc) * H + u] : 0.f;
    hl[n] = h_init;
    if (s == 0) vin(n, layer, 0)[H + u] = h_init;
    if (!XLDS && layer == 0 && lg < H)
      vin(n, 0, 0)[lg] = (valid[n] && lg < I) ? a.x[bsrc[n] * a.x_sb + lg] : 0.f;
  }
  if constexpr (XLDS) preload_x<H, NB>(xs, a, bsrc, valid);
  __syncthreads();

  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }
  const int iters = T + NL - 1;
  for (int it = 0; it < iters; ++it) {
    prio_by_progress(it, iters, a.prio);
    const int t = it - layer;
    if (t >= 0 && t < T) {
      const int p = t & 1;
      float xnext[NB];
      if (!XLDS && layer == 0 && lg < H) {
        const int tn = min(t + 1, T - 1);
        const int kx = min(lg, I - 1);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float v = a.x[bsrc[n] * a.x_sb + (int64_t)tn * a.x_st + kx];  // unconditional load
          xnext[n] = (t + 1 < T && valid[n] && lg < I) ? v : 0.f;
        }
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const float* src = vin(n, layer, p) + k0;
        if (XLDS && layer == 0 && k0 < H) src = xs + ((int64_t)n * T + t) * H + k0;
        const float4* v4 = reinterpret_cast<const float4*>(src);
        // packed fp32 FMAs over k pairs (v_pk_fma_f32: 2 MACs per lane and
        // instruction, 64 instead of 128 per step), halves summed at the end
        pdrnn_f2 acc2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int k4 = 0; k4 < KS / 4; ++k4) {
          const float4 v = v4[k4];
          const pdrnn_f2 vlo = {v.x, v.y}, vhi = {v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc2[q] = __builtin_elementwise_fma(w2[q][2 * k4], vlo, acc2[q]);
            acc2[q] = __builtin_elementwise_fma(w2[q][2 * k4 + 1], vhi, acc2[q]);
          }
        }
        float acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = group_sum<S>(acc2[q].x + acc2[q].y) + bias[q];
        if constexpr (S == 2 && NB == 1 && SAVE) {
          // the unit's two lanes split the activations (lane 0: i, g; lane
          // 1: f, o; one DPP swap exchanges them) and the stores: every lane
          // writes one LDS slot and three global words, no branches
          const float z0 = s == 0 ? acc[0] : acc[1];
          const float z1 = s == 0 ? acc[2] : acc[3];
          const float a0 = fast_rcp(1.f + __builtin_amdgcn_exp2f(z0));               // i | f
          const float s1 = fast_rcp(1.f + __builtin_amdgcn_exp2f(z1));
          const float a1 = s == 0 ? fmaf(s1, 2.f, -1.f) : s1;                         // g | o
          const float b0 = dpp_swap1(a0), b1 = dpp_swap1(a1);
          const float ig = s == 0 ? a0 : b0, fg = s == 0 ? b0 : a0;
          const float gg = s == 0 ? a1 : b1, og = s == 0 ? b1 : a1;
          const float cn = fmaf(fg, c[n], ig * gg);
          const float th = fmaf(fast_rcp(1.f + __builtin_amdgcn_exp2f(cn * (2.f * kNegLog2eK))), 2.f, -1.f);
          const float h = og * th;
          c[n] = cn;
          hl[n] = h;
          // lane 0: own-h slot of the next step; lane 1: the next layer's
          // input slot (top layer: its own slot again, same value)
          float* hslot = (s == 0 || layer == NL - 1) ? vin(n, layer, p ^ 1) + H + u : vin(n, layer + 1, p) + u;
          *hslot = h;
          const int64_t row = ((int64_t)layer * B + bbase + n) * T + t;
          float* act = a.act + row * 5 * H + u;
          act[(s == 0 ? 0 : 1) * H] = s == 0 ? ig : fg;
          act[(s == 0 ? 2 : 3) * H] = s == 0 ? gg : og;
          float* w3 = s == 0 ? act + 4 * H : a.hseq + row * H + u;
          *w3 = s == 0 ? cn : h;
          continue;
        }
        // (two sequences per workgroup, inference) the rows are pre-scaled
        // here too: acc = -log2(e) z, doubled for the g gate
        static_assert(S == 2, "the activations below expect the pre-scaled rows of the 2-lane map");
        const float ig = fast_rcp(1.f + __builtin_amdgcn_exp2f(acc[0]));
        const float fg = fast_rcp(1.f + __builtin_amdgcn_exp2f(acc[1]));
        const float gg = fmaf(fast_rcp(1.f + __builtin_amdgcn_exp2f(acc[2])), 2.f, -1.f);
        const float og = fast_rcp(1.f + __builtin_amdgcn_exp2f(acc[3]));
        const float cn = fmaf(fg, c[n], ig * gg);
        const float h = og * tanhf_fast(cn);
        c[n] = cn;
        hl[n] = h;
        if (s == 0) vin(n, layer, p ^ 1)[H + u] = h;
        if (layer < NL - 1 && s == (S > 1 ? 1 : 0)) vin(n, layer + 1, p)[u] = h;
        if (valid[n]) {
          const int b = bbase + n;
          if constexpr (SAVE) {
            const int64_t row = ((int64_t)layer * B + b) * T + t;
            if (s == 0) a.hseq[row * H + u] = h;
            float* act = a.act + row * 5 * H;
            const float items[5] = {ig, fg, gg, og, cn};
#pragma unroll
            for (int item = 0; item < 5; ++item)
              if (item % S == s) act[item * H + u] = items[item];
          } else {
            if (a.out && layer == NL - 1 && s == 0) a.out[b * a.o_sb + (int64_t)t * a.o_st + u] = h;
          }
        }
      }
      if (!XLDS && layer == 0 && lg < H) {
#pragma unroll
        for (int n = 0; n < NB; ++n) vin(n, 0, p ^ 1)[lg] = xnext[n];
      }
    }
    lds_barrier();
  }
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = stamp_real();
  }

#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    if (valid[n] && s == 0) {
      a.hn[((int64_t)layer * B + b) * H + u] = hl[n];
      a.cn[((int64_t)layer * B + b) * H + u] = c[n];
    }
  }
  if constexpr (HEAD) fwd_head_epilogue<H, NB>(a, smem, bbase);
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[4] = sr_in; st[5] = stamp_real(); st[6] = stamp_cu();
  }
  // the second wave's SIMD (bit 32 marks the slot as written)
  if (a.stamps && tid == 64) a.stamps[(uint64_t)blockIdx.x * 8 + 7] = stamp_cu() | (1ull << 32);
}

// ---------------------------------------------------------------------------
// Forward, gate-split lane map (default): a layer group is 4H lanes, lane =
// (unit u, gate q) with the 4 gates of a unit in one DPP quad.  Each lane owns
// ONE full row of [W_ih | W_hh] (pre-scaled by -log2(e), and by 2 for the g
// gate so tanh(x) = 2*sigmoid(2x) - 1), computes its dot product with packed
// fp32 FMAs (v_pk_fma_f32, 2 MACs per instruction), applies ONE transcendental
// activation, and the quad exchanges the four activated gates with DPP quad
// broadcasts.  Compared with the K-split map this removes the cross-lane
// partial-sum tree and three of the four activations from every lane's
// per-timestep dependency chain (the recurrence is latency-bound: one wave per
// SIMD at motion batch sizes).
// ---------------------------------------------------------------------------
constexpr float kNegLog2e = -1.4426950408889634f;

// CELL 1 = GRU on the same lane map: the quad's four rows are [r | z | n_x |
// n_h] (n_x = W_in x + b_in and n_h = W_hn h + b_hn kept linear), packed by the
// host as a 4-block stack with zero blocks (W_ih: [W_ir; W_iz; W_in; 0], W_hh:
// [W_hr; W_hz; 0; W_hn]); n = tanh(n_x + r n_h), h = n + z (h_prev - n).  The
// saved activation slots hold r, z, n_x, n_h and n (in the cell-state slot).
template <int H, int NB, bool SAVE, bool XLDS, bool HEAD, int CELL = 0>
// xs_off >= 0: x is staged at smem + xs_off (the one-launch step puts it
// where its backward half expects it, so the backward does not stage it again)
__device__ __forceinline__ void lstm_small_fwd_gs_body(const PdrnnLstmSmallFwdArgs& a, int xs_off = -1,
                                                       bool head_pre = false, float* dh_lds = nullptr) {
  constexpr int K = 2 * H;
  constexpr int LANES = 4 * H;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int NL = a.NL, B = a.B, T = a.T, I = a.I;
  const int tid = threadIdx.x;
  const uint64_t sr_in = (a.stamps && tid == 0) ? stamp_real() : 0;
  const int layer = __builtin_amdgcn_readfirstlane(tid / LANES);
  const int lg = tid - layer * LANES;
  const int u = lg >> 2;
  const int q = lg & 3;
  const int r = q * H + u;
  const int bbase = blockIdx.x * NB;
  const int Iin = layer == 0 ? I : H;

  float* xs = smem + (xs_off >= 0 ? xs_off : NB * NL * 2 * K);
  auto vin = [&](int n, int l, int p) -> float* { return smem + ((n * NL + l) * 2 + p) * K; };
  HeadPre hpre{};
  if constexpr (HEAD) {
    if (head_pre) hpre = head_prefetch<H, NB>(a, bbase);
  }

  // activation: sigma(z) with z pre-scaled, then a = sigma * am + ab
  // (GRU n_x / n_h rows stay linear: unscaled weights, activation skipped)
  const bool lin = CELL == 1 && q >= 2;
  const float gsc = (CELL == 0 && q == 2) ? 2.f : 1.f;
  const float am = gsc;
  const float ab = (CELL == 0 && q == 2) ? -1.f : 0.f;
  const float wsc = lin ? 1.f : kNegLog2e * gsc;

  pdrnn_f2 w2[K / 2];
  float bias;
  {
    const float* wih = a.w_ih[layer] + (int64_t)r * Iin;
    const float* whh = a.w_hh[layer] + (int64_t)r * H;
#pragma unroll
    for (int kk = 0; kk < K / 2; ++kk) {
      float v0, v1;
      const int k = 2 * kk;
      if (k < H) {  // compile-time per unrolled kk
        const float t0 = wih[min(k, Iin - 1)], t1 = wih[min(k + 1, Iin - 1)];
        v0 = k < Iin ? t0 : 0.f;
        v1 = k + 1 < Iin ? t1 : 0.f;
      } else {
        v0 = whh[k - H];
        v1 = whh[k + 1 - H];
      }
      w2[kk] = pdrnn_f2{wround(v0, a.w_bf16) * wsc, wround(v1, a.w_bf16) * wsc};
    }
    bias = ((a.b_ih[layer] ? wround(a.b_ih[layer][r], a.w_bf16) : 0.f) +
            (a.b_hh[layer] ? wround(a.b_hh[layer][r], a.w_bf16) : 0.f)) * wsc;
  }

  int bsrc[NB];
  bool valid[NB];
  float c[NB], hl[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    valid[n] = b < B;
    bsrc[n] = valid[n] ? (a.idx ? (int)a.idx[b] : b) : 0;
    const int bc = min(b, B - 1);
    const float h_init = (a.h0 && valid[n]) ? a.h0[((int64_t)layer * B + bc) * H + u] : 0.f;
    c[n] = (a.c0 && valid[n]) ? a.c0[((int64_t)layer * B + bc) * H + u] : 0.f;
    hl[n] = h_init;
    if (q == 0) vin(n, layer, 0)[H + u] = h_init;
    if (!XLDS && layer == 0 && lg < H)
      vin(n, 0, 0)[lg] = (valid[n] && lg < I) ? a.x[bsrc[n] * a.x_sb + lg] : 0.f;
  }
  if constexpr (XLDS) preload_x<H, NB>(xs, a, bsrc, valid);
  __syncthreads();

  // per-lane output streams (advanced by one timestep per active iteration)
  // lane q writes act item q (i,f,g,o); q==0 also writes c_t, q==1 writes h_t
  float* out1[NB];
  float* out2[NB];
  int64_t step1 = 0, step2 = 0;
  if constexpr (SAVE) {
    step1 = 5 * H;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int bc = min(bbase + n, B - 1);
      const int64_t row0 = ((int64_t)layer * B + bc) * T;
      out1[n] = a.act + row0 * 5 * H + q * H + u;
      out2[n] = q == 0 ? a.act + row0 * 5 * H + 4 * H + u : a.hseq + row0 * H + u;
    }
    step2 = q == 0 ? 5 * H : H;
  } else {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      out1[n] = a.out ? a.out + (int64_t)min(bbase + n, B - 1) * a.o_sb + u : nullptr;
      out2[n] = nullptr;
    }
    step1 = a.o_st;
  }
  const bool write2 = SAVE && q < 2;
  const bool write1 = SAVE || (a.out != nullptr && layer == NL - 1 && q == 0);

  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }
  const int iters = T + NL - 1;
  for (int it = 0; it < iters; ++it) {
    prio_by_progress(it, iters, a.prio);
    const int t = it - layer;
    if (t >= 0 && t < T) {
      const int p = t & 1;
      float xnext[NB];
      if (!XLDS && layer == 0 && lg < H) {
        const int tn = min(t + 1, T - 1);
        const int kx = min(lg, I - 1);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float v = a.x[bsrc[n] * a.x_sb + (int64_t)tn * a.x_st + kx];
          xnext[n] = (t + 1 < T && valid[n] && lg < I) ? v : 0.f;
        }
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const float* src_in = vin(n, layer, p);
        if (XLDS && layer == 0) src_in = xs + ((int64_t)n * T + t) * H;
        const float* src_h = vin(n, layer, p) + H;
        pdrnn_f2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        // the whole [x_t; h_{t-1}] operand vector in flight at once (one LDS
        // latency per step; left to itself the scheduler keeps 2-3 reads in
        // flight to save VGPRs and exposes the latency ~6 times per step)
        float4 vin4[K / 4];
#pragma unroll
        for (int k4 = 0; k4 < K / 4; ++k4)
          vin4[k4] = (4 * k4 < H) ? reinterpret_cast<const float4*>(src_in)[k4]
                                  : reinterpret_cast<const float4*>(src_h)[k4 - H / 4];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k4 = 0; k4 < K / 4; ++k4) {
          const float4 v = vin4[k4];
          acc[(2 * k4) & 3] = __builtin_elementwise_fma(w2[2 * k4], pdrnn_f2{v.x, v.y}, acc[(2 * k4) & 3]);
          acc[(2 * k4 + 1) & 3] =
              __builtin_elementwise_fma(w2[2 * k4 + 1], pdrnn_f2{v.z, v.w}, acc[(2 * k4 + 1) & 3]);
        }
        const pdrnn_f2 s2 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        const float z = (s2.x + s2.y) + bias;  // = -log2(e) * gsc * preactivation
        const float sg = fast_rcp(1.f + __builtin_amdgcn_exp2f(z));
        const float act = lin ? z : fmaf(sg, am, ab);  // sigmoid, or tanh for the g gate
        const float ig = quad_bcast(act, 0);
        const float fg = quad_bcast(act, 1);
        const float gg = quad_bcast(act, 2);
        const float og = quad_bcast(act, 3);
        float cn, h;
        if constexpr (CELL == 0) {
          cn = fmaf(fg, c[n], ig * gg);
          const float th = fmaf(fast_rcp(1.f + __builtin_amdgcn_exp2f(cn * (2.f * kNegLog2e))), 2.f, -1.f);
          h = og * th;
        } else {  // GRU: ig = r, fg = z, gg = n_x, og = n_h; cn carries n
          const float pre = fmaf(ig, og, gg);
          cn = fmaf(fast_rcp(1.f + __builtin_amdgcn_exp2f(pre * (2.f * kNegLog2e))), 2.f, -1.f);
          h = fmaf(fg, hl[n] - cn, cn);
        }
        c[n] = cn;
        hl[n] = h;
        if (q == 0) vin(n, layer, p ^ 1)[H + u] = h;
        if (q == 1 && layer < NL - 1) vin(n, layer + 1, p)[u] = h;
        if (valid[n]) {
          if (write1) out1[n][(int64_t)t * step1] = SAVE ? act : h;
          if (write2) out2[n][(int64_t)t * step2] = q == 0 ? cn : h;
        }
      }
      if (!XLDS && layer == 0 && lg < H) {
#pragma unroll
        for (int n = 0; n < NB; ++n) vin(n, 0, p ^ 1)[lg] = xnext[n];
      }
    }
    lds_barrier();
  }
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = stamp_real();
  }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    if (valid[n] && q == 0) {
      a.hn[((int64_t)layer * B + b) * H + u] = hl[n];
      if (CELL == 0) a.cn[((int64_t)layer * B + b) * H + u] = c[n];
    }
  }
  if constexpr (HEAD) fwd_head_epilogue<H, NB>(a, smem, bbase, head_pre ? &hpre : nullptr, dh_lds);
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[4] = sr_in; st[5] = stamp_real(); st[6] = stamp_cu();
  }
}

template <int H, int NB, bool SAVE, bool XLDS, bool HEAD, int CELL = 0>
__global__ void __launch_bounds__(512) lstm_small_fwd_gs_kernel(PdrnnLstmSmallFwdArgs a) {
  lstm_small_fwd_gs_body<H, NB, SAVE, XLDS, HEAD, CELL>(a);
}

template <int H, int S2, int NB, bool XLDS>
__global__ void __launch_bounds__(512) lstm_small_bwd_kernel(PdrnnLstmSmallBwdArgs a) {
  constexpr int R = 4 * H;        // gate rows
  constexpr int K = 2 * H;        // columns of [W_ih | W_hh] (input padded to H)
  constexpr int RS = R / S2;      // rows per column lane
  constexpr int G = K * S2;       // lanes per layer group
  constexpr int CH = 4;           // float4 chunks per LDS read burst (bounds VGPRs)
  static_assert(G >= R, "S2 must be >= 2");
  static_assert(RS % (4 * CH) == 0, "row slice must be a multiple of the chunk");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int NL = a.NL, B = a.B, T = a.T, I = a.I;
  const int tid = threadIdx.x;
  const int layer = __builtin_amdgcn_readfirstlane(tid / G);
  const int lg = tid - layer * G;
  const int bbase = blockIdx.x * NB;
  const int Iin = layer == 0 ? I : H;

  // LDS carve: dg[NB][NL][R] | dhrec[NB][NL][H] | dha[NB][NL][H] | xs[NB][T][H]
  float* dg_s = smem;
  float* dhrec_s = dg_s + NB * NL * R;
  float* dha_s = dhrec_s + NB * NL * H;
  float* xs = dha_s + NB * NL * H;
  auto dg = [&](int n, int l) { return dg_s + (n * NL + l) * R; };
  auto dhrec = [&](int n, int l) { return dhrec_s + (n * NL + l) * H; };
  auto dha = [&](int n, int l) { return dha_s + (n * NL + l) * H; };

  // Row role (lanes < 4H): gate row r = q*H + u.
  const bool is_row = lg < R;
  const int q = lg / H;
  const int u = lg % H;
  // Column role: column k of [W_ih | W_hh], row slice s2.
  const int k = lg / S2;
  const int s2 = lg % S2;

  // This lane's column: rows s2*RS .. s2*RS+RS-1 at a fixed stride
  // (branch-free addressing; zero-padded input columns k >= I).
  const bool col_in = k < H;
  const bool col_live = !col_in || k < Iin;
  const int64_t col_stride = col_in ? Iin : H;
  const int64_t col_off = col_in ? (int64_t)s2 * RS * Iin + k : (int64_t)s2 * RS * H + (k - H);
  float W[RS], dW[RS];
  {
    const float* base = (col_in ? a.w_ih[layer] : a.w_hh[layer]) + (col_live ? col_off : 0);
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      const float v = base[j * col_stride];
      W[j] = col_live ? wround(v, a.w_bf16) : 0.f;
      dW[j] = 0.f;
    }
  }
  float db = 0.f;
  float dc[NB];
  int bsrc[NB];
  bool valid[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    valid[n] = b < B;
    bsrc[n] = valid[n] ? (a.idx ? (int)a.idx[b] : b) : 0;
    const int bc = min(b, B - 1);
    dc[n] = (is_row && a.dcn && valid[n]) ? a.dcn[((int64_t)layer * B + bc) * H + u] : 0.f;
    if (lg < H) {
      dhrec(n, layer)[lg] = (a.dhn && valid[n]) ? a.dhn[((int64_t)layer * B + bc) * H + lg] : 0.f;
      dha(n, layer)[lg] = 0.f;
    }
  }
  if constexpr (XLDS) {
    for (int n = 0; n < NB; ++n) {
      float* dst = xs + (int64_t)n * T * H;
      const int64_t base = (int64_t)bsrc[n] * a.x_sb;
      for (int e = tid; e < T * H; e += blockDim.x) {
        const int t = e / H, kk = e - t * H;
        const float v = ldx(a.x, base + (int64_t)t * a.x_st + min(kk, I - 1), a.x_bf16);
        dst[e] = (valid[n] && kk < I) ? v : 0.f;
      }
    }
  }

  // ---- per-timestep operands, prefetched TWO steps ahead (ping-pong sets) --
  // Loads are unconditional on clamped, always-valid addresses and masked
  // afterwards: no control flow around them and no register copies between
  // iterations, so the compiler's waitcnt tracking keeps them in flight
  // across both barriers of the step in between.
  // Raw values only: masking happens at the point of use (a select on a
  // freshly loaded register would force the wait right at the load).
  struct RowOps { float i, f, g, o, c, cp, dout; };
  const bool top = layer == NL - 1;
  auto load_row = [&](int t, int n) {
    const int b = min(bbase + n, B - 1);
    const int tc = min(max(t, 0), T - 1);
    const float* act = a.act + (((int64_t)layer * B + b) * T + tc) * 5 * H + u;
    RowOps r;
    r.i = act[0 * H]; r.f = act[1 * H]; r.g = act[2 * H]; r.o = act[3 * H]; r.c = act[4 * H];
    const float* cpp = tc > 0 ? act - H : (a.c0 ? a.c0 + ((int64_t)layer * B + b) * H + u : act);
    r.cp = *cpp;
    const float* dp = (top && a.dout) ? a.dout + b * a.d_sb + (int64_t)tc * a.d_st + u : act;
    r.dout = *dp;
    return r;
  };
  // global part of the column input (everything except layer-0 x under XLDS)
  auto load_in = [&](int t, int n) -> float {
    const int b = min(bbase + n, B - 1);
    const int tc = min(max(t, 0), T - 1);
    const float* p;
    if (k < H) {
      const float* px = a.x + bsrc[n] * a.x_sb + (int64_t)tc * a.x_st + min(k, I - 1);
      const float* ph = a.hseq + (((int64_t)(layer > 0 ? layer - 1 : 0) * B + b) * T + tc) * H + k;
      p = layer == 0 ? px : ph;
    } else {
      const int kh = k - H;
      const float* ph = a.hseq + (((int64_t)layer * B + b) * T + max(tc - 1, 0)) * H + kh;
      const float* p0 = a.h0 ? a.h0 + ((int64_t)layer * B + b) * H + kh : ph;
      p = tc > 0 ? ph : p0;
    }
    return *p;
  };
  // masks, recomputed where the values are consumed
  auto in_live = [&](int t, int n) -> bool {
    if (!valid[n] || t < 0 || t >= T) return false;
    if (k < H) return layer > 0 || k < I;
    return t > 0 || a.h0 != nullptr;
  };
  const bool in_from_lds = XLDS && layer == 0 && k < H;

  const int t_first = T - 1 + (NL - 1 - layer);  // this layer's t at it = 0
  RowOps ropA[NB], ropB[NB];
  float inA[NB], inB[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    ropA[n] = load_row(t_first, n);
    inA[n] = load_in(t_first, n);
    ropB[n] = load_row(t_first - 1, n);
    inB[n] = load_in(t_first - 1, n);
  }
  __syncthreads();

  auto step = [&](int it, RowOps (&rop)[NB], float (&inp)[NB]) {
    const int t = t_first - it;
    const bool active = t >= 0 && t < T;
    // ---------------- row phase: dgates ----------------
    if (active && is_row) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const RowOps& r = rop[n];
        const float cp = (t > 0 || a.c0) ? r.cp : 0.f;
        float dh = dhrec(n, layer)[u] + ((top && a.dout) ? r.dout : 0.f);
        if (layer < NL - 1) dh += dha(n, layer)[u];
        const float tc = tanhf_fast(r.c);
        const float dcp = fmaf(dh * r.o, 1.f - tc * tc, dc[n]);
        const float d_i = dcp * r.g * r.i * (1.f - r.i);
        const float d_f = dcp * cp * r.f * (1.f - r.f);
        const float d_g = dcp * r.i * (1.f - r.g * r.g);
        const float d_o = dh * tc * r.o * (1.f - r.o);
        float dgv = q == 0 ? d_i : (q == 1 ? d_f : (q == 2 ? d_g : d_o));
        if (!valid[n]) dgv = 0.f;
        dc[n] = dcp * r.f;
        dg(n, layer)[lg] = dgv;
        db += dgv;
      }
    }
    // refill this set for step t-2 (consumed two iterations from now)
#pragma unroll
    for (int n = 0; n < NB; ++n) rop[n] = load_row(t - 2, n);
    lds_barrier();
    // ---------------- column phase: dh_{t-1}, d(input), dW ----------------
    if (active) {
      float in_v[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n)
        in_v[n] = in_from_lds ? xs[((int64_t)n * T + t) * H + k] : (in_live(t, n) ? inp[n] : 0.f);
      float ds[NB][4];  // 4 independent chains per sequence (FMA latency)
#pragma unroll
      for (int n = 0; n < NB; ++n) ds[n][0] = ds[n][1] = ds[n][2] = ds[n][3] = 0.f;
#pragma unroll
      for (int c0 = 0; c0 < RS / 4; c0 += CH) {
        float4 g[NB][CH];
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float4* g4 = reinterpret_cast<const float4*>(dg(n, layer) + s2 * RS);
#pragma unroll
          for (int cc = 0; cc < CH; ++cc) g[n][cc] = g4[c0 + cc];
        }
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) {
          const int j = 4 * (c0 + cc);
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            ds[n][0] = fmaf(W[j + 0], g[n][cc].x, ds[n][0]);
            ds[n][1] = fmaf(W[j + 1], g[n][cc].y, ds[n][1]);
            ds[n][2] = fmaf(W[j + 2], g[n][cc].z, ds[n][2]);
            ds[n][3] = fmaf(W[j + 3], g[n][cc].w, ds[n][3]);
            dW[j + 0] = fmaf(g[n][cc].x, in_v[n], dW[j + 0]);
            dW[j + 1] = fmaf(g[n][cc].y, in_v[n], dW[j + 1]);
            dW[j + 2] = fmaf(g[n][cc].z, in_v[n], dW[j + 2]);
            dW[j + 3] = fmaf(g[n][cc].w, in_v[n], dW[j + 3]);
          }
        }
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const float tot = group_sum<S2>((ds[n][0] + ds[n][1]) + (ds[n][2] + ds[n][3]));
        if (s2 == 0) {
          if (k >= H) {
            dhrec(n, layer)[k - H] = tot;
          } else if (layer > 0) {
            dha(n, layer - 1)[k] = tot;
          } else if (a.dx && valid[n] && k < I) {
            a.dx[(bbase + n) * a.dx_sb + (int64_t)t * a.dx_st + k] = tot;
          }
        }
      }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) inp[n] = in_from_lds ? 0.f : load_in(t - 2, n);
    lds_barrier();
  };

  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }
  const int iters = T + NL - 1;
  int it = 0;
  for (; it + 1 < iters; it += 2) {
    prio_by_progress(it / 2, iters / 2, a.prio);
    step(it, ropA, inA);
    step(it + 1, ropB, inB);
  }
  if (it < iters) step(it, ropA, inA);
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = stamp_real();
  }

  // ---------------- epilogue: initial-state grads + partial dW slab --------
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = bbase + n;
    if (!valid[n]) continue;
    if (a.dh0 && lg < H) a.dh0[((int64_t)layer * B + b) * H + lg] = dhrec(n, layer)[lg];
    if (a.dc0 && is_row && q == 0) a.dc0[((int64_t)layer * B + b) * H + u] = dc[n];
  }
  float* slab = a.slab + (int64_t)blockIdx.x * a.P;
  if (col_live) {
    float* dst = slab + (col_in ? a.off_wih[layer] : a.off_whh[layer]) + col_off;
#pragma unroll
    for (int j = 0; j < RS; ++j) dst[j * col_stride] = dW[j];
  }
  if (is_row) {
    if (a.off_bih[layer] >= 0) slab[a.off_bih[layer] + lg] = db;
    if (a.off_bhh[layer] >= 0) slab[a.off_bhh[layer] + lg] = db;
  }
}

// ---------------------------------------------------------------------------
// Backward, unit-group lane map (default): a layer group is H*L lanes, lane =
// (unit u, j) with the L lanes of a unit adjacent.  Lane j owns the row slice
// [j*RS, (j+1)*RS) (RS = 4H/L) of COLUMN u of both W_hh and W_ih, and the
// matching dW accumulators.  Per timestep:
//   row phase : lanes j<4 compute dgate_j[u] (the quad exchanges the saved
//               activations with DPP), publish it to LDS (parity buffer);
//   barrier   : the only one of the step;
//   col phase : every lane reads its RS dgates, forms partial
//               dh_{t-1}[u] = sum_r W_hh[r][u] dg[r] and d(input)[u], and
//               accumulates dW[r][u] += dg[r] * input; an L-lane DPP reduction
//               gives every lane of the group the full dh_{t-1}[u] -- kept in a
//               register for the next row phase (no LDS round trip, no second
//               barrier); d(input) goes to the layer below through a parity
//               buffer that it reads two iterations later (layer lag 2).
// Packed fp32 FMAs (v_pk_fma_f32) throughout.
// ---------------------------------------------------------------------------
// LEAN: the fused training-step configuration (zero initial states, loss only
// through h_T of the top layer, no dx / dh0 / dc0 outputs) with every optional
// operand folded away at compile time -- fewer live pointers and no per-step
// branches on the hot path.
// CELL 1 = GRU (packing as in the forward): the gate-gradient vector is
// [dr*r(1-r) | dz*z(1-z) | dpre_n | dpre_n*r] with dpre_n = dh (1-z) (1-n^2),
// so the column phase (W^T g, dW += g h^T / g x^T) is the LSTM's unchanged;
// the direct path dh_{t-1} += dh_t z rides in the dc register.
// W columns (u) of this lane's rows j*RS.. as float2 pairs along rows
// (W_hh and W_ih; W_ih columns past the layer input are zero).
template <int H, int L>
struct BwdCols {
  pdrnn_f2 whh[4 * H / L / 2], wih[4 * H / L / 2];
};
template <int H, int L>
__device__ __forceinline__ BwdCols<H, L> bwd_load_cols(const PdrnnLstmSmallBwdArgs& a) {
  constexpr int RS = 4 * H / L;
  constexpr int LANES = H * L;
  const int tid = threadIdx.x;
  const int layer = __builtin_amdgcn_readfirstlane(tid / LANES);
  const int lg = tid - layer * LANES;
  const int u = lg / L, j = lg % L;
  const int Iin = layer == 0 ? a.I : H;
  const int r0 = j * RS;
  const bool ih_live = u < Iin;
  BwdCols<H, L> w;
  const float* ph = a.w_hh[layer] + (int64_t)r0 * H + u;
  const float* pi = a.w_ih[layer] + (int64_t)r0 * Iin + min(u, Iin - 1);
#pragma unroll
  for (int rr = 0; rr < RS / 2; ++rr) {
    w.whh[rr] = pdrnn_f2{wround(ph[(2 * rr) * H], a.w_bf16), wround(ph[(2 * rr + 1) * H], a.w_bf16)};
    const float x0 = pi[(int64_t)(2 * rr) * Iin], x1 = pi[(int64_t)(2 * rr + 1) * Iin];
    w.wih[rr] = ih_live ? pdrnn_f2{wround(x0, a.w_bf16), wround(x1, a.w_bf16)} : pdrnn_f2{0.f, 0.f};
  }
  return w;
}

template <int H, int L, int NB, bool XLDS, bool LEAN, int CELL = 0, bool DWOUT = false>
// xs_off >= 0: x already staged at smem + xs_off by the forward half of the
// one-launch step (same layout, same workgroup): not loaded again.
// wpre: the W columns, loaded by the caller ahead of time (one-launch step:
// issued before the forward so their latency hides behind it).
// dh_lds: the top layer's dh_T of this workgroup's (single) sequence in LDS.
// DWOUT: no register-resident dW / db accumulators and no slab row; every
// step's gate gradients go to a.dg_out instead (one 4-byte store per row lane,
// overwriting the activation slot that lane has just consumed when dg_out ==
// act) and lstm_small_dw.hip forms the weight gradients on the matrix cores.
// The 64 accumulator VGPRs it frees raise the resident workgroups per CU
// (B = 1440: three residency rounds become two), and the per-step rank-1
// updates (~1/3 of a step's VALU issue) leave the recurrence's critical path.
__device__ __forceinline__ void lstm_small_bwd_gs_body(const PdrnnLstmSmallBwdArgs& a, int xs_off = -1,
                                                       const BwdCols<H, L>* wpre = nullptr,
                                                       const float* dh_lds = nullptr) {
  constexpr int R = 4 * H;
  constexpr int RS = R / L;          // rows per lane
  constexpr int LANES = H * L;
  static_assert(L >= 4 && RS % 4 == 0, "need >= 4 lanes per unit, float4 row slices");
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int NL = a.NL, B = a.B, T = a.T, I = a.I;
  const int tid = threadIdx.x;
  const uint64_t sr_in = (a.stamps && tid == 0) ? stamp_real() : 0;
  const int layer = __builtin_amdgcn_readfirstlane(tid / LANES);
  const int lg = tid - layer * LANES;
  const int u = lg / L;
  const int j = lg % L;
  const int q = j & 3;
  const bool rowlane = j < 4;
  const int Iin = layer == 0 ? I : H;
  const bool top = layer == NL - 1;
  const int lag = 2 * (NL - 1 - layer);
  const float* const h0p = LEAN ? nullptr : a.h0;
  const float* const c0p = LEAN ? nullptr : a.c0;
  const float* const doutp = LEAN ? nullptr : a.dout;
  const float* const dcnp = LEAN ? nullptr : a.dcn;
  float* const dxp = LEAN ? nullptr : a.dx;
  float* const dh0p = LEAN ? nullptr : a.dh0;
  float* const dc0p = LEAN ? nullptr : a.dc0;
  const bool top_only = LEAN ? true : a.dhn_top_only;

  // LDS: dg[NB][NL][2][RP] | dha[NB][NL][2][H] | xs[NB][T][H]
  // The gate-gradient vector is stored with a 4-float pad after every RS-row
  // slice: the L lanes of a unit read slices j*RS.. as float4s, and with an
  // unpadded RS = 32 slices j and j + 2 hit the same banks (2-way conflict,
  // ~150 cycles per step, profiles/r2_small_kernels_pmc.md).
  constexpr int RP = R + L * 4;
  float* dg_s = smem;
  float* dha_s = dg_s + NB * NL * 2 * RP;
  float* xs = xs_off >= 0 ? smem + xs_off : dha_s + NB * NL * 2 * H;
  auto dgbuf = [&](int n, int l, int p) { return dg_s + ((n * NL + l) * 2 + p) * RP; };
  auto dhabuf = [&](int n, int l, int p) { return dha_s + ((n * NL + l) * 2 + p) * H; };

  // ---- W columns (u) for rows j*RS.., as float2 pairs along rows ----------
  // Loaded ONCE and shared by the NB sequences a workgroup interleaves; the
  // grid is persistent over batch tiles (workgroup g handles tiles g, g+G, ...)
  // and the dW accumulators run across all of them, so a workgroup writes one
  // slab row however many sequences it processed.
  const int r0 = j * RS;
  const bool ih_live = u < Iin;
  float gm[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) gm[g] = q == g ? 1.f : 0.f;
  pdrnn_f2 whh[RS / 2], wih[RS / 2], dwhh[RS / 2], dwih[RS / 2];
  if (wpre) {
#pragma unroll
    for (int rr = 0; rr < RS / 2; ++rr) {
      whh[rr] = wpre->whh[rr];
      wih[rr] = wpre->wih[rr];
    }
  } else {
    const BwdCols<H, L> w = bwd_load_cols<H, L>(a);
#pragma unroll
    for (int rr = 0; rr < RS / 2; ++rr) {
      whh[rr] = w.whh[rr];
      wih[rr] = w.wih[rr];
    }
  }
#pragma unroll
  for (int rr = 0; rr < RS / 2; ++rr) {
    dwhh[rr] = pdrnn_f2{0.f, 0.f};
    dwih[rr] = pdrnn_f2{0.f, 0.f};
  }
  float db = 0.f;
  uint64_t st0 = 0, sr0 = 0;
  if (a.stamps && tid == 0) { st0 = stamp_cycles(); sr0 = stamp_real(); }

  struct Ops { float aq, ct, cp, dout, hprev, xin; };
  for (int b0 = blockIdx.x * NB; b0 < B; b0 += gridDim.x * NB) {
    int bs[NB], bsrc[NB];
    bool valid[NB];
    float dh[NB], dc[NB], dha_r[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      valid[n] = b0 + n < B;
      bs[n] = min(b0 + n, B - 1);  // invalid slots recompute the last sequence, never store
      bsrc[n] = a.idx ? (int)a.idx[bs[n]] : bs[n];
      dh[n] = 0.f;
      dha_r[n] = 0.f;
      if (dh_lds) {
        dh[n] = top ? dh_lds[u] : 0.f;
      } else if (a.dhn) {
        if (top_only) dh[n] = top ? a.dhn[(int64_t)bs[n] * H + u] : 0.f;
        else dh[n] = a.dhn[((int64_t)layer * B + bs[n]) * H + u];
      }
      dc[n] = dcnp ? dcnp[((int64_t)layer * B + bs[n]) * H + u] : 0.f;
      if (lg < H) {
        dhabuf(n, layer, 0)[lg] = 0.f;
        dhabuf(n, layer, 1)[lg] = 0.f;
      }
    }
    if constexpr (XLDS) {
      if (xs_off < 0) {
#pragma unroll
        for (int n = 0; n < NB; ++n)
          stage_x<H>(xs + (int64_t)n * T * H, a.x, (int64_t)bsrc[n] * a.x_sb, a.x_st, T, I, a.x_bf16, true,
                     (DWOUT && valid[n]) ? a.xg_out + (int64_t)bs[n] * T * a.xg_ld : nullptr, a.xg_ld);
      }
    }

    // ---- raw per-timestep operands (prefetched 2 steps ahead, masked at use)
    // Every stream is a buffer descriptor on a wave-uniform base (SGPRs), a
    // per-lane byte offset fixed for the whole loop (VGPR) and a per-step
    // scalar offset: one buffer_load per operand, no per-step VALU address
    // arithmetic.  Out-of-range steps are clamped, the values masked at use.
    // NB > 1 with x in LDS: the NB sequences of a tile are consecutive rows
    // (bs[n] >= bs[0]), so ONE descriptor per stream serves all of them and a
    // sequence's rows are a wave-uniform byte delta folded into the scalar
    // offset -- 4 SGPRs per stream instead of 4 NB (the paired-sequence BPTT
    // spilled SGPRs into VGPR lanes inside the recurrence)
    constexpr bool kShared = XLDS && NB > 1;
    constexpr int ND = kShared ? 1 : NB;
    __amdgpu_buffer_rsrc_t r_act[ND], r_own[ND], r_in[ND];
    uint32_t d_act[NB], d_h[NB], d_dg[NB];
    const int x_layer0 = layer == 0 && !XLDS;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const int64_t lb = (int64_t)layer * B + bs[n];
      r_act[n] = uniform_rsrc(a.act + lb * T * 5 * H);
      r_own[n] = uniform_rsrc(a.hseq + lb * T * H);
      r_in[n] = uniform_rsrc(x_layer0 ? a.x + (int64_t)bsrc[n] * a.x_sb
                                      : a.hseq + ((int64_t)(layer > 0 ? layer - 1 : 0) * B + bs[n]) * T * H);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const uint32_t dn = kShared ? (uint32_t)(bs[n] - bs[0]) * (uint32_t)T : 0u;
      d_act[n] = __builtin_amdgcn_readfirstlane(dn * 5u * H * 4u);
      d_h[n] = __builtin_amdgcn_readfirstlane(dn * (uint32_t)H * 4u);
      d_dg[n] = DWOUT ? __builtin_amdgcn_readfirstlane(dn * (uint32_t)a.dg_st * 4u) : 0u;
    }
    const bool has_dout = top && doutp != nullptr;
    // deferred dW: this row's gate-gradient stream (same row layout as act)
    __amdgpu_buffer_rsrc_t r_dg[ND];
    uint32_t st_dg = 0;
    if constexpr (DWOUT) {
      st_dg = (uint32_t)a.dg_st * 4;
#pragma unroll
      for (int n = 0; n < ND; ++n) r_dg[n] = uniform_rsrc(a.dg_out + ((int64_t)layer * B + bs[n]) * T * a.dg_st);
    }
    const uint32_t vo_q = (q * H + u) * 4, vo_c = (4 * H + u) * 4, vo_u = u * 4;
    const uint32_t vo_x = (x_layer0 ? min(u, I - 1) : u) * 4;
    const uint32_t st_act = 5 * H * 4, st_h = H * 4;
    const uint32_t st_x = x_layer0 ? (uint32_t)a.x_st * 4 : st_h;
    // Branch-free: every operand is loaded every step and masked at use.  A
    // load under a branch makes the waitcnt pass fall back to vmcnt(0) at the
    // join, which would wait for the prefetches issued for later steps too.
    auto load_ops = [&](int n, int t) {
      // scalar offsets (readfirstlane: provably uniform -> SGPR soffset, no waterfall)
      const uint32_t tc = __builtin_amdgcn_readfirstlane((uint32_t)min(max(t, 0), T - 1));
      const uint32_t tp = tc > 0 ? tc - 1 : 0;
      const uint32_t so_a = __builtin_amdgcn_readfirstlane(tc * st_act);
      const uint32_t so_ap = __builtin_amdgcn_readfirstlane(tp * st_act);
      const uint32_t so_h = __builtin_amdgcn_readfirstlane(tp * st_h);
      const uint32_t so_x = __builtin_amdgcn_readfirstlane(tc * st_x);
      Ops o;
      const int nd = kShared ? 0 : n;
      o.aq = bload(r_act[nd], vo_q, so_a + d_act[n]);
      o.ct = bload(r_act[nd], vo_c, so_a + d_act[n]);
      o.cp = bload(r_act[nd], vo_c, so_ap + d_act[n]);
      // optional operands (generic kernel only): descriptors built on demand
      // to keep the SGPR budget of the hot loop
      const int64_t lb = (int64_t)layer * B + bs[n];
      if (c0p && tc == 0) o.cp = bload(uniform_rsrc(c0p + lb * H), vo_u, 0);
      o.dout = has_dout ? bload(uniform_rsrc(doutp + bs[n] * a.d_sb), vo_u,
                                __builtin_amdgcn_readfirstlane(tc * (uint32_t)a.d_st * 4))
                        : 0.f;
      o.hprev = bload(r_own[nd], vo_u, so_h + d_h[n]);
      if (h0p && tc == 0) o.hprev = bload(uniform_rsrc(h0p + lb * H), vo_u, 0);
      o.xin = bload(r_in[nd], vo_x, so_x + (x_layer0 ? 0u : d_h[n]));
      return o;
    };

    const int t_first = T - 1 + lag;
    Ops opA[NB], opB[NB];
    // issue order pinned (A's loads, then B's): the loop's counted vmcnt waits
    // are the max over its entry edges, so a reordered prologue would make
    // every in-loop wait conservative
#pragma unroll
    for (int n = 0; n < NB; ++n) opA[n] = load_ops(n, t_first);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NB; ++n) opB[n] = load_ops(n, t_first - 1);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // The step body is branch-free (inactive steps compute and mask): a branch
    // join makes the waitcnt pass conservative, and every conservative
    // vmcnt here would wait for the prefetches of the next two steps.
    const int dha_tgt = layer > 0 ? layer - 1 : NL - 1;  // top layer's dha slots are never read
    // the lean contract wants no input gradient: layer 0 skips W_ih^T g (a
    // quarter to a half of its column-phase FMAs) -- unless the dW updates
    // still need the column loop's operands (they do not depend on it)
    const bool need_dx = !LEAN || layer > 0;
    auto step = [&](int it, Ops* op) {
      const int t = t_first - it;
      const bool active = t >= 0 && t < T;
      const int p = it & 1;
      // ---------------- row phase ----------------
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float dht = dh[n] + (has_dout ? op[n].dout : 0.f);
        if (!top) dht += dha_r[n];  // dh from the layer above (prefetched, see the column phase)
        const float ig = quad_bcast(op[n].aq, 0), fg = quad_bcast(op[n].aq, 1);
        const float gg = quad_bcast(op[n].aq, 2), og = quad_bcast(op[n].aq, 3);
        // this lane's gate gradient by arithmetic with 0/1 lane masks
        // (gm[q] = [q == lane's gate]): a select chain over q compiles into
        // divergent exec-masked branches inside the recurrence
        const float own = op[n].aq;
        float dgv, dcn;
        if constexpr (CELL == 0) {
          const float cp = (t > 0 || c0p) ? op[n].cp : 0.f;
          const float tc = tanhf_fast(op[n].ct);
          const float dcp = fmaf(dht * og, 1.f - tc * tc, dc[n]);
          // i: dcp gg s'(i)  f: dcp cp s'(f)  g: dcp ig t'(g)  o: dht tc s'(o)
          const float oth = fmaf(gm[0], gg, fmaf(gm[1], cp, fmaf(gm[2], ig, gm[3] * tc)));
          const float src = fmaf(gm[3], dht - dcp, dcp);
          const float der = fmaf(gm[2], 1.f - own, own) - own * own;
          dgv = src * oth * der;
          dcn = dcp * fg;
        } else {  // GRU: ig = r, fg = z, og = n_h, ct = n
          const float hp = (t > 0 || h0p) ? op[n].hprev : 0.f;
          const float nn = op[n].ct;
          const float dpn = dht * (1.f - fg) * (1.f - nn * nn);
          // r: dpn n_h s'(r)  z: dht (h - n) s'(z)  n_x: dpn  n_h: dpn r
          const float a0 = fmaf(gm[1], dht - dpn, dpn);
          const float a1 = fmaf(gm[0], og, fmaf(gm[1], hp - nn, fmaf(gm[3], ig, gm[2])));
          const float a2 = fmaf(gm[0] + gm[1], own - own * own - 1.f, 1.f);
          dgv = a0 * a1 * a2;
          dcn = dht * fg;  // direct path into dh_{t-1}
        }
        dgv = active ? dgv : 0.f;  // inactive: zero gate gradients (dW, db, dh unaffected)
        dc[n] = active ? dcn : dc[n];
        if (L == 4 || rowlane) {
          dgbuf(n, layer, p)[q * H + u + ((q * H + u) / RS) * 4] = dgv;
          if constexpr (!DWOUT) db += valid[n] ? dgv : 0.f;
        }
        if constexpr (DWOUT) {
          // branch-free: a step outside [0, T), an unused batch slot or a
          // duplicate lane (L = 8) stores out of the buffer's range, which the
          // hardware drops (a branch around it would make the loop's vmcnt
          // waits conservative, see load_ops)
          const bool st_ok = active && valid[n] && (L == 4 || rowlane);
          const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)min(max(t, 0), T - 1) * st_dg);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, dgv), r_dg[kShared ? 0 : n],
                                                st_ok ? vo_q : 0x80000000u, so + d_dg[n], 0);
        }
      }
      lds_barrier();
      // ---------------- column phase ----------------
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const float hprev = (t > 0 || h0p) ? op[n].hprev : 0.f;
        // both candidates live at once (a select, not a branch): otherwise the
        // LDS read reuses the prefetch register and waits on in-flight loads
        const int tcl = min(max(t, 0), T - 1);
        const float xsv = XLDS ? xs[((int64_t)n * T + tcl) * H + u] : 0.f;
        const float xgv = (layer > 0 || u < I) ? op[n].xin : 0.f;
        const float xin = (XLDS && layer == 0) ? xsv : xgv;
        // an invalid slot still runs the recurrence but contributes nothing to dW
        const float hw = valid[n] ? hprev : 0.f, xw = valid[n] ? xin : 0.f;
        const float4* g4 = reinterpret_cast<const float4*>(dgbuf(n, layer, p) + r0 + j * 4);
        // all of this lane's gate-gradient slice in flight at once: one
        // LDS latency per step instead of one per read batch
        float4 gv[RS / 4];
#pragma unroll
        for (int r4 = 0; r4 < RS / 4; ++r4) gv[r4] = g4[r4];
        __builtin_amdgcn_sched_barrier(0);
        pdrnn_f2 sh[2] = {{0.f, 0.f}, {0.f, 0.f}}, sx[2] = {{0.f, 0.f}, {0.f, 0.f}};
        const pdrnn_f2 hb = {hw, opaque_copy(hw)}, xb = {xw, opaque_copy(xw)};
#pragma unroll
        for (int r4 = 0; r4 < RS / 4; ++r4) {
          const float4 g = gv[r4];
          const pdrnn_f2 g01 = {g.x, g.y}, g23 = {g.z, g.w};
          sh[0] = __builtin_elementwise_fma(whh[2 * r4], g01, sh[0]);
          sh[1] = __builtin_elementwise_fma(whh[2 * r4 + 1], g23, sh[1]);
          if (need_dx) {  // wave-uniform (one layer per wave); no loads inside
            sx[0] = __builtin_elementwise_fma(wih[2 * r4], g01, sx[0]);
            sx[1] = __builtin_elementwise_fma(wih[2 * r4 + 1], g23, sx[1]);
          }
          if constexpr (!DWOUT) {
            dwhh[2 * r4] = __builtin_elementwise_fma(g01, hb, dwhh[2 * r4]);
            dwhh[2 * r4 + 1] = __builtin_elementwise_fma(g23, hb, dwhh[2 * r4 + 1]);
            dwih[2 * r4] = __builtin_elementwise_fma(g01, xb, dwih[2 * r4]);
            dwih[2 * r4 + 1] = __builtin_elementwise_fma(g23, xb, dwih[2 * r4 + 1]);
          }
        }
        // pin this step's dW updates here: they feed nothing until the
        // epilogue, and left free the scheduler sinks them into the next
        // step (keeping this step's gate-gradient slice live across it)
        if constexpr (!DWOUT) {
#pragma unroll
          for (int rr = 0; rr < RS / 2; ++rr) asm volatile("" : "+v"(dwhh[rr]), "+v"(dwih[rr]));
        }
        const pdrnn_f2 shs = sh[0] + sh[1], sxs = sx[0] + sx[1];
        float dhn_ = group_sum<L>(shs.x + shs.y);  // dh_{t-1}[u] on every lane of the unit
        if constexpr (CELL == 1) dhn_ += dc[n];
        dh[n] = active ? dhn_ : dh[n];
        if (need_dx) {
          const float dx = group_sum<L>(sxs.x + sxs.y);
          // every lane of the unit holds dx: all write the same value (no
          // branch); consumed by layer-1 at it+2 (same parity)
          dhabuf(n, dha_tgt, p)[u] = dx;
          if (!LEAN && layer == 0 && dxp && active && j == 0 && u < I && valid[n])
            dxp[bs[n] * a.dx_sb + (int64_t)t * a.dx_st + u] = dx;
        }
      }
      // dh the layer above wrote for the NEXT iteration (its column phase of
      // it-1, published by this iteration's barrier): read now, off the next
      // row phase's critical path.  Its next overwrite is after the next barrier.
      if (!top) {
#pragma unroll
        for (int n = 0; n < NB; ++n) dha_r[n] = dhabuf(n, layer, (it + 1) & 1)[u];
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        op[n] = load_ops(n, t - 2);  // refill for two steps ahead
      }
    };

    const int iters = T + 2 * (NL - 1);
    // progress over all of this workgroup's tiles, in step pairs
    const int tiles = (B - (int)blockIdx.x * NB + (int)gridDim.x * NB - 1) / ((int)gridDim.x * NB);
    const int tile = (b0 - (int)blockIdx.x * NB) / ((int)gridDim.x * NB);
    const int hp = (iters + 1) / 2;
    int it = 0;
    for (; it + 1 < iters; it += 2) {
      prio_by_progress(tile * hp + it / 2, tiles * hp, a.prio);
      step(it, opA);
      step(it + 1, opB);
    }
    if (it < iters) step(it, opA);

    if (j == 0) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        if (!valid[n]) continue;
        if (dh0p) dh0p[((int64_t)layer * B + bs[n]) * H + u] = dh[n];
        if (CELL == 0 && dc0p) dc0p[((int64_t)layer * B + bs[n]) * H + u] = dc[n];
      }
    }
    __syncthreads();  // LDS is reused by the next tile
  }
  if (a.stamps && tid == 0) {
    uint64_t* st = a.stamps + (uint64_t)blockIdx.x * 8;
    st[0] = st0; st[1] = stamp_cycles(); st[2] = sr0; st[3] = stamp_real();
    st[4] = sr_in; st[5] = st[3]; st[6] = stamp_cu();
  }

  // ---------------- epilogue: this workgroup's partial dW / db ----------
  if constexpr (DWOUT) {
    // the dW kernel streams whole stages: the PDRNN_DW_PAD_ROWS padding rows
    // behind the last layer's gate gradients must hold finite values (masked
    // operands are multiplied by zero there, and NaN * 0 = NaN)
    if (blockIdx.x == 0) {
      float* pad = a.dg_out + (int64_t)NL * B * T * a.dg_st;
      for (int e = threadIdx.x; e < PDRNN_DW_PAD_ROWS * a.dg_st; e += blockDim.x) pad[e] = 0.f;
    }
    return;
  }
  float* slab = a.slab + (int64_t)blockIdx.x * a.P;
  {
    float* dst = slab + a.off_whh[layer] + (int64_t)r0 * H + u;
#pragma unroll
    for (int rr = 0; rr < RS / 2; ++rr) {
      dst[(2 * rr) * H] = dwhh[rr].x;
      dst[(2 * rr + 1) * H] = dwhh[rr].y;
    }
  }
  if (ih_live) {
    float* dst = slab + a.off_wih[layer] + (int64_t)r0 * Iin + u;
#pragma unroll
    for (int rr = 0; rr < RS / 2; ++rr) {
      dst[(int64_t)(2 * rr) * Iin] = dwih[rr].x;
      dst[(int64_t)(2 * rr + 1) * Iin] = dwih[rr].y;
    }
  }
  if (rowlane) {
    if (a.off_bih[layer] >= 0) slab[a.off_bih[layer] + q * H + u] = db;
    if (a.off_bhh[layer] >= 0) slab[a.off_bhh[layer] + q * H + u] = db;
  }
}

template <int H, int L, int NB, bool XLDS, bool LEAN, int CELL = 0>
__global__ void __launch_bounds__(512) lstm_small_bwd_gs_kernel(PdrnnLstmSmallBwdArgs a) {
  lstm_small_bwd_gs_body<H, L, NB, XLDS, LEAN, CELL>(a);
}

// Lean BPTT with the weight gradients deferred to lstm_small_dw.hip.
// NB = 2: two sequences per workgroup share the register-resident W columns
// (64 of the ~147 VGPRs of a lane), so a workgroup carries twice the batch at
// about the same register cost: B = 1440 (1152) fits ONE residency round of
// 720 (576) workgroups at 3 waves per SIMD instead of two rounds of one
// sequence each -- the recurrence's 130 dependent steps are paid once, each
// step issuing both sequences' independent chains.
template <int H, int L, int NB, bool XLDS, int CELL>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NB > 1 ? 3 : 1)))
lstm_small_bwd_dwout_kernel(PdrnnLstmSmallBwdArgs a) {
  lstm_small_bwd_gs_body<H, L, NB, XLDS, true, CELL, true>(a);
}

// ---------------------------------------------------------------------------
// Whole training step of the latency regime in ONE launch: when the backward
// grid is one sequence per workgroup (B <= resident workgroups) and both maps
// use the same NL*4H lanes (gate-split forward, L = 4 unit-group backward),
// workgroup b runs sequence b's forward + head/CE epilogue and then its own
// BPTT.  Every operand the backward reads (saved activations, h sequence,
// dh_T) was written by this workgroup, so no grid-wide dependency exists: the
// kernel boundary between the two launches (tail of the slowest forward
// workgroup + the backward's launch and wave start) disappears, and each
// workgroup goes straight from its forward into its backward.
// ---------------------------------------------------------------------------
template <int H, bool XLDS, int CELL>
__global__ void __launch_bounds__(512) lstm_small_step_gs_kernel(PdrnnLstmSmallFwdArgs f, PdrnnLstmSmallBwdArgs b) {
  extern __shared__ __attribute__((aligned(16))) float smem_step[];
  static_assert(H <= 32, "dh_T slot must fit the L = 8 padding slack (NL * 2 * 16 floats >= H)");
  // x staged once, past the backward's gate-gradient / dh buffers (the larger
  // of the two halves' operand areas, bwd_gs_lds<H, 1> with L = 4 lanes)
  const int xs_off = XLDS ? f.NL * 2 * (4 * H + 4 * 4 + H) : -1;
  // the backward's W columns and the head's label / weights are issued now:
  // their latency hides behind the forward recurrence (registers are free --
  // the backward half sets the kernel's VGPR budget)
  const BwdCols<H, 4> wcols = bwd_load_cols<H, 4>(b);
  // dh_T slot: the launch's LDS slack past x (bwd_gs_lds pads for L = 8)
  float* dh_lds = XLDS ? smem_step + xs_off + f.T * H : nullptr;
  lstm_small_fwd_gs_body<H, 1, true, XLDS, true, CELL>(f, xs_off, true, dh_lds);
  // this workgroup's global stores (activations, h, dh_T) before its own
  // backward loads them: a workgroup-scope release/acquire (the barrier's
  // own fences) is enough -- every wave of the workgroup shares the CU's
  // L1, which holds no line of these buffers (the forward never loads them,
  // and the L1 is invalidated at kernel start).  An agent-scope fence here
  // would write back the XCD's L2 (measured: +6 us/step at B = 180).  The
  // LDS operand buffers are reused by the backward.
  __syncthreads();
  lstm_small_bwd_gs_body<H, 4, 1, XLDS, true, CELL>(b, xs_off, &wcols, dh_lds);
}

// ---- Host side -------------------------------------------------------------
// Every kernel family has ONE function (<family>_kernel) that maps the runtime
// flags of a launch to its instantiation -- entry point, sequences per
// workgroup, block size, dynamic LDS -- and launch() / resident() work on that,
// so a launcher and its grid query cannot disagree.  with_int / with_bools turn
// runtime values into integral_constants; `if constexpr` in the family
// functions keeps the instantiated set to what is dispatched.
struct Kernel { const void* fn; int nb, block; size_t lds; hipError_t err; };  // nb: sequences per workgroup
inline Kernel no_kernel(hipError_t e) { return {nullptr, 1, 0, 0, e}; }
template <class K>
Kernel kernel(K* fn, int nb, int block, size_t lds) { return {(const void*)fn, nb, block, lds, hipSuccess}; }

// f(integral_constant<int, N>) for the N of Ns that equals v, else `miss`
template <int... Ns, class R, class F>
R with_int(int v, R miss, F&& f) {
  (void)((v == Ns && (miss = f(std::integral_constant<int, Ns>{}), true)) || ...);
  return miss;
}
// f(bool_constant...) for the given runtime flags, in order
template <class F> auto with_bools(F&& f) { return f(); }
template <class F, class... Rest>
auto with_bools(F&& f, bool flag, Rest... rest) {
  auto on = [&](auto... c) { return f(std::true_type{}, c...); };
  auto off = [&](auto... c) { return f(std::false_type{}, c...); };
  return flag ? with_bools(on, rest...) : with_bools(off, rest...);
}

// ... and f(integral_constant<int, H>) for the hidden sizes the kernels are built for
template <class R, class F> R with_hidden(int H, R miss, F&& f) { return with_int<16, 32, 64>(H, miss, f); }

template <class... Args>
hipError_t launch(const Kernel& k, int grid, hipStream_t st, const Args*... args) {
  if (k.err != hipSuccess) return k.err;
  void* argv[] = {const_cast<Args*>(args)...};
  (void)hipLaunchKernel(k.fn, dim3(grid), dim3(k.block), argv, k.lds, st);
  return hipGetLastError();
}

// Workgroups of a kernel that can be resident on the current device (occupancy
// query x CU count).  The query costs a driver round trip: cached per thread.
int resident(const Kernel& k) {
  struct Entry { const void* fn; int dev, block; size_t lds; int val; };
  static thread_local std::vector<Entry> cache;
  int per_cu = 0, cus = 0, dev = 0;
  (void)hipGetDevice(&dev);
  for (const Entry& e : cache)
    if (e.fn == k.fn && e.dev == dev && e.block == k.block && e.lds == k.lds) return e.val;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, k.block, k.lds);
  const int val = (per_cu < 1 ? 1 : per_cu) * (cus < 1 ? 1 : cus);
  if (cache.size() >= 64) cache.clear();  // (sequence lengths come and go)
  cache.push_back({k.fn, dev, k.block, k.lds, val});
  return val;
}

inline int tiles(int B, int nb) { return (B + nb - 1) / nb; }
// Persistent grid of the backward: resident workgroups, capped by the batch tiles.
int persistent_grid(const Kernel& k, int B) {
  if (k.err != hipSuccess) return -1;
  const int t = tiles(B, k.nb), cap = resident(k);
  return t < cap ? t : cap;
}

// Dynamic LDS: the operand buffers of nb sequences, plus their x image when it fits.
inline size_t x_bytes(int H, int nb, int T) { return sizeof(float) * (size_t)nb * T * H; }
inline bool x_in_lds(int H, int nb, int T) { return x_bytes(H, nb, T) <= (size_t)kXldsBytes; }
inline size_t with_x(size_t lds, int H, int nb, int T) { return lds + (x_in_lds(H, nb, T) ? x_bytes(H, nb, T) : 0); }
inline size_t fwd_lds(int H, int nb, int NL) { return sizeof(float) * nb * NL * 2 * (2 * H); }
// (dg slices padded by 4 floats per lane slice, L <= 8 lanes per unit)
inline size_t bwd_gs_lds(int H, int nb, int NL) { return sizeof(float) * nb * NL * 2 * (4 * H + 8 * 4 + H); }

// lanes per hidden unit of the unit-group backward (row slices of 4H / L = 32 at H = 64)
template <int H> constexpr int kUnitLanes = H == 64 ? 8 : 4;

// Forward.  split 1: gate-split map (4 lanes per unit, one gate each), LSTM and
// GRU.  split 2: 2-lane K-split map, LSTM only; its 2H lanes per layer must
// fill whole waves (H >= 32).  K splits of 4 / 8 lanes per unit are never the
// widest valid map (a stack that fits them fits the gate-split map) and are not
// built.  1 or 2 sequences per workgroup; workgroups of at most 512 lanes (the
// launch bound keeps 256 VGPRs per lane available).  HEAD (with SAVE only): the
// fused training step's classifier head + CE epilogue.
template <int H>
Kernel fwd_kernel(const PdrnnLstmSmallFwdArgs* a, int nb, int split, bool save) {
  const bool gru = a->cell == 1, head = save && a->head_w;
  if (gru && split != 1) return no_kernel(hipErrorInvalidConfiguration);
  if ((split != 1 && split != 2) || (split == 2 && H < 32)) return no_kernel(hipErrorInvalidValue);
  const int block = a->NL * H * (split == 1 ? 4 : 2);
  if (block > 512) return no_kernel(hipErrorInvalidConfiguration);
  if ((gru && a->head_w && !save) || (head && a->C > 16)) return no_kernel(hipErrorInvalidValue);
  if (split == 1) nb = nb == 2 ? 2 : 1;
  return with_int<1, 2>(nb, no_kernel(hipErrorInvalidValue), [&](auto nb_c) {
    constexpr int NB = decltype(nb_c)::value;
    const size_t lds = with_x(fwd_lds(H, NB, a->NL), H, NB, a->T);
    return with_bools([&](auto SAVE, auto XLDS, auto HEAD, auto GRU, auto KSPLIT) {
      if constexpr ((HEAD && !SAVE) || (KSPLIT && (GRU || H < 32))) return no_kernel(hipErrorInvalidValue);
      else if constexpr (KSPLIT) return kernel(lstm_small_fwd_kernel<H, 2, NB, SAVE, XLDS, HEAD>, NB, block, lds);
      else return kernel(lstm_small_fwd_gs_kernel<H, NB, SAVE, XLDS, HEAD, GRU ? 1 : 0>, NB, block, lds);
    }, save, x_in_lds(H, NB, a->T), head, gru, split == 2);
  });
}

// the fused training step's backward contract: zero initial state, loss through h_T only
inline bool bwd_lean(const PdrnnLstmSmallBwdArgs* a) {
  return !a->h0 && !a->c0 && !a->dout && !a->dcn && !a->dx && !a->dh0 && !a->dc0 && a->dhn && a->dhn_top_only;
}

// Unit-group backward with register-resident dW: 1..3 sequences per workgroup
// for the LSTM at H <= 32, one at H = 64 and for the GRU.
template <int H>
Kernel bwd_gs_kernel(int cell, int nb, int NL, int T, bool lean) {
  constexpr int L = kUnitLanes<H>;
  if (NL * H * L > 512) return no_kernel(hipErrorInvalidConfiguration);
  return with_int<1, 2, 3>(nb, no_kernel(hipErrorInvalidConfiguration), [&](auto nb_c) {
    constexpr int NB = decltype(nb_c)::value;
    return with_bools([&](auto XLDS, auto LEAN, auto GRU) {
      if constexpr (NB > 1 && (GRU || H == 64)) return no_kernel(hipErrorInvalidConfiguration);
      else return kernel(lstm_small_bwd_gs_kernel<H, L, NB, XLDS, LEAN, GRU ? 1 : 0>, NB, NL * H * L,
                         with_x(bwd_gs_lds(H, NB, NL), H, NB, T));
    }, x_in_lds(H, NB, T), lean, cell == 1);
  });
}

// Row/column-split backward (split 2: 4H lanes per layer, one sequence per
// workgroup; the 4-slice row split is not built: a stack that fits it fits
// the unit-group map).
template <int H>
Kernel bwd_rowsplit_kernel(int nb, int NL, int T) {
  if (NL * 4 * H > 512) return no_kernel(hipErrorInvalidConfiguration);
  if (nb != 1) return no_kernel(hipErrorInvalidValue);
  return with_bools([&](auto XLDS) {
    return kernel(lstm_small_bwd_kernel<H, 2, 1, XLDS>, 1, NL * 4 * H, with_x(sizeof(float) * NL * 6 * H, H, 1, T));
  }, x_in_lds(H, 1, T));
}

template <int H>
hipError_t launch_bwd(const PdrnnLstmSmallBwdArgs* a, int nb, int split, int grid, hipStream_t st) {
  if (a->cell == 1 && (split != 1 || nb != 1)) return hipErrorInvalidConfiguration;
  if (split != 1 && split != 2) return hipErrorInvalidValue;
  const Kernel k = split == 1 ? bwd_gs_kernel<H>(a->cell, nb, a->NL, a->T, bwd_lean(a))
                              : bwd_rowsplit_kernel<H>(nb, a->NL, a->T);
  if (split == 2) grid = tiles(a->B, 1);
  return launch(k, grid > 0 ? grid : persistent_grid(k, a->B), st, a);
}

// One-launch step (H <= 32): gate-split forward + head/CE + L = 4 unit-group
// backward of sequence b in workgroup b.
template <int H>
hipError_t launch_step(const PdrnnLstmSmallFwdArgs* f, const PdrnnLstmSmallBwdArgs* b, hipStream_t st) {
  if (f->NL * 4 * H > 512 || f->B != b->B || f->T != b->T || f->NL != b->NL) return hipErrorInvalidConfiguration;
  if (!f->head_w || f->C > 16 || !bwd_lean(b)) return hipErrorInvalidValue;
  const size_t lds_f = fwd_lds(H, 1, f->NL), lds_b = bwd_gs_lds(H, 1, f->NL);
  const Kernel k = with_bools([&](auto XLDS, auto GRU) {
    return kernel(lstm_small_step_gs_kernel<H, XLDS, GRU ? 1 : 0>, 1, f->NL * 4 * H,  // = NL * H * L with L = 4
                  with_x(lds_f > lds_b ? lds_f : lds_b, H, 1, f->T));
  }, x_in_lds(H, 1, f->T), f->cell == 1);
  return launch(k, f->B, st, f, b);
}

// Deferred-dW backward (DWOUT).  The instantiations without the LDS x image,
// and H = 64 with two sequences, serve the residency queries only: the launch
// refuses them.
template <int H>
Kernel dwout_kernel(int cell, int nb, int NL, int T) {
  return with_int<1, 2>(nb, no_kernel(hipErrorInvalidValue), [&](auto nb_c) {
    constexpr int NB = decltype(nb_c)::value, L = kUnitLanes<H>;
    return with_bools([&](auto XLDS, auto GRU) {
      return kernel(lstm_small_bwd_dwout_kernel<H, L, NB, XLDS, GRU ? 1 : 0>, NB, NL * H * L,
                    with_x(bwd_gs_lds(H, NB, NL), H, NB, T));
    }, x_in_lds(H, NB, T), cell == 1);
  });
}

// Sequences per workgroup of the deferred-dW backward: 2 when pairing the
// sequences takes fewer residency rounds than one per workgroup (B = 1152 /
// 1440 at H = 32: one round instead of two), else 1.  PDRNN_TUNE dwout_nb=1|2
// forces one (A/B measurements).
template <int H>
int bwd_dwout_nb(int NL, int T, int B, int cell) {
  const int env = pdrnn_tune_int("dwout_nb", 0);  // per call: tests flip it in-process
  if (env == 1 || env == 2) return env;
  if (H > 32 || NL * H * kUnitLanes<H> > 512) return 1;
  const int cap1 = resident(dwout_kernel<H>(cell, 1, NL, T)), cap2 = resident(dwout_kernel<H>(cell, 2, NL, T));
  const int r1 = (B + cap1 - 1) / cap1, r2 = ((B + 1) / 2 + cap2 - 1) / cap2;
  return r2 < r1 ? 2 : 1;
}

// Balanced persistent grid: the fewest residency rounds, then the fewest
// workgroups that still finish in that many rounds -- every workgroup walks
// the same number of batch tiles (B = 1440 at 768 resident: 720 x 2, not a
// second round of 672 behind a first of 768), and fewer co-resident waves
// make each recurrence step cheaper.
template <int H>
int bwd_dwout_grid(int NL, int T, int B, int cell, int nb) {
  const Kernel k = dwout_kernel<H>(cell, nb, NL, T);
  if (k.err != hipSuccess) return -1;
  const int cap = resident(k), t = tiles(B, nb);
  if (t <= cap) return t;
  const int rounds = (t + cap - 1) / cap;
  return (t + rounds - 1) / rounds;
}

template <int H>
hipError_t launch_bwd_dwout(const PdrnnLstmSmallBwdArgs* a, hipStream_t st, int grid, int nb) {
  if (a->NL * H * kUnitLanes<H> > 512) return hipErrorInvalidConfiguration;
  if (!bwd_lean(a) || !a->dg_out || a->dg_st < 4 * H) return hipErrorInvalidValue;
  // x is staged once per sequence (and written to xg_out): it has to fit LDS
  if ((nb == 2 && H > 32) || !x_in_lds(H, nb, a->T) || !a->xg_out) return hipErrorInvalidConfiguration;
  if (grid <= 0) grid = bwd_dwout_grid<H>(a->NL, a->T, a->B, a->cell, nb);
  return launch(dwout_kernel<H>(a->cell, nb, a->NL, a->T), grid, st, a);
}

}  // namespace
}  // namespace pdrnn

extern "C" {

// PDRNN_TUNE dwout=0 disables the deferred-dW backward, dwout=force selects it at
// every batch size (tests: the one-launch step would otherwise take B <= one
// residency round).  Returns 0 (not covered), 1 (covered), 2 (covered, forced).
int pdrnn_lstm_small_dwout_ok(int H, int NL, int T) {
  // read per call (one host query per training step): tests flip it in-process
  char e[16];
  const int mode = !pdrnn_tune_str("dwout", e, (int)sizeof(e)) ? 1 : (e[0] == '0' ? 0 : (strcmp(e, "force") == 0 ? 2 : 1));
  if (mode == 0 || T < 4 || NL < 1 || NL > PDRNN_MAX_LAYERS) return 0;
  if (H != 16 && H != 32 && H != 64) return 0;
  if (!pdrnn::x_in_lds(H, 1, T)) return 0;  // LDS-resident x only
  return NL * H * (H >= 64 ? 8 : 4) <= 512 ? mode : 0;
}

// (LSTM and GRU instantiations share the register budget -- same VGPR class;
// the LSTM's is the one queried)
int pdrnn_lstm_small_bwd_dwout_nb(int H, int NL, int T, int B) {
  return pdrnn::with_hidden(H, -1, [&](auto h) { return pdrnn::bwd_dwout_nb<h>(NL, T, B, 0); });
}
int pdrnn_lstm_small_bwd_dwout_grid(int H, int NL, int T, int B, int nb) {
  return pdrnn::with_hidden(H, -1, [&](auto h) { return pdrnn::bwd_dwout_grid<h>(NL, T, B, 0, nb); });
}

hipError_t pdrnn_lstm_small_bwd_dwout(const PdrnnLstmSmallBwdArgs* a, int H, int grid, int nb, hipStream_t stream) {
  if (a->x_bf16 && !pdrnn::x_in_lds(H, nb > 1 ? nb : 1, a->T)) return hipErrorInvalidConfiguration;
  if (nb != 1 && nb != 2) return hipErrorInvalidValue;
  return pdrnn::with_hidden(H, hipErrorInvalidValue, [&](auto h) {
    return pdrnn::launch_bwd_dwout<h>(a, stream, grid, nb);
  });
}

// 1 when the fused one-launch step covers (H, NL, B, launch config): the
// gate-split forward with one sequence per workgroup, the L = 4 unit-group
// backward, and a backward grid of one sequence per workgroup (gridb == B).
int pdrnn_lstm_small_step_ok(int H, int NL, int B, int nb_fwd, int split_fwd, int nb_bwd, int split_bwd,
                             int gridb) {
  if ((H != 16 && H != 32) || nb_fwd != 1 || split_fwd != 1 || nb_bwd != 1 || split_bwd != 1) return 0;
  return NL * 4 * H <= 512 && gridb == B;
}

// Fused forward + head/CE + BPTT launch of the latency regime (see
// lstm_small_step_gs_kernel); H in {16, 32}.
hipError_t pdrnn_lstm_small_step(const PdrnnLstmSmallFwdArgs* f, const PdrnnLstmSmallBwdArgs* b, int H,
                                 hipStream_t stream) {
  if (f->x_bf16 && !pdrnn::x_in_lds(H, 1, f->T)) return hipErrorInvalidConfiguration;
  return pdrnn::with_int<16, 32>(H, hipErrorInvalidValue, [&](auto h) { return pdrnn::launch_step<h>(f, b, stream); });
}

// H in {16, 32}: 4 lanes per unit in both passes, up to 4 layers per 512-lane
// workgroup.  H = 64: the backward's 8 lanes per unit fill it with one layer.
int pdrnn_lstm_small_supported(int H, int I, int NL) {
  if (I < 1 || I > H || NL < 1) return 0;
  if (H == 16 || H == 32) return NL <= PDRNN_MAX_LAYERS;
  return H == 64 && NL == 1;
}

// Largest split whose workgroup fits: more lanes per unit = shorter
// per-timestep critical path (latency-bound small batches); the host may
// request a smaller one for throughput-bound large batches.
int pdrnn_lstm_small_max_split(int H, int NL, int backward) {
  if (backward) {
    if (NL * H * (H >= 64 ? 8 : 4) <= 512) return 1;  // unit-group map
    if (NL * 4 * H <= 512 && (2 * H) % 16 == 0) return 2;  // 2-slice row split
    return 0;
  }
  if (NL * 4 * H <= 512) return 1;  // gate-split map
  if (NL * H * 2 <= 512 && (H * 2) % 64 == 0) return 2;  // 2-lane K split
  return 0;
}

hipError_t pdrnn_lstm_small_fwd(const PdrnnLstmSmallFwdArgs* a, int H, int nb, int split, int save,
                                hipStream_t stream) {
  // bf16 inputs are widened while staging x into LDS: needs the LDS-resident x path
  if (a->x_bf16 && !pdrnn::x_in_lds(H, nb > 1 ? nb : 1, a->T)) return hipErrorInvalidConfiguration;
  return pdrnn::with_hidden(H, hipErrorInvalidValue, [&](auto h) {
    const pdrnn::Kernel k = pdrnn::fwd_kernel<h>(a, nb, split, save != 0);
    return pdrnn::launch(k, pdrnn::tiles(a->B, k.nb), stream, a);
  });
}

hipError_t pdrnn_lstm_small_bwd(const PdrnnLstmSmallBwdArgs* a, int H, int nb, int split, int grid,
                                hipStream_t stream) {
  if (a->x_bf16 && (split != 1 || !pdrnn::x_in_lds(H, nb > 1 ? nb : 1, a->T))) return hipErrorInvalidConfiguration;
  return pdrnn::with_hidden(H, hipErrorInvalidValue, [&](auto h) {
    return pdrnn::launch_bwd<h>(a, nb, split, grid, stream);
  });
}

// Slab rows (= grid) the backward will use for (H, NL, T, B, split).  The
// general LSTM instantiation is the one queried whatever the launch will be
// (GRU, lean contract): the slab rows, and with them the order in which the
// gradients are summed, depend on neither.
int pdrnn_lstm_small_bwd_grid(int H, int NL, int T, int B, int nb, int split) {
  if (split != 1) return (B + nb - 1) / nb;
  return pdrnn::with_hidden(H, -1, [&](auto h) {
    return pdrnn::persistent_grid(pdrnn::bwd_gs_kernel<h>(0, nb, NL, T, false), B);
  });
}

}  // extern "C"
