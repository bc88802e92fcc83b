// Char-LM evaluation: vocabulary head + log-softmax + NLL + argmax in one
// kernel, for gfx950.  The logits live in MFMA accumulators from the product
// to the loss: they are never stored and never rounded to 16 bits.
//
//   row_nll[r] = logsumexp_v(h[r] . w[v] + bias[v]) - (h[r] . w[label_r] + bias[label_r])
//   pred[r]    = argmax_v of the same logits, the lowest index on ties
//   accum     += [sum row_nll, n_valid, n_correct]  (fp64)
//
// Work split.  A workgroup of 8 waves owns 256 rows of h and walks all V
// columns in passes of 256.  Wave w owns rows 32 w .. 32 w + 31 (two 16-row A
// fragments, read straight from global memory: no other wave needs them) and
// in a pass all 16 column tiles: 2 x 16 accumulators of v_mfma_f32_16x16x32.
// The pass's W tile [256 columns, 64 k] goes through LDS, fetched once per
// workgroup (register-staged one tile ahead, 144-byte rows: the 16 lanes of a
// fragment read land on 64 different banks).  In the accumulator layout a lane
// holds column lane & 15 of every tile for rows 4 (lane >> 4) + 0..3: a row's
// max / argmax / sum-exp / target logit is a scan over the lane's own 16
// registers followed by a 4-step butterfly over the 16-lane group.  V > 256:
// further passes fold into a running (max, sum, argmax, target) with the usual
// rescale by exp(old max - new max).  Columns >= V are zero operands and are
// masked out of max, sum and argmax; rows >= N are never read or written.
//
// Workgroup sums are fp64, taken in a fixed order, written to `partial`; a
// second one-block launch adds them up in a fixed order and adds the totals
// to accum: bitwise reproducible, and nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pdrnn/api.h"
#include "pdrnn/common.h"

namespace pdrnn {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BF16 {
  static __device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                   c, 0, 0, 0);
  }
};
struct F16 {
  static __device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b),
                                                  c, 0, 0, 0);
  }
};

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * kWave;
constexpr int kRows = kWaves * 32;       // rows of a workgroup: 32 per wave
constexpr int kCols = 256;               // columns of a pass
constexpr int kTiles = kCols / 16;       // column tiles of a pass
constexpr int kBK = 64;                  // k of a staged W tile
constexpr int kLdsRow = kBK * 2 + 16;    // bytes: a W row of the tile plus one 16-byte slot of padding
constexpr int kStage = kCols * (kBK / 8) / kThreads;  // 16-byte pieces of the tile per thread

struct Dims {
  int64_t N, ldh, ignore_index;
  int H, V;
};

// A row's running statistics over the column passes.
struct RowStat {
  float m, s, t;  // maximum, sum of exp(logit - m), target logit
  int a;          // argmax
};

__device__ __forceinline__ uint4 keep_if(bool c, const uint4& v) {
  return make_uint4(c ? v.x : 0u, c ? v.y : 0u, c ? v.z : 0u, c ? v.w : 0u);
}

// FULL: V is a multiple of 256, every pass has all 16 column tiles (no per-tile test in the product loop).
template <class DT, bool FULL>
__global__ __launch_bounds__(kThreads, 2) void head_nll_kernel(
    const uint16_t* __restrict__ hp, const uint16_t* __restrict__ wp, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, float* __restrict__ row_nll, int* __restrict__ pred,
    double* __restrict__ partial, const Dims d) {
  __shared__ __attribute__((aligned(16))) unsigned char wt[kCols * kLdsRow];
  __shared__ RowStat s_stat[kRows];  // written and read by the row's own wave
  __shared__ int s_lab[kRows];       // the label, -1 where the row is not valid
  __shared__ float s_nll[kRows];
  __shared__ int s_flag[kRows];      // bit 0 valid, bit 1 correct
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, kq = lane >> 4;
  const int H = d.H, V = d.V;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;

  if (tid < kRows) {
    int64_t l = -1;
    if (row0 + tid < d.N) {
      l = labels[row0 + tid];
      PDRNN_DEVICE_ASSERT(l == d.ignore_index || (l >= 0 && l < V));
      if (l == d.ignore_index || l < 0 || l >= V) l = -1;
    }
    s_lab[tid] = (int)l;
  }

  // Masked operands are read from a clamped, always valid address and zeroed
  // afterwards: nothing outside h[0:N] and w[0:V] is ever touched.
  // The A fragments' rows (m = 0, 1): row0 + 32 wave + 16 m + c16, k = 8 kq + 0..7 of a 32-block.
  const uint16_t* hrow0;
  const uint16_t* hrow1;
  const bool hlive0 = row0 + wave * 32 + c16 < d.N, hlive1 = row0 + wave * 32 + 16 + c16 < d.N;
  hrow0 = hp + (hlive0 ? row0 + wave * 32 + c16 : 0) * d.ldh + kq * 8;
  hrow1 = hp + (hlive1 ? row0 + wave * 32 + 16 + c16 : 0) * d.ldh + kq * 8;
  // Piece i of this thread's share of a W tile: column (tid >> 3) + 64 i of the pass, k = 8 (tid & 7) of the tile.
  const int scol = tid >> 3, sk = (tid & 7) * 8;
  unsigned char* const swr = wt + scol * kLdsRow + (tid & 7) * 16;
  const unsigned char* const brd = wt + c16 * kLdsRow + kq * 16;

  const int nkc = (H + kBK - 1) / kBK;  // (H % 32 == 0: the last tile may hold one 32-block)
  for (int vbase = 0; vbase < V; vbase += kCols) {
    const int vrem = V - vbase;
    const int ntiles = FULL ? kTiles : min(kTiles, (vrem + 15) / 16);
    f32x4 acc0[kTiles], acc1[kTiles];
#pragma unroll
    for (int n = 0; n < kTiles; ++n) acc0[n] = acc1[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    int woff[kStage];
    bool wlive[kStage];
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int col = scol + 64 * i;
      wlive[i] = FULL || col < vrem;
      woff[i] = (vbase + (wlive[i] ? col : 0)) * H;
    }
    // The next tile's W pieces and A fragments [m][32-block], as loaded: the
    // masks are applied where they are consumed, so the loads stay in flight
    // during the current tile's products.
    uint4 stage[kStage], an00, an01, an10, an11;
    {
      const int ks = sk < H ? sk : 0, k1 = 32 < H ? 32 : 0;
#pragma unroll
      for (int i = 0; i < kStage; ++i) stage[i] = *reinterpret_cast<const uint4*>(wp + woff[i] + ks);
      an00 = *reinterpret_cast<const uint4*>(hrow0);
      an10 = *reinterpret_cast<const uint4*>(hrow1);
      an01 = *reinterpret_cast<const uint4*>(hrow0 + k1);
      an11 = *reinterpret_cast<const uint4*>(hrow1 + k1);
    }
    for (int kc = 0; kc < nkc; ++kc) {
      const bool kw = kc * kBK + sk < H, ka1 = kc * kBK + 32 < H;
      __syncthreads();  // the tile before this one has been read
#pragma unroll
      for (int i = 0; i < kStage; ++i)
        *reinterpret_cast<uint4*>(swr + i * 64 * kLdsRow) = keep_if(wlive[i] && kw, stage[i]);
      const uint4 a00 = keep_if(hlive0, an00), a10 = keep_if(hlive1, an10);
      const uint4 a01 = keep_if(hlive0 && ka1, an01), a11 = keep_if(hlive1 && ka1, an11);
      __syncthreads();
      {
        // past the last tile (k >= H) the addresses are clamped and the values unused
        const int k0 = (kc + 1) * kBK;
        const int ks = k0 + sk < H ? k0 + sk : 0, ka = k0 < H ? k0 : 0, kb = k0 + 32 < H ? k0 + 32 : 0;
#pragma unroll
        for (int i = 0; i < kStage; ++i) stage[i] = *reinterpret_cast<const uint4*>(wp + woff[i] + ks);
        an00 = *reinterpret_cast<const uint4*>(hrow0 + ka);
        an10 = *reinterpret_cast<const uint4*>(hrow1 + ka);
        an01 = *reinterpret_cast<const uint4*>(hrow0 + kb);
        an11 = *reinterpret_cast<const uint4*>(hrow1 + kb);
      }
      __builtin_amdgcn_sched_barrier(0);  // (the loads are issued before the products, not after)
      // (k >= H of the last tile: zero operands on both sides.)  Column tile
      // n + 1's fragments are read while tile n's products issue.
      uint4 b0 = *reinterpret_cast<const uint4*>(brd), b1 = *reinterpret_cast<const uint4*>(brd + 64);
#pragma unroll
      for (int n = 0; n < kTiles; ++n) {
        uint4 nb0 = b0, nb1 = b1;
        if (n + 1 < kTiles) {
          nb0 = *reinterpret_cast<const uint4*>(brd + (n + 1) * 16 * kLdsRow);
          nb1 = *reinterpret_cast<const uint4*>(brd + (n + 1) * 16 * kLdsRow + 64);
        }
        if (FULL || n < ntiles) {
          acc0[n] = DT::mfma(a00, b0, acc0[n]);
          acc1[n] = DT::mfma(a10, b0, acc1[n]);
          acc0[n] = DT::mfma(a01, b1, acc0[n]);
          acc1[n] = DT::mfma(a11, b1, acc1[n]);
        }
        b0 = nb0;
        b1 = nb1;
      }
    }

    // ---- the pass's columns into the rows' running statistics ---------------
    // the lane's 8 result rows (m, j): 32 wave + 16 m + 4 kq + j of the workgroup
    float bs[kTiles];
#pragma unroll
    for (int n = 0; n < kTiles; ++n) {
      const int col = vbase + n * 16 + c16;
      bs[n] = (bias != nullptr && col < V) ? bias[col] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4* const acc = m == 0 ? acc0 : acc1;
        const int lr = wave * 32 + m * 16 + kq * 4 + j;
        const int lab = s_lab[lr];
        float pm = -INFINITY, t = 0.f;
        int pa = V;
#pragma unroll
        for (int n = 0; n < kTiles; ++n) {
          if (FULL || n < ntiles) {
            const int col = vbase + n * 16 + c16;
            const float v = acc[n][j] + bs[n];
            acc[n][j] = v;
            if (col < V && (v > pm || (v != v && pm == pm))) { pm = v; pa = col; }  // ascending columns: the first maximum stays
            t += col == lab ? v : 0.f;
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float om = __shfl_xor(pm, o, 64);
          const int oa = __shfl_xor(pa, o, 64);
          t += __shfl_xor(t, o, 64);
          if (om > pm || (om == pm && oa < pa) || (om != om && (pm == pm || oa < pa))) { pm = om; pa = oa; }
        }
        RowStat st{pm, 0.f, t, pa};
        float scale = 0.f;
        if (vbase != 0) {
          // every column of this pass lies above the earlier passes': an equal maximum keeps the earlier index
          const RowStat old = s_stat[lr];
          if (!(pm > old.m || (pm != pm && old.m == old.m))) { st.m = old.m; st.a = old.a; }
          st.t += old.t;
          scale = old.s * __expf(old.m - st.m);
        }
        float ps = 0.f;
#pragma unroll
        for (int n = 0; n < kTiles; ++n) {
          if (FULL || n < ntiles) {
            const int col = vbase + n * 16 + c16;
            ps += col < V ? __expf(acc[n][j] - st.m) : 0.f;
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) ps += __shfl_xor(ps, o, 64);
        st.s = scale + ps;
        if (c16 == 0) s_stat[lr] = st;
      }
  }
  __syncthreads();

  // ---- per row: the loss and the prediction; per workgroup: the sums --------
  if (tid < kRows) {
    const int64_t r = row0 + tid;
    const RowStat st = s_stat[tid];
    const int lab = s_lab[tid];
    const bool valid = lab >= 0;
    const int pr = st.a < V ? st.a : 0;  // (nothing compared greater than -inf: a valid index all the same)
    const float nll = valid ? (st.m + __logf(st.s)) - st.t : 0.f;
    const bool in = r < d.N;
    if (in) {
      row_nll[r] = nll;
      pred[r] = pr;
    }
    s_nll[tid] = in ? nll : 0.f;
    s_flag[tid] = in ? (valid ? 1 : 0) | (valid && pr == lab ? 2 : 0) : 0;
  }
  __syncthreads();
  if (wave == 0) {
    double sl = 0.0;
    int nv = 0, nc = 0;
#pragma unroll
    for (int i = 0; i < kRows / kWave; ++i) {
      sl += (double)s_nll[i * kWave + lane];
      nv += s_flag[i * kWave + lane] & 1;
      nc += (s_flag[i * kWave + lane] >> 1) & 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sl += __shfl_xor(sl, o, 64);
      nv += __shfl_xor(nv, o, 64);
      nc += __shfl_xor(nc, o, 64);
    }
    if (lane == 0) {
      double* p = partial + (int64_t)blockIdx.x * 3;
      p[0] = sl;
      p[1] = (double)nv;
      p[2] = (double)nc;
    }
  }
}

// accum += the workgroups' partial sums, in a fixed order, in fp64.
__global__ __launch_bounds__(256) void head_nll_finalize(const double* partial, int nblocks, double* accum) {
  __shared__ double red[3][256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    s0 += partial[(int64_t)i * 3 + 0];
    s1 += partial[(int64_t)i * 3 + 1];
    s2 += partial[(int64_t)i * 3 + 2];
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) accum[threadIdx.x] += red[threadIdx.x][0];
}

}  // namespace
}  // namespace pdrnn

extern "C" {

int pdrnn_head_nll_supported(int H, int V, int dtype) {
  return H >= 32 && H % 32 == 0 && H <= 16384 && V >= 1 && V <= 1024 && (dtype == 0 || dtype == 1);
}

int pdrnn_head_nll_blocks(int64_t N) { return (int)((N + pdrnn::kRows - 1) / pdrnn::kRows); }

hipError_t pdrnn_head_nll(const PdrnnHeadNllArgs* a, hipStream_t stream) {
  if (a->N < 1 || a->N > ((int64_t)1 << 37) || a->ldh < a->H || a->ldh % 8 != 0 ||
      !pdrnn_head_nll_supported(a->H, a->V, a->dtype))
    return hipErrorInvalidValue;
  const int nblocks = pdrnn_head_nll_blocks(a->N);
  const pdrnn::Dims d{a->N, a->ldh, a->ignore_index, a->H, a->V};
  const uint16_t* h = static_cast<const uint16_t*>(a->h);
  const uint16_t* w = static_cast<const uint16_t*>(a->w);
  const bool full = a->V % pdrnn::kCols == 0;
#define PDRNN_HEAD_NLL(DT, FULL)                                                                        \
  pdrnn::head_nll_kernel<pdrnn::DT, FULL><<<nblocks, pdrnn::kThreads, 0, stream>>>(h, w, a->bias, a->labels, a->row_nll, \
                                                                                  a->pred, a->partial, d)
  if (a->dtype == 0) {
    if (full) PDRNN_HEAD_NLL(BF16, true); else PDRNN_HEAD_NLL(BF16, false);
  } else {
    if (full) PDRNN_HEAD_NLL(F16, true); else PDRNN_HEAD_NLL(F16, false);
  }
#undef PDRNN_HEAD_NLL
  PDRNN_HIP_CHECK(hipGetLastError());
  pdrnn::head_nll_finalize<<<1, 256, 0, stream>>>(a->partial, nblocks, a->accum);
  return hipGetLastError();
}

}  // extern "C"
