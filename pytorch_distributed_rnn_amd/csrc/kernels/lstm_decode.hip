// Char-LM generation: one LSTM layer for ONE token and up to 16 streams per
// launch, the vocabulary head, and the Gumbel-max sampler, for gfx950.
//
// Decoding a token is a chain of matrix-vector products: the work is streaming
// the weights (about 28 MB at 2 x 1024, resident in the Infinity Cache), and
// the training kernels' 256-row tiles and per-step host work are all overhead.
// Here a token is L + 1 short launches on one stream and nothing else:
//   * lstm_decode_layer<DT, FIRST, PICK>: [x_t | h_{t-1}] [W_ih | W_hh]^T on
//     v_mfma_f32_16x16x32 with the WEIGHTS as the A operand and the streams,
//     padded to 16, as B.  A workgroup owns 16 gate-interleaved rows (4 hidden
//     units); its 8 waves split K and reduce through LDS.  In the accumulator
//     layout a lane then holds rows 4(lane >> 4) + {0, 1, 2, 3} = gates i, f,
//     g, o of one unit for stream lane & 15: the cell runs on a lane's own
//     four registers, no exchange.  Padding streams are zero operands and are
//     never stored.
//   * FIRST (layer 0) first picks each stream's input token -- forced, the
//     prompt's last, or sampled from the previous position's logits -- and
//     reads x_t straight from that row of the 16-bit embedding.  Every
//     workgroup samples the same B tokens on its own (B x V values, an argmax);
//     workgroup 0 alone records them.  With a top-k / nucleus filter or the
//     log-probs wanted, the Pick::filtered instantiation first finds each row's
//     keep threshold by a bitwise selection in registers (sample_tokens_filtered_n).
//   * lstm_decode_head<DT>: logits = h_top W_fc^T + b_fc in fp32, 16
//     vocabulary rows per workgroup, rows past V masked.
//   * Beam search (the Pick::beam instantiations; pdrnn/decode_rng.h: the
//     rule): G groups of W beams are G W <= 16 of the streams.  In sampling's
//     place layer 0 selects each group's W best of its W V candidates
//     (beam_select_n) and every layer reads h_{t-1} and c of stream parent[n]
//     instead of n; the last selection and the backtrace are lstm_decode_beam_pick.
// h ping-pongs between two buffers by token parity (every workgroup reads all
// of h_{t-1} while the others write h_t); layer l > 0 reads layer l - 1's h_t
// of the same token.  All ordering is kernel boundaries on one stream: nothing
// inside a launch waits for another workgroup.  Sampling and the search share
// one token loop on the host (decode_positions) and differ in the layer-0
// instantiation and in the launch after the last position.
//
// The GRU (Cell::gru) is the same launches with another cell.  A unit's four A
// rows are r, z, n_x, n_h: the n gate's input and recurrent parts land in
// separate accumulator registers of one lane, and n = tanh(n_x + b_in + r (n_h
// + b_hn)) again needs no exchange.  n_h has no x part and n_x no h part: the
// rows come from the training kernels' zero-padded gate-interleaved stacks
// ([r | z | n_x | 0] and [r | z | 0 | n_h], ops/gru_large.py), read exactly as
// the LSTM's.  (Leaving the zero quarter unread -- the lanes of that row slot
// predicated off, rows straight from nn.GRU's [3H, .] -- measured slower at
// B = 1 and B = 16: profiles/r18/gru_decode.md.)  h_t = n + z (h_{t-1} - n)
// reads h_{t-1} from an fp32 master, which lives where the LSTM keeps c
// (LayerArgs::c) and is updated in place like it; the 16-bit ping-pong h is
// its rounding.
//
// The wide tile (lstm_decode_layer_wide, lstm_decode_head_wide; 17 to 64
// streams): the weights are the A operand, so one weight load can feed several
// stream tiles.  A wave loads its weight block once, the [x | h] block of NT =
// 2, 3 or 4 tiles of 16 streams (a padding stream: a copy of the last stream's,
// never stored), and issues NT MFMAs into NT accumulators, each
// over the blocks kb = wave, wave + 8, ... in that order; wave j < NT then sums
// tile j over the eight waves in wave order and runs its cell (the head: its
// bias add and stores), the epilogues side by side.  A stream's accumulation
// chain, reduction order and cell arithmetic are the 16-stream kernel's: its
// h, c, logits and tokens do not depend on how the batch is tiled.  The wide
// beam search (the Pick::beam instantiations of lstm_decode_layer_wide,
// lstm_decode_beam_pick_wide): G W in (16, 64] streams, groups free to lie
// across tile boundaries; a group's search is bit for bit the 16-stream one.
//
// Reference semantics: torch.nn.Embedding + nn.LSTM (gate order i, f, g, o) or
// nn.GRU (r, z, n) + nn.Linear stepped one token at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pdrnn/api.h"
#include "pdrnn/common.h"
#include "pdrnn/decode_rng.h"

namespace pdrnn {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BF16 {
  static __device__ __forceinline__ uint16_t from_f(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
  static __device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                   c, 0, 0, 0);
  }
};
struct F16 {
  static __device__ __forceinline__ uint16_t from_f(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
  static __device__ __forceinline__ f32x4 mfma(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b),
                                                  c, 0, 0, 0);
  }
};

constexpr int kWaves = 8;               // K-split waves of a workgroup
constexpr int kThreads = kWaves * kWave;
constexpr int kStreams = 16;            // the MFMA tile's N side

// What the sampler reads and writes (shared by layer 0 and the final launch).
struct SampleArgs {
  const float* scratch;   // [B, V] logits of the previous position
  int64_t* tokens;        // [B, N]
  int B, V, N;
  float temperature;      // 0: greedy
  uint32_t seed, stream0, pos0;
  // the filtered sampler only (sample_tokens_filtered_n)
  int top_k;              // 0: off
  float top_p;            // 0 or >= 1: off
  float* threshold;       // [B, N] or null
  float* logprobs;        // [B, N] or null
};

// tok[b] = argmax_v(logit / T + g), the lowest index on ties, for every stream
// b < B; position p of the N generated ones (hash position pos0 + p).  Wave w
// takes streams w, w + 8, ...; all lanes of the workgroup must call.  (The draw
// stands here and again in sample_tokens_filtered_n, as it was: written once as
// a shared helper it changed the filtered kernels' code, profiles/r16/decode_refactor.md.)
__device__ __forceinline__ void sample_tokens(const SampleArgs& s, int p, int* tok) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < s.B; b += kWaves) {
    const uint32_t key = decode_key(s.seed, s.stream0 + (uint32_t)b, s.pos0 + (uint32_t)p);
    const float* row = s.scratch + (int64_t)b * s.V;
    float best = -INFINITY;
    int bi = s.V;
    for (int v = lane; v < s.V; v += kWave) {
      float val = row[v];
      if (s.temperature != 0.f) {
        const float u = decode_uniform(decode_word(key, (uint32_t)v));
        val = val / s.temperature + -logf(-logf(u));
      }
      if (val > best) { best = val; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) tok[b] = bi < s.V ? bi : 0;  // (all-NaN logits: a valid row all the same)
  }
}

// Thread b < B records stream b's token (threshold, log-prob) at column p.
template <bool FILT>
__device__ __forceinline__ void record_sample(const SampleArgs& s, int p, const int* tok, const float* thr,
                                              const float* lp) {
  if (threadIdx.x < s.B) {
    const int64_t at = (int64_t)threadIdx.x * s.N + p;
    s.tokens[at] = tok[threadIdx.x];
    if constexpr (FILT) {
      if (s.threshold != nullptr) s.threshold[at] = thr[threadIdx.x];
      if (s.logprobs != nullptr) s.logprobs[at] = lp[threadIdx.x];
    }
  }
}

// a token held inside the vocabulary: a bad value reads no memory outside the embedding
__device__ __forceinline__ int64_t clamp_token(int64_t t, int V) {
  PDRNN_DEVICE_ASSERT(t >= 0 && t < V);
  return t < 0 ? 0 : (t >= V ? V - 1 : t);
}

constexpr int kSlots = 16;  // logits a lane holds at the most: ceil(1024 / 64)

// f(Slots<NS>): NS the slots a lane needs for a row of V (the launch's: V is uniform)
template <int NS>
struct Slots {
  static constexpr int value = NS;
};
template <class F>
__device__ __forceinline__ void with_slots(int V, F&& f) {
  if (V <= 1 * kWave) f(Slots<1>{});
  else if (V <= 2 * kWave) f(Slots<2>{});
  else if (V <= 4 * kWave) f(Slots<4>{});
  else if (V <= 8 * kWave) f(Slots<8>{});
  else f(Slots<kSlots>{});
}

// A lane's entries lane, lane + 64, ... of a row of V: every load in flight at
// once, the index held inside the row.  The slots past V hold a copy of the
// last entry: the caller sets them to -inf where it first reads the values
// (masking here instead cost the filtered sampler a select per slot and beam
// layer 0 four VGPRs, profiles/r16/decode_resources.md).
template <int NS>
__device__ __forceinline__ void load_row(const float* row, int V, float (&l)[NS]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int v = lane + i * kWave;
    l[i] = row[v < V ? v : V - 1];
  }
}

// The value of another lane of the row of 16, by a DPP control; of any lane of the wave.
template <int CTRL, class T>
__device__ __forceinline__ T dpp_peer(T x) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <class T>
__device__ __forceinline__ T lane_value(T x, int lane) {
  return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}

struct Sum {
  static __device__ __forceinline__ float op(float a, float b) { return a + b; }
};
struct Max {
  static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return a > b ? a : b; }
};

// Wave-wide reduction in a fixed order, no LDS path.  Within a row of 16 lanes
// a butterfly: the lanes paired at a stage combine the same two values (a + b
// and b + a: the same bits), so the row's lanes end equal -- quad_perm
// [1 0 3 2], [2 3 0 1], then row_half_mirror and row_mirror, which pair a lane
// with one of the other, already equal, quad or half.  The four row values are
// then read out and combined as (r0 + r1) + (r2 + r3) in every lane.  Every
// wave of every workgroup that starts from the same row ends with the same
// bits: with Sum that is what makes all of them find the same threshold and token.
template <class Op, class T>
__device__ __forceinline__ T wave_reduce(T x) {
  x = Op::op(x, dpp_peer<0xb1>(x));
  x = Op::op(x, dpp_peer<0x4e>(x));
  x = Op::op(x, dpp_peer<0x141>(x));
  x = Op::op(x, dpp_peer<0x140>(x));
  return Op::op(Op::op(lane_value(x, 0), lane_value(x, 16)), Op::op(lane_value(x, 32), lane_value(x, 48)));
}

// sum{w : key >= t}: a lane's slots in order, then the wave's sum.  The terms
// are >= 0 and rounding is monotone, so the sum does not grow with t.
template <int NS>
__device__ __forceinline__ float mass_at_least(const uint32_t (&key)[NS], const float (&w)[NS], uint32_t t) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i) acc += key[i] >= t ? w[i] : 0.f;
  return wave_reduce<Sum>(acc);
}

// |{key >= t}|, t > 0 (slots past V hold key 0)
template <int NS>
__device__ __forceinline__ int count_at_least(const uint32_t (&key)[NS], uint32_t t) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) n += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[i] >= t));
  return n;
}

// sample_tokens with the filters of pdrnn/decode_rng.h: the same draw over the
// entries l_v >= tau, and thr[b] = tau, lp[b] = the drawn token's log-prob
// under the kept distribution.  A lane holds entries lane, lane + 64, ... of
// the row (NS >= V / 64 of them) in registers, as values, as order-preserving
// keys and (where a mass is needed) as weights w = exp(y - max y).  tau's key
// is built bit by bit from the top: a bit stays set while the entries at or
// above the candidate still number top_k (wave ballots) or still weigh top_p
// of the top-k survivors (mass_at_least) -- the largest key with that property
// is an entry's own.  Counts are integers and the sums are the same
// instructions on the same values in every workgroup: all of them find the
// same tau and token.
template <int NS>
__device__ __forceinline__ void sample_tokens_filtered_n(const SampleArgs& s, int p, int* tok, float* thr, float* lp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = s.V;
  const bool greedy = s.temperature == 0.f;  // no filter, log-prob at T = 1
  const float T = greedy ? 1.f : s.temperature;
  const int top_k = (!greedy && s.top_k > 0 && s.top_k < V) ? s.top_k : 0;
  const bool nucleus = !greedy && s.top_p > 0.f && s.top_p < 1.f;
  const bool mass = nucleus || s.logprobs != nullptr;
  for (int b = wave; b < s.B; b += kWaves) {
    const uint32_t hkey = decode_key(s.seed, s.stream0 + (uint32_t)b, s.pos0 + (uint32_t)p);
    const float* row = s.scratch + (int64_t)b * V;
    float l[NS], w[NS];
    uint32_t key[NS];
    load_row<NS>(row, V, l);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const bool in = lane + i * kWave < V;
      l[i] = !in ? -INFINITY : l[i] == 0.f ? 0.f : l[i];  // (-0 counts as +0)
      key[i] = in ? decode_order_key(l[i]) : 0;
      m = fmaxf(m, l[i] / T);
      w[i] = 0.f;
    }
    if (mass) {
      m = wave_reduce<Max>(m);
#pragma unroll
      for (int i = 0; i < NS; ++i) w[i] = expf(l[i] / T - m);  // (slots past V: exp(-inf) = 0)
    }

    uint32_t t = 0;
    if (top_k) {
#pragma unroll 1
      for (uint32_t bit = 0x80000000u; bit != 0; bit >>= 1)
        if (count_at_least<NS>(key, t | bit) >= top_k) t |= bit;
    }
    if (nucleus) {
      // over the top-k survivors: their mass is the target's base, and the
      // search ends at or above t since mass(t) >= top_p mass(t)
      const float target = s.top_p * mass_at_least<NS>(key, w, t);
      uint32_t tp = 0;
#pragma unroll 1
      for (uint32_t bit = 0x80000000u; bit != 0; bit >>= 1)
        if (mass_at_least<NS>(key, w, tp | bit) >= target) tp |= bit;
      t = tp > t ? tp : t;
    }
    const float tau = (top_k || nucleus) ? decode_key_value(t) : -INFINITY;

    float best = -INFINITY;
    int bi = V;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int v = lane + i * kWave;
      if (v < V && l[i] >= tau) {
        float val = l[i];
        if (!greedy) {
          const float u = decode_uniform(decode_word(hkey, (uint32_t)v));
          val = val / s.temperature + -logf(-logf(u));
        }
        if (val > best) { best = val; bi = v; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    bi = bi < V ? bi : 0;  // (all-NaN logits: a valid row all the same)
    float lpv = 0.f;
    if (s.logprobs != nullptr) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < NS; ++i) acc += l[i] >= tau ? w[i] : 0.f;
      lpv = row[bi] / T - m - logf(wave_reduce<Sum>(acc));
    }
    if (lane == 0) {
      tok[b] = bi;
      thr[b] = tau;
      lp[b] = lpv;
    }
  }
}

// The workgroup's sampling of position p: tok (thr, lp) [B] in LDS.
template <bool FILT>
__device__ __forceinline__ void sample_position(const SampleArgs& s, int p, int* tok, float* thr, float* lp) {
  if constexpr (FILT) with_slots(s.V, [&](auto ns) { sample_tokens_filtered_n<decltype(ns)::value>(s, p, tok, thr, lp); });
  else sample_tokens(s, p, tok);
}

// ---- beam search (pdrnn/decode_rng.h: the rule) -------------------------------
// What one selection reads and writes.  Selection q works on position q's
// logits: it reads row q of cum / done and writes row q + 1 and column q of
// tokens / parents / lp, so no workgroup reads what another writes in a launch.
struct BeamArgs {
  const float* scratch;  // [S, V] logits of position q, S = G W
  float* cum;            // [N + 1, S]
  int32_t* done;         // [N + 1, S]
  int64_t* tokens;       // [S, N]
  int32_t* parents;      // [S, N] stream indices of the launch
  float* lp;             // [S, N] or null
  int G, W, V, N;
  int stop;              // -1: none
};

// A stream's W best candidates in rank order, for up to MAXS streams.
template <int MAXS>
struct BeamCands {
  uint32_t ck[MAXS][kStreams];  // score keys (0: none),
  int cv[MAXS][kStreams];       // tokens
  float cl[MAXS][kStreams];     // and log-probs
};
// the new slots
template <int MAXS>
struct BeamSlots {
  int parent[MAXS], tok[MAXS], done[MAXS];
  float cum[MAXS], lp[MAXS];
};
template <int MAXS>
struct BeamLdsOf {
  BeamCands<MAXS> c;
  BeamSlots<MAXS> s;
};
typedef BeamLdsOf<kStreams> BeamLds;

// The workgroup barrier of a selection: the wide kernels have their own (below).
struct BlockSync {
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// One selection, by every lane of the workgroup; the candidate lists in C, the
// new slots end in L (MAXS streams at the most; SYNC: the workgroup's barrier).
//   1. A wave per stream (waves take streams wave, wave + 8, ...), the row in
//      registers as in sample_tokens_filtered_n: log-softmax, score keys, then
//      the row's W best in rank order by W rounds of (wave max of the keys,
//      first holder by ballots: the lowest slot, then the lowest lane, is the
//      lowest v), into LDS.  A stream contributes at most W winners, and they
//      are among these.
//   2. A wave per group (groups wave, wave + 8, ...): lane j < W holds the head
//      of stream j's list; W rounds of (wave max of the heads, the lowest lane
//      holding it) merge them.
// Integer keys, ballots and fixed-order sums: the same bits in every workgroup,
// and for a group the same bits whichever launch holds it, and wherever in it.
template <int NS, class SYNC, int MAXS>
__device__ __forceinline__ void beam_select_n(const BeamArgs& b, int q, BeamCands<MAXS>& C, BeamSlots<MAXS>& L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = b.V, W = b.W, S = b.G * b.W;
  const float* cum = b.cum + (int64_t)q * S;
  const int32_t* done = b.done + (int64_t)q * S;
  for (int s = wave; s < S; s += kWaves) {
    const float* row = b.scratch + (int64_t)s * V;
    const float cs = cum[s];
    const bool ds = done[s] != 0;
    float l[NS], lpv[NS];
    uint32_t key[NS];
    load_row<NS>(row, V, l);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      if (lane + i * kWave >= V) l[i] = -INFINITY;
      m = fmaxf(m, l[i]);
    }
    m = wave_reduce<Max>(m);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      l[i] -= m;
      acc += lane + i * kWave < V ? expf(l[i]) : 0.f;
    }
    const float lse = logf(wave_reduce<Sum>(acc));
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int v = lane + i * kWave;
      lpv[i] = ds ? 0.f : l[i] - lse;
      const bool cand = v < V && (!ds || v == b.stop);
      key[i] = cand ? beam_score_key(ds ? cs : cs + lpv[i]) : 0;
    }
#pragma unroll 1
    for (int r = 0; r < W; ++r) {
      uint32_t mx = 0;
#pragma unroll
      for (int i = 0; i < NS; ++i) mx = Max::op(mx, key[i]);
      mx = wave_reduce<Max>(mx);
      int wv = 0;
      float wl = 0.f;
      if (mx != 0) {
        bool found = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const unsigned long long bal = __builtin_amdgcn_ballot_w64(key[i] == mx);
          if (!found && bal != 0) {
            found = true;
            const int at = __builtin_ctzll(bal);
            wv = i * kWave + at;
            wl = lane_value(lpv[i], at);
            if (lane == at) key[i] = 0;
          }
        }
      }
      if (lane == 0) {
        C.ck[s][r] = mx;
        C.cv[s][r] = wv;
        C.cl[s][r] = wl;
      }
    }
  }
  SYNC::sync();
  for (int g = wave; g < b.G; g += kWaves) {
    const int s = g * W + (lane < W ? lane : 0);
    int head = 0;
#pragma unroll 1
    for (int i = 0; i < W; ++i) {
      const uint32_t k = lane < W && head < W ? C.ck[s][head] : 0;
      const uint32_t mx = wave_reduce<Max>(k);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(lane < W && k == mx);
      const int j = __builtin_ctzll(bal);  // (a group always has W candidates: lane 0 at the worst)
      PDRNN_DEVICE_ASSERT(mx != 0);
      if (lane == j) {
        const int slot = g * W + i, v = head < W ? C.cv[s][head] : 0;
        L.parent[slot] = s;
        L.tok[slot] = v;
        L.cum[slot] = mx != 0 ? decode_key_value(mx) : -INFINITY;
        L.lp[slot] = head < W ? C.cl[s][head] : 0.f;
        L.done[slot] = done[s] != 0 || v == b.stop;
        ++head;
      }
    }
  }
  SYNC::sync();
}

__device__ __forceinline__ void beam_select(const BeamArgs& b, int q, BeamLds& L) {
  with_slots(b.V, [&](auto ns) { beam_select_n<decltype(ns)::value, BlockSync>(b, q, L.c, L.s); });
}

// selection q's record (one workgroup's job)
template <int MAXS>
__device__ __forceinline__ void beam_record(const BeamArgs& b, int q, const BeamSlots<MAXS>& L) {
  const int S = b.G * b.W, s = threadIdx.x;
  if (s >= S) return;
  const int64_t at = (int64_t)s * b.N + q;
  b.tokens[at] = L.tok[s];
  b.parents[at] = L.parent[s];
  if (b.lp != nullptr) b.lp[at] = L.lp[s];
  b.cum[(int64_t)(q + 1) * S + s] = L.cum[s];
  b.done[(int64_t)(q + 1) * S + s] = L.done[s];
}

// a parent held inside its group's streams: a bad value reads no memory outside the buffers
__device__ __forceinline__ int beam_parent(int par, int n, int W) {
  const int lo = n - n % W;
  PDRNN_DEVICE_ASSERT(par >= lo && par < lo + W);
  return par < lo ? lo : (par >= lo + W ? lo + W - 1 : par);
}

struct LayerArgs {
  const uint16_t* wx;     // [4H, Kx] gate-interleaved rows 4u + q (GRU: q = r, z, n_x, 0)
  const uint16_t* wh;     // [4H, H] (GRU: q = r, z, 0, n_h)
  const float* bias;      // [4H] b_ih + b_hh, interleaved; GRU: b_ir + b_hr, b_iz + b_hz, b_in, b_hn per unit
  const uint16_t* x;      // FIRST: the embedding [V, Kx]; else the layer below's h_t [B, Kx]
  const uint16_t* hprev;  // [B, H]
  uint16_t* hout;         // [B, H]
  float* c;               // [B, H], updated in place: c, or the GRU's fp32 h
  const int64_t* first;   // FIRST: [B] input tokens of position 0
  const int64_t* forced;  // FIRST: [B, N] input tokens of every position, or null
  SampleArgs s;
  int H, Kx, p;
  BeamArgs b;             // Pick::beam: the search (s: B, V and N only)
};

// How position p's input token is chosen in layer 0.  The layers above read
// only "beam or not" from it: they exist for sample and beam.
enum class Pick { sample, filtered, beam };

// The stack's cell (PdrnnLstmDecodeStack::cell): what a lane does with its four sums.
enum class Cell { lstm = 0, gru = 1 };

// Sum of the waves' partial accumulators, in wave order, into wave 0.
__device__ __forceinline__ f32x4 reduce_waves(f32x4 acc, f32x4 (*red)[kWave]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  red[wave][lane] = acc;
  __syncthreads();
  f32x4 sum = red[0][lane];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) sum += red[w][lane];
  return sum;
}

// Pick::filtered (layer 0 only, chosen on the host): the filtered sampler and
// its two outputs; a launch sequence with no filter and no output wanted never
// runs it.
//
// Pick::beam: stream n continues stream par = parent[n] of the previous
// position: it reads h_{t-1} and c (the GRU: the fp32 h) of par in every layer
// (x of a layer above 0 is the layer below's h_t, already in new-slot order).
// Layer 0 selects (beam_select; by every workgroup, recorded by workgroup 0);
// the layers above read the record.  c stays in place, for both cells: a unit's
// 16 streams are 16 lanes of wave 0 of one workgroup, which loads c[par] in one
// instruction and stores c[n] in a later one that depends on the loaded value,
// so every lane's load has completed before any lane's store; no other
// workgroup touches the unit.
//
// Every __syncthreads() below is reached by all threads of a workgroup: what
// guards the sampling and the selection (p, forced, blockIdx) is uniform in it.
template <class DT, bool FIRST, Pick PICK, Cell CELL>
__global__ __launch_bounds__(kThreads) void lstm_decode_layer(const LayerArgs a) {
  static_assert(FIRST || PICK != Pick::filtered, "the filter is layer 0's");
  constexpr bool FILT = PICK == Pick::filtered, BEAM = PICK == Pick::beam;
  __shared__ f32x4 red[kWaves][kWave];
  __shared__ int tok[kStreams];
  __shared__ float thr[FILT ? kStreams : 1], lp[FILT ? kStreams : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int B = a.s.B, H = a.H, Kx = a.Kx;
  const bool live = n < B;
  int par = n;  // the stream whose state stream n continues

  const uint16_t* xrow = a.x + (int64_t)n * Kx;  // (read only where live)
  if constexpr (BEAM && FIRST) {
    __shared__ BeamLds L;
    if (a.p > 0) {
      beam_select(a.b, a.p - 1, L);
      if (blockIdx.x == 0) beam_record(a.b, a.p - 1, L.s);
    }
    int64_t t = 0;
    if (live) {
      if (a.p == 0) t = a.first[n];
      else t = L.s.tok[n], par = L.s.parent[n];
      t = clamp_token(t, a.s.V);
      par = beam_parent(par, n, a.b.W);
    }
    xrow = a.x + t * Kx;
  } else if constexpr (BEAM) {
    if (live && a.p > 0) par = beam_parent(a.b.parents[(int64_t)n * a.b.N + a.p - 1], n, a.b.W);
  } else if constexpr (FIRST) {
    // the sampled token is needed as an input only when nothing is forced;
    // forced runs still record it, which is workgroup 0's job alone
    const bool sample = a.p > 0 && (a.forced == nullptr || blockIdx.x == 0);
    if (sample) sample_position<FILT>(a.s, a.p - 1, tok, thr, lp);
    __syncthreads();
    if (sample && blockIdx.x == 0) record_sample<FILT>(a.s, a.p - 1, tok, thr, lp);
    int64_t t = 0;
    if (live) {
      if (a.forced != nullptr) t = a.forced[(int64_t)n * a.s.N + a.p];
      else if (a.p == 0) t = a.first[n];
      else t = tok[n];
      t = clamp_token(t, a.s.V);
    }
    xrow = a.x + t * Kx;
  }

  // K blocks of 32: [0, Kx / 32) from x and W_ih, the rest from h_{t-1} and
  // W_hh; wave w takes blocks w, w + 8, ...  Lane: weight row lane & 15 (A),
  // stream lane & 15 (B), k = 8 (lane >> 4) + 0..7 of the block in both.
  const uint16_t* xr = xrow + kq * 8;
  const uint16_t* hr = a.hprev + (int64_t)par * H + kq * 8;
  const int nkx = Kx / 32, nkb = nkx + H / 32;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int row = blockIdx.x * 16 + n;  // < 4H: the grid is H / 4
  const uint16_t* wxr = a.wx + (int64_t)row * Kx + kq * 8;
  const uint16_t* whr = a.wh + (int64_t)row * H + kq * 8;
#pragma unroll 8
  for (int kb = wave; kb < nkb; kb += kWaves) {
    const bool inx = kb < nkx;
    const int k = (inx ? kb : kb - nkx) * 32;
    const uint4 w = *reinterpret_cast<const uint4*>((inx ? wxr : whr) + k);
    const uint4 v = live ? *reinterpret_cast<const uint4*>((inx ? xr : hr) + k) : zero;
    acc = DT::mfma(w, v, acc);
  }
  const f32x4 z = reduce_waves(acc, red);
  if (wave != 0 || !live) return;

  // lane: unit 4 blockIdx + (lane >> 4), stream n; z[q] is gate (GRU: row slot) q of it
  const int u = blockIdx.x * 4 + kq;
  const float* bs = a.bias + 4 * u;
  const int64_t at = (int64_t)n * H + u;
  if constexpr (CELL == Cell::lstm) {
    const float gi = sigmoidf_fast(z[0] + bs[0]);
    const float gf = sigmoidf_fast(z[1] + bs[1]);
    const float gg = tanhf_fast(z[2] + bs[2]);
    const float go = sigmoidf_fast(z[3] + bs[3]);
    const float cn = fmaf(gf, a.c[(int64_t)par * H + u], gi * gg);
    a.c[at] = cn;
    a.hout[at] = DT::from_f(go * tanhf_fast(cn));
  } else {
    const float gr = sigmoidf_fast(z[0] + bs[0]);
    const float gz = sigmoidf_fast(z[1] + bs[1]);
    const float gn = tanhf_fast(fmaf(gr, z[3] + bs[3], z[2] + bs[2]));
    float hn = fmaf(gz, a.c[(int64_t)par * H + u] - gn, gn);  // h_{t-1} in fp32: the master
    // the 16-bit h is the rounding of the STORED master: without this the fp16 store is a fused
    // multiply-add-convert of its own, rounded once, and differs from it in the last place now and then
    asm volatile("" : "+v"(hn));
    a.c[at] = hn;
    a.hout[at] = DT::from_f(hn);
  }
}

struct HeadArgs {
  const uint16_t* w;   // [V, H]
  const float* bias;   // [V] or null
  const uint16_t* h;   // [B, H] the top layer's h_t
  float* scratch;      // [B, V]
  float* logits;       // [B, N, V] or null
  int B, H, V, N, p;
};

template <class DT>
__global__ __launch_bounds__(kThreads) void lstm_decode_head(const HeadArgs a) {
  __shared__ f32x4 red[kWaves][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int H = a.H;
  const bool live = n < a.B;
  const int row = blockIdx.x * 16 + n;  // vocabulary row of the A operand; the tail rows are zero operands
  const bool rowok = row < a.V;
  const uint16_t* wr = a.w + (int64_t)row * H + kq * 8;
  const uint16_t* hr = a.h + (int64_t)n * H + kq * 8;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int kb = wave; kb < H / 32; kb += kWaves) {
    const uint4 w = rowok ? *reinterpret_cast<const uint4*>(wr + kb * 32) : zero;
    const uint4 v = live ? *reinterpret_cast<const uint4*>(hr + kb * 32) : zero;
    acc = DT::mfma(w, v, acc);
  }
  const f32x4 z = reduce_waves(acc, red);
  if (wave != 0 || !live) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = blockIdx.x * 16 + kq * 4 + i;
    if (v >= a.V) break;
    const float y = z[i] + (a.bias != nullptr ? a.bias[v] : 0.f);
    a.scratch[(int64_t)n * a.V + v] = y;
    if (a.logits != nullptr) a.logits[((int64_t)n * a.N + a.p) * a.V + v] = y;
  }
}

// The last token: sampled from the last position's logits, recorded, fed to nothing.
template <bool FILT>
__global__ __launch_bounds__(kThreads) void lstm_decode_sample(const SampleArgs s) {
  __shared__ int tok[kStreams];
  __shared__ float thr[FILT ? kStreams : 1], lp[FILT ? kStreams : 1];
  sample_position<FILT>(s, s.N - 1, tok, thr, lp);
  __syncthreads();
  record_sample<FILT>(s, s.N - 1, tok, thr, lp);
}

// ---- the wide tile: NT = 2, 3, 4 tiles of 16 streams per launch ----------------
constexpr int kWideStreams = 4 * kStreams;
// K blocks whose loads a wave issues before their MFMAs: 4 (1 + NT) uint4s, 12 to
// 20, beside the 8 x 2 = 16 the 16-stream kernels' unroll asks for.
constexpr int kWideUnroll = 4;

// The wide kernels use plain fp32 operations only (no v_pk_*_f32; the same
// target feature lstm_bidir_infer's build flag turns off for its whole file).
// Helpers inlined into them are compiled the same way, and only an always_inline
// function is inlined into one of other features: hence the lambda's attribute
// and a barrier of their own, __syncthreads() word for word.
#if defined(__HIP_DEVICE_COMPILE__)
#define PDRNN_PLAIN_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PDRNN_PLAIN_F32
#endif

__device__ __forceinline__ void workgroup_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool FILT>
__device__ __forceinline__ void sample_position_wide(const SampleArgs& s, int p, int* tok, float* thr, float* lp) {
  if constexpr (FILT)
    with_slots(s.V, [&](auto ns) __attribute__((always_inline)) {
      sample_tokens_filtered_n<decltype(ns)::value>(s, p, tok, thr, lp);
    });
  else sample_tokens(s, p, tok);
}

struct WideSync {
  static __device__ __forceinline__ void sync() { workgroup_barrier(); }
};

// beam_select for G W in (16, 64] streams: the same two steps, the same
// arithmetic of a row and the same integer keys, over more rows and more groups
// -- step 1 is up to eight rows per wave (W rounds each), step 2 up to eight
// groups per wave (W = 1: 64 groups) -- with the wide kernels' own barrier.
__device__ __forceinline__ void beam_select_wide(const BeamArgs& b, int q, BeamCands<kWideStreams>& C,
                                                 BeamSlots<kWideStreams>& L) {
  with_slots(b.V, [&](auto ns) __attribute__((always_inline)) {
    beam_select_n<decltype(ns)::value, WideSync>(b, q, C, L);
  });
}

// The wide layer kernel's LDS.  The K loop's reduction buffer is the large
// part (8 KB a tile); a search's candidate lists (12 KB) lie in the same
// storage: the selection's last barrier comes after the last read of a list,
// and the first write of a partial sum after that barrier.
template <int NT, bool BEAM>
union WideLds {
  f32x4 red[kWaves][NT][kWave];
};
template <int NT>
union WideLds<NT, true> {
  f32x4 red[kWaves][NT][kWave];
  BeamCands<kWideStreams> cand;
};

// Every wave's NT partial accumulators into LDS; on return (after the barrier)
// wave j < NT holds tile j's sum over the waves in wave order 0..7, the order of
// reduce_waves.  The waves past NT get tile 0's and have nothing to do with it.
template <int NT>
__device__ __forceinline__ f32x4 reduce_tiles(const f32x4 (&acc)[NT], f32x4 (*red)[NT][kWave]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NT; ++j) red[wave][j][lane] = acc[j];
  workgroup_barrier();
  const int j = wave < NT ? wave : 0;
  f32x4 sum = red[0][j][lane];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) sum += red[w][j][lane];
  return sum;
}

// A wave's K blocks kb = wave, wave + 8, ... < nkb in that order into each of the
// NT accumulators: wload(kb) the weight operand, loaded once, vload(j, kb) tile
// j's.  Four blocks at a time, every load issued before the first MFMA; the
// blocks left over one by one.
template <class DT, int NT, class WL, class VL>
__device__ __forceinline__ void wide_k_loop(int nkb, f32x4 (&acc)[NT], WL wload, VL vload) {
  constexpr int U = kWideUnroll;
  int kb = threadIdx.x >> 6;
  for (; kb + (U - 1) * kWaves < nkb; kb += U * kWaves) {
    uint4 w[U], v[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u] = wload(kb + u * kWaves);
#pragma unroll
      for (int j = 0; j < NT; ++j) v[u][j] = vload(j, kb + u * kWaves);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = DT::mfma(w[u], v[u][j], acc[j]);
    }
  }
  for (; kb < nkb; kb += kWaves) {
    const uint4 w = wload(kb);
    uint4 v[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) v[j] = vload(j, kb);
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = DT::mfma(w, v[j], acc[j]);
  }
}

// lstm_decode_layer for B in (16 (NT - 1), 16 NT] streams: stream 16 j + (lane &
// 15) is column lane & 15 of tile j.  Sampling (Pick::sample, Pick::filtered) as
// there, the LDS arrays 16 NT long.
//
// Pick::beam: G groups of W beams are the B = G W streams, as in
// lstm_decode_layer, and a group may lie across a tile boundary (W = 3: group 5
// is streams 15, 16, 17).  Tile j's operand rows of h_{t-1} are then rows of
// parents that may belong to tile j - 1 or j + 1: plain row reads.  The in-place
// c (the GRU: fp32 h) is the one hazard: wave j runs tile j's epilogue, and wave
// 0 would store c[15] while wave 1 still has to load it as the parent of stream
// 16.  So every epilogue wave loads c[par] and has the value in a register (the
// empty asm that uses it makes the compiler wait for the load) BEFORE a
// workgroup barrier that all eight waves reach, and stores c[s] AFTER it: every
// load of the unit's c has completed before any store to it.  No other
// workgroup touches the unit.
template <class DT, bool FIRST, Pick PICK, Cell CELL, int NT>
__global__ __launch_bounds__(kThreads) PDRNN_PLAIN_F32 void lstm_decode_layer_wide(const LayerArgs a) {
  static_assert(FIRST || PICK != Pick::filtered, "the filter is layer 0's");
  static_assert(NT >= 2 && NT * kStreams <= kWideStreams, "2 to 4 tiles");
  constexpr bool FILT = PICK == Pick::filtered, BEAM = PICK == Pick::beam;
  constexpr int NS = NT * kStreams;
  __shared__ WideLds<NT, BEAM> lds;
  auto& red = lds.red;
  __shared__ int tok[BEAM ? 1 : NS];
  __shared__ float thr[FILT ? NS : 1], lp[FILT ? NS : 1];
  __shared__ BeamSlots<BEAM && FIRST ? kWideStreams : 1> slots;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int B = a.s.B, H = a.H, Kx = a.Kx;

  if constexpr (BEAM && FIRST) {
    if (a.p > 0) {
      beam_select_wide(a.b, a.p - 1, lds.cand, slots);
      if (blockIdx.x == 0) beam_record(a.b, a.p - 1, slots);
    }
  } else if constexpr (FIRST) {
    const bool sample = a.p > 0 && (a.forced == nullptr || blockIdx.x == 0);
    if (sample) sample_position_wide<FILT>(a.s, a.p - 1, tok, thr, lp);
    workgroup_barrier();
    if (sample && blockIdx.x == 0) record_sample<FILT>(a.s, a.p - 1, tok, thr, lp);
  }
  // Tile j's operand rows of this lane.  A padding stream reads stream B - 1's
  // rows: every load is then unconditional (a guarded uint4 load, also one whose
  // value a select replaces by zero, compiles to four dword loads behind four
  // branches here).  An MFMA column depends on its own B column alone and a
  // padding column is never stored, so what it holds reaches nothing.
  const uint16_t* xr[NT];
  const uint16_t* hr[NT];
  bool live[NT];
  int pe = 0;  // Pick::beam: the parent of this lane's epilogue stream 16 wave + n
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    live[j] = j * kStreams + n < B;
    const int s = live[j] ? j * kStreams + n : B - 1;
    int par = s;  // the stream whose state stream s continues (a padding stream: stream B - 1's)
    const uint16_t* xrow = a.x + (int64_t)s * Kx;
    if constexpr (BEAM && FIRST) {
      int64_t t = a.first[s];
      if (a.p > 0) t = slots.tok[s], par = slots.parent[s];
      xrow = a.x + clamp_token(t, a.s.V) * Kx;
    } else if constexpr (BEAM) {
      if (a.p > 0) par = a.b.parents[(int64_t)s * a.b.N + a.p - 1];
    } else if constexpr (FIRST) {
      int64_t t = 0;
      if (live[j]) {
        if (a.forced != nullptr) t = a.forced[(int64_t)s * a.s.N + a.p];
        else if (a.p == 0) t = a.first[s];
        else t = tok[s];
        t = clamp_token(t, a.s.V);
      }
      xrow = a.x + t * Kx;
    }
    if constexpr (BEAM) {
      par = beam_parent(par, s, a.b.W);
      if (wave == j) pe = par;
    }
    xr[j] = xrow + kq * 8;
    hr[j] = a.hprev + (int64_t)par * H + kq * 8;
  }

  // the K blocks as in lstm_decode_layer: one weight load, NT operand loads, NT MFMAs
  const int nkx = Kx / 32, nkb = nkx + H / 32;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int row = blockIdx.x * 16 + n;  // < 4H: the grid is H / 4
  const uint16_t* wxr = a.wx + (int64_t)row * Kx + kq * 8;
  const uint16_t* whr = a.wh + (int64_t)row * H + kq * 8;
  wide_k_loop<DT, NT>(
      nkb, acc,
      [&](int kb) __attribute__((always_inline)) {
        return *reinterpret_cast<const uint4*>(kb < nkx ? wxr + kb * 32 : whr + (kb - nkx) * 32);
      },
      [&](int j, int kb) __attribute__((always_inline)) {
        return *reinterpret_cast<const uint4*>(kb < nkx ? xr[j] + kb * 32 : hr[j] + (kb - nkx) * 32);
      });
  const f32x4 z = reduce_tiles<NT>(acc, red);
  const int s = wave * kStreams + n;  // wave j < NT: tile j's epilogue
  const bool mine = wave < NT && s < B;
  float cpar = 0.f;  // Pick::beam: the parent's c (the GRU: fp32 h)
  if constexpr (BEAM) {
    // which another wave's tile may hold: loaded, and arrived, before the barrier that every
    // wave reaches; the stores below come after it (see above the kernel)
    if (mine) cpar = a.c[(int64_t)pe * H + blockIdx.x * 4 + kq];
    asm volatile("" : "+v"(cpar));
    workgroup_barrier();
  }
  if (!mine) return;

  // lane: unit 4 blockIdx + (lane >> 4), stream s; the cell exactly as in lstm_decode_layer
  const int u = blockIdx.x * 4 + kq;
  const float* bs = a.bias + 4 * u;
  const int64_t at = (int64_t)s * H + u;
  const float cp = BEAM ? cpar : a.c[at];  // c (the GRU: fp32 h) entering the position
  if constexpr (CELL == Cell::lstm) {
    const float gi = sigmoidf_fast(z[0] + bs[0]);
    const float gf = sigmoidf_fast(z[1] + bs[1]);
    const float gg = tanhf_fast(z[2] + bs[2]);
    const float go = sigmoidf_fast(z[3] + bs[3]);
    const float cn = fmaf(gf, cp, gi * gg);
    a.c[at] = cn;
    a.hout[at] = DT::from_f(go * tanhf_fast(cn));
  } else {
    const float gr = sigmoidf_fast(z[0] + bs[0]);
    const float gz = sigmoidf_fast(z[1] + bs[1]);
    const float gn = tanhf_fast(fmaf(gr, z[3] + bs[3], z[2] + bs[2]));
    float hn = fmaf(gz, cp - gn, gn);
    asm volatile("" : "+v"(hn));  // (the 16-bit h is the rounding of the stored master, as there)
    a.c[at] = hn;
    a.hout[at] = DT::from_f(hn);
  }
}

template <class DT, int NT>
__global__ __launch_bounds__(kThreads) PDRNN_PLAIN_F32 void lstm_decode_head_wide(const HeadArgs a) {
  __shared__ f32x4 red[kWaves][NT][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kq = lane >> 4;
  const int H = a.H;
  // vocabulary row of the A operand; the rows past V read row V - 1 and the padding streams stream B - 1
  // (unconditional loads, as in the layer kernel: an output row or column that is never stored)
  const int row = min(blockIdx.x * 16 + n, a.V - 1);
  const uint16_t* wr = a.w + (int64_t)row * H + kq * 8;
  const uint16_t* hr[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) hr[j] = a.h + (int64_t)min(j * kStreams + n, a.B - 1) * H + kq * 8;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  wide_k_loop<DT, NT>(
      H / 32, acc,
      [&](int kb) __attribute__((always_inline)) { return *reinterpret_cast<const uint4*>(wr + kb * 32); },
      [&](int j, int kb) __attribute__((always_inline)) { return *reinterpret_cast<const uint4*>(hr[j] + kb * 32); });
  const f32x4 z = reduce_tiles<NT>(acc, red);
  const int s = wave * kStreams + n;
  if (wave >= NT || s >= a.B) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = blockIdx.x * 16 + kq * 4 + i;
    if (v >= a.V) break;
    const float y = z[i] + (a.bias != nullptr ? a.bias[v] : 0.f);
    a.scratch[(int64_t)s * a.V + v] = y;
    if (a.logits != nullptr) a.logits[((int64_t)s * a.N + a.p) * a.V + v] = y;
  }
}

// lstm_decode_sample for up to 64 streams
template <bool FILT>
__global__ __launch_bounds__(kThreads) PDRNN_PLAIN_F32 void lstm_decode_sample_wide(const SampleArgs s) {
  __shared__ int tok[kWideStreams];
  __shared__ float thr[FILT ? kWideStreams : 1], lp[FILT ? kWideStreams : 1];
  sample_position_wide<FILT>(s, s.N - 1, tok, thr, lp);
  workgroup_barrier();
  record_sample<FILT>(s, s.N - 1, tok, thr, lp);
}

// Selection q as a launch of its own (one workgroup): the one after the last
// position.  hyp != null: the parents are then traced back, a thread per final
// slot, into hyp [S, N] (and hyp_lp from lp), the last column from LDS.
__global__ __launch_bounds__(kThreads) void lstm_decode_beam_pick(const BeamArgs b, int q, int64_t* hyp, float* hyp_lp) {
  __shared__ BeamLds L;
  beam_select(b, q, L);
  beam_record(b, q, L.s);
  const int S = b.G * b.W, i = threadIdx.x;
  if (hyp == nullptr || i >= S) return;
  int at = i;
  for (int k = q; k >= 0; --k) {
    const int64_t src = (int64_t)at * b.N + k, dst = (int64_t)i * b.N + k;
    hyp[dst] = k == q ? L.s.tok[at] : b.tokens[src];
    if (hyp_lp != nullptr) hyp_lp[dst] = k == q ? L.s.lp[at] : b.lp[src];
    at = beam_parent(k == q ? L.s.parent[at] : b.parents[src], at, b.W);
  }
}

// lstm_decode_beam_pick for up to 64 final slots (the same lines: written once as a shared
// helper they changed the 16-stream kernel's code)
__global__ __launch_bounds__(kThreads) PDRNN_PLAIN_F32 void lstm_decode_beam_pick_wide(const BeamArgs b, int q, int64_t* hyp,
                                                                                        float* hyp_lp) {
  __shared__ BeamLdsOf<kWideStreams> L;
  beam_select_wide(b, q, L.c, L.s);
  beam_record(b, q, L.s);
  const int S = b.G * b.W, i = threadIdx.x;
  if (hyp == nullptr || i >= S) return;
  int at = i;
  for (int k = q; k >= 0; --k) {
    const int64_t src = (int64_t)at * b.N + k, dst = (int64_t)i * b.N + k;
    hyp[dst] = k == q ? L.s.tok[at] : b.tokens[src];
    if (hyp_lp != nullptr) hyp_lp[dst] = k == q ? L.s.lp[at] : b.lp[src];
    at = beam_parent(k == q ? L.s.parent[at] : b.parents[src], at, b.W);
  }
}

// The token loop of both modes: per position the layer-0 kernel of the mode,
// the layers above and the head, L + 1 launches on the one stream.  k arrives
// with the mode's part (s, b, forced) filled in; the caller enqueues the
// mode's last launch.  NT > 1: the wide kernels of NT stream tiles, the same grids.
template <class DT, Pick PICK, Cell CELL, int NT>
hipError_t decode_positions_of(const PdrnnLstmDecodeStack& a, int n_tokens, LayerArgs k, hipStream_t stream) {
  constexpr Pick ABOVE = PICK == Pick::beam ? Pick::beam : Pick::sample;
  const int B = a.B, H = a.H, V = a.V, L = a.L;
  const uint16_t* h = static_cast<const uint16_t*>(a.h);
  uint16_t* hm = static_cast<uint16_t*>(a.h);
  const int64_t BH = (int64_t)B * H, slot = (int64_t)L * BH;
  k.first = a.first;
  k.H = H;
  for (int p = 0; p < n_tokens; ++p) {
    const int64_t in = (p & 1) * slot, out = ((p + 1) & 1) * slot;  // h_{t-1} and h_t of every layer
    k.p = p;
    for (int l = 0; l < L; ++l) {
      k.wx = static_cast<const uint16_t*>(a.w_ih[l]);
      k.wh = static_cast<const uint16_t*>(a.w_hh[l]);
      k.bias = a.bias[l];
      k.x = l == 0 ? static_cast<const uint16_t*>(a.emb) : h + out + (l - 1) * BH;
      k.hprev = h + in + l * BH;
      k.hout = hm + out + l * BH;
      k.c = a.c + l * BH;
      k.Kx = l == 0 ? a.E : H;
      if constexpr (NT == 1) {
        if (l == 0) lstm_decode_layer<DT, true, PICK, CELL><<<H / 4, kThreads, 0, stream>>>(k);
        else lstm_decode_layer<DT, false, ABOVE, CELL><<<H / 4, kThreads, 0, stream>>>(k);
      } else {
        if (l == 0) lstm_decode_layer_wide<DT, true, PICK, CELL, NT><<<H / 4, kThreads, 0, stream>>>(k);
        else lstm_decode_layer_wide<DT, false, ABOVE, CELL, NT><<<H / 4, kThreads, 0, stream>>>(k);
      }
      PDRNN_HIP_CHECK(hipGetLastError());
    }
    const HeadArgs hd{static_cast<const uint16_t*>(a.w_fc), a.b_fc, h + out + (L - 1) * BH, a.scratch, a.logits,
                      B, H, V, n_tokens, p};
    if constexpr (NT == 1) lstm_decode_head<DT><<<(V + 15) / 16, kThreads, 0, stream>>>(hd);
    else lstm_decode_head_wide<DT, NT><<<(V + 15) / 16, kThreads, 0, stream>>>(hd);
    PDRNN_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

template <class DT, Pick PICK, int NT = 1>
hipError_t decode_positions(const PdrnnLstmDecodeStack& a, int n_tokens, const LayerArgs& k, hipStream_t stream) {
  switch (a.cell) {
    case 0: return decode_positions_of<DT, PICK, Cell::lstm, NT>(a, n_tokens, k, stream);
    case 1: return decode_positions_of<DT, PICK, Cell::gru, NT>(a, n_tokens, k, stream);
  }
  return hipErrorInvalidValue;
}

// the stack's limits by its cell
int stack_supported(const PdrnnLstmDecodeStack& st) {
  if (st.cell == 0) return pdrnn_lstm_decode_supported(st.B, st.H, st.E, st.V, st.L, st.dtype);
  return st.cell == 1 && pdrnn_gru_decode_supported(st.B, st.H, st.E, st.V, st.L, st.dtype);
}

template <class DT, int NT = 1>
hipError_t decode_beam(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  LayerArgs k{};
  k.b = BeamArgs{st.scratch, a->cum, a->done, a->tokens, a->parents, a->lp, a->G, a->W, st.V, n_tokens, a->stop};
  k.s.B = st.B;
  k.s.V = st.V;
  k.s.N = n_tokens;
  PDRNN_HIP_CHECK((decode_positions<DT, Pick::beam, NT>(st, n_tokens, k, stream)));
  if constexpr (NT == 1) lstm_decode_beam_pick<<<1, kThreads, 0, stream>>>(k.b, n_tokens - 1, a->hyp, a->hyp_lp);
  else lstm_decode_beam_pick_wide<<<1, kThreads, 0, stream>>>(k.b, n_tokens - 1, a->hyp, a->hyp_lp);
  return hipGetLastError();
}

// the wide search by its tile count NT = ceil(G W / 16)
template <class DT>
hipError_t decode_beam_wide(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  switch ((a->stack.B + kStreams - 1) / kStreams) {
    case 2: return decode_beam<DT, 2>(a, n_tokens, stream);
    case 3: return decode_beam<DT, 3>(a, n_tokens, stream);
    case 4: return decode_beam<DT, 4>(a, n_tokens, stream);
  }
  return hipErrorInvalidValue;
}

template <class DT, int NT = 1>
hipError_t decode(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  const bool top_k = a->top_k > 0 && a->top_k < st.V, top_p = a->top_p > 0.f && a->top_p < 1.f;
  // the filtered sampler only where it has something to do: a filter at T > 0, or an output to fill
  const bool filt = (a->temperature != 0.f && (top_k || top_p)) || a->threshold != nullptr || a->logprobs != nullptr;
  LayerArgs k{};
  k.s = SampleArgs{st.scratch, a->tokens, st.B, st.V, n_tokens, a->temperature, a->seed, a->stream0, a->pos0,
                   top_k ? a->top_k : 0, top_p ? a->top_p : 0.f, a->threshold, a->logprobs};
  k.forced = a->forced;
  PDRNN_HIP_CHECK(filt ? (decode_positions<DT, Pick::filtered, NT>(st, n_tokens, k, stream))
                       : (decode_positions<DT, Pick::sample, NT>(st, n_tokens, k, stream)));
  if constexpr (NT == 1) {
    if (filt) lstm_decode_sample<true><<<1, kThreads, 0, stream>>>(k.s);
    else lstm_decode_sample<false><<<1, kThreads, 0, stream>>>(k.s);
  } else {
    if (filt) lstm_decode_sample_wide<true><<<1, kThreads, 0, stream>>>(k.s);
    else lstm_decode_sample_wide<false><<<1, kThreads, 0, stream>>>(k.s);
  }
  return hipGetLastError();
}

// the wide call by its tile count NT = ceil(B / 16)
template <class DT>
hipError_t decode_wide(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  switch ((a->stack.B + kStreams - 1) / kStreams) {
    case 2: return decode<DT, 2>(a, n_tokens, stream);
    case 3: return decode<DT, 3>(a, n_tokens, stream);
    case 4: return decode<DT, 4>(a, n_tokens, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace
}  // namespace pdrnn

extern "C" {

int pdrnn_lstm_decode_supported(int B, int H, int E, int V, int L, int dtype) {
  return B >= 1 && B <= pdrnn::kStreams && pdrnn_lstm_large_supported(H) && E >= 32 && E % 32 == 0 && V >= 1 &&
         V <= 1024 && L >= 1 && (dtype == 0 || dtype == 1);
}

// the GRU stack goes through the same tile: the same limits
int pdrnn_gru_decode_supported(int B, int H, int E, int V, int L, int dtype) {
  return pdrnn_lstm_decode_supported(B, H, E, V, L, dtype);
}

int pdrnn_gru_decode_beam_supported(int G, int W, int H, int E, int V, int L, int dtype) {
  return pdrnn_lstm_decode_beam_supported(G, W, H, E, V, L, dtype) && pdrnn_gru_decode_supported(G * W, H, E, V, L, dtype);
}

hipError_t pdrnn_lstm_decode(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  if (n_tokens < 1 || !pdrnn::stack_supported(st)) return hipErrorInvalidValue;
  if (!(a->temperature >= 0.f) || a->top_k < 0 || !(a->top_p >= 0.f)) return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode<pdrnn::BF16>(a, n_tokens, stream) : pdrnn::decode<pdrnn::F16>(a, n_tokens, stream);
}

// 17 to 64 streams through the wide kernels; every other limit is the 16-stream predicate's
int pdrnn_lstm_decode_wide_supported(int B, int H, int E, int V, int L, int dtype) {
  return B > pdrnn::kStreams && B <= pdrnn::kWideStreams && pdrnn_lstm_decode_supported(pdrnn::kStreams, H, E, V, L, dtype);
}

int pdrnn_gru_decode_wide_supported(int B, int H, int E, int V, int L, int dtype) {
  return B > pdrnn::kStreams && B <= pdrnn::kWideStreams && pdrnn_gru_decode_supported(pdrnn::kStreams, H, E, V, L, dtype);
}

hipError_t pdrnn_lstm_decode_wide(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  const bool fits = st.cell == 0   ? pdrnn_lstm_decode_wide_supported(st.B, st.H, st.E, st.V, st.L, st.dtype)
                    : st.cell == 1 ? pdrnn_gru_decode_wide_supported(st.B, st.H, st.E, st.V, st.L, st.dtype)
                                   : 0;
  if (n_tokens < 1 || !fits) return hipErrorInvalidValue;
  if (!(a->temperature >= 0.f) || a->top_k < 0 || !(a->top_p >= 0.f)) return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode_wide<pdrnn::BF16>(a, n_tokens, stream)
                       : pdrnn::decode_wide<pdrnn::F16>(a, n_tokens, stream);
}

hipError_t pdrnn_gru_decode_wide(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  return a->stack.cell == 1 ? pdrnn_lstm_decode_wide(a, n_tokens, stream) : hipErrorInvalidValue;
}

int pdrnn_lstm_decode_beam_supported(int G, int W, int H, int E, int V, int L, int dtype) {
  return G >= 1 && W >= 1 && W <= pdrnn::kStreams && G <= pdrnn::kStreams && G * W <= pdrnn::kStreams &&
         pdrnn_lstm_decode_supported(G * W, H, E, V, L, dtype);
}

hipError_t pdrnn_lstm_decode_beam(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  if (n_tokens < 1 || !pdrnn_lstm_decode_beam_supported(a->G, a->W, st.H, st.E, st.V, st.L, st.dtype) ||
      st.B != a->G * a->W || !pdrnn::stack_supported(st))
    return hipErrorInvalidValue;
  if (a->stop < -1 || a->stop >= st.V || (a->hyp_lp != nullptr && a->lp == nullptr) || a->hyp == nullptr)
    return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode_beam<pdrnn::BF16>(a, n_tokens, stream)
                       : pdrnn::decode_beam<pdrnn::F16>(a, n_tokens, stream);
}

// 17 to 64 streams of groups of up to 16 beams; every other limit is the wide decode predicate's
int pdrnn_lstm_decode_beam_wide_supported(int G, int W, int H, int E, int V, int L, int dtype) {
  return G >= 1 && W >= 1 && W <= pdrnn::kStreams && G <= pdrnn::kWideStreams && G * W <= pdrnn::kWideStreams &&
         pdrnn_lstm_decode_wide_supported(G * W, H, E, V, L, dtype);
}

int pdrnn_gru_decode_beam_wide_supported(int G, int W, int H, int E, int V, int L, int dtype) {
  return pdrnn_lstm_decode_beam_wide_supported(G, W, H, E, V, L, dtype) &&
         pdrnn_gru_decode_wide_supported(G * W, H, E, V, L, dtype);
}

hipError_t pdrnn_lstm_decode_beam_wide(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  const bool fits = st.cell == 0   ? pdrnn_lstm_decode_beam_wide_supported(a->G, a->W, st.H, st.E, st.V, st.L, st.dtype)
                    : st.cell == 1 ? pdrnn_gru_decode_beam_wide_supported(a->G, a->W, st.H, st.E, st.V, st.L, st.dtype)
                                   : 0;
  if (n_tokens < 1 || !fits || st.B != a->G * a->W) return hipErrorInvalidValue;
  if (a->stop < -1 || a->stop >= st.V || (a->hyp_lp != nullptr && a->lp == nullptr) || a->hyp == nullptr)
    return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode_beam_wide<pdrnn::BF16>(a, n_tokens, stream)
                       : pdrnn::decode_beam_wide<pdrnn::F16>(a, n_tokens, stream);
}

hipError_t pdrnn_lstm_decode_beam_select(const float* logits, float* cum, int32_t* done, int64_t* tokens,
                                         int32_t* parents, float* lp, int G, int W, int V, int stop,
                                         hipStream_t stream) {
  if (G < 1 || W < 1 || G > pdrnn::kStreams || W > pdrnn::kStreams || G * W > pdrnn::kStreams || V < 1 || V > 1024 ||
      stop < -1 || stop >= V)
    return hipErrorInvalidValue;
  const pdrnn::BeamArgs b{logits, cum, done, tokens, parents, lp, G, W, V, 1, stop};
  pdrnn::lstm_decode_beam_pick<<<1, pdrnn::kThreads, 0, stream>>>(b, 0, nullptr, nullptr);
  return hipGetLastError();
}

}  // extern "C"
