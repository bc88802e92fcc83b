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
// Reference semantics: torch.nn.Embedding + nn.LSTM (gate order i, f, g, o) +
// nn.Linear stepped one token at a time.
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

struct BeamLds {
  uint32_t ck[kStreams][kStreams];  // a stream's W best candidates in rank order: score keys (0: none),
  int cv[kStreams][kStreams];       // tokens
  float cl[kStreams][kStreams];     // and log-probs
  int parent[kStreams], tok[kStreams], done[kStreams];  // the new slots
  float cum[kStreams], lp[kStreams];
};

// One selection, by every lane of the workgroup; the new slots end in L.
//   1. A wave per stream, the row in registers as in sample_tokens_filtered_n:
//      log-softmax, score keys, then the row's W best in rank order by W rounds
//      of (wave max of the keys, first holder by ballots: the lowest slot, then
//      the lowest lane, is the lowest v), into LDS.  A stream contributes at
//      most W winners, and they are among these.
//   2. A wave per group: lane j < W holds the head of stream j's list; W rounds
//      of (wave max of the heads, the lowest lane holding it) merge them.
// Integer keys, ballots and fixed-order sums: the same bits in every workgroup.
template <int NS>
__device__ __forceinline__ void beam_select_n(const BeamArgs& b, int q, BeamLds& L) {
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
        L.ck[s][r] = mx;
        L.cv[s][r] = wv;
        L.cl[s][r] = wl;
      }
    }
  }
  __syncthreads();
  for (int g = wave; g < b.G; g += kWaves) {
    const int s = g * W + (lane < W ? lane : 0);
    int head = 0;
#pragma unroll 1
    for (int i = 0; i < W; ++i) {
      const uint32_t k = lane < W && head < W ? L.ck[s][head] : 0;
      const uint32_t mx = wave_reduce<Max>(k);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(lane < W && k == mx);
      const int j = __builtin_ctzll(bal);  // (a group always has W candidates: lane 0 at the worst)
      PDRNN_DEVICE_ASSERT(mx != 0);
      if (lane == j) {
        const int slot = g * W + i, v = head < W ? L.cv[s][head] : 0;
        L.parent[slot] = s;
        L.tok[slot] = v;
        L.cum[slot] = mx != 0 ? decode_key_value(mx) : -INFINITY;
        L.lp[slot] = head < W ? L.cl[s][head] : 0.f;
        L.done[slot] = done[s] != 0 || v == b.stop;
        ++head;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void beam_select(const BeamArgs& b, int q, BeamLds& L) {
  with_slots(b.V, [&](auto ns) { beam_select_n<decltype(ns)::value>(b, q, L); });
}

// selection q's record (one workgroup's job)
__device__ __forceinline__ void beam_record(const BeamArgs& b, int q, const BeamLds& L) {
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
  const uint16_t* wx;     // [4H, Kx] gate-interleaved rows 4u + q
  const uint16_t* wh;     // [4H, H]
  const float* bias;      // [4H] b_ih + b_hh, interleaved
  const uint16_t* x;      // FIRST: the embedding [V, Kx]; else the layer below's h_t [B, Kx]
  const uint16_t* hprev;  // [B, H]
  uint16_t* hout;         // [B, H]
  float* c;               // [B, H], updated in place
  const int64_t* first;   // FIRST: [B] input tokens of position 0
  const int64_t* forced;  // FIRST: [B, N] input tokens of every position, or null
  SampleArgs s;
  int H, Kx, p;
  BeamArgs b;             // Pick::beam: the search (s: B, V and N only)
};

// How position p's input token is chosen in layer 0.  The layers above read
// only "beam or not" from it: they exist for sample and beam.
enum class Pick { sample, filtered, beam };

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
// position: it reads h_{t-1} and c of par in every layer (x of a layer above 0
// is the layer below's h_t, already in new-slot order).  Layer 0 selects
// (beam_select; by every workgroup, recorded by workgroup 0); the layers above
// read the record.  c stays in place: a unit's 16 streams are 16 lanes of wave
// 0 of one workgroup, which loads c[par] in one instruction and stores c[n] in
// a later one that depends on the loaded value, so every lane's load has
// completed before any lane's store; no other workgroup touches the unit.
//
// Every __syncthreads() below is reached by all threads of a workgroup: what
// guards the sampling and the selection (p, forced, blockIdx) is uniform in it.
template <class DT, bool FIRST, Pick PICK>
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
      if (blockIdx.x == 0) beam_record(a.b, a.p - 1, L);
    }
    int64_t t = 0;
    if (live) {
      if (a.p == 0) t = a.first[n];
      else t = L.tok[n], par = L.parent[n];
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
  const int row = blockIdx.x * 16 + n;  // < 4H: the grid is H / 4
  const uint16_t* wxr = a.wx + (int64_t)row * Kx + kq * 8;
  const uint16_t* whr = a.wh + (int64_t)row * H + kq * 8;
  const uint16_t* xr = xrow + kq * 8;
  const uint16_t* hr = a.hprev + (int64_t)par * H + kq * 8;
  const int nkx = Kx / 32, nkb = nkx + H / 32;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
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

  // lane: unit 4 blockIdx + (lane >> 4), stream n; z[q] is gate q of it
  const int u = blockIdx.x * 4 + kq;
  const float* bs = a.bias + 4 * u;
  const float gi = sigmoidf_fast(z[0] + bs[0]);
  const float gf = sigmoidf_fast(z[1] + bs[1]);
  const float gg = tanhf_fast(z[2] + bs[2]);
  const float go = sigmoidf_fast(z[3] + bs[3]);
  const int64_t at = (int64_t)n * H + u;
  const float cn = fmaf(gf, a.c[(int64_t)par * H + u], gi * gg);
  a.c[at] = cn;
  a.hout[at] = DT::from_f(go * tanhf_fast(cn));
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

// Selection q as a launch of its own (one workgroup): the one after the last
// position.  hyp != null: the parents are then traced back, a thread per final
// slot, into hyp [S, N] (and hyp_lp from lp), the last column from LDS.
__global__ __launch_bounds__(kThreads) void lstm_decode_beam_pick(const BeamArgs b, int q, int64_t* hyp, float* hyp_lp) {
  __shared__ BeamLds L;
  beam_select(b, q, L);
  beam_record(b, q, L);
  const int S = b.G * b.W, i = threadIdx.x;
  if (hyp == nullptr || i >= S) return;
  int at = i;
  for (int k = q; k >= 0; --k) {
    const int64_t src = (int64_t)at * b.N + k, dst = (int64_t)i * b.N + k;
    hyp[dst] = k == q ? L.tok[at] : b.tokens[src];
    if (hyp_lp != nullptr) hyp_lp[dst] = k == q ? L.lp[at] : b.lp[src];
    at = beam_parent(k == q ? L.parent[at] : b.parents[src], at, b.W);
  }
}

// The token loop of both modes: per position the layer-0 kernel of the mode,
// the layers above and the head, L + 1 launches on the one stream.  k arrives
// with the mode's part (s, b, forced) filled in; the caller enqueues the
// mode's last launch.
template <class DT, Pick PICK>
hipError_t decode_positions(const PdrnnLstmDecodeStack& a, int n_tokens, LayerArgs k, hipStream_t stream) {
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
      if (l == 0) lstm_decode_layer<DT, true, PICK><<<H / 4, kThreads, 0, stream>>>(k);
      else lstm_decode_layer<DT, false, ABOVE><<<H / 4, kThreads, 0, stream>>>(k);
      PDRNN_HIP_CHECK(hipGetLastError());
    }
    const HeadArgs hd{static_cast<const uint16_t*>(a.w_fc), a.b_fc, h + out + (L - 1) * BH, a.scratch, a.logits,
                      B, H, V, n_tokens, p};
    lstm_decode_head<DT><<<(V + 15) / 16, kThreads, 0, stream>>>(hd);
    PDRNN_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

template <class DT>
hipError_t decode_beam(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  LayerArgs k{};
  k.b = BeamArgs{st.scratch, a->cum, a->done, a->tokens, a->parents, a->lp, a->G, a->W, st.V, n_tokens, a->stop};
  k.s.B = st.B;
  k.s.V = st.V;
  k.s.N = n_tokens;
  PDRNN_HIP_CHECK((decode_positions<DT, Pick::beam>(st, n_tokens, k, stream)));
  lstm_decode_beam_pick<<<1, kThreads, 0, stream>>>(k.b, n_tokens - 1, a->hyp, a->hyp_lp);
  return hipGetLastError();
}

template <class DT>
hipError_t decode(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  const bool top_k = a->top_k > 0 && a->top_k < st.V, top_p = a->top_p > 0.f && a->top_p < 1.f;
  // the filtered sampler only where it has something to do: a filter at T > 0, or an output to fill
  const bool filt = (a->temperature != 0.f && (top_k || top_p)) || a->threshold != nullptr || a->logprobs != nullptr;
  LayerArgs k{};
  k.s = SampleArgs{st.scratch, a->tokens, st.B, st.V, n_tokens, a->temperature, a->seed, a->stream0, a->pos0,
                   top_k ? a->top_k : 0, top_p ? a->top_p : 0.f, a->threshold, a->logprobs};
  k.forced = a->forced;
  PDRNN_HIP_CHECK(filt ? (decode_positions<DT, Pick::filtered>(st, n_tokens, k, stream))
                       : (decode_positions<DT, Pick::sample>(st, n_tokens, k, stream)));
  if (filt) lstm_decode_sample<true><<<1, kThreads, 0, stream>>>(k.s);
  else lstm_decode_sample<false><<<1, kThreads, 0, stream>>>(k.s);
  return hipGetLastError();
}

}  // namespace
}  // namespace pdrnn

extern "C" {

int pdrnn_lstm_decode_supported(int B, int H, int E, int V, int L, int dtype) {
  return B >= 1 && B <= pdrnn::kStreams && pdrnn_lstm_large_supported(H) && E >= 32 && E % 32 == 0 && V >= 1 &&
         V <= 1024 && L >= 1 && (dtype == 0 || dtype == 1);
}

hipError_t pdrnn_lstm_decode(const PdrnnLstmDecodeArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  if (n_tokens < 1 || !pdrnn_lstm_decode_supported(st.B, st.H, st.E, st.V, st.L, st.dtype)) return hipErrorInvalidValue;
  if (!(a->temperature >= 0.f) || a->top_k < 0 || !(a->top_p >= 0.f)) return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode<pdrnn::BF16>(a, n_tokens, stream) : pdrnn::decode<pdrnn::F16>(a, n_tokens, stream);
}

int pdrnn_lstm_decode_beam_supported(int G, int W, int H, int E, int V, int L, int dtype) {
  return G >= 1 && W >= 1 && W <= pdrnn::kStreams && G <= pdrnn::kStreams && G * W <= pdrnn::kStreams &&
         pdrnn_lstm_decode_supported(G * W, H, E, V, L, dtype);
}

hipError_t pdrnn_lstm_decode_beam(const PdrnnLstmDecodeBeamArgs* a, int n_tokens, hipStream_t stream) {
  const PdrnnLstmDecodeStack& st = a->stack;
  if (n_tokens < 1 || !pdrnn_lstm_decode_beam_supported(a->G, a->W, st.H, st.E, st.V, st.L, st.dtype) ||
      st.B != a->G * a->W)
    return hipErrorInvalidValue;
  if (a->stop < -1 || a->stop >= st.V || (a->hyp_lp != nullptr && a->lp == nullptr) || a->hyp == nullptr)
    return hipErrorInvalidValue;
  return st.dtype == 0 ? pdrnn::decode_beam<pdrnn::BF16>(a, n_tokens, stream)
                       : pdrnn::decode_beam<pdrnn::F16>(a, n_tokens, stream);
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
