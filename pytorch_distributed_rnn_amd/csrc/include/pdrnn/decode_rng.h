// The sampling rule of the char-LM decode path, written once: the kernels
// (kernels/lstm_decode.hip) include it, ops/decode.py:gumbel_noise mirrors it
// step for step.  Below it the filter rule and the beam-search rule.
//
// Gumbel-max: token = argmax_v(logit_v / temperature + g_v), g_v = -log(-log u_v)
// with u_v uniform in (0, 1), samples softmax(logits / temperature) with no
// normalisation and no prefix sum.  u_v comes from a stateless counter hash of
// (seed, stream, position, v), so every workgroup can draw the same token on
// its own and a stream's draws do not depend on which other streams share the
// launch.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDRNN_RNG_FN __host__ __device__ inline
#else
#define PDRNN_RNG_FN inline
#endif

namespace pdrnn {

// 32-bit finaliser (the "lowbias32" constants): every input bit reaches every
// output bit, so consecutive v give unrelated words.
PDRNN_RNG_FN uint32_t decode_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the part of the hash shared by all v of one (seed, stream, position)
PDRNN_RNG_FN uint32_t decode_key(uint32_t seed, uint32_t stream, uint32_t pos) {
  uint32_t h = decode_mix(seed + 0x9e3779b9u);
  h = decode_mix(h ^ (stream * 0x85ebca6bu));
  return decode_mix(h ^ (pos * 0xc2b2ae35u));
}

PDRNN_RNG_FN uint32_t decode_word(uint32_t key, uint32_t v) { return decode_mix(key ^ v); }

// u = ((r >> 8) + 0.5) 2^-24 in fp32.  The sum is rounded to 24 bits, so the
// top word would give exactly 1 and an infinite g: u is held at the largest
// float below 1 (g <= 16.64).  The smallest u is 2^-25 (g >= -2.86).
PDRNN_RNG_FN float decode_uniform(uint32_t r) {
  const float u = ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-08f;
  return u < 0.99999994f ? u : 0.99999994f;
}

// ---- top-k and nucleus filtering --------------------------------------------
// Gumbel-max needs no sorted distribution: a filter is a per-row threshold tau,
// token = argmax over {v : l_v >= tau} of l_v / T + g_v, with g_v the noise
// above, drawn for the same v whatever the filter (ops/decode.py:keep_threshold
// mirrors the rule).  For fp32 logits l_v, temperature T > 0, top_k, top_p:
//   1. top-k on the raw logits: tau_k = the k-th largest l_v counted with
//      multiplicity (top_k = 0 or >= V: off, tau_k = -inf).  l_v >= tau_k is
//      kept: everything tied with the k-th survives, no index tie-break.
//   2. top-p over those survivors, renormalised: y_v = l_v / T, w_v =
//      exp(y_v - max y); tau_p = the largest logit value tau with
//      sum{w_v : l_v >= tau} >= top_p * sum{w_v : l_v >= tau_k}  (top_p = 0 or
//      >= 1: off).  Ties at the boundary are all kept.
//   3. tau = max(tau_k, tau_p), the smallest kept logit (-inf: both off).
//   4. log-prob of the drawn token: y_tok - max y - log(sum{w_v : l_v >= tau}).
//   5. Temperature 0 (greedy) ignores both filters; its log-prob is the
//      argmax's under T = 1, unfiltered.
// -inf logits are ordinary values of weight 0.  -0 counts as +0.
//
// The threshold is found by selection over order-preserving 32-bit keys of the
// logits: larger float <=> larger unsigned key.
PDRNN_RNG_FN uint32_t decode_order_key(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

PDRNN_RNG_FN float decode_key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// ---- beam search --------------------------------------------------------------
// A launch holds G groups (prompts) of W beams, G W <= 16; stream s = g W + j is
// beam j of group g (ops/decode.py:beam_select mirrors one position's rule).
//   Start: the W streams of a group enter position 0 with the prompt's state
//     and last token, cum[0] = 0, cum[j > 0] = -inf (the copies cannot fill the
//     beam), done = false.
//   Position p, from its fp32 logits l[s, :]:  m_s = max_v l[s, v],
//     lp_s(v) = (l[s, v] - m_s) - log sum_v exp(l[s, v] - m_s)  in fp32 in that
//     order, the max and the sum in the fixed order of the filters' wave_max /
//     wave_sum (every workgroup gets the same bits).
//     A live stream's candidates are every v with cand = cum_s + lp_s(v); a done
//     stream has the single candidate v = stop with cand = cum_s, log-prob 0.
//     Per group the W best candidates become the new beams in rank order: cand
//     descending, then source beam j ascending, then v ascending.  -inf is an
//     ordinary value (with V < W or at position 0 the tail fills with -inf
//     candidates in (j, v) order); a NaN score ranks, and is kept, as -inf; -0
//     counts as +0.
//     New slot i: parent[i] = j, token[i] = v, cum[i] = cand,
//     done[i] = done_j or v == stop.
//   Next position: slot i reads the embedding row of token[i] and, in every
//     layer, the h and c of slot parent[i].
//   After N positions the parents are traced back into hypotheses [G, W, N] in
//     final rank order.
//
// The rank of a score is the order of its key: NaN as -inf, -0 as +0.  Every
// candidate's key is > 0, so 0 can stand for "no candidate".
PDRNN_RNG_FN float beam_score(float cand) {
  if (cand != cand) return -__builtin_inff();
  return cand == 0.f ? 0.f : cand;
}
PDRNN_RNG_FN uint32_t beam_score_key(float cand) { return decode_order_key(beam_score(cand)); }

}  // namespace pdrnn
