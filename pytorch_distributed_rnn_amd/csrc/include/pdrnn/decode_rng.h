// The sampling rule of the char-LM decode path, written once: the kernels
// (kernels/lstm_decode.hip) include it, ops/decode.py:gumbel_noise mirrors it
// step for step.
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

}  // namespace pdrnn
