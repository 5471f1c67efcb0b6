// Temperature sampling as a perturbed argmax (Gumbel-max): a token drawn from softmax(score / T) is
// argmax_v(score[v] / T + g[v]) with g i.i.d. standard Gumbel. The noise is a pure function of (clip seed,
// step, token) through a counter-based generator, so every kernel that scores a token — the LM-head epilogues,
// the vocabulary pass, the finalize's re-scoring loops — and the host (wcb_sample_noise, the tests' numpy
// restatement) compute the same value with no state, no vocabulary-wide pass and no second launch.
//
//   r = philox4x32_10((v >> 2, t, 0, 0), (lo32(seed), hi32(seed)))[v & 3]      t = 0-based generated-token index
//   u = ((r >> 9) + 0.5f) · 2^-23                                              exact in f32, 0 < u < 1
//   g = -logf(-logf(u))                                                         the accurate logf
//   x = fmaf(score, inv_T, g)                                                   inv_T = 1.0f / T (host); -inf stays -inf
//
// (23 bits, not 24: n + 0.5 is a 24-bit significand only for n < 2^23. With r >> 8 the upper half of the range
// rounds to even in f32 and n = 2^24 - 1 gives u = 1, g = +inf — a forced token about once per 2^24 draws.)
// Four neighbouring tokens share one Philox block; only the values are specified (a kernel may compute the
// block per lane). Host and device compile these very functions.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WCB_HD __host__ __device__ __forceinline__
#else
#define WCB_HD inline
#endif

namespace wcb {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c[4] → c[4]
WCB_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the 32 random bits of (seed, step, token)
WCB_HD uint32_t sample_bits(uint64_t seed, int step, int v) {
  uint32_t c[4] = {(uint32_t)v >> 2, (uint32_t)step, 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int j = v & 3;
  return j == 0 ? c[0] : j == 1 ? c[1] : j == 2 ? c[2] : c[3];
}

// uniform in (0, 1): the top 23 bits, centred in their cell (exact in f32: 2^-24 <= u <= 1 - 2^-24)
WCB_HD float sample_uniform(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// standard Gumbel noise g(seed, step, v)
WCB_HD float sample_noise(uint64_t seed, int step, int v) {
  return -logf(-logf(sample_uniform(sample_bits(seed, step, v))));
}

// the perturbed score every sampled comparison uses: monotone in `score`, -inf stays -inf (inv_T > 0, g finite)
WCB_HD float sample_perturb(float score, float inv_T, float g) { return fmaf(score, inv_T, g); }

}  // namespace wcb
