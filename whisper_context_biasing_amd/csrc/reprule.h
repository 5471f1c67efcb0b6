// Repeat rules of the greedy decoder: the repetition penalty (HF RepetitionPenaltyLogitsProcessor) and the
// no-repeat n-gram ban (HF NoRepeatNGramLogitsProcessor). One definition of the arithmetic and of the suffix
// match: select_finalize_kernel<.., REP> and the host function wcb_repeat_rules_apply_host compile these very
// functions.
//
// For a decoder row, hist[0..L) is what HF's processors see as input_ids: the row's live prompt tokens, the start
// token, the forced language / task tail and every token generated so far (dead left-padding slots of a ragged
// batch are not part of it). On the raw f32 logits x, before anything else of the step:
//   penalty p > 0:  for every distinct v in hist   x[v] = x[v] < 0 ? x[v]·p : x[v] / p     (one f32 multiply, or one
//                   correctly rounded f32 division; never a multiply by a reciprocal)
//   n-gram n >= 1:  if L >= n, for every i in [0, L - n] with hist[i .. i+n-1) == hist[L-n+1 .. L):
//                   x[hist[i + n - 1]] = -inf   (a token is banned when ANY of its occurrences matches)
// p = 1 and n = 0 mean "off".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WCB_REP_HD __host__ __device__ __forceinline__
#else
#define WCB_REP_HD inline
#endif

namespace wcb {

WCB_REP_HD float rep_penalty(float x, float p) { return x < 0.f ? x * p : x / p; }

// the n - 1 tokens from hist[i] equal the last n - 1 tokens of hist[0..L): position i + n - 1 then holds a token
// that would complete an n-gram already in the history (0 <= i <= L - n; n == 1: always)
WCB_REP_HD bool rep_ngram_match(const int* hist, int L, int n, int i) {
  for (int j = 0; j < n - 1; ++j)
    if (hist[i + j] != hist[L - n + 1 + j]) return false;
  return true;
}

}  // namespace wcb
