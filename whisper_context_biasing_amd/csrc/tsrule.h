// Token rules of the greedy decoder: the deny lists (HF SuppressTokensLogitsProcessor /
// SuppressTokensAtBeginLogitsProcessor) and Whisper's timestamp grammar (HF WhisperTimeStampLogitsProcessor
// with _detect_timestamp_from_logprob). One definition of the state machine: select_finalize_kernel, the
// host function wcb_token_rules_apply_host and the runtime's bitmap builder compile these very functions.
//
// For a decoder row that has generated g[0..t) after its prompt, ts0 = timestamp_begin, V = vocab:
//   last = t >= 1 and g[t-1] >= ts0          pen = t < 2 or g[t-2] >= ts0          L = the last timestamp generated
//   text tokens  [text_lo, ts0):  text_lo = 0; eos when last and not pen; ts0 (none) when t == 0
//   timestamps   [lo, hi]:        none when last and pen; lo = ts0, or L when last and not pen, or L + 1 otherwise
//                                 (a timestamp was generated); hi = V - 1, or ts0 + max_initial at t == 0
//   rule 5: logsumexp(score[lo..hi]) > max(score[text range]) → the text range is excluded as well
// The deny bitmap (suppress ids; begin_suppress ids too at t == 0; no_timestamps with the grammar on)
// applies to the text range. The row state is two ints, zero at the start of a decode:
//   w0 = t << 2 | bit 0: g[t-1] was a timestamp | bit 1: g[t-2] was one          w1 = L + 1 (0: none yet)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WCB_TS_HD __host__ __device__ __forceinline__
#else
#define WCB_TS_HD inline
#endif

namespace wcb {

struct TsRule {
  int on = 0;          // 1: the timestamp grammar applies
  int ts0 = 0;         // timestamp_begin
  int max_init = -1;   // max_initial_timestamp_index (< 0: no limit)
};

struct TsAllowed {
  int text_lo;   // text candidates are [text_lo, ts0) (text_lo == ts0: none)
  int lo, hi;    // timestamp candidates are [lo, hi] (lo > hi: none)
};

WCB_TS_HD TsAllowed ts_allowed(const TsRule& r, int V, int eos, int w0, int w1) {
  const int t = w0 >> 2;
  const bool last = t >= 1 && (w0 & 1);
  const bool pen = t < 2 || (w0 & 2);
  TsAllowed a;
  a.text_lo = t == 0 ? r.ts0 : (last && !pen) ? eos : 0;
  a.lo = r.ts0;
  a.hi = V - 1;
  if (w1 > 0) a.lo = (last && !pen) ? w1 - 1 : w1;   // L, or L + 1
  if (t == 0 && r.max_init >= 0 && r.ts0 + r.max_init < a.hi) a.hi = r.ts0 + r.max_init;
  if (last && pen) { a.lo = 1; a.hi = 0; }
  return a;
}

// the row state after the row emitted `tok`
WCB_TS_HD void ts_advance(const TsRule& r, int tok, int& w0, int& w1) {
  const bool is_ts = tok >= r.ts0;
  w0 = (((w0 >> 2) + 1) << 2) | ((w0 & 1) << 1) | (is_ts ? 1 : 0);
  if (is_ts) w1 = tok + 1;
}

WCB_TS_HD bool deny_bit(const uint32_t* bits, int v) { return (bits[v >> 5] >> (v & 31)) & 1u; }

}  // namespace wcb
