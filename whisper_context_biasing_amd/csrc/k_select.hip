// Greedy token selection fused with the bias-list log-prob boost and the generate() bookkeeping.
//
// Semantics (restating the greedy step of [tf] generation/utils.py:2894-2936 plus the build-defined
// A8 boost, oracle/bias_ref.py):
//   score[v] = logit[v] + lam * n(s, v)               (f32 product, f32 add: bias_bonus)
//   n(s, v)  = d' - d + min(k, d + 1 - d')            d = depth(s), k = keep(s), d' = depth(delta(s, v))
//   score[eos] = -inf while step < min_new_tokens     (MinNewTokens semantics, benchmark mode)
//   tok = argmax(score), lowest index on ties (torch.argmax); finished rows emit pad;
//   finished |= tok == eos; s <- delta(s, tok).       lam == 0 → plain greedy, bit-identical.
// delta(s, v) = trans(s) entry if v is listed (lands deeper than depth 1), else the root child
// root_child[v] (only word-start tokens may start a match: the host leaves the others at -1), else
// the root. So n = k - d for every token, + 1 on the root children (the root bitmap), and the exact
// value on the few tokens of trans(s). The vocabulary-wide pass (or the LM-head epilogue) reads the
// logits once applying lam·(rowbase + root bit), rowbase = k - d of the row's state; the per-row
// finalize re-scores only trans(s) — exact because lam >= 0 (checked on the host) and n on a trans
// token is never below the vocabulary-pass value, so an underestimated copy never wins.
//
// Per-utterance lists (FOREST, kernels.h ForestArgs): row m scores against its own clip's automaton.
// The vocabulary pass is handed an all-zero root bitmap, so it applies lam·rowbase only; the finalize
// re-scores trans(s) and the clip's root-children list (n = k - d + 1). Exact by the same argument: the
// vocabulary-pass copy of a root child is one lam short (never above its exact value), and a token in
// both lists keeps the larger candidate, the trans value (never below k - d + 1). delta(s, v) looks in
// trans(s), then in the clip's list, then falls back to the clip's root.
//
// Temperature sampling (SAMPLE instantiations, SelectArgs::seeds; sample.h): every comparison above is made
// on x[v] = sample_perturb(score[v], 1/T, g(seed of the row, step, v)) instead of score[v], so the chosen
// token is a draw from softmax(score / T) (Gumbel-max). The finalize stays exact by the same argument: both
// copies of a token carry the same noise g and x is monotone in score, so an underestimated copy never wins;
// a masked EOS stays -inf. The log-prob of the chosen token is still its raw logit − logsumexp(raw logits).
//
// Token rules (SelectArgs::deny / deny0 / ts; tsrule.h): a denied token's candidate is -inf in every pass. With
// the timestamp grammar on, the deny bitmaps cover [ts0, V) as well, so the partials and the re-scoring loops
// yield the best allowed TEXT token (recomputed over [eos, ts0) from the logits in the one state whose text
// range is that short); the finalize then scores the row's allowed timestamp range [lo, hi] from the logits
// with lam·rowbase — a timestamp is a token no list names — reduces (max, Σexp) and the argmax in the fixed
// lane-strided-then-butterfly order, and takes the best timestamp when logsumexp(timestamps) > max(text)
// (rule 5: both sides carry the same log-softmax normaliser) or when it is the better candidate outright. A row
// whose every candidate is -inf emits EOS. The log-prob of the chosen token stays raw logit − logsumexp(raw).
//
// Repeat rules (REP instantiations, SelectArgs::rep; reprule.h): with hist = the row's live prompt slots and its
// generated tokens, x[v] is penalised (x < 0 ? x·p : x / p) for every v in hist and set to -inf for every v that
// would complete an n-gram of hist, before the boost. Both rules touch only tokens of hist, so one bit per (row,
// token) — the seen bitmap, set from the prompt at decode start and by every finalize for its chosen token —
// splits the work: the vocabulary pass treats a seen token as a denied one, and the finalize walks the history
// (at most n_text_ctx positions, one wave) scoring each position's token from the logits with the penalty, the ban
// and the exact n(s, v) (trans(s), then the root bit / the clip's root children). Exact for any p > 0:
//   1. an unseen token is exact in the partials: neither rule touches it, and the trans(s) / root-children
//      re-scoring of the unseen ones is the argument above, unchanged;
//   2. every seen token is offered once per occurrence with its exact score — the occurrences of one token carry
//      the same value under the same index (the banned set is collected first, so a ban through any occurrence
//      reaches all of them), and the re-scoring loops skip seen tokens, so no inexact copy of one competes;
//   3. no ordering between seen and unseen scores is assumed: with p < 1 a seen token may rise above the unseen
//      best, and it wins the merge then; the argmax over the union, lowest index on ties, is better()'s.
// The chosen token's log-prob stays raw. Not combined with SAMPLE or the timestamp grammar (refused by the runtime).
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace wcb {

WCB_DEV bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// One wave merges a row's n softmax partials (common.h lse_merge) in a fixed order — lane-strided, then the xor
// butterfly, as the argmax partials — into (m, s) on every lane: logsumexp of the row = m + log(s).
WCB_DEV void merge_lse_partials(const float* pm, const float* ps, int n, int lane, float& m, float& s) {
  m = -INFINITY;
  s = 0.f;
  for (int c = lane; c < n; c += 64) lse_merge(m, s, pm[c], ps[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    lse_merge(m, s, om, os);
  }
}

template <bool SAMPLE>
__global__ __launch_bounds__(256) void select_partial_kernel(SelectArgs a) {
  const int m = blockIdx.y, c = blockIdx.x;
  const int chunk = (a.V + a.nchunk - 1) / a.nchunk;
  const int v0 = c * chunk, v1 = min(a.V, v0 + chunk);
  const float* row = a.logits + (long)m * a.ld;
  const bool mask_eos = *a.step < a.min_new;
  const int rb = a.rowbase[m];
  const uint32_t* deny = (a.deny0 && *a.step == 0) ? a.deny0 : a.deny;
  [[maybe_unused]] const int step = SAMPLE ? *a.step : 0;
  [[maybe_unused]] const float inv_t = SAMPLE ? *a.inv_t : 1.f;
  [[maybe_unused]] const uint64_t seed = SAMPLE ? a.seeds[m] : 0ull;
  const uint32_t* seen = a.rep.seen ? a.rep.seen + (long)m * a.rep.words : nullptr;   // repeat rules (null: none)
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = v0 + threadIdx.x; v < v1; v += 256) {
    float x = row[v];
    if (a.lam != 0.f) x = bias_bonus(x, a.lam, rb + (int)((a.root_bits[v >> 5] >> (v & 31)) & 1u));
    if constexpr (SAMPLE) x = sample_perturb(x, inv_t, sample_noise(seed, step, v));
    if (mask_eos && v == a.eos) x = -INFINITY;
    if (deny && deny_bit(deny, v)) x = -INFINITY;
    if (seen && deny_bit(seen, v)) x = -INFINITY;
    if (better(x, v, bv, bi)) { bv = x; bi = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  __shared__ float sv[4];
  __shared__ int si[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sv[w] = bv; si[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float best = sv[0];
    int bidx = si[0];
    for (int k = 1; k < 4; ++k)
      if (better(sv[k], si[k], best, bidx)) { best = sv[k]; bidx = si[k]; }
    a.part_val[m * a.nchunk + c] = best;
    a.part_idx[m * a.nchunk + c] = bidx;
  }
}

// One wave per row; the last row to finish (atomic ticket) advances the step/position counters.
// EMB: the row's next-step input embedding in the same launch (k_norm.hip embed_kernel's arithmetic and
// stats grouping, 64 columns per pass).
// RAG (ragged prompts, with EMB): the row's next position is the next slot minus the row's prompt offset.
// REP (repeat rules, never with SAMPLE): the history pass of the comment at the top; every line of it sits under
// `if constexpr (REP)`, so the other instantiations are the code they were.
template <typename T, bool EMB, bool FOREST, bool SAMPLE = false, bool RAG = false, bool REP = false>
__global__ __launch_bounds__(64) void select_finalize_kernel(SelectArgs a) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int step = *a.step;
  [[maybe_unused]] const uint32_t* seen = REP ? a.rep.seen + (long)m * a.rep.words : nullptr;
  const int pos0 = EMB ? *a.pos : 0;   // read before this row's ticket: the last arriver advances it
  const bool mask_eos = step < a.min_new;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < a.nchunk; c += 64) {
    const float v = a.part_val[m * a.nchunk + c];
    const int i = a.part_idx[m * a.nchunk + c];
    if (better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  // token log-probs: the row's softmax partials in the same fixed order (lane-strided, then the butterfly)
  float lm = -INFINITY, ls = 0.f;
  if (a.out_logprob) merge_lse_partials(a.part_max + (long)m * a.nchunk, a.part_sum + (long)m * a.nchunk, a.nchunk, lane, lm, ls);
  const int s = a.state[m];
  const int t0 = a.trans_off[s], t1 = a.trans_off[s + 1];
  // token rules (wave-uniform; null / off: the step as it always was)
  const uint32_t* deny = (a.deny0 && step == 0) ? a.deny0 : a.deny;
  const bool ts_on = !SAMPLE && a.ts.on;
  int text_lo = 0, w0 = 0, w1 = 0;
  TsAllowed ta{0, 1, 0};
  if (ts_on) {
    w0 = a.ts_state[2 * m];
    w1 = a.ts_state[2 * m + 1];
    ta = ts_allowed(a.ts, a.V, a.eos, w0, w1);
    text_lo = ta.text_lo;
    if (text_lo > 0) {   // the partials hold the best of all text tokens: this state's text range is [text_lo, ts0)
      const float* row = a.logits + (long)m * a.ld;
      const int rb = a.rowbase[m];
      bv = -INFINITY;
      bi = 0x7fffffff;
      for (int v = text_lo + lane; v < a.ts.ts0; v += 64) {
        float x = row[v];
        if (a.lam != 0.f) x = bias_bonus(x, a.lam, rb + (int)((a.root_bits[v >> 5] >> (v & 31)) & 1u));
        if (mask_eos && v == a.eos) x = -INFINITY;
        if (deny_bit(deny, v)) x = -INFINITY;
        if (better(x, v, bv, bi)) { bv = x; bi = v; }
      }
    }
  }
  if (a.lam != 0.f) {
    const float* row = a.logits + (long)m * a.ld;
    const int d = a.st_depth[s], k = a.st_keep[s];
    [[maybe_unused]] const float inv_t = SAMPLE ? *a.inv_t : 1.f;
    [[maybe_unused]] const uint64_t seed = SAMPLE ? a.seeds[m] : 0ull;
    for (int t = t0 + lane; t < t1; t += 64) {
      const int v = a.trans_tok[t];
      const int d2 = a.st_depth[a.trans_dst[t]];
      float x = bias_bonus(row[v], a.lam, d2 - d + min(k, d + 1 - d2));
      if constexpr (SAMPLE) x = sample_perturb(x, inv_t, sample_noise(seed, step, v));
      if (mask_eos && v == a.eos) x = -INFINITY;
      if ((deny && deny_bit(deny, v)) || v < text_lo) x = -INFINITY;
      if constexpr (REP) {   // a seen token is the history pass's to offer
        if (deny_bit(seen, v)) x = -INFINITY;
      }
      if (better(x, v, bv, bi)) { bv = x; bi = v; }
    }
    if constexpr (FOREST) {   // the clip's root children: n = k - d + 1 (the vocabulary pass gave them k - d)
      for (int t = a.forest.rc_off[m] + lane; t < a.forest.rc_off[m + 1]; t += 64) {
        const int v = a.forest.rc_tok[t];
        float x = bias_bonus(row[v], a.lam, k - d + 1);
        if constexpr (SAMPLE) x = sample_perturb(x, inv_t, sample_noise(seed, step, v));
        if (mask_eos && v == a.eos) x = -INFINITY;
        if ((deny && deny_bit(deny, v)) || v < text_lo) x = -INFINITY;
        if constexpr (REP) {
          if (deny_bit(seen, v)) x = -INFINITY;
        }
        if (better(x, v, bv, bi)) { bv = x; bi = v; }
      }
    }
  }
  if constexpr (REP) {
    // the row's history into LDS: its live prompt slots, then what it has generated. The host keeps L within
    // kRepMaxHist (check_repeat refuses n_text_ctx > kRepMaxHist, and every decode has P + max_new <= n_text_ctx + 1,
    // so L <= P + max_new - 1 <= n_text_ctx): the clamp below only guards the LDS arrays, it never drops a token
    __shared__ int hs[kRepMaxHist];
    __shared__ uint32_t banw[kRepBanWords];   // the banned tokens of this step, one bit per token (words <= kRepBanWords)
    const float p = __int_as_float(a.rep.par[0]);
    const int n = a.rep.par[1];
    const int off = a.rep.poff ? a.rep.poff[m] : 0;
    const int Lp = a.rep.P - off;
    const int L = min(Lp + step, kRepMaxHist);
    for (int i = lane; i < L; i += 64)
      hs[i] = i >= Lp ? a.out_ids[(long)m * a.out_ld + i - Lp]
                      : a.rep.prompt ? a.rep.prompt[(long)m * a.rep.prompt_ld + off + i] : a.rep.start_tok;
    const bool ngram = n >= 1 && L >= n;
    if (ngram)
      for (int i = lane; i < a.rep.words; i += 64) banw[i] = 0u;
    __syncthreads();
    // pass 1: the banned set — the token after every history position that matches the suffix. A bit per token, so
    // a ban through any occurrence reaches every occurrence, and pass 2 asks one bit per position
    if (ngram) {
      for (int i = lane; i <= L - n; i += 64) {
        const int v = hs[i + n - 1];
        if (v >= 0 && v < a.V && rep_ngram_match(hs, L, n, i)) atomicOr(&banw[v >> 5], 1u << (v & 31));
      }
    }
    __syncthreads();
    // pass 2: every history position offers its token with the exact score
    const float* row = a.logits + (long)m * a.ld;
    const int d = a.st_depth[s], k = a.st_keep[s];
    for (int j = lane; j < L; j += 64) {
      const int v = hs[j];
      if (v < 0 || v >= a.V) continue;
      float x = rep_penalty(row[v], p);
      if (ngram && ((banw[v >> 5] >> (v & 31)) & 1u)) x = -INFINITY;
      if (a.lam != 0.f) {   // n(s, v): trans(s), then the root bit / the clip's root children, else k - d
        int nu = k - d;
        bool listed = false;
        for (int t = t0; t < t1 && !listed; ++t)
          if (a.trans_tok[t] == v) {
            const int d2 = a.st_depth[a.trans_dst[t]];
            nu = d2 - d + min(k, d + 1 - d2);
            listed = true;
          }
        if (!listed) {
          if constexpr (FOREST) {
            for (int t = a.forest.rc_off[m]; t < a.forest.rc_off[m + 1]; ++t)
              if (a.forest.rc_tok[t] == v) nu = k - d + 1;
          } else {
            nu += (int)((a.root_bits[v >> 5] >> (v & 31)) & 1u);
          }
        }
        x = bias_bonus(x, a.lam, nu);
      }
      if (mask_eos && v == a.eos) x = -INFINITY;
      if (deny && deny_bit(deny, v)) x = -INFINITY;
      if (better(x, v, bv, bi)) { bv = x; bi = v; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }   // (one token from both lists: the larger value stands)
  }
  if (ts_on) {   // (bv, bi) is the best allowed text token; the allowed timestamps [lo, hi] from the logits
    const float* row = a.logits + (long)m * a.ld;
    const int rb = a.rowbase[m];
    float tm = -INFINITY, tsum = 0.f, tv = -INFINITY;
    int ti = 0x7fffffff;
    for (int v = ta.lo + lane; v <= ta.hi; v += 64) {   // at most 1501 columns: 24 per lane
      float x = row[v];
      if (a.lam != 0.f) x = bias_bonus(x, a.lam, rb);
      lse_push(tm, tsum, x);
      if (better(x, v, tv, ti)) { tv = x; ti = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(tm, o, 64), os = __shfl_xor(tsum, o, 64);
      lse_merge(tm, tsum, om, os);
      const float ov = __shfl_xor(tv, o, 64);
      const int oi = __shfl_xor(ti, o, 64);
      if (better(ov, oi, tv, ti)) { tv = ov; ti = oi; }
    }
    const float lse_ts = tsum > 0.f ? tm + logf(tsum) : -INFINITY;
    if (lse_ts > bv || better(tv, ti, bv, bi)) { bv = tv; bi = ti; }
  }
  if ((REP || deny || ts_on) && !(bv > -INFINITY)) bi = 0x7fffffff;   // every candidate excluded: EOS (below)
  const bool fin = a.finished[m] != 0;
  // a row with no comparable value (all NaN) keeps bi = INT_MAX: emit EOS rather than an index past
  // the vocabulary (the next step's embedding lookup must stay in bounds)
  const int tok = fin ? a.pad : (bi >= 0 && bi < a.V ? bi : a.eos);
  // AC transition: tok in trans(s) → its target, else the root child, else root
  int dst = -1;
  for (int t = t0 + lane; t < t1; t += 64)
    if (a.trans_tok[t] == tok) dst = a.trans_dst[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dst = max(dst, __shfl_xor(dst, o, 64));
  int rdst = -1;   // FOREST: tok among the clip's root children
  if constexpr (FOREST) {
    for (int t = a.forest.rc_off[m] + lane; t < a.forest.rc_off[m + 1]; t += 64)
      if (a.forest.rc_tok[t] == tok) rdst = a.forest.rc_dst[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rdst = max(rdst, __shfl_xor(rdst, o, 64));
  }
  if constexpr (EMB) {
    // 8 consecutive columns per lane (16-byte accesses of T; the fragment-major copy holds them
    // contiguously too), the optional per-st_w-column partials in embed_kernel's lane-butterfly order
    const int d = a.d, p = RAG ? max(min(pos0 + 1 - a.pos_off[m], a.n_pos - 1), 0) : min(pos0 + 1, a.n_pos - 1);
    const T* er = reinterpret_cast<const T*>(a.emb) + (long)tok * d;
    const T* pr = reinterpret_cast<const T*>(a.pemb) + (long)p * d;
    if (a.st) {   // (older skinny consumers only) one column per lane, as embed_kernel
      for (int c0 = 0; c0 < d; c0 += 64) {
        const int c = c0 + lane;
        const float v = DT<T>::tof(er[c]) + DT<T>::tof(pr[c]);
        float s1 = v, s2 = v * v;
        if (a.st_w == 32) {
#pragma unroll
          for (int o = 1; o < 32; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
        } else {
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
        }
        if ((c & (a.st_w - 1)) == 0) {
          a.st[((long)m * (d / a.st_w) + c / a.st_w) * 2] = s1;
          a.st[((long)m * (d / a.st_w) + c / a.st_w) * 2 + 1] = s2;
        }
      }
    }
    for (int c = lane * 8; c < d; c += 512) {   // (d % 8 == 0)
      float v[8];
      float ev[8], pv[8];
      load8f<T>(er + c, ev);
      load8f<T>(pr + c, pv);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ev[e] + pv[e];
      float* xr = a.x + (long)m * d + c;
      *reinterpret_cast<f32x4*>(xr) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(xr + 4) = f32x4{v[4], v[5], v[6], v[7]};
      if (a.x16) store8<T>(reinterpret_cast<T*>(a.x16) + (long)m * d + c, v);
      if (a.x16fm) {
        const int kw = a.fm_kpw * 32, w2 = c / kw, ks2 = (c % kw) >> 5, lg = (c & 31) >> 3;
        store8<T>(reinterpret_cast<T*>(a.x16fm) + ((((long)(m >> 4) * a.fm_nw + w2) * a.fm_kpw + ks2) * 64 + lg * 16 + (m & 15)) * 8, v);
      }
    }
  }
  if (lane == 0) {
    if constexpr (FOREST) {
      if (dst < 0) dst = rdst >= 0 ? rdst : a.forest.root[m];
    } else {
      if (dst < 0) dst = (tok >= 0 && tok < a.V && a.root_child[tok] >= 0) ? a.root_child[tok] : 0;
    }
    a.state[m] = dst;
    a.rowbase[m] = a.st_keep[dst] - a.st_depth[dst];
    a.next_ids[m] = tok;
    if constexpr (REP) {   // the chosen token joins the history (this row's words: no other wave writes them)
      if (tok >= 0 && tok < a.V) a.rep.seen[(long)m * a.rep.words + (tok >> 5)] |= 1u << (tok & 31);
    }
    if (ts_on && !fin) {   // finished rows keep their state
      ts_advance(a.ts, tok, w0, w1);
      a.ts_state[2 * m] = w0;
      a.ts_state[2 * m + 1] = w1;
    }
    a.out_ids[(long)m * a.out_ld + step] = tok;
    if (a.out_score) a.out_score[m] = fin ? 0.f : bv;
    if (a.out_logprob)   // the chosen token's raw logit against the row's logsumexp
      a.out_logprob[(long)m * a.out_ld + step] = fin ? 0.f : a.logits[(long)m * a.ld + tok] - (lm + logf(ls));
    // no-speech probability (with out_logprob): step 0 scores the start token's position, so its raw softmax at
    // <|nospeech|> is Whisper's no_speech_prob — one float per row from the logsumexp just merged
    if (a.out_nsp && step == 0) a.out_nsp[m] = expf(a.logits[(long)m * a.ld + a.nsp_token] - (lm + logf(ls)));
    const bool nf = fin || tok == a.eos;
    a.finished[m] = nf ? 1 : 0;
    // one 64-bit counter: arrivals in the low word, unfinished rows in the high word, so the row that
    // arrives last reads the complete count from the value its own add returns — no fence (the other
    // rows' stores are read only by later launches, behind the kernel boundary)
    const unsigned long long old = atomicAdd(a.ticket_unfin, 1ull + (nf ? 0ull : (1ull << 32)));
    if ((unsigned)(old & 0xffffffffull) == (unsigned)(a.M - 1)) {   // every row has arrived
      const int nun = (int)(old >> 32) + (nf ? 0 : 1);
      *a.step = step + 1;
      *a.pos = *a.pos + 1;
      if (nun == 0 && *a.all_done == 0) *a.all_done = step + 1;
      *a.ticket_unfin = 0ull;
    }
  }
}

// Causal prefill (runtime.cpp prefill): the token ids of positions *pos .. *pos + np - 1 of every
// row, rows (row, position) row-major; ld 0 = one prefix shared by every row.
__global__ void prefill_ids_kernel(int* ids, const int* src, int R, int np, int ld, const int* pos) {
  const int p = *pos;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R * np; i += gridDim.x * blockDim.x)
    ids[i] = src[(long)(i / np) * ld + p + i % np];
}
void prefill_ids(int* ids, const int* src, int R, int np, int ld, const int* pos, hipStream_t s) {
  const int grid = std::min((R * np + 255) / 256, 256);
  WCB_LAUNCH(prefill_ids_kernel, dim3(grid), dim3(256), 0, s, ids, src, R, np, ld, pos);
}
__global__ void add_i32_kernel(int* p, int v) {
  if (threadIdx.x == 0) *p += v;
}
void add_i32(int* p, int v, hipStream_t s) { WCB_LAUNCH(add_i32_kernel, dim3(1), dim3(64), 0, s, p, v); }

// Teacher forcing / prompt prefill: next_ids[b] = forced[b·ld + (*pos) + 1]; pos += 1.
__global__ void advance_forced_kernel(int* next_ids, const int* forced, int M, int ld, int* pos) {
  const int p = *pos;
  __syncthreads();
  for (int b = threadIdx.x; b < M; b += blockDim.x) next_ids[b] = forced[(long)b * ld + p + 1];
  __syncthreads();
  if (threadIdx.x == 0) *pos = p + 1;
}
void advance_forced(int* next_ids, const int* forced, int M, int ld, int* pos, hipStream_t s) {
  WCB_LAUNCH(advance_forced_kernel, dim3(1), dim3(256), 0, s, next_ids, forced, M, ld, pos);
}

// next_ids[b] = src[b·ld + col]
__global__ void gather_col_kernel(int* dst, const int* src, int M, int ld, int col) {
  for (int b = threadIdx.x; b < M; b += blockDim.x) dst[b] = src[(long)b * ld + col];
}
void gather_col(int* dst, const int* src, int M, int ld, int col, hipStream_t s) {
  WCB_LAUNCH(gather_col_kernel, dim3(1), dim3(256), 0, s, dst, src, M, ld, col);
}

struct IntChunk { int n; int v[256]; };
__global__ void write_i32_kernel(int* dst, IntChunk c) {
  for (int i = threadIdx.x; i < c.n; i += blockDim.x) dst[i] = c.v[i];
}
void write_i32(int* dst, const int* host_src, int n, hipStream_t s) {
  for (int o = 0; o < n; o += 256) {
    IntChunk c;
    c.n = n - o < 256 ? n - o : 256;
    for (int i = 0; i < c.n; ++i) c.v[i] = host_src[o + i];
    WCB_LAUNCH(write_i32_kernel, dim3(1), dim3(256), 0, s, dst + o, c);
  }
}

template <bool FOREST, bool SAMPLE, bool REP = false>
static void select_finalize_launch(const SelectArgs& a, hipStream_t s) {
  if (a.emb && a.pos_off) {   // ragged prompts: the embedding at the row's own position
    if (a.dtype == kBF16) WCB_LAUNCH((select_finalize_kernel<bf16_t, true, FOREST, SAMPLE, true, REP>), dim3(a.M), dim3(64), 0, s, a);
    else if (a.dtype == kF16) WCB_LAUNCH((select_finalize_kernel<f16_t, true, FOREST, SAMPLE, true, REP>), dim3(a.M), dim3(64), 0, s, a);
    else WCB_LAUNCH((select_finalize_kernel<float, true, FOREST, SAMPLE, true, REP>), dim3(a.M), dim3(64), 0, s, a);
  } else if (!a.emb) {
    WCB_LAUNCH((select_finalize_kernel<float, false, FOREST, SAMPLE, false, REP>), dim3(a.M), dim3(64), 0, s, a);
  } else if (a.dtype == kBF16) {
    WCB_LAUNCH((select_finalize_kernel<bf16_t, true, FOREST, SAMPLE, false, REP>), dim3(a.M), dim3(64), 0, s, a);
  } else if (a.dtype == kF16) {
    WCB_LAUNCH((select_finalize_kernel<f16_t, true, FOREST, SAMPLE, false, REP>), dim3(a.M), dim3(64), 0, s, a);
  } else {
    WCB_LAUNCH((select_finalize_kernel<float, true, FOREST, SAMPLE, false, REP>), dim3(a.M), dim3(64), 0, s, a);
  }
}
void select_finalize(const SelectArgs& a, hipStream_t s) {
  if (a.rep.seen) {   // repeat rules: the REP instantiations (greedy, no timestamp grammar)
    if (a.seeds || a.ts.on) throw std::runtime_error("internal error: repeat rules with sampling or the timestamp grammar");
    if (a.forest.root) select_finalize_launch<true, false, true>(a, s);
    else select_finalize_launch<false, false, true>(a, s);
  } else if (a.seeds) {   // temperature sampling: the sampled instantiations
    if (a.forest.root) select_finalize_launch<true, true>(a, s);
    else select_finalize_launch<false, true>(a, s);
  } else if (a.forest.root) {
    select_finalize_launch<true, false>(a, s);
  } else {
    select_finalize_launch<false, false>(a, s);
  }
}

// decode start with repeat rules: one workgroup per row clears the row's words, then sets the bits of its live
// prompt slots (ids outside [0, V) ignored)
__global__ __launch_bounds__(256) void rep_init_kernel(RepArgs r, int V) {
  const int m = blockIdx.x;
  uint32_t* w = r.seen + (long)m * r.words;
  for (int i = threadIdx.x; i < r.words; i += 256) w[i] = 0u;
  __syncthreads();
  const int off = r.poff ? r.poff[m] : 0;
  for (int i = off + threadIdx.x; i < r.P; i += 256) {
    const int v = r.prompt ? r.prompt[(long)m * r.prompt_ld + i] : r.start_tok;
    if (v >= 0 && v < V) atomicOr(&w[v >> 5], 1u << (v & 31));
  }
}
void rep_init(const RepArgs& r, int rows, int V, hipStream_t s) {
  WCB_LAUNCH(rep_init_kernel, dim3(rows), dim3(256), 0, s, r, V);
}

// decode start with per-utterance lists: every row in its clip's root state (the zero fill means "state 0",
// which is clip 0's root only)
__global__ void forest_init_kernel(ForestArgs f, int* state, int* rowbase, int R, int nb) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
    state[r] = f.root[r / nb];
    if (rowbase) rowbase[r] = 0;   // keep - depth of a root
  }
}
void forest_init(const ForestArgs& f, int* state, int* rowbase, int R, int nb, hipStream_t s) {
  WCB_LAUNCH(forest_init_kernel, dim3((R + 255) / 256), dim3(256), 0, s, f, state, rowbase, R, nb);
}

// The partial merges of select_finalize_kernel on their own (wcb_op_lm_head_lse): one wave per row,
// argmax[m] = the best partial (lowest index on ties), lse[m] = max + log(sum) of the merged softmax partials.
__global__ __launch_bounds__(64) void lse_finalize_kernel(const float* part_val, const int* part_idx, const float* part_max,
                                                          const float* part_sum, int nchunk, float* lse, int* argmax) {
  const int m = blockIdx.x, lane = threadIdx.x;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < nchunk; c += 64) {
    const float v = part_val[m * nchunk + c];
    const int i = part_idx[m * nchunk + c];
    if (better(v, i, bv, bi)) { bv = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  float lm, ls;
  merge_lse_partials(part_max + (long)m * nchunk, part_sum + (long)m * nchunk, nchunk, lane, lm, ls);
  if (lane == 0) {
    argmax[m] = bi;
    lse[m] = lm + logf(ls);
  }
}
void lm_head_lse_finalize(const float* part_val, const int* part_idx, const float* part_max, const float* part_sum, int M,
                          int nchunk, float* lse, int* argmax, hipStream_t s) {
  WCB_LAUNCH(lse_finalize_kernel, dim3(M), dim3(64), 0, s, part_val, part_idx, part_max, part_sum, nchunk, lse, argmax);
}

void select_greedy(const SelectArgs& a, hipStream_t s) {
  if (a.seeds) WCB_LAUNCH(select_partial_kernel<true>, dim3(a.nchunk, a.M), dim3(256), 0, s, a);
  else WCB_LAUNCH(select_partial_kernel<false>, dim3(a.nchunk, a.M), dim3(256), 0, s, a);
  select_finalize(a, s);
}

}  // namespace wcb
