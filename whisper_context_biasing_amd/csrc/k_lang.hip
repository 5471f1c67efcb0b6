// Language detection: the language head and its finalize.
//
// Semantics (HF WhisperGenerationMixin.detect_language, [tf] generation_whisper.py): after one decoder pass over
// [decoder_start] at position 0, the logits of the language tokens [lang_begin, lang_begin + n_lang) alone decide:
//   id[b]       = argmax over the candidate languages (lowest index on ties)
//   probs[b][i] = softmax over the candidate languages (0 for a language that is no candidate)
// Every other column of the vocabulary is masked (HF sets them to -inf before the argmax and the softmax).
//
// lang_head_kernel: logits[m][c] = LN(x_m) · W[c] for the 16-column tiles that cover the language range (at most
// kLangTiles tiles; lang_begin is 50259 = 3 mod 16, so the first tile starts before the range and the last one ends
// after it), with the decoder's final LayerNorm of the f32 residual row fused (LN: the row is normalised once per
// workgroup into LDS, rounded to the model type as every LN-fused projection's A operand is), or on rows already in the
// model type (the op-level entry point). Products and sums in f32; one wave per column, lanes strided over K, then the
// butterfly, so a row's logits never depend on the batch it is in.
//
// lang_finalize_kernel: one wave per row over the tiles' columns (at most 112, lane-strided): the columns outside the
// language range and the non-candidates are masked, (max, Σexp) and the argmax are reduced in a fixed order — lane-
// strided, then the xor butterfly — and the row's id, its probabilities and the language column of its device-side
// prompt row are written with plain stores. No scratch, no LDS.
#include "common.h"
#include "kernels.h"

namespace wcb {

template <typename T, bool LN>
__global__ __launch_bounds__(256) void lang_head_kernel(LangArgs a) {
  __shared__ float ys[kLangMaxK];
  const int m = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K;
  if constexpr (LN) {
    const float* xr = static_cast<const float*>(a.A) + (long)m * a.lda;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += xr[k];
    const float mean = wave_sum(s) / K;
    float q = 0.f;
    for (int k = lane; k < K; k += 64) { const float t = xr[k] - mean; q += t * t; }
    const float rstd = rsqrtf(wave_sum(q) / K + 1e-5f);   // every wave the same bits: the same order of sums
    for (int k = threadIdx.x; k < K; k += 256)
      ys[k] = DT<T>::tof(DT<T>::fromf((xr[k] - mean) * rstd * a.ln_w[k] + a.ln_b[k]));
  } else {
    const T* ar = static_cast<const T*>(a.A) + (long)m * a.lda;
    for (int k = threadIdx.x; k < K; k += 256) ys[k] = DT<T>::tof(ar[k]);
  }
  __syncthreads();
  const T* W = static_cast<const T*>(a.W);
  const int c0 = a.col0 + blockIdx.x * 16;
  for (int j = wave; j < 16; j += 4) {
    const int c = c0 + j;
    if (c >= a.col1) break;   // (the last tile of a vocabulary that ends inside it)
    const T* wr = W + (long)c * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(ys[k], DT<T>::tof(wr[k]), acc);
    acc = wave_sum(acc);
    if (lane == 0) a.logits[(long)m * a.ld + c] = acc;
  }
}

WCB_DEV bool lang_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(64) void lang_finalize_kernel(LangArgs a) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const float* row = a.logits + (long)m * a.ld;
  const int n = a.col1 - a.col0;   // <= 16 * kLangTiles = 128: at most two columns per lane
  float v[2];
  int idx[2];
  float mx = -INFINITY, sm = 0.f, bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = lane + 64 * t, c = a.col0 + j, i = c - a.lang_begin;
    bool ok = j < n && i >= 0 && i < a.n_lang;
    if (ok && a.cand) ok = (a.cand[i >> 5] >> (i & 31)) & 1u;
    v[t] = ok ? row[c] : -INFINITY;
    idx[t] = i;
    if (ok) {
      lse_push(mx, sm, v[t]);
      if (lang_better(v[t], i, bv, bi)) { bv = v[t]; bi = i; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
    lse_merge(mx, sm, om, os);
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (lang_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (bi < 0 || bi >= a.n_lang) bi = 0;   // no finite candidate (non-finite logits): still a language token
  if (a.out_probs) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (idx[t] >= 0 && idx[t] < a.n_lang && lane + 64 * t < n)
        a.out_probs[(long)m * a.n_lang + idx[t]] = v[t] == -INFINITY ? 0.f : expf(v[t] - mx) / sm;
  }
  if (lane == 0) {
    const int id = a.lang_begin + bi;
    if (a.out_ids) a.out_ids[m] = id;
    if (a.prompts) a.prompts[(long)m * a.prompt_ld + a.prompt_col] = id;
  }
}

template <typename T>
static void lang_head_t(const LangArgs& a, hipStream_t s) {
  const dim3 grid((a.col1 - a.col0 + 15) / 16, a.M), blk(256);
  if (a.ln_w) WCB_LAUNCH((lang_head_kernel<T, true>), grid, blk, 0, s, a);
  else WCB_LAUNCH((lang_head_kernel<T, false>), grid, blk, 0, s, a);
}

void lang_head(DType t, const LangArgs& a, hipStream_t s) {
  switch (t) {
    case kBF16: lang_head_t<bf16_t>(a, s); break;
    case kF16: lang_head_t<f16_t>(a, s); break;
    case kF32: lang_head_t<float>(a, s); break;
  }
}

void lang_finalize(const LangArgs& a, hipStream_t s) {
  WCB_LAUNCH(lang_finalize_kernel, dim3(a.M), dim3(64), 0, s, a);
}

}  // namespace wcb
