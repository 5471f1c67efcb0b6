/* libwcb — MI355X-native Whisper contextual-biasing inference path (C ABI).
 *
 * The reference exposes no native plugin API: its hot-path boundary is the Python class contract of
 * `WhisperForConditionalGenerationWeightCE` (models/whisper_medical.py:12-172) driven by
 * `scripts/evaluation.py:164-206` and the feature extractor call at data_utils/data_loader.py:171.
 * Each entry point below replaces one piece of that surface; the Python mirror
 * `whisper_context_biasing_amd.model.WhisperCB` binds them with ctypes.
 *
 * Conventions: return 0 on success, a negative wcb_status otherwise (message: wcb_last_error);
 * no exception crosses the ABI. Activation buffers are caller-owned DEVICE memory; weights,
 * workspaces and KV caches are library-owned. One handle per GPU; calls on one handle are
 * serialised by the caller. `stream` is a hipStream_t (NULL = default stream).
 */
#ifndef WCB_H_
#define WCB_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wcb_handle wcb_handle;
typedef struct wcb_bias wcb_bias;
typedef struct wcb_bias_batch wcb_bias_batch;

enum wcb_status {
  WCB_OK = 0,
  WCB_ERR_ARG = -1,       /* invalid argument / shape (ValueError in the reference) */
  WCB_ERR_STATE = -2,     /* call out of order (e.g. weights not finalized) */
  WCB_ERR_HIP = -3,       /* HIP runtime error */
  WCB_ERR_UNSUPPORTED = -4
};

enum wcb_dtype { WCB_BF16 = 0, WCB_F16 = 1, WCB_F32 = 2 };

/* Model dimensions (HF WhisperConfig fields; encoder and decoder depth are equal for every size). */
typedef struct {
  int d_model, n_layers, n_heads, ffn, vocab, n_mel;
  int n_audio_ctx;   /* 1500 */
  int n_text_ctx;    /* 448 */
  int eos_token_id, pad_token_id, decoder_start_token_id;
  int dtype;         /* wcb_dtype of weights and activations (f32 accumulation everywhere) */
} wcb_model_desc;

/* Decode configuration (replaces the GenerationConfig of scripts/evaluation.py:173-179). */
typedef struct {
  int max_new_tokens;   /* generate(max_length=N) of the reference → at most N new tokens */
  int min_new_tokens;   /* EOS masked while fewer tokens were generated (benchmark mode) */
  int num_beams;        /* 1 = greedy (the reference eval setting) */
  float bias_boost;     /* lambda >= 0 of the bias-list boost; 0 = plain greedy bit-for-bit */
  int use_graph;        /* replay the decode step as a captured hipGraph */
  int async_out;        /* 1: do not make `stream` wait for the decode; outputs valid after
                           wcb_synchronize (lets the next call's front end + encoder overlap it) */
} wcb_gen_cfg;

/* replaces WhisperForConditionalGenerationWeightCE(config) (models/whisper_medical.py:16-22) */
int wcb_create(const wcb_model_desc* desc, int device, wcb_handle** out);
void wcb_destroy(wcb_handle* h);
const char* wcb_last_error(const wcb_handle* h);

/* alternative formulations the tests compare (defaults are fixed per model; no environment variables):
 *   "xmode" 0/1        decoder cross-attention over per-layer K/V, or in encoder space (before finalize)
 *   "beam_xmode" 0/1   the same for beam search (before finalize)
 *   "group_rows" n     decoder rows per layer chain (16..512)
 *   "xenc_variant" v   encoder-space kernel variant, "xvariant" v  K/V cross-attention kernel variant
 *   "flash_split" n    key ranges per (clip, head) of the beam-search cross-attention (flash kernel), 1..8
 *   "beam_xattn" v     beam-search cross-attention: keys split over the waves of one (clip, head) workgroup
 *                      (1: 4 waves x 2 LDS stages, 2: 2 x 4, 3: 2 x 5) or the flash kernel over key ranges (0)
 *   "ln_fold" 0/1      decode rows > 64 (16-bit): LayerNorm folded into the projection (1, default: finalize
 *                      keeps W·diag(γ) copies of QKV / cross-q / fc1, ≈ +1/4 of the decoder weights), or its own
 *                      launch (0); before finalize
 *   "merge_v" 0/1      greedy encoder-space cross-attention: range merge and W_v fused (1) or two launches
 *   "xpart16" 0/1      greedy encoder-space cross-attention (fused merge): the key-range partials stored in the
 *                      model dtype, each normalised by its own softmax sum, (max, sum) in f32 (1, default: half
 *                      the partial bytes) or unnormalised f32 partials (0)
 *   "xq_kq" 0/1        greedy encoder-space cross-attention query (lean path): q'_h = W_k,hᵀ q_h computed inside
 *                      the LN-fused q_proj launch (1) or as a launch of its own (0, default); bit-identical
 *   "lean" 0/1         decode projections of <= 64 rows (16-bit) on the lean single-tile kernel (1, default)
 *                      or the general decode GEMM (0); bit-identical. Before finalize: with it finalize keeps
 *                      fragment-major copies of the decoder projection weights and the token embedding (the
 *                      decoder weights once more in memory, e.g. ≈ +1.8 GB at large-v3 fp16)
 *   "lean_x" 0/1       lean path, one position per row: the residual writers also write the 16-bit rows
 *                      fragment-major for the LayerNorm-fused QKV / xq / fc1 (1, default); bit-identical
 *   "decode_contexts" n  decode contexts in flight (1..4): calls decode on n streams from n buffers (4 is
 *                      refused while a step-wise decode owns context 3)
 *   "steps_per_graph" n  decode steps captured per replayed hipGraph (1..64, default 8)
 *   "align_ws" n       MiB of the token-timestamp weights workspace (1..65536, default 1024): a batch above it is
 *                      aligned in groups of clips (wcb_align); the frames do not depend on it
 *   "xenc_fm" 0/1      greedy encoder-space cross-attention reads the encoder output in the fragment-major chunk
 *                      layout (1, default; 1 KiB contiguous per load wave-instruction) or the row layout (0)
 *   "ring_kt" 1/2      decode rows > 64: 64-deep K sub-tiles per LDS-ring stage of the projection tiles
 *   "beam_wide" 0/1    decode rows 65-96 (C5's beam rows): out / xo / xq / fc1 on the wide single-burst tiles
 *                      with fragment-major weights (1, default) or the LDS-ring tiles (0); before finalize
 *   "beam_wfm" 0/1     decode rows > 64: the LDS-ring tiles read fragment-major weight copies (0, default);
 *                      before finalize
 *   "beam_raster" n    decode rows > 64: ring tile order in bands of n row panels, column tiles outer (0, default:
 *                      row panels outer)
 *   "lean_fold" 0/1    <= 64 rows: the LayerNorm-fused projections (QKV, cross-q, fc1) with the LayerNorm folded
 *                      into fragment-major W·diag(γ) copies (1, default) or normalised in the kernel (0); before
 *                      finalize
 *   "xqk" 0/1          greedy cross query (encoder space, lean, folded): q_h and q'_h = W_k,hᵀ q_h in one launch
 *                      with no hand-off, each workgroup recomputing its head's q_h (1, default) or the xq → kq
 *                      launches (0)
 *   "xqk_chunks" n     fused cross query: q' column chunks per head, each chunk's workgroup recomputing q_h (2, 4,
 *                      8 (default), 16); bit-identical
 *   "lean_mf2" 0/1     <= 64 rows: every lean projection on 32-row workgroups where the chain has > 16 rows (1) or
 *                      only the LN-fused N >= 2048 ones (0, default); bit-identical
 *   "mel_split" 0/1    log-mel DFT as split-bf16 MFMAs (1) or exact-f32 MFMAs (0, default); both within 2e-5 of
 *                      the reference feature extractor
 *   "lm_walkers" n     greedy LM head: column walkers per row block = argmax partials per row (128, 192, 256
 *                      (default), 384, 512, 1024; before finalize); the selected ids do not depend on it
 *   "merge_os" 1/2     greedy range merge + W_v: a head's 64 outputs in one workgroup of 2 rows (1, default) or
 *                      over two workgroups of 4 rows (2); bit-identical
 *   "beam_chunks" 0/1  beam top-K over 16 vocabulary chunks per row, one workgroup each (1) or one workgroup
 *                      per row (0, default)
 *   "xenc_split" n     key ranges per row of the greedy encoder-space cross-attention (1..16, before finalize)
 *   "enc_flash" v      encoder flash attention tiling: 2 (32 queries per wave), 4 (64 queries, default)
 *   "enc_raster" n     encoder GEMM tile order: bands of n row panels, column tiles outer (8, default;
 *                      0: row-major); bit-identical
 *   "enc_gemm" v       encoder GEMM kernels: 4 (default) the ping-pong kernel, 256- or 192-wide tiles by the
 *                      fewer tile rounds; 1 the LDS-ring kernel's 256x192 tiles where 192-wide wins; 0 the
 *                      LDS-ring kernel everywhere; 5 the ping-pong kernel's 192-wide tiles wherever N allows
 *                      (162 VGPRs: room on a CU for a decode workgroup beside it; measured 1 % slower)
 * While a step-wise decode is open (wcb_decode_begin .. wcb_decode_end) only decode_contexts, enc_flash,
 * enc_gemm, enc_raster and steps_per_graph may change: the others shape the state it carries between steps. */
int wcb_set_option(wcb_handle* h, const char* name, int value);

/* replaces from_pretrained / load_state_dict: one HF state-dict tensor (host f32, C order), staged
 * on the device. Names follow the reference's state dict (model.encoder.layers.{i}.self_attn.q_proj.weight,
 * ...). proj_out.weight is tied to model.decoder.embed_tokens.weight (models/whisper_medical.py:14). */
int wcb_set_weight(wcb_handle* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* a BORROWED device tensor (e.g. a torch CUDA tensor or a view into an RCCL-broadcast blob) */
typedef struct wcb_tensor_view {
  const char* name;     /* HF state-dict name */
  const void* data;     /* device pointer of element [0,...,0] */
  int dtype;            /* wcb_dtype of the elements */
  int ndim;             /* 1..4 */
  int64_t shape[4];
  int64_t stride[4];    /* in elements */
} wcb_tensor_view;
/* stages n device tensors without a host round trip (gathered and widened to f32 on the device, on
 * `stream`); the views are not read after the call returns. Mixes freely with wcb_set_weight. */
int wcb_load_weights(wcb_handle* h, const wcb_tensor_view* views, int n, void* stream);
/* build the device layouts from the staged tensors on the device (fused QKV with q pre-scaled,
 * im2col conv weights, W_k,hᵀ panels, all-layer cross-KV stack), rounded once to the model dtype;
 * staging buffers are released. */
int wcb_finalize_weights(wcb_handle* h);

/* replaces WhisperFeatureExtractor.__call__ (data_utils/data_loader.py:171-172):
 * pcm f32 [B][pcm_stride] (first n_samples valid, zero-padded/trimmed to 480000)
 * → mel_out f32 [B][n_mel][3000]. */
int wcb_log_mel(wcb_handle* h, const float* pcm, int B, int n_samples, int64_t pcm_stride, float* mel_out,
                void* stream);

/* replaces WhisperEncoder.forward ([tf] modeling_whisper.py:592-646): mel f32 [B][n_mel][3000]
 * → enc_out [B][1500][d] in the model dtype (may be NULL: result kept internally for decode). */
int wcb_encode(wcb_handle* h, const float* mel, int B, void* enc_out, void* stream);

/* replaces model.generate(input_features, max_length=...) as called by
 * [tf] trainer_seq2seq.py:329: greedy (num_beams = 1) or HF beam search (num_beams 2..8,
 * [tf] generation/utils.py:3208) from [decoder_start] (+ optional prefix), bias boost,
 * out_ids int32 DEVICE [B][cfg->max_new_tokens] (finished rows padded with pad_token_id; beams: the
 * best finished sequence of each clip), *out_steps = number of generated columns (greedy: all rows
 * finished or max_new_tokens; beams: the longest best sequence — with async_out, max_new_tokens: the
 * length is not read back, columns past a clip's best sequence hold pad_token_id).
 * The front end/encoder run on one library stream and the decode on another, with two cross-K/V
 * buffers: call i+1's encoder overlaps call i's decode (async_out = 1 keeps `stream` free). */
int wcb_generate(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                 const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream);

/* Step-wise decoding (SURVEY §8(b) wcb_decode_begin / wcb_decode_step): the decode step of wcb_generate
 * one token per call, for callers that inspect every step (the reference's surface is generate(); this is
 * the streaming form of it). `enc` = encoder output [B][1500][d] in the model dtype (DEVICE, copied /
 * projected at begin: not retained), `prefix` = per-utterance prompt [B][prefix_len] (HOST, NULL:
 * decoder_start_token_id only; positions 0 .. prefix_len-2 are prefilled, the last one is the first step's
 * input), EOS masked while fewer than min_new_tokens were generated. One active state per handle (it owns
 * decode context 3, so decode_contexts must be <= 3). The bias automaton must be the same (or NULL) at
 * every step of one decode.
 *  - greedy (num_beams = 1): wcb_decode_step writes next_ids [B] (int32, DEVICE) and, when non-NULL,
 *    scores [B] (f32, DEVICE: the chosen token's logit + bias boost; 0 for finished rows); finished rows
 *    emit pad_token_id.
 *  - beam search (num_beams = nb in 2..8, HF _beam_search, [tf] generation/utils.py:3208-3524, one
 *    iteration per step; rows R = B·nb, beam i of utterance b = row b·nb + i): wcb_decode_begin caps the
 *    length at max_target_positions as generate() does by default, wcb_decode_begin_beams at prefix +
 *    max_new_tokens (generate(max_length=...); the cap is a stopping criterion, so it changes the beams).
 *    wcb_decode_step writes the token each running beam appended, next_ids [R], and when non-NULL the
 *    running log-prob sums, scores [R]; wcb_decode_parents then gives parents [R] (int32, DEVICE): the
 *    beam (0..nb-1 of the same utterance) each running beam extends — the running sequences are the
 *    parents' sequences plus next_ids. Once every utterance is done a step changes nothing.
 *    Once every utterance is done (wcb_decode_info's *done) the search is frozen: a step writes parents =
 *    identity and next_ids = pad_token_id, so a consumer that extends its hypotheses every step is unchanged.
 *  - wcb_decode_info: *max_new = the state's column capacity (max_target_positions - prefix_len for
 *    wcb_decode_begin, max_new_tokens for wcb_decode_begin_beams), *steps = the steps taken, *done = 1 once
 *    every utterance (row) has finished (blocks on the decode stream for it); each pointer may be NULL.
 *  - wcb_decode_result: out_ids [B][out_ld] (int32, DEVICE) receives the n generated columns, *out_steps
 *    (host) = n: greedy, the steps taken (finished rows padded); beams, the best finished sequence of each
 *    utterance so far with n its longest length — after the steps generate() takes, exactly generate()'s
 *    output. out_ld < n is refused (WCB_ERR_ARG); out_ld = *max_new always holds the result. */
typedef struct wcb_state wcb_state;
int wcb_decode_begin(wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prefix, int prefix_len,
                     float bias_boost, int min_new_tokens, wcb_state** out, void* stream);
int wcb_decode_begin_beams(wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prefix, int prefix_len,
                           int max_new_tokens, float bias_boost, int min_new_tokens, wcb_state** out, void* stream);
int wcb_decode_step(wcb_handle* h, wcb_state* st, const wcb_bias* bias, int32_t* next_ids, float* scores, void* stream);
int wcb_decode_parents(wcb_handle* h, wcb_state* st, int32_t* parents, void* stream);
int wcb_decode_info(wcb_handle* h, wcb_state* st, int32_t* max_new, int32_t* steps, int32_t* done);
int wcb_decode_result(wcb_handle* h, wcb_state* st, int32_t* out_ids, int out_ld, int32_t* out_steps, void* stream);
int wcb_decode_end(wcb_handle* h, wcb_state* st);

/* wait for every queued front-end / encoder / decode operation of the handle */
int wcb_synchronize(wcb_handle* h);

/* replaces forward(input_features, decoder_input_ids) (models/whisper_medical.py:45-111):
 * dec_ids int32 DEVICE [B][T] → logits f32 DEVICE [B][T][vocab]; enc_out as in wcb_encode. */
int wcb_forward(wcb_handle* h, const float* mel, int B, const int32_t* dec_ids, int T, float* logits,
                void* enc_out, void* stream);

/* replaces forward(encoder_outputs=..., decoder_input_ids) (models/whisper_medical.py:54-55, 93-111, the
 * decoder on a given encoder output, no re-encode): enc = encoder output [B][1500][d] in the model dtype
 * (DEVICE, e.g. wcb_encode's enc_out; copied / projected, not retained) → logits as wcb_forward, bit for
 * bit the logits wcb_forward computes from the mel that produced enc. */
int wcb_forward_enc(wcb_handle* h, const void* enc, int B, const int32_t* dec_ids, int T, float* logits, void* stream);

/* replaces forward(..., use_cache=True) / forward(..., past_key_values=...) (models/whisper_medical.py:54-55,
 * 89-110: the decoder's self-attention KV cache carried between calls): `st` = a step-wise state begun with
 * wcb_decode_begin(enc, B, 1, NULL, ...) (it owns the encoder output and the cache); each call appends
 * positions [n, n + T) for dec_ids [B][T] (int32, DEVICE), n = the positions appended so far, and writes
 * their logits [B][T][vocab] (f32, DEVICE). A state used here takes no wcb_decode_step. */
int wcb_forward_cached(wcb_handle* h, wcb_state* st, const int32_t* dec_ids, int T, float* logits, void* stream);

/* bias list: n_phrases token sequences, phrase i = tokens[offsets[i] .. offsets[i+1]) (host
 * arrays), built into an Aho-Corasick automaton on the device. word_start (host, [vocab] bytes, or
 * NULL = every token) marks the tokens a match may START at — for a BPE vocabulary the tokens that
 * begin a word (leading space); tokenise phrases as they appear inside a transcript. Boost
 * semantics (oracle/bias_ref.py, k_select.hip): each token scores +lam·n(s, v) where n counts the
 * tokens the transition adds to the current match minus the dropped, unfinished ones (retraction);
 * completed phrases keep their bonus.
 * Lifetime: an automaton belongs to the handle that created it; wcb_bias_destroy waits for that
 * handle's queued work and drops the decode graphs that captured it (serialise it with the handle's
 * other calls, like every call on a handle). It may outlive the handle (destroy it afterwards). */
int wcb_bias_create(wcb_handle* h, const int32_t* tokens, const int32_t* offsets, int n_phrases,
                    const uint8_t* word_start, wcb_bias** out);
void wcb_bias_destroy(wcb_bias* b);
int wcb_bias_num_states(const wcb_bias* b);

/* Per-utterance bias lists: clip b of a batch is boosted with its own phrase list L_b (possibly empty), every
 * decoder row of clip b (greedy: row b; beams: rows b·nb .. b·nb+nb-1) scored exactly as one wcb_bias of L_b
 * would score it; the same lambda and word_start mask for every clip.
 * wcb_bias_batch_create compiles B automata into one forest: phrase p = tokens[phrase_off[p] ..
 * phrase_off[p+1]), clip b owns phrases clip_off[b] .. clip_off[b+1]) (host arrays; phrase_off has
 * clip_off[B] + 1 entries). One state space with a root state per clip: trans_off / trans_tok / trans_dst /
 * st_depth / st_keep are global CSR arrays as in wcb_bias, and each clip's gated root children are a
 * token-sorted list (rc_off[B+1], rc_tok, rc_dst) — no vocabulary-sized array per clip. The object is HOST
 * data bound to no stream: a decode call copies it (asynchronously, on the decode stream) into device buffers
 * the handle owns, so it may be destroyed as soon as that call returns, async_out = 1 included. Token ids
 * outside [0, vocab), decreasing offsets and B outside 1..64 are WCB_ERR_ARG.
 * wcb_bias_batch_num_states: the states of clip `clip`'s automaton (root included), clip = -1: of the forest. */
int wcb_bias_batch_create(wcb_handle* h, int B, const int32_t* tokens, const int32_t* phrase_off,
                          const int32_t* clip_off, const uint8_t* word_start, wcb_bias_batch** out);
void wcb_bias_batch_destroy(wcb_bias_batch* bb);
int wcb_bias_batch_num_states(const wcb_bias_batch* bb, int clip);

/* wcb_generate with the forest in place of the shared automaton (bb built for exactly B clips, else
 * WCB_ERR_ARG). The device buffers the forest is copied into have a capacity that only grows (a larger forest
 * waits for the handle's queued work and reallocates); the captured decode graph reads the forest through
 * them, so successive calls with different lists within the capacity replay the same graph. */
int wcb_generate_biased(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias_batch* bb,
                        const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream);

/* installs the forest on a step-wise state: after wcb_decode_begin / wcb_decode_begin_beams (bb built for
 * the state's B clips), before the first wcb_decode_step; every wcb_decode_step of that state must then be
 * given bias = NULL (a non-NULL bias is WCB_ERR_ARG). */
int wcb_decode_bias_batch(wcb_handle* h, wcb_state* st, const wcb_bias_batch* bb);

/* Token log-probabilities and sequence scores.
 *  - token log-prob (greedy): logprob[b][t] = logit[b][t][tok] − logsumexp_v(logit[b][t][v]) over the RAW f32
 *    logits of step t — the model's own distribution. The bias boost and the min_new_tokens EOS mask change
 *    which token is chosen; they never enter the log-prob (a phrase forced in by lambda shows as a low log-prob
 *    under a boosted token). A position where an already finished row emits pad holds 0.0f; the EOS a row
 *    emits itself carries its real log-prob. Computed on chip: the LM head keeps per (row, workgroup) online-
 *    softmax partials (max, Σ exp(v − max)) of the columns it walks beside its argmax partials, and the
 *    selection kernel merges them in a fixed order (deterministic for a given "lm_walkers").
 *  - sequence score (beam search): seq_score[b] = the score of the returned (best finished) hypothesis of clip
 *    b, HF's sequences_scores: the length-normalised sum of its processed (boosted) token log-probs.
 *  - With both off every existing path launches exactly what it launched before; with log-probs on the
 *    selected ids are bit-identical to the same call with them off, in every dtype.
 * wcb_generate_scored: wcb_generate (bias, bb = NULL) / wcb_generate_biased (bb) with the scores; at most one of
 * bias / bb non-NULL (else WCB_ERR_ARG). Greedy: out_logprobs f32 DEVICE [B][cfg->max_new_tokens], laid out and
 * copied out like out_ids (async_out included), out_seq_scores must be NULL. Beams: out_seq_scores f32 DEVICE
 * [B], out_logprobs must be NULL. The wrong pointer for the mode: WCB_ERR_UNSUPPORTED. Both NULL: exactly
 * wcb_generate / wcb_generate_biased. A scored greedy decode replays a captured graph of its own, kept beside
 * the unscored one of its decode context. */
int wcb_generate_scored(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                        const wcb_bias_batch* bb, const int32_t* prefix, int prefix_len, int32_t* out_ids,
                        float* out_logprobs, float* out_seq_scores, int32_t* out_steps, void* stream);
/* step-wise: after wcb_decode_begin and before the first wcb_decode_step, on a greedy state (a beam-search
 * state: WCB_ERR_UNSUPPORTED; after a step or on a forward cache: WCB_ERR_STATE). Every step then also records
 * the log-prob of the token it chose. */
int wcb_decode_enable_logprobs(wcb_handle* h, wcb_state* st);
/* shaped like wcb_decode_result: out [B][out_ld] (f32, DEVICE) receives the log-probs of the n steps taken so
 * far, *out_steps (host) = n; out_ld < n is WCB_ERR_ARG; log-probs not enabled: WCB_ERR_STATE. */
int wcb_decode_logprobs(wcb_handle* h, wcb_state* st, float* out, int out_ld, int32_t* out_steps, void* stream);

/* Temperature sampling (greedy decodes): the token of a step is drawn from softmax(score / T), score = logit +
 * bias boost (a masked EOS stays excluded), as a perturbed argmax — Gumbel-max — inside the kernels that take
 * the argmax today, with no logits leaving the chip:
 *   x[v] = fmaf(score[v], 1.0f / T, g(seed, t, v)),  token = argmax_v x[v] (lowest index on ties)
 *   g(seed, t, v) = -logf(-logf(u)),  u = ((r >> 9) + 0.5f) * 2^-23 (exact in f32, 0 < u < 1),
 *   r = philox4x32_10(counter (v >> 2, t, 0, 0), key (lo32(seed), hi32(seed)))[v & 3]
 * with seed the clip's 64-bit seed and t the 0-based index of the generated token (csrc/sample.h holds the one
 * definition the kernels and wcb_sample_noise compile). A decode is a pure function of (inputs, seeds, T): the
 * same seeds give the same tokens, in generate and step-wise, eager and graph replay, whatever the batch split.
 * Token log-probs keep their meaning (raw logit - logsumexp of the raw logits: untempered, no boost). Step-wise,
 * wcb_decode_step's `scores` holds the winner's perturbed value x (not its boosted logit). Seeds and 1/T are
 * copied on the decode stream into a buffer of the decode context (the host array may be freed on return,
 * async_out = 1 and several decode contexts in flight included); a sampled decode replays a captured graph of
 * its own, kept beside the unscored and scored ones, whose key never contains the seeds or the temperature.
 * With sampling off every existing path launches exactly the kernels, arguments and graphs it launched before.
 * Errors: temperature <= 0 or not finite, NULL seeds: WCB_ERR_ARG; num_beams > 1 / a beam-search state:
 * WCB_ERR_UNSUPPORTED; both bias and bb: WCB_ERR_ARG. */
typedef struct { float temperature;        /* > 0 */
                 const uint64_t* seeds;    /* HOST [B], one per clip */ } wcb_sample_cfg;

/* wcb_generate_scored's greedy form with sampling; out_logprobs may be NULL */
int wcb_generate_sampled(wcb_handle*, const float* mel, int B, const wcb_gen_cfg*, const wcb_sample_cfg*,
                         const wcb_bias*, const wcb_bias_batch*, const int32_t* prefix, int prefix_len,
                         int32_t* out_ids, float* out_logprobs, int32_t* out_steps, void* stream);
/* after wcb_decode_begin, before the first step, greedy state only (beam state: WCB_ERR_UNSUPPORTED;
   after a step or on a forward cache: WCB_ERR_STATE); seeds HOST [B] */
int wcb_decode_enable_sampling(wcb_handle*, wcb_state*, float temperature, const uint64_t* seeds);
/* wcb_op_lm_head_lse with the perturbed argmax: seeds HOST [M]; sampled[M] int32 DEVICE */
int wcb_op_lm_head_sample(int dtype, const void* A, const void* W, int M, int V, int K, int walkers,
                          float temperature, const uint64_t* seeds, int step, float* logits, long ld,
                          float* lse, int32_t* sampled, void* stream);

/* Per-clip prompts of different lengths in one greedy batch. Clip b's prompt of prompt_len[b] tokens
 * — the decoder start token last, so 1 = no prompt — sits right-aligned in row b of `prompts` HOST [B][prompt_ld]:
 * columns prompt_ld - prompt_len[b] .. prompt_ld - 1; the columns before it are ignored (the library writes the pad
 * token there). Clip b decodes exactly as it decodes alone with that prompt as `prefix`: its position embeddings
 * count from its own first token and its self-attention never reads the slots before it, while the step counter,
 * the K/V write slot and the captured graph stay those of a prompt_ld-long dense prompt. Both arrays are copied on
 * the decode stream through pinned staging: they are free on return, async_out = 1 included; the graph key holds
 * the fact "ragged", never the lengths. All lengths equal to prompt_ld: the dense kernels.
 * wcb_generate_prompted = wcb_generate_sampled (smp non-NULL) / wcb_generate_scored's greedy form (smp NULL;
 * out_logprobs may be NULL) with these prompts; it composes with the shared automaton, the bias batch, log-probs,
 * sampling and the handle's token rules. out_ids [B][cfg->max_new_tokens] as every wcb_generate*: the generated
 * columns only. wcb_decode_begin_prompted = wcb_decode_begin's greedy form; wcb_decode_step / _result / _logprobs /
 * _enable_logprobs / _enable_sampling / _bias_batch then work on the state as on any greedy one.
 * Errors: prompt_len[b] outside [1, prompt_ld], prompt_ld + max_new_tokens > max_target_positions + 1 (the rule of
 * prefix_len): WCB_ERR_ARG; num_beams > 1: WCB_ERR_UNSUPPORTED (beam scores are normalised by a length that counts
 * the prompt, so a clip would not decode as it does alone). wcb_align (token timestamps) takes one shared prefix:
 * not after a ragged call with enc = NULL. */
int wcb_generate_prompted(wcb_handle*, const float* mel, int B, const wcb_gen_cfg*, const wcb_sample_cfg*,
                          const wcb_bias*, const wcb_bias_batch*, const int32_t* prompts, int prompt_ld,
                          const int32_t* prompt_len, int32_t* out_ids, float* out_logprobs, int32_t* out_steps,
                          void* stream);
int wcb_decode_begin_prompted(wcb_handle*, const void* enc, int B, const int32_t* prompts, int prompt_ld,
                              const int32_t* prompt_len, float bias_boost, int min_new_tokens, wcb_state** out,
                              void* stream);
/* HOST, no GPU: out[i] = g(seed, step, v0 + i), the same inline function the kernels compile */
int wcb_sample_noise(uint64_t seed, int step, int v0, int n, float* out);

/* ---- token rules of the greedy decoder: deny lists and Whisper's timestamp grammar, applied on the chip at
 * every step (HF SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and
 * WhisperTimeStampLogitsProcessor with _detect_timestamp_from_logprob; semantics: csrc/tsrule.h).
 * With t tokens generated after the prompt: `suppress` ids are never chosen, `begin_suppress` ids not at t == 0;
 * with timestamps = 1 the row follows the timestamp grammar over the ids >= timestamp_begin (pairs, never
 * decreasing, a first timestamp of at most timestamp_begin + max_initial_timestamp_index, a timestamp whenever
 * the timestamps' summed probability exceeds the best text token's) and no_timestamps_token_id is never chosen.
 * A row whose every token is excluded emits EOS. Token log-probs are unaffected (raw log-softmax). */
typedef struct { const int32_t* suppress; int n_suppress;
                 const int32_t* begin_suppress; int n_begin_suppress;
                 int timestamps;                 /* 0 / 1 */
                 int timestamp_begin, no_timestamps_token_id;   /* read with timestamps = 1 */
                 int max_initial_timestamp_index; /* < 0: no limit */ } wcb_token_rules;
/* Handle state, like a generation config: applies to every greedy decode begun afterwards (wcb_generate, _biased,
 * _scored, _sampled, wcb_decode_begin / wcb_decode_step); NULL removes the rules. Waits for queued work, then
 * uploads the two deny bitmaps into handle-owned buffers. WCB_ERR_STATE before wcb_finalize_weights or while a
 * step-wise decode is open; WCB_ERR_ARG for an id outside [0, vocab), timestamp_begin outside (eos, vocab), or,
 * with timestamps = 1, a deny id >= timestamp_begin. With rules installed num_beams > 1 is WCB_ERR_UNSUPPORTED;
 * with timestamps = 1 so is a sampled decode. Ruled decodes replay captured graphs of their own. */
int wcb_set_token_rules(wcb_handle*, const wcb_token_rules* /* NULL: none */);
/* HOST, no GPU: scores[vocab] of a row that generated `generated[0..n)`: -inf written exactly where the device
 * excludes a token (rule 5 in double), so argmax(scores) is the device's token (all -inf: EOS). */
int wcb_token_rules_apply_host(const wcb_token_rules*, int vocab, int eos, const int32_t* generated, int n,
                               float* scores);
/* The LM head with the deny bitmap plus the rule reduction of the finalize on caller operands (as
 * wcb_op_lm_head_lse; lam = 0, no EOS mask): row m has generated `generated[m·gen_ld .. + lens[m])` (HOST);
 * next_ids[M] int32 DEVICE. Rows at t == 0 and t > 0 in one call with begin_suppress ids and no timestamps:
 * WCB_ERR_ARG (the bitmap of a launch is chosen by its step). */
int wcb_op_lm_head_rules(int dtype, const void* A, const void* W, int M, int V, int K, int walkers,
                         const wcb_token_rules* rules, int eos, const int32_t* generated, int gen_ld,
                         const int32_t* lens, float* logits, long ld, int32_t* next_ids, void* stream);

/* ---- repeat rules of the greedy decoder: HF's repetition_penalty and no_repeat_ngram_size, applied on the chip at
 * every step (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor; semantics: csrc/reprule.h, DESIGN.md
 * §5i). hist = what HF's processors see as input_ids for the row: its live prompt tokens, the start token, the
 * forced language / task tail (a detected language included) and every token generated so far; the dead left-padding
 * slots of a ragged batch are not part of it. On the raw f32 logits, before the boost, the EOS mask and the deny lists:
 *   repetition_penalty p > 0:  x[v] = x[v] < 0 ? x[v]·p : x[v] / p  for every distinct v in hist (f32: one multiply or
 *                              one correctly rounded division)
 *   no_repeat_ngram_size n:    with L = len(hist) >= n >= 1, x[hist[i+n-1]] = -inf for every i in [0, L-n] whose n-1
 *                              tokens from hist[i] equal the last n-1 tokens of hist
 * p = 1 and n = 0 mean off. Token log-probs are unaffected (raw log-softmax). */
typedef struct { float repetition_penalty; int no_repeat_ngram_size; } wcb_repeat_rules;
/* Handle state, like wcb_set_token_rules: applies to every greedy decode begun afterwards (wcb_generate, _biased,
 * _scored, _prompted, _lang, wcb_decode_begin* / wcb_decode_step); NULL removes the rules. No device work: every decode
 * writes the two values into its own context on its stream, so decodes with different values replay one captured
 * graph. WCB_ERR_STATE before wcb_finalize_weights or while a step-wise decode is open; WCB_ERR_ARG for a penalty that
 * is not finite or <= 0, or n < 0. With the rules installed, refused at decode time with WCB_ERR_UNSUPPORTED:
 * num_beams > 1, a sampled decode, token rules with timestamps = 1, wcb_generate_windows, and a model with more than
 * 448 text positions or more than 53248 vocabulary entries (the history and the banned set of a row live in LDS). */
int wcb_set_repeat_rules(wcb_handle*, const wcb_repeat_rules* /* NULL: none */);
/* HOST, no GPU: both rules applied in place to scores[vocab] of a row whose history is hist[0..n_hist) — the same
 * inline functions the kernels compile. WCB_ERR_ARG for an id outside [0, vocab). */
int wcb_repeat_rules_apply_host(const wcb_repeat_rules*, int vocab, const int32_t* hist, int n_hist, float* scores);
/* The LM head with the per-row seen bitmap plus the history pass of the finalize on caller operands (as
 * wcb_op_lm_head_rules; lam = 0, no EOS mask): row m's history is hist[m·hist_ld .. + lens[m]) (HOST, 1 <= lens[m] <=
 * min(hist_ld, 448)); the bitmap is built from it by the decode-start kernel; next_ids[M] int32 DEVICE, logits f32. */
int wcb_op_lm_head_repeat(int dtype, const void* A, const void* W, int M, int V, int K, int walkers,
                          const wcb_repeat_rules* rules, int eos, const int32_t* hist, int hist_ld,
                          const int32_t* lens, float* logits, long ld, int32_t* next_ids, void* stream);

/* ---- token-level timestamps from cross-attention (HF return_token_timestamps / _extract_token_timestamps, per
 * clip and batch-invariant; semantics: csrc/dtw.h). A teacher-forced post-pass over the ids any
 * decode produced: the causal prefill of wcb_forward_enc with the LM head off and a capture kernel after the cross
 * query of every layer that has selected heads; the column statistics, median filter, head mean, the DTW and its
 * backtrace all run on the chip. For a clip with generated columns g[0..n), e = its first EOS (n: none), prefix
 * length P, S_b = num_frames[b] / 2:
 *   rows      i in [0, m), m = min(e, n - 1): the cross-attention of the position whose input is g[i] (P + i)
 *   weights   softmax over all n_audio_ctx frames, cropped to S_b afterwards; per (head, frame) normalised over the
 *             m rows (population std; a column with std 0 gives 0), median filter of `median_width` along the
 *             frames (reflect padding), M = -(mean over the heads), f32
 *   frame[i]  = the time index of the first DTW path cell of row i; rows >= m repeat frame[m - 1]; m <= 1: 0
 * heads HOST [n_heads][2] = (layer, head) pairs (n_heads 0 / heads NULL: every head of the layers >= n_layers / 2);
 * num_frames HOST [B] mel frames of every clip (NULL: all 2 * n_audio_ctx). */
typedef struct { const int32_t* heads; int n_heads;
                 int median_width;              /* odd, 1 .. 15 */
                 const int32_t* num_frames; } wcb_align_cfg;
/* ids int32 DEVICE [B][ld] (columns [0, n) read; ld >= n), prefix / prefix_len as wcb_generate, out_frames int32
 * DEVICE [B][n], matrix_out f32 DEVICE [B][n - 1][n_audio_ctx] or NULL (rows < m, columns < S_b written).
 * enc = encoder output [B][n_audio_ctx][d] in the model dtype (DEVICE, as wcb_forward_enc), or NULL: the encoder
 * state the handle's latest wcb_generate* call left in its decode context — the pass is queued on that context's
 * stream behind the decode (async_out decodes included), the next call's encoder waits for it, and `stream` is
 * made to wait for the pass (no host wait); post-passes of one handle run one after the other, whichever decode
 * context each uses: they share the handle's workspaces; WCB_ERR_STATE
 * when there is none, B differs, or another call took the context since. WCB_ERR_ARG: a head out of range, more
 * than 32 selected heads in one layer, an even or non-positive width, num_frames outside [2 * median_width,
 * 2 * n_audio_ctx], B > 64, prefix_len + n - 1 > n_text_ctx; a width above 15: WCB_ERR_UNSUPPORTED. The weights
 * workspace [clips][heads][n - 1][n_audio_ctx] f32 is bounded (1 GiB; option "align_ws", MiB): above it the clips are
 * processed in groups, one teacher-forced pass per group. */
int wcb_align(wcb_handle* h, const void* enc, int B, const int32_t* ids, int ld, int n, const int32_t* prefix,
              int prefix_len, const wcb_align_cfg* cfg, int32_t* out_frames, float* matrix_out, void* stream);
/* The capture kernel on caller operands, as one layer of one teacher-forced pass runs it: query rows q [clips * rps][ldq]
 * in `dtype` (row clip * rps + j is position pos0 + j of that clip, head h at column h * q_hstride, `dim` values),
 * keys by `layout`: 0 the cross-K cache [clips][H][S][64] (dim = 64), 1 the encoder output [clips][S][dim] in rows,
 * 2 the same, laid out fragment-major by the op first (16-bit, the widths the encoder-space decode covers) ->
 * w f32 DEVICE [nclip][nh][nrow][S]: for the clips [clip0, clip0 + nclip), the heads `heads` HOST [nh] and the
 * alignment rows i = pos0 + j - P in [0, nrow), softmax over the S keys of q . key; other rows are not written.
 * Blocks until done. */
int wcb_op_align_capture(int dtype, const void* q, long ldq, int q_hstride, const void* keys, int layout, int clips,
                         int H, int dim, int S, int rps, int pos0, int P, int nrow, int clip0, int nclip,
                         const int32_t* heads, int nh, float* w, void* stream);
/* The matrix kernel on caller operands: w f32 DEVICE [N][heads][m_max][S_ld], lens int32 DEVICE [N] (rows of every
 * item), frames int32 DEVICE [N] (S_b of every item, NULL: S_ld) -> M f32 DEVICE [N][m_max][S_ld]. m_max <= 447. */
int wcb_op_align_matrix(const float* w, int N, int heads, int m_max, int S_ld, const int32_t* lens,
                        const int32_t* frames, int median_width, float* M, void* stream);
/* The DTW kernel on caller operands: M f32 DEVICE [N][m_max][S_ld], lens / frames as above -> out_frames int32
 * DEVICE [N][n_out] and, when path_text is non-NULL, the path as path_text / path_time int32 DEVICE [N][m_max +
 * S_ld] with its length path_len int32 DEVICE [N]. Blocks until done (it may own a trace workspace). */
int wcb_op_dtw(const float* M, int N, int m_max, int S_ld, const int32_t* lens, const int32_t* frames, int n_out,
               int32_t* out_frames, int32_t* path_text, int32_t* path_time, int32_t* path_len, void* stream);
/* HOST, no GPU: the same recurrence (csrc/dtw.h) on M [m][ld] (S columns read): frames [n_out] as above, and when
 * path_text is non-NULL the path (capacity m + S each) and *path_len. */
int wcb_dtw_host(const float* M, int m, int S, long ld, int32_t* frames, int n_out, int32_t* path_text,
                 int32_t* path_time, int32_t* path_len);

/* ---- long-form transcription: audio past 30 s (HF WhisperGenerationMixin's long-form branch; the seek loop itself runs
 * on the host, whisper_context_biasing_amd/longform.py; semantics: DESIGN.md §5g).
 * wcb_log_mel_long: the feature extractor with truncation = False, padding = "longest": pcm f32 DEVICE [B][pcm_stride],
 * clip b's first n_valid[b] samples valid (HOST [B]) and the rest up to n_total read as zero, reflect padding resolved at
 * n_total -> mel_out f32 DEVICE [B][n_mel][T_ld], T = n_total / 160 frames written per row (columns T .. T_ld - 1 are not
 * touched), the max - 8 clamp over all T frames of the clip. Like wcb_log_mel it needs no weights (any created handle).
 * WCB_ERR_ARG: B outside 1..64, n_total < 800 or > pcm_stride, T_ld < T, n_valid[b] outside [0, n_total]. */
int wcb_log_mel_long(wcb_handle* h, const float* pcm, int B, const int32_t* n_valid, int n_total, int64_t pcm_stride,
                     float* mel_out, int T_ld, void* stream);
/* The windows of one decode: row r is the 3000-frame window of clip clip_idx[r] that starts at mel frame seek[r] and
 * holds seek_num_frames[r] frames, zero (0.0 in the feature domain, HF _get_input_segment) from there to frame 3000.
 * mel f32 DEVICE [clips][n_mel][T_ld] with T valid frames per row; the three int arrays are HOST [rows] and are copied
 * on the encoder stream (free on return). The cut writes the encoder's conv-input layout directly: no [rows][n_mel][3000]
 * intermediate. WCB_ERR_ARG: rows outside 1..64, clip_idx outside [0, clips), seek < 0, seek_num_frames outside
 * [1, 3000], seek + seek_num_frames > T, T > T_ld. */
typedef struct { const float* mel; int clips, T, T_ld;
                 const int32_t* clip_idx; const int32_t* seek; const int32_t* seek_num_frames; } wcb_windows;
/* wcb_encode after the cut: enc_out [rows][1500][d] as wcb_encode's. With T = T_ld = 3000, seek 0 and 3000 frames it is
 * bit for bit wcb_encode of the same features. */
int wcb_encode_windows(wcb_handle* h, const wcb_windows* w, int rows, void* enc_out, void* stream);
/* wcb_generate_prompted's greedy, unsampled form on the windows (out_logprobs may be NULL), plus out_no_speech f32 DEVICE
 * [rows] (nullable; needs out_logprobs, else WCB_ERR_UNSUPPORTED): no_speech_prob[r] = exp(logit[<|nospeech|>] -
 * logsumexp(raw logits)) at the start token's position — the logits of generation step 0 — with <|nospeech|> the id
 * before <|notimestamps|>. The scored finalize writes it from the logsumexp it merges for the token log-probs: no logits
 * leave the chip; boost, deny lists and grammar never enter it. Decodes with it on replay graphs of their own; with it
 * off every path launches what it launched before. num_beams > 1: WCB_ERR_UNSUPPORTED. */
int wcb_generate_windows(wcb_handle* h, const wcb_windows* w, int rows, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                         const wcb_bias_batch* bb, const int32_t* prompts, int prompt_ld, const int32_t* prompt_len,
                         int32_t* out_ids, float* out_logprobs, float* out_no_speech, int32_t* out_steps, void* stream);
/* step-wise: after wcb_decode_enable_logprobs and before the first step (else WCB_ERR_STATE; beam state:
 * WCB_ERR_UNSUPPORTED); wcb_decode_no_speech copies the [B] probabilities out once a step was taken. */
int wcb_decode_enable_no_speech(wcb_handle* h, wcb_state* st);
int wcb_decode_no_speech(wcb_handle* h, wcb_state* st, float* out, void* stream);
/* the window cut on caller operands: xt [rows][3002][n_mel] in `dtype`; arguments and errors as wcb_windows. Blocks. */
int wcb_op_window_cut(int dtype, const float* mel, int clips, int n_mel, int T, int T_ld, int rows, const int32_t* clip_idx,
                      const int32_t* seek, const int32_t* seek_num_frames, void* xt, void* stream);

/* ---- language prompts and per-clip language detection (HF generate(language=, task=) / detect_language; semantics:
 * DESIGN.md §5h, csrc/k_lang.hip). The language tokens are the ids [lang_begin, lang_begin + n_lang) right after the
 * decoder start token (Whisper: lang_begin = decoder_start_token_id + 1, n_lang = 99 or 100). Detection is one decoder
 * pass over [decoder_start] at position 0 on the cross-attention state of the call's own decode context — a greedy
 * step without selection whose LM head is the language head: f32 logits of the 16-column tiles that cover the range
 * only, the final LayerNorm fused — then lang_finalize_kernel, one wave per row: columns outside the range and
 * non-candidates masked, (max, Σexp) and the argmax (lowest index on ties) reduced in a fixed order, so a clip's
 * result never depends on its batch. No logits leave the chip.
 * wcb_detect_language: enc = encoder output [B][1500][d] in the model dtype (DEVICE, as wcb_decode_begin's: copied /
 * projected into the step-wise decode context, so WCB_ERR_STATE while a step-wise decode is open) -> out_ids int32
 * DEVICE [B] (token ids), out_probs f32 DEVICE [B][n_lang] or NULL (softmax over the candidate languages, 0 elsewhere).
 * candidates: HOST bitmap of n_lang bits (bit i of word i / 32 = language lang_begin + i may be chosen; copied by
 * value on the decode stream, free on return) or NULL = every language.
 * Errors: B outside 1..64, a range that does not lie inside (eos_token_id, vocab) or n_lang outside 1..113:
 * WCB_ERR_ARG; a candidate bitmap with no bit set: WCB_ERR_ARG. */
int wcb_detect_language(wcb_handle* h, const void* enc, int B, int lang_begin, int n_lang, const uint32_t* candidates,
                        int32_t* out_ids, float* out_probs, void* stream);
/* A language slot in per-clip prompts: every row of `prompts` holds, column_from_end columns before its last one (the
 * column prompt_ld - 1 - column_from_end, the same for all rows in the right-aligned layout), a language token that the
 * library fills in on the device: after the encoder the detection pass runs in the decode stream, the finalize stores
 * every row's id into that column of the context's prompt rows, then the ordinary (ragged) prefill reads them — the
 * prefill overwrites self-attention slot 0, and the pass advances no per-row decode state (automaton states, timestamp
 * words, log-prob sums, step and sampling counters). The pass is eager like the prefill; the step graphs are those of
 * the same call without the slot, so other audio, languages or candidates capture nothing. out_ids (DEVICE [B],
 * nullable) / out_probs (DEVICE [B][n_lang], nullable) receive what wcb_detect_language writes. */
typedef struct { int lang_begin, n_lang;
                 const uint32_t* candidates;     /* HOST bitmap of n_lang bits, NULL: every language */
                 int column_from_end;            /* >= 0; every prompt_len[b] must be >= column_from_end + 2 */
                 int32_t* out_ids; float* out_probs; } wcb_lang_cfg;
/* wcb_generate_prompted / wcb_decode_begin_prompted with the slot (lang = NULL: exactly those). Errors as theirs and
 * as wcb_detect_language's; a prompt_len[b] < column_from_end + 2: WCB_ERR_ARG; num_beams > 1 with a language slot:
 * WCB_ERR_UNSUPPORTED. */
int wcb_generate_lang(wcb_handle*, const float* mel, int B, const wcb_gen_cfg*, const wcb_sample_cfg*, const wcb_bias*,
                      const wcb_bias_batch*, const int32_t* prompts, int prompt_ld, const int32_t* prompt_len,
                      const wcb_lang_cfg* lang, int32_t* out_ids, float* out_logprobs, int32_t* out_steps, void* stream);
int wcb_decode_begin_lang(wcb_handle*, const void* enc, int B, int num_beams, const int32_t* prompts, int prompt_ld,
                          const int32_t* prompt_len, const wcb_lang_cfg* lang, float bias_boost, int min_new_tokens,
                          wcb_state** out, void* stream);
/* The language head and its finalize on caller operands (as wcb_op_lm_head_rules; no LayerNorm): A [M][K], W [V][K] in
 * dtype (M <= 64, K <= 2560) -> logits f32 DEVICE [M][ld] (ld >= V; only the columns of the 16-column tiles that cover
 * the range are written, cut at V), out_ids int32 DEVICE [M], out_probs f32 DEVICE [M][n_lang] or NULL; candidates HOST
 * or NULL. The range must lie inside [0, V). Blocks until done. */
int wcb_op_lang_head(int dtype, const void* A, const void* W, int M, int V, int K, int lang_begin, int n_lang,
                     const uint32_t* candidates, int32_t* out_ids, float* out_probs, float* logits, long ld, void* stream);

/* debug counters by name (not part of wcb_profile_read): "graph_captures" = decode graphs instantiated so
 * far on this handle. Unknown name: WCB_ERR_ARG. */
int wcb_debug_counter(const wcb_handle* h, const char* name, int64_t* out);

/* per-kernel time accounting for the benchmark's roofline. enable bit 0: HIP events around every
 * front-end / encoder launch on its stream; bit 1: device time stamps (s_memrealtime) written by the
 * decode cross-attention kernel, which runs inside the replayed step graph where events cannot
 * bracket a single node. 0 disables; counters are reset. */
int wcb_profile_enable(wcb_handle* h, int enable);
/* fills up to n entries: name, launches, total milliseconds, algorithmic flops, algorithmic bytes */
int wcb_profile_read(wcb_handle* h, int n, char (*names)[32], int64_t* launches, double* ms,
                     double* flops, double* bytes);

/* entry i of wcb_profile_read: the (demangled) kernel symbol of the class's first launch and its grid
 * in threads (x·y·z), as rocprofv3 names them (Kernel_Name; Grid_Size = Grid_Size_X·Y·Z); "" when the class
 * launched nothing or was stamped on the device */
int wcb_profile_kernel(wcb_handle* h, int i, char* name, int cap, int64_t* grid);

/* debug: copy an internal workspace buffer (xt, hbuf, x, h, qkv, att, ffn, encout, xkv, logits; step_logits:
 * the step-wise decode's last logits rows, row stride = vocab rounded up to a multiple of 128)
 * into dst (device) after synchronising; enc_layers limits later encodes to that many layers
 * (-1 = all). bytes == 0 only sets the limit. */
int wcb_debug_copy(wcb_handle* h, const char* name, void* dst, int64_t bytes, int enc_layers);

/* ---- kernel-level entry points (parity tests and microbenchmarks) ---- */
/* out[M][N] = act(A[M][K] · W[N][K]ᵀ + bias) (+ resid), row-major, dtype of A/W = dtype */
int wcb_op_gemm(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act,
                const float* resid, void* out, int out_f32, void* stream);
/* the same with the encoder-GEMM kernel chosen: kernel 1 = the ping-pong kernel where it covers the shape
 * and is the faster one (16-bit, N % 256 == 0, K % 64 == 0, K >= 128, M >= 256; the LDS-ring kernel's
 * 256x192 tiles where those leave fewer tile rounds), 4 = the same with the ping-pong kernel's own 192-wide
 * tiles there (option "enc_gemm"), 2 / 5 = the ping-pong kernel's 256- / 192-wide tiles for every shape they
 * cover (residual epilogue included), 0 = the LDS-ring / tile kernels; decode-row (beam) tiles, 16-bit,
 * M > 64: 6 = the LDS-ring tiles, 10·FM + FN (11, 12, 21, 22, 41, 42, 51, 52) = the wide single-burst
 * tiles of 16·FM rows x 16·FN columns (K = 768, 1024 or 1280; resid, when given, must equal out; a shape
 * the wide tiles do not cover runs on the ring tiles), 100 + that: W given fragment-major
 * ([N / 16][K / 32][64 lanes][8]: element (n, k) at lane 16·((k % 32) / 8) + n % 16, slot k % 8) */
int wcb_op_gemm_kernel(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act,
                       const float* resid, void* out, int out_f32, int kernel, void* stream);
/* decode-step fused form: out[M][N] = act(LN(X) · W[N][K]ᵀ + bias), X f32 [M][K] (M <= 64), with the
 * LayerNorm row statistics taken from stats[M][K/16][2] = per-16-column (Σx, Σx²) partials */
int wcb_op_gemm_ln(int dtype, const float* X, const float* ln_w, const float* ln_b, const float* stats,
                   const void* W, int M, int N, int K, const float* bias, int act, void* out, int out_f32,
                   void* stream);
/* the decode step's input embedding as decode_step / prefill_step launch it: row r reads token ids[r] (an id outside
 * [0, V) reads row 0) and position *pos + r % rps, or with pos_off (DEVICE [M / rps], ragged prompts; nullable)
 * clamp(*pos + r % rps - pos_off[r / rps], 0, n_pos - 1). tok_emb [V][d], pos_emb [n_pos][d] in dtype; ids [M], pos
 * DEVICE. Without pos_off the position is not clamped: the caller keeps *pos + rps <= n_pos.
 * -> x f32 [M][d]; optional: x16 [M][d] = T(x); x16fm = the same fragment-major for the lean LayerNorm-fused
 * projections ([ceil(M / 16)][d / 32][64 lanes][8]: element (r, c) at lane 16·((c % 32) / 8) + r % 16, slot c % 8;
 * 16-bit, d = 64, 512 .. 5120 of the lean table, else WCB_ERR_UNSUPPORTED; rows >= M are not written); stats
 * [M][d / st_w][2] = per-st_w-column (Σx, Σx²), st_w 16 or 32. */
int wcb_op_embed(int dtype, const void* tok_emb, const void* pos_emb, const int32_t* ids, const int32_t* pos,
                 const int32_t* pos_off, int M, int d, int V, int n_pos, int rps, float* x, void* x16, void* x16fm,
                 float* stats, int st_w, void* stream);

/* One decode-step projection launch, configured as the decoder's layer loop configures it (runtime.cpp
 * decode_rows), on caller operands. The caller passes plain tensors; the derived operands — W' = W·diag(γ), u, c
 * (the folded LayerNorm), the fragment-major weight copies, the W_k,hᵀ repack, x16 = T(x) — are built by the
 * preparation code wcb_finalize_weights runs. Fragment-major activations and row statistics come from the caller
 * (wcb_op_embed or a WCB_PROJ_RESID launch write them). 16-bit dtypes, except path WCB_PATH_DEC (f32 too).
 * kind:
 *   QKV      LN-fused, columns < n_split -> out [M][n_split], the others -> kv [2][kv_B][H][kv_T][64] (H =
 *            (N - n_split) / 128) of cache row r / kv_rps at position *pos + r % kv_rps (the caller keeps *pos +
 *            kv_rps <= kv_T)
 *   LN_PLAIN out [M][N] = LN(x)·Wᵀ + b;  LN_GELU  the same through erf-GELU (out_fm: written fragment-major for a
 *            consumer with K = N, path LEAN_FOLD_FM)
 *   RESID    x f32 [M][N] += A·Wᵀ + b in place, out16 [M][N] = T(x) (required), optional out16_fm, st_out
 *            ([M][N / 16][2], path DEC) / rst_out ([M][N / 32][2], paths RING_FOLD, WIDE); A = a16 [M][K], or a_fm
 *   KQ       N = K = d: out [M][H·d], q'_h = W_k,hᵀ q_h of the q rows a16 [M][d], Wk = cross k_proj.weight [d][d]
 *   XQK      N = K = d: the LN-fused q projection (W, bias) and KQ in one launch: out [M][H·d] only
 * path (M <= 64): DEC the general decode GEMM, LEAN the lean kernel, LEAN_FOLD with the LayerNorm folded into the
 *   weights, LEAN_FOLD_FM with fragment-major activations as well (a_fm in; out_fm / out16_fm out); RESID and KQ
 *   have no LayerNorm: on the two folded paths they are the lean launch;
 *   (M > 64): LN_RING a LayerNorm launch then the LDS-ring tile, RING_FOLD the ring tile with the folded LayerNorm
 *   (rst_in required; rst_out on RESID), WIDE the wide single-burst tiles (12; LN_GELU 22) with the same.
 * A (kind, path, shape) the path's launcher does not cover is WCB_ERR_UNSUPPORTED: nothing falls back. *taken
 * (HOST, nullable) receives the launcher that ran (1 lean, 2 fused cross query, 3 decode GEMM, 4 skinny, 5 + 256·t
 * ring tile (t = 1: 64x64, 2: 64x32, 3: 32x32), 6 wide tile, 7 two-stage tile). u_out / c_out (f32 [N]) and wg_out
 * ([N][K], dtype) receive the folded operands when non-NULL. Blocks until done (it owns the derived operands). */
enum wcb_proj_kind { WCB_PROJ_QKV = 0, WCB_PROJ_LN_PLAIN = 1, WCB_PROJ_LN_GELU = 2, WCB_PROJ_RESID = 3, WCB_PROJ_KQ = 4,
                     WCB_PROJ_XQK = 5 };
enum wcb_proj_path { WCB_PATH_DEC = 0, WCB_PATH_LEAN = 1, WCB_PATH_LEAN_FOLD = 2, WCB_PATH_LEAN_FOLD_FM = 3,
                     WCB_PATH_LN_RING = 4, WCB_PATH_RING_FOLD = 5, WCB_PATH_WIDE = 6 };
typedef struct {
  int kind, path, dtype;
  int M, N, K;
  const float* ln_w; const float* ln_b;   /* γ, β [K] (LN kinds, XQK) */
  const void* W; const float* bias;       /* W [N][K] (HF layout) in dtype, bias f32 [N] */
  const void* Wk;                         /* KQ, XQK: encoder_attn.k_proj.weight [d][d] in dtype */
  float* x;                               /* LN kinds, XQK: f32 rows [M][K]; RESID: [M][N], updated in place */
  const void* a16;                        /* LN kinds, XQK: T(x) [M][K] (NULL: derived); RESID, KQ: the A rows */
  const void* a_fm;                       /* LEAN_FOLD_FM: A fragment-major; whole row blocks are read: allocate
                                             M rounded up to 32 rows (N >= 2048 LN-fused launches take 32-row workgroups) */
  void* out; int out_fm;
  void* out16; void* out16_fm;            /* RESID */
  const float* st_in; float* st_out;      /* per-16-column (Σx, Σx²): the older skinny consumers */
  const float* rst_in; float* rst_out;    /* per-32-column (Σx, Σx²): the folded ring / wide tiles */
  void* kv; const int32_t* pos; int kv_B, kv_T, kv_rps, n_split;   /* QKV */
  int ring_kt;                            /* M > 64: 1 or 2 (0: 1) */
  int xqk_nch;                            /* XQK: 2, 4, 8, 16 (0: 8) */
  float* u_out; float* c_out; void* wg_out;
  int32_t* taken;
} wcb_dec_proj;
int wcb_op_dec_proj(const wcb_dec_proj* p, void* stream);

/* the greedy LM head with its softmax partials, then the partial merge (no LayerNorm, no boost, no EOS mask):
 * A [M][K], W [V][K] in dtype (M <= 64) → logits f32 [M][ld] (ld >= V), lse[M] = logsumexp of each logits row,
 * argmax[M] (lowest index on ties). Runs the kernels the decode step runs for that dtype / K / M: the column
 * walk with `walkers` workgroups per row block (0: the kernel default; 16-bit at K = 64, 512, 768, 1024, 1280
 * on a fragment-major copy of W, as the runtime's) for K = 64 .. 1280, the older skinny kernel's 64-column
 * epilogue for K = 32 and 2560; another K is WCB_ERR_UNSUPPORTED. Blocks until done (it owns scratch buffers). */
int wcb_op_lm_head_lse(int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float* logits, long ld,
                       float* lse, int32_t* argmax, void* stream);
/* y[M][d] (dtype) = LayerNorm(x f32 [M][d]) * w + b, eps 1e-5 */
int wcb_op_layernorm(int dtype, const float* x, const float* w, const float* b, void* y, int M, int d,
                     void* stream);
/* o[B][Sq][H*64] = softmax(q kᵀ) v per head (q pre-scaled), k/v [B][Sk][H*64];
 * flash=1 selects the MFMA kernel (16-bit dtypes; Sq <= 16: the few-query form of beam search), 100 the
 * MFMA kernel with 64 queries per wave, 200 / 201 / 202 (Sq <= 16) the beam kernel (the keys of a (set,
 * head) split over its waves, merged in the workgroup: 4 waves x 2 LDS stages, 2 x 4, 2 x 5), -n (Sq <= 16)
 * the MFMA kernel over n key ranges merged in
 * fixed order; 0 the decode kernel; n >= 2 the decode kernel with n split-KV key chunks combined by the
 * last-arriving chunk. */
int wcb_op_attention(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H, int Sq,
                     int Sk, int flash, void* stream);
/* decode attention in the runtime's layout: q/o [B][H*64], K/V head-major [B][H][Sk][64]; one query
 * per (row, head), nsplit key chunks (split-KV), kernel variant (k_attn.hip launch_decode; 6 = the
 * one-token self-attention kernel, nsplit 1; 7 = the same with the key count read on the device, as the
 * decode step runs it: the lean form for 16-bit). */
int wcb_op_attention_decode(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H,
                            int Sk, int nsplit, int variant, void* stream);
/* the same with a per-row key window (ragged prompts, below): q/o [B][Sq][H*64], the Sq causal queries of a row at
 * slots Sk-Sq .. Sk-1 (query i sees keys up to its own slot), K/V head-major [B][H][Sk][64]; key_start DEVICE [B]:
 * the query at slot s of row b attends keys [min(key_start[b], s), s]; keys below the window are never read into
 * the result (they may be non-finite). variant: 0..5 the prefill kernels of k_attn.hip launch_decode (any Sq),
 * + 100*n = with n split-KV key chunks (the argument list has no nsplit of its own: the runtime's self-attention
 * never splits, the chunking is reachable for the kernel tests only); 6 / 7 the one-token kernels of
 * wcb_op_attention_decode (Sq = 1). key_start = NULL launches the dense kernels on the same arguments (every query
 * sees keys 0 .. its slot); with every start 0 the windowed result equals theirs bit for bit. */
int wcb_op_attention_decode_window(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H,
                                   int Sq, int Sk, const int32_t* key_start, int variant, void* stream);

/* decoder cross-attention in encoder space (k_xenc.hip), the xmode-1 decode path:
 * o[B][d] = Σ_h-blocks W_v,h softmax_j(q'_h · enc_j) enc_j + b_v with q'_h = W_k,hᵀ q_h;
 * q [B][H*64] (pre-scaled by 1/8), enc [B][S][d], wkt = W_k repacked [H][d][64] (element (h,c,i) =
 * W_k[h*64+i][c]), wv [d][d] (HF layout), bv f32 [d]; nsplit key ranges per row (1..16). 16-bit dtypes.
 * variant: attn_xenc kernel variant; + 100 = merge kernel + grouped W_v GEMM instead of the fused merge. */
int wcb_op_cross_attention_enc(int dtype, const void* q, const void* enc, const void* wkt, const void* wv,
                               const float* bv, void* o, int B, int H, int S, int nsplit, int variant, void* stream);

/* Bias-weighted cross entropy — replaces the loss block of
 * WhisperForConditionalGenerationWeightCE.forward (models/whisper_medical.py:113-156): weight
 * bias_weight on every label token covered by a contiguous match of one of its utterance's spans
 * (:118-133), −log_softmax(logits)[label]·w over labels ≠ −100, summed / (valid count + 1e-8)
 * (:136-151). spans == NULL: nn.CrossEntropyLoss(ignore_index=−100) mean (:152-155).
 * logits f32 [B·T][ld] (device), labels [B][T], spans [B][N][Lmax] with span_len [B][N] (0 = empty
 * span, skipped — :122-127); per_token [B·T] (device, caller-owned) receives −logp·w·valid;
 * loss (device f32 scalar) and count (device, nullable) the mean and the valid-label count.
 * Labels must be −100 or in [0, V). Async on `stream`; deterministic (fixed-order reduction). */
int wcb_op_weighted_ce(const float* logits, long ld, int B, int T, int V, const int32_t* labels,
                       const int32_t* spans, const int32_t* span_len, int N, int Lmax, float bias_weight,
                       float* per_token, float* loss, int32_t* count, void* stream);

/* Host-side scoring (csrc/metric.cpp, no GPU): the arithmetic of utils/compute_metric.py on
 * already-normalised text. wcb_wer_counts: per utterance i, errors[i] = word-level Levenshtein
 * distance between refs[i] and hyps[i] (whitespace-separated words) and ref_words[i] = |words(refs[i])|
 * — corpus WER = Σerrors / Σref_words, as evaluate's "wer" (jiwer) computes it at
 * compute_metric.py:159. n_threads <= 0: all hardware threads. wcb_bias_counts: compute_bias_wer's
 * per-utterance tallies (compute_metric.py:200-230): non-overlapping phrase counts in ref / pred. */
int wcb_wer_counts(const char* const* refs, const char* const* hyps, int n, int64_t* errors, int64_t* ref_words,
                   int n_threads);
int wcb_bias_counts(const char* ref, const char* pred, const char* const* phrases, int n_phrases,
                    int64_t* distance, int64_t* tokens);

#ifdef __cplusplus
}
#endif
#endif /* WCB_H_ */
