// libwcb host runtime: C-ABI entry points (include/wcb.h), weight repacking, workspaces, the
// encoder pipeline, the hipGraph-replayed greedy decode loop, the bias-list automaton builder and
// per-kernel time accounting.
//
// Maps onto the reference as follows:
//   wcb_log_mel   ↔ WhisperFeatureExtractor.__call__   (data_utils/data_loader.py:171-172)
//   wcb_encode    ↔ WhisperEncoder.forward             ([tf] modeling_whisper.py:592-646)
//   wcb_generate  ↔ model.generate(input_features, max_length) (scripts/evaluation.py:173-206,
//                   [tf] trainer_seq2seq.py:329, [tf] generation/utils.py:2783-2944 greedy loop)
//   wcb_forward   ↔ WhisperForConditionalGenerationWeightCE.forward (models/whisper_medical.py:45-111)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cxxabi.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include <cstdlib>
#include <deque>
#include <atomic>

#include "../../include/wcb.h"
#include "kernels.h"
#include "sample.h"
#include "dtw.h"

using namespace wcb;

namespace {

struct WcbError : std::runtime_error {
  int code;
  WcbError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess)                                                                      \
      throw WcbError(WCB_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));             \
  } while (0)
#define REQUIRE(c, msg)                                       \
  do {                                                        \
    if (!(c)) throw WcbError(WCB_ERR_ARG, std::string(msg)); \
  } while (0)

constexpr int kFrames = 3000, kNCol = 416, kNSamp = 480000;
constexpr int kXSplit = 8;   // max cross-attention key chunks per (row, head) (partials buffer size)

int esize(int dt) { return dt == WCB_F32 ? 4 : 2; }

// host f32 → device element bits
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t b) {
    if (b <= bytes) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    HIPCHK(hipMalloc(&p, b));
    // zeroed and complete before any (non-blocking) library stream can touch it
    HIPCHK(hipMemsetAsync(p, 0, b, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    bytes = b;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename X> X* as() const { return reinterpret_cast<X*>(p); }
};

struct LayerW {
  void* qkv_w = nullptr; float* qkv_b = nullptr;   // [3d][d] (q rows pre-scaled by 1/8), bias (k = 0)
  void* o_w = nullptr; float* o_b = nullptr;
  float *ln1_w = nullptr, *ln1_b = nullptr;
  void* xq_w = nullptr; float* xq_b = nullptr;     // decoder cross-attention q (pre-scaled)
  void* xo_w = nullptr; float* xo_b = nullptr;
  float *lnx_w = nullptr, *lnx_b = nullptr;
  void* fc1_w = nullptr; float* fc1_b = nullptr;
  void* fc2_w = nullptr; float* fc2_b = nullptr;
  float *ln2_w = nullptr, *ln2_b = nullptr;
  // decoder, 16-bit: the pre-block LayerNorms folded into their consumers for rows > 64 (ring LNF,
  // gemm_impl.h): W' = W·diag(γ) (T), u = Σ_k W'[n][k], c = Σ_k β_k W[n][k] + bias, for QKV (ln1),
  // cross-q (lnx), fc1 (ln2)
  void *qkv_wg = nullptr, *xq_wg = nullptr, *fc1_wg = nullptr;
  float *ln1_u = nullptr, *ln1_c = nullptr, *lnx_u = nullptr, *lnx_c = nullptr, *ln2_u = nullptr, *ln2_c = nullptr;
  // encoder-space cross-attention (k_xenc.hip): W_k,hᵀ repacked [H][d][64], W_v [d][d], b_v
  void* xkt_w = nullptr; void* xv_w = nullptr; float* xv_b = nullptr;
  // decoder, 16-bit: fragment-major copies for the lean decode projections (kernels.h frag_major)
  void *qkv_fm = nullptr, *o_fm = nullptr, *xq_fm = nullptr, *xkt_fm = nullptr, *xo_fm = nullptr, *fc1_fm = nullptr,
       *fc2_fm = nullptr;
  void* xv_fm = nullptr;   // W_v for the greedy range merge (xenc_merge_v_kernel's A-fragment order)
  void *qkv_wgfm = nullptr, *xq_wgfm = nullptr, *fc1_wgfm = nullptr;   // folded weights fragment-major (beam_wide / beam_wfm)
};

struct ProfEntry {
  std::string name;
  int64_t launches = 0;
  double ms = 0, flops = 0, bytes = 0;
  const void* fn = nullptr;   // kernel of the class's first launch and its grid in threads
  long grid = 0;
};

}  // namespace

struct wcb_bias {
  int n_states = 1;
  int vocab = 0;
  uint64_t id = 0;                  // decode-graph cache key (never reused, unlike the address)
  wcb_handle* owner = nullptr;      // the handle whose decode graphs may hold these device buffers
  DevBuf root_bits, root_child, trans_off, trans_tok, trans_dst;
  DevBuf st_depth, st_keep;         // per state: trie depth, deepest completed phrase on its path
};

// Per-utterance bias lists (wcb.h wcb_bias_batch): B automata compiled on the host into one state space.
// Host data only; a decode call copies it into the decode context's device buffers (install_forest).
struct wcb_bias_batch {
  int B = 0, vocab = 0;
  std::vector<int> root;                           // [B] root state of clip b (= first state of its block)
  std::vector<int> n_states;                       // [B] states of clip b's automaton (root included)
  std::vector<int> rc_off, rc_tok, rc_dst;         // [B + 1], gated root children per clip, token-sorted
  std::vector<int> trans_off, trans_tok, trans_dst;   // global CSR over all states
  std::vector<int> st_depth, st_keep;              // per state
};

// device view of an installed forest (stable pointers into DecCtx::forest)
struct ForestDev {
  ForestArgs f;
  const int *trans_off = nullptr, *trans_tok = nullptr, *trans_dst = nullptr, *st_depth = nullptr, *st_keep = nullptr;
};

// One decode: its shape and what its selection needs. The step-wise API hands it out as its state (one active per
// handle, on decode context kMaxCtx-1); wcb_generate* keeps one on its stack for the length of the call.
struct wcb_state {
  wcb_handle* h = nullptr;
  int B = 0, P = 1, T = 0, steps = 0, max_new = 0, min_new = 0, xmode = 1;
  int fwd = 0;   // positions appended by wcb_forward_cached (a forward-cache state takes no decode steps)
  float lam = 0.f;
  uint64_t bias_id = 0;
  int nb = 1;    // beams per utterance (> 1: beam search, rows R = B·nb; the running beams in bm)
  BeamArgs bm;
  bool forest = false;   // per-utterance lists installed (wcb_decode_bias_batch): every step takes bias = NULL
  ForestDev fd;
  bool logprobs = false; // wcb_decode_enable_logprobs: every step also writes its column of the context's lpbuf
  bool sampling = false; // wcb_decode_enable_sampling: every step draws its tokens (the context's samp words)
  bool ragged = false;   // per-clip prompts of different lengths (left-padded to P): every step reads the context's poff
  bool no_speech = false; // wcb_decode_enable_no_speech: the first step also writes the context's nsp floats
  RepArgs rep;           // repeat rules of this decode (the handle's at its start; seen null: none)
};

// lean decode projection classes stamped inside the replayed decode graph (stamps pass), by region
static const char* const kLeanStampClass[] = {"dec_xattn", "dec_qkv", "dec_out", "dec_xq", "dec_xo", "dec_fc1", "dec_fc2",
                                              "dec_kq"};
static int lean_stamp_region(const char* cls) {
  for (int r = 1; r < 8; ++r)
    if (!strcmp(cls, kLeanStampClass[r])) return r;
  return 0;
}

// The captured decode step of one kind of call: one step, and steps_per_graph consecutive steps in one graph
// (null when that is 1), with the key naming everything the capture baked in
struct StepGraphs {
  hipGraphExec_t one = nullptr, k = nullptr;
  std::string key;
  void drop() {
    for (hipGraphExec_t* g : {&one, &k}) {
      if (*g) (void)hipGraphExecDestroy(*g);
      *g = nullptr;
    }
    key.clear();
  }
};

// Decode state of one in-flight generate call. Two contexts (one per cross-K/V buffer) let call
// i+1 decode on its own stream while call i is still decoding: two latency-bound step chains share
// the GPU instead of one.
struct DecCtx {
  static constexpr int kMaxSub = 8;             // row groups of <= 64 rows (beam search: B·nb rows)
  hipStream_t hs = nullptr;                     // decode stream of this context
  hipStream_t sub[kMaxSub] = {};                // row-group chains (fork/join inside the step graph)
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSub] = {};
  int dec_B = 0, dec_T = 0;
  DevBuf kvself, dx, dx16, dx16fm, dh, dq, dqp, du, datt, dffn, dstats, drst, xpart, xml, xticket, logits, part_val, part_idx, ints,
      pids, outbuf, forced, beam;
  DevBuf kq_cnt;   // 64-bit arrival counters of the fused xq+kq launches [L][kMaxSub][4 row blocks][H] (monotonic)
  int nchunk = 64;
  int* done_h = nullptr;                        // pinned: the "all rows finished" step of the last 2 chunks
  hipEvent_t ev_poll[2] = {};
  // token log-probs (wcb_generate_scored, wcb_decode_enable_logprobs): the LM head's softmax partials
  // [rows][nchunk] beside part_val, the log-prob rows [rows][out_ld] beside outbuf — allocated by the first
  // scored call
  DevBuf part_max, part_sum, lpbuf;
  // temperature sampling (wcb_generate_sampled, wcb_decode_enable_sampling): samp = one 64-bit word holding
  // the bits of inv_T = 1 / T in its low half, then the per-row seeds [64] — written on the decode stream at
  // the start of every sampled call, read by the sampled kernels through this stable address, so the
  // sampled graphs hold for every seed and temperature
  DevBuf samp;
  // the captured decode steps, one slot per kind of call: a ruled (wcb_set_token_rules), a sampled and a scored
  // (token log-probs) decode each launch other kernels or arguments, so every combination replays its own graphs
  // and no kind of call evicts another's
  StepGraphs graphs[32];
  StepGraphs& graphs_of(bool ruled, bool sampled, bool scored, bool no_speech = false, bool repeat = false) {
    return graphs[16 * repeat + 8 * no_speech + 4 * ruled + 2 * sampled + scored];
  }
  void drop_graphs() {
    for (StepGraphs& g : graphs) g.drop();
  }
  // per-utterance bias forest of the call decoding in this context: device buffer carved by the capacities
  // (states, transitions, root children; they only grow: quiesce + realloc, the graph key names them), the
  // pinned staging copy the asynchronous upload reads, and the event of the last upload from it
  DevBuf forest;
  int f_ns = 0, f_nt = 0, f_nrc = 0;
  int* f_stage = nullptr;
  size_t f_stage_words = 0;
  hipEvent_t ev_fcopy = nullptr;
  bool f_copy_pending = false;
  // ragged prompts (wcb_generate_prompted, wcb_decode_begin_prompted): poff = the slot offset
  // Pmax − P_b of every row [kPromptRows], allocated once and never moved (the ragged graphs hold its address, the
  // graph key only the fact); the left-padded prompts and the offsets go up on the decode stream from the pinned
  // p_stage, as the forest does
  DevBuf poff;
  // repeat rules (wcb_set_repeat_rules): seen = the per-row token bitmap [kRepRows][vocab_pad / 32],
  // rep_par = two words (the bits of the f32 penalty, the n-gram size). Both allocated once by the first such decode
  // and never moved: the graphs hold the addresses, the graph key only the fact — the values are written by value on
  // the decode stream at the start of every such decode, as samp is
  DevBuf seen, rep_par;
  // no-speech probability (wcb_generate_windows, wcb_decode_enable_no_speech): one float per row [64], written by
  // the scored finalize at step 0; allocated once and never moved (the graphs of such decodes hold its address)
  DevBuf nsp;
  // language detection (wcb_detect_language, the language slot of wcb_generate_lang / wcb_decode_begin_lang): the
  // candidate bitmap [kLangWords], written by value on the decode stream at the start of every such call
  DevBuf lang;
  int* p_stage = nullptr;
  size_t p_stage_words = 0;
  hipEvent_t ev_pcopy = nullptr;
  bool p_copy_pending = false;
};

struct wcb_handle {
  wcb_model_desc d{};
  DType dt = kBF16;
  int device = 0;
  std::string err;
  hipStream_t he = nullptr;   // front end + encoder + cross-K/V stream (overlaps the previous batch's decode)
  // Decode contexts in flight: call i decodes in context i % nctx from cross-K/V buffer i % nctx while
  // the encoder stream already works on the next call. Measured: 2 contexts, one chain each.
  static constexpr int kMaxCtx = 4;
  int nctx = 2;
  hipEvent_t ev_xkv[kMaxCtx] = {}, ev_dec[kMaxCtx] = {};   // cross-K/V buffer k written / decode reading it done
  int gen_count = 0;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  static constexpr int kMaxSub = DecCtx::kMaxSub;
  DecCtx dc[kMaxCtx];
  int n_sub = 1;   // row groups per decode step on concurrent streams (fork/join inside the graph);
                   // with two decode contexts in flight one chain each measured best
  // Cross-attention: one workgroup per (row, head) over all 1500 keys. Measured (tools/xattn_bench.py,
  // head-major K/V cycling 12 layers): split-KV hand-offs cost more than they hide at 16-32 rows.
  int xsplit = 1;
  // cross-attention kernel variant over precomputed K/V (k_attn.hip launch_decode), fixed at create
  // from the model — never from the batch, whose composition must not change a clip's tokens (the
  // two kernels sum in different orders): the single-pass kernel (1) for 20 heads (large-v3, C5:
  // 1076 -> 1110 audio-s/s), the two-pass kernel (0) otherwise (medium, C3: 2435 vs 2048 with 1)
  int xvariant = 0;
  // beam-search cross-attention on the flash kernel (16-bit, the rows of a clip grouped): key ranges
  // per (clip, head), merged by flash_merge_kernel. Fixed per handle (never from the batch). Measured
  // (audio-s/s, splits 1 / 2 / 4): C3 4491 / 4531 / 4452, C5 1405 / 1484 / 1485.
  int flash_split = 2;
  // the same with the clip's keys split over the 4 waves of one (clip, head) workgroup, merged in the
  // workgroup (option "beam_xattn" 1..3; 0, default = the flash kernel above, whose 4 waves split
  // 16-query blocks — with 5 beams three of them compute on padding, yet it measured as fast: the
  // launch streams 393 MB of K/V per layer at C3, ~5.3 TB/s, bandwidth- not compute-bound)
  int beam_xattn = 0;   // measured: C3 4.37 / 4.41 ms/token (1 / 0), C5 3.60 / 3.49: within noise / worse
  // decode rows > 64 (16-bit): pre-block LayerNorms folded into the ring-tile projections (option
  // "ln_fold" 1: γ folded into the weights, (μ, r) from the residual writers' per-32-column partial
  // sums, applied in the epilogue — no per-element work in the K loop, no LayerNorm launch) or a
  // LayerNorm launch before each projection (0). (Round 2's in-loop form — A scaled by γ and the row
  // sums accumulated inside the K loop — measured slower than the launch and is gone.)
  int ln_fold = 1;
  // greedy cross-attention (encoder space): range merge and W_v in one launch (option "merge_v";
  // C2 16,570 vs 16,259 audio-s/s for the two launches)
  int merge_v = 1;
  // greedy cross-attention: range partials in the model dtype, normalised per range (option "xpart16";
  // half the partial bytes the attention writes and the merge reads; (max, Σp) stay f32). Measured: C2
  // 19,607 / 19,555 vs 19,276 / 19,395 audio-s/s (interleaved, one box); the GPU suite (goldens, bf16
  // margin gates) green with it
  int xpart16 = 1;
  // greedy cross-attention query (<= 64 rows, encoder space, lean path): q'_h = W_k,hᵀ q_h inside the
  // LN-fused q_proj launch (option "xq_kq" 1; gemm_impl.h dec_lean_kernel FZ 2) or as a launch of its
  // own (0, default; bit-identical). Serialised, the fused launch is the faster (6.9 vs 4.4 + 3.0 µs);
  // inside the pipelined graph its in-launch hand-off stretches to 9.3 µs with the other chain and the
  // encoder beside it, and the C2 bench measured 19,084 (two launches) vs 18,999 (fused), mean of five
  // interleaved pairs
  int xq_kq = 0;
  // decode rows > 64: 64-deep K sub-tiles per ring stage of the 64x32 / 32x32 tiles (option "ring_kt",
  // 1 or 2; C5 1,594 -> 1,644 audio-s/s)
  int ring_kt = 2;
  // decode rows 65-96 (C5's 80 beam rows), K = d_model: out / xo / xq / fc1 on the wide single-burst tiles
  // (gemm_impl.h gemm_wide_kernel) instead of the ring tiles (option "beam_wide", set before finalize).
  // tools/beam_gemm_bench.py (80 rows, d = 1280, cold weights): out 6.3 -> 5.3 µs (16 x 32 tiles,
  // fragment-major W), fc1 13.5 -> 9.8 µs (32 x 32); QKV stays on the ring (7.5 vs 9.4); at C3's 320 rows
  // the ring tiles win every shape. C5 bench 2,478 / 2,485 vs 2,446 / 2,429 audio-s/s (interleaved)
  int beam_wide = 1;
  // decode rows > 64, ring tiles: the weights read from fragment-major copies (option "beam_wfm", set
  // before finalize: the folded QKV / xq / fc1 weights get such copies too) and the tile order (option
  // "beam_raster": bands of n row panels with the column tiles outer, so the row tiles sharing a weight
  // tile run on one XCD; 0 = row panels outer)
  int beam_wfm = 0;
  // <= 64 rows (greedy), the LN-fused lean projections (QKV, xq, fc1): the LayerNorm folded into the weights
  // (W·diag(γ) fragment-major, c, u: the beam tiles' algebra) instead of normalising the A rows in the kernel
  // (option "lean_fold", set before finalize). C2 bench 19,777 / 20,001 / 19,974 vs 19,527 / 19,553 / 19,692
  // audio-s/s (interleaved): the MFMAs start as soon as the rows land, the statistics ride the partial-tile
  // barrier — the in-kernel LayerNorm cost its launches ~1.1 µs each (xq 3.89 vs out 2.78 µs in-graph)
  int lean_fold = 1;
  // greedy cross query: the q projection and q'_h = W_k,hᵀ q_h in one launch, each workgroup recomputing its
  // head's q_h (gemm_impl.h dec_xqk_kernel; option "xqk"; needs lean_fold) instead of xq → kq: one launch
  // boundary less per layer, no hand-off. C2 20,423 / 20,431 / 20,382 vs 20,243 / 20,295 / 20,097 (interleaved)
  int xqk = 1;
  // q' column chunks per head of the fused cross query (option "xqk_chunks": 2, 4, 8, 16; C2: 4 within noise of
  // 8, 2 and 16 slower)
  int xqk_nch = 8;
  // greedy range merge + W_v (16-bit partials): a head's 64 outputs over 1 or 2 workgroups (option "merge_os";
  // 2 measured slower: C2 20,114 / 20,074 / 20,080 vs 20,325 / 20,343 / 20,300, interleaved)
  int merge_os = 1;
  // greedy LM head: column walkers per row block (option "lm_walkers", before finalize; = the argmax
  // partials per row select_finalize reduces). C2 (interleaved pairs): 256 walkers 20,464-20,644 vs 512
  // 20,353-20,395 audio-s/s; 128 and 1024 no better than 512, 384 equal to 256 — fewer walkers re-read and
  // re-normalise the rows fewer times, and the walk of ~13 tiles each still hides its weight stream
  int lm_walkers = 256;
  // log-mel DFT: the f32 products as six bf16 MFMA products of 3-part splits (hi, mid, lo; the dropped terms
  // below 2^-24 relative) instead of f32 MFMAs (option "mel_split")
  int mel_split = 0;
  // lean projections on 32-row workgroups wherever the chain has > 16 rows (option "lean_mf2"; default:
  // only the LN-fused N >= 2048 ones). Measured 2.7 % slower at C2 (19,803-19,948 vs 20,424-20,521)
  int lean_mf2 = 0;
  // beam top-K: each row's vocabulary in kBeamChunks chunks, one workgroup per (chunk, row) (option
  // "beam_chunks" 1) or one workgroup per row (0, default; k_beam.hip beam_select). Measured: C3 6,160 vs
  // 6,228, C5 2,517 vs 2,518 audio-s/s — the per-row kernel's 320 (80) long workgroups already run beside
  // the other decode context's launches, so spreading the scan over the chip only adds contention
  int beam_chunks = 0;
  int beam_raster = 0;
  // greedy LM head: the final LayerNorm in a launch of its own (option "lm_ln_split" 1) or inside the
  // column walk (0, default: with the f32 copies of the A rows no longer held across the statistics
  // barrier the fused walker is 22.46 vs 22.19 µs + the LayerNorm launch, tools/dec_kernel_bench.hip)
  int lm_ln_split = 0;
  // encoder flash attention tiling (option "enc_flash"): 2 = 32 queries per wave, 4 = 64 queries per
  // wave. Measured (tools/microbench.py, small / medium encoder shapes, µs): 2: 358 / 878, 4: 313 / 808
  // (3 / 4 LDS stages at 32 queries measured 328 / 887 and 399 / 1041: removed)
  int enc_flash_qw = 4;
  // Cross-attention formulation: 1 = encoder space (k_xenc.hip: the step streams the encoder output,
  // no cross-K/V precompute; 16-bit dtypes, d <= 1024), 0 = precomputed per-layer K/V (f32 "exact"
  // mode, large-v3). Fixed at create (WCB_XMODE overrides where supported).
  int xmode = 1;
  // beam search (num_beams > 1) reads precomputed per-clip cross-K/V (xmode 0) even when greedy uses
  // the encoder-space kernel: its per-row work is smaller and the beams of a clip share the K/V
  // (measured on C3, medium beam 5: 1805 vs 1414 audio-s/s). WCB_BEAM_XMODE=1 keeps encoder space.
  int beam_xmode = 0;
  // decoder rows per decode chain (WCB_GROUP_ROWS). One chain for every row count by default: the
  // beam configurations decode faster as one chain of 80-320-row launches than as 64-row chains on
  // parallel streams (measured: C3 1814 -> 2215, C5 864 -> 983 audio-s/s; profiles/r01c_sweep_grp_*)
  int group_rows = 512;
  // key ranges per row of the encoder-space kernel (rows x ranges workgroups). With 16-bit partials
  // (xpart16) measured C2 6: 19,496 / 19,581, 8: 19,356 / 19,301, 10: 18,246, 12: 18,743, 16: 18,120
  int xenc_split = 6;
  // the decode's copy of the encoder output in the fragment-major chunk layout (k_xenc.hip
  // xenc_fm_kernel): 1 KiB contiguous per load wave-instruction of the register-ring kernel, where the
  // row layout touches 16 rows x 64 B (option "xenc_fm"; variants 1 and 2; bit-identical)
  int xenc_fm = 1;
  int xenc_variant = 1; // attn_xenc kernel variant (k_xenc.hip)
  // decoder LayerNorm input of the fused LN projections: 1 = the T-typed copy of the residual stream
  // the producers write beside the f32 rows (half the bytes per projection workgroup; C2 decode 1.066
  // vs 1.110 ms/token), 0 = the f32 rows (f32 mode). WCB_LN16 overrides.
  int ln16 = 1;
  int vocab_pad = 0;    // LM-head rows padded to a multiple of 128 (zero rows): the MFMA tile path's N
  int steps_per_graph = 8;   // decode steps captured per replayed graph (option "steps_per_graph")
  // decode projections of <= 64 rows on dec_lean_kernel (gemm_impl.h; bit-identical to
  // gemm_dec_kernel, one kernel-argument round trip and one load burst per launch; option "lean")
  int lean = 1;
  // lean path: the residual writers (embedding, out / xo / fc2 projections) also write the 16-bit rows
  // fragment-major for the LayerNorm-fused consumers (QKV, xq, fc1); option "lean_x"
  int lean_x = 1;
  int64_t n_graph_captures = 0;   // decode graphs instantiated so far (wcb_debug_counter "graph_captures")
  struct wcb_state* step_state = nullptr;   // the active step-wise decode (wcb_decode_begin), if any
  // token rules (wcb_set_token_rules): the deny bitmaps [vocab_pad / 32] of every step and of step 0, allocated by
  // the first call and never moved (the ruled graphs hold their addresses); deny0 is read only when has0
  bool rules_on = false, rules_has0 = false;
  TsRule rules_ts;
  DevBuf rules_deny, rules_deny0;
  // repeat rules (wcb_set_repeat_rules): the two values; the device state lives in the decode contexts
  bool rep_on = false;
  float rep_p = 1.f;
  int rep_n = 0;
  // encoder GEMM tile order (option "enc_raster"): bands of n row panels with the column tiles outer
  // (GemmArgs::raster; 0 = row-major). 8 measured best with the round-3 ring kernel (whisper-small:
  // QKV 185 -> 177, fc1 297 -> 281, out 118 -> 116 us, fc2 within noise; profiles/r03f_enc_gemm_bench.txt)
  int enc_raster = 8;
  // encoder GEMMs (option "enc_gemm"): the ping-pong kernel (gemm_impl.h gemm_pp_kernel), 256-wide tiles
  // and 192-wide where those leave fewer tile rounds (4, default: C2 out 90.4 -> 89.2, fc2 273.4 -> 261.2 µs
  // against the LDS-ring kernel's 256x192 tiles, tools/enc_bench.py gemm; the bench line within noise),
  // the LDS-ring kernel for those (1), or the LDS-ring kernel everywhere (0)
  int enc_gemm = 4;
  // decode projections on gemm_dec_kernel (K supported): the LayerNorm consumers compute their row
  // statistics from the rows they load, so the producers publish no per-16-column partial sums
  bool dec_gemm = false;
  std::map<std::string, DevBuf> staged;   // every parameter as a dense f32 device tensor until finalize
  std::vector<DevBuf> owned;
  bool ready = false;
  int dbg_enc_layers = -1;   // debug: run only this many encoder layers (-1 = all)
  // weights
  void *conv1_w = nullptr, *conv2_w = nullptr;
  float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr;
  int k1pad = 0;
  std::vector<LayerW> enc, dec;
  float *enc_ln_w = nullptr, *enc_ln_b = nullptr, *dec_ln_w = nullptr, *dec_ln_b = nullptr;
  void* xkv_w = nullptr; float* xkv_b = nullptr;
  void *tok_emb = nullptr, *dec_pos = nullptr;
  void* tok_emb_fm = nullptr;   // 16-bit: fragment-major copy of tok_emb for the greedy LM head
  // mel tables
  DevBuf dft, dft3, mel_lo, mel_hi, mel_w, clip_max;
  DevBuf win_ints;   // long-form: clip index, seek and frame count of every window row [3][kWinRows], or n_valid [B] (stream he)
  // encoder workspace
  int enc_B = 0;
  DevBuf xt, hbuf, x, h, qkv, att, ffn, encout;
  // per decode context: cross-K/V (xmode 0) or the encoder output (xmode 1); buffer k is read by
  // decode context k while the encoder stream fills the next one
  DevBuf xkv2[kMaxCtx];
  // token timestamps (wcb_align): the post-pass's workspaces — w [clips of a group][heads][rows][S], the cost
  // matrices, the teacher-forced ids, the per-clip rows and frames, the prefix, the DTW trace when it does not
  // fit in LDS — and the decode context the latest wcb_generate* call left its encoder state in
  DevBuf al_w, al_M, al_tf, al_lens, al_frames, al_prefix, al_trace;
  int last_gen_buf = -1, last_gen_B = 0, last_gen_xm = 0, last_gen_id = -1;
  // the workspaces are the handle's while a post-pass runs on its decode context's stream: every post-pass first
  // waits for the one before it (ev_align), whichever context that ran in
  hipEvent_t ev_align = nullptr;
  bool align_pending = false;
  size_t align_ws_bytes = (size_t)1 << 30;   // bound of al_w (option "align_ws", MiB): above it the clips go in groups
  // default (empty) bias automaton
  std::unique_ptr<wcb_bias> empty_bias;
  std::vector<wcb_bias*> biases;     // live automatons created on this handle (lifetime, wcb.h)
  // device error word: set by a kernel whose in-launch hand-off wait ran out its spin bound (common.h
  // group_arrive_wait); read and cleared by wcb_synchronize (and the blocking calls that wait anyway)
  DevBuf dev_err;
  // profiling
  bool prof = false, prof_stamps = false;
  std::vector<ProfEntry> prof_e;
  std::deque<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_pending;
  std::vector<hipEvent_t> ev_pool;
  DevBuf stamps, stamp_acc;                   // decode device stamps (graph nodes): cross-attention + the lean projections
  // stamp regions per decode context: 0 the cross-attention, 1.. the lean projection classes
  static constexpr int kStampRegions = 8;
  unsigned long long* stamp_base(int buf, int region) {
    return stamps.as<unsigned long long>() + ((size_t)buf * kStampRegions + region) * stamp_slots() * 2 * kStampSub;
  }
  double xattn_bytes = 0, xattn_flops = 0;    // algorithmic work of the stamped launches
  long stamp_slots() const { return (long)d.n_text_ctx * d.n_layers * kMaxSub; }   // per context

  int H() const { return d.n_heads; }
  int S() const { return d.n_audio_ctx; }

  void* upload(const void* src, size_t bytes) {
    owned.emplace_back();
    owned.back().ensure(bytes);
    HIPCHK(hipMemcpy(owned.back().p, src, bytes, hipMemcpyHostToDevice));
    return owned.back().p;
  }
  float* upload_f(const std::vector<float>& v) { return reinterpret_cast<float*>(upload(v.data(), v.size() * 4)); }
  void* own(size_t bytes) {
    owned.emplace_back();
    owned.back().ensure(bytes);
    return owned.back().p;
  }
  // staged parameter `name` (f32 device), element count checked
  const float* W(const std::string& name, size_t expect) {
    auto it = staged.find(name);
    if (it == staged.end()) throw WcbError(WCB_ERR_STATE, "missing weight " + name);
    if (it->second.bytes != expect * 4)
      throw WcbError(WCB_ERR_ARG, "weight " + name + " has " + std::to_string(it->second.bytes / 4) +
                                      " elements, expected " + std::to_string(expect));
    return it->second.as<float>();
  }

  // ---------------------------------------------------------------- profiling helpers
  int prof_id(const char* name) {
    for (size_t i = 0; i < prof_e.size(); ++i)
      if (prof_e[i].name == name) return (int)i;
    prof_e.push_back(ProfEntry{name});
    return (int)prof_e.size() - 1;
  }
  hipEvent_t get_ev() {
    if (!ev_pool.empty()) { auto e = ev_pool.back(); ev_pool.pop_back(); return e; }
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    return e;
  }
  template <typename F>
  void timed(const char* name, double flops, double bytes, hipStream_t st, F&& f) {
    if (!prof) { f(); return; }
    const int id = prof_id(name);
    hipEvent_t a = get_ev(), b = get_ev();
    g_launch_timer = LaunchTimer{a, b, 0};   // kernel begin/end timestamps (kernels.h, WCB_LAUNCH)
    try {
      f();
    } catch (...) {
      g_launch_timer = LaunchTimer{};
      throw;
    }
    const int n = g_launch_timer.n;
    if (n && !prof_e[id].fn) {
      prof_e[id].fn = g_launch_timer.fn;
      prof_e[id].grid = g_launch_timer.grid;
    }
    g_launch_timer = LaunchTimer{};
    if (n == 0) {   // nothing launched (copies / memsets only): a zero-width interval
      HIPCHK(hipEventRecord(a, st));
      HIPCHK(hipEventRecord(b, st));
    }
    prof_e[id].launches += 1;
    prof_e[id].flops += flops;
    prof_e[id].bytes += bytes;
    prof_pending.push_back({id, {a, b}});
  }
  // an enclosing interval (e.g. the whole decode loop) from plain stream events: enqueue-to-completion,
  // used for totals only, never for a per-launch duration
  template <typename F>
  void timed_wall(const char* name, hipStream_t st, F&& f) {
    if (!prof) { f(); return; }
    const int id = prof_id(name);
    hipEvent_t a = get_ev(), b = get_ev();
    HIPCHK(hipEventRecord(a, st));
    f();
    HIPCHK(hipEventRecord(b, st));
    prof_e[id].launches += 1;
    prof_pending.push_back({id, {a, b}});
  }
  void prof_collect() {
    while (!prof_pending.empty()) {
      auto& p = prof_pending.front();
      HIPCHK(hipEventSynchronize(p.second.second));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, p.second.first, p.second.second));
      prof_e[p.first].ms += ms;
      ev_pool.push_back(p.second.first);
      ev_pool.push_back(p.second.second);
      prof_pending.pop_front();
    }
  }
};

namespace {

thread_local std::string g_err;
std::atomic<uint64_t> g_next_bias_id{1};

template <typename F>
int guarded(wcb_handle* h, F&& f) {
  try {
    f();
    return WCB_OK;
  } catch (const WcbError& e) {
    (h ? h->err : g_err) = e.what();
    return e.code;
  } catch (const std::exception& e) {
    (h ? h->err : g_err) = e.what();
    return WCB_ERR_ARG;
  }
}

// ---------------------------------------------------------------------------- mel tables
double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; }
double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; }

// Slaney filters [201][n_mel] as [tf] audio_utils.py:638-729 (norm="slaney", mel_scale="slaney")
std::vector<double> mel_filters(int n_mel) {
  const int nf = 201;
  std::vector<double> mf(n_mel + 2), ff(n_mel + 2), fft(nf), out((size_t)nf * n_mel, 0.0);
  const double mmin = hz_to_mel(0.0), mmax = hz_to_mel(8000.0);
  for (int i = 0; i < n_mel + 2; ++i) {
    // np.linspace: start + i*step, last point exactly stop
    mf[i] = (i == n_mel + 1) ? mmax : mmin + i * ((mmax - mmin) / (n_mel + 1));
    ff[i] = mel_to_hz(mf[i]);
  }
  for (int k = 0; k < nf; ++k) fft[k] = (k == nf - 1) ? 8000.0 : k * (8000.0 / (nf - 1));
  for (int k = 0; k < nf; ++k)
    for (int m = 0; m < n_mel; ++m) {
      const double down = -(ff[m] - fft[k]) / (ff[m + 1] - ff[m]);
      const double up = (ff[m + 2] - fft[k]) / (ff[m + 2] - ff[m + 1]);
      const double v = std::max(0.0, std::min(down, up));
      out[(size_t)k * n_mel + m] = v * (2.0 / (ff[m + 2] - ff[m]));
    }
  return out;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

const char* wcb_last_error(const wcb_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int wcb_create(const wcb_model_desc* desc, int device, wcb_handle** out) {
  return guarded(nullptr, [&] {
    REQUIRE(desc && out, "null argument");
    REQUIRE(desc->d_model % 64 == 0 && desc->d_model / desc->n_heads == 64, "head_dim must be 64");
    REQUIRE(desc->dtype >= 0 && desc->dtype <= 2, "dtype");
    REQUIRE(desc->n_mel == 80 || desc->n_mel == 128, "n_mel must be 80 or 128");
    REQUIRE(desc->n_audio_ctx * 2 == kFrames, "n_audio_ctx must be 1500");
    HIPCHK(hipSetDevice(device));
    auto h = std::make_unique<wcb_handle>();
    h->d = *desc;
    h->dt = DType(desc->dtype);
    h->device = device;
    HIPCHK(hipStreamCreateWithPriority(&h->he, hipStreamNonBlocking, 0));
    // decode streams: created on first use (ensure_ctx_streams), one per decode context in use. HIP
    // maps streams onto a small pool of hardware queues (GPU_MAX_HW_QUEUES, 4 by default); a context
    // whose queue is shared with the caller's stream inherits the caller's cross-stream waits (the
    // sync_out of every front-end call), which serialised the two decode chains (measured: C2 step
    // 102-139 ms when the library's streams predated the caller's, 52 ms otherwise). Streams that are
    // never used take no queue.
    for (int ci = 0; ci < wcb_handle::kMaxCtx; ++ci) {
      DecCtx& D = h->dc[ci];
      HIPCHK(hipEventCreateWithFlags(&D.ev_fork, hipEventDisableTiming));
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&D.done_h), 2 * sizeof(int), hipHostMallocDefault));
      for (hipEvent_t& e : D.ev_poll) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      for (int i = 0; i < DecCtx::kMaxSub; ++i) HIPCHK(hipEventCreateWithFlags(&D.ev_join[i], hipEventDisableTiming));
    }
    for (int i = 0; i < wcb_handle::kMaxCtx; ++i) {
      HIPCHK(hipEventCreateWithFlags(&h->ev_xkv[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&h->ev_dec[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
    h->xvariant = desc->n_heads >= 20 ? 1 : 0;
    h->xmode = xenc_supported(h->dt, desc->d_model) ? 1 : 0;
    h->beam_xmode = 0;
    if (h->dt == kF32) h->ln16 = 0;   // f32 "exact" mode: the copy would be the f32 rows themselves
    h->dec_gemm = gemm_dec_supported(h->dt, desc->d_model);
    // DFT table [416 cols][416 k]: col 2b = win·cos(2πbk/400), col 2b+1 = −win·sin(2πbk/400)
    std::vector<float> dft((size_t)kNCol * kNCol, 0.f);
    for (int c = 0; c < 402; ++c) {
      const int bin = c >> 1;
      for (int k = 0; k < 400; ++k) {
        const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * k / 400.0);
        const double ang = 2.0 * M_PI * (double)((long)bin * k % 400) / 400.0;
        dft[(size_t)c * kNCol + k] = (float)(win * ((c & 1) ? -std::sin(ang) : std::cos(ang)));
      }
    }
    h->dft.ensure(dft.size() * 4);
    HIPCHK(hipMemcpy(h->dft.p, dft.data(), dft.size() * 4, hipMemcpyHostToDevice));
    {   // the same table as three bf16 parts (hi, mid, lo: each the RNE bf16 of the remainder of the double
        // value): the split-bf16 DFT (k_logmel.hip SPLIT) multiplies with these
      auto bf = [](double v, double& back) -> uint16_t {
        const float f = (float)v;
        uint32_t u;
        std::memcpy(&u, &f, 4);
        u += 0x7fffu + ((u >> 16) & 1u);   // round to nearest even (finite values only)
        const uint16_t hbits = (uint16_t)(u >> 16);
        const uint32_t w = (uint32_t)hbits << 16;
        float g;
        std::memcpy(&g, &w, 4);
        back = g;
        return hbits;
      };
      std::vector<uint16_t> t3((size_t)3 * kNCol * kNCol, 0);
      for (int c = 0; c < 402; ++c) {
        const int bin = c >> 1;
        for (int k = 0; k < 400; ++k) {
          const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * k / 400.0);
          const double ang = 2.0 * M_PI * (double)((long)bin * k % 400) / 400.0;
          double r = win * ((c & 1) ? -std::sin(ang) : std::cos(ang)), back;
          for (int part = 0; part < 3; ++part) {
            t3[(size_t)part * kNCol * kNCol + (size_t)c * kNCol + k] = bf(r, back);
            r -= back;
          }
        }
      }
      h->dft3.ensure(t3.size() * 2);
      HIPCHK(hipMemcpy(h->dft3.p, t3.data(), t3.size() * 2, hipMemcpyHostToDevice));
    }
    const auto fb = mel_filters(desc->n_mel);
    std::vector<int> lo(desc->n_mel), hi(desc->n_mel);
    std::vector<float> w((size_t)desc->n_mel * 32, 0.f);
    for (int m = 0; m < desc->n_mel; ++m) {
      int a = -1, b = -1;
      for (int k = 0; k < 201; ++k)
        if ((float)fb[(size_t)k * desc->n_mel + m] != 0.f) { if (a < 0) a = k; b = k; }
      if (a < 0) { a = 0; b = -1; }
      REQUIRE(b - a + 1 <= 32, "mel filter wider than 32 bins");
      lo[m] = a;
      hi[m] = b + 1;
      for (int k = a; k <= b; ++k) w[(size_t)m * 32 + (k - a)] = (float)fb[(size_t)k * desc->n_mel + m];
    }
    h->mel_lo.ensure(lo.size() * 4);
    h->mel_hi.ensure(hi.size() * 4);
    h->mel_w.ensure(w.size() * 4);
    HIPCHK(hipMemcpy(h->mel_lo.p, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mel_hi.p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mel_w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    // empty automaton (root only) so greedy without a bias list uses the same kernels
    auto eb = std::make_unique<wcb_bias>();
    eb->vocab = desc->vocab;
    const int nw = (desc->vocab + 31) / 32;
    eb->root_bits.ensure((size_t)nw * 4);
    eb->root_child.ensure((size_t)desc->vocab * 4);
    HIPCHK(hipMemsetAsync(eb->root_child.p, 0xff, (size_t)desc->vocab * 4, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    std::vector<int> off = {0, 0};
    eb->trans_off.ensure(8);
    HIPCHK(hipMemcpy(eb->trans_off.p, off.data(), 8, hipMemcpyHostToDevice));
    eb->trans_tok.ensure(4);
    eb->trans_dst.ensure(4);
    eb->st_depth.ensure(4);   // root: depth 0, keep 0 (zeroed)
    eb->st_keep.ensure(4);
    h->empty_bias = std::move(eb);
    h->dev_err.ensure(4);
    *out = h.release();
  });
}

void wcb_destroy(wcb_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (wcb_bias* b : h->biases) b->owner = nullptr;   // still valid to destroy; no graph holds them now
  for (DecCtx& D : h->dc) {
    D.drop_graphs();
    for (DevBuf* b : {&D.kvself, &D.dx, &D.dx16, &D.dx16fm, &D.dh, &D.dq, &D.dqp, &D.du, &D.datt, &D.dffn, &D.dstats, &D.drst, &D.xpart, &D.xml, &D.xticket,
                      &D.logits, &D.part_val, &D.part_idx, &D.ints, &D.outbuf, &D.forced, &D.beam, &D.kq_cnt, &D.part_max, &D.part_sum,
                      &D.lpbuf})
      b->release();
    if (D.ev_fork) (void)hipEventDestroy(D.ev_fork);
    for (hipEvent_t e : D.ev_poll)
      if (e) (void)hipEventDestroy(e);
    if (D.done_h) (void)hipHostFree(D.done_h);
    D.forest.release();
    D.poff.release();
    D.seen.release();
    D.rep_par.release();
    D.nsp.release();
    D.lang.release();
    if (D.p_stage) (void)hipHostFree(D.p_stage);
    if (D.ev_pcopy) (void)hipEventDestroy(D.ev_pcopy);
    if (D.f_stage) (void)hipHostFree(D.f_stage);
    if (D.ev_fcopy) (void)hipEventDestroy(D.ev_fcopy);
    for (int i = 0; i < DecCtx::kMaxSub; ++i) {
      if (D.ev_join[i]) (void)hipEventDestroy(D.ev_join[i]);
      if (D.sub[i]) (void)hipStreamDestroy(D.sub[i]);
    }
    if (D.hs) (void)hipStreamDestroy(D.hs);
  }
  for (auto& b : h->owned) b.release();
  for (DevBuf* b : {&h->dft, &h->dft3, &h->mel_lo, &h->mel_hi, &h->mel_w, &h->clip_max, &h->win_ints, &h->xt, &h->hbuf, &h->x, &h->h,
                    &h->qkv, &h->att, &h->ffn, &h->encout, &h->stamps, &h->stamp_acc, &h->dev_err, &h->rules_deny,
                    &h->rules_deny0, &h->al_w, &h->al_M, &h->al_tf, &h->al_lens, &h->al_frames, &h->al_prefix, &h->al_trace})
    b->release();
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->ev_align) (void)hipEventDestroy(h->ev_align);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  if (h->ev_out) (void)hipEventDestroy(h->ev_out);
  if (h->he) (void)hipStreamDestroy(h->he);
  for (int i = 0; i < wcb_handle::kMaxCtx; ++i) {
    h->xkv2[i].release();
    if (h->ev_xkv[i]) (void)hipEventDestroy(h->ev_xkv[i]);
    if (h->ev_dec[i]) (void)hipEventDestroy(h->ev_dec[i]);
  }
  delete h;
}

namespace {
void quiesce(wcb_handle* h);
void drop_graphs(wcb_handle* h);
}  // namespace

int wcb_set_option(wcb_handle* h, const char* name, int value) {
  return guarded(h, [&] {
    REQUIRE(h && name, "bad argument");
    const std::string n = name;
    // An open step-wise decode carries device state across wcb_decode_step calls that the decode options
    // shaped (the next input's embedding and its fragment-major copy, the LayerNorm statistics the residual
    // writers published, the encoder-output layout): only the encoder-side and generate()-only options may
    // change under it (decode_contexts has its own check below).
    static const char* const kFreeWhileStepwise[] = {"decode_contexts", "enc_flash", "enc_gemm", "enc_raster",
                                                     "steps_per_graph", "kq_cnt_seed", "align_ws"};
    bool free_opt = false;
    for (const char* f : kFreeWhileStepwise) free_opt |= n == f;
    REQUIRE(free_opt || !h->step_state, "option " + n + ": a step-wise decode is active (wcb_decode_end first)");
    if (n == "xmode" || n == "beam_xmode") {
      REQUIRE(!h->ready, "option " + n + " selects the weight layouts: set it before wcb_finalize_weights");
      REQUIRE(value == 0 || value == 1, "option " + n + ": 0 or 1");
      // encoder space only where the kernel exists (16-bit, d <= 1024): elsewhere the K/V formulation
      if (n == "xmode") h->xmode = value && xenc_supported(h->dt, h->d.d_model);
      else h->beam_xmode = value && h->xmode;
      if (!h->xmode) h->beam_xmode = 0;
    } else if (n == "decode_contexts") {
      REQUIRE(value >= 1 && value <= wcb_handle::kMaxCtx, "option decode_contexts: 1..4");
      // the step-wise state owns context kMaxCtx-1: generate() may not cycle into it while it is open
      REQUIRE(!h->step_state || value < wcb_handle::kMaxCtx,
              "option decode_contexts: 4 while a step-wise decode is active (wcb_decode_end first)");
      h->nctx = value;
    } else if (n == "group_rows") {
      REQUIRE(value >= 16 && value <= 512, "option group_rows: 16..512");
      h->group_rows = value;
    } else if (n == "xenc_variant") {
      REQUIRE(value >= 0 && value <= 3, "option xenc_variant: 0..3");
      h->xenc_variant = value;
    } else if (n == "enc_flash") {
      REQUIRE(value == 2 || value == 4, "option enc_flash: 2 or 4");
      h->enc_flash_qw = value;
    } else if (n == "xenc_split") {
      REQUIRE(!h->ready, "option xenc_split: set before the weights are finalized");
      REQUIRE(value >= 1 && value <= kXencMaxSplit, "option xenc_split: 1..16");
      h->xenc_split = value;
    } else if (n == "lm_ln_split") {
      h->lm_ln_split = value != 0;
    } else if (n == "ring_kt") {
      REQUIRE(value == 1 || value == 2, "option ring_kt: 1 or 2");
      h->ring_kt = value;
    } else if (n == "kq_cnt_seed") {
      // test hook: every allocated arrival counter of the fused xq+kq launches set to 4·value (a generation
      // boundary of the 4-member groups), e.g. just below 2^31 or 2^32 to check that no counter width wraps
      REQUIRE(value >= 0, "option kq_cnt_seed: >= 0");
      quiesce(h);
      for (DecCtx& D : h->dc) {
        if (!D.kq_cnt.p) continue;
        std::vector<unsigned long long> v(D.kq_cnt.bytes / 8, 4ull * (unsigned long long)value);
        HIPCHK(hipMemcpy(D.kq_cnt.p, v.data(), v.size() * 8, hipMemcpyHostToDevice));
      }
    } else if (n == "align_ws") {
      REQUIRE(value >= 1 && value <= 65536, "option align_ws: 1..65536 (MiB)");
      h->align_ws_bytes = (size_t)value << 20;
    } else if (n == "steps_per_graph") {
      REQUIRE(value >= 1 && value <= 64, "option steps_per_graph: 1..64");
      h->steps_per_graph = value;
    } else if (n == "xenc_fm") {
      h->xenc_fm = value != 0;
    } else if (n == "xq_kq") {
      h->xq_kq = value != 0;
    } else if (n == "enc_gemm") {
      REQUIRE(value == 0 || value == 1 || value == 4 || value == 5, "option enc_gemm: 0, 1, 4 or 5");
      h->enc_gemm = value;
    } else if (n == "enc_raster") {
      REQUIRE(value >= 0 && value <= 64, "option enc_raster: 0..64");
      h->enc_raster = value;
    } else if (n == "lean") {
      // the lean path's fragment-major weight copies are built at finalize only when it is on
      REQUIRE(!h->ready, "option lean selects weight layouts: set it before wcb_finalize_weights");
      h->lean = value != 0;
    } else if (n == "lean_x") {
      h->lean_x = value != 0;
    } else if (n == "xpart16") {
      h->xpart16 = value != 0;
    } else if (n == "merge_v") {
      h->merge_v = value != 0;
    } else if (n == "ln_fold") {
      // the folded W·diag(γ) copies are built at finalize only when it is on
      REQUIRE(!h->ready, "option ln_fold selects weight layouts: set it before wcb_finalize_weights");
      h->ln_fold = value != 0;
    } else if (n == "lean_mf2") {
      h->lean_mf2 = value != 0;
    } else if (n == "mel_split") {
      h->mel_split = value != 0;
    } else if (n == "lm_walkers") {
      REQUIRE(!h->ready, "option lm_walkers sizes the argmax partials: set it before wcb_finalize_weights");
      REQUIRE(value == 128 || value == 192 || value == 256 || value == 384 || value == 512 || value == 1024,
              "option lm_walkers: 128, 192, 256, 384, 512 or 1024");
      h->lm_walkers = value;
    } else if (n == "merge_os") {
      REQUIRE(value == 1 || value == 2, "option merge_os: 1 or 2");
      h->merge_os = value;
    } else if (n == "xqk_chunks") {
      REQUIRE(value == 2 || value == 4 || value == 8 || value == 16, "option xqk_chunks: 2, 4, 8 or 16");
      h->xqk_nch = value;
    } else if (n == "xqk") {
      h->xqk = value != 0;
    } else if (n == "lean_fold") {
      REQUIRE(!h->ready, "option lean_fold selects weight layouts: set it before wcb_finalize_weights");
      h->lean_fold = value != 0;
    } else if (n == "beam_chunks") {
      h->beam_chunks = value != 0;
    } else if (n == "beam_wfm") {
      REQUIRE(!h->ready, "option beam_wfm selects weight layouts: set it before wcb_finalize_weights");
      h->beam_wfm = value != 0;
    } else if (n == "beam_raster") {
      REQUIRE(value >= 0 && value <= 64, "option beam_raster: 0..64");
      h->beam_raster = value;
    } else if (n == "beam_wide") {
      // the wide tiles read fragment-major copies of the folded xq / fc1 weights, built at finalize
      REQUIRE(!h->ready, "option beam_wide selects weight layouts: set it before wcb_finalize_weights");
      h->beam_wide = value != 0;
    } else if (n == "beam_xattn") {
      REQUIRE(value >= 0 && value <= 3, "option beam_xattn: 0..3");
      h->beam_xattn = value;
    } else if (n == "flash_split") {
      REQUIRE(value >= 1 && value <= kXSplit, "option flash_split: 1..8");
      h->flash_split = value;
    } else if (n == "xvariant") {
      REQUIRE(value >= 0 && value <= 5, "option xvariant: 0..5");
      h->xvariant = value;
    } else {
      throw WcbError(WCB_ERR_ARG, "unknown option " + n);
    }
    quiesce(h);
    drop_graphs(h);   // captured decode steps baked the old configuration in
  });
}

int wcb_set_weight(wcb_handle* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return guarded(h, [&] {
    REQUIRE(h && name && data && shape && ndim >= 1, "null argument");
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    HIPCHK(hipSetDevice(h->device));
    DevBuf& b = h->staged[name];
    b.release();
    b.ensure(n * 4);
    HIPCHK(hipMemcpy(b.p, data, n * 4, hipMemcpyHostToDevice));
  });
}

int wcb_load_weights(wcb_handle* h, const wcb_tensor_view* views, int n, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && (views || n == 0) && n >= 0, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < n; ++k) {
      const wcb_tensor_view& v = views[k];
      REQUIRE(v.name && v.data && v.ndim >= 1 && v.ndim <= 4, "bad tensor view");
      REQUIRE(v.dtype == WCB_F32 || v.dtype == WCB_BF16 || v.dtype == WCB_F16, "tensor view dtype");
      WeightView w;   // right-aligned into 4 dims
      size_t cnt = 1;
      for (int i = 0; i < v.ndim; ++i) {
        REQUIRE(v.shape[i] >= 1, "tensor view shape");
        w.shape[4 - v.ndim + i] = v.shape[i];
        w.stride[4 - v.ndim + i] = v.stride[i];
        cnt *= (size_t)v.shape[i];
      }
      DevBuf& b = h->staged[v.name];
      b.release();
      b.ensure(cnt * 4);
      view_to_f32(DType(v.dtype), v.data, w, b.as<float>(), s);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));   // the borrowed views are not read after return
  });
}

int wcb_finalize_weights(wcb_handle* h) {
  return guarded(h, [&] {
    REQUIRE(h, "null handle");
    HIPCHK(hipSetDevice(h->device));
    const int d = h->d.d_model, L = h->d.n_layers, F = h->d.ffn, V = h->d.vocab, nm = h->d.n_mel, H = h->H();
    const size_t dd = (size_t)d * d, e = esize(h->d.dtype);
    HIPCHK(hipStreamSynchronize(h->he));
    const hipStream_t st = h->he;
    // owned model-dtype / f32 tensors built from the staged f32 parameters on the device
    auto rp = [&](bool f32, void* dst, const float* src, std::initializer_list<int> n, std::initializer_list<long> sv,
                  std::initializer_list<long> tv, float scale = 1.f) {
      RepackArgs a;
      a.dst = dst; a.src = src; a.scale = scale;
      std::copy(n.begin(), n.end(), a.n);
      std::copy(sv.begin(), sv.end(), a.s);
      std::copy(tv.begin(), tv.end(), a.t);
      repack(f32 ? kF32 : h->dt, a, st);
    };
    auto dense = [&](bool f32, const float* src, size_t cnt, float scale = 1.f) -> void* {
      void* p = h->own(cnt * (f32 ? 4 : e));
      rp(f32, p, src, {1, 1, (int)cnt}, {0, 0, 1}, {0, 0, 1}, scale);
      return p;
    };
    auto T_ = [&](const std::string& name, size_t cnt, float scale = 1.f) { return dense(false, h->W(name, cnt), cnt, scale); };
    auto F_ = [&](const std::string& name, size_t cnt, float scale = 1.f) {
      return reinterpret_cast<float*>(dense(true, h->W(name, cnt), cnt, scale));
    };
    DevBuf check;
    check.ensure(4);
    // conv1: W1[o][c][k] → [o][k·n_mel + c], K padded to a multiple of 64 with zeros
    h->k1pad = (3 * nm + 63) / 64 * 64;
    h->conv1_w = h->own((size_t)d * h->k1pad * e);   // zeroed on allocation (the K padding)
    rp(false, h->conv1_w, h->W("model.encoder.conv1.weight", (size_t)d * nm * 3), {d, 3, nm}, {(long)nm * 3, 1, 3},
       {(long)h->k1pad, nm, 1});
    h->conv1_b = F_("model.encoder.conv1.bias", d);
    // conv2: W2[o][c][k] → [o][k·d + c]
    h->conv2_w = h->own(dd * 3 * e);
    rp(false, h->conv2_w, h->W("model.encoder.conv2.weight", dd * 3), {d, 3, d}, {(long)d * 3, 1, 3}, {3L * d, d, 1});
    h->conv2_b = F_("model.encoder.conv2.bias", d);
    h->enc_pos = F_("model.encoder.embed_positions.weight", (size_t)h->S() * d);
    auto attn_qkv = [&](const std::string& p, LayerW& lw) {
      // q scaling head_dim^-0.5 = 0.125 (exact power of two: folding it is bit-identical)
      lw.qkv_w = h->own(3 * dd * e);
      rp(false, lw.qkv_w, h->W(p + "q_proj.weight", dd), {1, 1, (int)dd}, {0, 0, 1}, {0, 0, 1}, 0.125f);
      rp(false, (char*)lw.qkv_w + dd * e, h->W(p + "k_proj.weight", dd), {1, 1, (int)dd}, {0, 0, 1}, {0, 0, 1});
      rp(false, (char*)lw.qkv_w + 2 * dd * e, h->W(p + "v_proj.weight", dd), {1, 1, (int)dd}, {0, 0, 1}, {0, 0, 1});
      lw.qkv_b = reinterpret_cast<float*>(h->own(3 * (size_t)d * 4));   // k has no bias: zeros
      rp(true, lw.qkv_b, h->W(p + "q_proj.bias", d), {1, 1, d}, {0, 0, 1}, {0, 0, 1}, 0.125f);
      rp(true, lw.qkv_b + 2 * d, h->W(p + "v_proj.bias", d), {1, 1, d}, {0, 0, 1}, {0, 0, 1});
      lw.o_w = T_(p + "out_proj.weight", dd);
      lw.o_b = F_(p + "out_proj.bias", d);
    };
    auto mlp = [&](const std::string& p, LayerW& lw) {
      lw.ln1_w = F_(p + "self_attn_layer_norm.weight", d);
      lw.ln1_b = F_(p + "self_attn_layer_norm.bias", d);
      lw.ln2_w = F_(p + "final_layer_norm.weight", d);
      lw.ln2_b = F_(p + "final_layer_norm.bias", d);
      lw.fc1_w = T_(p + "fc1.weight", (size_t)F * d);
      lw.fc1_b = F_(p + "fc1.bias", F);
      lw.fc2_w = T_(p + "fc2.weight", (size_t)d * F);
      lw.fc2_b = F_(p + "fc2.bias", d);
    };
    auto zero_bias = [&](const std::string& name) {   // Whisper's encoder_attn.k_proj has no bias
      auto it = h->staged.find(name);
      if (it == h->staged.end()) return;
      count_diff(it->second.as<float>(), nullptr, (long)(it->second.bytes / 4), check.as<int>(), st);
    };
    h->enc.assign(L, LayerW{});
    h->dec.assign(L, LayerW{});
    const bool kv_stack = h->xmode == 0 || h->beam_xmode == 0;
    if (kv_stack) {
      h->xkv_w = h->own((size_t)2 * L * dd * e);
      h->xkv_b = reinterpret_cast<float*>(h->own((size_t)2 * L * d * 4));   // k rows: zero bias
    }
    for (int i = 0; i < L; ++i) {
      const std::string pe = "model.encoder.layers." + std::to_string(i) + ".";
      attn_qkv(pe + "self_attn.", h->enc[i]);
      mlp(pe, h->enc[i]);
      const std::string pd = "model.decoder.layers." + std::to_string(i) + ".";
      attn_qkv(pd + "self_attn.", h->dec[i]);
      mlp(pd, h->dec[i]);
      LayerW& lw = h->dec[i];
      lw.xq_w = T_(pd + "encoder_attn.q_proj.weight", dd, 0.125f);
      lw.xq_b = F_(pd + "encoder_attn.q_proj.bias", d, 0.125f);
      lw.xo_w = T_(pd + "encoder_attn.out_proj.weight", dd);
      lw.xo_b = F_(pd + "encoder_attn.out_proj.bias", d);
      lw.lnx_w = F_(pd + "encoder_attn_layer_norm.weight", d);
      lw.lnx_b = F_(pd + "encoder_attn_layer_norm.bias", d);
      const float* wk = h->W(pd + "encoder_attn.k_proj.weight", dd);
      const float* wv = h->W(pd + "encoder_attn.v_proj.weight", dd);
      const float* bv = h->W(pd + "encoder_attn.v_proj.bias", d);
      zero_bias(pd + "encoder_attn.k_proj.bias");
      if (h->xmode == 1) {
        // W_k,hᵀ: [H][d][64], element (h, c, i) = W_k[h·64 + i][c] (K = 64 contiguous for the MFMA)
        lw.xkt_w = h->own(dd * e);
        rp(false, lw.xkt_w, wk, {H, d, 64}, {64L * d, 1, d}, {(long)d * 64, 64, 1});
        lw.xv_w = dense(false, wv, dd);
        lw.xv_b = reinterpret_cast<float*>(dense(true, bv, d));
      }
      if (kv_stack) {   // cross K/V projection of every layer fused into one [2·L·d][d] weight: rows (l, k|v, d)
        rp(false, (char*)h->xkv_w + (size_t)(2 * i) * dd * e, wk, {1, 1, (int)dd}, {0, 0, 1}, {0, 0, 1});
        rp(false, (char*)h->xkv_w + (size_t)(2 * i + 1) * dd * e, wv, {1, 1, (int)dd}, {0, 0, 1}, {0, 0, 1});
        rp(true, h->xkv_b + (size_t)(2 * i + 1) * d, bv, {1, 1, d}, {0, 0, 1}, {0, 0, 1});
      }
    }
    if (h->dt != kF32) {
      for (int i = 0; i < L; ++i) {
        LayerW& lw = h->dec[i];
        // W' = W·diag(γ) rounded to T, u = Σ_k W'[n][k] (of the rounded W': the epilogue's μ·u then
        // removes exactly the mean the accumulator carries), c = Σ_k β_k W[n][k] + bias
        auto fold = [&](const void* W, int N, const float* gam, const float* bet, const float* bias, void*& Wg, float*& u,
                        float*& c) {
          Wg = h->own((size_t)N * d * e);
          u = reinterpret_cast<float*>(h->own((size_t)N * 4));
          c = reinterpret_cast<float*>(h->own((size_t)N * 4));
          scale_cols(h->dt, W, N, d, gam, Wg, st);
          ln_fold(h->dt, W, N, d, gam, bet, bias, u, c, st);          // c (u overwritten below)
          ln_fold(h->dt, Wg, N, d, nullptr, nullptr, nullptr, u, nullptr, st);
        };
        if (h->ln_fold) {   // (decode rows > 64 only; memory: QKV + xq + fc1 weights once more per layer)
          fold(lw.qkv_w, 3 * d, lw.ln1_w, lw.ln1_b, lw.qkv_b, lw.qkv_wg, lw.ln1_u, lw.ln1_c);
          fold(lw.xq_w, d, lw.lnx_w, lw.lnx_b, lw.xq_b, lw.xq_wg, lw.lnx_u, lw.lnx_c);
          fold(lw.fc1_w, F, lw.ln2_w, lw.ln2_b, lw.fc1_b, lw.fc1_wg, lw.ln2_u, lw.ln2_c);
        }
        // fragment-major copies for the lean decode projections (<= 64 rows): each weight wave-instruction
        // then reads 1 KiB contiguous (tools/dec_kernel_bench.hip: out 3.75 -> 3.16, fc2 8.39 -> 6.43 µs)
        auto fm = [&](const void* W, int N, int K) -> void* {
          int nw = 0, kpw = 0;
          if (!h->lean || !W || N % 16 || !lean_cfg(K, nw, kpw)) return nullptr;   // (lean path only)
          void* p = h->own((size_t)N * K * e);
          frag_major(h->dt, W, N, K, nw, kpw, p, st);
          return p;
        };
        lw.qkv_fm = fm(lw.qkv_w, 3 * d, d);
        lw.o_fm = fm(lw.o_w, d, d);
        lw.xq_fm = fm(lw.xq_w, d, d);
        lw.xo_fm = fm(lw.xo_w, d, d);
        lw.fc1_fm = fm(lw.fc1_w, F, d);
        lw.fc2_fm = fm(lw.fc2_w, d, F);
        if (lw.xkt_w) lw.xkt_fm = fm(lw.xkt_w, H * d, 64);
        if ((h->beam_wide || h->beam_wfm || h->lean_fold) && h->ln_fold) {   // the folded weights fragment-major
          lw.xq_wgfm = fm(lw.xq_wg, d, d);
          lw.fc1_wgfm = fm(lw.fc1_wg, F, d);
          if (h->beam_wfm || h->lean_fold) lw.qkv_wgfm = fm(lw.qkv_wg, 3 * d, d);
        }
        if (lw.xv_w && h->lean && h->dt != kF32 && d % 128 == 0 && d <= 1024) {   // 16 output rows per wave, all of K per wave
          lw.xv_fm = h->own((size_t)d * d * e);
          frag_major(h->dt, lw.xv_w, d, d, 1, d / 32, lw.xv_fm, st);
        }
      }
    }
    h->enc_ln_w = F_("model.encoder.layer_norm.weight", d);
    h->enc_ln_b = F_("model.encoder.layer_norm.bias", d);
    h->dec_ln_w = F_("model.decoder.layer_norm.weight", d);
    h->dec_ln_b = F_("model.decoder.layer_norm.bias", d);
    h->vocab_pad = (V + 127) / 128 * 128;   // zero rows past V (own() zeroes): logits columns ≥ V are 0
    h->tok_emb = h->own((size_t)h->vocab_pad * d * e);
    rp(false, h->tok_emb, h->W("model.decoder.embed_tokens.weight", (size_t)V * d), {1, 1, (int)((size_t)V * d)},
       {0, 0, 1}, {0, 0, 1});
    h->dec_pos = T_("model.decoder.embed_positions.weight", (size_t)h->d.n_text_ctx * d);
    if (h->dt != kF32) {   // the greedy LM head's column walk reads a fragment-major copy (zero rows past V)
      int nw = 0, kpw = 0;
      if (h->lean && lean_cfg(d, nw, kpw)) {
        h->tok_emb_fm = h->own((size_t)h->vocab_pad * d * e);
        frag_major(h->dt, h->tok_emb, h->vocab_pad, d, nw, kpw, h->tok_emb_fm, st);
      }
    }
    int bad_bias = 0, untied = 0;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(&bad_bias, check.p, 4, hipMemcpyDeviceToHost));
    REQUIRE(bad_bias == 0, "encoder_attn.k_proj has no bias in Whisper ([tf] modeling_whisper.py:279)");
    if (h->staged.count("proj_out.weight")) {   // tied to the embedding (models/whisper_medical.py:14)
      HIPCHK(hipMemsetAsync(check.p, 0, 4, st));
      const size_t n = (size_t)V * d;
      count_diff(h->W("proj_out.weight", n), h->W("model.decoder.embed_tokens.weight", n), (long)n, check.as<int>(), st);
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(&untied, check.p, 4, hipMemcpyDeviceToHost));
      REQUIRE(untied == 0, "proj_out.weight must be tied to model.decoder.embed_tokens.weight");
    }
    HIPCHK(hipGetLastError());
    h->staged.clear();
    h->ready = true;
  });
}

}  // extern "C"

// ============================================================================== pipelines
namespace {

// caller stream → library stream `to` (inputs ready)
void sync_in(wcb_handle* h, void* stream, hipStream_t to) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventRecord(h->ev_in, (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(to, h->ev_in, 0));
}
// library stream `from` → caller stream (outputs ready)
void sync_out(wcb_handle* h, void* stream, hipStream_t from) {
  HIPCHK(hipEventRecord(h->ev_out, from));
  HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0));
  HIPCHK(hipGetLastError());
}
// the device error word (after the streams drained): a hand-off that ran out its bound means the launch's
// workgroups were not co-resident and its outputs are unsynchronised — an error, never silent
void check_dev_err(wcb_handle* h) {
  int e = 0;
  HIPCHK(hipMemcpy(&e, h->dev_err.p, 4, hipMemcpyDeviceToHost));
  if (e) {
    HIPCHK(hipMemset(h->dev_err.p, 0, 4));
    throw WcbError(WCB_ERR_HIP, "an in-launch hand-off wait timed out (workgroups not co-resident): outputs invalid");
  }
}
// drain every library stream (before any workspace reallocation)
void quiesce(wcb_handle* h) {
  HIPCHK(hipStreamSynchronize(h->he));
  for (DecCtx& D : h->dc)
    if (D.hs) HIPCHK(hipStreamSynchronize(D.hs));
}

void ensure_enc_ws(wcb_handle* h, int B) {
  if (B <= h->enc_B) return;
  quiesce(h);
  const size_t e = esize(h->d.dtype), d = h->d.d_model, S = h->S(), M = (size_t)B * S;
  h->xt.ensure(((size_t)B * (kFrames + 2) * h->d.n_mel + 256) * e);
  h->hbuf.ensure(((size_t)B * (kFrames + 1) * d + 256) * e);
  h->x.ensure(M * d * 4);
  h->h.ensure(M * d * e);
  h->qkv.ensure(M * 3 * d * e);
  h->att.ensure(M * d * e);
  h->ffn.ensure(M * h->d.ffn * e);
  h->encout.ensure(M * d * e);
  h->clip_max.ensure((size_t)B * 4);
  h->enc_B = B;
}

GemmArgs rowgemm(const void* A, long lda, const void* W, int M, int N, int K, void* out, long ldc) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.M = M; g.N = N; g.K = K; g.out = out; g.ldc = ldc;
  return g;
}

// decode projections: always the skinny kernel (rows over grid.y), also for row groups > 64 rows
GemmArgs drow(const void* A, long lda, const void* W, int M, int N, int K, void* out, long ldc) {
  GemmArgs g = rowgemm(A, lda, W, M, N, K, out, ldc);
  g.skinny = 1;
  return g;
}

// algorithmic bytes of a decode-step GEMM: the weights once, the A rows, the written C rows
double gemm_bytes(const wcb_handle* h, const GemmArgs& g) {
  const double e = esize(h->d.dtype);
  const double a_bytes = g.ln_w && !g.ln_a16 ? 4.0 : e;
  const double c_bytes = g.out_f32 ? 4.0 : e;
  return (double)g.N * g.K * e + (double)g.M * g.K * a_bytes + (double)g.M * g.N * c_bytes;
}
// one decode-step GEMM launch; timed per class only in the eager profiling pass (events cannot
// bracket a node of a replayed graph)
void dgemm(wcb_handle* h, const char* cls, const GemmArgs& g, hipStream_t st) {
  h->timed(cls, 2.0 * g.M * g.N * g.K, gemm_bytes(h, g), st, [&] { gemm(h->dt, g, st); });
}

void run_gemm(wcb_handle* h, const char* cls, const GemmArgs& g0) {
  GemmArgs g = g0;
  g.raster = h->enc_raster;
  g.pp = h->enc_gemm;
  h->timed(cls, 2.0 * g.M * g.N * g.K, 0.0, h->he, [&] { gemm(h->dt, g, h->he); });
}

// WhisperEncoder.forward ([tf] modeling_whisper.py:592-646) on mel f32 [B][n_mel][3000]; the final
// LayerNorm writes [B][1500][d] to enc_out (h->encout when null)
// the windows of a long-form call: rows of 3000 frames cut from long features (wcb_windows, checked by check_windows)
constexpr int kWinRows = 64;
constexpr int kTimestampTokens = 1501;   // <|0.00|> .. <|30.00|>, the last ids of every Whisper vocabulary
void check_windows(const wcb_windows* w, int rows) {
  REQUIRE(w && w->mel && w->clip_idx && w->seek && w->seek_num_frames, "windows: mel, clip_idx, seek and seek_num_frames are required");
  REQUIRE(rows >= 1 && rows <= kWinRows, "windows: 1 .. 64 rows per call");
  REQUIRE(w->clips >= 1 && w->T >= 1 && w->T_ld >= w->T, "windows: clips >= 1 and 1 <= T <= T_ld are required");
  for (int r = 0; r < rows; ++r) {
    const std::string at = "windows row " + std::to_string(r) + ": ";
    REQUIRE(w->clip_idx[r] >= 0 && w->clip_idx[r] < w->clips, at + "clip index outside [0, clips)");
    REQUIRE(w->seek[r] >= 0, at + "seek < 0");
    REQUIRE(w->seek_num_frames[r] >= 1 && w->seek_num_frames[r] <= kFrames, at + "seek_num_frames outside [1, 3000]");
    REQUIRE((long)w->seek[r] + w->seek_num_frames[r] <= w->T, at + "seek + seek_num_frames > T");
  }
}
// the three int arrays onto the encoder stream (by value in a launch: the caller's arrays are free on return)
const int* upload_windows(wcb_handle* h, const wcb_windows* w, int rows) {
  h->win_ints.ensure((size_t)3 * kWinRows * 4);   // once: 3 x 64 ints
  int v[3 * kWinRows] = {};
  for (int r = 0; r < rows; ++r) {
    v[r] = w->clip_idx[r]; v[kWinRows + r] = w->seek[r]; v[2 * kWinRows + r] = w->seek_num_frames[r];
  }
  write_i32(h->win_ints.as<int>(), v, 3 * kWinRows, h->he);
  return h->win_ints.as<int>();
}

void encode_impl(wcb_handle* h, const float* mel, int B, void* enc_out, const wcb_windows* win = nullptr) {
  ensure_enc_ws(h, B);
  const int d = h->d.d_model, S = h->S(), nm = h->d.n_mel, H = h->H();
  const long M = (long)B * S;
  const size_t e = esize(h->d.dtype);
  const long xt_stride = (long)(kFrames + 2) * nm, hb_stride = (long)(kFrames + 1) * d;
  if (win) {   // long-form: row b is a window of the long features, cut on the chip
    const int* wi = upload_windows(h, win, B);
    h->timed("mel_window_cut", 0, 0, h->he, [&] {
      mel_window_to_conv_input(h->dt, win->mel, nm, win->T_ld, wi, wi + kWinRows, wi + 2 * kWinRows, B, h->xt.p, xt_stride, h->he);
    });
  } else {
    h->timed("mel_to_conv_input", 0, 0, h->he, [&] { mel_to_conv_input(h->dt, mel, B, nm, h->xt.p, xt_stride, h->he); });
  }
  {  // conv1 + GELU → hbuf rows 1..3000 of every clip (row 0 = conv2's zero padding)
    GemmArgs g = rowgemm(h->xt.p, nm, h->conv1_w, B * kFrames, d, h->k1pad, (char*)h->hbuf.p + d * e, d);
    g.a_Mb = kFrames; g.a_strideB = xt_stride;
    g.c_Mb = kFrames; g.c_strideB = hb_stride;
    g.bias = h->conv1_b; g.act = 1;
    run_gemm(h, "enc_conv1", g);
  }
  {  // conv2 (stride 2) + GELU + positions → x (f32 residual stream)
    GemmArgs g = rowgemm(h->hbuf.p, 2L * d, h->conv2_w, (int)M, d, 3 * d, h->x.p, d);
    g.a_Mb = S; g.a_strideB = hb_stride;
    g.c_Mb = S; g.c_strideB = (long)S * d;   // c_Mb also indexes the position table
    g.bias = h->conv2_b; g.act = 1; g.addrow = h->enc_pos; g.out_f32 = 1;
    run_gemm(h, "enc_conv2", g);
  }
  const int nl = h->dbg_enc_layers >= 0 ? std::min(h->dbg_enc_layers, h->d.n_layers) : h->d.n_layers;
  for (int l = 0; l < nl; ++l) {
    const LayerW& w = h->enc[l];
    h->timed("layernorm", 0, M * d * (4.0 + e), h->he, [&] { layernorm(h->dt, h->x.as<float>(), w.ln1_w, w.ln1_b, h->h.p, (int)M, d, h->he); });
    GemmArgs q = rowgemm(h->h.p, d, w.qkv_w, (int)M, 3 * d, d, h->qkv.p, 3 * d);
    q.bias = w.qkv_b;
    run_gemm(h, "enc_qkv", q);
    AttnArgs a;
    a.q = h->qkv.p; a.ldq = 3 * d; a.q_Sb = S; a.Sq = S;
    a.k = (char*)h->qkv.p + d * e; a.v = (char*)h->qkv.p + 2 * d * e;
    a.k_sb = (long)S * 3 * d; a.k_sh = 64; a.k_sk = 3 * d;
    a.o = h->att.p; a.ldo = d; a.o_Sb = S; a.B = B; a.H = H; a.nkeys = S;
    a.variant = h->dt == kF32 ? 4 : h->enc_flash_qw;   // (f32: the VALU kernel below)
    h->timed("enc_attn", 4.0 * B * H * (double)S * S * 64, 0, h->he, [&] {
      if (!attention_flash(h->dt, a, h->he)) attention_decode(h->dt, a, h->he);
    });
    GemmArgs o = rowgemm(h->att.p, d, w.o_w, (int)M, d, d, h->x.p, d);
    o.bias = w.o_b; o.resid = h->x.as<float>(); o.out_f32 = 1;
    run_gemm(h, "enc_out", o);
    h->timed("layernorm", 0, M * d * (4.0 + e), h->he, [&] { layernorm(h->dt, h->x.as<float>(), w.ln2_w, w.ln2_b, h->h.p, (int)M, d, h->he); });
    GemmArgs f1 = rowgemm(h->h.p, d, w.fc1_w, (int)M, h->d.ffn, d, h->ffn.p, h->d.ffn);
    f1.bias = w.fc1_b; f1.act = 1;
    run_gemm(h, "enc_fc1", f1);
    GemmArgs f2 = rowgemm(h->ffn.p, h->d.ffn, w.fc2_w, (int)M, d, h->d.ffn, h->x.p, d);
    f2.bias = w.fc2_b; f2.resid = h->x.as<float>(); f2.out_f32 = 1;
    if (h->dt == kF16) f2.clamp = 65504.f - 1000.f;   // fp16 layer-output clamp (large-v3 fp16 config)
    run_gemm(h, "enc_fc2", f2);
  }
  void* dst = enc_out ? enc_out : h->encout.p;
  h->timed("layernorm", 0, M * d * (4.0 + e), h->he, [&] { layernorm(h->dt, h->x.as<float>(), h->enc_ln_w, h->enc_ln_b, dst, (int)M, d, h->he); });
}

// device ints of a decode context: I_TU = the greedy select's 64-bit arrival | unfinished counter (8-byte aligned)
enum { I_STEP = 0, I_POS = 1, I_DONE = 2, I_TICKET = 3, I_UNFIN = 4, I_TU = 6, I_NEXT = 16 };

// the per-row ints of a decode of R rows, behind I_NEXT: [R] each, ts_state [R][2] (token rules: the timestamp
// grammar's row state, read by the ruled greedy finalize alone)
struct RowInts {
  int *next, *state, *finished, *rowbase, *ts_state;   // input ids, automaton state, finished flag, k - d of the state
  RowInts(const DecCtx& D, int R)
      : next(D.ints.as<int>() + I_NEXT), state(next + R), finished(next + 2 * R), rowbase(next + 3 * R), ts_state(next + 4 * R) {}
  // the int block of R rows: what ensure_dec_ws allocates (+ 16 of slack) and the start of a decode zeroes
  static size_t words(int R) { return I_NEXT + 6 * (size_t)R; }
};

void drop_graphs(wcb_handle* h) {
  for (DecCtx& D : h->dc) D.drop_graphs();
}

// positions per prefill pass: up to kPrefillRows activation rows (bounds the row workspaces)
constexpr int kPrefillRows = 256;
int prefill_chunk(int R) { return std::max(1, kPrefillRows / std::max(R, 1)); }
// activation rows of a decode of R rows whose prefill carries n positions (none: its steps' R rows)
int prefill_rows(int R, int n) { return n > 0 ? R * std::min(prefill_chunk(R), n) : R; }

// decode workspace: B decoder rows (clips x beams) reading `clips` encoder outputs; activation
// buffers for `rows` >= B rows (a prefill pass carries several positions per decoder row)
// contexts [c0, c1) (default: the generate() contexts 0 .. nctx-1; the step-wise decode state owns
// context kMaxCtx-1)
// the decode streams of contexts [c0, c1), created on first use at the highest priority (the decode
// chains are latency-bound and the next batch's encoder runs beside them: their workgroups dispatch
// ahead of encoder tiles); row-group streams only when n_sub > 1
hipStream_t make_dec_stream(wcb_handle* h) {
  hipStream_t s = nullptr;
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_hi));
  return s;
}

void ensure_ctx_streams(wcb_handle* h, int c0, int c1) {
  for (int ci = c0; ci < c1; ++ci) {
    DecCtx& D = h->dc[ci];
    if (D.hs && (h->n_sub <= 1 || D.sub[0])) continue;
    if (!D.hs) D.hs = make_dec_stream(h);
    for (int i = 0; i < DecCtx::kMaxSub && h->n_sub > 1; ++i)
      if (!D.sub[i]) D.sub[i] = make_dec_stream(h);
  }
}

void ensure_dec_ws(wcb_handle* h, int clips, int B, int T, int out_ld, int xmode, int rows = 0, int c0 = 0, int c1 = -1) {
  if (c1 < 0) c1 = h->nctx;
  ensure_ctx_streams(h, c0, c1);
  rows = std::max(rows, B);
  const size_t e = esize(h->d.dtype), d = h->d.d_model, L = h->d.n_layers, S = h->S();
  const DecCtx& D0 = h->dc[c1 - 1];   // every context of the range is sized together
  const size_t xbuf = xmode ? (size_t)xenc_fm_elems(clips, (int)S, (int)d) * e : 2 * L * (size_t)clips * S * d * e;
  const size_t need[] = {xbuf, 2 * L * (size_t)B * T * d * e, (size_t)rows * d * 4,
                         (size_t)rows * h->d.ffn * e, (size_t)B * h->vocab_pad * 4, (RowInts::words(B) + 16) * 4,
                         (size_t)B * out_ld * 4};
  const DevBuf* have[] = {&h->xkv2[c1 - 1], &D0.kvself, &D0.dx, &D0.dffn, &D0.logits, &D0.ints, &D0.outbuf};
  bool grow = false;
  for (int i = 0; i < 7; ++i) grow |= need[i] > have[i]->bytes;
  if (!grow && B <= D0.dec_B && T <= D0.dec_T) return;
  quiesce(h);
  drop_graphs(h);
  for (int ci = c0; ci < c1; ++ci) {
    DecCtx& D = h->dc[ci];
    h->xkv2[ci].ensure(need[0]);
    D.kvself.ensure(need[1]);
    D.dec_B = std::max(D.dec_B, B);
    D.dec_T = std::max(D.dec_T, T);
    D.dx.ensure((size_t)rows * d * 4);
    D.dx16.ensure((size_t)rows * d * e);
    D.dh.ensure((size_t)rows * d * e);
    D.dq.ensure((size_t)rows * d * e);
    D.datt.ensure((size_t)rows * d * e);
    // fragment-major copies: whole 16-row blocks, two blocks of slack (a 32-row workgroup past the rows)
    D.dffn.ensure(((size_t)(rows + 15) / 16 * 16 + 32) * h->d.ffn * e);
    D.dx16fm.ensure(((size_t)(rows + 15) / 16 * 16 + 32) * d * e);
    D.dstats.ensure((size_t)rows * (d / 16) * 2 * 4);
    D.drst.ensure((size_t)rows * (d / 32) * 2 * 4);
    D.xpart.ensure(std::max((size_t)rows * h->H() * kXSplit * 66, (size_t)rows * h->xenc_split * h->H() * d) * 4);
    D.xml.ensure((size_t)rows * h->xenc_split * h->H() * 2 * 4);
    D.dqp.ensure((size_t)rows * h->H() * d * e);
    D.du.ensure((size_t)rows * h->H() * d * e);
    D.xticket.ensure((size_t)rows * h->H() * 4);     // zeroed on allocation; combiners reset their slot
    D.kq_cnt.ensure((size_t)L * DecCtx::kMaxSub * 4 * h->H() * 8);   // zeroed on allocation, monotonic
    D.pids.ensure((size_t)rows * 4);
    D.logits.ensure((size_t)B * h->vocab_pad * 4);
    D.nchunk = lm_head_partials(h->dt, (int)d, h->d.vocab, h->lm_walkers);   // argmax partials per row of the LM head
    D.part_val.ensure((size_t)B * D.nchunk * 4);
    D.part_idx.ensure((size_t)B * D.nchunk * 4);
    D.ints.ensure(need[5]);
    D.outbuf.ensure(need[6]);
  }
}

// token log-probs: the scored decode's buffers of context D for B rows of out_ld columns (partials sized
// with D.nchunk, like part_val); a reallocation drains the streams and drops the context's graphs
void ensure_lp_ws(wcb_handle* h, DecCtx& D, int B, int out_ld) {
  const size_t np = (size_t)std::max(B, D.dec_B) * D.nchunk * 4, nl = (size_t)B * out_ld * 4;
  if (np <= D.part_max.bytes && np <= D.part_sum.bytes && nl <= D.lpbuf.bytes) return;
  quiesce(h);
  if (D.part_max.p || D.lpbuf.p) D.drop_graphs();   // (the first allocation frees nothing a graph could hold)
  D.part_max.ensure(np);
  D.part_sum.ensure(np);
  D.lpbuf.ensure(nl);
}

// cross-attention K/V of every decoder layer from the encoder output (A4), once per clip:
// one GEMM [B·1500, d] × [2·L·d, d]ᵀ written head-split as [L·2][B][H][1500][64]
void cross_kv(wcb_handle* h, int B, int buf, const void* enc) {
  const int d = h->d.d_model, S = h->S(), L = h->d.n_layers;
  GemmArgs g = rowgemm(enc, d, h->xkv_w, B * S, 2 * L * d, d, h->xkv2[buf].p, 0);
  g.bias = h->xkv_b; g.mode = 1; g.hs_S = S; g.hs_H = h->H(); g.hs_B = B;
  run_gemm(h, "xkv_gemm", g);
}

// the encoder-space decode's encoder output (xmode 1) in decode buffer `buf` from the row layout
// [B][S][d] (fragment-major chunk layout when xenc_fm applies: the layout the register-ring kernel
// streams), on stream st
bool xenc_fm_on(const wcb_handle* h) { return h->xenc_fm && (h->xenc_variant == 1 || h->xenc_variant == 2); }
void fill_xenc(wcb_handle* h, int buf, const void* src, int B, hipStream_t st) {
  if (xenc_fm_on(h)) {
    h->timed("xenc_layout", 0, 2.0 * B * h->S() * h->d.d_model * esize(h->d.dtype), st,
             [&] { xenc_to_fm(h->dt, src, h->xkv2[buf].p, B, h->S(), h->d.d_model, st); });
  } else if (src != h->xkv2[buf].p) {
    HIPCHK(hipMemcpyAsync(h->xkv2[buf].p, src, (size_t)B * h->S() * h->d.d_model * esize(h->d.dtype),
                          hipMemcpyDeviceToDevice, st));
  }
}

// Encoder state into decode context `buf` from the encoder output `enc` ([B][1500][d]: the caller's, or the encoder
// run just done): the copy the encoder-space kernel streams (xm 1, on st) or the cross-K/V GEMM (xm 0, always on the
// encoder stream). st = the encoder stream (a pipelined context, whose ev_dec[buf] it already waits for): ev_xkv[buf]
// is recorded for the decode stream. st = the step-wise context's own stream, which no event orders after the GEMM:
// that waits for the caller's stream, and the encoder stream is drained.
void enc_to_ctx(wcb_handle* h, int buf, const void* enc, int B, int xm, hipStream_t st, void* caller_stream) {
  const bool piped = st == h->he;
  if (xm == 1) {
    fill_xenc(h, buf, enc, B, st);
  } else {
    if (!piped) sync_in(h, caller_stream, h->he);
    cross_kv(h, B, buf, enc);
    if (!piped) HIPCHK(hipStreamSynchronize(h->he));
  }
  if (piped) HIPCHK(hipEventRecord(h->ev_xkv[buf], h->he));
}

struct StepCfg {
  int B = 0, T = 0, out_ld = 0, buf = 0;   // B: decoder rows (clips x beams); buf: which cross-K/V buffer the step reads
  bool lm_head = false, select = false;
  float* logits_out = nullptr; long logits_ld = 0;   // LM head destination
  const wcb_bias* bias = nullptr; float lam = 0.f; int min_new = 0;
  const int* forced = nullptr; int forced_ld = 0;    // advance_forced source when !select
  int clips = 0, nb = 1;               // encoder outputs (0: B) and decoder rows per encoder output
  int xmode = 1;                       // cross-attention formulation of this call (wcb_handle::xmode)
  int host_pos = -1;                   // decoder position of this step when known on the host (eager)
  const int* phys = nullptr;           // beam search: cache row of every key position [B][T]
  const BeamArgs* beam = nullptr;      // beam search selection (replaces the greedy select)
  int rps = 1;                         // positions per decoder row in this pass (> 1: causal prefill)
  float* score_out = nullptr;          // greedy select: the chosen token's (boosted) logit per row (step-wise API)
  // greedy: the step's input embedding was written by the previous step's select_finalize (or by
  // step_embed before the first step), and this step's finalize writes the next one
  bool embedded = false;
  const ForestDev* forest = nullptr;   // per-utterance bias lists (bias = the empty automaton then: zero root bitmap)
  // greedy select, token log-probs: [B][out_ld] f32 beside the ids (the context's lpbuf; ensure_lp_ws) — the LM
  // head then also writes its softmax partials and the finalize merges them. Null: the step as it always was
  float* logprob_out = nullptr;
  // greedy select, temperature sampling: the context's samp words (inv_T, then the seed of every row). Null:
  // the step as it always was
  const uint64_t* samp = nullptr;
  // greedy select, token rules (the handle's; null / off: the step as it always was): the deny bitmaps of the LM
  // head and the finalize, the timestamp grammar of the finalize (row state: two ints per row behind rowbase)
  const uint32_t* deny = nullptr; const uint32_t* deny0 = nullptr;
  TsRule ts;
  // token timestamps: a teacher-forced pass (rps > 1, all rows in one chain) also captures the cross-attention
  // weights of the selected heads. Null: the pass as it always was
  const struct AlignPass* align = nullptr;
  // greedy, ragged prompts: the slot offset of every row (the context's poff) — the self-attention windows and the
  // position embeddings shift by it. Null: the step as it always was
  const int* pos_off = nullptr;
  // greedy select with token log-probs: the first step also writes every row's no-speech probability here (the
  // context's nsp). Null: the step as it always was
  float* nsp_out = nullptr;
  // greedy select, repeat rules (start_repeat; seen null: the step as it always was): the LM head reads the seen
  // bitmap, the finalize is the REP instantiation
  RepArgs rep;
};

// the capture of one teacher-forced pass of wcb_align: per layer the selected (head, slot in the list) pairs; the
// pass carries positions pos0 .. of every clip, alignment row i = position - P, clips [clip0, clip0 + nclip) kept
struct AlignPass {
  std::vector<std::vector<std::pair<int, int>>> by_layer;
  int heads_total = 0, last_layer = 0;
  int P = 1, nrow = 0, pos0 = 0, clip0 = 0, nclip = 0;
  float* w = nullptr;   // [nclip][heads_total][nrow][S]
};

// what every pass over `rows` decoder rows in context buf starts from: the context's logits rows as the LM head's
// destination, no bias list, the handle's cross-attention formulation; the caller names the rest
StepCfg step_cfg(wcb_handle* h, int buf, int rows, int T, int out_ld) {
  StepCfg c;
  c.B = rows; c.T = T; c.out_ld = out_ld; c.buf = buf;
  c.logits_out = h->dc[buf].logits.as<float>(); c.logits_ld = h->vocab_pad;
  c.bias = h->empty_bias.get();
  c.xmode = h->xmode;
  return c;
}

// the bias automaton a selection walks into its arguments (SelectArgs / BeamArgs): the shared one, then — per-utterance
// lists — the forest's state space in its place, the clip's root children per row (the root bitmap stays bs's)
template <typename Args>
void set_automaton(Args& a, const wcb_bias* bs, const ForestDev* F) {
  a.root_bits = bs->root_bits.as<uint32_t>(); a.root_child = bs->root_child.as<int>();
  a.trans_off = bs->trans_off.as<int>(); a.trans_tok = bs->trans_tok.as<int>(); a.trans_dst = bs->trans_dst.as<int>();
  a.st_depth = bs->st_depth.as<int>(); a.st_keep = bs->st_keep.as<int>();
  if (!F) return;
  a.trans_off = F->trans_off; a.trans_tok = F->trans_tok; a.trans_dst = F->trans_dst;
  a.st_depth = F->st_depth; a.st_keep = F->st_keep; a.forest = F->f;
}

// the handle's token rules into a greedy step configuration
void apply_rules(const wcb_handle* h, StepCfg& c) {
  if (!h->rules_on) return;
  c.deny = h->rules_deny.as<uint32_t>();
  c.deny0 = h->rules_has0 ? h->rules_deny0.as<uint32_t>() : nullptr;
  c.ts = h->rules_ts;
}

// the residual's fragment-major copy applies (lean path): the lean LayerNorm table covers d, every
// LN consumer and residual writer has its weights' fragment-major copy, and the decode GEMMs publish
// no 16-column LayerNorm partials (the lean kernel writes none)
bool xfm_possible(const wcb_handle* h) {
  const int d = h->d.d_model;
  if (!h->lean || !h->lean_x || h->dt == kF32 || !h->ln16 || !h->dec_gemm) return false;
  if (d != 512 && d != 768 && d != 1024 && d != 1280) return false;
  for (const LayerW& w : h->dec)
    if (!w.qkv_fm || !w.o_fm || !w.xq_fm || !w.xo_fm || !w.fc1_fm || !w.fc2_fm) return false;
  return true;
}

// the folded LayerNorm of the > 64-row projections is available (16-bit, d a multiple of 32)
bool lnf_possible(const wcb_handle* h) {
  return h->ln_fold && h->dt != kF32 && h->d.d_model % 32 == 0 && h->d.d_model <= kLnfMaxK;
}

// wcb_align's capture after the cross query of layer l: q = the layer's cross query rows (xmode 0: q [M][d]) or
// their encoder-space form (xmode 1: q' [M][H·d]); the keys are the context's cross-K of the layer or its encoder
// output, whichever layout the decode reads
void align_hook(wcb_handle* h, const StepCfg& c, int l, const void* q, int rps, hipStream_t st_) {
  const AlignPass& ap = *c.align;
  const auto& hl = ap.by_layer[l];
  if (hl.empty()) return;
  const int d = h->d.d_model, S = h->S(), H = h->H(), clips = c.clips ? c.clips : c.B;
  const size_t e = esize(h->d.dtype);
  AlignCapArgs a;
  a.q = q; a.xmode = c.xmode; a.S = S;
  if (c.xmode == 1) {
    a.ldq = (long)H * d; a.q_hstride = d; a.dim = d;
    a.k = h->xkv2[c.buf].p; a.fm = xenc_fm_on(h);
    a.k_clip = a.fm ? xenc_fm_elems(1, S, d) : (long)S * d;
  } else {
    a.ldq = d; a.q_hstride = 64; a.dim = 64;
    a.k = (const char*)h->xkv2[c.buf].p + (size_t)l * 2 * clips * H * S * 64 * e;
    a.k_clip = (long)H * S * 64;
  }
  a.rps = rps; a.pos0 = ap.pos0; a.P = ap.P; a.nrow = ap.nrow; a.clip0 = ap.clip0; a.nclip = ap.nclip;
  a.nh = (int)hl.size(); a.heads_total = ap.heads_total;
  for (int i = 0; i < a.nh; ++i) { a.head[i] = hl[i].first; a.slot[i] = hl[i].second; }
  a.w = ap.w;
  h->timed("align_capture", 2.0 * ap.nclip * rps * a.nh * (double)S * a.dim,
           (double)ap.nclip * rps * a.nh * S * 4.0, st_, [&] { align_capture(h->dt, a, st_); });
}

// Decoder layers + LM head for rows [b0, b0 + nb) of the batch on stream `st_`: WhisperDecoder.forward
// with a KV cache ([tf] modeling_whisper.py:690-795). Every position-dependent quantity is read on
// the device, so the launch sequence replays as a hipGraph. Row-indexed buffers are addressed with
// the row offset; the KV caches keep the full-batch layout ([kv][B][H][T][64]).
void decode_rows(wcb_handle* h, const StepCfg& c, int b0, int nb, int chain, hipStream_t st_) {
  DecCtx& D = h->dc[c.buf];
  const int d = h->d.d_model, S = h->S(), H = h->H(), L = h->d.n_layers, B = c.B, T = c.T;
  const size_t e = esize(h->d.dtype);
  int* ints = D.ints.as<int>();
  int* pos = ints + I_POS;
  // prefill (c.rps > 1): every decoder row carries rps consecutive positions, rows (row, position)
  // row-major; b0 / nb count decoder rows (KV-cache rows), r0 / M activation rows
  const int rps = c.rps > 1 ? c.rps : 1, r0 = b0 * rps, M = nb * rps;
  float* x = D.dx.as<float>() + (size_t)r0 * d;
  char* x16 = (char*)D.dx16.p + (size_t)r0 * d * e;       // T copy of x: the LN-fused A operand
  const void* lna = h->ln16 ? x16 : nullptr;
  const int nbk = d / 16;
  float* st = D.dstats.as<float>() + (size_t)r0 * nbk * 2;
  float* st_pub = h->dec_gemm ? nullptr : st;   // LN partial sums only for the older skinny consumers
  // > 64 rows, 16-bit, decode GEMMs supported: every residual writer is a ring tile that publishes
  // per-32-column (Σx, Σx²) of its rows (and the embedding does), so the LN consumers fold the
  // LayerNorm into their tiles (ln_fold) instead of a LayerNorm launch each
  float* rst = D.drst.as<float>() + (size_t)r0 * (d / 32) * 2;
  char* dq = (char*)D.dq.p + (size_t)r0 * d * e;
  char* datt = (char*)D.datt.p + (size_t)r0 * d * e;
  char* dffn = (char*)D.dffn.p + (size_t)r0 * h->d.ffn * e;
  // More than 64 activation rows (beam rows, prefill passes): a LayerNorm launch into dh, then the
  // MFMA tile GEMM — each weight tile read once per 128 rows, where the row-block decode kernel reads
  // the weights once per 16-32 rows. Grouped (block-diagonal) products stay on the decode kernel.
  // Only where the tile grid is wide enough to stream the weights from many CUs: the LM head, and the
  // N >= 2048 projections (QKV, fc1) at >= 192 rows (C3: 320 beam rows); the d-wide projections keep
  // the decode kernel (and keep writing the 16-bit residual copy its LayerNorm consumers read).
  const bool tiled = M > 64;
  const bool lnf_ok = tiled && h->dec_gemm && lnf_possible(h);
  // fragment-major operands (lean path): this chain's rows start a 16-row block of the copies
  const bool fm_ok = !tiled && h->lean && h->dt != kF32 && lna && r0 % 16 == 0 && M <= 64;
  // the residual's fragment-major copy (written by the embedding and every residual writer, read by
  // the LayerNorm-fused projections); decode_step's and prefill_step's embeddings write it for every
  // row whenever xfm_possible
  // (one position per row: the lean QKV appends one key per row)
  char* x16fm = fm_ok && rps == 1 && xfm_possible(h) ? (char*)D.dx16fm.p + (size_t)r0 * d * e : nullptr;
  char* dh = (char*)D.dh.p + (size_t)r0 * d * e;
  int cur_l = 0;   // the layer being issued (the lean launches' stamp slot)
  Stamp lst;
  auto proj = [&](const char* cls, GemmArgs g) {
    const bool lm = g.W == h->tok_emb;
    // > 64 rows, 16-bit: every non-grouped projection on the 32/64-row LDS-ring tiles (tile 2; C5's
    // 80 beam rows: 0.5 TB/s of weights on the row-block decode kernel, which holds A in registers
    // and re-reads the weights per 32 rows)
    const bool ring = h->dt != kF32 && !lm && !g.st_out;
    if (tiled && !g.a_grp_n && (lm || ring || (M >= 192 && g.N >= 2048))) {
      if (g.ln_w && ring && g.ln_u && g.ln_wg && lnf_ok && lna) {   // LayerNorm folded into the ring tiles
        g.A = lna; g.lda = d; g.W = g.ln_wg; g.ldw = g.K; g.W_fm = g.ln_wg_fm;
        g.bias = g.ln_c; g.ln_w = g.ln_b = nullptr; g.st_in = nullptr; g.ln_a16 = nullptr;
        g.rst_in = rst; g.rst_nb = d / 32;
      } else if (g.ln_w) {
        g.W_fm = nullptr;
        g.ln_u = nullptr;
        const float* xa = static_cast<const float*>(g.A);
        h->timed("dec_ln", 0, (double)M * d * (4.0 + e), st_,
                 [&] { layernorm(h->dt, xa, g.ln_w, g.ln_b, dh, M, d, st_); });
        g.A = dh; g.lda = d;
        g.ln_w = g.ln_b = nullptr; g.st_in = nullptr; g.ln_a16 = nullptr;
      }
      g.tile = ring ? 2 : 1; g.skinny = 0; g.ring_kt = h->ring_kt;
      if (ring && g.resid && g.out16 && lnf_ok) g.rst_out = rst;   // residual writer: stats for the next LN
      // <= 96 beam rows (C5's 80), K = d_model, fragment-major weights at hand: the wide single-burst
      // tiles for out / xo / xq (16 x 32) and fc1 (32 x 32); QKV keeps the ring (tools/beam_gemm_bench.py)
      g.a_fm = 0; g.c_fm = 0; g.out16_fm = nullptr;
      if (ring && h->beam_wide && M <= 96 && g.K == d && g.W_fm && !g.kv_out) {
        const std::string cn = cls;
        if (cn == "dec_out" || cn == "dec_xo" || cn == "dec_xq") g.wide = 12;
        else if (cn == "dec_fc1") g.wide = 22;
      }
      if (!g.wide && !h->beam_wfm) g.W_fm = nullptr;
      if (ring) g.raster = h->beam_raster;
    } else {
      g.lean = h->lean;   // <= 64 rows: the lean single-tile kernel where it covers the launch
      g.lean_fold = h->lean_fold && g.ln_w && g.ln_wg_fm && g.ln_u && g.ln_c;
      g.lean_mf2 = h->lean_mf2;
      const int region = h->prof_stamps ? lean_stamp_region(cls) : 0;
      if (region) {   // stamps pass: this launch's start / end inside the replayed graph
        lst.base = h->stamp_base(c.buf, region);
        lst.pos = pos; lst.stride = L * wcb_handle::kMaxSub; lst.idx = cur_l * wcb_handle::kMaxSub + chain;
        g.lstamp = &lst;
      }
    }
    dgemm(h, cls, g, st_);
  };
  const size_t cache_l = 2 * (size_t)B * H * T * 64;   // elements per layer (K then V)
  const int clips = c.clips ? c.clips : B;
  const size_t xkv_l = 2 * (size_t)clips * H * S * 64;
  for (int l = 0; l < L; ++l) {
    cur_l = l;
    const LayerW& w = h->dec[l];
    char* cache = (char*)D.kvself.p + (l * cache_l + (size_t)b0 * H * T * 64) * e;
    GemmArgs q = drow(x, d, w.qkv_w, M, 3 * d, d, dq, d);    // LayerNorm fused (f32 A rows)
    q.ln_w = w.ln1_w; q.ln_b = w.ln1_b; q.st_in = st; q.st_nb = nbk; q.ln_a16 = lna;
    q.bias = w.qkv_b; q.mode = 2; q.n_split = d; q.kv_out = cache; q.hs_B = B; q.hs_H = H; q.kv_T = T; q.pos = pos;
    q.kv_rps = rps; q.ln_u = w.ln1_u; q.ln_c = w.ln1_c; q.ln_wg = w.qkv_wg; q.W_fm = w.qkv_fm; q.ln_wg_fm = w.qkv_wgfm;
    if (x16fm) { q.ln_a16 = x16fm; q.a_fm = 1; }
    proj("dec_qkv", q);
    AttnArgs a;
    a.q = dq; a.ldq = d; a.q_Sb = rps; a.Sq = rps; a.causal = rps > 1;
    const char* cache0 = (char*)D.kvself.p + l * cache_l * e;   // K/V rows addressed absolutely
    a.k = cache0; a.v = cache0 + (size_t)B * H * T * 64 * e;
    a.k_sb = (long)H * T * 64; a.k_sh = (long)T * 64; a.k_sk = 64;
    a.row0 = b0; a.phys = c.phys; a.phys_ld = T;
    a.o = datt; a.ldo = d; a.o_Sb = rps; a.B = nb; a.H = H; a.nkeys_dev = pos; a.nkeys_add = 1;
    a.kv_rows = rps == 1 ? T : 0;
    a.key_start = c.pos_off;   // ragged prompts: row b0 + b attends from its own first slot (null: every key)
    {
      const double t_keys = c.host_pos >= 0 ? c.host_pos + 1 : 0;   // keys this step (eager pass)
      h->timed("dec_self_attn", 4.0 * nb * H * t_keys * 64, nb * H * t_keys * 128.0 * e, st_,
               [&] { attention_decode(h->dt, a, st_); });
    }
    GemmArgs o = drow(datt, d, w.o_w, M, d, d, x, d);
    o.bias = w.o_b; o.resid = x; o.out_f32 = 1; o.st_out = st_pub; o.st_nb = nbk; o.out16 = x16; o.W_fm = w.o_fm;
    o.out16_fm = x16fm;
    proj("dec_out", o);
    if (c.xmode == 1) {
      // cross attention in encoder space: q'_h = W_k,hᵀ q_h (block-diagonal GEMM, K = 64), one pass
      // over the encoder output per layer for all heads, range combine + W_v,h + b_v
      char* dqp = (char*)D.dqp.p + (size_t)r0 * H * d * e;
      GemmArgs xq = drow(x, d, w.xq_w, M, d, d, dq, d);
      xq.ln_w = w.lnx_w; xq.ln_b = w.lnx_b; xq.st_in = st; xq.st_nb = nbk; xq.ln_a16 = lna;
      xq.bias = w.xq_b; xq.ln_u = w.lnx_u; xq.ln_c = w.lnx_c; xq.ln_wg = w.xq_wg; xq.W_fm = w.xq_fm; xq.ln_wg_fm = w.xq_wgfm;
      if (x16fm) { xq.ln_a16 = x16fm; xq.a_fm = 1; }
      // q'_h = W_k,hᵀ q_h in the q_proj launch: the lean LN table's widths, both fragment-major copies
      const bool kqf = h->xq_kq && h->lean && fm_ok && w.xq_fm && w.xkt_fm && (d == 512 || d == 768 || d == 1024 || d == 1280);
      if (kqf) {
        xq.kq_w = w.xkt_fm; xq.kq_out = dqp; xq.kq_ld = (long)H * d; xq.hs_H = H;
        xq.kq_cnt = D.kq_cnt.as<unsigned long long>() + ((size_t)l * DecCtx::kMaxSub + chain) * 4 * H;
        xq.kq_err = h->dev_err.as<int>();
      }
      // q_h and q'_h in one launch without a hand-off (option xqk; the folded q_proj weights)
      const bool xqk = !kqf && h->xqk && h->lean && fm_ok && h->lean_fold && w.xq_wgfm && w.xkt_fm && w.lnx_u &&
                       H * 64 == d && (d == 512 || d == 768 || d == 1024 || d == 1280);
      if (xqk) { xq.xqk_wk = w.xkt_fm; xq.xqk_out = dqp; xq.hs_H = H; xq.xqk_nch = h->xqk_nch; }
      proj("dec_xq", xq);
      if (!kqf && !xqk) {
        GemmArgs kq = drow(dq, d, w.xkt_w, M, H * d, 64, dqp, (long)H * d);
        kq.a_grp_n = d; kq.a_grp_off = 64; kq.W_fm = w.xkt_fm;
        proj("dec_kq", kq);
      }
      if (c.align) {
        align_hook(h, c, l, dqp, rps, st_);
        if (l == c.align->last_layer) break;   // nothing past the last selected layer's query is read
      }
      XencArgs xa;
      xa.fm = xenc_fm_on(h);
      xa.enc = h->xkv2[c.buf].p; xa.enc_sb = xa.fm ? xenc_fm_elems(1, S, d) : (long)S * d;
      xa.row0 = r0; xa.rows_per_enc = c.nb * rps;   // beams (and prefill positions) of a clip share its encoder output
      xa.qp = dqp; xa.rows = M; xa.H = H; xa.D = d; xa.S = S; xa.nsplit = h->xenc_split;
      xa.variant = h->xenc_variant;
      xa.part = D.xpart.as<float>() + (size_t)r0 * h->xenc_split * H * d;
      xa.ml = D.xml.as<float>() + (size_t)r0 * h->xenc_split * H * 2;
      const bool fused_merge = h->merge_v && d % 128 == 0;
      xa.part16 = h->xpart16 && xa.fm && fused_merge;
      xa.merge_os = h->merge_os;
      if (h->prof_stamps) {
        xa.stamp.base = h->stamp_base(c.buf, 0);
        xa.stamp.pos = pos;
        xa.stamp.stride = L * wcb_handle::kMaxSub; xa.stamp.idx = l * wcb_handle::kMaxSub + chain;
      }
      // algorithmic bytes: every distinct clip's encoder output once (beams of a clip share it)
      h->timed("dec_xattn", 4.0 * M * H * (double)S * d, (double)nb / c.nb * S * d * e, st_,
               [&] { xenc_attention(h->dt, xa, st_); });
      if (fused_merge) {   // range merge + o_h = W_v,h u_h + b_v,h in one launch
        h->timed("dec_xmerge", 0, (double)M * H * d * h->xenc_split * (xa.part16 ? e : 4.0) + (double)d * d * e, st_,
                 [&] { xenc_merge_v(h->dt, xa, w.xv_w, w.xv_b, datt, d, st_, w.xv_fm); });
      } else {
        char* du = (char*)D.du.p + (size_t)r0 * H * d * e;
        h->timed("dec_xmerge", 0, (double)M * H * d * (h->xenc_split * 4.0 + e), st_,
                 [&] { xenc_merge(h->dt, xa, du, (long)H * d, st_); });
        GemmArgs vg = drow(du, (long)H * d, w.xv_w, M, d, d, datt, d);    // o_h = W_v,h u_h + b_v,h
        vg.a_grp_n = 64; vg.a_grp_off = d; vg.bias = w.xv_b;
        proj("dec_vg", vg);
      }
    } else {
      // cross attention over the precomputed encoder K/V
      GemmArgs xq = drow(x, d, w.xq_w, M, d, d, dq, d);
      xq.ln_w = w.lnx_w; xq.ln_b = w.lnx_b; xq.st_in = st; xq.st_nb = nbk; xq.ln_a16 = lna;
      xq.bias = w.xq_b; xq.ln_u = w.lnx_u; xq.ln_c = w.lnx_c; xq.ln_wg = w.xq_wg; xq.W_fm = w.xq_fm; xq.ln_wg_fm = w.xq_wgfm;
      if (x16fm) { xq.ln_a16 = x16fm; xq.a_fm = 1; }
      proj("dec_xq", xq);
      if (c.align) {
        align_hook(h, c, l, dq, rps, st_);
        if (l == c.align->last_layer) break;
      }
      AttnArgs xa;
      const char* xkv = (const char*)h->xkv2[c.buf].p + l * xkv_l * e;
      xa.q = dq; xa.ldq = d; xa.q_Sb = 1; xa.Sq = 1;
      xa.k = xkv; xa.v = xkv + (size_t)clips * H * S * 64 * e;
      xa.row0 = r0; xa.b_div = c.nb * rps;     // beams (and prefill positions) of a clip share its cross K/V
      xa.k_sb = (long)H * S * 64; xa.k_sh = (long)S * 64; xa.k_sk = 64;
      xa.o = datt; xa.ldo = d; xa.o_Sb = 1; xa.B = M; xa.H = H; xa.nkeys = S;
      xa.nsplit = h->xsplit; xa.part = D.xpart.as<float>() + (size_t)r0 * H * kXSplit * 66;
      xa.ticket = D.xticket.as<int>() + (size_t)r0 * H;
      xa.variant = h->xvariant;   // fixed per handle: the same clip decodes alike in any batch
      if (h->prof_stamps) {
        xa.stamp.base = h->stamp_base(c.buf, 0);
        xa.stamp.pos = pos;
        xa.stamp.stride = L * wcb_handle::kMaxSub; xa.stamp.idx = l * wcb_handle::kMaxSub + chain;
      }
      // 16-bit, several rows per clip (beams, prefill positions), row group aligned to clips: the
      // MFMA flash kernel over (clip, head) blocks — each clip's K/V streamed once for all of its rows
      // (the per-row kernels re-read it once per beam). Chosen from the dtype and the decode shape,
      // never from the batch size.
      const int G = c.nb * rps;
      const bool grouped = h->dt != kF32 && G > 1 && r0 % G == 0 && M % G == 0;
      if (grouped) {
        xa.k = xkv + (size_t)(r0 / G) * xa.k_sb * e;
        xa.v = (const char*)xa.v + (size_t)(r0 / G) * xa.k_sb * e;
        xa.q_Sb = G; xa.Sq = G; xa.o_Sb = G; xa.B = M / G; xa.row0 = 0; xa.b_div = 1;
        xa.nsplit = h->flash_split; xa.ticket = nullptr;
        xa.part = D.xpart.as<float>() + (size_t)r0 * H * kXSplit * 66;
        if (h->beam_xattn && G <= 16) xa.variant = 6 + h->beam_xattn;   // keys split over the waves (attn_beam_kernel)
      }
      h->timed("dec_xattn", 4.0 * M * H * (double)S * 64, (double)nb / c.nb * H * S * 128.0 * e, st_, [&] {
        if (!grouped || !attention_flash(h->dt, xa, st_)) attention_decode(h->dt, xa, st_);
      });
    }
    GemmArgs xo = drow(datt, d, w.xo_w, M, d, d, x, d);
    xo.bias = w.xo_b; xo.resid = x; xo.out_f32 = 1; xo.st_out = st_pub; xo.st_nb = nbk; xo.out16 = x16; xo.W_fm = w.xo_fm;
    xo.out16_fm = x16fm;
    proj("dec_xo", xo);
    // MLP. Lean path (<= 64 rows, 16-bit): fc1 writes its output fragment-major in the layout fc2's
    // split of K = ffn reads (every A wave-instruction of fc2 then reads 1 KiB contiguous: its 98 KB of
    // activations per workgroup at d = 768 were the largest operand of the decode step)
    const bool afm = fm_ok && w.fc1_fm && w.fc2_fm &&
                     (d == 512 || d == 768 || d == 1024 || d == 1280) &&
                     (h->d.ffn == 2048 || h->d.ffn == 3072 || h->d.ffn == 4096 || h->d.ffn == 5120);
    GemmArgs f1 = drow(x, d, w.fc1_w, M, h->d.ffn, d, dffn, h->d.ffn);
    f1.ln_w = w.ln2_w; f1.ln_b = w.ln2_b; f1.st_in = st; f1.st_nb = nbk; f1.ln_a16 = lna;
    f1.bias = w.fc1_b; f1.act = 1; f1.ln_u = w.ln2_u; f1.ln_c = w.ln2_c; f1.ln_wg = w.fc1_wg; f1.W_fm = w.fc1_fm; f1.ln_wg_fm = w.fc1_wgfm;
    f1.c_fm = afm;
    if (x16fm) { f1.ln_a16 = x16fm; f1.a_fm = 1; }
    proj("dec_fc1", f1);
    GemmArgs f2 = drow(dffn, h->d.ffn, w.fc2_w, M, d, h->d.ffn, x, d);
    f2.bias = w.fc2_b; f2.resid = x; f2.out_f32 = 1; f2.st_out = st_pub; f2.st_nb = nbk; f2.out16 = x16; f2.W_fm = w.fc2_fm;
    f2.a_fm = afm;
    f2.out16_fm = x16fm;
    proj("dec_fc2", f2);
  }
  if (c.lm_head) {
    GemmArgs lm = drow(x, d, h->tok_emb, M, h->d.vocab, d, c.logits_out + (size_t)b0 * c.logits_ld, c.logits_ld);
    if (rps > 1) { lm.ldc = h->d.vocab; lm.c_Mb = rps; lm.c_strideB = c.logits_ld; }   // row (b, t) → b·ld + t·V
    // tile path: all vocab_pad columns (zero rows past V) into a logits buffer of that row stride
    const bool lm_tiled = tiled && rps == 1 && c.logits_ld >= h->vocab_pad;
    if (lm_tiled) lm.N = h->vocab_pad;
    lm.ln_w = h->dec_ln_w; lm.ln_b = h->dec_ln_b; lm.st_in = st; lm.st_nb = nbk; lm.ln_a16 = lna;
    if (h->lean) lm.W_fm = h->tok_emb_fm;
    if (h->lean && !tiled && rps == 1 && h->lm_ln_split) lm.ln_scratch = dh;   // the final LayerNorm in a launch of its own
    lm.out_f32 = 1;
    if (c.select && !c.beam) {   // argmax partials with the root boost + EOS mask fused into the LM head
      lm.walkers = h->lm_walkers;
      lm.sel_val = D.part_val.as<float>() + (size_t)b0 * D.nchunk;
      lm.sel_idx = D.part_idx.as<int>() + (size_t)b0 * D.nchunk;
      lm.sel_root_bits = c.bias->root_bits.as<uint32_t>(); lm.sel_lam = c.lam;
      lm.sel_rowbase = RowInts(D, c.B).rowbase + b0;   // per row k - d of its state (select_finalize)
      lm.sel_eos = h->d.eos_token_id; lm.sel_step = ints + I_STEP; lm.sel_min_new = c.min_new;
      if (c.logprob_out) {   // token log-probs: the softmax partials of the raw logits beside the argmax ones
        lm.sel_max = D.part_max.as<float>() + (size_t)b0 * D.nchunk;
        lm.sel_sum = D.part_sum.as<float>() + (size_t)b0 * D.nchunk;
      }
      if (c.samp) {   // temperature sampling: the sampled LM head compares perturbed scores
        lm.sel_inv_t = reinterpret_cast<const float*>(c.samp);
        lm.sel_seeds = c.samp + 1 + b0;
      }
      lm.sel_deny = c.deny; lm.sel_deny0 = c.deny0;   // token rules (null: none)
      if (c.rep.seen) { lm.sel_seen = c.rep.seen + (size_t)b0 * c.rep.words; lm.sel_seen_w = c.rep.words; }   // repeat rules
    }
    if (lm_tiled) {
      proj("lm_head", lm);
    } else {
      dgemm(h, "lm_head", lm, st_);
    }
  }
}

// One decode step for the whole batch: embedding, then the batch split into `h->n_sub` row groups
// whose layer chains run on separate streams (fork/join events, captured into the same graph) so
// the latency-bound projections of one group overlap the HBM-bound cross-attention of another;
// token selection (or teacher forcing) joins them.
// the decode step's input embedding (next_ids at the device position) into the residual rows, their
// 16-bit copies and LayerNorm partials
void step_embed(wcb_handle* h, const StepCfg& c) {
  DecCtx& D = h->dc[c.buf];
  const int d = h->d.d_model, B = c.B;
  int* ints = D.ints.as<int>();
  const bool r32 = h->dec_gemm && lnf_possible(h);   // 32-column stats for the folded LayerNorm (rows > 64)
  h->timed("dec_embed", 0, (double)B * d * (2.0 * esize(h->d.dtype) + 4), D.hs, [&] {
    embed(h->dt, h->tok_emb, h->dec_pos, RowInts(D, B).next, ints + I_POS, D.dx.as<float>(),
          !h->dec_gemm ? D.dstats.as<float>() : r32 ? D.drst.as<float>() : nullptr, B, d, D.hs, D.dx16.p, h->d.vocab, 1,
          r32 ? 32 : 16, xfm_possible(h) ? D.dx16fm.p : nullptr, c.pos_off, h->d.n_text_ctx);
  });
}

void decode_step(wcb_handle* h, const StepCfg& c) {
  DecCtx& D = h->dc[c.buf];
  const int d = h->d.d_model, B = c.B;
  int* ints = D.ints.as<int>();
  int* pos = ints + I_POS;
  const RowInts ri(D, B);
  if (!c.embedded) step_embed(h, c);
  // rows per chain: the skinny projections split rows over grid.y, so a chain can take any number
  // of rows (WCB_GROUP_ROWS; more chains overlap latency, fewer re-read the weights less often)
  const int ngrp = (B + h->group_rows - 1) / h->group_rows;
  const int ns = std::max(ngrp, std::max(1, std::min(h->n_sub, B)));
  if (ns == 1 || !D.sub[0]) {        // one stream: row groups back to back
    for (int i = 0; i < ns; ++i) {
      const int b0 = (int)((long)B * i / ns), b1 = (int)((long)B * (i + 1) / ns);
      decode_rows(h, c, b0, b1 - b0, i, D.hs);
    }
  } else {
    HIPCHK(hipEventRecord(D.ev_fork, D.hs));
    for (int i = 0; i < ns; ++i) {
      const int b0 = (int)((long)B * i / ns), b1 = (int)((long)B * (i + 1) / ns);
      HIPCHK(hipStreamWaitEvent(D.sub[i], D.ev_fork, 0));
      decode_rows(h, c, b0, b1 - b0, i, D.sub[i]);
      HIPCHK(hipEventRecord(D.ev_join[i], D.sub[i]));
    }
    for (int i = 0; i < ns; ++i) HIPCHK(hipStreamWaitEvent(D.hs, D.ev_join[i], 0));
  }
  if (c.select && c.beam) {
    h->timed("dec_select", 0, (double)B * h->d.vocab * 4, D.hs, [&] { beam_select(*c.beam, D.hs); });
  } else if (c.select) {
    SelectArgs s;
    s.logits = c.logits_out; s.ld = c.logits_ld; s.M = B; s.V = h->d.vocab;
    s.lam = c.lam;
    set_automaton(s, c.bias, c.forest);
    s.state = ri.state; s.finished = ri.finished; s.rowbase = ri.rowbase;
    s.eos = h->d.eos_token_id; s.pad = h->d.pad_token_id; s.min_new = c.min_new;
    s.step = ints + I_STEP; s.pos = pos; s.next_ids = ri.next;
    s.out_ids = D.outbuf.as<int>(); s.out_ld = c.out_ld;
    s.part_val = D.part_val.as<float>(); s.part_idx = D.part_idx.as<int>(); s.nchunk = D.nchunk;
    s.all_done = ints + I_DONE;
    s.ticket_unfin = reinterpret_cast<unsigned long long*>(ints + I_TU);
    s.out_score = c.score_out;
    if (c.logprob_out) {
      s.part_max = D.part_max.as<float>(); s.part_sum = D.part_sum.as<float>(); s.out_logprob = c.logprob_out;
    }
    if (c.samp) { s.inv_t = reinterpret_cast<const float*>(c.samp); s.seeds = c.samp + 1; }
    s.deny = c.deny; s.deny0 = c.deny0; s.ts = c.ts; s.ts_state = ri.ts_state;
    s.rep = c.rep;
    if (c.nsp_out && c.logprob_out) { s.out_nsp = c.nsp_out; s.nsp_token = h->d.vocab - kTimestampTokens - 2; }
    if (c.embedded) {   // the next step's input embedding in the same launch (embed()'s outputs)
      const bool r32 = h->dec_gemm && lnf_possible(h);
      s.emb = h->tok_emb; s.pemb = h->dec_pos; s.n_pos = h->d.n_text_ctx; s.d = d; s.dtype = h->dt;
      s.pos_off = c.pos_off;
      s.x = D.dx.as<float>(); s.x16 = D.dx16.p;
      // (greedy decodes <= 64 rows: the decode-GEMM consumers compute their own LayerNorm statistics, so
      // the 32-column partials of the > 64-row folded path are not published; the older skinny consumers
      // still read 16-column ones)
      s.st = !h->dec_gemm ? D.dstats.as<float>() : nullptr; s.st_w = 16;
      (void)r32;
      int nw = 0, kpw = 0;
      if (xfm_possible(h) && lean_cfg(d, nw, kpw)) { s.x16fm = D.dx16fm.p; s.fm_nw = nw; s.fm_kpw = kpw; }
    }
    h->timed("dec_select", 0, (double)B * D.nchunk * 8, D.hs, [&] { select_finalize(s, D.hs); });
  } else {
    advance_forced(ri.next, c.forced, B, c.forced_ld, pos, D.hs);
  }
}

// Causal prefill of np positions (*pos .. *pos + np - 1) of every decoder row in ONE pass of the
// decoder (prompt tokens / teacher forcing): ids from src[row·ld + position] (ld 0: one prefix shared
// by every row), rows (row, position) row-major, the KV cache written at those positions, the
// self-attention causal over the cache, the cross-attention rows mapped to their clip; LM head on
// every row when c.lm_head. Advances *pos by np. Eager (its shapes change with np).
void prefill_step(wcb_handle* h, StepCfg c, int np, const int* src, int ld) {
  DecCtx& D = h->dc[c.buf];
  const int d = h->d.d_model, R = c.B, M = R * np;
  int* ints = D.ints.as<int>();
  int* pos = ints + I_POS;
  c.rps = np;
  c.select = false;
  c.phys = nullptr;   // prompt keys: every row's own cache row (beam_init's identity map)
  c.beam = nullptr;
  h->timed("dec_embed", 0, (double)M * d * (2.0 * esize(h->d.dtype) + 4), D.hs, [&] {
    prefill_ids(D.pids.as<int>(), src, R, np, ld, pos, D.hs);
    const bool r32 = h->dec_gemm && lnf_possible(h);
    embed(h->dt, h->tok_emb, h->dec_pos, D.pids.as<int>(), pos, D.dx.as<float>(), r32 ? D.drst.as<float>() : nullptr, M,
          d, D.hs, D.dx16.p, h->d.vocab, np, 32, xfm_possible(h) ? D.dx16fm.p : nullptr, c.pos_off, h->d.n_text_ctx);
  });
  decode_rows(h, c, 0, R, 0, D.hs);
  add_i32(pos, np, D.hs);
}

// Beam-search state of decode context D (utterances B, nb beams each, R = B·nb rows): one buffer carved
// into [R] running / finished scores, finished flags and lengths, [R][Lg] running and finished
// sequences, [R][Tc] key map, [R][K] per-row candidates, [B][2] utterance flags, [R] parent beams.
// ensure_beam_buf sizes it (draining the streams first when it grows); beam_args carves it.
constexpr int kBeamBufs = 12;
void beam_words(int B, int nb, int Lg, int Tc, size_t* w) {
  const size_t R = (size_t)B * nb, K = 2 * (size_t)nb;
  const size_t C = kBeamChunks;   // candidate lists per (row, vocabulary chunk); chunk (max, Σexp)
  const size_t v[kBeamBufs] = {R, R, R, R, R * Lg, R * Lg, R * Tc, R * C * K, R * C * K, (size_t)B * 2, R, R * C * 2};
  std::copy(v, v + kBeamBufs, w);
}
void ensure_beam_buf(wcb_handle* h, DecCtx& D, int B, int nb, int Lg, int Tc) {
  size_t w[kBeamBufs], bytes = 0;
  beam_words(B, nb, Lg, Tc, w);
  for (size_t x : w) bytes += (x * 4 + 255) / 256 * 256;
  if (bytes > D.beam.bytes) { quiesce(h); D.beam.ensure(bytes); }
}

// Per-utterance bias forest of a decode in context D: the host forest copied into the context's device
// buffer on its decode stream (after the previous decode of the context in stream order, so a replayed
// graph never sees a half-written forest), through a pinned staging copy the handle owns — the caller may
// destroy `bb` as soon as the call returns. Device layout (ints), fixed by the capacities so the captured
// graph's pointers stay valid from call to call:
//   root [64] | rc_off [128] | st_depth [ns] | st_keep [ns] | trans_off [ns + 64] | trans_tok [nt] |
//   trans_dst [nt] | rc_tok [nrc] | rc_dst [nrc]
// A forest above a capacity grows the buffer (quiesce + realloc, as ensure_beam_buf; the graph key names
// the capacities, so the next call re-captures).
constexpr int kForestClips = 64;
int forest_cap(size_t n, int floor_) {
  size_t c = (size_t)floor_;
  while (c < n) c *= 2;
  return (int)c;
}
ForestDev install_forest(wcb_handle* h, DecCtx& D, const wcb_bias_batch* bb) {
  const size_t ns = bb->st_depth.size(), nt = bb->trans_tok.size(), nrc = bb->rc_tok.size();
  REQUIRE(bb->B <= kForestClips, "bias batch: more than 64 clips");
  REQUIRE(ns + nt + nrc < ((size_t)1 << 28), "bias batch too large");
  if ((int)ns > D.f_ns || (int)nt > D.f_nt || (int)nrc > D.f_nrc || !D.forest.p) {
    const int cs = std::max(D.f_ns, forest_cap(ns, 4096)), ct = std::max(D.f_nt, forest_cap(nt, 4096)),
              cr = std::max(D.f_nrc, forest_cap(nrc, 1024));
    quiesce(h);
    D.forest.release();
    D.forest.ensure(((size_t)kForestClips + 128 + 3 * (size_t)cs + 64 + 2 * (size_t)ct + 2 * (size_t)cr) * 4);
    D.f_ns = cs; D.f_nt = ct; D.f_nrc = cr;
  }
  int* base = D.forest.as<int>();
  int* d_root = base;
  int* d_rcoff = d_root + kForestClips;
  int* d_depth = d_rcoff + 128;
  int* d_keep = d_depth + D.f_ns;
  int* d_toff = d_keep + D.f_ns;
  int* d_ttok = d_toff + D.f_ns + 64;
  int* d_tdst = d_ttok + D.f_nt;
  int* d_rctok = d_tdst + D.f_nt;
  int* d_rcdst = d_rctok + D.f_nrc;
  // staging: wait for the upload that last read it, then refill
  const std::vector<int>* src[9] = {&bb->root, &bb->rc_off, &bb->st_depth, &bb->st_keep, &bb->trans_off,
                                    &bb->trans_tok, &bb->trans_dst, &bb->rc_tok, &bb->rc_dst};
  int* dst[9] = {d_root, d_rcoff, d_depth, d_keep, d_toff, d_ttok, d_tdst, d_rctok, d_rcdst};
  size_t words = 0;
  for (auto* v : src) words += v->size();
  if (!D.ev_fcopy) HIPCHK(hipEventCreateWithFlags(&D.ev_fcopy, hipEventDisableTiming));
  if (D.f_copy_pending) { HIPCHK(hipEventSynchronize(D.ev_fcopy)); D.f_copy_pending = false; }
  if (words > D.f_stage_words) {
    if (D.f_stage) (void)hipHostFree(D.f_stage);
    D.f_stage = nullptr;
    D.f_stage_words = 0;
    const size_t cap = std::max<size_t>(words * 2, 1 << 14);
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&D.f_stage), cap * 4, hipHostMallocDefault));
    D.f_stage_words = cap;
  }
  size_t o = 0;
  for (int i = 0; i < 9; ++i) {
    const size_t n = src[i]->size();
    if (!n) continue;
    std::memcpy(D.f_stage + o, src[i]->data(), n * 4);
    HIPCHK(hipMemcpyAsync(dst[i], D.f_stage + o, n * 4, hipMemcpyHostToDevice, D.hs));
    o += n;
  }
  HIPCHK(hipEventRecord(D.ev_fcopy, D.hs));
  D.f_copy_pending = true;
  ForestDev F;
  F.f.root = d_root; F.f.rc_off = d_rcoff; F.f.rc_tok = d_rctok; F.f.rc_dst = d_rcdst;
  F.trans_off = d_toff; F.trans_tok = d_ttok; F.trans_dst = d_tdst; F.st_depth = d_depth; F.st_keep = d_keep;
  return F;
}

// Per-clip prompts of different lengths: clip b's P_b = plen[b] prompt tokens (the start token last)
// live in slots off_b = P − P_b .. P − 1 of the context's P-wide prompt rows (D.forced), the slots before them hold the
// pad token (whatever the caller's array has there), and off_b goes into D.poff. Both go up on the decode stream from
// pinned staging, so the caller's arrays are free on return (async_out included) and a replayed graph never sees half
// an upload. Returns whether any clip is shorter than P (false: the dense kernels decode the call). The lengths were
// checked by the caller.
constexpr int kPromptRows = 64;
bool install_prompts(wcb_handle* h, DecCtx& D, const int32_t* prompts, int P, const int32_t* plen, int B) {
  const size_t np = (size_t)B * P, words = np + kPromptRows;
  if (!D.ev_pcopy) HIPCHK(hipEventCreateWithFlags(&D.ev_pcopy, hipEventDisableTiming));
  if (D.p_copy_pending) { HIPCHK(hipEventSynchronize(D.ev_pcopy)); D.p_copy_pending = false; }
  if (words > D.p_stage_words) {
    if (D.p_stage) (void)hipHostFree(D.p_stage);
    D.p_stage = nullptr;
    D.p_stage_words = 0;
    const size_t cap = std::max<size_t>(words * 2, 1 << 12);
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&D.p_stage), cap * 4, hipHostMallocDefault));
    D.p_stage_words = cap;
  }
  if (np * 4 > D.forced.bytes) { quiesce(h); D.forced.ensure(np * 4); }
  D.poff.ensure((size_t)kPromptRows * 4);   // once: the address the ragged graphs hold
  int* offs = D.p_stage + np;
  bool ragged = false;
  for (int b = 0; b < kPromptRows; ++b) offs[b] = b < B ? P - plen[b] : 0;
  for (int b = 0; b < B; ++b) {
    ragged |= offs[b] > 0;
    for (int s = 0; s < P; ++s) D.p_stage[(size_t)b * P + s] = s < offs[b] ? h->d.pad_token_id : prompts[(size_t)b * P + s];
  }
  HIPCHK(hipMemcpyAsync(D.forced.p, D.p_stage, np * 4, hipMemcpyHostToDevice, D.hs));
  HIPCHK(hipMemcpyAsync(D.poff.p, offs, (size_t)kPromptRows * 4, hipMemcpyHostToDevice, D.hs));
  HIPCHK(hipEventRecord(D.ev_pcopy, D.hs));
  D.p_copy_pending = true;
  return ragged;
}
void check_prompts(const int32_t* prompts, int prompt_ld, const int32_t* prompt_len, int B, int nb) {
  REQUIRE(prompts && prompt_len && prompt_ld >= 1, "prompts, prompt_len and prompt_ld >= 1 are required");
  for (int b = 0; b < B; ++b)
    REQUIRE(prompt_len[b] >= 1 && prompt_len[b] <= prompt_ld,
            "prompt_len[" + std::to_string(b) + "] = " + std::to_string(prompt_len[b]) + " outside [1, prompt_ld = " +
                std::to_string(prompt_ld) + "] (the start token counts)");
  if (nb > 1)
    throw WcbError(WCB_ERR_UNSUPPORTED, "per-clip prompts are greedy only (num_beams = 1): beam scores count the prompt");
}

// Temperature sampling of a decode in context D: inv_T = 1 / T and the per-row seeds into the context's samp
// words, stream-ordered on the decode stream and passed by value (write_i32: the caller's array is not read
// after the call returns, async_out and several contexts in flight included). The allocation is made once.
constexpr int kSampRows = 64;
void check_sampling(float temperature, const uint64_t* seeds) {
  REQUIRE(seeds, "sampling: seeds is required");
  REQUIRE(std::isfinite(temperature) && temperature > 0.f, "sampling: temperature must be finite and > 0");
}
const uint64_t* install_sampling(DecCtx& D, float temperature, const uint64_t* seeds, int rows) {
  REQUIRE(rows >= 1 && rows <= kSampRows, "sampling: 1 .. 64 rows");
  D.samp.ensure((size_t)(1 + kSampRows) * 8);
  int w[2 + 2 * kSampRows] = {};
  const float inv_t = 1.0f / temperature;
  std::memcpy(w, &inv_t, 4);
  std::memcpy(w + 2, seeds, (size_t)rows * 8);
  write_i32(D.samp.as<int>(), w, 2 + 2 * rows, D.hs);
  return D.samp.as<uint64_t>();
}

// Repeat rules of a greedy decode in context D, after its prompt rows are final (a detected language
// patched in) and before its first step: the two values into the context's words by value on the decode stream
// (write_i32, as install_sampling), every row's seen bitmap cleared and set from its live prompt slots. The prompt is
// what decode_start left in D.forced — one shared row (stride 0), [rows][P], left-padded with the offsets in D.poff —
// or the start token alone. Returns the device view the steps of this decode carry.
constexpr int kRepRows = 64;
void check_repeat(const wcb_handle* h, int nb, bool sampled, bool windows) {
  if (!h->rep_on) return;
  if (nb > 1)
    throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules are greedy only (num_beams = 1; wcb_set_repeat_rules(h, NULL) removes them)");
  if (sampled) throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules with sampling are not supported (greedy only)");
  if (h->rules_on && h->rules_ts.on)
    throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules with timestamp decoding are not supported (token rules with timestamps = 1)");
  if (windows) throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules with wcb_generate_windows are not supported");
  if (h->d.n_text_ctx > kRepMaxHist)
    throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules: more than 448 text positions");
  if (h->vocab_pad / 32 > kRepBanWords)
    throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules: a vocabulary above 53248 tokens");
}
RepArgs start_repeat(wcb_handle* h, DecCtx& D, int rows, int P, bool has_prefix, int prompt_ld, bool ragged) {
  REQUIRE(rows >= 1 && rows <= kRepRows, "repeat rules: 1 .. 64 rows");
  const int words = h->vocab_pad / 32;
  D.seen.ensure((size_t)kRepRows * words * 4);   // once: vocab_pad is fixed by the weights
  D.rep_par.ensure(8);
  int w[2] = {0, h->rep_n};
  std::memcpy(w, &h->rep_p, 4);
  write_i32(D.rep_par.as<int>(), w, 2, D.hs);
  RepArgs r;
  r.seen = D.seen.as<uint32_t>(); r.words = words; r.par = D.rep_par.as<int>();
  r.prompt = has_prefix ? D.forced.as<int>() : nullptr; r.prompt_ld = prompt_ld; r.P = has_prefix ? P : 1;
  r.start_tok = h->d.decoder_start_token_id;
  r.poff = ragged ? D.poff.as<int>() : nullptr;
  rep_init(r, rows, h->d.vocab, D.hs);
  return r;
}

// Lt: the total length cap (prefix + max new tokens, MaxLength), Tc: cache positions, Lg: max new tokens
BeamArgs beam_args(wcb_handle* h, DecCtx& D, int B, int nb, int P, int Lt, int Tc, int Lg, int min_new, float lam,
                   const wcb_bias* bs) {
  size_t w[kBeamBufs];
  beam_words(B, nb, Lg, Tc, w);
  char* p = (char*)D.beam.p;
  auto take = [&](int i) { char* q = p; p += (w[i] * 4 + 255) / 256 * 256; return q; };
  int* ints = D.ints.as<int>();
  BeamArgs bm;
  bm.run_sc = (float*)take(0); bm.fin_sc = (float*)take(1); bm.fin_done = (int*)take(2); bm.fin_len = (int*)take(3);
  bm.run_seq = (int*)take(4); bm.fin_seq = (int*)take(5); bm.phys = (int*)take(6);
  bm.cand_val = (float*)take(7); bm.cand_tok = (int*)take(8); bm.flags = (int*)take(9); bm.parent = (int*)take(10);
  bm.chunk_stats = (float*)take(11);
  bm.nchunk = h->beam_chunks ? kBeamChunks : 1;
  bm.logits = D.logits.as<float>(); bm.ld = h->vocab_pad; bm.V = h->d.vocab;
  bm.B = B; bm.nb = nb; bm.K = 2 * nb; bm.P = P; bm.Lt = Lt; bm.T = Tc;
  bm.eos = h->d.eos_token_id; bm.pad = h->d.pad_token_id; bm.min_new = min_new;
  bm.lam = lam; bm.len_pen = 1.f;
  set_automaton(bm, bs, nullptr);
  bm.step = ints + I_STEP; bm.pos = ints + I_POS; bm.all_done = ints + I_DONE; bm.ticket = ints + I_TICKET;
  const RowInts ri(D, B * nb);
  bm.next_ids = ri.next; bm.state = ri.state;
  bm.out_ids = D.outbuf.as<int>(); bm.out_ld = Lg; bm.out_len = ints + I_UNFIN;
  return bm;
}

// Causal prefill of positions [p_begin, p_end) of every row (ids from src, row stride ld: prefill_step), in passes
// of prefill_chunk(rows) positions; each(c, p0, np) names what a pass's configuration has of its own
template <typename F>
void prefill_range(wcb_handle* h, const StepCfg& sc, const int* src, int ld, int p_begin, int p_end, F&& each) {
  for (int p0 = p_begin, np; p0 < p_end; p0 += np) {
    np = std::min(prefill_chunk(sc.B), p_end - p0);
    StepCfg c = sc;
    each(c, p0, np);
    prefill_step(h, c, np, src, ld);
  }
}
void prefill_range(wcb_handle* h, const StepCfg& sc, const int* src, int ld, int p_begin, int p_end) {
  prefill_range(h, sc, src, ld, p_begin, p_end, [](StepCfg&, int, int) {});
}

// The start of decode `st` in context buf, on its stream: the int block zeroed, the prompt uploaded — `shared`: one
// host row [P] for every decoder row (row stride 0), else [B][P], clip b's on each of its beam rows; null: the
// start token — the beam state initialised (before the prefill: its self-attention reads keys through bm.phys),
// and the configuration every pass of the decode starts from. plen (greedy, with prefix [B][P] left-padded): the
// per-clip prompt lengths — install_prompts
StepCfg decode_start(wcb_handle* h, int buf, wcb_state& st, const int32_t* prefix, bool shared, const wcb_bias* bs,
                     const int32_t* plen = nullptr) {
  DecCtx& D = h->dc[buf];
  const int R = st.B * st.nb, P = st.P;
  HIPCHK(hipMemsetAsync(D.ints.p, 0, RowInts::words(R) * 4, D.hs));   // (the rule state with finished[])
  std::vector<int32_t> rows;
  if (prefix && !shared && !plen)
    for (int r = 0; r < R; ++r) rows.insert(rows.end(), prefix + (size_t)(r / st.nb) * P, prefix + (size_t)(r / st.nb + 1) * P);
  const size_t pbytes = (shared ? (size_t)P : rows.size()) * 4;
  if (prefix && pbytes > D.forced.bytes) { quiesce(h); D.forced.ensure(pbytes); }
  if (plen) {   // (greedy: one row per clip)
    st.ragged = install_prompts(h, D, prefix, P, plen, st.B);
  } else if (!prefix) {
    fill_i32(RowInts(D, R).next, h->d.decoder_start_token_id, R, D.hs);
  } else if (shared) {
    write_i32(D.forced.as<int>(), prefix, P, D.hs);
  } else {
    HIPCHK(hipMemcpyAsync(D.forced.p, rows.data(), pbytes, hipMemcpyHostToDevice, D.hs));
    HIPCHK(hipStreamSynchronize(D.hs));   // pageable host source
  }
  if (st.nb > 1) {
    st.bm = beam_args(h, D, st.B, st.nb, P, P + st.max_new, st.T, st.max_new, st.min_new, st.lam, bs);
    beam_init(st.bm, D.hs);
  }
  StepCfg sc = step_cfg(h, buf, R, st.T, st.max_new);
  sc.bias = bs; sc.lam = st.lam; sc.min_new = st.min_new;
  sc.forced = D.forced.as<int>(); sc.forced_ld = shared ? 0 : P;
  sc.clips = st.B; sc.nb = st.nb; sc.xmode = st.xmode;
  if (st.nb > 1) { sc.phys = st.bm.phys; sc.beam = &st.bm; }
  if (st.ragged) sc.pos_off = D.poff.as<int>();
  return sc;
}

// The prompt of a decode begun by decode_start: positions 0 .. P-2 in causal prefill passes, then the last prompt
// token as the first step's input — greedy: embedded here, every step's finalize then embeds the next one
void decode_prompt(wcb_handle* h, const StepCfg& sc, int P, bool has_prefix) {
  DecCtx& D = h->dc[sc.buf];
  prefill_range(h, sc, sc.forced, sc.forced_ld, 0, P - 1);
  if (has_prefix) gather_col(RowInts(D, sc.B).next, sc.forced, sc.B, sc.forced_ld, P - 1, D.hs);
  if (sc.nb == 1) step_embed(h, sc);
}

// Language detection. check_lang: the range and the candidates of a call (V, eos: the vocabulary's);
// detect_pass: the pass itself in the decode context of sc, on its stream.
void check_lang(int lang_begin, int n_lang, const uint32_t* cand, int eos, int V) {
  REQUIRE(n_lang >= 1 && n_lang <= 16 * kLangTiles - 15, "n_lang must be in [1, 113]");
  REQUIRE(lang_begin > eos && lang_begin <= V - n_lang,
          "language range [" + std::to_string(lang_begin) + ", " + std::to_string(lang_begin) + " + " + std::to_string(n_lang) +
              ") outside (eos, vocab)");
  if (cand) {
    bool any = false;
    for (int i = 0; i < n_lang; ++i) any |= (cand[i >> 5] >> (i & 31)) & 1u;
    REQUIRE(any, "language candidates: the bitmap names no language");
  }
}
// the candidate bitmap into the context (null: none) and the range's tile columns into the arguments
void lang_range(DecCtx& D, LangArgs& a, int lang_begin, int n_lang, const uint32_t* cand, int V, hipStream_t st) {
  a.lang_begin = lang_begin; a.n_lang = n_lang;
  a.col0 = lang_begin / 16 * 16;
  a.col1 = std::min((lang_begin + n_lang + 15) / 16 * 16, V);
  if (cand) {
    D.lang.ensure((size_t)kLangWords * 4);   // once: no call in flight reads it before the first one wrote it
    int w[kLangWords] = {};
    std::memcpy(w, cand, (size_t)((n_lang + 31) / 32) * 4);
    write_i32(D.lang.as<int>(), w, kLangWords, st);
    a.cand = D.lang.as<uint32_t>();
  }
}
// One decoder pass over [decoder_start] at position 0 for every row of the decode sc begins (its int block zeroed:
// position 0, nothing generated), the language head on the residual rows in place of the LM head, then the finalize:
// ids / probabilities out, and with patch_ld > 0 the language column of the context's prompt rows (D.forced
// [B][patch_ld]) patched. A greedy step without selection: it writes self-attention slot 0 (the prefill writes it
// again), the step's activations and the `next` ids (decode_prompt sets them again), and advances nothing.
void detect_pass(wcb_handle* h, const StepCfg& sc, int lang_begin, int n_lang, const uint32_t* cand, int32_t* out_ids,
                 float* out_probs, int patch_ld, int patch_col) {
  DecCtx& D = h->dc[sc.buf];
  StepCfg c = step_cfg(h, sc.buf, sc.B, sc.T, sc.out_ld);
  c.clips = sc.clips; c.nb = 1; c.xmode = sc.xmode; c.host_pos = 0;
  const int B = c.B, d = h->d.d_model;
  fill_i32(RowInts(D, B).next, h->d.decoder_start_token_id, B, D.hs);
  step_embed(h, c);
  const int ngrp = (B + h->group_rows - 1) / h->group_rows;   // the row groups of a greedy step, back to back
  const int ns = std::max(ngrp, std::max(1, std::min(h->n_sub, B)));
  for (int i = 0; i < ns; ++i) {
    const int b0 = (int)((long)B * i / ns), b1 = (int)((long)B * (i + 1) / ns);
    decode_rows(h, c, b0, b1 - b0, i, D.hs);
  }
  LangArgs a;
  a.A = D.dx.as<float>(); a.lda = d; a.ln_w = h->dec_ln_w; a.ln_b = h->dec_ln_b;
  a.W = h->tok_emb; a.K = d; a.M = B;
  a.logits = c.logits_out; a.ld = c.logits_ld;
  lang_range(D, a, lang_begin, n_lang, cand, h->d.vocab, D.hs);
  a.out_ids = out_ids; a.out_probs = out_probs;
  if (patch_ld > 0) { a.prompts = D.forced.as<int>(); a.prompt_ld = patch_ld; a.prompt_col = patch_col; }
  const double cols = a.col1 - a.col0;
  h->timed("lang_head", 2.0 * B * cols * d, cols * d * esize(h->d.dtype) + (double)B * d * 4, D.hs,
           [&] { lang_head(h->dt, a, D.hs); });
  h->timed("lang_finalize", 0, (double)B * cols * 4, D.hs, [&] { lang_finalize(a, D.hs); });
}
// the language slot of a prompted call, checked against its prompts (before any device work)
void check_lang_slot(const wcb_handle* h, const wcb_lang_cfg* L, int prompt_ld, const int32_t* prompt_len, int B, int nb) {
  if (nb > 1) throw WcbError(WCB_ERR_UNSUPPORTED, "a language slot is greedy only (num_beams = 1): the ragged path");
  check_lang(L->lang_begin, L->n_lang, L->candidates, h->d.eos_token_id, h->d.vocab);
  REQUIRE(L->column_from_end >= 0 && L->column_from_end <= prompt_ld - 2, "language slot: column_from_end outside [0, prompt_ld - 2]");
  for (int b = 0; b < B; ++b)
    REQUIRE(prompt_len[b] >= L->column_from_end + 2,
            "language slot: prompt_len[" + std::to_string(b) + "] puts the slot at or before the start token");
}

// per-utterance lists into decode `st` of context D, before its first step: the forest uploaded, every row in its
// clip's root state
void start_forest(wcb_handle* h, DecCtx& D, wcb_state& st, const wcb_bias_batch* bb) {
  const int R = st.B * st.nb;
  const RowInts ri(D, R);
  st.fd = install_forest(h, D, bb);
  forest_init(st.fd.f, ri.state, st.nb == 1 ? ri.rowbase : nullptr, R, st.nb, D.hs);
  st.forest = true;
}

// The decode step of sc captured into g under `key`: the 1-step graph and, when it differs, the graph of
// steps_per_graph consecutive steps (every position-dependent value is read on the device, so it is the
// single-step graph unrolled)
void capture_steps(wcb_handle* h, const StepCfg& sc, StepGraphs& g, const char* key) {
  DecCtx& D = h->dc[sc.buf];
  g.drop();
  const int ks[2] = {1, h->steps_per_graph};
  hipGraphExec_t* const exec[2] = {&g.one, &g.k};
  for (int ki = 0; ki < (ks[1] > 1 ? 2 : 1); ++ki) {
    hipGraph_t graph;
    HIPCHK(hipStreamBeginCapture(D.hs, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < ks[ki]; ++i) decode_step(h, sc);
    HIPCHK(hipStreamEndCapture(D.hs, &graph));
    HIPCHK(hipGraphInstantiate(exec[ki], graph, nullptr, nullptr, 0));
    ++h->n_graph_captures;
    HIPCHK(hipGraphDestroy(graph));
  }
  g.key = key;
}

// One wcb_generate* call: batch, prompt, outputs, then what only some entry points have — bias, scores, sampling.
// Null: prefix (the start token alone), bias / bb (no shared automaton / per-utterance forest), smp (argmax)
struct GenCall {
  const float* mel; int B; const wcb_gen_cfg* cfg;
  const int32_t* prefix; int prefix_len;
  int32_t *out_ids, *out_steps;
  void* stream;
  const wcb_bias* bias = nullptr; const wcb_bias_batch* bb = nullptr;
  float *out_logprobs = nullptr, *out_seq_scores = nullptr;
  const wcb_sample_cfg* smp = nullptr;
  // per-clip prompts (wcb_generate_prompted): HOST [B][prompt_ld] left-padded, lengths HOST [B]; prefix is then null
  const int32_t* prompts = nullptr; int prompt_ld = 0; const int32_t* prompt_len = nullptr;
  // long-form (wcb_generate_windows): the B rows are windows of long features (mel is then null), and the no-speech
  // probability of every row [B] (nullable; needs out_logprobs)
  const wcb_windows* win = nullptr; float* out_no_speech = nullptr;
  // language slot (wcb_generate_lang; with prompts): detected on the device before the prefill
  const wcb_lang_cfg* lang = nullptr;
};

// the step-wise decode context, after the check every step-wise entry point makes of its state (`what`: the
// entry's other required arguments are there; `msg`: its own wording of the refusal)
DecCtx& step_ctx(wcb_handle* h, const wcb_state* st, bool what = true, const char* msg = "bad argument (state of this handle)") {
  REQUIRE(h && st && st->h == h && h->step_state == st && what, msg);
  return h->dc[wcb_handle::kMaxCtx - 1];
}

}  // namespace

extern "C" {

int wcb_log_mel(wcb_handle* h, const float* pcm, int B, int n_samples, int64_t pcm_stride, float* mel_out, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && pcm && mel_out && B > 0 && n_samples > 0, "bad argument");
    REQUIRE(pcm_stride >= std::min(n_samples, kNSamp), "pcm_stride < n_samples");
    if ((size_t)B * 4 > h->clip_max.bytes) { quiesce(h); h->clip_max.ensure((size_t)std::max(B, h->enc_B) * 4); }
    sync_in(h, stream, h->he);
    h->timed("log_mel", 0, (double)B * (std::min(n_samples, kNSamp) * 4.0 + h->d.n_mel * kFrames * 4.0 * 3), h->he, [&] {
      logmel_power_mel(pcm, (long)pcm_stride, n_samples, B, h->dft.as<float>(), h->mel_split ? h->dft3.p : nullptr,
                       h->mel_lo.as<int>(), h->mel_hi.as<int>(),
                       h->mel_w.as<float>(), h->d.n_mel, mel_out, h->clip_max.as<unsigned>(), h->he);
      logmel_normalize(mel_out, h->clip_max.as<unsigned>(), B, h->d.n_mel, h->he);
    });
    sync_out(h, stream, h->he);
  });
}

int wcb_encode(wcb_handle* h, const float* mel, int B, void* enc_out, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && mel && B > 0, "bad argument");
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    ensure_enc_ws(h, B);
    sync_in(h, stream, h->he);
    encode_impl(h, mel, B, enc_out);
    sync_out(h, stream, h->he);
  });
}

int wcb_log_mel_long(wcb_handle* h, const float* pcm, int B, const int32_t* n_valid, int n_total, int64_t pcm_stride,
                     float* mel_out, int T_ld, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && pcm && mel_out && n_valid && B > 0 && B <= kWinRows, "bad argument (1 .. 64 clips)");
    REQUIRE(n_total >= 800 && pcm_stride >= n_total, "n_total must be at least 800 samples and at most pcm_stride");
    REQUIRE(T_ld >= n_total / 160, "T_ld < n_total / 160 frames");
    for (int b = 0; b < B; ++b) REQUIRE(n_valid[b] >= 0 && n_valid[b] <= n_total, "n_valid outside [0, n_total]");
    if ((size_t)B * 4 > h->clip_max.bytes) { quiesce(h); h->clip_max.ensure((size_t)std::max(B, h->enc_B) * 4); }
    h->win_ints.ensure((size_t)3 * kWinRows * 4);
    sync_in(h, stream, h->he);
    write_i32(h->win_ints.as<int>(), n_valid, B, h->he);
    h->timed("log_mel_long", 0, (double)B * (n_total * 4.0 + h->d.n_mel * (n_total / 160) * 4.0 * 3), h->he, [&] {
      logmel_long(pcm, (long)pcm_stride, h->win_ints.as<int>(), n_total, B, h->dft.as<float>(), h->mel_split ? h->dft3.p : nullptr,
                  h->mel_lo.as<int>(), h->mel_hi.as<int>(), h->mel_w.as<float>(), h->d.n_mel, mel_out, T_ld,
                  h->clip_max.as<unsigned>(), h->he);
    });
    sync_out(h, stream, h->he);
  });
}

int wcb_encode_windows(wcb_handle* h, const wcb_windows* w, int rows, void* enc_out, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h, "bad argument");
    check_windows(w, rows);
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    ensure_enc_ws(h, rows);
    sync_in(h, stream, h->he);
    encode_impl(h, nullptr, rows, enc_out, w);
    sync_out(h, stream, h->he);
  });
}

// every wcb_generate* entry point: encode, then decode greedily or by beam search
static void generate_impl(wcb_handle* h, const GenCall& c) {
  {
    const wcb_gen_cfg* cfg = c.cfg;
    const wcb_sample_cfg* smp = c.smp;
    const wcb_bias_batch* bb = c.bb;
    const int B = c.B;
    REQUIRE(h && cfg && c.out_ids && c.out_steps && B > 0, "bad argument");
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    const int nb = cfg->num_beams;
    REQUIRE(nb >= 1 && nb <= kMaxBeams, "num_beams must be in [1, 8]");
    if (smp) {
      check_sampling(smp->temperature, smp->seeds);
      if (nb > 1) throw WcbError(WCB_ERR_UNSUPPORTED, "sampling is greedy only (num_beams = 1)");
    }
    if (h->rules_on && nb > 1)
      throw WcbError(WCB_ERR_UNSUPPORTED, "token rules are greedy only (num_beams = 1; wcb_set_token_rules(h, NULL) removes them)");
    if (h->rules_on && h->rules_ts.on && smp)
      throw WcbError(WCB_ERR_UNSUPPORTED, "timestamp decoding with sampling is not supported (greedy only)");
    check_repeat(h, nb, smp != nullptr, c.win != nullptr);
    if (nb > 1 && c.out_logprobs)
      throw WcbError(WCB_ERR_UNSUPPORTED, "token log-probs are greedy only (beam search: out_seq_scores)");
    if (nb == 1 && c.out_seq_scores)
      throw WcbError(WCB_ERR_UNSUPPORTED, "sequence scores are beam-search only (greedy: out_logprobs)");
    const int R = B * nb;   // decoder rows: utterance b, beam i -> row b*nb + i
    REQUIRE(B <= 64, "batch > 64 per handle: split the batch");
    REQUIRE(R <= 64 * DecCtx::kMaxSub, "batch x num_beams > 512 rows per call: split the batch");
    REQUIRE(cfg->bias_boost >= 0.f, "bias_boost must be >= 0");
    REQUIRE(cfg->max_new_tokens >= 1, "max_new_tokens must be >= 1");
    REQUIRE(c.mel != nullptr || c.win != nullptr, "mel is required");
    if (c.win) check_windows(c.win, B);
    if (c.out_no_speech && !c.out_logprobs)
      throw WcbError(WCB_ERR_UNSUPPORTED, "the no-speech probability reuses the token log-probs' logsumexp: out_logprobs is required");
    const bool prompted = c.prompts || c.prompt_len;
    if (prompted) check_prompts(c.prompts, c.prompt_ld, c.prompt_len, B, nb);
    if (c.lang) check_lang_slot(h, c.lang, c.prompt_ld, c.prompt_len, B, nb);
    const int P = prompted ? c.prompt_ld : c.prefix ? c.prefix_len : 1;
    REQUIRE(P >= 1, "prefix_len must be >= 1");
    const int T = P + cfg->max_new_tokens;
    REQUIRE(T <= h->d.n_text_ctx + 1, "prefix + max_new_tokens exceeds max_target_positions");
    const wcb_bias* bs = c.bias ? c.bias : h->empty_bias.get();
    REQUIRE(bs == h->empty_bias.get() || bs->owner == h,
            "bias automaton was created on another handle (wcb_bias_create binds it to its handle)");
    REQUIRE(bs->vocab == h->d.vocab, "bias automaton built for another vocabulary");
    if (bb) {
      REQUIRE(bb->vocab == h->d.vocab, "bias batch built for another vocabulary");
      REQUIRE(bb->B == B, "bias batch: built for " + std::to_string(bb->B) + " clips, the call has " + std::to_string(B));
    }
    const bool fixed_len = cfg->min_new_tokens >= cfg->max_new_tokens;   // EOS masked: no host polling
    const int max_new = cfg->max_new_tokens, out_ld = max_new;
    const int Tc = std::min(T, h->d.n_text_ctx);
    if (nb > 1) {
      REQUIRE(max_new <= kBeamMaxLen && Tc <= kBeamMaxLen, "beam search: more than 448 positions");
      REQUIRE(cfg->bias_boost == 0.f || h->d.vocab <= kBeamMaxVocab, "beam search boost: vocabulary too large");
    }
    ensure_enc_ws(h, B);
    const int xm = nb > 1 ? h->beam_xmode : h->xmode;   // this call's cross-attention formulation
    ensure_dec_ws(h, B, R, Tc, out_ld, xm, prefill_rows(R, P - 1));
    const int buf = h->gen_count++ % h->nctx;
    h->last_gen_buf = buf; h->last_gen_B = B; h->last_gen_xm = xm; h->last_gen_id = h->gen_count;   // (wcb_align, enc = NULL)
    DecCtx& D = h->dc[buf];
    // beam state [R] / [R][max_new] / [R][Tc] / [R][K] / [B][2] in one buffer
    if (nb > 1) ensure_beam_buf(h, D, B, nb, max_new, Tc);
    if (c.out_logprobs) ensure_lp_ws(h, D, R, out_ld);
    // ---- encoder stream: front end → encoder → cross-K/V into buffer `buf` once the decode that
    //      last read that buffer has finished. It overlaps the previous call's decode.
    sync_in(h, c.stream, h->he);
    HIPCHK(hipStreamWaitEvent(h->he, h->ev_dec[buf], 0));
    if (xm == 1) {   // the decode reads the encoder output itself (re-laid out for the stream when xenc_fm)
      encode_impl(h, c.mel, B, xenc_fm_on(h) ? nullptr : h->xkv2[buf].p, c.win);
      if (xenc_fm_on(h)) fill_xenc(h, buf, h->encout.p, B, h->he);
    } else {
      encode_impl(h, c.mel, B, nullptr, c.win);
      h->timed_wall("xkv_gemm_total", h->he, [&] { cross_kv(h, B, buf, h->encout.p); });
    }
    HIPCHK(hipEventRecord(h->ev_xkv[buf], h->he));
    // ---- decode stream
    HIPCHK(hipStreamWaitEvent(D.hs, h->ev_xkv[buf], 0));
    int* ints = D.ints.as<int>();
    wcb_state st;
    st.h = h; st.B = B; st.nb = nb; st.P = P; st.T = Tc; st.max_new = max_new; st.min_new = cfg->min_new_tokens;
    st.lam = cfg->bias_boost; st.xmode = xm;
    StepCfg sc = prompted ? decode_start(h, buf, st, c.prompts, /*shared=*/false, bs, c.prompt_len)
                          : decode_start(h, buf, st, c.prefix, /*shared=*/true, bs);
    BeamArgs& bm = st.bm;
    if (bb) {   // per-utterance lists
      start_forest(h, D, st, bb);
      sc.forest = &st.fd;
      if (nb > 1) set_automaton(bm, bs, &st.fd);
    }
    if (c.out_logprobs) {   // every column a step does not reach stays 0
      sc.logprob_out = D.lpbuf.as<float>();
      HIPCHK(hipMemsetAsync(D.lpbuf.p, 0, (size_t)R * out_ld * 4, D.hs));
    }
    if (smp) sc.samp = install_sampling(D, smp->temperature, smp->seeds, R);
    if (c.out_no_speech) {
      D.nsp.ensure((size_t)kWinRows * 4);
      sc.nsp_out = D.nsp.as<float>();
    }
    const bool ruled = nb == 1 && h->rules_on;
    if (ruled) apply_rules(h, sc);
    if (c.lang)   // after the encoder, before the prefill: the pass, then the finalize that patches the prompt rows
      detect_pass(h, sc, c.lang->lang_begin, c.lang->n_lang, c.lang->candidates, c.lang->out_ids, c.lang->out_probs, P,
                  P - 1 - c.lang->column_from_end);
    decode_prompt(h, sc, P, c.prefix != nullptr || prompted);
    const bool has_prefix = c.prefix != nullptr || prompted;
    if (h->rep_on) sc.rep = st.rep = start_repeat(h, D, R, P, has_prefix, sc.forced_ld, st.ragged);
    sc.lm_head = true;
    sc.select = true;
    sc.embedded = nb == 1;   // greedy: decode_prompt embedded the first step's input
    // the graph reads a shared automaton through its own buffers (key: its id) and a per-utterance forest
    // through the context's stable buffers (key: forest mode and the capacities, never the lists)
    char key[256], bkey[64];
    if (bb) snprintf(bkey, sizeof bkey, "F%d.%d.%d", D.f_ns, D.f_nt, D.f_nrc);
    else snprintf(bkey, sizeof bkey, "%llu", (unsigned long long)bs->id);
    int kn = snprintf(key, sizeof key, "%d/%d/%d/%d/%s/%a/%d/%d/%d/%d", B, nb, Tc, out_ld, bkey,
                      cfg->bias_boost, cfg->min_new_tokens, h->n_sub, (int)h->prof_stamps, P);
    if (ruled)   // what a ruled graph bakes in beside the bitmaps' stable addresses
      kn += snprintf(key + kn, sizeof key - kn, "/R%d.%d.%d.%d", sc.ts.on, sc.ts.ts0, sc.ts.max_init, (int)h->rules_has0);
    if (st.ragged)   // ragged prompts: the windowed kernels reading the context's offsets — the fact, never the lengths
      kn += snprintf(key + kn, sizeof key - kn, "/G");
    if (sc.rep.seen)   // repeat rules: the fact and how the history reads the prompt rows — never p or n
      snprintf(key + kn, sizeof key - kn, "/Q%d", !has_prefix ? 0 : sc.forced_ld ? 2 : 1);
    // per-launch HIP events (profiling bit 0) cannot bracket nodes of a replayed graph: eager launches
    const bool use_graph = cfg->use_graph && !h->prof;
    // The decode step replays as a hipGraph; steps_per_graph steps are captured into one graph so the
    // per-replay gap is paid once per chunk. Natural-EOS mode polls the device "all finished" flag once
    // per chunk. A ruled, a sampled and a scored decode each replay graphs of their own under the same key
    // string (never the seeds or the temperature), so no kind of call evicts another's.
    const int chunk = h->steps_per_graph;
    int done = 0, steps = 0;
    StepGraphs& g = D.graphs_of(ruled, smp != nullptr, c.out_logprobs != nullptr, c.out_no_speech != nullptr, sc.rep.seen != nullptr);
    if (use_graph && (!g.one || g.key != key)) capture_steps(h, sc, g, key);
    // Natural-EOS mode (reference decoding) polls the device "all finished" step one chunk behind:
    // chunk k+1 is queued before the host waits for chunk k's flag, so the GPU never idles on the
    // host (at most one chunk of extra steps after the last row finished; the output is cut at it).
    int pending = -1;   // slot of the chunk whose flag is in flight
    h->timed_wall("decode_loop", D.hs, [&] {
      while (steps < max_new) {
        const int n = std::min(chunk, max_new - steps);
        if (use_graph && n == chunk && g.k) {
          HIPCHK(hipGraphLaunch(g.k, D.hs));
        } else {
          for (int i = 0; i < n; ++i) {
            if (use_graph) {
              HIPCHK(hipGraphLaunch(g.one, D.hs));
            } else {
              sc.host_pos = P - 1 + steps + i;
              decode_step(h, sc);
            }
          }
        }
        steps += n;
        if (fixed_len) continue;
        const int slot = (pending + 1) & 1;
        HIPCHK(hipMemcpyAsync(D.done_h + slot, ints + I_DONE, 4, hipMemcpyDeviceToHost, D.hs));
        HIPCHK(hipEventRecord(D.ev_poll[slot], D.hs));
        if (pending >= 0) {
          HIPCHK(hipEventSynchronize(D.ev_poll[pending]));
          if (D.done_h[pending] > 0) { done = D.done_h[pending]; break; }
        }
        pending = slot;
      }
      if (!fixed_len && done <= 0 && pending >= 0) {
        HIPCHK(hipEventSynchronize(D.ev_poll[pending]));
        done = D.done_h[pending];
      }
    });
    if (done <= 0) done = steps;
    if (h->prof_stamps) {   // fold this call's cross-attention stamps into the device accumulator
      const double launches_rows = (double)(P - 1 + steps) * h->d.n_layers * R * h->H() * h->S();
      // algorithmic bytes: K and V (xmode 0) or the encoder output once for all heads (xmode 1), of
      // every distinct clip once (the beams of a clip share its rows: counted per clip, not per row)
      const double launches_clips = launches_rows / nb;
      h->xattn_bytes += xm ? launches_clips / h->H() * h->d.d_model * esize(h->d.dtype)
                                 : launches_clips * 64 * 2 * esize(h->d.dtype);
      h->xattn_flops += xm ? launches_rows * h->d.d_model * 4 : launches_rows * 64 * 4;
      for (int r = 0; r < wcb_handle::kStampRegions; ++r)
        stamp_reduce(h->stamp_base(buf, r), h->stamp_slots(), h->stamp_acc.as<unsigned long long>() + 2 * r, D.hs);
    }
    if (nb > 1) {   // best finished sequence of every utterance; its columns = the longest of them
      bm.out_score = c.out_seq_scores;   // (nullable) that hypothesis's score, straight into the caller's [B]
      beam_output(bm, D.hs);
      HIPCHK(hipMemcpyAsync(c.out_ids, D.outbuf.p, (size_t)B * out_ld * 4, hipMemcpyDeviceToDevice, D.hs));
      if (cfg->async_out) {   // serving pipelines: every max_new column (pad past each best sequence), no
                              // host wait, so the next call's front end + encoder overlap this decode
        HIPCHK(hipEventRecord(h->ev_dec[buf], D.hs));
        *c.out_steps = max_new;
        return;
      }
      int olen = 0;
      HIPCHK(hipMemcpyAsync(&olen, ints + I_UNFIN, 4, hipMemcpyDeviceToHost, D.hs));
      HIPCHK(hipEventRecord(h->ev_dec[buf], D.hs));
      HIPCHK(hipStreamSynchronize(D.hs));
      if (h->xq_kq) check_dev_err(h);   // the in-launch hand-off's error word: outputs invalid if it is set
      *c.out_steps = std::min(olen, max_new);
      sync_out(h, c.stream, D.hs);
      return;
    }
    HIPCHK(hipMemcpyAsync(c.out_ids, D.outbuf.p, (size_t)B * out_ld * 4, hipMemcpyDeviceToDevice, D.hs));
    if (c.out_logprobs)
      HIPCHK(hipMemcpyAsync(c.out_logprobs, D.lpbuf.p, (size_t)B * out_ld * 4, hipMemcpyDeviceToDevice, D.hs));
    if (c.out_no_speech)
      HIPCHK(hipMemcpyAsync(c.out_no_speech, D.nsp.p, (size_t)B * 4, hipMemcpyDeviceToDevice, D.hs));
    HIPCHK(hipEventRecord(h->ev_dec[buf], D.hs));
    *c.out_steps = std::min(done, max_new);
    if (!cfg->async_out) {
      // blocking calls with the in-launch hand-off on (option xq_kq) validate its error word before the ids
      // are handed out; async calls report it at wcb_synchronize
      if (h->xq_kq) { HIPCHK(hipStreamSynchronize(D.hs)); check_dev_err(h); }
      sync_out(h, c.stream, D.hs);
    }
  }
}

int wcb_generate(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                 const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream) {
  return guarded(h, [&] { generate_impl(h, {mel, B, cfg, prefix, prefix_len, out_ids, out_steps, stream, bias}); });
}

int wcb_generate_biased(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias_batch* bb,
                        const int32_t* prefix, int prefix_len, int32_t* out_ids, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(bb, "wcb_generate_biased: the bias batch is required (wcb_generate decodes without one)");
    generate_impl(h, {mel, B, cfg, prefix, prefix_len, out_ids, out_steps, stream, nullptr, bb});
  });
}

int wcb_generate_scored(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                        const wcb_bias_batch* bb, const int32_t* prefix, int prefix_len, int32_t* out_ids,
                        float* out_logprobs, float* out_seq_scores, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(!(bias && bb), "wcb_generate_scored: a shared automaton or a bias batch, not both");
    generate_impl(h, {mel, B, cfg, prefix, prefix_len, out_ids, out_steps, stream, bias, bb, out_logprobs, out_seq_scores});
  });
}

int wcb_generate_sampled(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_sample_cfg* smp,
                         const wcb_bias* bias, const wcb_bias_batch* bb, const int32_t* prefix, int prefix_len,
                         int32_t* out_ids, float* out_logprobs, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(smp, "wcb_generate_sampled: the sampling configuration is required (wcb_generate_scored decodes without one)");
    REQUIRE(!(bias && bb), "wcb_generate_sampled: a shared automaton or a bias batch, not both");
    generate_impl(h, {mel, B, cfg, prefix, prefix_len, out_ids, out_steps, stream, bias, bb, out_logprobs, nullptr, smp});
  });
}

int wcb_generate_prompted(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_sample_cfg* smp,
                          const wcb_bias* bias, const wcb_bias_batch* bb, const int32_t* prompts, int prompt_ld,
                          const int32_t* prompt_len, int32_t* out_ids, float* out_logprobs, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && cfg, "bad argument");
    REQUIRE(!(bias && bb), "wcb_generate_prompted: a shared automaton or a bias batch, not both");
    REQUIRE(prompts && prompt_len, "wcb_generate_prompted: prompts and prompt_len are required (wcb_generate_sampled decodes one shared prompt)");
    GenCall c{mel, B, cfg, nullptr, 1, out_ids, out_steps, stream, bias, bb, out_logprobs, nullptr, smp};
    c.prompts = prompts; c.prompt_ld = prompt_ld; c.prompt_len = prompt_len;
    generate_impl(h, c);
  });
}

int wcb_generate_windows(wcb_handle* h, const wcb_windows* w, int rows, const wcb_gen_cfg* cfg, const wcb_bias* bias,
                         const wcb_bias_batch* bb, const int32_t* prompts, int prompt_ld, const int32_t* prompt_len,
                         int32_t* out_ids, float* out_logprobs, float* out_no_speech, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && cfg && w, "bad argument");
    REQUIRE(!(bias && bb), "wcb_generate_windows: a shared automaton or a bias batch, not both");
    REQUIRE(prompts && prompt_len, "wcb_generate_windows: prompts and prompt_len are required (prompt_len 1: the start token alone)");
    if (cfg->num_beams != 1) throw WcbError(WCB_ERR_UNSUPPORTED, "wcb_generate_windows is greedy only (num_beams = 1)");
    GenCall c{nullptr, rows, cfg, nullptr, 1, out_ids, out_steps, stream, bias, bb, out_logprobs, nullptr, nullptr};
    c.prompts = prompts; c.prompt_ld = prompt_ld; c.prompt_len = prompt_len;
    c.win = w; c.out_no_speech = out_no_speech;
    generate_impl(h, c);
  });
}

// ---- step-wise greedy decoding (SURVEY §8(b) wcb_decode_begin / wcb_decode_step): the decode step
// of wcb_generate, one token per call, on the decode context kMaxCtx-1 (its own stream and buffers,
// so generate() calls on contexts 0 .. nctx-1 are unaffected); eager launches (the caller inspects
// every step). One active state per handle.

// begin (greedy, nb = 1, or the beam path of wcb_generate, nb >= 2): the given encoder output into the context,
// the per-clip prefix prefilled on every row of the clip, the first step's input ready; the length cap is
// prefix + max_new_tokens, at most max_target_positions (generate()'s)
// plen (wcb_decode_begin_prompted): prefix = the per-clip prompts [B][prefix_len] left-padded, plen their lengths
static void decode_begin(wcb_handle* h, const void* enc, int B, int nb, const int32_t* prefix, int prefix_len,
                         int max_new_tokens, float bias_boost, int min_new_tokens, wcb_state** out, void* stream,
                         const int32_t* plen = nullptr, bool prompted = false, const wcb_lang_cfg* lang = nullptr) {
  REQUIRE(h && enc && out && B > 0 && B <= 64, "bad argument (1 <= B <= 64, enc and out required)");
  if (prompted) check_prompts(prefix, prefix_len, plen, B, nb);
  if (lang) check_lang_slot(h, lang, prefix_len, plen, B, nb);
  if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
  if (nb < 1) throw WcbError(WCB_ERR_ARG, "num_beams must be >= 1");
  REQUIRE(nb <= kMaxBeams, "num_beams must be in [2, 8] (greedy: num_beams = 1)");
  if (nb > 1 && h->rules_on)
    throw WcbError(WCB_ERR_UNSUPPORTED, "token rules are greedy only (num_beams = 1; wcb_set_token_rules(h, NULL) removes them)");
  check_repeat(h, nb, false, false);
  const int R = B * nb;
  REQUIRE(R <= 64 * DecCtx::kMaxSub, "batch x num_beams > 512 rows: split the batch");
  REQUIRE(h->nctx < wcb_handle::kMaxCtx, "step-wise decoding needs a free decode context (decode_contexts <= 3)");
  REQUIRE(!h->step_state, "a step-wise decode is already active on this handle (wcb_decode_end first)");
  REQUIRE(bias_boost >= 0.f && min_new_tokens >= 0 && (nb == 1 || max_new_tokens >= 1),
          nb == 1 ? "bias_boost and min_new_tokens must be >= 0" : "bias_boost and min_new_tokens must be >= 0, max_new_tokens >= 1");
  REQUIRE(nb == 1 || bias_boost == 0.f || h->d.vocab <= kBeamMaxVocab, "beam search boost: vocabulary too large");
  const int P = prefix ? prefix_len : 1;
  REQUIRE(P >= 1 && P < h->d.n_text_ctx, "prefix_len must be in [1, max_target_positions)");
  const int Tc = std::min(P + max_new_tokens, h->d.n_text_ctx);
  REQUIRE(nb == 1 || Tc <= kBeamMaxLen, "beam search: more than 448 positions");
  // owned until the device work below succeeded (HIPCHK throws through here)
  std::unique_ptr<wcb_state> st(new wcb_state);
  st->h = h; st->B = B; st->P = P; st->T = Tc; st->max_new = Tc - P; st->min_new = min_new_tokens;
  st->xmode = nb > 1 ? h->beam_xmode : h->xmode; st->lam = bias_boost; st->nb = nb;
  const int ci = wcb_handle::kMaxCtx - 1;
  ensure_dec_ws(h, B, R, Tc, st->max_new, st->xmode, prefill_rows(R, P - 1), ci, ci + 1);
  DecCtx& D = h->dc[ci];
  if (nb > 1) ensure_beam_buf(h, D, B, nb, st->max_new, Tc);
  sync_in(h, stream, D.hs);
  // the caller's encoder output [B][1500][d] (model dtype) is copied / projected into owned buffers
  enc_to_ctx(h, ci, enc, B, st->xmode, D.hs, stream);
  const StepCfg sc = decode_start(h, ci, *st, prefix, /*shared=*/false, h->empty_bias.get(), plen);
  if (lang) detect_pass(h, sc, lang->lang_begin, lang->n_lang, lang->candidates, lang->out_ids, lang->out_probs, P, P - 1 - lang->column_from_end);
  decode_prompt(h, sc, P, prefix != nullptr);
  if (h->rep_on) st->rep = start_repeat(h, D, R, P, prefix != nullptr, sc.forced_ld, st->ragged);
  HIPCHK(hipStreamSynchronize(D.hs));
  h->step_state = st.release();
  *out = h->step_state;
  sync_out(h, stream, D.hs);
}

int wcb_decode_begin(wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prefix, int prefix_len,
                     float bias_boost, int min_new_tokens, wcb_state** out, void* stream) {
  return guarded(h, [&] {   // to the default length cap (generate()'s max_length 448)
    decode_begin(h, enc, B, num_beams, prefix, prefix_len, h ? h->d.n_text_ctx : 0, bias_boost, min_new_tokens, out, stream);
  });
}

int wcb_decode_begin_prompted(wcb_handle* h, const void* enc, int B, const int32_t* prompts, int prompt_ld,
                              const int32_t* prompt_len, float bias_boost, int min_new_tokens, wcb_state** out, void* stream) {
  return guarded(h, [&] {   // greedy, to the default length cap as wcb_decode_begin
    decode_begin(h, enc, B, 1, prompts, prompt_ld, h ? h->d.n_text_ctx : 0, bias_boost, min_new_tokens, out, stream, prompt_len,
                 /*prompted=*/true);
  });
}

int wcb_decode_begin_lang(wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prompts, int prompt_ld,
                          const int32_t* prompt_len, const wcb_lang_cfg* lang, float bias_boost, int min_new_tokens,
                          wcb_state** out, void* stream) {
  return guarded(h, [&] {
    decode_begin(h, enc, B, num_beams, prompts, prompt_ld, h ? h->d.n_text_ctx : 0, bias_boost, min_new_tokens, out, stream,
                 prompt_len, /*prompted=*/true, lang);
  });
}

int wcb_generate_lang(wcb_handle* h, const float* mel, int B, const wcb_gen_cfg* cfg, const wcb_sample_cfg* smp,
                      const wcb_bias* bias, const wcb_bias_batch* bb, const int32_t* prompts, int prompt_ld,
                      const int32_t* prompt_len, const wcb_lang_cfg* lang, int32_t* out_ids, float* out_logprobs,
                      int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && cfg, "bad argument");
    REQUIRE(!(bias && bb), "wcb_generate_lang: a shared automaton or a bias batch, not both");
    REQUIRE(prompts && prompt_len, "wcb_generate_lang: prompts and prompt_len are required");
    GenCall c{mel, B, cfg, nullptr, 1, out_ids, out_steps, stream, bias, bb, out_logprobs, nullptr, smp};
    c.prompts = prompts; c.prompt_ld = prompt_ld; c.prompt_len = prompt_len; c.lang = lang;
    generate_impl(h, c);
  });
}

// language detection on a given encoder output: the step-wise decode context holds it for the length of the call
int wcb_detect_language(wcb_handle* h, const void* enc, int B, int lang_begin, int n_lang, const uint32_t* candidates,
                        int32_t* out_ids, float* out_probs, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && enc && out_ids && B > 0 && B <= 64, "bad argument (1 <= B <= 64, enc and out_ids required)");
    check_lang(lang_begin, n_lang, candidates, h->d.eos_token_id, h->d.vocab);
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    REQUIRE(h->nctx < wcb_handle::kMaxCtx, "language detection needs a free decode context (decode_contexts <= 3)");
    if (h->step_state) throw WcbError(WCB_ERR_STATE, "a step-wise decode is open on this handle (wcb_decode_end first)");
    const int ci = wcb_handle::kMaxCtx - 1, T = 2;
    ensure_dec_ws(h, B, B, T, 1, h->xmode, 0, ci, ci + 1);
    DecCtx& D = h->dc[ci];
    sync_in(h, stream, D.hs);
    enc_to_ctx(h, ci, enc, B, h->xmode, D.hs, stream);
    HIPCHK(hipMemsetAsync(D.ints.p, 0, RowInts::words(B) * 4, D.hs));
    StepCfg sc = step_cfg(h, ci, B, T, 1);
    sc.clips = B;
    detect_pass(h, sc, lang_begin, n_lang, candidates, out_ids, out_probs, 0, 0);
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_step(wcb_handle* h, wcb_state* st, const wcb_bias* bias, int32_t* next_ids, float* scores, void* stream) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, next_ids, "bad argument (state of this handle, next_ids)");
    REQUIRE(st->fwd == 0, "wcb_decode_step on a forward cache (wcb_forward_cached state)");
    if (st->steps >= st->max_new) {
      // the length cap: refused, except for a finished beam search, whose steps are frozen (identity
      // parents, pad ids; the device position stopped at the last cache slot)
      bool frozen = false;
      if (st->nb > 1) {
        int v = 0;
        HIPCHK(hipMemcpyAsync(&v, D.ints.as<int>() + I_DONE, 4, hipMemcpyDeviceToHost, D.hs));
        HIPCHK(hipStreamSynchronize(D.hs));
        frozen = v > 0;
      }
      REQUIRE(frozen, "max_target_positions reached");
    }
    REQUIRE(!st->forest || !bias, "wcb_decode_step: the state holds per-utterance lists (wcb_decode_bias_batch): bias must be NULL");
    const wcb_bias* bs = bias ? bias : h->empty_bias.get();
    REQUIRE(bs == h->empty_bias.get() || bs->owner == h, "bias automaton was created on another handle");
    REQUIRE(bs->vocab == h->d.vocab, "bias automaton built for another vocabulary");
    REQUIRE(st->steps == 0 || bs->id == st->bias_id, "the bias automaton must stay the same for the whole decode");
    sync_in(h, stream, D.hs);
    const int R = st->B * st->nb;
    StepCfg sc = step_cfg(h, wcb_handle::kMaxCtx - 1, R, st->T, st->max_new);
    sc.lm_head = true;
    sc.select = true;
    sc.bias = bs; sc.lam = st->lam; sc.min_new = st->min_new;
    sc.clips = st->B;
    sc.xmode = st->xmode;
    sc.host_pos = st->P - 1 + st->steps;
    if (st->nb > 1) {   // beam step: the running beams' new tokens, their scores (running log-prob sums)
      set_automaton(st->bm, bs, st->forest ? &st->fd : nullptr);
      sc.nb = st->nb;
      sc.phys = st->bm.phys;
      sc.beam = &st->bm;
    } else {
      sc.score_out = scores;
      sc.embedded = true;   // (wcb_decode_begin embedded the first input; each finalize embeds the next)
      if (st->logprobs) sc.logprob_out = D.lpbuf.as<float>();
      if (st->no_speech) sc.nsp_out = D.nsp.as<float>();
      if (st->sampling) sc.samp = D.samp.as<uint64_t>();
      if (st->ragged) sc.pos_off = D.poff.as<int>();
      apply_rules(h, sc);   // (fixed for the whole decode: wcb_set_token_rules is refused while the state is open)
      sc.rep = st->rep;
    }
    if (st->forest) sc.forest = &st->fd;
    decode_step(h, sc);
    HIPCHK(hipMemcpyAsync(next_ids, RowInts(D, R).next, (size_t)R * 4, hipMemcpyDeviceToDevice, D.hs));
    if (st->nb > 1 && scores)
      HIPCHK(hipMemcpyAsync(scores, st->bm.run_sc, (size_t)R * 4, hipMemcpyDeviceToDevice, D.hs));
    st->bias_id = bs->id;
    ++st->steps;
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_bias_batch(wcb_handle* h, wcb_state* st, const wcb_bias_batch* bb) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, bb, "bad argument (state of this handle, bias batch)");
    REQUIRE(st->fwd == 0, "wcb_decode_bias_batch on a forward cache (wcb_forward_cached state)");
    REQUIRE(st->steps == 0, "wcb_decode_bias_batch: after the first step (install it right after wcb_decode_begin)");
    REQUIRE(bb->vocab == h->d.vocab, "bias batch built for another vocabulary");
    REQUIRE(bb->B == st->B, "bias batch: built for " + std::to_string(bb->B) + " clips, the state has " + std::to_string(st->B));
    start_forest(h, D, *st, bb);
  });
}

int wcb_decode_begin_beams(wcb_handle* h, const void* enc, int B, int num_beams, const int32_t* prefix, int prefix_len,
                           int max_new_tokens, float bias_boost, int min_new_tokens, wcb_state** out, void* stream) {
  return guarded(h, [&] {
    REQUIRE(num_beams >= 2, "wcb_decode_begin_beams: num_beams must be >= 2 (greedy: wcb_decode_begin)");
    decode_begin(h, enc, B, num_beams, prefix, prefix_len, max_new_tokens, bias_boost, min_new_tokens, out, stream);
  });
}

int wcb_decode_parents(wcb_handle* h, wcb_state* st, int32_t* parents, void* stream) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, parents, "bad argument (state of this handle, parents)");
    REQUIRE(st->nb > 1, "wcb_decode_parents: not a beam-search state");
    REQUIRE(st->steps > 0, "wcb_decode_parents: no step taken yet");
    sync_in(h, stream, D.hs);
    HIPCHK(hipMemcpyAsync(parents, st->bm.parent, (size_t)st->B * st->nb * 4, hipMemcpyDeviceToDevice, D.hs));
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_info(wcb_handle* h, wcb_state* st, int32_t* max_new, int32_t* steps, int32_t* done) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st);
    if (max_new) *max_new = st->max_new;
    if (steps) *steps = st->steps;
    if (done) {   // the device's all-finished flag (I_DONE: the step at which every utterance / row was done)
      int v = 0;
      HIPCHK(hipMemcpyAsync(&v, D.ints.as<int>() + I_DONE, 4, hipMemcpyDeviceToHost, D.hs));
      HIPCHK(hipStreamSynchronize(D.hs));
      *done = v > 0 ? 1 : 0;
    }
  });
}

int wcb_decode_result(wcb_handle* h, wcb_state* st, int32_t* out_ids, int out_ld, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, out_ids && out_steps, "bad argument");
    REQUIRE(st->fwd == 0, "wcb_decode_result on a forward cache (wcb_forward_cached state)");
    int* ints = D.ints.as<int>();
    sync_in(h, stream, D.hs);
    int n = st->steps;
    if (st->nb > 1) {   // the best finished sequence of every utterance so far (generate()'s beam output)
      HIPCHK(hipMemsetAsync(ints + I_UNFIN, 0, 4, D.hs));
      beam_output(st->bm, D.hs);
      int olen = 0;
      HIPCHK(hipMemcpyAsync(&olen, ints + I_UNFIN, 4, hipMemcpyDeviceToHost, D.hs));
      HIPCHK(hipStreamSynchronize(D.hs));
      n = std::min(olen, st->max_new);
    }
    // the library's output rows are st->max_new wide; the caller's out_ld columns must hold the n generated
    REQUIRE(out_ld >= n && out_ld >= 1, "wcb_decode_result: out_ld " + std::to_string(out_ld) + " < the " +
                                            std::to_string(n) + " generated columns (wcb_decode_info gives the width)");
    if (n > 0)
      HIPCHK(hipMemcpy2DAsync(out_ids, (size_t)out_ld * 4, D.outbuf.p, (size_t)st->max_new * 4, (size_t)n * 4,
                              st->B, hipMemcpyDeviceToDevice, D.hs));
    *out_steps = n;
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_enable_logprobs(wcb_handle* h, wcb_state* st) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st);
    if (st->nb > 1) throw WcbError(WCB_ERR_UNSUPPORTED, "token log-probs are greedy only (a beam-search state)");
    if (st->fwd != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_logprobs on a forward cache (wcb_forward_cached state)");
    if (st->steps != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_logprobs: after the first step (right after wcb_decode_begin)");
    ensure_lp_ws(h, D, st->B, st->max_new);
    HIPCHK(hipMemsetAsync(D.lpbuf.p, 0, (size_t)st->B * st->max_new * 4, D.hs));
    st->logprobs = true;
  });
}

int wcb_decode_enable_no_speech(wcb_handle* h, wcb_state* st) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st);
    if (st->nb > 1) throw WcbError(WCB_ERR_UNSUPPORTED, "the no-speech probability is greedy only (a beam-search state)");
    if (st->fwd != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_no_speech on a forward cache (wcb_forward_cached state)");
    if (st->steps != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_no_speech: after the first step (right after wcb_decode_begin)");
    if (!st->logprobs) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_no_speech: enable the token log-probs first (wcb_decode_enable_logprobs)");
    D.nsp.ensure((size_t)kWinRows * 4);
    st->no_speech = true;
  });
}

int wcb_decode_no_speech(wcb_handle* h, wcb_state* st, float* out, void* stream) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, out, "bad argument");
    if (!st->no_speech) throw WcbError(WCB_ERR_STATE, "wcb_decode_no_speech: off (wcb_decode_enable_no_speech)");
    if (st->steps < 1) throw WcbError(WCB_ERR_STATE, "wcb_decode_no_speech: before the first step");
    sync_in(h, stream, D.hs);
    HIPCHK(hipMemcpyAsync(out, D.nsp.p, (size_t)st->B * 4, hipMemcpyDeviceToDevice, D.hs));
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_enable_sampling(wcb_handle* h, wcb_state* st, float temperature, const uint64_t* seeds) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st);
    check_sampling(temperature, seeds);
    if (st->nb > 1) throw WcbError(WCB_ERR_UNSUPPORTED, "sampling is greedy only (a beam-search state)");
    if (h->rules_on && h->rules_ts.on)
      throw WcbError(WCB_ERR_UNSUPPORTED, "timestamp decoding with sampling is not supported (greedy only)");
    if (st->rep.seen) throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules with sampling are not supported (greedy only)");
    if (st->fwd != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_sampling on a forward cache (wcb_forward_cached state)");
    if (st->steps != 0) throw WcbError(WCB_ERR_STATE, "wcb_decode_enable_sampling: after the first step (right after wcb_decode_begin)");
    install_sampling(D, temperature, seeds, st->B);
    st->sampling = true;
  });
}

int wcb_decode_logprobs(wcb_handle* h, wcb_state* st, float* out, int out_ld, int32_t* out_steps, void* stream) {
  return guarded(h, [&] {
    DecCtx& D = step_ctx(h, st, out && out_steps, "bad argument");
    if (!st->logprobs) throw WcbError(WCB_ERR_STATE, "wcb_decode_logprobs: log-probs are off (wcb_decode_enable_logprobs)");
    const int n = st->steps;
    REQUIRE(out_ld >= n && out_ld >= 1, "wcb_decode_logprobs: out_ld " + std::to_string(out_ld) + " < the " +
                                            std::to_string(n) + " steps taken");
    sync_in(h, stream, D.hs);
    if (n > 0)
      HIPCHK(hipMemcpy2DAsync(out, (size_t)out_ld * 4, D.lpbuf.p, (size_t)st->max_new * 4, (size_t)n * 4, st->B,
                              hipMemcpyDeviceToDevice, D.hs));
    *out_steps = n;
    sync_out(h, stream, D.hs);
  });
}

int wcb_decode_end(wcb_handle* h, wcb_state* st) {
  return guarded(h, [&] {
    HIPCHK(hipStreamSynchronize(step_ctx(h, st).hs));
    check_dev_err(h);
    h->step_state = nullptr;
    delete st;
  });
}

int wcb_synchronize(wcb_handle* h) {
  return guarded(h, [&] {
    REQUIRE(h, "null handle");
    quiesce(h);
    HIPCHK(hipGetLastError());
    check_dev_err(h);
  });
}

// Teacher forcing: the encoder output of `mel` (wcb_forward; also into enc_out when given) or the given one in its
// place (wcb_forward_enc: the same buffer or the same cross-K/V GEMM over it, so the logits are equal bit for bit)
// into the next decode context, then a causal prefill of positions 0 .. T-1 of every row, logits of every position
static void forward_impl(wcb_handle* h, const float* mel, const void* enc, void* enc_out, int B, const int32_t* dec_ids,
                         int T, float* logits, void* stream) {
  REQUIRE(h && (mel || enc) && dec_ids && logits && B > 0 && T > 0, "bad argument");
  if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
  REQUIRE(B <= 64, "batch > 64 per handle");
  REQUIRE(T <= h->d.n_text_ctx, "decoder_input_ids longer than max_target_positions");
  if (mel) ensure_enc_ws(h, B);
  ensure_dec_ws(h, B, B, T, 1, h->xmode, prefill_rows(B, T));
  const int buf = h->gen_count++ % h->nctx;
  DecCtx& D = h->dc[buf];
  sync_in(h, stream, h->he);
  HIPCHK(hipStreamWaitEvent(h->he, h->ev_dec[buf], 0));
  if (mel) {
    enc_out = enc_out ? enc_out : h->encout.p;
    encode_impl(h, mel, B, enc_out);
    enc = enc_out;
  }
  enc_to_ctx(h, buf, enc, B, h->xmode, h->he, stream);
  HIPCHK(hipStreamWaitEvent(D.hs, h->ev_xkv[buf], 0));
  HIPCHK(hipMemsetAsync(D.ints.p, 0, RowInts::words(B) * 4, D.hs));
  StepCfg sc = step_cfg(h, buf, B, T, 1);
  sc.lm_head = true;
  sc.logits_ld = (long)T * h->d.vocab;   // the caller's [B][T][V]: a pass writes positions p0 .. of every row
  prefill_range(h, sc, dec_ids, T, 0, T, [&](StepCfg& c, int p0, int) { c.logits_out = logits + (size_t)p0 * h->d.vocab; });
  HIPCHK(hipEventRecord(h->ev_dec[buf], D.hs));
  sync_out(h, stream, D.hs);
}

int wcb_forward(wcb_handle* h, const float* mel, int B, const int32_t* dec_ids, int T, float* logits, void* enc_out,
                void* stream) {
  return guarded(h, [&] {
    REQUIRE(mel, "bad argument");
    forward_impl(h, mel, nullptr, enc_out, B, dec_ids, T, logits, stream);
  });
}

int wcb_forward_enc(wcb_handle* h, const void* enc, int B, const int32_t* dec_ids, int T, float* logits, void* stream) {
  return guarded(h, [&] {
    REQUIRE(enc, "bad argument");
    forward_impl(h, nullptr, enc, nullptr, B, dec_ids, T, logits, stream);
  });
}

// ---- token-level timestamps (wcb.h)
static void check_median_width(int W) {
  REQUIRE(W >= 1 && (W & 1), "median_width must be odd and positive");
  if (W > 15) throw WcbError(WCB_ERR_UNSUPPORTED, "median_width above 15 is not supported");
}

int wcb_align(wcb_handle* h, const void* enc, int B, const int32_t* ids, int ld, int n, const int32_t* prefix,
              int prefix_len, const wcb_align_cfg* cfg, int32_t* out_frames, float* matrix_out, void* stream) {
  return guarded(h, [&] {
    REQUIRE(h && ids && cfg && out_frames && B > 0 && n > 0 && ld >= n, "bad argument");
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    REQUIRE(B <= 64, "batch > 64 per handle: split the batch");
    const int P = prefix ? prefix_len : 1;
    REQUIRE(P >= 1, "prefix_len must be >= 1");
    const int T = P + n - 1, nrow = n - 1, S = h->S(), L = h->d.n_layers, H = h->H();
    REQUIRE(T <= h->d.n_text_ctx, "prefix + generated ids exceed max_target_positions");
    check_median_width(cfg->median_width);
    if (S > kAlignMaxS) throw WcbError(WCB_ERR_UNSUPPORTED, "token timestamps: more than 1536 encoder positions");
    AlignPass ap;
    ap.by_layer.resize(L);
    if (cfg->heads && cfg->n_heads > 0) {
      for (int i = 0; i < cfg->n_heads; ++i) {
        const int l = cfg->heads[2 * i], hd = cfg->heads[2 * i + 1];
        REQUIRE(l >= 0 && l < L && hd >= 0 && hd < H, "alignment head (" + std::to_string(l) + ", " + std::to_string(hd) +
                                                          ") outside the model's layers / heads");
        ap.by_layer[l].push_back({hd, i});
      }
      ap.heads_total = cfg->n_heads;
    } else {   // OpenAI's default when a checkpoint names none: every head of the upper half of the layers
      for (int l = L / 2; l < L; ++l)
        for (int hd = 0; hd < H; ++hd) ap.by_layer[l].push_back({hd, ap.heads_total++});
    }
    for (int l = 0; l < L; ++l) {
      REQUIRE((int)ap.by_layer[l].size() <= kAlignMaxLayerHeads, "more than 32 alignment heads in one layer");
      if (!ap.by_layer[l].empty()) ap.last_layer = l;
    }
    std::vector<int> sb(B, S);
    if (cfg->num_frames)
      for (int b = 0; b < B; ++b) {
        REQUIRE(cfg->num_frames[b] >= 2 * cfg->median_width && cfg->num_frames[b] <= 2 * S,
                "num_frames outside [2 * median_width, 2 * n_audio_ctx]");
        sb[b] = cfg->num_frames[b] / 2;
      }
    int buf, xm;
    const int rows = prefill_rows(B, T);
    if (enc) {
      xm = h->xmode;
      ensure_dec_ws(h, B, B, T, 1, xm, rows);
      buf = h->gen_count++ % h->nctx;
    } else {
      if (h->last_gen_buf < 0 || h->last_gen_id != h->gen_count)
        throw WcbError(WCB_ERR_STATE, "wcb_align(enc = NULL): no encoder state of a wcb_generate call is held");
      if (h->last_gen_B != B)
        throw WcbError(WCB_ERR_STATE, "wcb_align(enc = NULL): the latest wcb_generate call had " +
                                          std::to_string(h->last_gen_B) + " clips, this call has " + std::to_string(B));
      buf = h->last_gen_buf;
      xm = h->last_gen_xm;
      ensure_dec_ws(h, B, B, T, 1, xm, rows);   // (the encoder-side buffer already has its size: kept)
    }
    DecCtx& D = h->dc[buf];
    // workspaces (a reallocation drains the streams first: an earlier post-pass may still read them)
    const size_t per_clip = (size_t)ap.heads_total * std::max(nrow, 1) * S * 4;
    const int gsz = (int)std::min<size_t>(B, std::max<size_t>(1, h->align_ws_bytes / per_clip));
    const size_t trace_clip = dtw_trace_bytes(nrow, S);
    const bool trace_ws = trace_clip > (size_t)kDtwLdsTrace;
    const size_t need[] = {gsz * per_clip, matrix_out ? 0 : (size_t)B * std::max(nrow, 1) * S * 4, (size_t)B * T * 4,
                           (size_t)B * 4, (size_t)B * 4, (size_t)P * 4, trace_ws ? B * trace_clip : 0};
    DevBuf* have[] = {&h->al_w, &h->al_M, &h->al_tf, &h->al_lens, &h->al_frames, &h->al_prefix, &h->al_trace};
    bool grow = false;
    for (int i = 0; i < 7; ++i) grow |= need[i] > have[i]->bytes;
    if (grow) {
      quiesce(h);
      for (int i = 0; i < 7; ++i) have[i]->ensure(need[i]);
    }
    if (enc) {   // the given encoder output into the context, as wcb_forward_enc
      sync_in(h, stream, h->he);
      HIPCHK(hipStreamWaitEvent(h->he, h->ev_dec[buf], 0));
      enc_to_ctx(h, buf, enc, B, xm, h->he, stream);
      HIPCHK(hipStreamWaitEvent(D.hs, h->ev_xkv[buf], 0));
    }
    sync_in(h, stream, D.hs);   // the ids
    if (h->align_pending) HIPCHK(hipStreamWaitEvent(D.hs, h->ev_align, 0));   // the workspaces: one pass at a time
    int* tf = h->al_tf.as<int>();
    int* lens = h->al_lens.as<int>();
    int* frames = h->al_frames.as<int>();
    float* M = matrix_out ? matrix_out : h->al_M.as<float>();
    if (prefix) write_i32(h->al_prefix.as<int>(), prefix, P, D.hs);
    write_i32(frames, sb.data(), B, D.hs);
    align_prep(ids, ld, n, prefix ? h->al_prefix.as<int>() : nullptr, P, h->d.decoder_start_token_id, h->d.eos_token_id,
               h->d.vocab, B, tf, lens, D.hs);
    ap.P = P; ap.nrow = nrow; ap.w = h->al_w.as<float>();
    StepCfg sc = step_cfg(h, buf, B, T, 1);
    sc.xmode = xm;
    for (int c0 = 0; c0 < B && nrow > 0; c0 += gsz) {
      ap.clip0 = c0; ap.nclip = std::min(gsz, B - c0);
      // teacher forcing over prefix + ids, LM head off: the causal prefill of wcb_forward_enc
      HIPCHK(hipMemsetAsync(D.ints.p, 0, RowInts::words(B) * 4, D.hs));
      prefill_range(h, sc, tf, T, 0, T, [&](StepCfg& c, int p0, int np) {
        ap.pos0 = p0;
        c.align = p0 + np > P ? &ap : nullptr;   // (a pass over prefix positions alone has no row to keep)
      });
      h->timed("align_matrix", 0, (double)ap.nclip * per_clip, D.hs, [&] {
        if (!align_matrix(ap.w, ap.nclip, ap.heads_total, nrow, S, lens + c0, frames + c0, cfg->median_width,
                          M + (size_t)c0 * nrow * S, D.hs))
          throw WcbError(WCB_ERR_UNSUPPORTED, "median_width not supported");
      });
    }
    DtwArgs da;
    da.M = M; da.m_max = nrow; da.S_ld = S; da.lens = lens; da.frames = frames; da.n_out = n; da.out_frames = out_frames;
    da.trace = trace_ws ? h->al_trace.as<unsigned>() : nullptr;
    h->timed("align_dtw", 0, (double)B * nrow * S * 4, D.hs, [&] { dtw(da, B, D.hs); });
    HIPCHK(hipEventRecord(h->ev_dec[buf], D.hs));
    if (!h->ev_align) HIPCHK(hipEventCreateWithFlags(&h->ev_align, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_align, D.hs));
    h->align_pending = true;
    sync_out(h, stream, D.hs);
  });
}

int wcb_op_align_capture(int dtype, const void* q, long ldq, int q_hstride, const void* keys, int layout, int clips,
                         int H, int dim, int S, int rps, int pos0, int P, int nrow, int clip0, int nclip,
                         const int32_t* heads, int nh, float* w, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(q && keys && heads && w && clips > 0 && H > 0 && rps > 0 && nrow > 0 && P >= 1 && pos0 >= 0, "bad argument");
    REQUIRE(dtype >= 0 && dtype <= 2 && layout >= 0 && layout <= 2, "dtype 0..2, layout 0..2");
    REQUIRE(clip0 >= 0 && nclip > 0 && clip0 + nclip <= clips, "clip range outside the batch");
    REQUIRE(nh >= 1 && nh <= kAlignMaxLayerHeads, "1..32 heads");
    REQUIRE(S >= 1 && S <= kAlignMaxS, "S must be in [1, 1536]");
    REQUIRE(layout == 0 ? dim == 64 : dim % 32 == 0 && dim >= 32, "dim: 64 against the K cache, a multiple of 32 otherwise");
    REQUIRE(q_hstride >= dim && ldq >= (long)q_hstride, "q strides");
    if (layout == 2 && !xenc_supported((DType)dtype, dim))
      throw WcbError(WCB_ERR_UNSUPPORTED, "no fragment-major encoder layout for this dtype / width");
    hipStream_t st = (hipStream_t)stream;
    AlignCapArgs a;
    a.q = q; a.ldq = ldq; a.q_hstride = q_hstride; a.k = keys; a.xmode = layout != 0; a.dim = dim; a.S = S;
    a.k_clip = layout == 0 ? (long)H * S * 64 : (long)S * dim;
    DevBuf fm;
    if (layout == 2) {
      fm.ensure((size_t)xenc_fm_elems(clips, S, dim) * 2);
      xenc_to_fm((DType)dtype, keys, fm.p, clips, S, dim, st);
      a.k = fm.p; a.fm = 1; a.k_clip = xenc_fm_elems(1, S, dim);
    }
    a.rps = rps; a.pos0 = pos0; a.P = P; a.nrow = nrow; a.clip0 = clip0; a.nclip = nclip; a.nh = nh; a.heads_total = nh;
    for (int i = 0; i < nh; ++i) {
      REQUIRE(heads[i] >= 0 && heads[i] < H, "head outside [0, H)");
      a.head[i] = heads[i]; a.slot[i] = i;
    }
    a.w = w;
    align_capture((DType)dtype, a, st);
    const hipError_t e = hipStreamSynchronize(st);
    fm.release();
    HIPCHK(e);
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_align_matrix(const float* w, int N, int heads, int m_max, int S_ld, const int32_t* lens, const int32_t* frames,
                        int median_width, float* M, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(w && lens && M && N > 0 && heads > 0 && S_ld > 0, "bad argument");
    REQUIRE(m_max >= 1 && m_max <= kAlignMaxRows, "m_max must be in [1, 447]");
    check_median_width(median_width);
    if (!align_matrix(w, N, heads, m_max, S_ld, lens, frames, median_width, M, (hipStream_t)stream))
      throw WcbError(WCB_ERR_UNSUPPORTED, "median_width not supported");
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_dtw(const float* M, int N, int m_max, int S_ld, const int32_t* lens, const int32_t* frames, int n_out,
               int32_t* out_frames, int32_t* path_text, int32_t* path_time, int32_t* path_len, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(M && lens && out_frames && N > 0 && S_ld > 0 && n_out >= m_max, "bad argument (n_out >= m_max)");
    REQUIRE(m_max >= 1 && m_max <= kAlignMaxRows, "m_max must be in [1, 447]");
    REQUIRE(!path_text == !path_time && (!path_text || path_len), "path_text, path_time and path_len go together");
    DevBuf trace;
    const size_t tb = dtw_trace_bytes(m_max, S_ld);
    if (tb > (size_t)kDtwLdsTrace) trace.ensure((size_t)N * tb);
    DtwArgs a;
    a.M = M; a.m_max = m_max; a.S_ld = S_ld; a.lens = lens; a.frames = frames; a.n_out = n_out; a.out_frames = out_frames;
    a.trace = trace.as<unsigned>();
    a.path_text = path_text; a.path_time = path_time; a.path_len = path_len; a.path_ld = m_max + S_ld;
    hipError_t e = hipSuccess;
    dtw(a, N, (hipStream_t)stream);
    e = hipStreamSynchronize((hipStream_t)stream);
    trace.release();
    HIPCHK(e);
    HIPCHK(hipGetLastError());
  });
}

int wcb_dtw_host(const float* M, int m, int S, long ld, int32_t* frames, int n_out, int32_t* path_text, int32_t* path_time,
                 int32_t* path_len) {
  return guarded(nullptr, [&] {
    REQUIRE(M && frames && m >= 0 && S >= 1 && ld >= S && n_out > 0, "bad argument");
    REQUIRE(!path_text == !path_time && (!path_text || path_len), "path_text, path_time and path_len go together");
    for (int i = 0; i < n_out; ++i) frames[i] = 0;
    if (path_len) *path_len = 0;
    if (m == 0) return;
    // two cost columns' worth of state would do; the rows are kept whole for clarity: prev = cost[i-1][·]
    std::vector<float> prev((size_t)S + 1, INFINITY), cur((size_t)S + 1);
    std::vector<uint8_t> trace((size_t)m * S);
    prev[0] = 0.f;
    for (int i = 1; i <= m; ++i) {
      cur[0] = INFINITY;
      for (int j = 1; j <= S; ++j)
        trace[(size_t)(i - 1) * S + j - 1] =
            (uint8_t)dtw_cell(prev[j - 1], prev[j], cur[j - 1], M[(size_t)(i - 1) * ld + j - 1], cur[j]);
      std::swap(prev, cur);
    }
    int i = m, j = S, len = 0, last = 0;
    while (i > 0 || j > 0) {
      if (path_text) { path_text[len] = i - 1; path_time[len] = j - 1; }
      ++len;
      if (i >= 1 && i - 1 < n_out) frames[i - 1] = j - 1;
      if (i == m) last = j - 1;
      const int stored = (i > 0 && j > 0) ? trace[(size_t)(i - 1) * S + j - 1] : 0;
      dtw_back(dtw_border(i, j, stored), i, j);
    }
    if (m <= 1) last = 0;
    for (int r = m; r < n_out; ++r) frames[r] = last;
    if (path_text) {
      std::reverse(path_text, path_text + len);
      std::reverse(path_time, path_time + len);
    }
    if (path_len) *path_len = len;
  });
}

int wcb_forward_cached(wcb_handle* h, wcb_state* st, const int32_t* dec_ids, int T, float* logits, void* stream) {
  return guarded(h, [&] {
    step_ctx(h, st, dec_ids && logits && T > 0, "bad argument (state of this handle, dec_ids, logits, T > 0)");
    REQUIRE(st->steps == 0, "wcb_forward_cached on a state that wcb_decode_step has advanced");
    REQUIRE(st->P == 1, "wcb_forward_cached needs a state begun without a prefix");
    REQUIRE(st->fwd + T <= st->T, "past_key_values + decoder_input_ids exceed max_target_positions");
    const int ci = wcb_handle::kMaxCtx - 1, B = st->B;
    ensure_dec_ws(h, B, B, st->T, st->max_new, st->xmode, prefill_rows(B, T), ci, ci + 1);
    DecCtx& D = h->dc[ci];
    sync_in(h, stream, D.hs);
    // the new ids at their absolute positions of the [B][T] forced buffer (prefill_ids reads src[b·T + pos])
    if ((size_t)B * st->T * 4 > D.forced.bytes) { quiesce(h); D.forced.ensure((size_t)B * st->T * 4); }
    HIPCHK(hipMemcpy2DAsync(D.forced.as<int>() + st->fwd, (size_t)st->T * 4, dec_ids, (size_t)T * 4, (size_t)T * 4, B,
                            hipMemcpyDeviceToDevice, D.hs));
    StepCfg sc = step_cfg(h, ci, B, st->T, 1);
    sc.lm_head = true;
    sc.logits_ld = (long)T * h->d.vocab;   // the caller's [B][T][V], as wcb_forward
    sc.clips = B;
    sc.xmode = st->xmode;
    prefill_range(h, sc, D.forced.as<int>(), st->T, 0, T,
                  [&](StepCfg& c, int p0, int) { c.logits_out = logits + (size_t)p0 * h->d.vocab; });
    st->fwd += T;
    sync_out(h, stream, D.hs);
  });
}

// ------------------------------------------------------------------------------ bias automaton
// Aho-Corasick automaton of phrases [p0, p1) (phrase p = tokens[offsets[p] .. offsets[p + 1])), states
// numbered from 0 = its root: trie depth and keep per state, trans(s) as CSR (local state ids), and the
// gated root children (token, depth-1 state) in ascending token order.
extern "C++" {
namespace {
struct HostAc {
  std::vector<int> depth, keep, off, tok, dst;
  std::vector<std::pair<int, int>> rc;
};
HostAc build_ac(const int32_t* tokens, const int32_t* offsets, int p0, int p1, int V, const uint8_t* word_start) {
    // trie
    std::vector<std::map<int, int>> ch(1);
    std::vector<int> depth(1, 0);
    std::vector<char> end(1, 0);
    for (int p = p0; p < p1; ++p) {
      int s = 0;
      REQUIRE(offsets[p + 1] >= offsets[p], "offsets must be non-decreasing");
      for (int i = offsets[p]; i < offsets[p + 1]; ++i) {
        const int v = tokens[i];
        REQUIRE(v >= 0 && v < V, "bias token id out of range");
        auto it = ch[s].find(v);
        if (it == ch[s].end()) {
          ch.emplace_back();
          depth.push_back(depth[s] + 1);
          end.push_back(0);
          const int nn = (int)ch.size() - 1;
          ch[s][v] = nn;
          s = nn;
        } else {
          s = it->second;
        }
      }
      if (s) end[s] = 1;
    }
    const int ns = (int)ch.size();
    std::vector<int> fail(ns, 0), keep(ns, 0), order;
    order.reserve(ns);
    std::deque<int> q;
    for (auto& kv : ch[0]) {
      fail[kv.second] = 0;
      keep[kv.second] = end[kv.second] ? 1 : 0;
      q.push_back(kv.second);
    }
    while (!q.empty()) {
      const int s = q.front();
      q.pop_front();
      order.push_back(s);
      for (auto& kv : ch[s]) {
        keep[kv.second] = end[kv.second] ? depth[kv.second] : keep[s];
        int f = fail[s];
        while (f && !ch[f].count(kv.first)) f = fail[f];
        auto it = ch[f].find(kv.first);
        fail[kv.second] = (it != ch[f].end() && it->second != kv.second) ? it->second : 0;
        q.push_back(kv.second);
      }
    }
    // trans(s): every token whose transition from s lands at depth >= 2 (root children are the
    // vocabulary-wide bitmap). Walk the failure chain; the first (deepest) state owning the token wins.
    std::vector<int> off(ns + 1, 0), tok, dst;
    for (int s = 0; s < ns; ++s) {
      std::map<int, int> t;
      for (int f = s; f != 0; f = fail[f])
        for (auto& kv : ch[f])
          if (!t.count(kv.first)) t[kv.first] = kv.second;
      for (auto& kv : t)
        if (depth[kv.second] >= 2) { tok.push_back(kv.first); dst.push_back(kv.second); }
      off[s + 1] = (int)tok.size();
    }
    // root children: a match may START only at a word-start token (word_start == null: any token)
    HostAc ac;
    for (auto& kv : ch[0])
      if (!word_start || word_start[kv.first]) ac.rc.emplace_back(kv.first, kv.second);
    ac.depth = std::move(depth); ac.keep = std::move(keep);
    ac.off = std::move(off); ac.tok = std::move(tok); ac.dst = std::move(dst);
    return ac;
}
}  // namespace
}  // extern "C++"

int wcb_bias_create(wcb_handle* h, const int32_t* tokens, const int32_t* offsets, int n_phrases,
                    const uint8_t* word_start, wcb_bias** out) {
  return guarded(h, [&] {
    REQUIRE(h && out && n_phrases >= 0 && (n_phrases == 0 || (tokens && offsets)), "bad argument");
    const int V = h->d.vocab;
    const HostAc ac = build_ac(tokens, offsets, 0, n_phrases, V, word_start);
    const int ns = (int)ac.depth.size();
    const std::vector<int>&depth = ac.depth, &keep = ac.keep, &off = ac.off, &tok = ac.tok, &dst = ac.dst;
    std::vector<uint32_t> bits((V + 31) / 32, 0u);
    std::vector<int> rc(V, -1);
    for (auto& kv : ac.rc) {
      bits[kv.first >> 5] |= 1u << (kv.first & 31);
      rc[kv.first] = kv.second;
    }
    auto b = std::make_unique<wcb_bias>();
    b->n_states = ns;
    b->vocab = V;
    b->id = g_next_bias_id.fetch_add(1);   // process-wide: a graph key never names another handle's bias
    b->owner = h;
    HIPCHK(hipSetDevice(h->device));
    b->root_bits.ensure(bits.size() * 4);
    HIPCHK(hipMemcpy(b->root_bits.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
    b->root_child.ensure(rc.size() * 4);
    HIPCHK(hipMemcpy(b->root_child.p, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    b->trans_off.ensure(off.size() * 4);
    HIPCHK(hipMemcpy(b->trans_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    b->trans_tok.ensure(std::max<size_t>(tok.size(), 1) * 4);
    b->trans_dst.ensure(std::max<size_t>(dst.size(), 1) * 4);
    if (!tok.empty()) {
      HIPCHK(hipMemcpy(b->trans_tok.p, tok.data(), tok.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(b->trans_dst.p, dst.data(), dst.size() * 4, hipMemcpyHostToDevice));
    }
    b->st_depth.ensure((size_t)ns * 4);
    b->st_keep.ensure((size_t)ns * 4);
    HIPCHK(hipMemcpy(b->st_depth.p, depth.data(), (size_t)ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->st_keep.p, keep.data(), (size_t)ns * 4, hipMemcpyHostToDevice));
    h->biases.push_back(b.get());
    *out = b.release();
  });
}

// Lifetime (wcb.h): the decode graphs of the owning handle capture the automaton's device buffers.
// Destroying it waits for the handle's queued work and drops those graphs (they are re-captured by
// the next wcb_generate), so a graph can never replay reads of freed memory.
void wcb_bias_destroy(wcb_bias* b) {
  if (!b) return;
  if (wcb_handle* h = b->owner) {
    (void)hipSetDevice(h->device);
    try {
      quiesce(h);
    } catch (...) {
    }
    const std::string id = "/" + std::to_string(b->id) + "/";
    for (DecCtx& D : h->dc)
      for (const StepGraphs& g : D.graphs)
        if (g.key.find(id) != std::string::npos) { D.drop_graphs(); break; }
    h->biases.erase(std::remove(h->biases.begin(), h->biases.end(), b), h->biases.end());
  }
  for (DevBuf* x : {&b->root_bits, &b->root_child, &b->trans_off, &b->trans_tok, &b->trans_dst, &b->st_depth, &b->st_keep})
    x->release();
  delete b;
}

int wcb_bias_num_states(const wcb_bias* b) { return b ? b->n_states : 0; }

// ---- per-utterance bias lists: B automata in one state space (host data; wcb.h wcb_bias_batch)
int wcb_bias_batch_create(wcb_handle* h, int B, const int32_t* tokens, const int32_t* phrase_off, const int32_t* clip_off,
                          const uint8_t* word_start, wcb_bias_batch** out) {
  return guarded(h, [&] {
    REQUIRE(h && out && clip_off, "bad argument (handle, clip_off and out are required)");
    REQUIRE(B >= 1 && B <= kForestClips, "bias batch: 1 <= B <= 64");
    const int V = h->d.vocab;
    REQUIRE(clip_off[0] >= 0, "clip_off must start at >= 0");
    for (int b = 0; b < B; ++b) REQUIRE(clip_off[b + 1] >= clip_off[b], "clip_off must be non-decreasing");
    const int P = clip_off[B];
    REQUIRE(P == 0 || (tokens && phrase_off), "bad argument (tokens and phrase_off are required with phrases)");
    if (P) REQUIRE(phrase_off[0] >= 0, "phrase_off must start at >= 0");
    for (int p = 0; p < P; ++p) REQUIRE(phrase_off[p + 1] >= phrase_off[p], "phrase_off must be non-decreasing");
    auto bb = std::make_unique<wcb_bias_batch>();
    bb->B = B;
    bb->vocab = V;
    bb->rc_off.push_back(0);
    bb->trans_off.push_back(0);
    for (int b = 0; b < B; ++b) {
      const HostAc ac = build_ac(tokens, phrase_off, clip_off[b], clip_off[b + 1], V, word_start);
      const int s0 = (int)bb->st_depth.size(), t0 = (int)bb->trans_tok.size(), ns = (int)ac.depth.size();
      bb->root.push_back(s0);
      bb->n_states.push_back(ns);
      bb->st_depth.insert(bb->st_depth.end(), ac.depth.begin(), ac.depth.end());
      bb->st_keep.insert(bb->st_keep.end(), ac.keep.begin(), ac.keep.end());
      for (int s = 1; s <= ns; ++s) bb->trans_off.push_back(t0 + ac.off[s]);
      bb->trans_tok.insert(bb->trans_tok.end(), ac.tok.begin(), ac.tok.end());
      for (int d : ac.dst) bb->trans_dst.push_back(s0 + d);
      for (auto& kv : ac.rc) { bb->rc_tok.push_back(kv.first); bb->rc_dst.push_back(s0 + kv.second); }
      bb->rc_off.push_back((int)bb->rc_tok.size());
    }
    *out = bb.release();
  });
}

void wcb_bias_batch_destroy(wcb_bias_batch* bb) { delete bb; }

int wcb_bias_batch_num_states(const wcb_bias_batch* bb, int clip) {
  if (!bb) return 0;
  if (clip < 0) return (int)bb->st_depth.size();
  return clip < bb->B ? bb->n_states[clip] : 0;
}

int wcb_debug_counter(const wcb_handle* h, const char* name, int64_t* out) {
  if (!h || !name || !out) return WCB_ERR_ARG;
  if (!strcmp(name, "graph_captures")) { *out = h->n_graph_captures; return WCB_OK; }
  return WCB_ERR_ARG;
}

int wcb_debug_copy(wcb_handle* h, const char* name, void* dst, int64_t bytes, int enc_layers) {
  return guarded(h, [&] {
    REQUIRE(h && name, "bad argument");
    h->dbg_enc_layers = enc_layers;
    const std::map<std::string, DevBuf*> bufs = {{"xt", &h->xt}, {"hbuf", &h->hbuf}, {"x", &h->x}, {"h", &h->h},
                                                 {"qkv", &h->qkv}, {"att", &h->att}, {"ffn", &h->ffn},
                                                 {"encout", &h->encout}, {"xkv", &h->xkv2[0]},
                                                 {"logits", &h->dc[0].logits},
                                                 {"step_logits", &h->dc[wcb_handle::kMaxCtx - 1].logits}};
    if (bytes == 0) return;   // only set the layer limit
    REQUIRE(dst, "null dst");
    auto it = bufs.find(name);
    REQUIRE(it != bufs.end(), std::string("unknown buffer ") + name);
    REQUIRE((size_t)bytes <= it->second->bytes, "bytes exceeds buffer size");
    quiesce(h);
    HIPCHK(hipMemcpy(dst, it->second->p, (size_t)bytes, hipMemcpyDeviceToDevice));
  });
}

int wcb_profile_enable(wcb_handle* h, int enable) {
  return guarded(h, [&] {
    REQUIRE(h, "null handle");
    quiesce(h);
    h->prof_collect();
    h->prof = (enable & 1) != 0;          // HIP events around front-end / encoder launches
    h->prof_stamps = (enable & 2) != 0;   // device stamps in the decode cross-attention (graph nodes)
    h->prof_e.clear();
    h->xattn_bytes = h->xattn_flops = 0;
    if (h->prof_stamps) {
      const size_t sb = (size_t)h->nctx * wcb_handle::kStampRegions * h->stamp_slots() * 16 * kStampSub;
      h->stamps.ensure(sb);
      h->stamp_acc.ensure(16 * wcb_handle::kStampRegions);
      HIPCHK(hipMemsetAsync(h->stamps.p, 0, sb, nullptr));
      HIPCHK(hipMemsetAsync(h->stamp_acc.p, 0, 16 * wcb_handle::kStampRegions, nullptr));
      HIPCHK(hipStreamSynchronize(nullptr));
    }
  });
}

int wcb_profile_read(wcb_handle* h, int n, char (*names)[32], int64_t* launches, double* ms, double* flops, double* bytes) {
  int count = 0;
  const int rc = guarded(h, [&] {
    REQUIRE(h, "null handle");
    h->prof_collect();
    if (h->prof_stamps && h->stamp_acc.p) {   // decode cross-attention + lean projections: device-stamped launches
      quiesce(h);
      unsigned long long acc[2 * wcb_handle::kStampRegions] = {};
      HIPCHK(hipMemcpy(acc, h->stamp_acc.p, sizeof(acc), hipMemcpyDeviceToHost));
      if (acc[1]) {
        const int id = h->prof_id("dec_xattn");
        h->prof_e[id].launches = (int64_t)acc[1];
        h->prof_e[id].ms = (double)acc[0] / 1e5;   // 100 MHz s_memrealtime ticks
        h->prof_e[id].bytes = h->xattn_bytes;
        h->prof_e[id].flops = h->xattn_flops;
      }
      for (int r = 1; r < wcb_handle::kStampRegions; ++r) {
        if (!acc[2 * r + 1]) continue;
        const int id = h->prof_id((std::string(kLeanStampClass[r]) + "@graph").c_str());
        h->prof_e[id].launches = (int64_t)acc[2 * r + 1];
        h->prof_e[id].ms = (double)acc[2 * r] / 1e5;
      }
    }
    for (size_t i = 0; i < h->prof_e.size() && (int)i < n; ++i) {
      snprintf(names[i], 32, "%s", h->prof_e[i].name.c_str());
      launches[i] = h->prof_e[i].launches;
      ms[i] = h->prof_e[i].ms;
      flops[i] = h->prof_e[i].flops;
      bytes[i] = h->prof_e[i].bytes;
    }
    count = (int)h->prof_e.size();
  });
  return rc == WCB_OK ? count : rc;
}

int wcb_profile_kernel(wcb_handle* h, int i, char* name, int cap, int64_t* grid) {
  return guarded(h, [&] {
    REQUIRE(h && name && cap > 0, "bad argument");
    REQUIRE(i >= 0 && i < (int)h->prof_e.size(), "profile entry out of range");
    const ProfEntry& e = h->prof_e[i];
    std::string nm;
    if (e.fn) {
      const char* raw = hipKernelNameRefByPtr(e.fn, nullptr);
      if (raw) {
        int st = 0;
        char* dm = abi::__cxa_demangle(raw, nullptr, nullptr, &st);
        nm = (st == 0 && dm) ? dm : raw;
        free(dm);
      }
    }
    snprintf(name, (size_t)cap, "%s", nm.c_str());
    if (grid) *grid = e.grid;
  });
}

// ------------------------------------------------------------------------------ kernel-level ops
int wcb_op_gemm_kernel(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act,
                       const float* resid, void* out, int out_f32, int kernel, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(A && W && out && M > 0 && N > 0 && K > 0, "bad argument");
    REQUIRE(N % 8 == 0, "N must be a multiple of 8");
    REQUIRE(K % (dtype == WCB_F32 ? 32 : 64) == 0, "K must be a multiple of the 128-byte K tile");
    REQUIRE((kernel >= 0 && kernel <= 7 && kernel != 3) || kernel == 106 || kernel == 107 ||
            (kernel % 100 >= 11 && kernel % 100 <= 52 && kernel < 200),
            "kernel: 0, 1, 2, 4, 5, 6, 7 or a wide tile config 11-52 (+100 on 6, 7 and the wide configs: W fragment-major)");
    const bool wfm = kernel >= 100;
    kernel %= 100;
    GemmArgs g = rowgemm(A, K, W, M, N, K, out, N);
    g.bias = bias; g.act = act; g.resid = resid; g.out_f32 = out_f32;
    g.raster = 8;
    if (kernel >= 6) {   // the decode-row (beam) tiles: 6 / 7 = LDS-ring tiles (7: row panels outer, the
                         // runtime's order before option beam_raster), 10·FM + FN = gemm_wide_kernel
      REQUIRE(M > 64 && dtype != WCB_F32, "decode-row tiles: 16-bit, M > 64");
      g.tile = 2; g.ring_kt = 2;
      if (kernel == 7) g.raster = 0;
      if (kernel <= 7 && wfm) g.W_fm = W;
      if (kernel > 7) {
        g.wide = kernel;
        if (wfm) g.W_fm = W;
        REQUIRE(!resid || resid == out, "wide tiles: the residual is updated in place (resid == out)");
      }
    } else {
      g.pp = kernel;
    }
    gemm(DType(dtype), g, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_gemm(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int act,
                const float* resid, void* out, int out_f32, void* stream) {
  return wcb_op_gemm_kernel(dtype, A, W, M, N, K, bias, act, resid, out, out_f32, 1, stream);
}

int wcb_op_gemm_ln(int dtype, const float* X, const float* ln_w, const float* ln_b, const float* stats,
                   const void* W, int M, int N, int K, const float* bias, int act, void* out, int out_f32, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(X && ln_w && ln_b && stats && W && out && M > 0 && M <= 64 && N > 0 && K % 16 == 0, "bad argument");
    GemmArgs g = rowgemm(X, K, W, M, N, K, out, N);
    g.ln_w = ln_w; g.ln_b = ln_b; g.st_in = stats; g.st_nb = K / 16;
    g.bias = bias; g.act = act; g.out_f32 = out_f32;
    gemm(DType(dtype), g, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_embed(int dtype, const void* tok_emb, const void* pos_emb, const int32_t* ids, const int32_t* pos,
                 const int32_t* pos_off, int M, int d, int V, int n_pos, int rps, float* x, void* x16, void* x16fm,
                 float* stats, int st_w, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(tok_emb && pos_emb && ids && pos && x, "bad argument (tables, ids, pos and x are required)");
    REQUIRE(dtype >= WCB_BF16 && dtype <= WCB_F32, "dtype");
    REQUIRE(M > 0 && d > 0 && V > 0 && n_pos > 0 && rps >= 1 && M % rps == 0, "bad shape (M a multiple of rps)");
    REQUIRE(!stats || ((st_w == 16 || st_w == 32) && d % st_w == 0), "stats: st_w 16 or 32, d a multiple of it");
    int nw = 0, kpw = 0;
    if (x16fm && (dtype == WCB_F32 || !lean_cfg(d, nw, kpw)))
      throw WcbError(WCB_ERR_UNSUPPORTED, "x16fm: 16-bit, d in the lean table (64, 512 .. 5120)");
    // step_embed / prefill_step: the same call, the caller's buffers in place of the decode context's
    embed(DType(dtype), tok_emb, pos_emb, ids, pos, x, stats, M, d, (hipStream_t)stream, x16, V, rps, stats ? st_w : 16,
          x16fm, pos_off, n_pos);
    HIPCHK(hipGetLastError());
  });
}

// One projection launch of decode_rows() on caller operands. The GemmArgs fields are the ones decode_rows() sets
// for the kind (QKV: the "dec_qkv" block; LN_PLAIN / XQK: "dec_xq"; LN_GELU: "dec_fc1"; RESID: "dec_out" / "dec_xo" /
// "dec_fc2"; KQ: "dec_kq"), then the ones its proj() lambda sets for the row count (> 64 rows: the fold / LayerNorm
// launch / tile / wide block; <= 64: lean, lean_fold); the derived operands are built as wcb_finalize_weights
// builds them (its fold and fm lambdas, the W_kt repack).
int wcb_op_dec_proj(const wcb_dec_proj* p, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(p, "null descriptor");
    const int kind = p->kind, path = p->path, M = p->M, N = p->N, K = p->K;
    REQUIRE(kind >= WCB_PROJ_QKV && kind <= WCB_PROJ_XQK, "kind");
    REQUIRE(path >= WCB_PATH_DEC && path <= WCB_PATH_WIDE, "path");
    REQUIRE(p->dtype >= WCB_BF16 && p->dtype <= WCB_F32, "dtype");
    REQUIRE(M > 0 && N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0 && M <= 4096, "bad shape (N % 16, K % 64, M <= 4096)");
    const bool ln = kind == WCB_PROJ_QKV || kind == WCB_PROJ_LN_PLAIN || kind == WCB_PROJ_LN_GELU || kind == WCB_PROJ_XQK;
    const bool kq = kind == WCB_PROJ_KQ || kind == WCB_PROJ_XQK;
    if (ln) REQUIRE(p->ln_w && p->ln_b && p->W && p->bias && p->x && p->out, "LN kinds: ln_w, ln_b, W, bias, x and out");
    if (kq) REQUIRE(p->Wk && p->out && N == K, "KQ / XQK: Wk and out, N = K = d_model");
    if (kind == WCB_PROJ_KQ) REQUIRE(p->a16, "KQ: the q rows (a16)");
    if (kind == WCB_PROJ_RESID)
      REQUIRE(p->W && p->bias && p->x && p->out16 && (p->a16 || p->a_fm), "RESID: W, bias, x, out16 and the A rows");
    const int rps = p->kv_rps > 1 ? p->kv_rps : 1;
    int H = 0;
    if (kind == WCB_PROJ_QKV) {
      REQUIRE(p->kv && p->pos && p->kv_B > 0 && p->kv_T > 0, "QKV: kv, pos, kv_B and kv_T");
      REQUIRE(p->n_split > 0 && p->n_split % 64 == 0 && p->n_split < N && (N - p->n_split) % 128 == 0,
              "QKV: n_split a multiple of 64, K and V of whole 64-wide heads after it");
      REQUIRE(M % rps == 0 && M / rps <= p->kv_B && rps <= p->kv_T, "QKV: M / kv_rps cache rows within kv_B");
      H = (N - p->n_split) / 128;
    }
    REQUIRE(p->ring_kt >= 0 && p->ring_kt <= 2, "ring_kt: 1 or 2");
    REQUIRE(p->xqk_nch == 0 || p->xqk_nch == 2 || p->xqk_nch == 4 || p->xqk_nch == 8 || p->xqk_nch == 16, "xqk_nch");
    // ---- what the path is defined for
    const bool lean = path >= WCB_PATH_LEAN && path <= WCB_PATH_LEAN_FOLD_FM;
    const bool fold = path == WCB_PATH_LEAN_FOLD || path == WCB_PATH_LEAN_FOLD_FM;
    const bool fm = path == WCB_PATH_LEAN_FOLD_FM;
    const bool tiled = path >= WCB_PATH_LN_RING;
    const bool tfold = path == WCB_PATH_RING_FOLD || path == WCB_PATH_WIDE;
    auto unsupported = [](const std::string& m) { throw WcbError(WCB_ERR_UNSUPPORTED, m); };
    if (p->dtype == WCB_F32 && (path != WCB_PATH_DEC || kq)) unsupported("f32: path DEC, no cross-query kinds");
    if (tiled ? (M <= 64 || kind == WCB_PROJ_KQ || kind == WCB_PROJ_XQK) : (M > 64 && kind != WCB_PROJ_KQ))
      unsupported("paths DEC / LEAN*: M <= 64 (KQ on DEC: any M); tile paths: M > 64, not KQ / XQK");
    if (lean && M > 64) unsupported("lean paths: M <= 64");
    const bool lnk = K == 512 || K == 768 || K == 1024 || K == 1280;
    if (lean && ln && !lnk) unsupported("lean LN-fused projections: K 512, 768, 1024, 1280");
    if (lean && kind == WCB_PROJ_RESID && !lnk && K != 2048 && K != 3072 && K != 4096 && K != 5120)
      unsupported("lean residual writers: K 512 .. 5120 of the lean table");
    // (RESID and KQ have no LayerNorm: on the folded lean paths they are the lean launch, as in decode_rows())
    if (kind == WCB_PROJ_XQK && !fold) unsupported("XQK: the folded lean paths");
    if (kind == WCB_PROJ_QKV && lean && rps > 1) unsupported("lean QKV: one position per row");
    if (kind == WCB_PROJ_QKV && path == WCB_PATH_WIDE) unsupported("QKV keeps the ring tiles");
    if (tfold && ln && (K > kLnfMaxK || K % 32)) unsupported("folded tiles: K <= 1280");
    if (path == WCB_PATH_WIDE && (K != 768 && K != 1024 && K != 1280)) unsupported("wide tiles: K 768, 1024, 1280");
    if (path == WCB_PATH_WIDE && kind == WCB_PROJ_RESID && N != K) unsupported("wide residual writers: N = K = d_model");
    if (p->st_out && (path != WCB_PATH_DEC || kind != WCB_PROJ_RESID)) unsupported("st_out: RESID on path DEC");
    if (p->rst_out && !(tfold && kind == WCB_PROJ_RESID && N % 32 == 0)) unsupported("rst_out: RESID on RING_FOLD / WIDE");
    if (p->out16_fm && !(fm && kind == WCB_PROJ_RESID && (N == 512 || N == 768 || N == 1024 || N == 1280)))
      unsupported("out16_fm: RESID on LEAN_FOLD_FM, N 512 .. 1280");
    if (p->out_fm && !(fm && kind == WCB_PROJ_LN_GELU && (N == 2048 || N == 3072 || N == 4096 || N == 5120)))
      unsupported("out_fm: LN_GELU on LEAN_FOLD_FM, N 2048 .. 5120");
    if (p->a_fm && !fm) unsupported("a_fm: path LEAN_FOLD_FM");
    if (fm && ln) REQUIRE(p->a_fm, "LEAN_FOLD_FM: the fragment-major rows (a_fm)");
    if (tfold && ln) REQUIRE(p->rst_in, "RING_FOLD / WIDE: the 32-column statistics (rst_in)");
    if (kind == WCB_PROJ_RESID && !p->a_fm) REQUIRE(p->a16, "RESID: a16");

    // ---- derived operands (wcb_finalize_weights' preparation code)
    const DType dt = DType(p->dtype);
    const size_t e = esize(p->dtype);
    hipStream_t st = (hipStream_t)stream;
    struct Scratch { DevBuf b; ~Scratch() { b.release(); } } wg, wgfm, wfm, ub, cb, x16b, dh, wkf, wkt, wktfm;
    auto fmcopy = [&](Scratch& s, const void* W, int n, int k) -> void* {
      int nw = 0, kpw = 0;
      if (dt == kF32 || !W || n % 16 || !lean_cfg(k, nw, kpw)) return nullptr;
      s.b.ensure((size_t)n * k * e);
      frag_major(dt, W, n, k, nw, kpw, s.b.p, st);
      return s.b.p;
    };
    const void* x16 = p->a16;
    if (ln && dt != kF32 && !x16 && !fm) {   // x16 = T(x)
      x16b.b.ensure((size_t)M * K * e);
      RepackArgs r;
      r.dst = x16b.b.p; r.src = p->x; r.n[2] = M * K; r.s[2] = 1; r.t[2] = 1;
      repack(dt, r, st);
      x16 = x16b.b.p;
    }
    const bool need_fold = ln && dt != kF32 && (fold || tfold || p->u_out || p->c_out || p->wg_out);
    if (need_fold) {   // W' = W·diag(γ), c, then u of the rounded W'
      wg.b.ensure((size_t)N * K * e); ub.b.ensure((size_t)N * 4); cb.b.ensure((size_t)N * 4);
      scale_cols(dt, p->W, N, K, p->ln_w, wg.b.p, st);
      ln_fold(dt, p->W, N, K, p->ln_w, p->ln_b, p->bias, ub.b.as<float>(), cb.b.as<float>(), st);
      ln_fold(dt, wg.b.p, N, K, nullptr, nullptr, nullptr, ub.b.as<float>(), nullptr, st);
      if (fold || path == WCB_PATH_WIDE) fmcopy(wgfm, wg.b.p, N, K);
    }
    const int d = K, Hq = K / 64;
    if (kq) {   // W_k,hᵀ: [H][d][64], element (h, c, i) = W_k[h·64 + i][c]
      wkf.b.ensure((size_t)d * d * 4); wkt.b.ensure((size_t)d * d * e);
      WeightView v;
      v.shape[3] = (long)d * d; v.stride[3] = 1;
      view_to_f32(dt, p->Wk, v, wkf.b.as<float>(), st);
      RepackArgs r;
      r.dst = wkt.b.p; r.src = wkf.b.as<float>();
      r.n[0] = Hq; r.n[1] = d; r.n[2] = 64;
      r.s[0] = 64L * d; r.s[1] = 1; r.s[2] = d;
      r.t[0] = (long)d * 64; r.t[1] = 64; r.t[2] = 1;
      repack(dt, r, st);
      if (lean) fmcopy(wktfm, wkt.b.p, Hq * d, 64);
    }

    // ---- the launch's arguments: decode_rows()' block for the kind
    GemmArgs g;
    if (kind == WCB_PROJ_KQ) {
      g = drow(p->a16, d, wkt.b.p, M, Hq * d, 64, p->out, (long)Hq * d);
      g.a_grp_n = d; g.a_grp_off = 64; g.W_fm = wktfm.b.p;
    } else if (kind == WCB_PROJ_RESID) {
      g = drow(p->a_fm ? p->a_fm : p->a16, K, p->W, M, N, K, p->x, N);
      g.bias = p->bias; g.resid = p->x; g.out_f32 = 1; g.st_out = p->st_out; g.st_nb = N / 16; g.out16 = p->out16;
      if (lean || path == WCB_PATH_WIDE) g.W_fm = fmcopy(wfm, p->W, N, K);
      g.a_fm = p->a_fm != nullptr;
      g.out16_fm = p->out16_fm;
    } else {
      const int ldc = kind == WCB_PROJ_QKV ? p->n_split : N;
      g = drow(p->x, K, p->W, M, N, K, kind == WCB_PROJ_XQK ? nullptr : p->out, ldc);
      g.ln_w = p->ln_w; g.ln_b = p->ln_b; g.st_in = p->st_in; g.st_nb = K / 16;
      g.ln_a16 = dt != kF32 ? x16 : nullptr;
      g.bias = p->bias;
      g.ln_u = ub.b.as<float>(); g.ln_c = cb.b.as<float>(); g.ln_wg = wg.b.p; g.ln_wg_fm = wgfm.b.p;
      if (lean) g.W_fm = fmcopy(wfm, p->W, N, K);
      if (kind == WCB_PROJ_QKV) {
        g.mode = 2; g.n_split = p->n_split; g.kv_out = p->kv; g.hs_B = p->kv_B; g.hs_H = H; g.kv_T = p->kv_T;
        g.pos = p->pos; g.kv_rps = rps;
      }
      if (kind == WCB_PROJ_LN_GELU) { g.act = 1; g.c_fm = p->out_fm; }
      if (fm) { g.ln_a16 = p->a_fm; g.a_fm = 1; }
      if (kind == WCB_PROJ_XQK) { g.xqk_wk = wktfm.b.p; g.xqk_out = p->out; g.hs_H = Hq; g.xqk_nch = p->xqk_nch; }
    }
    // ---- decode_rows()' proj(): > 64 rows on the tiles, else the lean switches
    if (tiled) {
      if (ln && tfold) {   // LayerNorm folded into the tile
        g.A = x16; g.lda = K; g.W = g.ln_wg; g.ldw = K; g.W_fm = g.ln_wg_fm;
        g.bias = g.ln_c; g.ln_w = g.ln_b = nullptr; g.st_in = nullptr; g.ln_a16 = nullptr;
        g.rst_in = p->rst_in; g.rst_nb = K / 32;
      } else if (ln) {     // a LayerNorm launch of its own
        g.W_fm = nullptr; g.ln_u = nullptr;
        dh.b.ensure((size_t)M * K * e);
        layernorm(dt, p->x, g.ln_w, g.ln_b, dh.b.p, M, K, st);
        g.A = dh.b.p; g.lda = K;
        g.ln_w = g.ln_b = nullptr; g.st_in = nullptr; g.ln_a16 = nullptr;
      }
      g.tile = 2; g.skinny = 0; g.ring_kt = p->ring_kt == 2 ? 2 : 1;
      if (kind == WCB_PROJ_RESID && tfold) g.rst_out = p->rst_out;
      g.a_fm = 0; g.c_fm = 0; g.out16_fm = nullptr;
      if (path == WCB_PATH_WIDE) {
        if (!g.W_fm) unsupported("wide tiles: no fragment-major weights for this shape");
        g.wide = kind == WCB_PROJ_LN_GELU ? 22 : 12;
      } else {
        g.W_fm = nullptr;
      }
    } else {
      if (!ln || !(fold || tfold)) { g.ln_u = nullptr; g.ln_c = nullptr; g.ln_wg = nullptr; g.ln_wg_fm = nullptr; }
      g.lean = lean;
      g.lean_fold = fold && g.ln_w && g.ln_wg_fm && g.ln_u && g.ln_c;
      if (fold && ln && !g.lean_fold) unsupported("folded lean launch: no folded operands for this shape");
    }
    int taken = kTakenNone;
    g.taken = &taken;
    try {
      gemm(dt, g, st);
    } catch (const WcbError&) {
      throw;
    } catch (const std::runtime_error& err) {   // an operand combination no launcher of the path takes
      throw WcbError(WCB_ERR_UNSUPPORTED, err.what());
    }
    HIPCHK(hipGetLastError());
    if (need_fold) {
      if (p->u_out) HIPCHK(hipMemcpyAsync(p->u_out, ub.b.p, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
      if (p->c_out) HIPCHK(hipMemcpyAsync(p->c_out, cb.b.p, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
      if (p->wg_out) HIPCHK(hipMemcpyAsync(p->wg_out, wg.b.p, (size_t)N * K * e, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));   // the derived operands are freed on return
    if (p->taken) *p->taken = taken;
    const int want = kind == WCB_PROJ_XQK ? kTakenXqk : lean ? kTakenLean : path == WCB_PATH_DEC ? kTakenDecMf :
                     path == WCB_PATH_WIDE ? kTakenWide : kTakenRingDec;
    if ((taken & 255) != want)
      throw WcbError(WCB_ERR_UNSUPPORTED, "the path's launcher does not cover this launch (launcher " + std::to_string(taken & 255) +
                                              " ran; the outputs are not the path's)");
  });
}

// wcb_op_lm_head_lse, and wcb_op_lm_head_sample (seeds non-null: the sampled kernels, step on the device)
static int op_lm_head(int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float* logits, long ld,
                      float* lse, int32_t* argmax, void* stream, bool sampled, float temperature, const uint64_t* seeds,
                      int step) {
  return guarded(nullptr, [&] {
    REQUIRE(A && W && logits && lse && argmax && M > 0 && M <= 64 && V > 0 && K > 0 && ld >= V,
            "bad argument (1 <= M <= 64, ld >= V, every pointer)");
    REQUIRE(dtype >= WCB_BF16 && dtype <= WCB_F32, "dtype");
    REQUIRE(walkers >= 0 && walkers <= 4096, "walkers: 0 (default) .. 4096");
    if (sampled) {
      check_sampling(temperature, seeds);
      REQUIRE(step >= 0, "step must be >= 0");
    }
    const DType dt = DType(dtype);
    // the widths the decode step's LM head runs at: the decode GEMM's column walk, or the older skinny kernel
    if (!gemm_dec_supported(dt, K) && K != 32 && K != 2560)
      throw WcbError(WCB_ERR_UNSUPPORTED, "K: 64, 128, 256, 384, 512, 768, 1024, 1280 (column walk) or 32, 2560 (skinny kernel)");
    hipStream_t st = (hipStream_t)stream;
    const int wk = walkers > 0 ? walkers : kDecWalkers;
    const int nchunk = lm_head_partials(dt, K, V, wk);
    struct Scratch { DevBuf b; ~Scratch() { b.release(); } } pv, pi, pm, ps, zero, wpad, wfm, samp;
    const size_t np = (size_t)M * nchunk * 4;
    pv.b.ensure(np); pi.b.ensure(np); pm.b.ensure(np); ps.b.ensure(np); zero.b.ensure(16);
    GemmArgs lm = drow(A, K, W, M, V, K, logits, ld);
    lm.out_f32 = 1;
    lm.walkers = wk;
    lm.sel_val = pv.b.as<float>(); lm.sel_idx = pi.b.as<int>();
    lm.sel_max = pm.b.as<float>(); lm.sel_sum = ps.b.as<float>();
    lm.sel_step = zero.b.as<int>();   // step 0 against min_new 0: no EOS mask; lam 0: no boost
    if (sampled) {   // [0] the step counter, then inv_T and the seeds laid out as a decode context's samp words
      samp.b.ensure(8 + (size_t)(1 + M) * 8);
      int w[4 + 2 * 64] = {};
      const float inv_t = 1.0f / temperature;
      w[0] = step;
      std::memcpy(w + 2, &inv_t, 4);
      std::memcpy(w + 4, seeds, (size_t)M * 8);
      write_i32(samp.b.as<int>(), w, 4 + 2 * M, st);
      lm.sel_step = samp.b.as<int>();   // (min_new 0: still no EOS mask)
      lm.sel_inv_t = reinterpret_cast<const float*>(samp.b.as<int>() + 2);
      lm.sel_seeds = samp.b.as<uint64_t>() + 2;
    }
    int nw = 0, kpw = 0;
    if (dt != kF32 && gemm_dec_supported(dt, K) && lean_cfg(K, nw, kpw)) {
      // as the runtime's token embedding: a fragment-major copy of whole 16-row tiles, zero rows past V
      const size_t e = esize(dtype), vp = (size_t)(V + 15) / 16 * 16;
      wpad.b.ensure(vp * K * e);
      wfm.b.ensure(vp * K * e);
      HIPCHK(hipMemcpyAsync(wpad.b.p, W, (size_t)V * K * e, hipMemcpyDeviceToDevice, st));
      frag_major(dt, wpad.b.p, (int)vp, K, nw, kpw, wfm.b.p, st);
      lm.W_fm = wfm.b.p;
    }
    gemm(dt, lm, st);
    lm_head_lse_finalize(lm.sel_val, lm.sel_idx, lm.sel_max, lm.sel_sum, M, nchunk, lse, argmax, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the scratch buffers are freed on return
  });
}

int wcb_op_lm_head_lse(int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float* logits, long ld,
                       float* lse, int32_t* argmax, void* stream) {
  return op_lm_head(dtype, A, W, M, V, K, walkers, logits, ld, lse, argmax, stream, false, 0.f, nullptr, 0);
}

int wcb_op_lm_head_sample(int dtype, const void* A, const void* W, int M, int V, int K, int walkers, float temperature,
                          const uint64_t* seeds, int step, float* logits, long ld, float* lse, int32_t* sampled,
                          void* stream) {
  return op_lm_head(dtype, A, W, M, V, K, walkers, logits, ld, lse, sampled, stream, true, temperature, seeds, step);
}

int wcb_op_lang_head(int dtype, const void* A, const void* W, int M, int V, int K, int lang_begin, int n_lang,
                     const uint32_t* candidates, int32_t* out_ids, float* out_probs, float* logits, long ld, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(A && W && logits && out_ids && M > 0 && M <= 64 && V > 0 && K > 0 && K <= kLangMaxK && ld >= V,
            "bad argument (1 <= M <= 64, 1 <= K <= 2560, ld >= V, every pointer)");
    REQUIRE(dtype >= WCB_BF16 && dtype <= WCB_F32, "dtype");
    check_lang(lang_begin, n_lang, candidates, -1, V);
    hipStream_t st = (hipStream_t)stream;
    DecCtx scratch;   // (only its candidate words are used)
    struct Free { DecCtx& D; ~Free() { D.lang.release(); } } free_{scratch};
    LangArgs a;
    a.A = A; a.lda = K; a.W = W; a.K = K; a.M = M;
    a.logits = logits; a.ld = ld;
    lang_range(scratch, a, lang_begin, n_lang, candidates, V, st);
    a.out_ids = out_ids; a.out_probs = out_probs;
    lang_head(DType(dtype), a, st);
    lang_finalize(a, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the scratch words are freed on return
  });
}

int wcb_sample_noise(uint64_t seed, int step, int v0, int n, float* out) {
  return guarded(nullptr, [&] {
    REQUIRE(out && n >= 0 && step >= 0 && v0 >= 0 && (long)v0 + n <= 0x7fffffffL, "bad argument (out, n, step, v0 >= 0)");
    for (int i = 0; i < n; ++i) out[i] = sample_noise(seed, step, v0 + i);
  });
}

// ---- token rules (wcb.h wcb_token_rules; csrc/tsrule.h)
extern "C++" {
namespace {

void check_rules(const wcb_token_rules* r, int V, int eos) {
  REQUIRE(r->n_suppress >= 0 && r->n_begin_suppress >= 0, "token rules: negative list length");
  REQUIRE((r->n_suppress == 0 || r->suppress) && (r->n_begin_suppress == 0 || r->begin_suppress), "token rules: null id list");
  REQUIRE(r->timestamps == 0 || r->timestamps == 1, "token rules: timestamps must be 0 or 1");
  const int lim = r->timestamps ? r->timestamp_begin : V;
  if (r->timestamps) {
    REQUIRE(r->timestamp_begin > eos && r->timestamp_begin < V, "token rules: timestamp_begin must lie in (eos, vocab)");
    REQUIRE(r->no_timestamps_token_id >= 0 && r->no_timestamps_token_id < r->timestamp_begin,
            "token rules: no_timestamps_token_id must lie in [0, timestamp_begin)");
  }
  for (int i = 0; i < r->n_suppress; ++i)
    REQUIRE(r->suppress[i] >= 0 && r->suppress[i] < V && r->suppress[i] < lim,
            "token rules: suppress id outside [0, vocab) (with timestamps: [0, timestamp_begin))");
  for (int i = 0; i < r->n_begin_suppress; ++i)
    REQUIRE(r->begin_suppress[i] >= 0 && r->begin_suppress[i] < V && r->begin_suppress[i] < lim,
            "token rules: begin_suppress id outside [0, vocab) (with timestamps: [0, timestamp_begin))");
}

TsRule rules_ts(const wcb_token_rules* r) {
  TsRule t;
  t.on = r->timestamps;
  t.ts0 = r->timestamps ? r->timestamp_begin : 0;
  t.max_init = r->max_initial_timestamp_index < 0 ? -1 : r->max_initial_timestamp_index;
  return t;
}

// the deny bitmaps of every step (d) and of step 0 (d0), `words` 32-bit words each: the suppress ids, at step 0
// the begin_suppress ids too; with the timestamp grammar no_timestamps and every id of [timestamp_begin, V) — the
// LM head's winner is then the best allowed text token, the finalize scores the timestamps itself
void build_deny(const wcb_token_rules* r, int V, size_t words, std::vector<uint32_t>& d, std::vector<uint32_t>& d0) {
  d.assign(words, 0u);
  auto set = [](std::vector<uint32_t>& b, int v) { b[(size_t)v >> 5] |= 1u << (v & 31); };
  for (int i = 0; i < r->n_suppress; ++i) set(d, r->suppress[i]);
  if (r->timestamps) {
    set(d, r->no_timestamps_token_id);
    for (int v = r->timestamp_begin; v < V; ++v) set(d, v);
  }
  d0 = d;
  for (int i = 0; i < r->n_begin_suppress; ++i) set(d0, r->begin_suppress[i]);
}

}  // namespace
}  // extern "C++"

int wcb_set_token_rules(wcb_handle* h, const wcb_token_rules* r) {
  return guarded(h, [&] {
    REQUIRE(h, "null handle");
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    if (h->step_state) throw WcbError(WCB_ERR_STATE, "wcb_set_token_rules: a step-wise decode is active (wcb_decode_end first)");
    if (!r) { h->rules_on = false; return; }
    check_rules(r, h->d.vocab, h->d.eos_token_id);
    const size_t words = (size_t)h->vocab_pad / 32;
    std::vector<uint32_t> d, d0;
    build_deny(r, h->d.vocab, words, d, d0);
    quiesce(h);   // queued decodes read the bitmaps
    h->rules_deny.ensure(words * 4);    // (allocated once: vocab_pad is fixed by the weights)
    h->rules_deny0.ensure(words * 4);
    HIPCHK(hipMemcpy(h->rules_deny.p, d.data(), words * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->rules_deny0.p, d0.data(), words * 4, hipMemcpyHostToDevice));
    h->rules_has0 = r->n_begin_suppress > 0;
    h->rules_ts = rules_ts(r);
    h->rules_on = true;
  });
}

int wcb_token_rules_apply_host(const wcb_token_rules* r, int vocab, int eos, const int32_t* generated, int n, float* scores) {
  return guarded(nullptr, [&] {
    REQUIRE(r && scores && vocab > 0 && eos >= 0 && eos < vocab && n >= 0 && (n == 0 || generated), "bad argument");
    check_rules(r, vocab, eos);
    const size_t words = ((size_t)vocab + 127) / 128 * 4;
    std::vector<uint32_t> d, d0;
    build_deny(r, vocab, words, d, d0);
    const TsRule ts = rules_ts(r);
    const uint32_t* deny = n == 0 ? d0.data() : d.data();
    if (!ts.on) {
      for (int v = 0; v < vocab; ++v)
        if (deny_bit(deny, v)) scores[v] = -INFINITY;
      return;
    }
    int w0 = 0, w1 = 0;
    for (int i = 0; i < n; ++i) {
      REQUIRE(generated[i] >= 0 && generated[i] < vocab, "generated id outside [0, vocab)");
      ts_advance(ts, generated[i], w0, w1);
    }
    const TsAllowed a = ts_allowed(ts, vocab, eos, w0, w1);
    double tmax = -INFINITY, xmax = -INFINITY;
    for (int v = 0; v < ts.ts0; ++v) {
      if (v < a.text_lo || deny_bit(deny, v)) scores[v] = -INFINITY;
      xmax = std::max(xmax, (double)scores[v]);
    }
    for (int v = ts.ts0; v < vocab; ++v) {
      if (v < a.lo || v > a.hi) scores[v] = -INFINITY;
      tmax = std::max(tmax, (double)scores[v]);
    }
    double sum = 0.0;
    if (tmax > -INFINITY)
      for (int v = a.lo; v <= a.hi; ++v) sum += std::exp((double)scores[v] - tmax);
    const double lse = sum > 0.0 ? tmax + std::log(sum) : -INFINITY;
    if (lse > xmax)   // rule 5: the timestamps together outweigh the best text token
      for (int v = 0; v < ts.ts0; ++v) scores[v] = -INFINITY;
  });
}

int wcb_op_lm_head_rules(int dtype, const void* A, const void* W, int M, int V, int K, int walkers,
                         const wcb_token_rules* rules, int eos, const int32_t* generated, int gen_ld, const int32_t* lens,
                         float* logits, long ld, int32_t* next_ids, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(A && W && logits && next_ids && rules && lens && M > 0 && M <= 64 && V > 0 && K > 0 && ld >= V && eos >= 0 && eos < V,
            "bad argument (1 <= M <= 64, ld >= V, 0 <= eos < V, every pointer)");
    REQUIRE(dtype >= WCB_BF16 && dtype <= WCB_F32, "dtype");
    REQUIRE(walkers >= 0 && walkers <= 4096, "walkers: 0 (default) .. 4096");
    check_rules(rules, V, eos);
    const DType dt = DType(dtype);
    if (!gemm_dec_supported(dt, K) && K != 32 && K != 2560)
      throw WcbError(WCB_ERR_UNSUPPORTED, "K: 64, 128, 256, 384, 512, 768, 1024, 1280 (column walk) or 32, 2560 (skinny kernel)");
    const TsRule ts = rules_ts(rules);
    // the row states after their histories; the launch's step: 0 when every row is at t == 0
    std::vector<int> host((size_t)2 * M, 0);
    int n0 = 0;
    for (int m = 0; m < M; ++m) {
      REQUIRE(lens[m] >= 0 && (lens[m] == 0 || (generated && gen_ld >= lens[m])), "lens / generated");
      n0 += lens[m] == 0;
      int w0 = 0, w1 = 0;
      for (int i = 0; i < lens[m]; ++i) {
        const int tok = generated[(size_t)m * gen_ld + i];
        REQUIRE(tok >= 0 && tok < V, "generated id outside [0, vocab)");
        ts_advance(ts, tok, w0, w1);
      }
      host[2 * m] = w0;
      host[2 * m + 1] = w1;
    }
    REQUIRE(ts.on || rules->n_begin_suppress == 0 || n0 == 0 || n0 == M,
            "rows at t == 0 and t > 0 in one call with begin_suppress ids (the bitmap of a launch is chosen by its step)");
    hipStream_t st = (hipStream_t)stream;
    const int wk = walkers > 0 ? walkers : kDecWalkers;
    const int nchunk = lm_head_partials(dt, K, V, wk);
    struct Scratch { DevBuf b; ~Scratch() { b.release(); } } pv, pi, zi, bm, wpad, wfm;
    const size_t np = (size_t)M * nchunk * 4, words = ((size_t)V + 127) / 128 * 4;
    pv.b.ensure(np); pi.b.ensure(np);
    std::vector<uint32_t> d, d0;
    build_deny(rules, V, words, d, d0);
    bm.b.ensure(2 * words * 4);
    HIPCHK(hipMemcpyAsync(bm.b.p, d.data(), words * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(bm.b.as<uint32_t>() + words, d0.data(), words * 4, hipMemcpyHostToDevice, st));
    // one zeroed int block: the counters, then the per-row arrays of a one-step decode with an empty forest
    // (every row in root state 0, no transitions, no root children), the rule states and the id column
    int* z = nullptr;
    const size_t zn = 16 + (size_t)10 * M + 8;
    zi.b.ensure(zn * 4);
    z = zi.b.as<int>();
    int* zstate = z + 16;
    int* zts = z + 16 + 6 * M + 8;
    int* zout = zts + 2 * M;
    const int step0 = n0 == M ? 0 : 1;
    write_i32(z, &step0, 1, st);
    write_i32(zts, host.data(), 2 * M, st);
    GemmArgs lm = drow(A, K, W, M, V, K, logits, ld);
    lm.out_f32 = 1;
    lm.walkers = wk;
    lm.sel_val = pv.b.as<float>(); lm.sel_idx = pi.b.as<int>();
    lm.sel_step = z;   // min_new 0: no EOS mask; lam 0: no boost
    lm.sel_deny = bm.b.as<uint32_t>();
    lm.sel_deny0 = rules->n_begin_suppress > 0 ? bm.b.as<uint32_t>() + words : nullptr;
    int nw = 0, kpw = 0;
    if (dt != kF32 && gemm_dec_supported(dt, K) && lean_cfg(K, nw, kpw)) {   // as op_lm_head: fragment-major weights
      const size_t e = esize(dtype), vp = (size_t)(V + 15) / 16 * 16;
      wpad.b.ensure(vp * K * e);
      wfm.b.ensure(vp * K * e);
      HIPCHK(hipMemcpyAsync(wpad.b.p, W, (size_t)V * K * e, hipMemcpyDeviceToDevice, st));
      frag_major(dt, wpad.b.p, (int)vp, K, nw, kpw, wfm.b.p, st);
      lm.W_fm = wfm.b.p;
    }
    gemm(dt, lm, st);
    SelectArgs s;
    s.logits = logits; s.ld = ld; s.M = M; s.V = V;
    s.trans_off = zstate + 5 * M + 2; s.trans_tok = nullptr; s.trans_dst = nullptr;
    s.st_depth = zstate + 5 * M + 4; s.st_keep = zstate + 5 * M + 5;
    s.state = zstate; s.finished = zstate + M; s.rowbase = zstate + 2 * M;
    s.forest.root = zstate + 3 * M; s.forest.rc_off = zstate + 4 * M;   // [M + 1] zeros
    s.eos = eos; s.pad = eos; s.min_new = 0;
    s.step = z; s.pos = z + 1; s.all_done = z + 2;
    s.ticket_unfin = reinterpret_cast<unsigned long long*>(z + 4);
    s.next_ids = next_ids; s.out_ids = zout; s.out_ld = 2;
    s.part_val = lm.sel_val; s.part_idx = lm.sel_idx; s.nchunk = nchunk;
    s.deny = lm.sel_deny; s.deny0 = lm.sel_deny0; s.ts = ts; s.ts_state = zts;
    select_finalize(s, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the scratch buffers and the pageable host sources live until here
  });
}

// ---- repeat rules (csrc/reprule.h)
extern "C++" {
namespace {
void check_repeat_rules(const wcb_repeat_rules* r) {
  REQUIRE(std::isfinite(r->repetition_penalty) && r->repetition_penalty > 0.f, "repetition_penalty must be finite and > 0");
  REQUIRE(r->no_repeat_ngram_size >= 0, "no_repeat_ngram_size must be >= 0");
}
}  // namespace
}  // extern "C++"

int wcb_set_repeat_rules(wcb_handle* h, const wcb_repeat_rules* r) {
  return guarded(h, [&] {
    REQUIRE(h, "null handle");
    if (!h->ready) throw WcbError(WCB_ERR_STATE, "weights not finalized");
    if (h->step_state) throw WcbError(WCB_ERR_STATE, "wcb_set_repeat_rules: a step-wise decode is active (wcb_decode_end first)");
    if (!r) { h->rep_on = false; return; }
    check_repeat_rules(r);
    // (no device work: every decode writes the values into its own context, stream-ordered, at its start)
    h->rep_p = r->repetition_penalty;
    h->rep_n = r->no_repeat_ngram_size;
    h->rep_on = !(h->rep_p == 1.f && h->rep_n == 0);   // both at "off": the decode as it always was
  });
}

int wcb_repeat_rules_apply_host(const wcb_repeat_rules* r, int vocab, const int32_t* hist, int n_hist, float* scores) {
  return guarded(nullptr, [&] {
    REQUIRE(r && scores && vocab > 0 && n_hist >= 0 && (n_hist == 0 || hist), "bad argument");
    check_repeat_rules(r);
    for (int i = 0; i < n_hist; ++i) REQUIRE(hist[i] >= 0 && hist[i] < vocab, "history id outside [0, vocab)");
    const float p = r->repetition_penalty;
    const int n = r->no_repeat_ngram_size, L = n_hist;
    std::vector<char> seen((size_t)vocab, 0);
    for (int i = 0; i < L; ++i) {   // every distinct token once
      if (seen[hist[i]]) continue;
      seen[hist[i]] = 1;
      scores[hist[i]] = rep_penalty(scores[hist[i]], p);
    }
    if (n >= 1 && L >= n)
      for (int i = 0; i <= L - n; ++i)
        if (rep_ngram_match(hist, L, n, i)) scores[hist[i + n - 1]] = -INFINITY;
  });
}

int wcb_op_lm_head_repeat(int dtype, const void* A, const void* W, int M, int V, int K, int walkers,
                          const wcb_repeat_rules* rules, int eos, const int32_t* hist, int hist_ld, const int32_t* lens,
                          float* logits, long ld, int32_t* next_ids, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(A && W && logits && next_ids && rules && hist && lens && M > 0 && M <= 64 && V > 0 && K > 0 && ld >= V && eos >= 0 &&
                eos < V && hist_ld >= 1,
            "bad argument (1 <= M <= 64, ld >= V, 0 <= eos < V, every pointer)");
    REQUIRE(dtype >= WCB_BF16 && dtype <= WCB_F32, "dtype");
    REQUIRE(walkers >= 0 && walkers <= 4096, "walkers: 0 (default) .. 4096");
    check_repeat_rules(rules);
    if (V > kRepBanWords * 32) throw WcbError(WCB_ERR_UNSUPPORTED, "repeat rules: a vocabulary above 53248 tokens");
    const DType dt = DType(dtype);
    if (!gemm_dec_supported(dt, K) && K != 32 && K != 2560)
      throw WcbError(WCB_ERR_UNSUPPORTED, "K: 64, 128, 256, 384, 512, 768, 1024, 1280 (column walk) or 32, 2560 (skinny kernel)");
    // the histories as left-padded prompt rows [M][hist_ld] with their offsets: the layout of a ragged decode at step 0
    std::vector<int> rows((size_t)M * hist_ld, 0), offs((size_t)M, 0);
    for (int m = 0; m < M; ++m) {
      REQUIRE(lens[m] >= 1 && lens[m] <= hist_ld && lens[m] <= kRepMaxHist, "lens outside [1, min(hist_ld, 448)]");
      offs[m] = hist_ld - lens[m];
      for (int i = 0; i < lens[m]; ++i) {
        const int tok = hist[(size_t)m * hist_ld + i];
        REQUIRE(tok >= 0 && tok < V, "history id outside [0, vocab)");
        rows[(size_t)m * hist_ld + offs[m] + i] = tok;
      }
    }
    hipStream_t st = (hipStream_t)stream;
    const int wk = walkers > 0 ? walkers : kDecWalkers;
    const int nchunk = lm_head_partials(dt, K, V, wk);
    struct Scratch { DevBuf b; ~Scratch() { b.release(); } } pv, pi, zi, bm, hb, wpad, wfm;
    const size_t np = (size_t)M * nchunk * 4, words = ((size_t)V + 127) / 128 * 4;
    pv.b.ensure(np); pi.b.ensure(np);
    bm.b.ensure((size_t)M * words * 4);
    hb.b.ensure(((size_t)M * hist_ld + M + 2) * 4);
    int* d_rows = hb.b.as<int>();
    int* d_offs = d_rows + (size_t)M * hist_ld;
    int* d_par = d_offs + M;
    write_i32(d_rows, rows.data(), M * hist_ld, st);
    write_i32(d_offs, offs.data(), M, st);
    int par[2] = {0, rules->no_repeat_ngram_size};
    std::memcpy(par, &rules->repetition_penalty, 4);
    write_i32(d_par, par, 2, st);
    RepArgs rp;
    rp.seen = bm.b.as<uint32_t>(); rp.words = (int)words; rp.par = d_par;
    rp.prompt = d_rows; rp.prompt_ld = hist_ld; rp.P = hist_ld; rp.start_tok = 0; rp.poff = d_offs;
    rep_init(rp, M, V, st);
    // one zeroed int block: the counters (step 0), then the per-row arrays of a one-step decode with an empty forest
    const size_t zn = 16 + (size_t)10 * M + 8;
    zi.b.ensure(zn * 4);
    int* z = zi.b.as<int>();
    int* zstate = z + 16;
    int* zts = z + 16 + 6 * M + 8;
    int* zout = zts + 2 * M;
    GemmArgs lm = drow(A, K, W, M, V, K, logits, ld);
    lm.out_f32 = 1;
    lm.walkers = wk;
    lm.sel_val = pv.b.as<float>(); lm.sel_idx = pi.b.as<int>();
    lm.sel_step = z;   // min_new 0: no EOS mask; lam 0: no boost
    lm.sel_seen = rp.seen; lm.sel_seen_w = rp.words;
    int nw = 0, kpw = 0;
    if (dt != kF32 && gemm_dec_supported(dt, K) && lean_cfg(K, nw, kpw)) {   // as op_lm_head: fragment-major weights
      const size_t e = esize(dtype), vp = (size_t)(V + 15) / 16 * 16;
      wpad.b.ensure(vp * K * e);
      wfm.b.ensure(vp * K * e);
      HIPCHK(hipMemcpyAsync(wpad.b.p, W, (size_t)V * K * e, hipMemcpyDeviceToDevice, st));
      frag_major(dt, wpad.b.p, (int)vp, K, nw, kpw, wfm.b.p, st);
      lm.W_fm = wfm.b.p;
    }
    gemm(dt, lm, st);
    SelectArgs s;
    s.logits = logits; s.ld = ld; s.M = M; s.V = V;
    s.trans_off = zstate + 5 * M + 2; s.trans_tok = nullptr; s.trans_dst = nullptr;
    s.st_depth = zstate + 5 * M + 4; s.st_keep = zstate + 5 * M + 5;
    s.state = zstate; s.finished = zstate + M; s.rowbase = zstate + 2 * M;
    s.forest.root = zstate + 3 * M; s.forest.rc_off = zstate + 4 * M;   // [M + 1] zeros
    s.eos = eos; s.pad = eos; s.min_new = 0;
    s.step = z; s.pos = z + 1; s.all_done = z + 2;
    s.ticket_unfin = reinterpret_cast<unsigned long long*>(z + 4);
    s.next_ids = next_ids; s.out_ids = zout; s.out_ld = 2;
    s.part_val = lm.sel_val; s.part_idx = lm.sel_idx; s.nchunk = nchunk;
    s.ts_state = zts;
    s.rep = rp;
    select_finalize(s, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the scratch buffers live until here
  });
}

int wcb_op_window_cut(int dtype, const float* mel, int clips, int n_mel, int T, int T_ld, int rows, const int32_t* clip_idx,
                      const int32_t* seek, const int32_t* seek_num_frames, void* xt, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(dtype >= 0 && dtype <= 2 && xt && n_mel >= 1, "bad argument");
    const wcb_windows w{mel, clips, T, T_ld, clip_idx, seek, seek_num_frames};
    check_windows(&w, rows);
    DevBuf ints;
    ints.ensure((size_t)3 * kWinRows * 4);
    int v[3 * kWinRows] = {};
    for (int r = 0; r < rows; ++r) { v[r] = clip_idx[r]; v[kWinRows + r] = seek[r]; v[2 * kWinRows + r] = seek_num_frames[r]; }
    hipStream_t st = (hipStream_t)stream;
    write_i32(ints.as<int>(), v, 3 * kWinRows, st);
    mel_window_to_conv_input((DType)dtype, mel, n_mel, T_ld, ints.as<int>(), ints.as<int>() + kWinRows, ints.as<int>() + 2 * kWinRows,
                             rows, xt, (long)(kFrames + 2) * n_mel, st);
    HIPCHK(hipStreamSynchronize(st));
    ints.release();
  });
}

int wcb_op_layernorm(int dtype, const float* x, const float* w, const float* b, void* y, int M, int d, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(x && w && b && y && M > 0 && d > 0 && d % 64 == 0 && d <= 2048, "bad argument");
    layernorm(DType(dtype), x, w, b, y, M, d, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_attention_decode(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H, int Sk,
                            int nsplit, int variant, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(q && k && v && o && B > 0 && H > 0 && Sk > 0 && Sk <= 2048 && nsplit >= 1 && nsplit <= 64, "bad argument");
    AttnArgs a;   // decode layout: q/o [B][H·64], K/V head-major [B][H][Sk][64] (the cross-K/V layout)
    a.q = q; a.ldq = (long)H * 64; a.q_Sb = 1; a.Sq = 1;
    a.k = k; a.v = v; a.k_sb = (long)H * Sk * 64; a.k_sh = (long)Sk * 64; a.k_sk = 64;
    a.o = o; a.ldo = (long)H * 64; a.o_Sb = 1; a.B = B; a.H = H; a.nkeys = Sk;
    a.variant = variant;
    if (variant == 6 || variant == 7) a.kv_rows = Sk;   // the one-token self-attention kernel (speculative first keys)
    int* nk_dev = nullptr;
    if (variant == 7) {   // the key count read on the device (decode graphs): the lean self-attention kernel
      // per-call, stream-ordered scratch (a shared buffer would race between calls on different streams),
      // written by a kernel whose argument carries the value (no pageable host source)
      HIPCHK(hipMallocAsync(reinterpret_cast<void**>(&nk_dev), 4, (hipStream_t)stream));
      const int nk1 = Sk - 1;
      write_i32(nk_dev, &nk1, 1, (hipStream_t)stream);
      a.nkeys_dev = nk_dev; a.nkeys_add = 1;
    }
    static DevBuf part, ticket;
    if (nsplit > 1) {
      a.nsplit = nsplit;
      part.ensure((size_t)B * H * nsplit * 66 * 4);
      ticket.ensure((size_t)B * H * 4);
      a.part = part.as<float>();
      a.ticket = ticket.as<int>();
    }
    attention_decode(DType(dtype), a, (hipStream_t)stream);
    if (nk_dev) HIPCHK(hipFreeAsync(nk_dev, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_attention_decode_window(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H, int Sq,
                                   int Sk, const int32_t* key_start, int variant, void* stream) {
  return guarded(nullptr, [&] {
    const int kind = variant % 100, nsplit = variant >= 100 ? variant / 100 : 1;
    REQUIRE(q && k && v && o && B > 0 && H > 0 && Sq > 0 && Sq <= Sk && Sk <= 2048, "bad argument");
    REQUIRE(kind >= 0 && kind <= 7 && nsplit >= 1 && nsplit <= 64, "variant: 0..5 (+ 100·chunks), 6 or 7");
    REQUIRE(kind < 6 || (Sq == 1 && nsplit == 1), "variants 6 and 7 are the one-token kernels (Sq = 1, no split)");
    AttnArgs a;   // the runtime's self-attention call: q/o [B][Sq][H·64], K/V head-major [B][H][Sk][64]
    a.q = q; a.ldq = (long)H * 64; a.q_Sb = Sq; a.Sq = Sq; a.causal = Sq > 1;
    a.k = k; a.v = v; a.k_sb = (long)H * Sk * 64; a.k_sh = (long)Sk * 64; a.k_sk = 64;
    a.o = o; a.ldo = (long)H * 64; a.o_Sb = Sq; a.B = B; a.H = H; a.nkeys = Sk - Sq + 1;
    a.variant = kind; a.key_start = key_start;   // (null: the same launch on the dense kernels)
    if (kind >= 6) a.kv_rows = Sk;
    int* nk_dev = nullptr;
    if (kind == 7) {   // the key count read on the device: the lean kernel (wcb_op_attention_decode's variant 7)
      HIPCHK(hipMallocAsync(reinterpret_cast<void**>(&nk_dev), 4, (hipStream_t)stream));
      const int nk1 = Sk - 1;
      write_i32(nk_dev, &nk1, 1, (hipStream_t)stream);
      a.nkeys_dev = nk_dev; a.nkeys_add = 1;
    }
    static DevBuf part, ticket;   // split-KV workspace of this test entry point (zeroed on growth)
    if (nsplit > 1) {
      a.nsplit = nsplit;
      part.ensure((size_t)B * H * Sq * nsplit * 66 * 4);
      ticket.ensure((size_t)B * H * Sq * 4);
      a.part = part.as<float>();
      a.ticket = ticket.as<int>();
    }
    attention_decode(DType(dtype), a, (hipStream_t)stream);
    if (nk_dev) HIPCHK(hipFreeAsync(nk_dev, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_cross_attention_enc(int dtype, const void* q, const void* enc, const void* wkt, const void* wv,
                               const float* bv, void* o, int B, int H, int S, int nsplit, int variant, void* stream) {
  return guarded(nullptr, [&] {
    const int d = H * 64;
    REQUIRE(q && enc && wkt && wv && bv && o && B > 0 && B <= 64 && H > 0 && S > 0 && nsplit >= 1 &&
                nsplit <= kXencMaxSplit, "bad argument");
    REQUIRE(xenc_supported(DType(dtype), d), "encoder-space cross-attention needs a 16-bit dtype and d <= 1024");
    static DevBuf qp, u, part, ml;   // workspaces of this test entry point
    const size_t e = esize(dtype);
    qp.ensure((size_t)B * H * d * e);
    u.ensure((size_t)B * H * d * e);
    part.ensure((size_t)B * nsplit * H * d * 4);
    ml.ensure((size_t)B * nsplit * H * 2 * 4);
    GemmArgs kq = rowgemm(q, d, wkt, B, H * d, 64, qp.p, (long)H * d);
    kq.a_grp_n = d; kq.a_grp_off = 64;
    gemm(DType(dtype), kq, (hipStream_t)stream);
    XencArgs xa;
    xa.enc = enc; xa.enc_sb = (long)S * d; xa.qp = qp.p; xa.rows = B; xa.H = H; xa.D = d; xa.S = S;
    xa.nsplit = nsplit; xa.part = part.as<float>(); xa.ml = ml.as<float>();
    xa.variant = variant % 100;
    xa.part16 = variant >= 1000 && d % 128 == 0;   // variant + 1000: 16-bit normalised range partials
    if (xa.part16) xa.variant = 1;
    xenc_attention(DType(dtype), xa, (hipStream_t)stream);
    if (d % 128 == 0 && (variant < 100 || variant >= 1000)) {   // the runtime's default: merge + W_v fused
      xenc_merge_v(DType(dtype), xa, wv, bv, o, d, (hipStream_t)stream);
    } else {   // variant + 100: merge kernel + grouped W_v GEMM (option merge_v = 0, and d = 64)
      xenc_merge(DType(dtype), xa, u.p, (long)H * d, (hipStream_t)stream);
      GemmArgs vg = rowgemm(u.p, (long)H * d, wv, B, d, d, o, d);
      vg.a_grp_n = 64; vg.a_grp_off = d; vg.bias = bv;
      gemm(DType(dtype), vg, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_weighted_ce(const float* logits, long ld, int B, int T, int V, const int32_t* labels,
                       const int32_t* spans, const int32_t* span_len, int N, int Lmax, float bias_weight,
                       float* per_token, float* loss, int32_t* count, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(logits && labels && per_token && loss && B > 0 && T > 0 && V > 0 && ld >= V, "bad argument");
    REQUIRE(!spans || (span_len && N > 0 && Lmax > 0), "spans need span_len, N > 0 and Lmax > 0");
    WceArgs a;
    a.logits = logits; a.ld = ld; a.B = B; a.T = T; a.V = V; a.labels = labels;
    a.spans = spans; a.span_len = span_len; a.N = spans ? N : 0; a.Lmax = spans ? Lmax : 0;
    a.use_spans = spans ? 1 : 0; a.bias_weight = bias_weight;
    a.per_token = per_token; a.loss = loss; a.count = count;
    weighted_ce(a, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
  });
}

int wcb_op_attention(int dtype, const void* q, const void* k, const void* v, void* o, int B, int H, int Sq, int Sk,
                     int flash, void* stream) {
  return guarded(nullptr, [&] {
    REQUIRE(q && k && v && o && B > 0 && H > 0 && Sq > 0 && Sk > 0 && Sk <= 2048, "bad argument");
    AttnArgs a;
    const long ld = (long)H * 64;
    a.q = q; a.ldq = ld; a.q_Sb = Sq; a.Sq = Sq;
    a.k = k; a.v = v; a.k_sb = (long)Sk * ld; a.k_sh = 64; a.k_sk = ld;
    a.o = o; a.ldo = ld; a.o_Sb = Sq; a.B = B; a.H = H; a.nkeys = Sk;
    const bool beam = flash >= 200 && flash <= 202;
    if (flash == 1 || flash == 100 || beam || flash < 0) {
      // 100: 64 queries per wave;
      // 200 / 201 / 202: the beam kernel (keys split over the waves, Sq <= 16; 4 waves x 2 stages, 2 x 4,
      // 2 x 5); -n: n key ranges + merge (Sq <= 16)
      a.variant = flash == 100 ? 4 : beam ? 7 + (flash - 200) : 1;
      REQUIRE(!beam || Sq <= 16, "the beam kernel takes at most 16 query rows per set");
      REQUIRE(dtype != WCB_F32, "flash attention needs a 16-bit dtype");
      static DevBuf fpart;
      if (flash < 0) {
        REQUIRE(-flash <= 8 && Sq <= 16, "flash key split: 1..8 ranges, Sq <= 16");
        a.nsplit = -flash;
        fpart.ensure((size_t)B * H * Sq * a.nsplit * 66 * 4);
        a.part = fpart.as<float>();
      }
      attention_flash(DType(dtype), a, (hipStream_t)stream);
    } else {
      static DevBuf part, ticket;   // split-KV workspace of this test entry point (zeroed on growth)
      if (flash > 1) {
        a.nsplit = flash;
        part.ensure((size_t)B * H * Sq * flash * 66 * 4);
        ticket.ensure((size_t)B * H * Sq * 4);
        a.part = part.as<float>();
        a.ticket = ticket.as<int>();
      }
      attention_decode(DType(dtype), a, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
  });
}

}  // extern "C"
