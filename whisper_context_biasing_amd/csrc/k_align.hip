// Token-level timestamps from cross-attention (HF _extract_token_timestamps), gfx950.
//   align_prep_kernel     per clip: the first EOS of its generated ids → m, and the teacher-forced input row
//   align_capture_kernel  softmax over all S frames of the scaled q·k scores of the selected heads of one layer,
//                         for the rows of a teacher-forced pass → w [clip][head][row][S] f32
//   align_matrix_kernel   column statistics over the m rows, normalise, median filter along the frames, head mean,
//                         negate → M [clip][m][S_b] f32
//   dtw_kernel            the DTW of csrc/dtw.h on anti-diagonals, one workgroup per clip, one thread per row;
//                         backtrace and frame per token in the same launch
#include <algorithm>

#include "common.h"
#include "dtw.h"

namespace wcb {

// ------------------------------------------------------------------------------------------------ lengths
// ids [B][ld] (the n generated columns of every clip) → lens[b] = min(first EOS, n - 1) and the teacher-forced
// input tf [B][P + n - 1] = prefix, then g[0 .. n-2] (ids clamped into the vocabulary: the embedding's bound)
__global__ __launch_bounds__(64) void align_prep_kernel(const int* __restrict__ ids, int ld, int n,
                                                        const int* __restrict__ prefix, int P, int start_tok, int eos,
                                                        int vocab, int* __restrict__ tf, int* __restrict__ lens) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* g = ids + (long)b * ld;
  int first = n;
  for (int i = lane; i < n; i += 64)
    if (g[i] == eos) { first = i; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (lane == 0) lens[b] = min(first, n - 1);
  if (!tf) return;
  const int T = P + n - 1;
  for (int p = lane; p < T; p += 64) {
    const int v = p < P ? (prefix ? prefix[p] : start_tok) : g[p - P];
    tf[(long)b * T + p] = min(max(v, 0), vocab - 1);
  }
}

void align_prep(const int* ids, int ld, int n, const int* prefix, int P, int start_tok, int eos, int vocab, int B,
                int* tf, int* lens, hipStream_t s) {
  WCB_LAUNCH(align_prep_kernel, dim3(B), dim3(64), 0, s, ids, ld, n, prefix, P, start_tok, eos, vocab, tf, lens);
}

// ------------------------------------------------------------------------------------------------ capture
// One workgroup = 16 query rows of one (clip, selected head) against all S keys: scores as MFMA tiles with the
// keys as the A operand (a lane then holds 4 consecutive keys of one query: 16-byte stores), the wave w takes
// the 16-key tiles w, w + 4, ..., every score stays in registers through the softmax. S <= kAlignMaxS.
constexpr int kCapTiles = kAlignMaxS / 16 / 4;   // 16-key tiles per wave

// the address of the fragment of keys [16·t16, 16·t16 + 16) x columns [32·kk, 32·kk + 32) in lane order
template <typename T>
WCB_DEV const T* cap_key_frag(const AlignCapArgs& a, const T* kbase, int t16, int kk, int lane) {
  if (a.fm) {   // xenc_to_fm's chunk layout: [chunk of 32 keys][NW][2 halves][KSW][64 lanes][8]
    const int D = a.dim;
    const int NW = D >= 128 ? 4 : D / 32, CW = D / NW, KSW = CW / 32;
    const int col0 = 32 * kk, wv = col0 / CW, ks = (col0 % CW) / 32;
    const long frag = ((((long)(t16 >> 1)) * NW + wv) * 2 + (t16 & 1)) * KSW + ks;
    return kbase + frag * 512 + lane * 8;
  }
  const int key = min(16 * t16 + (lane & 15), a.S - 1);
  return kbase + (long)key * a.dim + 32 * kk + 8 * (lane >> 4);
}

template <typename T>
__global__ __launch_bounds__(256) void align_capture_kernel(AlignCapArgs a) {
  __shared__ float red[4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * 16, hs = blockIdx.y, clip = a.clip0 + blockIdx.z;
  const int head = a.head[hs], slot = a.slot[hs];
  // query row of this lane's MFMA column: position pos0 + j of the clip, alignment row i = that - P
  const int jq = j0 + (lane & 15);
  const int iq = a.pos0 + jq - a.P;
  const bool qok = jq < a.rps && iq >= 0 && iq < a.nrow;
  if (a.pos0 + j0 + 15 - a.P < 0 || a.pos0 + j0 - a.P >= a.nrow) return;   // no alignment row in this tile
  const T* qrow = reinterpret_cast<const T*>(a.q) + ((long)clip * a.rps + min(jq, a.rps - 1)) * a.ldq +
                  (long)head * a.q_hstride + 8 * (lane >> 4);
  const T* kbase = reinterpret_cast<const T*>(a.k) + (long)clip * a.k_clip + (a.xmode ? 0 : (long)head * a.S * 64);
  const int ntile = (a.S + 15) >> 4;
  f32x4 acc[kCapTiles];
#pragma unroll
  for (int t = 0; t < kCapTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < a.dim / 32; ++kk) {
    const auto qf = load_frag<T>(qrow + 32 * kk);
#pragma unroll
    for (int t = 0; t < kCapTiles; ++t) {
      const int t16 = wave + 4 * t;
      if (t16 < ntile) acc[t] = mma16(load_frag<T>(cap_key_frag<T>(a, kbase, t16, kk, lane)), qf, acc[t]);
    }
  }
  // acc[t][e] = score of key 16·(wave + 4t) + 4·(lane >> 4) + e for query lane & 15
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < kCapTiles; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int key = 16 * (wave + 4 * t) + 4 * (lane >> 4) + e;
      if (key >= a.S) acc[t][e] = -INFINITY;
      mx = fmaxf(mx, acc[t][e]);
    }
  mx = xor32_max(xor16_max(mx));
  if (lane < 16) red[wave][lane] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][lane & 15], red[1][lane & 15]), fmaxf(red[2][lane & 15], red[3][lane & 15]));
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < kCapTiles; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[t][e] = expf(acc[t][e] - mx);   // (masked keys: exp(-inf) = 0)
      sum += acc[t][e];
    }
  sum = xor32_add(xor16_add(sum));
  if (lane < 16) red[wave][lane] = sum;
  __syncthreads();
  sum = (red[0][lane & 15] + red[1][lane & 15]) + (red[2][lane & 15] + red[3][lane & 15]);
  if (!qok) return;
  float* wrow = a.w + ((((long)blockIdx.z * a.heads_total + slot) * a.nrow + iq) * a.S);
#pragma unroll
  for (int t = 0; t < kCapTiles; ++t) {
    const int key = 16 * (wave + 4 * t) + 4 * (lane >> 4);
    if (key + 3 < a.S && (a.S & 3) == 0) {   // (rows of S floats: 16-byte aligned only then)
      *reinterpret_cast<f32x4*>(wrow + key) = f32x4{acc[t][0] / sum, acc[t][1] / sum, acc[t][2] / sum, acc[t][3] / sum};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (key + e < a.S) wrow[key + e] = acc[t][e] / sum;
    }
  }
}

void align_capture(DType t, const AlignCapArgs& a, hipStream_t s) {
  const dim3 grid((a.rps + 15) / 16, a.nh, a.nclip);
  switch (t) {
    case kBF16: WCB_LAUNCH(align_capture_kernel<bf16_t>, grid, dim3(256), 0, s, a); break;
    case kF16: WCB_LAUNCH(align_capture_kernel<f16_t>, grid, dim3(256), 0, s, a); break;
    case kF32: WCB_LAUNCH(align_capture_kernel<float>, grid, dim3(256), 0, s, a); break;
  }
}

// ------------------------------------------------------------------------------------------------ matrix
// One workgroup = 32 frame columns of one clip over every head and row: thread (cx = column, ry = row lane of 8).
// Per head: mean and 1 / std of the 32 + W - 1 columns the median windows touch (reflect padding at both ends of
// [0, S_b)), in f64 over the m rows; then per (row, column) the median of the W normalised neighbours, summed
// over the heads in head order into acc [m][32] (LDS). A column with std = 0 normalises to 0.
constexpr int kMatCols = 32, kMatRows = 8;

// reflect padding of [0, S); clamped: a halo column no kept window reads may lie further out than one reflection
WCB_DEV int reflect(int s, int S) {
  const int r = s < 0 ? -s : s >= S ? 2 * (S - 1) - s : s;
  return min(max(r, 0), S - 1);
}

template <int W>
__global__ __launch_bounds__(256) void align_matrix_kernel(const float* __restrict__ w, int heads, int m_max, int S_ld,
                                                           const int* __restrict__ lens, const int* __restrict__ frames,
                                                           float* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int HC = kMatCols + W - 1;
  double* part = reinterpret_cast<double*>(lds);            // [kMatRows][HC]
  double* mean = part + kMatRows * HC;                      // [HC]
  double* rstd = mean + HC;                                 // [HC]
  float* acc = reinterpret_cast<float*>(rstd + HC);         // [m][kMatCols]
  const int b = blockIdx.y, s0 = blockIdx.x * kMatCols;
  const int m = min(lens[b], m_max), Sb = frames ? min(frames[b], S_ld) : S_ld;
  if (m <= 0 || s0 >= Sb || Sb < W) return;
  const int tid = threadIdx.x, cx = tid & (kMatCols - 1), ry = tid / kMatCols;
  for (int i = tid; i < m * kMatCols; i += 256) acc[i] = 0.f;
  for (int h = 0; h < heads; ++h) {
    const float* wh = w + ((long)b * heads + h) * m_max * S_ld;
    for (int pass = 0; pass < 2; ++pass) {   // 0: Σ w → mean; 1: Σ (w - mean)² → 1 / std
      for (int hc = cx; hc < HC; hc += kMatCols) {
        const int col = reflect(s0 + hc - W / 2, Sb);
        const double mu = pass ? mean[hc] : 0.0;
        double sum = 0.0;
        for (int i = ry; i < m; i += kMatRows) {
          const double v = (double)wh[(long)i * S_ld + col] - mu;
          sum += pass ? v * v : v;
        }
        part[ry * HC + hc] = sum;
      }
      __syncthreads();
      if (tid < HC) {
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < kMatRows; ++r) sum += part[r * HC + tid];
        if (pass) rstd[tid] = sum > 0.0 ? 1.0 / sqrt(sum / m) : 0.0;
        else mean[tid] = sum / m;
      }
      __syncthreads();
    }
    if (s0 + cx < Sb) {
      for (int i = ry; i < m; i += kMatRows) {
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const int col = reflect(s0 + cx + k - W / 2, Sb);
          z[k] = (float)(((double)wh[(long)i * S_ld + col] - mean[cx + k]) * rstd[cx + k]);
        }
        // the W / 2 + 1 smallest in order (selection on compile-time indices: registers)
#pragma unroll
        for (int p = 0; p <= W / 2; ++p)
#pragma unroll
          for (int q = p + 1; q < W; ++q) {
            const float lo = fminf(z[p], z[q]), hi = fmaxf(z[p], z[q]);
            z[p] = lo; z[q] = hi;
          }
        acc[i * kMatCols + cx] += z[W / 2];
      }
    }
    __syncthreads();   // mean / rstd are rewritten by the next head
  }
  if (s0 + cx < Sb)
    for (int i = ry; i < m; i += kMatRows)
      M[((long)b * m_max + i) * S_ld + s0 + cx] = -(acc[i * kMatCols + cx] / (float)heads);
}

size_t align_matrix_lds(int W, int m_max) {
  const int HC = kMatCols + W - 1;
  return (size_t)(kMatRows + 2) * HC * 8 + (size_t)std::max(m_max, 1) * kMatCols * 4;
}

bool align_matrix(const float* w, int N, int heads, int m_max, int S_ld, const int* lens, const int* frames, int W,
                  float* M, hipStream_t s) {
  const dim3 grid((S_ld + kMatCols - 1) / kMatCols, N);
  const size_t sh = align_matrix_lds(W, m_max);
#define WCB_AM(WW)                                                                                                  \
  case WW: {                                                                                                        \
    static bool attr = false;                                                                                       \
    if (!attr) {                                                                                                    \
      (void)hipFuncSetAttribute((const void*)align_matrix_kernel<WW>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                (int)align_matrix_lds(WW, kAlignMaxRows));                                          \
      attr = true;                                                                                                  \
    }                                                                                                               \
    WCB_LAUNCH(align_matrix_kernel<WW>, grid, dim3(256), sh, s, w, heads, m_max, S_ld, lens, frames, M);            \
    return true;                                                                                                    \
  }
  switch (W) { WCB_AM(1) WCB_AM(3) WCB_AM(5) WCB_AM(7) WCB_AM(9) WCB_AM(11) WCB_AM(13) WCB_AM(15) default: return false; }
#undef WCB_AM
}

// ------------------------------------------------------------------------------------------------ DTW
// Thread t owns row t of the clip's matrix and walks its columns; at step k it is at column k - t, so a step is
// one anti-diagonal. It needs its own previous cost ("left") and thread t-1's last two ("up", and the one before
// as the diagonal): by a wave shuffle, and for lane 0 of a later wave through an LDS slot per wave and parity
// with one workgroup barrier per step — a clip of at most 64 rows runs in one wave and takes no barrier in the
// sweep. The matrix values of the next kDtwU steps are loaded while the current ones are consumed. The trace is
// packed 2 bits per cell, 16 cells of a row per word, in LDS when the launch's [m_max][words] fits and in the
// given workspace otherwise. Thread 0 then walks the path back from (m, S), writing the frame of every row.
constexpr int kDtwU = 8;

__global__ __launch_bounds__(kAlignMaxRows + 1) void dtw_kernel(DtwArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xch = reinterpret_cast<float*>(lds);   // [2][8]
  int* bc = reinterpret_cast<int*>(lds + 64);   // [4]: path length, frame of the last row
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m = max(0, min(a.lens[b], a.m_max));
  const int S = a.frames ? max(1, min(a.frames[b], a.S_ld)) : a.S_ld;
  const int words = dtw_trace_words(a.S_ld);
  unsigned* trace = a.trace ? a.trace + (long)b * a.m_max * words : reinterpret_cast<unsigned*>(lds + 128);
  int* outf = a.out_frames + (long)b * a.n_out;
  if (m == 0) {
    for (int i = t; i < a.n_out; i += blockDim.x) outf[i] = 0;
    if (t == 0 && a.path_len) a.path_len[b] = 0;
    return;
  }
  const bool multi = m > 64;   // uniform in the workgroup
  if (t < 16) xch[t] = INFINITY;
  if (multi) __syncthreads();
  const bool row = t < m;
  const float* Mrow = a.M + ((long)b * a.m_max + (row ? t : 0)) * a.S_ld;
  float val = INFINITY;                       // this row's last cost: cost[t+1][0] = inf before its first column
  float diag = t == 0 ? 0.f : INFINITY;       // cost[t][column - 1] of the step ahead
  unsigned word = 0;
  const int nstep = m + S - 1;
  float cur[kDtwU], nxt[kDtwU];
#pragma unroll
  for (int u = 0; u < kDtwU; ++u) {
    const int j = u - t;
    cur[u] = (row && j >= 0 && j < S) ? Mrow[j] : 0.f;
  }
  for (int k0 = 0; k0 < nstep; k0 += kDtwU) {
#pragma unroll
    for (int u = 0; u < kDtwU; ++u) {
      const int j = k0 + kDtwU + u - t;
      nxt[u] = (row && j >= 0 && j < S) ? Mrow[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kDtwU; ++u) {
      const int k = k0 + u;
      if (k < nstep) {   // uniform
        const int j = k - t;
        float up = __shfl_up(val, 1, 64);
        if (lane == 0) up = wave == 0 ? INFINITY : xch[((k + 1) & 1) * 8 + wave - 1];
        if (row && j >= 0 && j < S) {
          float c;
          const int tr = dtw_cell(diag, up, val, cur[u], c);
          val = c;
          word |= (unsigned)tr << ((j & 15) * 2);
          if ((j & 15) == 15 || j == S - 1) {
            trace[t * words + (j >> 4)] = word;
            word = 0;
          }
        }
        diag = up;
        if (multi) {
          if (lane == 63) xch[(k & 1) * 8 + wave] = val;
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kDtwU; ++u) cur[u] = nxt[u];
  }
  __syncthreads();
  if (t == 0) {
    int i = m, j = S, len = 0, last = 0;
    int* pt = a.path_text ? a.path_text + (long)b * a.path_ld : nullptr;
    int* pj = a.path_time ? a.path_time + (long)b * a.path_ld : nullptr;
    while ((i > 0 || j > 0) && len < m + S) {   // (a walk is at most m + S - 1 cells)
      if (pt && len < a.path_ld) { pt[len] = i - 1; pj[len] = j - 1; }
      ++len;
      if (i >= 1) outf[i - 1] = j - 1;   // the last visit of a row, in this order, is its first path cell
      if (i == m) last = j - 1;
      const int stored = (i > 0 && j > 0) ? dtw_trace_get(trace + (i - 1) * words, j - 1) : 0;
      dtw_back(dtw_border(i, j, stored), i, j);
    }
    bc[0] = len;
    bc[1] = m <= 1 ? 0 : last;
    if (a.path_len) a.path_len[b] = len;
  }
  __syncthreads();
  const int len = bc[0], last = bc[1];
  for (int i = m + t; i < a.n_out; i += blockDim.x) outf[i] = last;
  if (a.path_text) {   // the walk wrote the path backwards
    int* pt = a.path_text + (long)b * a.path_ld;
    int* pj = a.path_time + (long)b * a.path_ld;
    for (int p = t; p < len / 2; p += blockDim.x) {
      const int q = len - 1 - p;
      const int x = pt[p], y = pj[p];
      pt[p] = pt[q]; pj[p] = pj[q];
      pt[q] = x; pj[q] = y;
    }
  }
}

size_t dtw_trace_bytes(int m_max, int S_ld) { return (size_t)std::max(m_max, 1) * dtw_trace_words(S_ld) * 4; }

void dtw(const DtwArgs& a, int N, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dtw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 + kDtwLdsTrace);
    attr = true;
  }
  const int threads = std::max(64, (a.m_max + 63) / 64 * 64);
  const size_t sh = 128 + (a.trace ? 0 : dtw_trace_bytes(a.m_max, a.S_ld));
  WCB_LAUNCH(dtw_kernel, dim3(N), dim3(threads), sh, s, a);
}

}  // namespace wcb
