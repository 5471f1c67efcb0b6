// Dynamic time warping of the token-timestamp alignment (transformers' _dynamic_time_warping, the function HF's
// _extract_token_timestamps runs on the host). One definition of the recurrence: the DTW kernel (k_align.hip)
// and the host function wcb_dtw_host compile these very functions, so the two paths are equal bit for bit.
//
// For a cost matrix M [m rows = tokens][S columns = frames], all in f32:
//   cost[0][0] = 0, cost[0][j > 0] = cost[i > 0][0] = +inf
//   cost[i][j] = M[i-1][j-1] + c,  c = the diagonal cost[i-1][j-1] if it is strictly less than both others (trace 0),
//                else "up" cost[i-1][j] if strictly less than both (trace 1), else "left" cost[i][j-1] (trace 2)
//   backtrace from (m, S): trace 0 → (i-1, j-1), 1 → (i-1, j), 2 → (i, j-1); row 0 counts as trace 2, column 0 as
//   trace 1 (so the walk ends at (0, 0)); every visited (i, j) is the path cell (text i-1, time j-1)
//   frame[i] = the time index of the first path cell (in forward order) whose text index is i
// A comparison with a NaN is false, as in numpy: the choice falls through to "left".
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WCB_DTW_HD __host__ __device__ __forceinline__
#else
#define WCB_DTW_HD inline
#endif

namespace wcb {

// one cell: the three-way choice and the f32 add; returns the trace (0 diagonal, 1 up, 2 left)
WCB_DTW_HD int dtw_cell(float diag, float up, float left, float m, float& cost) {
  int t;
  float c;
  if (diag < up && diag < left) { c = diag; t = 0; }
  else if (up < diag && up < left) { c = up; t = 1; }
  else { c = left; t = 2; }
  cost = m + c;   // an add alone: nothing to contract into a fused multiply-add
  return t;
}

// the trace the backtrace follows at (i, j): the borders override the stored value
WCB_DTW_HD int dtw_border(int i, int j, int stored) { return i == 0 ? 2 : j == 0 ? 1 : stored; }

// one backtrace step
WCB_DTW_HD void dtw_back(int trace, int& i, int& j) {
  i -= trace != 2;   // 0: both, 1: the row, 2: the column
  j -= trace != 1;
}

// the trace packed 2 bits per cell, 16 cells of one row per 32-bit word: cell (row r, column c), 0-based
WCB_DTW_HD int dtw_trace_words(int S) { return (S + 15) >> 4; }
WCB_DTW_HD int dtw_trace_get(const unsigned* row_words, int c) { return (row_words[c >> 4] >> ((c & 15) * 2)) & 3; }

}  // namespace wcb
