// pk_dtw.h -- definition, layout and envelope of dynamic time warping and the statistics along its path (dtw.hip).
// The definition is this project's own: no band constraint, no slope weights, the squared Euclidean distance as the local cost.
//
// One pair: N >= 1 rows (frames of x), M >= 1 columns (frames of y).
//   local cost, matrix mode:  c(i, j) is a given float32.
//   local cost, feature mode: x is (N, D) float32, y is (M, D) float32, a column range [k0, k1) is given.  s = 0.0 (float64);
//              for k = k0 ... k1 - 1 ascending: d = (double)x[i, k] - (double)y[j, k]; s = s + d * d -- every operation a separate
//              IEEE float64 operation (no fused multiply-add); c(i, j) = (float)s, one rounding to nearest.
//   forward:   float64, every c converted exactly.  Q(0, 0) = c(0, 0); Q(i, j) = c(i, j) + min(Q(i - 1, j - 1), Q(i - 1, j),
//              Q(i, j - 1)) with +inf outside the matrix: one addition per cell.
//   decision:  the predecessor of (i, j) is the smallest of the three; ties go to the diagonal first, then to (i - 1, j), then to
//              (i, j - 1).  In row 0 the predecessor is (0, j - 1) and in column 0 it is (i - 1, 0) whatever the values are (on
//              finite costs that is what the rule gives; it keeps a path with status 1 inside the matrix).
//   backtrack: from (N - 1, M - 1) to (0, 0); the path is returned in forward order as ix, iy (int32, length P,
//              max(N, M) <= P <= N + M - 1).  The path buffer of a pair has N + M - 1 entries; those from P on are never written.
//   outputs:   P, the path, cost = Q(N - 1, M - 1) (float64), status = 1 iff some c(i, j) is not finite (the path is then
//              unspecified), else 0.
//
// k_dtw: one wave per pair.  Rows are cut into strips of R = dtw_strip_rows(N) contiguous rows (R in {1, 2, 4, 8, 16}), strip g
// holds rows g * R ... g * R + R - 1; a pass is 64 strips (DTW_PASS_ROWS = 1024 rows at R = 16), lane l owns strip pass * 64 + l
// and keeps its Q of the previous column in registers.  Lanes run skewed: at step t lane l works on column t - l.  The bottom
// value of lane l - 1 arrives by a cross-lane move, the diagonal neighbour is the value received one step earlier; the last row
// of a pass is carried to the next pass through a global row of M doubles (two rows, used alternately).  Costs are read
// DTW_AHEAD(R) columns at a time, one block ahead of the one being computed.
// Decision words: the 2-bit decisions (0 diagonal, 1 up, 2 left) of strip g in column j are one 32-bit word, bits 2 r, 2 r + 1
// for row g * R + r; the word is at j * G + g with G = ceil(N / R) strips: a pair has M * G words.  They stay in LDS while that
// number is at most DTW_LDS_WORDS; above it they go to a global workspace (128-byte aligned per pair) and come back for the
// backtrack in blocks of floor(DTW_LDS_WORDS / G) whole columns, by independent coalesced loads.
// The backtrack walks on LDS, every lane alike; the reversed path is staged in a global workspace (i << 16 | j) and written
// out forward once P is known.
//
// k_dtw_cost: feature mode's cost matrix, DTW_TILE x DTW_TILE cells per workgroup, the x and y tiles in LDS.  In pk_dtw_run it
// writes into a grow-only workspace of the context; a call whose matrices exceed the cap (DTW_COST_CAP_BYTES unless
// pk_dtw_cost_cap set another) is run in several launches over consecutive pairs in the caller's order (a launch holds at
// least one pair, so the workspace never exceeds max(cap, 4 N M bytes of the largest pair)).
//
// Path statistics of one pair: a path (ix, iy, length P), the feature streams with a column range as above, optional uint8
// masks mx (N), my (M).  s_p is the float64 s of (ix[p], iy[p]) before its rounding to float32.
//   sum_sq = sum s_p, sum_sqrt = sum sqrt(s_p) over the steps with mx[ix[p]] != 0 and my[iy[p]] != 0 (all steps without masks);
//   n11, n10, n01, n00 (int64): the steps by (mx != 0, my != 0), over all steps (without masks n11 = P).
// THE ORDER of the float64 sums: one workgroup of DTW_STATS_THREADS work items per pair; item t adds the terms of steps t,
// t + DTW_STATS_THREADS, t + 2 DTW_STATS_THREADS, ... ascending to a_t = 0.0 (a step outside the masks adds nothing); then
// for h = DTW_STATS_THREADS / 2, / 4, ..., 1: a_t = a_t + a_(t + h) for t < h; the sum is a_0.
// status = 2 iff a path entry lies outside the pair (that step is left out), else 0.
#pragma once
#include <cstdint>

constexpr int DTW_MAX_ROWS = 4096;        // N
constexpr int DTW_MAX_COLS = 4096;        // M
constexpr int DTW_MAX_DIM = 128;          // D
constexpr int DTW_MAX_STRIP = 16;         // R: one 32-bit word holds a strip's decisions of a column
constexpr int DTW_PASS_ROWS = 64 * DTW_MAX_STRIP;
constexpr int DTW_LDS_WORDS = 12288;      // 32-bit decision words of a pair that stay in LDS (48 KiB); the stage of a global store
constexpr int DTW_TILE = 32;              // k_dtw_cost: cells per side of a workgroup's tile
constexpr int DTW_COST_THREADS = 256;
constexpr int DTW_STATS_THREADS = 256;
constexpr long DTW_COST_CAP_BYTES = 256L << 20;

// rows of a strip: the smallest of 1, 2, 4, 8, 16 with 64 strips covering N (16 from N = 513 on: longer x takes several passes)
static inline int dtw_strip_rows(int N) {
    int R = 1;
    while (R < DTW_MAX_STRIP && 64 * R < N) R *= 2;
    return R;
}
static inline int dtw_strips(int N) { return (N + dtw_strip_rows(N) - 1) / dtw_strip_rows(N); }
// 32-bit decision words of an N x M pair
static inline long dtw_words(int N, int M) { return (long)M * dtw_strips(N); }
// columns read ahead as one block by a lane that owns R rows: about 64 values in flight
constexpr int DTW_AHEAD(int R) { return R >= 16 ? 4 : 8; }
