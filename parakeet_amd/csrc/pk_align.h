// pk_align.h -- definition, layout and envelope of the monotonic alignment search and the focus rate (align.hip).
//
// Monotonic alignment search of one utterance: S rows (decoder steps) x T columns (tokens), 1 <= T <= S, scores v[s, t]
// (float32, higher is better).  A path has t(0) = 0, t(S - 1) = T - 1, t(s + 1) - t(s) in {0, 1}.
//   forward:   Q(0, 0) = v(0, 0); Q(s, t) = v(s, t) + max(Q(s - 1, t), Q(s - 1, t - 1)) for t <= s, in float64 (v converted
//              exactly: one IEEE addition per cell, no product); Q(s, t) = -inf for t > s and for t = -1.
//   backtrack: from (S - 1, T - 1); at row s >= 1 in column t stay in t iff Q(s - 1, t) >= Q(s - 1, t - 1) (ties stay), else go
//              to t - 1.
//   outputs:   durations[t] = rows of the path in column t (each >= 1, sum S), path[s], score = Q(S - 1, T - 1),
//              status = 1 iff a v(s, t) with t <= s is not finite (the durations are then unspecified), else 0.
//   attention: v = logf(A < eps ? eps : A), formed on the device (a NaN stays a NaN).
// Entries with t > s are never used (they may hold anything); entries outside the S x T map are never read.
//
// k_mas: one wave per utterance.  Lane l owns the C = ceil(T / 64) columns l * C ... l * C + C - 1 and keeps their Q of the
// previous row in registers; Q(s - 1, l * C - 1) arrives from lane l - 1 by a cross-lane move.  Rows are read MAS_ROWS(C)
// at a time, one block ahead of the one being computed.  The decision "go to t - 1" of column l * C + c at row s is bit l of
// the 64-bit word c of row s: a row is C words = 2 * C 32-bit words, an utterance S * 2 * ceil(T / 64) of them.  They stay
// in LDS while that number is at most MAS_LDS_WORDS; above it they go to a global workspace (sized from the batch's
// utterances that need it) and come back for the backtrack MAS_STAGE_WORDS64 words at a time, read ahead into LDS.
//
// Focus rate of a map: F = (1 / S) sum_s max_t A[s, t].  The row maximum is taken in fp32 (exact; a NaN entry is skipped by
// fmaxf).  THE ORDER of the float64 sum: one workgroup of FR_WAVES waves per map; wave w adds the maxima of rows w,
// w + FR_WAVES, w + 2 FR_WAVES, ... ascending to a_w = 0; F = ((a_0 + a_1) + (a_2 + a_3)) / (double)S.
#pragma once
#include <cstdint>

constexpr int MAS_MAX_COLS = 1024;        // T
constexpr int MAS_MAX_ROWS = 16384;       // S
constexpr int MAS_MAX_C = MAS_MAX_COLS / 64;
constexpr int MAS_LDS_WORDS = 12288;      // 32-bit decision words of an utterance that stay in LDS (48 KiB)
constexpr int MAS_STAGE_WORDS64 = 1024;   // 64-bit words of a global store's rows staged in LDS at a time (8 KiB)
constexpr int FR_THREADS = 256;
constexpr int FR_WAVES = FR_THREADS / 64;

// rows read ahead as one block by a lane that owns C columns: about 32 values in flight
constexpr int MAS_ROWS(int C) { return 32 / C < 2 ? 2 : 32 / C; }

static inline int mas_cols_per_lane(int T) { return (T + 63) / 64; }
// 32-bit decision words of an S x T utterance
static inline long mas_words(long S, int T) { return S * 2 * mas_cols_per_lane(T); }
