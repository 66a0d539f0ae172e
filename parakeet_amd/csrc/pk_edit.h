// pk_edit.h -- definition, layout and envelope of the edit (Levenshtein) distance of token sequences and its alignment
// (edit.hip): what word / character / phone error rates are counted from (parakeet_amd/utils/error_rate.py).
//
// One pair: ref, N >= 0 int32 ids, and hyp, M >= 0 int32 ids.  Any int32 value is an id; only equality is used.
//   forward:   cells 0 <= i <= N, 0 <= j <= M, int32.  D(i, 0) = i, D(0, j) = j; for i, j >= 1:
//              D(i, j) = D(i - 1, j - 1)                                           if ref[i - 1] == hyp[j - 1],
//                        1 + min(D(i - 1, j - 1), D(i - 1, j), D(i, j - 1))        otherwise.
//              distance = D(N, M).  (The recurrence of parakeet/utils/error_rate.py; its shortcuts for equal and for empty
//              sequences and its swap to the shorter row are properties of the result, not rules of their own.)
//   alignment: this project's own (that module returns the distance alone).  Walk back from (N, M): at i = 0 the step is an
//              insertion (to (0, j - 1)), at j = 0 a deletion (to (i - 1, 0)); where ref[i - 1] == hyp[j - 1] it is a hit and
//              goes to (i - 1, j - 1); otherwise, among the predecessors whose value is D(i, j) - 1, the substitution
//              (i - 1, j - 1) is taken first, then the deletion (i - 1, j), then the insertion (i, j - 1): the tie order of
//              pk_dtw.h.
//   outputs:   distance (int32); the ops in forward order as uint8 -- 0 hit, 1 substitution, 2 deletion, 3 insertion --, their
//              number P with max(N, M) <= P <= N + M (a pair's buffer has N + M entries; those from P on are never written);
//              the counts H, S, D, I (int32) of the four ops.  S + D + I = distance, H + S + D = N, H + S + I = M.
//   N = 0, M = 0 and both are valid pairs (M insertions, N deletions, nothing).
//
// k_edit<R, MODE>: one wave per pair, the structure of k_dtw (pk_dtw.h).  The rows 1 ... N are cut into strips of
// R = edit_strip_rows(N) rows (1, 2, 4, 8 or 16); strip g holds rows g * R + 1 ... g * R + R, a pass is 64 strips, lane l owns
// strip pass * 64 + l, keeps its ref ids and its D of the previous column in registers and works, at step t, on column
// t - l + 1.  The bottom value of lane l - 1 arrives by one DPP wave shift (the values are int32), the diagonal neighbour is the
// value received one step earlier; the last row of a pass is carried to the next through a global row of M int32 (two rows,
// used alternately).  The hyp ids are read EDIT_AHEAD columns at a time, one block ahead of the one being computed.
// The chain per cell is one addition and one minimum: with e = D(i - 1, j - 1) on equal ids and 1 + min(D(i - 1, j - 1),
// D(i, j - 1)) otherwise -- which does not wait for the cell above --, D(i, j) = min(e, D(i - 1, j) + 1).  That is the
// definition: neighbouring cells of D differ by at most 1, so on equal ids D(i - 1, j - 1) <= D(i - 1, j) + 1.
// MODE 0 stops there.  MODE 1 keeps the 2-bit op of every cell (what the walk back takes there: the codes above) in one 32-bit
// word per strip and column, bits 2 r, 2 r + 1 for row g * R + r + 1, at (j - 1) * G + g with G = ceil(N / R) strips: a pair has
// M * G words.  They stay in LDS while that number is at most EDIT_LDS_WORDS; above it they go to a global workspace (128-byte
// aligned per pair) and come back for the walk in blocks of floor(EDIT_LDS_WORDS / G) whole columns.  The walk runs on LDS,
// every lane alike; the reversed ops are staged in a global workspace, 64 at a time, and written out forward once P is known.
#pragma once
#include <cstdint>

constexpr int EDIT_MAX_LEN = 4096;         // N, M (the limit of pk_dtw.h)
constexpr int EDIT_MAX_STRIP = 16;         // R: one 32-bit word holds a strip's ops of a column
constexpr int EDIT_PASS_ROWS = 64 * EDIT_MAX_STRIP;
constexpr int EDIT_LDS_WORDS = 12288;      // 32-bit op words of a pair that stay in LDS (48 KiB); the stage of a global store
constexpr int EDIT_AHEAD = 8;              // columns of hyp ids (and of the carry row) read ahead as one block

// rows of a strip: the smallest of 1, 2, 4, 8, 16 with 64 strips covering N (16 from N = 513 on: longer ref takes several passes)
static inline int edit_strip_rows(int N) {
    int R = 1;
    while (R < EDIT_MAX_STRIP && 64 * R < N) R *= 2;
    return R;
}
static inline int edit_strips(int N) { return (N + edit_strip_rows(N) - 1) / edit_strip_rows(N); }
// 32-bit op words of an N x M pair (mode 1)
static inline long edit_words(int N, int M) { return (long)M * edit_strips(N); }
