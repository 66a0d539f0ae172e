// pk_stats.h -- definition, summation order and envelope of the streaming feature statistics (stats.hip).
//
// STATE of an accumulator over feature dimension D:
//   n      rows seen (int64);
//   K[c]   the shift (D x float32), fixed ONCE: the caller's shift, else the first row the accumulator ever sees (row 0 of the
//          first non-empty utterance of the first update that has one);
//   S1[c]  = sum_r (x[r, c] - K[c])      float64;
//   S2[c]  = sum_r (x[r, c] - K[c])^2    float64.
// ARITHMETIC: d = (double)x[r, c] - (double)K[c] (exact operands, one IEEE subtraction); q = d * d (one IEEE product);
// every sum below is a chain of single IEEE float64 additions -- nothing is contracted into an fma.  Every accumulator
// starts at +0.0.
//
// THE ORDER.  An utterance of L rows is cut into tiles of R = stats_tile_rows(D) rows anchored at ITS first row: tile i holds
// the utterance's rows i R ... min(L, (i + 1) R) - 1; there are ceil(L / R) tiles (none for L = 0).  One workgroup of
// STATS_THREADS = 256 work items sums one tile:
//   the map     CW = stats_col_width(D) = min(64, the smallest power of two >= D) column slots, G = 256 / CW row slots;
//               work item t has column slot j = t % CW and row slot g = t / CW.
//                 D >= 33 (CW = 64, G = 4): a wave is a row slot, its lanes read 64 consecutive floats of one row (wide map);
//                 D <= 32 (CW < 64): a wave covers 64 / CW consecutive rows x CW columns, i.e. (row, column) pairs; for
//                 D = 1 every lane of the workgroup owns a row slot (narrow map).
//               Columns are taken in chunks c0 = 0, CW, 2 CW, ...: slot j owns column c = c0 + j (idle where c >= D).
//   a slot      for its column, row slot g adds the tile's rows g, g + G, g + 2 G, ... ascending to p1[g], p2[g];
//   the slots   for (s = G / 2; s >= 1; s /= 2) p[g] = p[g] + p[g + s] for every g < s at once (a halving tree);
//               the tile's partial sums are p1[0], p2[0].
// An utterance's sums U1[c], U2[c] are its tiles' partials added in ascending tile order to an accumulator that starts at
// +0.0 (an empty utterance has U = 0).  The utterances' sums are added to the state in call order: S = S + U_b for
// b = 0, 1, ..., B - 1 of an update, update after update.  None of this depends on the batch, the grid, any other utterance
// or where the utterance lies in the packed buffer: an utterance's U is the same bytes alone and in any batch for a given
// K, and a corpus gives the same state bytes in any split into updates at utterance boundaries.
//
// DERIVED (host, float64): mean = K + S1 / n; var = max(S2 - S1^2 / n, 0) / n (population variance); scale = sqrt(var), set
// to 1 where var <= n eps var + (n eps mean)^2 (eps = 2^-52: scikit-learn's constant-feature test).  NaN and Inf propagate.
//
// ENVELOPE (else PK_EUNSUPPORTED, before any launch): 1 <= D <= STATS_MAX_DIM; every lens[b] <= 2^31 - 1; at most
// STATS_MAX_TILES tiles in one update.  The sum of the lengths is 64-bit.
#pragma once
#include <cstdint>

constexpr int STATS_MAX_DIM = 1024;
constexpr int STATS_THREADS = 256;
constexpr long STATS_MAX_TILES = 1L << 24;
constexpr int STATS_UNROLL = 8;   // rows a slot loads before it adds them (in order)
constexpr int STATS_FOLD_COLS = 32;    // k_stats_fold: values of the 2 D sums per workgroup ...
constexpr int STATS_FOLD_ROWS = 256;   // ... and utterances staged in LDS at a time (64 KiB); neither changes the order

static inline int stats_col_width(int D) {
    int cw = 1;
    while (cw < D && cw < 64) cw *= 2;
    return cw;
}
// rows per tile: about 32768 floats (128 KiB), a power of two in 32 ... 4096
static inline int stats_tile_rows(int D) {
    const int cw = stats_col_width(D), nc = (D + cw - 1) / cw;
    int r = 4096;
    while (r > 32 && (long)r * cw * nc > 32768) r /= 2;
    return r;
}
