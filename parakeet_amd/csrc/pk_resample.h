// pk_resample.h -- geometry of the ragged polyphase FIR kernel (resample.hip).
//
// Output n of an utterance uses phase (n * down) mod up and input base floor(n * down / up).  A tile is up * C * R consecutive
// outputs that start at an utterance-relative multiple of the tile, so its first output has phase 0 and input base
// tile_index * C * R * down exactly: everything inside a tile is a small int relative to that base.
// A work item (g, c) owns A * R outputs: the A neighbouring residues r = A * g + a of the output index mod up, and of each
// the R outputs  r + (c * R + q) * up, q = 0 ... R - 1.  The R outputs of a residue share its phase (r * down) mod up, so a
// coefficient is loaded once and used R times; their inputs lie `down` samples apart.  The A residues have input bases
// within D = ceil((A - 1) * down / up) samples of each other, so with their rows of the table shifted against each other
// by that difference (and padded with zeros to taps + D steps) they walk the same input samples: a sample is read from
// LDS once and used A times.
#pragma once
#include <cstdint>

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_SPAN = 16128;       // floats of a tile's input span in LDS (63 KiB)
constexpr int RS_MAX_TILE = 4096;        // outputs per tile, unless one period (`up` outputs) is longer
constexpr int RS_MAX_RATIO = 4096;       // 1 <= up, down
constexpr int RS_MAX_TAPS = 8192;
constexpr long RS_MAX_TABLE = 4L << 20;  // up * taps, floats

struct rs_plan {
    int R = 1, C = 1, A = 1;             // outputs per residue, work items per residue group, residues per work item
    int G = 1;                           // residue groups: ceil(up / A)
    int D = 0;                           // the largest shift between the rows of a group
    int steps = 0;                       // taps + D: input samples a work item walks per q
    int tile = 0;                        // up * C * R
    int span = 0;                        // C * R * down + steps - 1 input samples staged per tile
};

// The plan of a (up, down, taps) handle: the admissible (R, C) -- span within RS_MAX_SPAN, tile within RS_MAX_TILE -- that
// keeps most of the 256 threads busy with the most coefficient reuse.  R = C = 1 is always admissible inside the envelope.
static inline rs_plan rs_make_plan(int up, int down, int taps) {
    rs_plan best;
    best.A = up >= 2 ? 2 : 1;
    best.G = (up + best.A - 1) / best.A;
    best.D = (int)(((long)(best.A - 1) * down + up - 1) / up);
    best.steps = taps + best.D;
    double best_score = -1.0;
    for (int R = 8; R >= 1; R >>= 1)
        for (int C = 1; C <= RS_THREADS * 4; ++C) {
            const long cr = (long)C * R;
            if (cr * down + best.steps - 1 > RS_MAX_SPAN) break;
            if (cr * up > RS_MAX_TILE && cr > 1) break;
            const long items = (long)best.G * C;
            const long slots = (items + RS_THREADS - 1) / RS_THREADS * RS_THREADS;
            const double score = (double)items / (double)slots * R / (R + 2.0);
            if (score > best_score * (1.0 + 1e-9)) {
                best_score = score;
                best.R = R;
                best.C = C;
            }
        }
    best.tile = up * best.C * best.R;
    best.span = best.C * best.R * down + best.steps - 1;
    return best;
}
