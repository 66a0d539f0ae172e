// pk_pitch.h -- geometry of the pitch estimator's kernel (pitch.hip).
//
// Frame i of an utterance reads L = W + tau_max samples from s = i * hop - L / 2 (zeros outside the utterance) and needs
//   d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2,   tau = 1 ... tau_max.
// A tile is F consecutive frames of one utterance, staged once in LDS: (F - 1) * hop + L samples (plus the few a lag group
// past tau_max reads).  A work item (f, g) owns frame f of the tile and the R neighbouring lags 1 + g R ... 1 + g R + R - 1:
// it reads x[s + j] once per j (the same LDS address for all lag groups of a frame: a broadcast) and keeps
// x[s + j + tau ... tau + R - 1] in a sliding register window, one new LDS read per j.  Work items are dealt to the lanes
// with g fastest, so neighbouring lanes read window addresses R words apart: R is ODD, which puts the 32 lanes of a
// ds_read_b32 group on 32 different banks.
#pragma once
#include <cstdint>

constexpr int PT_THREADS = 256;
constexpr int PT_R = 9;                  // lags per work item (odd: see above)
constexpr int PT_MAX_TAU = 960;          // tau_max: 48 kHz at f0min 50 Hz
constexpr int PT_MAX_HOP = 16384;
constexpr int PT_MAX_F = 32;             // frames per tile
constexpr int PT_MAX_LDS = 16128;        // floats of LDS per workgroup: the staged span and the F rows of d (63 KiB)
constexpr int PT_SCAN_CHUNK = 256;       // frames per scan step of the continuous-f0 kernel
// the tracker (k_pitch_cand, k_pitch_viterbi)
constexpr int PTK_MAX_K = 8;             // candidates per frame: the 64 lanes of a wave are the 8 x 8 (predecessor, state) pairs
constexpr int PTK_SLOTS = (PT_MAX_TAU + 63) / 64;   // lags per lane of the candidate kernel
constexpr int PTK_CH = 64;               // frames whose candidates are staged in LDS at a time
constexpr int PTK_BP_LDS = 4096;         // frames whose backpointer words (8 bytes each) stay in LDS; longer tracks use a workspace
constexpr int PTK_MAX_FRAMES = 1 << 22;  // frames per track

struct pt_plan {
    int L = 0;                           // W + tau_max
    int G = 0;                           // lag groups: ceil(tau_max / R)
    int F = 1;                           // frames per tile
    int span = 0;                        // staged samples: (F - 1) * hop + W + G * R + 1
    int row = 0;                         // floats per row of d: tau_max + 1
};

static inline int pt_span(int F, int hop, int W, int G) { return (F - 1) * hop + W + G * PT_R + 1; }

// The plan of a (hop, tau_max, W) handle: the F within the LDS budget that keeps most of the 256 threads busy in the
// difference loop (ties: the larger tile, which stages a sample fewer times).  F = 1 always fits inside the envelope.
static inline pt_plan pt_make_plan(int hop, int tau_max, int W) {
    pt_plan p;
    p.L = W + tau_max;
    p.G = (tau_max + PT_R - 1) / PT_R;
    p.row = tau_max + 1;
    double best = -1.0;
    for (int F = 1; F <= PT_MAX_F; ++F) {
        if ((long)pt_span(F, hop, W, p.G) + (long)F * p.row > PT_MAX_LDS) break;
        const long items = (long)F * p.G;
        const long slots = (items + PT_THREADS - 1) / PT_THREADS * PT_THREADS;
        const double score = (double)items / (double)slots;
        if (score >= best) {
            best = score;
            p.F = F;
        }
    }
    p.span = pt_span(p.F, hop, W, p.G);
    return p;
}
