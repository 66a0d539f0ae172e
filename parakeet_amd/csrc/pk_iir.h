// pk_iir.h -- definition, plan and summation orders of the recursive filters and of gated loudness (iir.hip).
// The loudness measure is this project's own restatement of ITU-R BS.1770-4 for ONE channel (it is NOT pyloudnorm and NOT
// libebur128; blocks lie on a 100 ms SAMPLE grid, which needs sr % 10 == 0).  tests/iir_ref.py restates everything below in
// float64 numpy scalars; change one, change the other.
//
// FILTER.  S second-order sections, 1 <= S <= IIR_MAX_SECTIONS, each scipy's row (b0, b1, b2, a0, a1, a2) in float64 with
// a0 == 1.  Input float32, widened to float64.  Transposed direct form II, every operation a separate IEEE float64 operation
// (no fused multiply-add); sections ascending, v the section's input and o its output:
//     o  = b0 * v + z0
//     z0 = (b1 * v - a1 * o) + z1
//     z1 = b2 * v - a2 * o
//     v  = o
// The state starts at zero.  A filtered sample is rounded once to float32 where a float32 result is asked for.  Float64
// subnormals are kept (a decaying state walks through them after digital silence).
//
// THE PLAN.  Chunks of IIR_CHUNK = 256 samples start at the utterance's sample 0.  n = 2 S, state order z0, z1 of section 0,
// then of section 1, ...
//   P        (n x n): column j is the end state of one chunk of ZERO input (the float32 0 widened, run through the recurrence
//            as it stands) from the unit state e_j.  Computed on the device by the same recurrence code when the handle is
//            created (k_iir_transition: lane j runs column j).
//   local    for every FULL chunk c (c < L / 256): q_c = the end state of the chunk run from the zero state.
//   carry    s_0 = 0; for every full chunk c:  s_(c+1)[i] = ((...(0.0 + P[i][0] s_c[0]) + P[i][1] s_c[1]) + ...) + q_c[i],
//            j ascending, every product and every sum rounded.
//   apply    every chunk (the last may be partial) is re-run from s_c and its outputs are produced.
// This is not the bits of a sample-by-sample run over the whole signal (P s + q rounds differently); it is deterministic and
// independent of the batch: the same bits alone, in any batch and at any position.  No atomics anywhere.
//
// LOUDNESS of an utterance of L samples at rate sr (sr % 10 == 0, 8 000 <= sr <= 192 000; h = sr / 10 >= IIR_CHUNK), through
// a filter handle that holds the weighting (audio.k_weighting(sr) for BS.1770).  z = the filtered sample in float64, NOT
// rounded to float32.
//   pieces   chunk c keeps two accumulators, for hop segment g0 = (256 c) / h and for g0 + 1 (a chunk touches no third one).
//            Each starts at 0.0 and adds z * z sample by sample, ascending (the product rounded, then the sum); sample t of the
//            chunk belongs to g0 iff 256 c + t < (g0 + 1) h.  The same pass keeps max|x| of the chunk (exact in any order).
//   segments G = L / h.  seg[g], g < G = the sum from 0.0 of the pieces for g of the chunks c = (g h) / 256 ... ((g + 1) h - 1)
//            / 256, ascending.  Samples at or beyond G h are filtered but not counted.
//   blocks   J = max(0, G - 3);  p_j = (((seg[j] + seg[j+1]) + seg[j+2]) + seg[j+3]) / (double)(4 h)   (400 ms, 75 % overlap).
//   gates    in the POWER domain (the device evaluates no logarithm).  ABS = LOUD_ABS, the float64 of 10.0 ** -6.9309
//            (-70 LUFS).  Gate 1 keeps j iff p_j > ABS: count n1, sum sum1.  REL = 0.1 * (sum1 / (double)n1)  (-10 LU).
//            Gate 2 keeps j iff gate 1 keeps it and p_j > REL: count n2, sum sum2.  mean = sum2 / (double)n2.
//            n1 == 0 (which covers J == 0): mean = 0, n2 = 0, REL = 0.
//            THE ORDER over blocks, the same for both gates: one workgroup of LOUD_THREADS = 256 items per utterance; item t
//            adds the kept p_j for j = t, t + 256, ... ascending to a_t = 0.0; then for h' = 128, 64, ..., 1: a_t = a_t +
//            a_(t + h') for t < h'.  The sum is a_0.
//   peak     max|x| over all L samples (the sample peak; 0 for L == 0).
//   host     LUFS = -0.691 + 10 log10(mean) in float64, -inf when n2 == 0.
//
// k_iir_transition:  one wave; lane j < n runs column j of P.
// k_iir_local:       one wave of IIR_LANES = 64 chunks of one utterance, one lane per chunk.  The wave's chunks pass through LDS
//                    in four stages of 64 samples: row r of the tile is 64 consecutive samples of chunk r (a coalesced 256-byte
//                    load), rows IIR_TILE_LD = 65 floats apart so that the 64 lanes walking their own rows read 64 banks.
// k_iir_carry:       one wave per utterance; lane i < n keeps row i of P in registers, the state is broadcast by lane reads.
// k_iir_apply:       the layout of k_iir_local; filter mode writes the outputs back through the tile (coalesced stores),
//                    loudness mode stores the chunk's two pieces and its peak.
// k_loud_segments:   one work item per hop segment.
// k_loud_gate:       THE ORDER over blocks; one workgroup per utterance.
// k_gain:            y = x * g (one float32 rounding), g per utterance.
#pragma once
#include <cstdint>

constexpr int IIR_CHUNK = 256;
constexpr int IIR_LANES = 64;              // chunks per wave of the local / apply kernels
constexpr int IIR_STAGE = 64;              // samples of every chunk in LDS at a time
constexpr int IIR_TILE_LD = IIR_STAGE + 1; // floats between the rows of the tile
constexpr int IIR_MAX_SECTIONS = 8;
constexpr int IIR_MAX_BATCH = 65535;
constexpr long IIR_MAX_SAMPLES = 1L << 30; // per utterance
constexpr int IIR_CARRY_AHEAD = 8;         // chunks of a stretch of the carry kernel: their q loaded ahead of the chain, their s stored behind it
constexpr int LOUD_THREADS = 256;
constexpr int LOUD_SR_MIN = 8000, LOUD_SR_MAX = 192000;
constexpr double LOUD_ABS = 1.1724653045822956e-07;   // 10.0 ** -6.9309

static inline long iir_chunks(long L) { return (L + IIR_CHUNK - 1) / IIR_CHUNK; }
static inline long iir_full_chunks(long L) { return L / IIR_CHUNK; }
