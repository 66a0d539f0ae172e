// pk_pvoc.h -- definition and plan of the phase vocoder (pvoc.hip): a spectrogram re-timed by a rate, what
// librosa 0.8's phase_vocoder(D, rate, hop_length) computes, restated WITHOUT any transcendental function.  It is this project's
// own restatement (librosa is not a dependency and nobody has compared the two outputs); tests/pvoc_ref.py restates everything
// below in float64 numpy; change one, change the other.
//
// WHY NO ANGLE.  librosa keeps phase_acc, emits mag * exp(i phase_acc) and advances phase_acc by angle(D[k+1]) - angle(D[k]),
// with the expected advance subtracted, the rest wrapped to +-pi and the expected advance added back.  Modulo 2 pi the
// subtraction, the wrap and the addition cancel, so exp(i phase_acc) is a running product of unit phasors and hop_length has
// no effect on the result.
//
// DEFINITION.  D: F >= 1 frames of n_bin complex float32 values, widened to float64; every bin on its own.  Every operation
// below is a separate IEEE float64 operation (no fused multiply-add); sqrt and / are the correctly rounded ones.
//     m(z)   = sqrt(re * re + im * im)                                    (two products, one sum, one root; not hypot)
//     u(z)   = (re / m(z), im / m(z)) if m(z) > 0 else (1, 0)             (numpy's angle(0) == 0)
//     T      = ceil((double)F / rate)                                     (= len(numpy.arange(0, F, rate)))
//     step_t = (double)t * rate ;  k_t = floor(step_t) ;  a_t = step_t - (double)k_t             for t = 0 ... T - 1
//     D[k] with k >= F reads as 0 + 0i  (so m = 0, u = (1, 0))
//     m0 = m(D[k_t]), m1 = m(D[k_t + 1]);  mag_t = (1.0 - a_t) * m0 + a_t * m1                   (two products, then the sum)
//     p_0    = u(D[0])
//     out_t  = ((float)(mag_t * p_t.re), (float)(mag_t * p_t.im))         (one float32 rounding each)
//     then, with (a, b) = u(D[k_t]) and (c, d) = u(D[k_t + 1]):
//         w    = (c * a + d * b,  d * a - c * b)                          (u(D[k_t + 1]) times the conjugate of u(D[k_t]))
//         q    = (p.re * w.re - p.im * w.im,  p.re * w.im + p.im * w.re)
//         mq   = sqrt(q.re * q.re + q.im * q.im)
//         p_(t+1) = (q.re / mq, q.im / mq)
// Float64 subnormals are kept.  A spectrum value so small that re * re + im * im is 0 counts as zero (m = 0, u = (1, 0)).
//
// THE PLAN.  k_pvoc: one lane per (utterance, bin), PVOC_THREADS = 64 bins of one utterance per workgroup, every lane walking
// its T steps in order with p in registers.  The lanes of a wave read neighbouring bins of the same two rows and write
// neighbouring bins of one row (coalesced in the packed re | im layout).  The loads of PVOC_AHEAD steps are issued before the
// chain of those steps (their addresses depend on t alone), unconditionally from a row index clamped into the utterance; a
// row at or beyond F is selected to zero afterwards.  No reduction, no atomics, no LDS: an utterance's bytes are the same
// alone, in any batch and at any position.
#pragma once
#include <cmath>
#include <cstdint>

constexpr int PVOC_THREADS = 64;           // bins per workgroup (one wave)
constexpr int PVOC_AHEAD = 4;              // steps whose rows are loaded ahead of their chain
constexpr int PVOC_MAX_BATCH = 65535;
constexpr int64_t PVOC_MAX_FRAMES = (int64_t)1 << 31;   // T must stay below

// T of the definition, as a double (the caller checks the range before converting); F >= 1, rate finite and > 0
static inline double pvoc_num_frames(int64_t F, double rate) { return std::ceil((double)F / rate); }
