// pk_stoi.h -- definition, layout and summation orders of short-time objective intelligibility (stoi.hip).
// STOI: Taal, Hendriks, Heusdens, Jensen 2011; ESTOI: Jensen, Taal 2016.  The restatement below is this project's own (it is
// NOT pystoi and NOT the MATLAB code: tests/stoi_ref.py restates it in float64 numpy; change one, change the other).
//
// Both signals are at STOI_FS = 10 kHz and of the same length L.  w = numpy.hanning(258)[1:-1] (256 points, float64 on the
// host, rounded once to float32).  EPS = 2^-52.
//   frames:   the frames of L samples start at 0, 128, 256, ... strictly below L - 256: F(L) = 0 for L <= 256, else
//             (L - 257) / 128 + 1 (integer division).  The same rule both times frames are taken.
//   1 mask:   ss_i = sum_n (w_n x_i[n])^2 of the CLEAN signal in float32, in THE ORDER: lane l of a wave adds n = l, l + 64,
//             l + 128, l + 192 ascending to 0 with fused multiply-adds of the rounded product w_n x_n, then for h = 32, 16, ...,
//             1 every lane adds the value of lane l ^ h.  e_i = 20 log10(sqrt((double)ss_i) + EPS) in float64; e_max is that
//             of the largest ss (the maximum is exact in any order).  Frame i is kept iff e_max - 40 - e_i < 0.  K kept
//             frames, their indices ascending in a list (an exclusive scan of the flags).
//   2 rebuild: sample n of a rebuilt signal, n in [0, (K - 1) 128 + 256) (none for K = 0), c = n / 128, r = n % 128:
//             v = 0; if c >= 1: v = w[r + 128] x[128 idx[c - 1] + r + 128]; if c < K: v = v + w[r] x[128 idx[c] + r]
//             (float32; the earlier frame first).  Clean and degraded alike, through the clean signal's list.  The rebuilt
//             signal has K - 1 frames by the rule above (0 for K <= 1).
//   3 bands:  a frame of a rebuilt signal times w, zero-padded to 512, transformed by the plan of pk_rfft.h (n = 512, stride
//             128, a 512-float window of w followed by 256 zeros; the source is zero-padded so that a frame's 512 reads stay
//             inside it).  Band j = 0 ... 14: s = 0; for k = lo_j ... hi_j - 1 ascending: s = s + (re_k re_k + im_k im_k), every
//             operation rounded to float32 (no fused multiply-add); the band is sqrtf(s) (correctly rounded).  lo / hi: the bins
//             nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid k * 10000 / 512, computed in float64 on the host (stoi_edges).
//   4 segments (float64 from the float32 bands, every operation a separate IEEE float64 operation, no fused multiply-add;
//             sums over n or j ascending from 0.0): segment m is the 15 x 30 block of frames [m, m + 30), S = (K - 1) - 29.
//             STOI, per band row:  a = ||x|| / (||y|| + EPS);  y'_n = min(a y_n, x_n (1 + 10^(15/20)));  mean = (sum) / 30;
//                     xh_n = (x_n - mean_x) / (||x - mean_x|| + EPS), yh likewise from y';  c_j = sum_n xh_n yh_n;
//                     the segment's value is sum_j c_j.
//             ESTOI:  rows normalised as above (mean, then norm + EPS; no clipping), then every column the same way (mean over
//                     the 15 bands); c_n = sum_j of the products of column n; the segment's value is sum_n c_n.
//             THE ORDER over segments: one workgroup of STOI_RED_THREADS items per utterance; item t adds the values of segments
//             t, t + STOI_RED_THREADS, ... ascending to a_t = 0.0; then for h = STOI_RED_THREADS / 2, / 4, ..., 1: a_t = a_t +
//             a_(t + h) for t < h.  d = a_0 / (15 S) (STOI) or a_0 / (30 S) (ESTOI).  S <= 0: d = NaN with segments = 0 (that
//             is documented, and is not pystoi's 1e-5).
// No atomics anywhere.  Nothing of an utterance's computation depends on the batch around it: the same bits alone, in any
// batch and at any position.
//
// k_stoi_energy:   one wave per frame of the clean signal.
// k_stoi_mask:     one workgroup per utterance: the maximum, the flags, the scan in chunks of STOI_THREADS with a carry.
// k_stoi_rebuild:  one work item per sample of an utterance's region of the padded buffers; writes the zeros behind the
//                  rebuilt signal and the row map of the transform (row m of an utterance is transformed iff m < K - 1).
//                  An utterance's region has (F + 3) 128 floats: the last transformed frame is K - 2 <= F - 2 (F - 1 where
//                  pk_stoi_bands transforms a given signal) and ends at (F - 1) 128 + 512.  The kept counts stay on the
//                  device: every buffer is sized by F.
// k_stoi_bands:    one work item per (frame, band).
// k_stoi_segments: one wave per run of STOI_RUN = 4 consecutive segments of one utterance: the run's 33 frames x 15 bands of
//                  both signals (3 960 bytes) are staged once in LDS and every value of a segment is read from there; lane
//                  16 s + j owns band row j of segment s (its 30 values in sequence), for ESTOI lane 32 s' + n then owns column
//                  n of a segment (two steps of two segments).
// k_stoi_reduce:   THE ORDER over segments.
#pragma once
#include <cmath>
#include <cstdint>

constexpr int STOI_FS = 10000;
constexpr int STOI_FRAME = 256;
constexpr int STOI_HOP = 128;
constexpr int STOI_NFFT = 512;
constexpr int STOI_BANDS = 15;            // J
constexpr int STOI_SEG = 30;              // N
constexpr int STOI_THREADS = 256;
constexpr int STOI_RUN = 4;               // segments per wave of k_stoi_segments
constexpr int STOI_SEG_WAVES = 4;         // waves per workgroup of k_stoi_segments
constexpr int STOI_RED_THREADS = 256;
constexpr int STOI_MAX_BATCH = 65535;
constexpr long STOI_MAX_SAMPLES = 1L << 30;   // per utterance
constexpr double STOI_EPS = 2.220446049250313e-16;   // 2^-52
constexpr double STOI_RANGE_DB = 40.0;
constexpr double STOI_CLIP = 6.623413251903491;      // 1 + 10^(15 / 20)

static inline long stoi_frames(long L) { return L <= STOI_FRAME ? 0 : (L - STOI_FRAME - 1) / STOI_HOP + 1; }

// lo[j], hi[j]: bins [lo, hi) of band j
static inline void stoi_edges(int* lo, int* hi) {
    for (int j = 0; j < STOI_BANDS; ++j) {
        const double cf = 150.0 * std::pow(2.0, (double)j / 3.0);
        const double fl = cf * std::pow(2.0, -1.0 / 6.0), fh = cf * std::pow(2.0, 1.0 / 6.0);
        int bl = 0, bh = 0;
        double dl = 1e300, dh = 1e300;
        for (int k = 0; k <= STOI_NFFT / 2; ++k) {                 // the first of equally near bins, as numpy.argmin
            const double f = (double)k * STOI_FS / STOI_NFFT;
            if ((f - fl) * (f - fl) < dl) dl = (f - fl) * (f - fl), bl = k;
            if ((f - fh) * (f - fh) < dh) dh = (f - fh) * (f - fh), bh = k;
        }
        lo[j] = bl;
        hi[j] = bh;
    }
}
