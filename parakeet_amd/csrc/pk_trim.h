// pk_trim.h -- geometry, accumulation order and envelope of the silence-trimming kernels (trim.hip).
//
// Frame power.  Frame i of an utterance of N samples covers x~[i * hop - pad + j], j < Lf (pad = Lf / 2 when centred, else
// 0); x~ continues the utterance by reflection (x~[-m] = x[m], x~[N - 1 + m] = x[N - 1 - m]) or by zeros and is never the
// packed buffer's neighbour.  A tile is T consecutive frames of one utterance; its (T - 1) * hop + Lf samples are staged
// once in LDS and one wave owns a frame at a time.
//
// THE ORDER (the error bound of tests/trim_ref.py and DESIGN 4.5f is derived from these three lines):
//   s_l = fma(x~_j, x~_j, s_l) over j = l, l + 64, l + 128, ... < Lf ascending, from s_l = +0, for each lane l = 0 ... 63;
//   t   = the butterfly s_l + s_(l ^ 32), then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (IEEE addition commutes: every lane holds the same t);
//   P   = t / (float)Lf, one correctly rounded division (the square root of that, correctly rounded, when rms is asked for).
// j counts from the frame's own first sample, so the order involves neither the tile, nor the frame's position in it, nor
// the batch: a frame's P is the same bits wherever it is computed, centred or not.
// A term passes through at most ceil(Lf / 64) FMA roundings, six additions and the division; the terms are non-negative, so
// the error is relative: (ceil(Lf / 64) + 7) u.
#pragma once
#include <cstdint>

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_FRAME = 16384;      // Lf, and the VAD window w
constexpr int TR_MAX_TILE = 64;          // frames per tile
constexpr int TR_LDS_SMALL = 8192;       // floats of LDS per workgroup when a frame fits (32 KiB: four workgroups per CU) ...
constexpr int TR_LDS_LARGE = 16384;      // ... and when only the longest frames do not (64 KiB)
constexpr int TR_SCAN_CHUNK = 256;       // windows per step of the mask kernel (one per thread)
constexpr int TR_MAX_AVG = 64;           // W: moving-average width
constexpr int TR_MAX_SILENCE = 64;       // S: the dilation's structuring element has S + 1 ones
constexpr int TR_HALO = 32;              // the mask a chunk's dilation reads on either side: (S + 1) / 2 <= 32, and the flags
                                         // the mask's count reads beyond that: W / 2 <= 32
constexpr int TR_GATHER_WINDOWS = 16;    // windows per workgroup of the gather
constexpr int TR_NORM_TILE = 16384;      // samples per workgroup of the peak kernels

enum { TR_PAD_NONE = 0, TR_PAD_REFLECT = 1, TR_PAD_CONSTANT = 2 };

// frames of N samples: 1 + (N + 2 pad - Lf) / hop, none when the padded utterance is shorter than a frame
static inline long tr_num_frames(long N, int Lf, int hop, int mode) {
    const long padded = N + (mode == TR_PAD_NONE ? 0 : 2 * (long)(Lf / 2));
    return padded < Lf ? 0 : 1 + (padded - Lf) / hop;
}

// frames per tile: as many as the LDS budget holds, at most TR_MAX_TILE
static inline int tr_tile_frames(int Lf, int hop) {
    const int budget = Lf <= TR_LDS_SMALL ? TR_LDS_SMALL : TR_LDS_LARGE;
    const int T = (budget - Lf) / hop + 1;
    return T < 1 ? 1 : (T > TR_MAX_TILE ? TR_MAX_TILE : T);
}
