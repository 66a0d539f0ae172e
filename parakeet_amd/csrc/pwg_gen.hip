// pwg_gen.hip -- the shape-generic Parallel WaveGAN path: any residual / gate / skip / aux channel count and any odd
// kernel size inside the envelope of pwg_gen_check.  pwg.hip's pk_pwg_* entry points call it for every configuration its
// tuned kernels (in/out 1, kernel 3, residual 64, gate 128, skip 64, aux 80) cannot take, and for that one as well under
// the handle option "generic_kernel".
//
// Reference: parakeet/models/parallel_wavegan/parallel_wavegan.py -- ResidualBlock.forward :284-315,
// PWGGenerator.forward :445-472, inference :498-520.
//
// Data flow.  The conditioning is pwg.hip's: conv_in as an implicit GEMM, then every layer's conv1x1_aux
// at FRAME rate as one exact-fp32 GEMM [frames x AUX] x [AUX x layers*G] (AUX zero-padded to a multiple of 16 inside
// the engine), and the upsampler as the composite phase filter table (9 edge classes x hop phases x 5 frames) applied
// per sample inside the layer kernel.  The residual stream x (R channels) and the skip sum (SK channels) are fp32 in a
// blocked timeline: block k holds samples [32k, 32k + 32) of all channels, addr(ch, t) = (t >> 5) * CH * 32 + ch * 32 +
// (t & 31).  Utterances start on 64-sample boundaries and are separated by zero gaps of at least the widest tap reach
// ((kernel - 1) / 2 * max dilation), so a dilated tap that leaves its utterance reads zeros -- the reference's zero
// padding -- and a ragged batch costs nothing extra.  Positions past an utterance's end inside its last tile are
// written as zeros by a select, never by a multiplication (0 * Inf).
//
// k_pwg_block_gen, one residual block over a tile of 64 samples (4 waves):
//   phase 1  per (gate pair block of 32 + 32 rows, 32-sample half): the dilated conv K = kernel * R, N = 32 samples for
//            the tanh rows and the sigmoid rows, + bias + upsampled conditioning, tanh(a) * sigmoid(b) in registers; the
//            gated z [64 samples][G/2] goes to LDS;
//   phase 2  per (32 output rows of [conv1x1_out ; conv1x1_skip], 32-sample half): ONE contraction (R + SK) x G/2 over z,
//            then x' = (x + out) * sqrt(1/2) and skip (+)= s.
// Weights are pre-packed MFMA fragments streamed from L2 (at 128 / 256 / 128 a layer is 650 KB fp32 and does not fit
// LDS).  Math: F32 exact on v_mfma_f32_32x32x2_f32; F16X3 / BF16X3 as a_hi*b_hi + a_lo*b_hi + a_hi*b_lo on
// v_mfma_f32_32x32x16_{f16,bf16}, operands block scaled (pk_split.h): x by a measured power of two per 32-sample half
// tile (the maxima of the 32-sample blocks its taps touch, written by the producer of x), z by 2^14, fp16 weights by
// one power of two per tensor.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pk_gemm.h"
#include "pk_mfma.h"
#include "pk_split.h"
#include "pwg_gen.h"

namespace {

typedef __bf16 gbf16x8 __attribute__((ext_vector_type(8)));

constexpr int GT = 64;           // samples per workgroup tile
constexpr int GUPW = 5;          // frames of the composite upsampler (pwg.hip: UPW)
constexpr int GUPW_PAD = 8;      // table row stride (pwg.hip: UPW_PAD)
constexpr int G_EDGE_CLASS = 9;
constexpr int G_MAX_UP_TAPS = 17;
constexpr int G_P_LEAD = 8;      // margin rows around the frame-rate projection
constexpr float G_SQRT_HALF = 0.70710678118654752440f;

enum { GM_F32 = 0, GM_F16X3 = 1, GM_BF16X3 = 2 };

template <int MODE> struct GSplit { typedef f16x8 vec; typedef _Float16 elem; };
template <> struct GSplit<GM_BF16X3> { typedef gbf16x8 vec; typedef __bf16 elem; };
__device__ __forceinline__ f32x16 g_mfma16(gbf16x8 a, gbf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 g_mfma16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// hi = round(v), lo = round(v - hi) (round to nearest even in both formats)
template <class V, class E>
__device__ __forceinline__ void g_split8(const float (&v)[8], V& hi, V& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = (E)v[e];
        lo[e] = (E)(v[e] - (float)hi[e]);
    }
}

struct GenTabs {
    const int* tile_t0;    // [tiles] timeline offset of the tile (multiple of 64)
    const int* tile_utt;   // [tiles] utterance
    const int* utt_toff;   // [B] timeline offset of sample 0
    const int* utt_S;      // [B] samples
    const int* utt_F;      // [B] frames
    const int* utt_row0;   // [B] P row of frame 0
    const int* utt_off;    // [B] offset in the packed noise / wav
};

// x0 = first_conv(noise) (Conv1D 1 -> R, k = 1), zeros past the utterance; max|x0| per 32-sample block
__global__ __launch_bounds__(256) void k_pwg_first_gen(const float* __restrict__ noise, const float* __restrict__ w,
                                                       const float* __restrict__ bias, GenTabs tb, int R,
                                                       float* __restrict__ x, unsigned* __restrict__ xe) {
    __shared__ unsigned xm[2];
    const int tile = blockIdx.x;
    const int t0 = tb.tile_t0[tile], b = tb.tile_utt[tile];
    const int j = threadIdx.x & (GT - 1);
    const int s = t0 - tb.utt_toff[b] + j;
    const bool valid = s < tb.utt_S[b];
    if (threadIdx.x < 2) xm[threadIdx.x] = 0u;
    __syncthreads();
    const float nz = valid ? noise[(long)tb.utt_off[b] + s] : 0.f;
    float* xb = x + (long)((t0 + j) >> 5) * R * 32 + (j & 31);
    float m = 0.f;
    for (int ch = threadIdx.x >> 6; ch < R; ch += 4) {
        const float y = valid ? fmaf(w[ch], nz, bias[ch]) : 0.f;
        xb[ch * 32] = y;
        m = fmaxf(m, fabsf(y));
    }
    atomicMax(&xm[j >> 5], __float_as_uint(m));
    __syncthreads();
    if (threadIdx.x < 2) xe[(t0 >> 5) + threadIdx.x] = xm[threadIdx.x];
}

// ZScore + padded row timeline for conv_in's implicit GEMM (pwg.hip: k_pwg_convin_prep), AUX columns zero-padded to AUXP
__global__ void k_pwg_convin_prep_gen(const float* __restrict__ mel, const float* __restrict__ mu,
                                      const float* __restrict__ sigma, int use_norm, const int* __restrict__ prow_src,
                                      int rows, int aux, int auxp, float* __restrict__ out) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < auxp; c += blockDim.x) {
        float v = 0.f;
        if (r < rows && c < aux) {
            v = mel[(long)prow_src[r] * aux + c];
            if (use_norm) v = (v - mu[c]) / sigma[c];
        }
        out[(long)r * auxp + c] = v;
    }
}

struct GenLayer {
    const float* xin;
    float* xout;
    float* skip;
    const unsigned* xe_in;   // max|x| per 32-sample block of xin (fp32 bits)
    unsigned* xe_out;
    const float* w1f;        // F32:   [2*GH/32 row blocks][K*R/2 k-steps][64 lanes]
    const float* w2f;        //        [OP/32][GH/2][64]
    const void* w1h;         // split: [2*GH/32][K*R/16][hi, lo][64][8]
    const void* w2h;         //        [OP/32][GH/16][hi, lo][64][8]
    const float* bias;       // [G conv | R out | SK skip]
    const float* P;          // frame-rate conditioning, this layer's G columns; row r = P row r
    const float* uptab;      // [9 classes][hop phases][8]
    GenTabs tb;
    int ldp, hop;
    int R, G, SK, K, dil;
    int GH, OP;              // G/2 and R + SK rounded up to 32
    int first;               // layer 0: skip = s, not skip += s
    int k1, k2;              // split: weight exponents (fragments hold w * 2^k)
};

// One residual block over 64-sample tiles (see the header).  ZMAX: LDS row stride of z (>= GH + 1).
template <int MODE, int ZMAX>
__global__ __launch_bounds__(256) void k_pwg_block_gen(GenLayer a) {
    __shared__ float zl[GT * ZMAX];   // z [sample][gated channel]
    __shared__ unsigned xm[2];
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 31, hi = lane >> 5;
    const int t0 = a.tb.tile_t0[tile], b = a.tb.tile_utt[tile];
    const int toff = a.tb.utt_toff[b], S = a.tb.utt_S[b], F = a.tb.utt_F[b], row0 = a.tb.utt_row0[b];
    const int cK = (a.K - 1) / 2;
    const int R = a.R, GH = a.GH, Gh = a.G / 2;
    if (threadIdx.x < 2) xm[threadIdx.x] = 0u;
    // ---- phase 1: dilated conv + conditioning + gate
    const int npair = GH / 32;
    for (int u = wave; u < 2 * npair; u += 4) {
        const int jb = u >> 1, st = u & 1;
        const int ts = t0 + 32 * st;
        const int s = ts - toff + n;
        const bool valid = s < S;
        f32x16 aa = {}, ab = {};
        int kx = 0;
        if constexpr (MODE != GM_F32) {   // the x operand's scale: max over the blocks this half tile's taps touch
            unsigned m = 0u;
            for (int tap = 0; tap < a.K; ++tap) {
                const int p = ts + (tap - cK) * a.dil;
                m = max(m, a.xe_in[p >> 5]);
                m = max(m, a.xe_in[(p + 31) >> 5]);
            }
            kx = blk_scale_exp(m);
        }
        if constexpr (MODE == GM_F32) {
            const int ks1 = a.K * R / 2;
            const float* wa = a.w1f + (size_t)jb * ks1 * 64 + lane;
            const float* wb = a.w1f + (size_t)(npair + jb) * ks1 * 64 + lane;
            int ks = 0;
            for (int tap = 0; tap < a.K; ++tap) {
                const int p = ts + n + (tap - cK) * a.dil;
                const float* xp = a.xin + (long)(p >> 5) * R * 32 + (p & 31);
                for (int ci = hi; ci < R; ci += 2, ++ks) {
                    const float xv = xp[ci * 32];
                    aa = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[(size_t)ks * 64], xv, aa, 0, 0, 0);
                    ab = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[(size_t)ks * 64], xv, ab, 0, 0, 0);
                }
            }
        } else {
            typedef typename GSplit<MODE>::vec V;
            typedef typename GSplit<MODE>::elem E;
            const int ks1 = a.K * R / 16;
            const V* wa = reinterpret_cast<const V*>(a.w1h) + (size_t)jb * ks1 * 128 + lane;
            const V* wb = reinterpret_cast<const V*>(a.w1h) + (size_t)(npair + jb) * ks1 * 128 + lane;
            const float xs = pow2f(kx);
            int ks = 0;
            for (int tap = 0; tap < a.K; ++tap) {
                const int p = ts + n + (tap - cK) * a.dil;
                const float* xp = a.xin + (long)(p >> 5) * R * 32 + (p & 31);
                for (int c0 = 8 * hi; c0 < R; c0 += 16, ++ks) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = xp[(c0 + e) * 32] * xs;
                    V bh, bl;
                    g_split8<V, E>(v, bh, bl);
                    const V ah = wa[(size_t)ks * 128], al = wa[(size_t)ks * 128 + 64];
                    const V ch = wb[(size_t)ks * 128], cl = wb[(size_t)ks * 128 + 64];
                    aa = g_mfma16(ah, bh, aa);
                    aa = g_mfma16(al, bh, aa);
                    aa = g_mfma16(ah, bl, aa);
                    ab = g_mfma16(ch, bh, ab);
                    ab = g_mfma16(cl, bh, ab);
                    ab = g_mfma16(ch, bl, ab);
                }
            }
        }
        // conditioning: composite upsampler over 5 frames of this lane's sample (clamped into the utterance)
        const int sc = valid ? s : S - 1;
        const int f = sc / a.hop, ph = sc - f * a.hop;
        const int cls = min(f, 2) * 3 + min(F - 1 - f, 2);
        const float* twp = a.uptab + ((size_t)cls * a.hop + ph) * GUPW_PAD;
        float tw[GUPW];
#pragma unroll
        for (int j = 0; j < GUPW; ++j) tw[j] = twp[j];
        const float* pr = a.P + (long)(row0 + f - 2) * a.ldp;
        const float inv = MODE == GM_F32 ? 1.f : pow2f(-(a.k1 + kx));
        float* zrow = zl + (32 * st + n) * ZMAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = 32 * jb + mfma_row(r, hi);
            float z = 0.f;
            if (j < Gh) {
                float ca = 0.f, cb = 0.f;
#pragma unroll
                for (int q = 0; q < GUPW; ++q) {
                    ca = fmaf(tw[q], pr[(long)q * a.ldp + j], ca);
                    cb = fmaf(tw[q], pr[(long)q * a.ldp + Gh + j], cb);
                }
                const float va = aa[r] * inv + a.bias[j] + ca;
                const float vb = ab[r] * inv + a.bias[Gh + j] + cb;
                z = tanhf(va) * (1.f / (1.f + expf(-vb)));
            }
            zrow[j] = valid ? z : 0.f;
        }
    }
    __syncthreads();
    // ---- phase 2: [conv1x1_out ; conv1x1_skip] over z, residual and skip epilogue
    const int nob = a.OP / 32;
    for (int u = wave; u < 2 * nob; u += 4) {
        const int ob = u >> 1, st = u & 1;
        const int ts = t0 + 32 * st;
        const bool valid = ts - toff + n < S;
        const float* zr = zl + (32 * st + n) * ZMAX;
        f32x16 acc = {};
        float inv = 1.f;
        if constexpr (MODE == GM_F32) {
            const int ks2 = GH / 2;
            const float* w = a.w2f + (size_t)ob * ks2 * 64 + lane;
            for (int ks = 0; ks < ks2; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(size_t)ks * 64], zr[2 * ks + hi], acc, 0, 0, 0);
        } else {
            typedef typename GSplit<MODE>::vec V;
            typedef typename GSplit<MODE>::elem E;
            const int ks2 = GH / 16;
            const V* w = reinterpret_cast<const V*>(a.w2h) + (size_t)ob * ks2 * 128 + lane;
            for (int ks = 0; ks < ks2; ++ks) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = zr[16 * ks + 8 * hi + e] * PK_UNIT_SCALE;
                V bh, bl;
                g_split8<V, E>(v, bh, bl);
                const V ah = w[(size_t)ks * 128], al = w[(size_t)ks * 128 + 64];
                acc = g_mfma16(ah, bh, acc);
                acc = g_mfma16(al, bh, acc);
                acc = g_mfma16(ah, bl, acc);
            }
            inv = pow2f(-(PK_UNIT_EXP + a.k2));
        }
        const long blk = ts >> 5;
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * ob + mfma_row(r, hi);
            if (o < R) {
                const long i = blk * R * 32 + o * 32 + n;
                const float v = acc[r] * inv + a.bias[a.G + o];
                const float y = valid ? (a.xin[i] + v) * G_SQRT_HALF : 0.f;
                a.xout[i] = y;
                m = fmaxf(m, fabsf(y));
            } else if (o < R + a.SK) {
                const long i = blk * a.SK * 32 + (o - R) * 32 + n;
                const float v = acc[r] * inv + a.bias[a.G + o];
                const float y = a.first ? v : a.skip[i] + v;
                a.skip[i] = valid ? y : 0.f;
            }
        }
        atomicMax(&xm[st], __float_as_uint(m));
    }
    __syncthreads();
    if (threadIdx.x < 2) a.xe_out[(t0 >> 5) + threadIdx.x] = xm[threadIdx.x];
}

struct GenLast {
    const float* skip;
    const float* w1f;   // [SKP/32][SK/2][64]: last_conv_layers.1
    const float* b1;    // [SKP]
    const float* w2;    // [SKP]: last_conv_layers.3
    float b2;
    float scale;        // sqrt(1 / layers)
    GenTabs tb;
    int SK, SKP;
    float* wav;
};

// relu(skip * sqrt(1/layers)) -> 1x1 SK -> SK -> relu -> 1x1 SK -> 1, exact fp32 (v_mfma_f32_32x32x2_f32)
__global__ __launch_bounds__(256) void k_pwg_last_gen(GenLast a) {
    __shared__ float part[16][GT];   // [row block * 2 + lane half][sample]: SKP <= 256
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 31, hi = lane >> 5;
    const int t0 = a.tb.tile_t0[tile], b = a.tb.tile_utt[tile];
    const int nob = a.SKP / 32, ks2 = a.SK / 2;
    for (int u = wave; u < 2 * nob; u += 4) {
        const int ob = u >> 1, st = u & 1;
        const float* sp = a.skip + (long)((t0 >> 5) + st) * a.SK * 32 + n;
        const float* w = a.w1f + (size_t)ob * ks2 * 64 + lane;
        f32x16 acc = {};
        for (int ks = 0; ks < ks2; ++ks) {
            const float y = fmaxf(sp[(2 * ks + hi) * 32] * a.scale, 0.f);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(size_t)ks * 64], y, acc, 0, 0, 0);
        }
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * ob + mfma_row(r, hi);
            ps = fmaf(fmaxf(acc[r] + a.b1[o], 0.f), a.w2[o], ps);
        }
        part[2 * ob + hi][32 * st + n] = ps;
    }
    __syncthreads();
    if (threadIdx.x < GT) {
        const int s = t0 - a.tb.utt_toff[b] + threadIdx.x;
        if (s < a.tb.utt_S[b]) {
            float v = a.b2;
            for (int q = 0; q < 2 * nob; ++q) v += part[q][threadIdx.x];
            a.wav[(long)a.tb.utt_off[b] + s] = v;
        }
    }
}

// debug tap 0: layer 0's sample-rate conditioning conv1x1_aux(upsample(c)) for one utterance (pwg.hip: k_pwg_aux_debug)
__global__ void k_pwg_aux_debug_gen(const float* __restrict__ P, int ldp, const float* __restrict__ uptab, int row0,
                                    int n_frames, int hop, float* __restrict__ out) {
    const int f = blockIdx.x, co = blockIdx.y;
    const int cls = min(f, 2) * 3 + min(n_frames - 1 - f, 2);
    for (int phase = threadIdx.x; phase < hop; phase += blockDim.x) {
        const float* w = uptab + ((long)cls * hop + phase) * GUPW_PAD;
        float acc = 0.f;
        for (int jj = 0; jj < GUPW; ++jj) acc = fmaf(w[jj], P[(long)(row0 + f + jj - 2) * ldp + co], acc);
        out[(long)co * n_frames * hop + (long)f * hop + phase] = acc;
    }
}

}  // namespace

// ================================================================== host side
struct pwg_gen {
    pk_pwg_cfg cfg;
    int hop = 256, R = 64, G = 128, SK = 64, AUX = 80, AUXP = 80, K = 3, GH = 64, OP = 128, SKP = 64;
    int gap = 64;
    pk_dbuf d_first_w, d_first_b, d_convin, d_waux, d_uptab, d_bias;
    pk_dbuf d_w1f, d_w2f, d_w1h, d_w2h, d_w1b, d_w2b;   // per layer: fp32 / fp16-split / bf16-split fragments
    size_t n1f = 0, n2f = 0, n1h = 0, n2h = 0;           // elements per layer (floats / halves)
    std::vector<int> k1, k2;                             // fp16 weight exponents per layer
    pk_dbuf d_l1, d_l1b, d_l2;
    float l2_bias = 0.f;
    pk_dbuf ws_mel, ws_noise, ws_wav, ws_cin, ws_c0, ws_P, ws_x0, ws_x1, ws_skip, ws_xe0, ws_xe1, ws_tab, ws_dbg;
    std::vector<int> last_frames, last_toff, last_cuL;
    int last_ldp = 0, last_x_final = 0;
    long last_Ttot = 0;
};

int pwg_gen_check(const pk_pwg_cfg& c) {
    if (c.in_channels != 1 || c.out_channels != 1)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: in_channels and out_channels must be 1 (got %d, %d)", c.in_channels, c.out_channels);
    if (c.kernel_size < 1 || c.kernel_size > 9 || c.kernel_size % 2 == 0)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: kernel_size must be odd, 1 ... 9 (got %d)", c.kernel_size);
    if (c.residual_channels < 16 || c.residual_channels > 256 || c.residual_channels % 16)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: residual_channels must be a multiple of 16, 16 ... 256 (got %d)", c.residual_channels);
    if (c.skip_channels < 16 || c.skip_channels > 256 || c.skip_channels % 16)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: skip_channels must be a multiple of 16, 16 ... 256 (got %d)", c.skip_channels);
    if (c.gate_channels < 32 || c.gate_channels > 512 || c.gate_channels % 32)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: gate_channels must be even with gate_channels/2 a multiple of 16, 32 ... 512 (got %d)",
                c.gate_channels);
    if (c.aux_channels < 1 || c.aux_channels > 512)
        PK_FAIL(PK_EUNSUPPORTED, "PWGGenerator: aux_channels must be 1 ... 512 (got %d)", c.aux_channels);
    return PK_OK;
}

static std::vector<double> gen_upsample_sim(std::vector<double> x, const pk_pwg_cfg& c,
                                            const std::vector<std::vector<double>>& firs) {
    for (int i = 0; i < c.n_upsample; ++i) {
        const int s = c.upsample_scales[i];
        const long n = (long)x.size() * s;
        std::vector<double> y(n, 0.0);
        for (long t = 0; t < n; ++t) {
            double acc = 0.0;
            for (int j = 0; j <= 2 * s; ++j) {
                const long u = t + j - s;
                if (u >= 0 && u < n) acc += firs[i][j] * x[u / s];
            }
            y[t] = acc;
        }
        x.swap(y);
    }
    return x;
}

static inline uint16_t gen_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float gen_bf16_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// hi / lo parts of w; half: fp16 (round to nearest even), else bf16
static inline void gen_split(float w, bool half, uint16_t& hi, uint16_t& lo) {
    if (half) {
        const _Float16 h = (_Float16)w, l = (_Float16)(w - (float)h);
        memcpy(&hi, &h, 2);
        memcpy(&lo, &l, 2);
    } else {
        hi = gen_bf16_rne(w);
        lo = gen_bf16_rne(w - gen_bf16_f32(hi));
    }
}
// fragments of an [M rows][Kd] matrix (rows in blocks of 32, row map given by `rowv`) for the two MFMA shapes:
//   fp32 [blk][Kd/2][64]: lane (i, hi) of k-step ks holds W[row i][2 ks + hi]
//   split [blk][Kd/16][hi, lo][64][8]: element e of lane (i, hi) holds W[row i][16 ks + 8 hi + e]
template <class Fn>
static void gen_pack(int nblk, int Kd, Fn rowv, float* f32, uint16_t* hh, uint16_t* hb, int kh) {
    for (int blk = 0; blk < nblk; ++blk)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 31, hi = lane >> 5;
            for (int ks = 0; ks < Kd / 2; ++ks) f32[((size_t)blk * (Kd / 2) + ks) * 64 + lane] = rowv(32 * blk + i, 2 * ks + hi);
            for (int ks = 0; ks < Kd / 16; ++ks)
                for (int e = 0; e < 8; ++e) {
                    const float w = rowv(32 * blk + i, 16 * ks + 8 * hi + e);
                    const size_t o = ((((size_t)blk * (Kd / 16) + ks) * 2) * 64 + lane) * 8 + e;
                    uint16_t a, b;
                    gen_split(std::ldexp(w, kh), true, a, b);
                    hh[o] = a;
                    hh[o + 512] = b;
                    gen_split(w, false, a, b);
                    hb[o] = a;
                    hb[o + 512] = b;
                }
        }
}

int pwg_gen_finalize(pwg_gen** gp, pk_ctx* ctx, const pk_pwg_cfg& c, const pk_param_map& params, int hop) {
    PK_TRY(pwg_gen_check(c));
    if (!*gp) *gp = new pwg_gen();
    pwg_gen* g = *gp;
    g->cfg = c;
    g->hop = hop;
    const int R = g->R = c.residual_channels, G = g->G = c.gate_channels, SK = g->SK = c.skip_channels;
    const int AUX = g->AUX = c.aux_channels;
    const int AUXP = g->AUXP = (AUX + 15) / 16 * 16;
    const int K = g->K = c.kernel_size;
    const int GH = g->GH = (G / 2 + 31) / 32 * 32;
    const int OP = g->OP = (R + SK + 31) / 32 * 32;
    const int SKP = g->SKP = (SK + 31) / 32 * 32;
    const int lps = c.layers / c.stacks;
    const int reach = (K - 1) / 2 * (1 << (lps - 1));
    g->gap = std::max(GT, (reach + GT - 1) / GT * GT);
    std::vector<float> w, bb;
    PK_TRY(pk_get_weight(params, "first_conv", {R, 1, 1}, w));
    PK_TRY(pk_get_vector(params, "first_conv.bias", R, bb));
    PK_TRY(pk_upload(ctx, g->d_first_w, w.data(), R * sizeof(float)));
    PK_TRY(pk_upload(ctx, g->d_first_b, bb.data(), R * sizeof(float)));
    // conv_in -> implicit-GEMM weight [K = tap * AUXP + ci][N = AUXP], zero rows / columns for the padding
    const int kin = 2 * c.aux_context_window + 1;
    if (kin > PK_GEMM_MAX_TAPS) PK_FAIL(PK_EUNSUPPORTED, "PWG: aux_context_window %d too wide", c.aux_context_window);
    PK_TRY(pk_get_weight(params, "upsample_net.conv_in", {AUX, AUX, kin}, w));
    {
        std::vector<float> wp((size_t)AUXP * AUXP * kin, 0.f), kn, packed;
        for (int co = 0; co < AUX; ++co)
            for (int ci = 0; ci < AUX; ++ci)
                for (int t = 0; t < kin; ++t) wp[((size_t)co * AUXP + ci) * kin + t] = w[((size_t)co * AUX + ci) * kin + t];
        pk_conv_to_kn(wp.data(), AUXP, AUXP, kin, kn);
        pk_gemm_pack(kn.data(), AUXP * kin, AUXP, packed);
        PK_TRY(pk_upload(ctx, g->d_convin, packed.data(), packed.size() * sizeof(float)));
    }
    // composite upsampler table (pwg.hip's construction): class (a, b) = (min(frames before, 2), min(frames after, 2))
    {
        std::vector<std::vector<double>> firs(c.n_upsample);
        for (int i = 0; i < c.n_upsample; ++i) {
            const int taps = 2 * c.upsample_scales[i] + 1;
            if (taps > G_MAX_UP_TAPS) PK_FAIL(PK_EUNSUPPORTED, "upsample scale %d unsupported", c.upsample_scales[i]);
            PK_TRY(pk_get_weight(params, "upsample_net.upsample.up_layers." + std::to_string(2 * i + 1), {1, 1, 1, taps}, w));
            firs[i].assign(w.begin(), w.begin() + taps);
        }
        std::vector<float> tab((size_t)G_EDGE_CLASS * hop * GUPW_PAD, 0.f);
        for (int a = 0; a <= 2; ++a)
            for (int b = 0; b <= 2; ++b) {
                const int Lc = a + b + 1, fc = a, cls = a * 3 + b;
                for (int fi = 0; fi < Lc; ++fi) {
                    std::vector<double> imp(Lc, 0.0);
                    imp[fi] = 1.0;
                    const std::vector<double> y = gen_upsample_sim(imp, c, firs);
                    const int jj = fi - fc + 2;
                    for (int p = 0; p < hop; ++p) tab[((size_t)cls * hop + p) * GUPW_PAD + jj] = (float)y[(size_t)fc * hop + p];
                }
            }
        PK_TRY(pk_upload(ctx, g->d_uptab, tab.data(), tab.size() * sizeof(float)));
    }
    // residual blocks
    {
        const int L = c.layers;
        const int nb1 = 2 * GH / 32, nb2 = OP / 32;
        g->n1f = (size_t)nb1 * (K * R / 2) * 64;
        g->n2f = (size_t)nb2 * (GH / 2) * 64;
        g->n1h = (size_t)nb1 * (K * R / 16) * 2 * 64 * 8;
        g->n2h = (size_t)nb2 * (GH / 16) * 2 * 64 * 8;
        std::vector<float> W1f(g->n1f * L), W2f(g->n2f * L), B((size_t)(G + R + SK) * L);
        std::vector<uint16_t> W1h(g->n1h * L), W1b(g->n1h * L), W2h(g->n2h * L), W2b(g->n2h * L);
        std::vector<float> Wa((size_t)AUXP * L * G, 0.f);   // [K = aux ch][N = layer * G + co]
        std::vector<float> wc, wa, wo, ws, bc, bo, bs;
        g->k1.assign(L, 0);
        g->k2.assign(L, 0);
        for (int l = 0; l < L; ++l) {
            const std::string p = "conv_layers." + std::to_string(l);
            PK_TRY(pk_get_weight(params, p + ".conv", {G, R, K}, wc));
            PK_TRY(pk_get_weight(params, p + ".conv1x1_aux", {G, AUX, 1}, wa));
            PK_TRY(pk_get_weight(params, p + ".conv1x1_out", {R, G / 2, 1}, wo));
            PK_TRY(pk_get_weight(params, p + ".conv1x1_skip", {SK, G / 2, 1}, ws));
            PK_TRY(pk_get_vector(params, p + ".conv.bias", G, bc));
            PK_TRY(pk_get_vector(params, p + ".conv1x1_out.bias", R, bo));
            PK_TRY(pk_get_vector(params, p + ".conv1x1_skip.bias", SK, bs));
            std::vector<float> w2all(wo);
            w2all.insert(w2all.end(), ws.begin(), ws.end());
            g->k1[l] = pk_weight_scale_exp(wc.data(), wc.size());
            g->k2[l] = pk_weight_scale_exp(w2all.data(), w2all.size());
            // dilated conv: row block jb < GH/32 = tanh rows 32 jb + i, else sigmoid rows G/2 + 32 (jb - GH/32) + i; k = tap * R + ci
            auto v1 = [&](int row, int k) -> float {
                const int half = row / GH, j = row % GH;
                if (j >= G / 2) return 0.f;
                const int co = half * (G / 2) + j, tap = k / R, ci = k % R;
                return wc[((size_t)co * R + ci) * K + tap];
            };
            // [conv1x1_out ; conv1x1_skip]: rows o < R out, R <= o < R + SK skip; k = gated channel
            auto v2 = [&](int o, int k) -> float {
                if (k >= G / 2 || o >= R + SK) return 0.f;
                return o < R ? wo[(size_t)o * (G / 2) + k] : ws[(size_t)(o - R) * (G / 2) + k];
            };
            gen_pack(nb1, K * R, v1, W1f.data() + g->n1f * l, W1h.data() + g->n1h * l, W1b.data() + g->n1h * l, g->k1[l]);
            gen_pack(nb2, GH, v2, W2f.data() + g->n2f * l, W2h.data() + g->n2h * l, W2b.data() + g->n2h * l, g->k2[l]);
            for (int ca = 0; ca < AUX; ++ca)
                for (int co = 0; co < G; ++co) Wa[(size_t)ca * L * G + (size_t)l * G + co] = wa[(size_t)co * AUX + ca];
            float* bl = B.data() + (size_t)(G + R + SK) * l;
            for (int i = 0; i < G; ++i) bl[i] = bc[i];
            for (int i = 0; i < R; ++i) bl[G + i] = bo[i];
            for (int i = 0; i < SK; ++i) bl[G + R + i] = bs[i];
        }
        PK_TRY(pk_upload(ctx, g->d_w1f, W1f.data(), W1f.size() * sizeof(float)));
        PK_TRY(pk_upload(ctx, g->d_w2f, W2f.data(), W2f.size() * sizeof(float)));
        PK_TRY(pk_upload(ctx, g->d_w1h, W1h.data(), W1h.size() * sizeof(uint16_t)));
        PK_TRY(pk_upload(ctx, g->d_w2h, W2h.data(), W2h.size() * sizeof(uint16_t)));
        PK_TRY(pk_upload(ctx, g->d_w1b, W1b.data(), W1b.size() * sizeof(uint16_t)));
        PK_TRY(pk_upload(ctx, g->d_w2b, W2b.data(), W2b.size() * sizeof(uint16_t)));
        PK_TRY(pk_upload(ctx, g->d_bias, B.data(), B.size() * sizeof(float)));
        std::vector<float> packed;
        pk_gemm_pack(Wa.data(), AUXP, L * G, packed);
        PK_TRY(pk_upload(ctx, g->d_waux, packed.data(), packed.size() * sizeof(float)));
    }
    // last layers (rows padded to SKP with zero weights and biases)
    {
        std::vector<float> w1, b1, w2, b2;
        PK_TRY(pk_get_weight(params, "last_conv_layers.1", {SK, SK, 1}, w1));
        PK_TRY(pk_get_vector(params, "last_conv_layers.1.bias", SK, b1));
        PK_TRY(pk_get_weight(params, "last_conv_layers.3", {1, SK, 1}, w2));
        PK_TRY(pk_get_vector(params, "last_conv_layers.3.bias", 1, b2));
        std::vector<float> A((size_t)(SKP / 32) * (SK / 2) * 64), b1p(SKP, 0.f), w2p(SKP, 0.f);
        for (int ob = 0; ob < SKP / 32; ++ob)
            for (int ks = 0; ks < SK / 2; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int o = 32 * ob + (lane & 31), ci = 2 * ks + (lane >> 5);
                    A[((size_t)ob * (SK / 2) + ks) * 64 + lane] = o < SK ? w1[(size_t)o * SK + ci] : 0.f;
                }
        for (int i = 0; i < SK; ++i) {
            b1p[i] = b1[i];
            w2p[i] = w2[i];
        }
        PK_TRY(pk_upload(ctx, g->d_l1, A.data(), A.size() * sizeof(float)));
        PK_TRY(pk_upload(ctx, g->d_l1b, b1p.data(), SKP * sizeof(float)));
        PK_TRY(pk_upload(ctx, g->d_l2, w2p.data(), SKP * sizeof(float)));
        g->l2_bias = b2[0];
    }
    return PK_OK;
}

int pwg_gen_infer(pwg_gen* g, const pwg_gen_call& k, const float* mel, const int32_t* frames, int32_t B,
                  const float* noise, float* wav, int32_t flags) {
    pk_ctx* ctx = k.ctx;
    const pk_pwg_cfg& c = g->cfg;
    const int hop = g->hop, gap = g->gap, R = g->R, G = g->G, SK = g->SK, AUX = g->AUX, AUXP = g->AUXP;
    // ---- layout: |gap| utt 0 |gap| utt 1 |gap| ... , every utterance starting on a 64-sample tile boundary
    std::vector<int> cuL(B + 1, 0), toff(B), utt_S(B), utt_off(B), tile_first(B + 1, 0);
    long t = gap, packed = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] <= 0) PK_FAIL(PK_EINVAL, "pk_pwg_infer: utterance %d has %d frames", b, frames[b]);
        const long S_b = (long)frames[b] * hop;
        if (S_b >= (1L << 24)) PK_FAIL(PK_EUNSUPPORTED, "pk_pwg_infer: utterance %d is longer than 2^24 samples", b);
        cuL[b + 1] = cuL[b] + frames[b];
        toff[b] = (int)t;
        utt_S[b] = (int)S_b;
        utt_off[b] = (int)packed;
        tile_first[b + 1] = tile_first[b] + (int)((S_b + GT - 1) / GT);
        packed += S_b;
        t += (S_b + GT - 1) / GT * GT + gap;
        if (t >= (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_pwg_infer: %ld samples do not fit one call", packed);
    }
    const long Ttot = t;
    const int sumL = cuL[B], ntiles = tile_first[B];
    const long sumS = packed;
    g->last_frames.assign(frames, frames + B);
    g->last_toff = toff;
    g->last_cuL = cuL;
    g->last_Ttot = Ttot;
    std::vector<int> tab;
    auto push = [&](const std::vector<int>& v) {
        const size_t o = tab.size();
        tab.insert(tab.end(), v.begin(), v.end());
        return o;
    };
    std::vector<int> tile_t0(ntiles), tile_utt(ntiles);
    for (int b = 0; b < B; ++b)
        for (int i = tile_first[b]; i < tile_first[b + 1]; ++i) {
            tile_t0[i] = toff[b] + (i - tile_first[b]) * GT;
            tile_utt[i] = b;
        }
    const size_t o_t0 = push(tile_t0), o_tu = push(tile_utt), o_toff = push(toff), o_S = push(utt_S);
    const size_t o_F = push(std::vector<int>(frames, frames + B)), o_row0 = push(cuL), o_off = push(utt_off);
    const int cw = c.aux_context_window;
    const int rows_p = sumL + 2 * cw * B;
    const int rows_p_alloc = ((rows_p + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    std::vector<int> prow_src(rows_p_alloc, 0), prow_out(rows_p_alloc, -1);
    for (int b = 0; b < B; ++b) {
        const int r0 = cuL[b] + 2 * cw * b;
        for (int jr = 0; jr < frames[b] + 2 * cw; ++jr) {
            const int f = jr - cw;
            if (flags & PK_PWG_C_HAS_CONTEXT) prow_src[r0 + jr] = r0 + jr;
            else prow_src[r0 + jr] = cuL[b] + (f < 0 ? 0 : (f >= frames[b] ? frames[b] - 1 : f));
            if (f >= 0 && f < frames[b]) prow_out[r0 + jr] = cuL[b] + f;
        }
    }
    const size_t o_psrc = push(prow_src), o_pout = push(prow_out);
    PK_TRY(g->ws_tab.reserve(tab.size() * sizeof(int)));
    PK_HIP(hipMemcpyAsync(g->ws_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));   // tab is a stack vector
    const int* d_tab = g->ws_tab.as<int>();
    GenTabs tb;
    tb.tile_t0 = d_tab + o_t0;
    tb.tile_utt = d_tab + o_tu;
    tb.utt_toff = d_tab + o_toff;
    tb.utt_S = d_tab + o_S;
    tb.utt_F = d_tab + o_F;
    tb.utt_row0 = d_tab + o_row0;
    tb.utt_off = d_tab + o_off;

    // ---- inputs
    const float* d_mel = mel;
    const float* d_noise = noise;
    float* d_wav = wav;
    if (flags & PK_HOST_IO) {
        const size_t mel_rows = (size_t)sumL + ((flags & PK_PWG_C_HAS_CONTEXT) ? (size_t)2 * cw * B : 0);
        PK_TRY(g->ws_mel.reserve(mel_rows * AUX * 4));
        PK_TRY(g->ws_wav.reserve((size_t)sumS * 4));
        PK_HIP(hipMemcpyAsync(g->ws_mel.p, mel, mel_rows * AUX * 4, hipMemcpyHostToDevice, ctx->stream));
        d_mel = g->ws_mel.as<float>();
        d_wav = g->ws_wav.as<float>();
        if (noise) {
            PK_TRY(g->ws_noise.reserve((size_t)sumS * 4));
            PK_HIP(hipMemcpyAsync(g->ws_noise.p, noise, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
            d_noise = g->ws_noise.as<float>();
        }
    }
    if (!noise) {   // x = randn(...) (:515-516): the next range of the handle's stream
        PK_TRY(g->ws_noise.reserve((size_t)sumS * 4));
        PK_TRY(pk_randn_device(ctx, g->ws_noise.as<float>(), sumS, k.seed, *k.rng_offset));
        *k.rng_offset += ((unsigned long long)sumS + 3) / 4 * 4;
        d_noise = g->ws_noise.as<float>();
    }
    // ---- workspaces; the gaps of x (and everything else) start as zeros
    const int rows_alloc = ((sumL + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    const int ldp = c.layers * G;
    g->last_ldp = ldp;
    const size_t nblk = (size_t)(Ttot / 32);
    PK_TRY(g->ws_c0.reserve((size_t)(rows_alloc + 2 * G_P_LEAD) * AUXP * 4));
    PK_TRY(g->ws_cin.reserve((size_t)(rows_p_alloc + 2 * G_P_LEAD) * AUXP * 4));
    PK_TRY(g->ws_P.reserve((size_t)(rows_alloc + 2 * G_P_LEAD) * ldp * 4));
    PK_TRY(g->ws_x0.reserve((size_t)R * Ttot * 4));
    PK_TRY(g->ws_x1.reserve((size_t)R * Ttot * 4));
    PK_TRY(g->ws_skip.reserve((size_t)SK * Ttot * 4));
    PK_TRY(g->ws_xe0.reserve(nblk * 4));
    PK_TRY(g->ws_xe1.reserve(nblk * 4));
    PK_HIP(hipMemsetAsync(g->ws_x0.p, 0, (size_t)R * Ttot * 4, ctx->stream));
    PK_HIP(hipMemsetAsync(g->ws_x1.p, 0, (size_t)R * Ttot * 4, ctx->stream));
    PK_HIP(hipMemsetAsync(g->ws_xe0.p, 0, nblk * 4, ctx->stream));
    PK_HIP(hipMemsetAsync(g->ws_xe1.p, 0, nblk * 4, ctx->stream));
    float* c0 = g->ws_c0.as<float>() + (size_t)G_P_LEAD * AUXP;
    float* P = g->ws_P.as<float>() + (size_t)G_P_LEAD * ldp;
    PK_HIP(hipMemsetAsync(g->ws_P.p, 0, (size_t)G_P_LEAD * ldp * 4, ctx->stream));
    PK_HIP(hipMemsetAsync(P + (size_t)sumL * ldp, 0, (size_t)(rows_alloc - sumL + G_P_LEAD) * ldp * 4, ctx->stream));
    // ---- conditioning at frame rate: conv_in, then all layers' conv1x1_aux as one GEMM
    {
        float* cin = g->ws_cin.as<float>() + (size_t)G_P_LEAD * AUXP;
        PK_LAUNCH(ctx, "pwg_convin_prep", k_pwg_convin_prep_gen, dim3(rows_p_alloc), dim3(128), 0, d_mel, k.mu, k.sigma,
                  (k.use_norm && (flags & PK_APPLY_NORMALIZER)) ? 1 : 0, d_tab + o_psrc, rows_p, AUX, AUXP, cin);
        pk_gemm_args a;
        a.A = cin;
        a.lda = AUXP;
        a.Wp = g->d_convin.as<float>();
        a.C = c0;
        a.ldc = AUXP;
        a.M = rows_p;
        a.N = AUXP;
        a.Cin = AUXP;
        a.taps = 2 * cw + 1;
        a.pad = cw;
        a.out_rowmap = d_tab + o_pout;
        PK_TRY(pk_gemm_launch(ctx, "pwg_convin_gemm", a));
        pk_gemm_args q;
        q.A = c0;
        q.lda = AUXP;
        q.Wp = g->d_waux.as<float>();
        q.C = P;
        q.ldc = ldp;
        q.M = sumL;
        q.N = ldp;
        q.Cin = AUXP;
        PK_TRY(pk_gemm_launch(ctx, "pwg_aux_gemm", q));
    }
    // ---- first conv, residual stack (optionally in chunks of whole utterances: scheduling only), last layers
    PK_LAUNCH(ctx, "pwg_first_gen", k_pwg_first_gen, dim3(ntiles), dim3(256), 0, d_noise, g->d_first_w.as<float>(),
              g->d_first_b.as<float>(), tb, R, g->ws_x0.as<float>(), g->ws_xe0.as<unsigned>());
    {
        const int lps = c.layers / c.stacks;
        std::vector<int> chunk_first;
        long acc = 0;
        for (int b = 0; b < B; ++b) {
            if (b == 0 || acc + utt_S[b] > k.chunk_samples) {
                chunk_first.push_back(b);
                acc = 0;
            }
            acc += utt_S[b];
        }
        chunk_first.push_back(B);
        const int mode = k.math == PK_PWG_MATH_F32 ? GM_F32 : (k.math == PK_PWG_MATH_BF16X3 ? GM_BF16X3 : GM_F16X3);
        for (size_t ck = 0; ck + 1 < chunk_first.size(); ++ck) {
            const int tile0 = tile_first[chunk_first[ck]], nt = tile_first[chunk_first[ck + 1]] - tile0;
            for (int l = 0; l < c.layers; ++l) {
                GenLayer a;
                a.xin = (l & 1) ? g->ws_x1.as<float>() : g->ws_x0.as<float>();
                a.xout = (l & 1) ? g->ws_x0.as<float>() : g->ws_x1.as<float>();
                a.skip = g->ws_skip.as<float>();
                a.xe_in = (l & 1) ? g->ws_xe1.as<unsigned>() : g->ws_xe0.as<unsigned>();
                a.xe_out = (l & 1) ? g->ws_xe0.as<unsigned>() : g->ws_xe1.as<unsigned>();
                a.w1f = g->d_w1f.as<float>() + g->n1f * l;
                a.w2f = g->d_w2f.as<float>() + g->n2f * l;
                const pk_dbuf& w1 = mode == GM_BF16X3 ? g->d_w1b : g->d_w1h;
                const pk_dbuf& w2 = mode == GM_BF16X3 ? g->d_w2b : g->d_w2h;
                a.w1h = w1.as<uint16_t>() + g->n1h * l;
                a.w2h = w2.as<uint16_t>() + g->n2h * l;
                a.bias = g->d_bias.as<float>() + (size_t)(G + R + SK) * l;
                a.P = P + (size_t)l * G;
                a.uptab = g->d_uptab.as<float>();
                a.tb = tb;
                a.tb.tile_t0 += tile0;
                a.tb.tile_utt += tile0;
                a.ldp = ldp;
                a.hop = hop;
                a.R = R;
                a.G = G;
                a.SK = SK;
                a.K = g->K;
                a.dil = 1 << (l % lps);
                a.GH = g->GH;
                a.OP = g->OP;
                a.first = l == 0;
                a.k1 = mode == GM_F16X3 ? g->k1[l] : 0;
                a.k2 = mode == GM_F16X3 ? g->k2[l] : 0;
                const bool wide = g->GH > 128;
                if (mode == GM_F32) {
                    if (wide) PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_F32, 260>), dim3(nt), dim3(256), 0, a);
                    else PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_F32, 132>), dim3(nt), dim3(256), 0, a);
                } else if (mode == GM_F16X3) {
                    if (wide) PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_F16X3, 260>), dim3(nt), dim3(256), 0, a);
                    else PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_F16X3, 132>), dim3(nt), dim3(256), 0, a);
                } else {
                    if (wide) PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_BF16X3, 260>), dim3(nt), dim3(256), 0, a);
                    else PK_LAUNCH(ctx, "pwg_block_gen", (k_pwg_block_gen<GM_BF16X3, 132>), dim3(nt), dim3(256), 0, a);
                }
            }
        }
        g->last_x_final = c.layers & 1;
    }
    {
        GenLast a;
        a.skip = g->ws_skip.as<float>();
        a.w1f = g->d_l1.as<float>();
        a.b1 = g->d_l1b.as<float>();
        a.w2 = g->d_l2.as<float>();
        a.b2 = g->l2_bias;
        a.scale = (float)std::sqrt(1.0 / c.layers);
        a.tb = tb;
        a.SK = SK;
        a.SKP = g->SKP;
        a.wav = d_wav;
        PK_LAUNCH(ctx, "pwg_last_gen", k_pwg_last_gen, dim3(ntiles), dim3(256), 0, a);
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(wav, d_wav, (size_t)sumS * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

int pwg_gen_debug_read(pwg_gen* g, pk_ctx* ctx, int32_t what, int32_t b, float* host_out, int64_t n_floats) {
    if (g->last_Ttot == 0) PK_FAIL(PK_ESTATE, "pk_pwg_debug_read: no inference has run");
    if (b < 0 || b >= (int)g->last_frames.size()) PK_FAIL(PK_EINVAL, "pk_pwg_debug_read: utterance out of range");
    const long S = (long)g->last_frames[b] * g->hop;
    if (what == 0) {
        if (n_floats != (int64_t)g->G * S) PK_FAIL(PK_ESHAPE, "pk_pwg_debug_read: expected %ld floats", (long)g->G * S);
        PK_TRY(g->ws_dbg.reserve((size_t)g->G * S * 4));
        const float* P = g->ws_P.as<float>() + (size_t)G_P_LEAD * g->last_ldp;
        PK_LAUNCH(ctx, "pwg_aux_debug", k_pwg_aux_debug_gen, dim3(g->last_frames[b], g->G), dim3(256), 0, P, g->last_ldp,
                  g->d_uptab.as<float>(), g->last_cuL[b], g->last_frames[b], g->hop, g->ws_dbg.as<float>());
        PK_HIP(hipStreamSynchronize(ctx->stream));
        PK_HIP(hipMemcpy(host_out, g->ws_dbg.p, (size_t)g->G * S * 4, hipMemcpyDeviceToHost));
        return PK_OK;
    }
    if (what == 3) PK_FAIL(PK_EUNSUPPORTED, "pk_pwg_debug_read: the generic path keeps no block maxima tap");
    const float* src;
    int rows;
    switch (what) {
        case 1: src = g->last_x_final ? g->ws_x1.as<float>() : g->ws_x0.as<float>(); rows = g->R; break;
        case 2: src = g->ws_skip.as<float>(); rows = g->SK; break;
        default: PK_FAIL(PK_EINVAL, "pk_pwg_debug_read: unknown tap %d", what);
    }
    if (n_floats != (int64_t)rows * S)
        PK_FAIL(PK_ESHAPE, "pk_pwg_debug_read: expected %ld floats, got %lld", rows * S, (long long)n_floats);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    const long t0 = g->last_toff[b];   // a multiple of 64
    const size_t pitch = (size_t)rows * 32;
    for (int ch = 0; ch < rows; ++ch) {
        if (S / 32 > 0)
            PK_HIP(hipMemcpy2D(host_out + (size_t)ch * S, 32 * sizeof(float), src + (t0 >> 5) * pitch + (size_t)ch * 32,
                               pitch * sizeof(float), 32 * sizeof(float), S / 32, hipMemcpyDeviceToHost));
        if (S % 32)
            PK_HIP(hipMemcpy(host_out + (size_t)ch * S + S / 32 * 32, src + ((t0 + S / 32 * 32) >> 5) * pitch + (size_t)ch * 32,
                             (size_t)(S % 32) * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PK_OK;
}

void pwg_gen_destroy(pwg_gen* g) {
    if (!g) return;
    pk_dbuf* bufs[] = {&g->d_first_w, &g->d_first_b, &g->d_convin, &g->d_waux, &g->d_uptab, &g->d_bias, &g->d_w1f, &g->d_w2f,
                       &g->d_w1h, &g->d_w2h, &g->d_w1b, &g->d_w2b, &g->d_l1, &g->d_l1b, &g->d_l2, &g->ws_mel, &g->ws_noise,
                       &g->ws_wav, &g->ws_cin, &g->ws_c0, &g->ws_P, &g->ws_x0, &g->ws_x1, &g->ws_skip, &g->ws_xe0,
                       &g->ws_xe1, &g->ws_tab, &g->ws_dbg};
    for (auto* b : bufs) b->release();
    delete g;
}
