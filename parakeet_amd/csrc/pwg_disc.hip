// pwg_disc.hip -- the Parallel WaveGAN discriminator on gfx950: every layer of the stack in one kernel, activations in LDS.
//
// Reference: parakeet/models/parallel_wavegan/parallel_wavegan.py PWGDiscriminator :523-630 -- layers - 1 blocks of
// Conv1D(kernel k, dilation d_i, padding (k - 1) / 2 * d_i) + LeakyReLU, d_0 = 1 and d_i = i (dilation_factor 1) or
// dilation_factor^i, then one Conv1D(conv_channels -> 1, k, dilation 1); and the three MSE terms the evaluator forms of its
// logits (parallel_wavegan_updater.py:192-223): sum (p - 1)^2 and sum p^2 per utterance.
//
// Layer by layer through memory the stack would move 2 * 4 * conv_channels bytes per sample and hidden layer.  Here one
// workgroup takes a window of W = pwgd_window(C) samples of one utterance -- an output tile and the receptive field (halo) on
// both sides, windows start at utterance-relative multiples of the tile -- and carries it through all layers in two LDS
// buffers [channel][position] that alternate as input and output; 4 bytes per sample come in, at most 4 go out.
//   block 0 (one input channel, K = k) and the last conv (one output row) are plain fp32 FMAs;
//   blocks 1 ... layers - 2 are MFMA contractions with K = k * C: out[cout][pos] = sum_(tap, cin) W[cout][cin][tap] *
//   x[cin][pos + (tap - (k - 1) / 2) * d].  The weights are the A operand (fragments packed at finalize, read through the
//   caches), the positions the 32 columns of a tile.  Each of the four waves owns PT position tiles and all CT = ceil(C / 32)
//   output-channel tiles of them, so a weight fragment is read once per wave and k-step.
// Every layer zero-pads ITS OWN input at the two ends of the utterance: an activation at a position outside [0, len) is 0 at
// every layer (not bias + LeakyReLU of zeros), written by a select in every epilogue.  The same select zeroes the positions
// of the window whose receptive field the window no longer covers (the valid span shrinks by (k - 1) / 2 * d_i per layer;
// the tile in the middle stays valid through the last layer), so that nothing undefined is ever stored.
//
// Math: PK_PWG_MATH_F32 on v_mfma_f32_32x32x2_f32; PK_PWG_MATH_F16X3 (default) as a_hi*b_hi + a_lo*b_hi +
// a_hi*b_lo on v_mfma_f32_32x32x16_f16 with block-scaled operands: the weights one exponent per tensor (folded into the
// stored fragments), the activations one exponent per window and layer, MEASURED in the producing layer's epilogue (max |x|
// over the window, after the select) -- no a-priori bound.  The window depends on the utterance alone, so do the scales.
//
// Loss terms: fp32 per logit, a tile's terms added in fp32 (butterfly inside a wave, the four waves in order), the tiles of
// an utterance in fp64 in a fixed order by a second kernel.  No atomics.  An utterance's logits and sums are the same bits
// alone, in any batch and at any position in it.
#include <cmath>
#include <exception>
#include <string>
#include <vector>

#include "pk_common.h"
#include "pk_mfma.h"
#include "pk_pwg_disc.h"

namespace {

struct pwgd_args {
    const float* wav;        // packed samples
    const long* woff;        // [B] first sample of an utterance
    const int* lens;         // [B]
    const int* tile_b;       // [tiles] utterance of a tile
    const int* tile0;        // [B + 1] first tile of an utterance
    float* logits;           // packed, or NULL
    float* part;             // [tiles][2] partial sums, or NULL
    const float* w0;         // [C][k] block 0
    const float* bias;       // [layers - 1][CP] hidden biases (zero rows past C)
    const float* wf32;       // blocks 1 ...: [k][C / 2][CT][64] fp32 fragments
    const f16x8* wf16;       // blocks 1 ...: [k][C / 16][CT][hi, lo][64] fp16 fragments of 2^kw * W
    const float* wlast;      // [k][C]
    float blast, slope;
    int C, k, nblocks;       // nblocks = layers - 1 hidden blocks
    int tile, halo;
    int dil[PWGD_MAX_LAYERS];
    int kw[PWGD_MAX_LAYERS]; // weight exponent of a block (F16X3)
    int dbg_layer;           // >= 0: the block whose activation goes to dbg_out
    float* dbg_out;          // (C, lens[0]) of the single utterance of a debug launch
};

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

template <int MATH, int CT, int PT>
__global__ __launch_bounds__(PWGD_THREADS) void k_pwgd(const pwgd_args a) {
    constexpr int W = 128 * PT, CP = 32 * CT;
    __shared__ float buf[2][CP * W];
    __shared__ float xin[W];
    __shared__ float s_amax[2][4];
    __shared__ float s_red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int tb = blockIdx.x, b = a.tile_b[tb], len = a.lens[b];
    const long base = a.woff[b];
    const int C = a.C, k = a.k, ch = (k - 1) / 2;
    const int g0 = (tb - a.tile0[b]) * a.tile - a.halo;   // utterance-relative position of window index 0
    const float slope = a.slope;

    for (int p = tid; p < W; p += PWGD_THREADS) {
        const int g = g0 + p;
        xin[p] = (g >= 0 && g < len) ? a.wav[base + g] : 0.f;
    }
    __syncthreads();

    // is window position p a defined activation after a block whose valid span starts at S?
    auto valid = [&](int p, int S) { return p >= S && p < W - S && (unsigned)(g0 + p) < (unsigned)len; };
    // the test tap (uniform branch, after the block's barrier): the tile's part of a block's output
    auto debug_dump = [&](const float* act) {
        for (int idx = tid; idx < C * a.tile; idx += PWGD_THREADS) {
            const int c = idx / a.tile, p = a.halo + (idx - c * a.tile);
            if (g0 + p < len) a.dbg_out[(long)c * len + (g0 + p)] = act[c * W + p];
        }
    };

    // ---- block 0: one input channel, fp32 FMAs
    int S = ch * a.dil[0];
    float m = 0.f;
    for (int idx = tid; idx < C * W; idx += PWGD_THREADS) {
        const int c = idx / W, p = idx - c * W;
        float acc = 0.f;
        for (int t = 0; t < k; ++t) {
            const int q = p + (t - ch) * a.dil[0];
            const float xv = (q >= 0 && q < W) ? xin[q] : 0.f;
            acc = fmaf(a.w0[c * k + t], xv, acc);
        }
        float v = leaky(acc + a.bias[c], slope);
        v = valid(p, S) ? v : 0.f;
        buf[0][c * W + p] = v;
        m = fmaxf(m, fabsf(v));
    }
    if (MATH == PK_PWG_MATH_F16X3) {
        m = wave_max64(m);
        if (lane == 0) s_amax[0][wave] = m;
    }
    __syncthreads();
    if (a.dbg_layer == 0) debug_dump(buf[0]);

    // ---- blocks 1 ... nblocks - 1: MFMA contractions, K = k * C
    for (int i = 1; i < a.nblocks; ++i) {
        const float* in = buf[(i - 1) & 1];
        float* out = buf[i & 1];
        const int d = a.dil[i];
        S += ch * d;
        f32x16 acc[PT][CT];
#pragma unroll
        for (int pi = 0; pi < PT; ++pi)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[pi][ct][r] = 0.f;
        float unscale = 1.f;
        if (MATH == PK_PWG_MATH_F32) {
            const float* wl = a.wf32 + (size_t)(i - 1) * k * (C / 2) * CT * 64 + lane;
            for (int t = 0; t < k; ++t) {
                int q[PT];
#pragma unroll
                for (int pi = 0; pi < PT; ++pi) {
                    const int p = (wave * PT + pi) * 32 + l31 + (t - ch) * d;
                    q[pi] = p < 0 ? 0 : (p > W - 1 ? W - 1 : p);   // past the window only undefined outputs read: any value does
                }
#pragma unroll 4
                for (int ks = 0; ks < C / 2; ++ks) {
                    float av[CT], bv[PT];
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) av[ct] = wl[(size_t)((t * (C / 2) + ks) * CT + ct) * 64];
#pragma unroll
                    for (int pi = 0; pi < PT; ++pi) bv[pi] = in[(2 * ks + hi) * W + q[pi]];
#pragma unroll
                    for (int pi = 0; pi < PT; ++pi)
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            acc[pi][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ct], bv[pi], acc[pi][ct], 0, 0, 0);
                }
            }
        } else {
            const float am = fmaxf(fmaxf(s_amax[(i - 1) & 1][0], s_amax[(i - 1) & 1][1]),
                                   fmaxf(s_amax[(i - 1) & 1][2], s_amax[(i - 1) & 1][3]));
            const int kx = blk_scale_exp(__float_as_uint(am));
            const float s = pow2f(kx);
            unscale = pow2f(-kx - a.kw[i]);
            const f16x8* wl = a.wf16 + (size_t)(i - 1) * k * (C / 16) * CT * 2 * 64 + lane;
            for (int t = 0; t < k; ++t) {
                int q[PT];
#pragma unroll
                for (int pi = 0; pi < PT; ++pi) {
                    const int p = (wave * PT + pi) * 32 + l31 + (t - ch) * d;
                    q[pi] = p < 0 ? 0 : (p > W - 1 ? W - 1 : p);
                }
#pragma unroll 2
                for (int kb = 0; kb < C / 16; ++kb) {
                    f16x8 bh[PT], bl[PT];
#pragma unroll
                    for (int pi = 0; pi < PT; ++pi) {
                        float v[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = in[(kb * 16 + 8 * hi + e) * W + q[pi]];
                        store_pair8(v, s, bh[pi], bl[pi]);
                    }
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const f16x8* wp = wl + (size_t)((t * (C / 16) + kb) * CT + ct) * 2 * 64;
                        const f16x8 ah = wp[0], al = wp[64];
#pragma unroll
                        for (int pi = 0; pi < PT; ++pi) {
                            acc[pi][ct] = mfma16(ah, bh[pi], acc[pi][ct]);
                            acc[pi][ct] = mfma16(al, bh[pi], acc[pi][ct]);
                            acc[pi][ct] = mfma16(ah, bl[pi], acc[pi][ct]);
                        }
                    }
                }
            }
        }
        // epilogue: unscale, bias, LeakyReLU, the select, the next layer's scale
        const float* bias = a.bias + i * CP;
        m = 0.f;
#pragma unroll
        for (int pi = 0; pi < PT; ++pi) {
            const int p = (wave * PT + pi) * 32 + l31;
            const bool ok = valid(p, S);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cout = ct * 32 + mfma_row(r, hi);
                    float v = acc[pi][ct][r];
                    if (MATH == PK_PWG_MATH_F16X3) v *= unscale;
                    v = leaky(v + bias[cout], slope);
                    v = ok ? v : 0.f;
                    out[cout * W + p] = v;
                    m = fmaxf(m, fabsf(v));
                }
        }
        if (MATH == PK_PWG_MATH_F16X3) {
            m = wave_max64(m);
            if (lane == 0) s_amax[i & 1][wave] = m;
        }
        __syncthreads();
        if (a.dbg_layer == i) debug_dump(out);
    }

    // ---- last conv: one output row, fp32 FMAs, then the loss terms of the tile
    const float* in = buf[(a.nblocks - 1) & 1];
    float t0 = 0.f, t1 = 0.f;
    for (int p = tid; p < W; p += PWGD_THREADS) {
        const int g = g0 + p;
        if (p < a.halo || p >= a.halo + a.tile || g >= len) continue;
        float acc = 0.f;
        for (int t = 0; t < k; ++t) {
            const int q = p + t - ch;   // halo >= ch: inside the window
            for (int c = 0; c < C; ++c) acc = fmaf(a.wlast[t * C + c], in[c * W + q], acc);
        }
        const float logit = acc + a.blast;
        if (a.logits) a.logits[base + g] = logit;
        const float e = logit - 1.f;
        t0 += e * e;
        t1 += logit * logit;
    }
    if (!a.part) return;
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) {
        t0 += __shfl_xor(t0, dd);
        t1 += __shfl_xor(t1, dd);
    }
    if (lane == 0) {
        s_red[0][wave] = t0;
        s_red[1][wave] = t1;
    }
    __syncthreads();
    if (tid < 2) a.part[(long)tb * 2 + tid] = ((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3];
}

// One block per utterance: out[b][c] = sum over its tiles of part[.][c], in fp64.  Thread t adds tiles t, t + 256, ... in
// ascending order, then a tree over the 256 threads: the order depends on the utterance's tile count alone.
__global__ __launch_bounds__(256) void k_pwgd_fold(const float* __restrict__ part, const int* __restrict__ tile0,
                                                   double* __restrict__ out) {
    __shared__ double sh[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int lo = tile0[b], n = tile0[b + 1] - lo;
    double a0 = 0.0, a1 = 0.0;
    for (int f = t; f < n; f += 256) {
        a0 += (double)part[(long)(lo + f) * 2];
        a1 += (double)part[(long)(lo + f) * 2 + 1];
    }
    sh[0][t] = a0;
    sh[1][t] = a1;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            sh[0][t] += sh[0][t + d];
            sh[1][t] += sh[1][t + d];
        }
        __syncthreads();
    }
    if (t < 2) out[(long)b * 2 + t] = sh[t][0];
}

}  // namespace

struct pk_pwgd {
    pk_ctx* ctx = nullptr;
    pk_pwgd_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int math = PK_PWG_MATH_F16X3;
    bool keep_input = false;
    int halo = 0, tile = 0, CT = 0;
    int dil[PWGD_MAX_LAYERS] = {0};
    int kw[PWGD_MAX_LAYERS] = {0};
    float blast = 0.f;
    pk_dbuf d_w0, d_bias, d_wf32, d_wf16, d_wlast;
    pk_dbuf ws_itab, ws_ltab, ws_wav, ws_logits, ws_part, ws_out, ws_dbg;
    // the last run's input, kept under pk_pwgd_set_debug for pk_pwgd_debug_read
    pk_dbuf last_wav;
    std::vector<int> last_lens;
    std::vector<long> last_woff;
};

// dilation of block i (:571-577) and the halo the stack needs; false when it leaves the kernel's window
static bool pwgd_geometry(const pk_pwgd_cfg& c, int* dil, int& halo) {
    const int ch = (c.kernel_size - 1) / 2, cap = pwgd_max_halo(c.conv_channels);
    long sum = 1;   // the last conv's dilation
    for (int i = 0; i < c.layers - 1; ++i) {
        long d = 1;
        if (i > 0) {
            if (c.dilation_factor == 1) d = i;
            else
                for (int j = 0; j < i && d <= 4096; ++j) d *= c.dilation_factor;
        }
        if (d > 4096) return false;
        dil[i] = (int)d;
        sum += d;
    }
    halo = (int)(ch * sum);
    return halo <= cap;
}

extern "C" int pk_pwgd_create(pk_ctx* ctx, const pk_pwgd_cfg* cfg, pk_pwgd** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_pwgd_create: NULL argument");
    *out = nullptr;
    const pk_pwgd_cfg& c = *cfg;
    if (c.in_channels != 1 || c.out_channels != 1)
        PK_FAIL(PK_EUNSUPPORTED, "PWGDiscriminator: in_channels and out_channels must be 1 (got %d, %d)", c.in_channels,
                c.out_channels);
    if (c.kernel_size < 1 || c.kernel_size > PWGD_MAX_K || c.kernel_size % 2 == 0)
        PK_FAIL(PK_EUNSUPPORTED, "PWGDiscriminator: kernel_size must be odd, 1 ... %d (got %d)", PWGD_MAX_K, c.kernel_size);
    if (c.layers < 3 || c.layers > PWGD_MAX_LAYERS)
        PK_FAIL(PK_EUNSUPPORTED, "PWGDiscriminator: layers must be 3 ... %d (got %d; the reference cannot run 2)",
                PWGD_MAX_LAYERS, c.layers);
    if (c.conv_channels < 16 || c.conv_channels > 128 || c.conv_channels % 16 != 0)
        PK_FAIL(PK_EUNSUPPORTED, "PWGDiscriminator: conv_channels must be a multiple of 16 in 16 ... 128 (got %d)",
                c.conv_channels);
    if (c.dilation_factor < 1)
        PK_FAIL(PK_EUNSUPPORTED, "PWGDiscriminator: dilation_factor must be >= 1 (got %d)", c.dilation_factor);
    if (!std::isfinite(c.negative_slope)) PK_FAIL(PK_EINVAL, "PWGDiscriminator: negative_slope is not finite");
    int dil[PWGD_MAX_LAYERS] = {0}, halo = 0;
    if (!pwgd_geometry(c, dil, halo))
        PK_FAIL(PK_EUNSUPPORTED,
                "PWGDiscriminator: the receptive field per side, (kernel_size - 1) / 2 * (sum of dilations + 1), must be at "
                "most %d samples at %d channels", pwgd_max_halo(c.conv_channels), c.conv_channels);
    pk_pwgd* h = new pk_pwgd();
    h->ctx = ctx;
    h->cfg = c;
    h->halo = halo;
    h->tile = pwgd_window(c.conv_channels) - 2 * halo;
    h->CT = (c.conv_channels + 31) / 32;
    for (int i = 0; i < PWGD_MAX_LAYERS; ++i) h->dil[i] = dil[i];
    *out = h;
    return PK_OK;
}

extern "C" int pk_pwgd_set_param(pk_pwgd* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_pwgd_set_param: handle is NULL");
    h->finalized = false;
    return pk_store_param(h->params, name, data, shape, ndim);
}

extern "C" int pk_pwgd_set_math(pk_pwgd* h, int32_t mode) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_pwgd_set_math: handle is NULL");
    if (mode == PK_PWG_MATH_BF16X3) PK_FAIL(PK_EUNSUPPORTED, "pk_pwgd_set_math: the discriminator has no split-bf16 variant");
    if (mode != PK_PWG_MATH_F32 && mode != PK_PWG_MATH_F16X3) PK_FAIL(PK_EINVAL, "pk_pwgd_set_math: unknown mode %d", mode);
    h->math = mode;
    return PK_OK;
}

extern "C" int pk_pwgd_set_debug(pk_pwgd* h, int32_t on) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_pwgd_set_debug: handle is NULL");
    h->keep_input = on != 0;
    if (!on) h->last_lens.clear();
    return PK_OK;
}

extern "C" int pk_pwgd_tile_samples(pk_pwgd* h, int32_t* tile, int32_t* halo) {
    if (!h || !tile || !halo) PK_FAIL(PK_EINVAL, "pk_pwgd_tile_samples: NULL argument");
    *tile = h->tile;
    *halo = h->halo;
    return PK_OK;
}

static int pwgd_finalize(pk_pwgd* h) {
    pk_ctx* ctx = h->ctx;
    const pk_pwgd_cfg& c = h->cfg;
    const int C = c.conv_channels, k = c.kernel_size, nb = c.layers - 1, CT = h->CT, CP = 32 * CT;
    auto key = [](int i) { return "conv_layers." + std::to_string(2 * i); };
    std::vector<float> w, bv;
    std::vector<float> bias((size_t)nb * CP, 0.f);
    for (int i = 0; i < nb; ++i)
        if (c.bias) {
            PK_TRY(pk_get_vector(h->params, key(i) + ".bias", C, bv));
            for (int o = 0; o < C; ++o) bias[(size_t)i * CP + o] = bv[o];
        }
    PK_TRY(pk_upload(ctx, h->d_bias, bias.data(), bias.size() * sizeof(float)));
    PK_TRY(pk_get_weight(h->params, key(0), {C, 1, k}, w));
    PK_TRY(pk_upload(ctx, h->d_w0, w.data(), (size_t)C * k * sizeof(float)));
    // blocks 1 ... nb - 1: the two fragment layouts, lane (r, hi) of a k-step holding row cout = 32 ct + r
    const size_t per32 = (size_t)k * (C / 2) * CT * 64, per16 = (size_t)k * (C / 16) * CT * 2 * 64 * 8;
    std::vector<float> f32(per32 * (nb - 1), 0.f);
    std::vector<uint16_t> f16(per16 * (nb - 1), 0);
    for (int i = 1; i < nb; ++i) {
        PK_TRY(pk_get_weight(h->params, key(i), {C, C, k}, w));
        const int kw = pk_weight_scale_exp(w.data(), w.size());
        h->kw[i] = kw;
        auto at = [&](int co, int ci, int t) { return co < C ? w[((size_t)co * C + ci) * k + t] : 0.f; };
        float* p32 = f32.data() + per32 * (i - 1);
        uint16_t* p16 = f16.data() + per16 * (i - 1);
        for (int t = 0; t < k; ++t)
            for (int ct = 0; ct < CT; ++ct)
                for (int lane = 0; lane < 64; ++lane) {
                    const int co = 32 * ct + (lane & 31), hi = lane >> 5;
                    for (int ks = 0; ks < C / 2; ++ks)
                        p32[((size_t)(t * (C / 2) + ks) * CT + ct) * 64 + lane] = at(co, 2 * ks + hi, t);
                    for (int kb = 0; kb < C / 16; ++kb)
                        for (int e = 0; e < 8; ++e) {
                            const float x = std::ldexp(at(co, 16 * kb + 8 * hi + e, t), kw);
                            const _Float16 xh = (_Float16)x, xl = (_Float16)(x - (float)xh);
                            const size_t o = ((((size_t)(t * (C / 16) + kb) * CT + ct) * 2) * 64 + lane) * 8 + e;
                            memcpy(&p16[o], &xh, 2);
                            memcpy(&p16[o + 512], &xl, 2);
                        }
                }
    }
    PK_TRY(pk_upload(ctx, h->d_wf32, f32.data(), std::max<size_t>(f32.size(), 1) * sizeof(float)));
    PK_TRY(pk_upload(ctx, h->d_wf16, f16.data(), std::max<size_t>(f16.size(), 8) * sizeof(uint16_t)));
    PK_TRY(pk_get_weight(h->params, key(nb), {1, C, k}, w));
    std::vector<float> wl((size_t)k * C);
    for (int ci = 0; ci < C; ++ci)
        for (int t = 0; t < k; ++t) wl[(size_t)t * C + ci] = w[(size_t)ci * k + t];
    PK_TRY(pk_upload(ctx, h->d_wlast, wl.data(), wl.size() * sizeof(float)));
    h->blast = 0.f;
    if (c.bias) {
        PK_TRY(pk_get_vector(h->params, key(nb) + ".bias", 1, bv));
        h->blast = bv[0];
    }
    h->finalized = true;
    return PK_OK;
}

extern "C" int pk_pwgd_finalize(pk_pwgd* h) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_pwgd_finalize: handle is NULL");
    PK_DEVICE(h->ctx->device);
    try {
        return pwgd_finalize(h);
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_pwgd_finalize: host tables: %s", e.what());
    }
}

// the stack over `B` utterances whose tables (lens | tile0 | tile_b in itab, woff in ltab) are on the device
static int pwgd_launch(pk_pwgd* h, const float* d_wav, int B, int tiles, float* d_logits, float* d_part, int dbg_layer,
                       float* d_dbg) {
    pk_ctx* ctx = h->ctx;
    const pk_pwgd_cfg& c = h->cfg;
    pwgd_args a;
    a.wav = d_wav;
    a.woff = h->ws_ltab.as<long>();
    a.lens = h->ws_itab.as<int>();
    a.tile0 = a.lens + B;
    a.tile_b = a.tile0 + B + 1;
    a.logits = d_logits;
    a.part = d_part;
    a.w0 = h->d_w0.as<float>();
    a.bias = h->d_bias.as<float>();
    a.wf32 = h->d_wf32.as<float>();
    a.wf16 = h->d_wf16.as<f16x8>();
    a.wlast = h->d_wlast.as<float>();
    a.blast = h->blast;
    a.slope = c.negative_slope;
    a.C = c.conv_channels;
    a.k = c.kernel_size;
    a.nblocks = c.layers - 1;
    a.tile = h->tile;
    a.halo = h->halo;
    for (int i = 0; i < PWGD_MAX_LAYERS; ++i) {
        a.dil[i] = h->dil[i];
        a.kw[i] = h->kw[i];
    }
    a.dbg_layer = dbg_layer;
    a.dbg_out = d_dbg;
    const dim3 grid(tiles), block(PWGD_THREADS);
#define PWGD_GO(M, CTV, PTV) PK_LAUNCH(ctx, "pwgd_stack", (k_pwgd<M, CTV, PTV>), grid, block, 0, a)
#define PWGD_SHAPE(M)                  \
    switch (h->CT) {                   \
        case 1: PWGD_GO(M, 1, 2); break; \
        case 2: PWGD_GO(M, 2, 2); break; \
        case 3: PWGD_GO(M, 3, 1); break; \
        default: PWGD_GO(M, 4, 1); break; \
    }
    if (h->math == PK_PWG_MATH_F32) {
        PWGD_SHAPE(PK_PWG_MATH_F32)
    } else {
        PWGD_SHAPE(PK_PWG_MATH_F16X3)
    }
#undef PWGD_SHAPE
#undef PWGD_GO
    return PK_OK;
}

// lens | tile0 | tile_b and woff of one call onto the device; -> tiles, samples
static int pwgd_tables(pk_pwgd* h, const char* who, const int32_t* lens, int B, int& tiles, long& sumS) {
    pk_ctx* ctx = h->ctx;
    std::vector<long> woff(B);
    std::vector<int> itab(lens, lens + B);
    sumS = 0;
    long nt = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "%s: utterance %d is empty", who, b);
        woff[b] = sumS;
        sumS += lens[b];
        itab.push_back((int)nt);
        nt += (lens[b] + h->tile - 1) / h->tile;
        if (sumS > 0x3fffffffL) PK_FAIL(PK_EUNSUPPORTED, "%s: more than 2^30 samples in one call", who);
    }
    itab.push_back((int)nt);
    for (int b = 0; b < B; ++b) itab.insert(itab.end(), (size_t)(itab[B + b + 1] - itab[B + b]), b);
    tiles = (int)nt;
    PK_TRY(h->ws_itab.reserve(itab.size() * sizeof(int)));
    PK_TRY(h->ws_ltab.reserve(woff.size() * sizeof(long)));
    PK_HIP(hipMemcpyAsync(h->ws_itab.p, itab.data(), itab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->ws_ltab.p, woff.data(), woff.size() * sizeof(long), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));   // the host tables go out of scope
    if (h->keep_input) {
        h->last_lens.assign(lens, lens + B);
        h->last_woff = woff;
    }
    return PK_OK;
}

extern "C" int pk_pwgd_run(pk_pwgd* h, const float* wav, const int32_t* lens, int32_t B, float* logits_out,
                           double* sums_out, int32_t flags) {
    if (!h || !wav || !lens) PK_FAIL(PK_EINVAL, "pk_pwgd_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pwgd_run: batch size must be positive");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_pwgd_run: call pk_pwgd_finalize first");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    int tiles = 0;
    long sumS = 0;
    try {
        PK_TRY(pwgd_tables(h, "pk_pwgd_run", lens, B, tiles, sumS));
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_pwgd_run: host tables: %s", e.what());
    }
    const bool host = (flags & PK_HOST_IO) != 0;
    const float* d_wav = wav;
    float* d_logits = logits_out;
    double* d_sums = sums_out;
    if (host) {
        PK_TRY(h->ws_wav.reserve((size_t)sumS * 4));
        PK_HIP(hipMemcpyAsync(h->ws_wav.p, wav, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
        d_wav = h->ws_wav.as<float>();
        if (logits_out) {
            PK_TRY(h->ws_logits.reserve((size_t)sumS * 4));
            d_logits = h->ws_logits.as<float>();
        }
        if (sums_out) {
            PK_TRY(h->ws_out.reserve((size_t)B * 2 * sizeof(double)));
            d_sums = h->ws_out.as<double>();
        }
    }
    if (h->keep_input) {
        PK_TRY(h->last_wav.reserve((size_t)sumS * 4));
        PK_HIP(hipMemcpyAsync(h->last_wav.p, d_wav, (size_t)sumS * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    float* d_part = nullptr;
    if (sums_out) {
        PK_TRY(h->ws_part.reserve((size_t)tiles * 2 * 4));
        d_part = h->ws_part.as<float>();
    }
    PK_TRY(pwgd_launch(h, d_wav, B, tiles, d_logits, d_part, -1, nullptr));
    if (sums_out)
        PK_LAUNCH(ctx, "pwgd_fold", k_pwgd_fold, dim3(B), dim3(256), 0, d_part, h->ws_itab.as<int>() + B, d_sums);
    if (host) {
        if (logits_out) PK_HIP(hipMemcpyAsync(logits_out, d_logits, (size_t)sumS * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (sums_out)
            PK_HIP(hipMemcpyAsync(sums_out, d_sums, (size_t)B * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_pwgd_debug_read(pk_pwgd* h, int32_t layer, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_pwgd_debug_read: NULL argument");
    if (h->last_lens.empty()) PK_FAIL(PK_ESTATE, "pk_pwgd_debug_read: no run since pk_pwgd_set_debug(h, 1)");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_pwgd_debug_read: the parameters changed since the last run");
    if (b < 0 || b >= (int)h->last_lens.size()) PK_FAIL(PK_EINVAL, "pk_pwgd_debug_read: utterance out of range");
    if (layer < 0 || layer >= h->cfg.layers - 1)
        PK_FAIL(PK_EINVAL, "pk_pwgd_debug_read: block %d out of range (the model has %d)", layer, h->cfg.layers - 1);
    const int len = h->last_lens[b], C = h->cfg.conv_channels;
    if (n_floats != (int64_t)C * len) PK_FAIL(PK_ESHAPE, "pk_pwgd_debug_read: expected %ld floats", (long)C * len);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    // the same kernel over this utterance alone (its windows are those of the batch), block `layer` stored on the way
    const float* d_wav = h->last_wav.as<float>() + h->last_woff[b];
    const std::vector<int> keep_lens = h->last_lens;
    const std::vector<long> keep_woff = h->last_woff;
    int tiles = 0;
    long sumS = 0;
    const int32_t one = len;
    int st;
    try {
        st = pwgd_tables(h, "pk_pwgd_debug_read", &one, 1, tiles, sumS);
    } catch (const std::exception& e) {
        pk_set_error("pk_pwgd_debug_read: host tables: %s", e.what());
        st = PK_ENOMEM;
    }
    h->last_lens = keep_lens;
    h->last_woff = keep_woff;
    PK_TRY(st);
    PK_TRY(h->ws_dbg.reserve((size_t)C * len * 4));
    PK_TRY(pwgd_launch(h, d_wav, 1, tiles, nullptr, nullptr, layer, h->ws_dbg.as<float>()));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    PK_HIP(hipMemcpy(host_out, h->ws_dbg.p, (size_t)C * len * 4, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" void pk_pwgd_destroy(pk_pwgd* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->d_w0, &h->d_bias, &h->d_wf32, &h->d_wf16, &h->d_wlast, &h->ws_itab, &h->ws_ltab, &h->ws_wav,
                       &h->ws_logits, &h->ws_part, &h->ws_out, &h->ws_dbg, &h->last_wav};
    for (auto* b : bufs) b->release();
    delete h;
}
