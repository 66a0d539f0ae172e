// hifigan.hip -- the HiFi-GAN generator (Kong et al. 2020) on gfx950: every convolution of the stack on one MFMA kernel.
//
// Structure (restated from the paper with the module layout of the usual HiFiGANGenerator; include/pk_synth.h has the
// parameter names): input_conv, then per stage a transposed convolution (stride s, kernel 2 s) and nb residual blocks whose
// outputs are averaged, then LeakyReLU(0.01), output_conv and tanh.  Every convolution zero-pads its own input at the two
// ends of the utterance.
//
// k_hfg_conv: out[co, t] = epi(bias[co] + sum_(tap, ci) W[co, ci, tap] * leaky_s(in[ci, t + t0 + tap * step])).  One workgroup
// takes HFG_TILE positions of one utterance (tiles start at utterance-relative multiples of the tile) and 32 * CT output
// channels.  The input window (tile + 2 * halo) is staged in LDS slab by slab of 32 input channels, [position][channel]:
// LeakyReLU is applied and the value split into its fp16 pair ONCE there, so a tap's B operand is one 16-byte LDS read and
// nothing is split inside the k-loop.  Positions outside the utterance and channels past C_in are written as 0
// by a select: LDS never holds an undefined value.  The weights are the A operand, packed as fragments at finalize and read
// through the caches; each of the four waves owns two 32-position tiles per fragment.
//   The transposed convolution runs on the same kernel in its phase-major form: with p = s / 2 + s % 2, k0 = (n + p) mod s,
//   m0 = (n + p - k0) / s:  y[:, n] = b + W[:, :, k0]^T x[:, m0] + W[:, :, k0 + s]^T x[:, m0 - 1]; blockIdx.z is the phase k0,
//   a two-tap convolution over input positions whose outputs land s apart.
// Epilogues (wave-uniform switch): store; + residual; + residual, then into the stage's block sum scaled by 1 / nb; tanh.
//
// Math: PK_PWG_MATH_F32 on v_mfma_f32_32x32x2_f32; PK_PWG_MATH_F16X3 (default) as a_hi*b_hi + a_lo*b_hi +
// a_hi*b_lo on v_mfma_f32_32x32x16_f16 with block-scaled operands: the weights one exponent per tensor, the activations one
// exponent per UTTERANCE and layer input, measured by the producer of that input (every workgroup writes the maximum of what
// it stored, the consumer takes the maximum over its utterance's slots) -- no a-priori bound, no guard, no atomics.  It is
// the maximum BEFORE the consumer's LeakyReLU, times max(1, |slope|): never less than the staged values'.
//
// Plain launches only: no grid barrier, no persistent loop, no spinning.  An utterance's samples are the same bits alone, in
// any batch and at any position in it: nothing a workgroup computes depends on another utterance.
#include <cmath>
#include <exception>
#include <string>
#include <vector>

#include "pk_common.h"
#include "pk_hifigan.h"
#include "pk_mfma.h"

namespace {

enum { HFG_EPI_STORE = 0, HFG_EPI_RES = 1, HFG_EPI_SUM = 2, HFG_EPI_TANH = 3 };

struct hfg_conv_args {
    const float* in;         // (C_in, len) per utterance, or (len, C_in) with in_pc
    float* out;              // (C_out, len * ostride) per utterance
    const float* res;        // residual, laid out as out (HFG_EPI_RES / HFG_EPI_SUM)
    const float* bias;       // [32 * CTtot], zero past C_out
    const float* wf32;       // [phase][tap][Cinp / 8][CTtot][64] float4 fragments
    const f16x8* wf16;       // [phase][tap][Cinp / 16][CTtot][hi, lo][64] fragments of 2^kw * W
    long ps32, ps16;         // fragments (float4 / f16x8) of one phase
    const int* lens;         // the input rate's tables: [B] positions of an utterance
    const long* offs;        // [B] positions before it
    const int* tile0;        // [B + 1] first tile
    const int* tile_b;       // [tiles] utterance of a tile
    const float* amax_in;    // maxima written by the input's producer: [producer tile][nsl_in]
    const int* atile0;       // [B + 1] the producer's first tile of an utterance
    float* amax_out;         // [tile][gridDim.y * gridDim.z], or NULL
    int nsl_in;
    int Cin, Cinp, Cout, CTtot;
    int ntaps, t0, step, halo;
    int in_pc;
    int transposed, s, pad;  // phase-major transposed convolution: stride, p
    int mode, first;
    float inv_nb, slope, amax_mul;
    int kw;
};

template <int MATH, int CT>
__global__ __launch_bounds__(HFG_THREADS) void k_hfg_conv(const hfg_conv_args a) {
    constexpr int PT = 2;
    constexpr int LDS_BYTES = MATH == PK_PWG_MATH_F32 ? HFG_LDS_F32 : HFG_LDS_F16;
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int tb = blockIdx.x, b = a.tile_b[tb], len = a.lens[b];
    const long off = a.offs[b];
    const int tile = tb - a.tile0[b];
    const int halo = a.halo, W = HFG_TILE + 2 * halo;
    const int g0 = tile * HFG_TILE - halo;   // utterance-relative position of window index 0
    int t0 = a.t0, ooff = 0, ostride = 1;
    if (a.transposed) {
        const int k0 = blockIdx.z;
        ostride = a.s;
        t0 = k0 < a.pad ? 1 : 0;
        ooff = k0 < a.pad ? k0 - a.pad + a.s : k0 - a.pad;
    }
    const float* in = a.in + off * a.Cin;
    const float slope = a.slope;

    float sc = 1.f, unscale = 1.f;
    if (MATH == PK_PWG_MATH_F16X3) {
        const long s0 = (long)a.atile0[b] * a.nsl_in;
        const int n = (a.atile0[b + 1] - a.atile0[b]) * a.nsl_in;
        float m = 0.f;
        for (int i = tid; i < n; i += HFG_THREADS) m = fmaxf(m, a.amax_in[s0 + i]);
        m = wave_max64(m);
        if (lane == 0) s_red[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) * a.amax_mul;
        const int kx = blk_scale_exp(__float_as_uint(m));
        sc = pow2f(kx);
        unscale = pow2f(-kx - a.kw);
    }

    f32x16 acc[PT][CT];
#pragma unroll
    for (int pi = 0; pi < PT; ++pi)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pi][ct][r] = 0.f;

    const int nKB = a.Cinp / 16, ct0 = blockIdx.y * CT;
    const int nslab = (a.Cinp + HFG_SLAB - 1) / HFG_SLAB;
    for (int sl = 0; sl < nslab; ++sl) {
        const int c0 = sl * HFG_SLAB;
        const int nkb = (a.Cinp - c0) >= HFG_SLAB ? 2 : 1;
        __syncthreads();   // the previous slab's reads (and those of s_red) are done
        // ---- stage the slab: LeakyReLU, the select, the split -- once per value
        const int ng = 2 * nkb;
        for (int it = tid; it < W * ng; it += HFG_THREADS) {
            const int g8 = it / W, p = it - g8 * W;   // consecutive threads take consecutive positions
            const int g = g0 + p;
            const bool okp = (unsigned)g < (unsigned)len;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c0 + g8 * 8 + e;
                float x = 0.f;
                if (okp && c < a.Cin) x = a.in_pc ? in[(long)g * a.Cin + c] : in[(long)c * len + g];
                v[e] = x > 0.f ? x : x * slope;
            }
            if (MATH == PK_PWG_MATH_F16X3) {
                f16x8 h, l;
                store_pair8(v, sc, h, l);
                st_h8(lds + p * HFG_ROW16 + g8 * 16, h);
                st_h8(lds + HFG_PLANE16 + p * HFG_ROW16 + g8 * 16, l);
            } else {
                f32x4* d = reinterpret_cast<f32x4*>(lds + p * HFG_ROW32 + g8 * 32);
                d[0] = f32x4{v[0], v[1], v[2], v[3]};
                d[1] = f32x4{v[4], v[5], v[6], v[7]};
            }
        }
        __syncthreads();
        // ---- the taps of this slab
        for (int t = 0; t < a.ntaps; ++t) {
            int q[PT];
#pragma unroll
            for (int pi = 0; pi < PT; ++pi) q[pi] = (wave * PT + pi) * 32 + l31 + halo + t0 + t * a.step;   // in [0, W)
            if (MATH == PK_PWG_MATH_F16X3) {
                const f16x8* wl = a.wf16 + (long)blockIdx.z * a.ps16 + lane;
                for (int kb = 0; kb < nkb; ++kb) {
                    f16x8 bh[PT], bl[PT];
#pragma unroll
                    for (int pi = 0; pi < PT; ++pi) {
                        const char* src = lds + q[pi] * HFG_ROW16 + kb * 32 + hi * 16;
                        bh[pi] = ld_h8(src);
                        bl[pi] = ld_h8(src + HFG_PLANE16);
                    }
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const f16x8* wp = wl + ((long)(t * nKB + c0 / 16 + kb) * a.CTtot + ct0 + ct) * 2 * 64;
                        const f16x8 ah = wp[0], al = wp[64];
#pragma unroll
                        for (int pi = 0; pi < PT; ++pi) {
                            acc[pi][ct] = mfma16(ah, bh[pi], acc[pi][ct]);
                            acc[pi][ct] = mfma16(al, bh[pi], acc[pi][ct]);
                            acc[pi][ct] = mfma16(ah, bl[pi], acc[pi][ct]);
                        }
                    }
                }
            } else {
                const f32x4* wl = reinterpret_cast<const f32x4*>(a.wf32) + (long)blockIdx.z * a.ps32 + lane;
                for (int k8 = 0; k8 < 2 * nkb; ++k8) {
                    f32x4 bv[PT];
#pragma unroll
                    for (int pi = 0; pi < PT; ++pi)
                        bv[pi] = *reinterpret_cast<const f32x4*>(lds + q[pi] * HFG_ROW32 + k8 * 32 + hi * 16);
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const f32x4 av = wl[((long)(t * 2 * nKB + c0 / 8 + k8) * a.CTtot + ct0 + ct) * 64];
#pragma unroll
                        for (int pi = 0; pi < PT; ++pi)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[pi][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[pi][e], acc[pi][ct], 0, 0, 0);
                    }
                }
            }
        }
    }

    // ---- epilogue: unscale, bias, the switch, the store, the maximum for the next consumer
    const int olen = len * ostride;
    float* out = a.out + off * ostride * a.Cout;
    const float* res = a.res ? a.res + off * ostride * a.Cout : nullptr;
    const int mode = a.mode;
    float m = 0.f;
#pragma unroll
    for (int pi = 0; pi < PT; ++pi) {
        const int g = tile * HFG_TILE + (wave * PT + pi) * 32 + l31;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (ct0 + ct) * 32 + mfma_row(r, hi);
                if (g < len && co < a.Cout) {
                    float v = acc[pi][ct][r];
                    if (MATH == PK_PWG_MATH_F16X3) v *= unscale;
                    v += a.bias[co];
                    const long o = (long)co * olen + (long)g * ostride + ooff;
                    if (mode == HFG_EPI_RES || mode == HFG_EPI_SUM) v += res[o];
                    if (mode == HFG_EPI_SUM) {
                        v *= a.inv_nb;
                        if (!a.first) v += out[o];
                    }
                    if (mode == HFG_EPI_TANH) v = tanhf(v);
                    out[o] = v;
                    m = fmaxf(m, fabsf(v));
                }
            }
    }
    if (a.amax_out) {
        m = wave_max64(m);
        __syncthreads();
        if (lane == 0) s_red[wave] = m;
        __syncthreads();
        if (tid == 0)
            a.amax_out[((long)tb * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z] =
                fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    }
}

// The mel on its way in: (optionally) the normaliser, a copy into the workspace in the caller's (frames, C) layout, and the
// maximum of a tile of 256 frames for input_conv's scale.
__global__ __launch_bounds__(HFG_THREADS) void k_hfg_prep(const float* __restrict__ mel, float* __restrict__ out,
                                                          const float* __restrict__ mu, const float* __restrict__ sigma,
                                                          int use_norm, const int* __restrict__ lens,
                                                          const long* __restrict__ offs, const int* __restrict__ tile0,
                                                          const int* __restrict__ tile_b, int C, float* __restrict__ amax) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = blockIdx.x, b = tile_b[tb], len = lens[b];
    const int r0 = (tb - tile0[b]) * HFG_TILE, rows = min(HFG_TILE, len - r0);
    const long base = (offs[b] + r0) * C;
    float m = 0.f;
    for (int i = tid; i < rows * C; i += HFG_THREADS) {
        float v = mel[base + i];
        if (use_norm) {
            const int c = i % C;
            v = (v - mu[c]) / sigma[c];
        }
        out[base + i] = v;
        m = fmaxf(m, fabsf(v));
    }
    m = wave_max64(m);
    if (lane == 0) s_red[wave] = m;
    __syncthreads();
    if (tid == 0) amax[tb] = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// one convolution of the stack as finalize packs it
struct hfg_conv {
    std::string name;
    int Cin = 0, Cinp = 0, Cout = 0, CTtot = 0, CT = 1;
    int k = 0, dil = 1;           // kernel and dilation; the transposed one: k = 2 s
    bool transposed = false;
    int s = 1;
    int kw = 0;
    size_t o32 = 0, o16 = 0, obias = 0;   // offsets into the handle's fragment / bias arrays (float4, f16x8, float)
    size_t ps32 = 0, ps16 = 0;
};

struct hfg_act {
    float* p = nullptr;
    float* amax = nullptr;
    int nsl = 1;
    int grate = 0;    // the rate whose tiles the producer's grid was laid over
};

}  // namespace

struct pk_hfg {
    pk_ctx* ctx = nullptr;
    pk_hfg_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int math = PK_PWG_MATH_F16X3;
    int hop = 1;
    bool use_norm = false;
    std::vector<hfg_conv> convs;   // input_conv | per stage: upsample, then blocks x dilations x (convs1[, convs2]) | output_conv
    pk_dbuf d_w32, d_w16, d_bias, d_mu, d_sigma;
    pk_dbuf ws_itab, ws_ltab, ws_mel, ws_act, ws_amax, ws_wav, ws_hostmel;
    // pinned staging of a call's tables (int part, then the long part) and the event after their copies: the upload does not
    // block the host, and the next call waits for this event alone before it overwrites the staging
    void* stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t stage_done = nullptr;
    bool stage_busy = false;
    int max_slots = 1;   // the most maxima one tile's producers write (output-channel groups x phases), over the model's convolutions
    // tables of the running call (offsets into ws_itab / ws_ltab per rate)
    std::vector<size_t> o_lens, o_tile0, o_tileb, o_offs;
    std::vector<int> ntiles;
    std::vector<long> sumL;
    // the last call, for pk_hfg_debug_read
    std::vector<int> last_frames;
    std::vector<long> last_off;
    bool last_valid = false;
    // pk_hfg_debug_conv: stop after launch dbg_stop (-1: never); what it wrote
    int dbg_stop = -1, dbg_count = 0, dbg_C = 0, dbg_rate = 0;
    const float* dbg_ptr = nullptr;
};

static int hfg_ch(const pk_hfg_cfg& c, int i) { return c.channels >> i; }

extern "C" int pk_hfg_create(pk_ctx* ctx, const pk_hfg_cfg* cfg, pk_hfg** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_hfg_create: NULL argument");
    *out = nullptr;
    const pk_hfg_cfg& c = *cfg;
    if (c.in_channels < 1 || c.in_channels > 512 || c.out_channels != 1)
        PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: in_channels must be 1 ... 512 and out_channels 1 (got %d, %d)", c.in_channels,
                c.out_channels);
    if (c.kernel_size < 3 || c.kernel_size > 11 || c.kernel_size % 2 == 0)
        PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: kernel_size must be odd, 3 ... 11 (got %d)", c.kernel_size);
    if (c.n_upsample < 1 || c.n_upsample > PK_HFG_MAX_STAGES)
        PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: 1 ... %d upsample stages (got %d)", PK_HFG_MAX_STAGES, c.n_upsample);
    long hop = 1;
    for (int i = 0; i < c.n_upsample; ++i) {
        const int s = c.upsample_scales[i];
        if (s < 2 || s > 16) PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: upsample_scales must be 2 ... 16 (got %d)", s);
        if (c.upsample_kernel_sizes[i] != 2 * s)
            PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: upsample_kernel_sizes[%d] must be 2 * upsample_scales[%d] = %d (got %d): "
                    "only then is a stage's length exactly scale times its input's", i, i, 2 * s, c.upsample_kernel_sizes[i]);
        hop *= s;
    }
    if (hop < 4 || hop > 1024) PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: the hop (product of the scales) must be 4 ... 1024 (got %ld)", hop);
    if (c.channels < 8 || c.channels > 512 || c.channels % (1 << c.n_upsample) != 0)
        PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: channels must be 8 ... 512 and halve exactly at every stage (got %d)", c.channels);
    for (int i = 0; i <= c.n_upsample; ++i)
        if (hfg_ch(c, i) < 8 || hfg_ch(c, i) % 8 != 0)
            PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: channels >> %d = %d must be a multiple of 8 in 8 ... 512", i, hfg_ch(c, i));
    if (c.n_blocks < 1 || c.n_blocks > PK_HFG_MAX_BLOCKS)
        PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: 1 ... %d residual blocks per stage (got %d)", PK_HFG_MAX_BLOCKS, c.n_blocks);
    for (int j = 0; j < c.n_blocks; ++j) {
        const int k = c.resblock_kernel_sizes[j];
        if (k < 3 || k > 11 || k % 2 == 0)
            PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: resblock_kernel_sizes must be odd, 3 ... 11 (got %d)", k);
        if (c.n_dilations[j] < 1 || c.n_dilations[j] > PK_HFG_MAX_DILS)
            PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: 1 ... %d dilations per residual block (got %d)", PK_HFG_MAX_DILS, c.n_dilations[j]);
        for (int n = 0; n < c.n_dilations[j]; ++n) {
            const int d = c.resblock_dilations[j][n];
            if (d < 1 || (k - 1) / 2 * d > HFG_MAX_HALO)
                PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator: (kernel - 1) / 2 * dilation must be 1 ... %d (kernel %d, dilation %d)",
                        HFG_MAX_HALO, k, d);
        }
    }
    if (!c.bias) PK_FAIL(PK_EUNSUPPORTED, "HiFiGANGenerator(bias=False) is not implemented");
    if (!std::isfinite(c.negative_slope)) PK_FAIL(PK_EINVAL, "HiFiGANGenerator: negative_slope is not finite");
    pk_hfg* h = new pk_hfg();
    h->ctx = ctx;
    h->cfg = c;
    h->hop = (int)hop;
    *out = h;
    return PK_OK;
}

extern "C" int pk_hfg_set_param(pk_hfg* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_hfg_set_param: handle is NULL");
    h->finalized = false;
    h->last_valid = false;
    return pk_store_param(h->params, name, data, shape, ndim);
}

extern "C" int pk_hfg_set_math(pk_hfg* h, int32_t mode) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_hfg_set_math: handle is NULL");
    if (mode == PK_PWG_MATH_BF16X3) PK_FAIL(PK_EUNSUPPORTED, "pk_hfg_set_math: the HiFi-GAN generator has no split-bf16 variant");
    if (mode != PK_PWG_MATH_F32 && mode != PK_PWG_MATH_F16X3) PK_FAIL(PK_EINVAL, "pk_hfg_set_math: unknown mode %d", mode);
    h->math = mode;
    return PK_OK;
}

extern "C" int pk_hfg_set_normalizer(pk_hfg* h, const float* mu, const float* sigma, int32_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_hfg_set_normalizer: handle is NULL");
    if (!mu && !sigma) {
        h->use_norm = false;
        return PK_OK;
    }
    if (!mu || !sigma || n != h->cfg.in_channels)
        PK_FAIL(PK_ESHAPE, "normalizer needs mu and sigma of %d elements", h->cfg.in_channels);
    PK_DEVICE(h->ctx->device);
    PK_TRY(pk_upload(h->ctx, h->d_mu, mu, n * sizeof(float)));
    PK_TRY(pk_upload(h->ctx, h->d_sigma, sigma, n * sizeof(float)));
    h->use_norm = true;
    return PK_OK;
}

// Fragments of one convolution: at(phase, co, ci, tap) is W in the kernel's orientation (zero past C_out / C_in).
template <class F>
static void hfg_pack(hfg_conv& cv, int phases, int ntaps, F at, std::vector<float>& f32, std::vector<uint16_t>& f16) {
    const int nKB = cv.Cinp / 16, CTt = cv.CTtot;
    cv.ps32 = (size_t)ntaps * 2 * nKB * CTt * 64;
    cv.ps16 = (size_t)ntaps * nKB * CTt * 2 * 64;
    cv.o32 = f32.size() / 4;
    cv.o16 = f16.size() / 8;
    f32.resize(f32.size() + cv.ps32 * phases * 4, 0.f);
    f16.resize(f16.size() + cv.ps16 * phases * 8, 0);
    for (int ph = 0; ph < phases; ++ph) {
        float* p32 = f32.data() + (cv.o32 + cv.ps32 * ph) * 4;
        uint16_t* p16 = f16.data() + (cv.o16 + cv.ps16 * ph) * 8;
        for (int t = 0; t < ntaps; ++t)
            for (int ct = 0; ct < CTt; ++ct)
                for (int lane = 0; lane < 64; ++lane) {
                    const int co = 32 * ct + (lane & 31), hi = lane >> 5;
                    for (int k8 = 0; k8 < 2 * nKB; ++k8)
                        for (int e = 0; e < 4; ++e)
                            p32[(((size_t)(t * 2 * nKB + k8) * CTt + ct) * 64 + lane) * 4 + e] = at(ph, co, 8 * k8 + 4 * hi + e, t);
                    for (int kb = 0; kb < nKB; ++kb)
                        for (int e = 0; e < 8; ++e) {
                            const float x = std::ldexp(at(ph, co, 16 * kb + 8 * hi + e, t), cv.kw);
                            const _Float16 xh = (_Float16)x, xl = (_Float16)(x - (float)xh);
                            const size_t o = ((((size_t)(t * nKB + kb) * CTt + ct) * 2) * 64 + lane) * 8 + e;
                            memcpy(&p16[o], &xh, 2);
                            memcpy(&p16[o + 512], &xl, 2);
                        }
                }
    }
}

static int hfg_finalize(pk_hfg* h) {
    pk_ctx* ctx = h->ctx;
    const pk_hfg_cfg& c = h->cfg;
    std::vector<float> f32, bias, w, bv;
    std::vector<uint16_t> f16;
    h->convs.clear();
    h->max_slots = 1;
    auto add = [&](const std::string& name, int Cin, int Cout, int k, int dil, bool transposed, int s) -> int {
        hfg_conv cv;
        cv.name = name;
        cv.Cin = Cin;
        cv.Cinp = (Cin + 15) / 16 * 16;
        cv.Cout = Cout;
        cv.CTtot = (Cout + 31) / 32;
        cv.CT = cv.CTtot % 4 == 0 ? 4 : (cv.CTtot % 2 == 0 ? 2 : 1);
        cv.k = k;
        cv.dil = dil;
        cv.transposed = transposed;
        cv.s = s;
        if (transposed) PK_TRY(pk_get_weight(h->params, name, {Cin, Cout, k}, w));
        else PK_TRY(pk_get_weight(h->params, name, {Cout, Cin, k}, w));
        PK_TRY(pk_get_vector(h->params, name + ".bias", Cout, bv));
        cv.kw = pk_weight_scale_exp(w.data(), w.size());
        cv.obias = bias.size();
        bias.resize(bias.size() + (size_t)32 * cv.CTtot, 0.f);
        for (int o = 0; o < Cout; ++o) bias[cv.obias + o] = bv[o];
        if (transposed)   // phase k0: taps k0 and k0 + s of W (C_in, C_out, 2 s)
            hfg_pack(cv, s, 2, [&](int ph, int co, int ci, int t) {
                return (co < Cout && ci < Cin) ? w[((size_t)ci * Cout + co) * k + ph + t * s] : 0.f; }, f32, f16);
        else
            hfg_pack(cv, 1, k, [&](int, int co, int ci, int t) {
                return (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * k + t] : 0.f; }, f32, f16);
        h->max_slots = std::max(h->max_slots, cv.CTtot / cv.CT * (transposed ? s : 1));
        h->convs.push_back(cv);
        return PK_OK;
    };
    PK_TRY(add("input_conv", c.in_channels, c.channels, c.kernel_size, 1, false, 1));
    for (int i = 0; i < c.n_upsample; ++i) {
        const int C = hfg_ch(c, i + 1);
        PK_TRY(add("upsamples." + std::to_string(i) + ".1", hfg_ch(c, i), C, 2 * c.upsample_scales[i], 1, true, c.upsample_scales[i]));
        for (int j = 0; j < c.n_blocks; ++j) {
            const std::string blk = "blocks." + std::to_string(i * c.n_blocks + j);
            for (int n = 0; n < c.n_dilations[j]; ++n) {
                PK_TRY(add(blk + ".convs1." + std::to_string(n) + ".1", C, C, c.resblock_kernel_sizes[j], c.resblock_dilations[j][n], false, 1));
                if (c.use_additional_convs)
                    PK_TRY(add(blk + ".convs2." + std::to_string(n) + ".1", C, C, c.resblock_kernel_sizes[j], 1, false, 1));
            }
        }
    }
    PK_TRY(add("output_conv.1", hfg_ch(c, c.n_upsample), 1, c.kernel_size, 1, false, 1));
    PK_TRY(pk_upload(ctx, h->d_w32, f32.data(), f32.size() * sizeof(float)));
    PK_TRY(pk_upload(ctx, h->d_w16, f16.data(), f16.size() * sizeof(uint16_t)));
    PK_TRY(pk_upload(ctx, h->d_bias, bias.data(), bias.size() * sizeof(float)));
    h->finalized = true;
    return PK_OK;
}

extern "C" int pk_hfg_finalize(pk_hfg* h) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_hfg_finalize: handle is NULL");
    PK_DEVICE(h->ctx->device);
    try {
        return hfg_finalize(h);
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_hfg_finalize: host tables: %s", e.what());
    }
}

// per rate r = 0 ... n_upsample: lens | tile0 | tile_b and offs of one call onto the device
static int hfg_tables(pk_hfg* h, const char* who, const int32_t* frames, int B) {
    pk_ctx* ctx = h->ctx;
    const pk_hfg_cfg& c = h->cfg;
    const int R = c.n_upsample + 1;
    std::vector<int> itab;
    std::vector<long> ltab;
    h->o_lens.assign(R, 0);
    h->o_tile0.assign(R, 0);
    h->o_tileb.assign(R, 0);
    h->o_offs.assign(R, 0);
    h->ntiles.assign(R, 0);
    h->sumL.assign(R, 0);
    long mul = 1;
    for (int r = 0; r < R; ++r) {
        if (r) mul *= c.upsample_scales[r - 1];
        h->o_lens[r] = itab.size();
        h->o_offs[r] = ltab.size();
        long sum = 0;
        for (int b = 0; b < B; ++b) {
            if (frames[b] < 1) PK_FAIL(PK_EINVAL, "%s: utterance %d has no frames", who, b);
            itab.push_back((int)(frames[b] * mul));
            ltab.push_back(sum);
            sum += frames[b] * mul;
            if (sum > 0x3fffffffL) PK_FAIL(PK_EUNSUPPORTED, "%s: more than 2^30 samples in one call", who);
        }
        h->sumL[r] = sum;
        h->o_tile0[r] = itab.size();
        long nt = 0;
        for (int b = 0; b < B; ++b) {
            itab.push_back((int)nt);
            nt += (frames[b] * mul + HFG_TILE - 1) / HFG_TILE;
        }
        itab.push_back((int)nt);
        h->o_tileb[r] = itab.size();
        for (int b = 0; b < B; ++b)
            itab.insert(itab.end(), (size_t)(itab[h->o_tile0[r] + b + 1] - itab[h->o_tile0[r] + b]), b);
        h->ntiles[r] = (int)nt;
    }
    PK_TRY(h->ws_itab.reserve(itab.size() * sizeof(int)));
    PK_TRY(h->ws_ltab.reserve(ltab.size() * sizeof(long)));
    // through the pinned staging: work queued before this call keeps running while the launches are issued
    const size_t ibytes = (itab.size() * sizeof(int) + 15) / 16 * 16, lbytes = ltab.size() * sizeof(long);
    if (h->stage_busy) {
        PK_HIP(hipEventSynchronize(h->stage_done));   // the previous call's copies have read the staging
        h->stage_busy = false;
    }
    if (ibytes + lbytes > h->stage_cap) {
        if (h->stage) PK_HIP(hipHostFree(h->stage));
        h->stage = nullptr;
        h->stage_cap = 0;
        const size_t want = (ibytes + lbytes) * 2 + 4096;
        PK_HIP(hipHostMalloc(&h->stage, want, hipHostMallocDefault));
        h->stage_cap = want;
    }
    if (!h->stage_done) PK_HIP(hipEventCreateWithFlags(&h->stage_done, hipEventDisableTiming));
    memcpy(h->stage, itab.data(), itab.size() * sizeof(int));
    memcpy((char*)h->stage + ibytes, ltab.data(), lbytes);
    PK_HIP(hipMemcpyAsync(h->ws_itab.p, h->stage, itab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->ws_ltab.p, (char*)h->stage + ibytes, lbytes, hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipEventRecord(h->stage_done, ctx->stream));
    h->stage_busy = true;
    return PK_OK;
}

// one convolution: `in` at rate r -> `out` (rate r, or r + 1 for the transposed one)
static int hfg_launch(pk_hfg* h, const hfg_conv& cv, int r, const hfg_act& in, hfg_act& out, const float* res, int mode,
                      int first, float inv_nb, float slope, int in_pc, bool want_amax) {
    pk_ctx* ctx = h->ctx;
    const int* itab = h->ws_itab.as<int>();
    hfg_conv_args a;
    a.in = in.p;
    a.out = out.p;
    a.res = res;
    a.bias = h->d_bias.as<float>() + cv.obias;
    a.wf32 = h->d_w32.as<float>() + cv.o32 * 4;
    a.wf16 = h->d_w16.as<f16x8>() + cv.o16;
    a.ps32 = (long)cv.ps32;
    a.ps16 = (long)cv.ps16;
    a.lens = itab + h->o_lens[r];
    a.offs = h->ws_ltab.as<long>() + h->o_offs[r];
    a.tile0 = itab + h->o_tile0[r];
    a.tile_b = itab + h->o_tileb[r];
    a.amax_in = in.amax;
    a.atile0 = itab + h->o_tile0[in.grate];
    a.nsl_in = in.nsl;
    a.Cin = cv.Cin;
    a.Cinp = cv.Cinp;
    a.Cout = cv.Cout;
    a.CTtot = cv.CTtot;
    a.in_pc = in_pc;
    a.transposed = cv.transposed ? 1 : 0;
    a.s = cv.s;
    a.pad = cv.s / 2 + cv.s % 2;
    if (cv.transposed) {
        a.ntaps = 2;
        a.t0 = 0;
        a.step = -1;
        a.halo = 1;
    } else {
        a.ntaps = cv.k;
        a.t0 = -(cv.k - 1) / 2 * cv.dil;
        a.step = cv.dil;
        a.halo = (cv.k - 1) / 2 * cv.dil;
    }
    a.mode = mode;
    a.first = first;
    a.inv_nb = inv_nb;
    a.slope = slope;
    a.amax_mul = std::fmax(1.f, std::fabs(slope));
    a.kw = cv.kw;
    const dim3 grid(h->ntiles[r], cv.CTtot / cv.CT, cv.transposed ? cv.s : 1), block(HFG_THREADS);
    a.amax_out = want_amax ? out.amax : nullptr;
    if (want_amax) {
        out.nsl = grid.y * grid.z;
        out.grate = r;
    }
#define HFG_GO(M, CTV) PK_LAUNCH(ctx, "hfg_conv", (k_hfg_conv<M, CTV>), grid, block, 0, a)
#define HFG_SHAPE(M)                 \
    switch (cv.CT) {                 \
        case 1: HFG_GO(M, 1); break; \
        case 2: HFG_GO(M, 2); break; \
        default: HFG_GO(M, 4); break; \
    }
    if (h->math == PK_PWG_MATH_F32) {
        HFG_SHAPE(PK_PWG_MATH_F32)
    } else {
        HFG_SHAPE(PK_PWG_MATH_F16X3)
    }
#undef HFG_SHAPE
#undef HFG_GO
    if (h->dbg_count++ == h->dbg_stop) {
        h->dbg_ptr = out.p;
        h->dbg_C = cv.Cout;
        h->dbg_rate = cv.transposed ? r + 1 : r;
    }
    return PK_OK;
}

// The stack over the call whose tables are on the device, from the prepared mel `d_mel` (its tile maxima in d_mel_amax).
// upto < 0: through tanh into d_wav; else stop after stage `upto` and return its output buffer in *stage_out.
#define HFG_STEP(call)                    \
    do {                                  \
        PK_TRY(call);                     \
        if (h->dbg_ptr) return PK_OK;     \
    } while (0)
static int hfg_chain(pk_hfg* h, const float* d_mel, float* d_mel_amax, float* d_wav, int upto, const float** stage_out) {
    const pk_hfg_cfg& c = h->cfg;
    const int S = c.n_upsample;
    size_t maxsz = (size_t)c.channels * h->sumL[0];
    for (int i = 0; i < S; ++i) maxsz = std::max(maxsz, (size_t)hfg_ch(c, i + 1) * h->sumL[i + 1]);
    maxsz = (maxsz + 63) / 64 * 64;
    if ((long)(maxsz * 5 * sizeof(float)) > HFG_WORKSPACE_CAP)
        PK_FAIL(PK_ENOMEM, "pk_hfg_infer: the call needs %zu MiB of activations, more than the %ld MiB a call may take: split the batch",
                maxsz * 5 * sizeof(float) >> 20, HFG_WORKSPACE_CAP >> 20);
    const size_t asz = (size_t)h->ntiles[S] * h->max_slots;   // a producer's grid has at most the last rate's tiles
    PK_TRY(h->ws_act.reserve(maxsz * 5 * sizeof(float)));
    PK_TRY(h->ws_amax.reserve(asz * 5 * sizeof(float)));
    hfg_act buf[5];
    for (int i = 0; i < 5; ++i) {
        buf[i].p = h->ws_act.as<float>() + maxsz * i;
        buf[i].amax = h->ws_amax.as<float>() + asz * i;
    }
    hfg_act *P = &buf[0], *X = &buf[1], *Y = &buf[2], *T = &buf[3], *Sm = &buf[4];
    hfg_act mel;
    mel.p = const_cast<float*>(d_mel);
    mel.amax = d_mel_amax;
    mel.nsl = 1;
    mel.grate = 0;
    const float slope = c.negative_slope;
    size_t ci = 0;
    h->dbg_count = 0;
    h->dbg_ptr = nullptr;
    HFG_STEP(hfg_launch(h, h->convs[ci++], 0, mel, *P, nullptr, HFG_EPI_STORE, 0, 1.f, 1.f, 1, true));
    for (int i = 0; i < S; ++i) {
        const int r = i + 1;
        HFG_STEP(hfg_launch(h, h->convs[ci++], i, *P, *X, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
        const float inv_nb = 1.f / (float)c.n_blocks;
        for (int j = 0; j < c.n_blocks; ++j) {
            hfg_act* cur = X;
            const int nd = c.n_dilations[j];
            for (int n = 0; n < nd; ++n) {
                const bool last = n == nd - 1, fin = last && j == c.n_blocks - 1;
                if (c.use_additional_convs) {
                    HFG_STEP(hfg_launch(h, h->convs[ci++], r, *cur, *T, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
                    hfg_act* dst = last ? Sm : Y;   // Y in place when cur is Y: a thread reads res[o], then writes out[o]
                    HFG_STEP(hfg_launch(h, h->convs[ci++], r, *T, *dst, cur->p, last ? HFG_EPI_SUM : HFG_EPI_RES, j == 0, inv_nb,
                                      slope, 0, last ? fin : true));
                    cur = Y;
                } else {
                    hfg_act* dst = last ? Sm : (cur == Y ? T : Y);
                    HFG_STEP(hfg_launch(h, h->convs[ci++], r, *cur, *dst, cur->p, last ? HFG_EPI_SUM : HFG_EPI_RES, j == 0, inv_nb,
                                      slope, 0, last ? fin : true));
                    cur = dst;
                }
            }
        }
        std::swap(P, Sm);   // the block mean is the next stage's input
        if (upto == i) {
            *stage_out = P->p;
            return PK_OK;
        }
    }
    hfg_act wav;
    wav.p = d_wav;
    HFG_STEP(hfg_launch(h, h->convs[ci++], S, *P, wav, nullptr, HFG_EPI_TANH, 0, 1.f, HFG_OUTPUT_SLOPE, 0, false));
    return PK_OK;
}

#undef HFG_STEP

extern "C" int pk_hfg_infer(pk_hfg* h, const float* mel, const int32_t* frames, int32_t B, float* wav_out, int32_t flags) {
    if (!h || !mel || !frames || !wav_out) PK_FAIL(PK_EINVAL, "pk_hfg_infer: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_hfg_infer: batch size must be positive");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_hfg_infer: call pk_hfg_finalize first");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    h->last_valid = false;
    try {
        PK_TRY(hfg_tables(h, "pk_hfg_infer", frames, B));
        h->last_frames.assign(frames, frames + B);
        h->last_off.assign(B, 0);
        for (int b = 1; b < B; ++b) h->last_off[b] = h->last_off[b - 1] + frames[b - 1];
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_hfg_infer: host tables: %s", e.what());
    }
    const pk_hfg_cfg& c = h->cfg;
    const int S = c.n_upsample;
    const bool host = (flags & PK_HOST_IO) != 0;
    const size_t nmel = (size_t)h->sumL[0] * c.in_channels, nwav = (size_t)h->sumL[S];
    const float* d_in = mel;
    float* d_wav = wav_out;
    if (host) {
        PK_TRY(h->ws_hostmel.reserve(nmel * 4));
        PK_HIP(hipMemcpyAsync(h->ws_hostmel.p, mel, nmel * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = h->ws_hostmel.as<float>();
        PK_TRY(h->ws_wav.reserve(nwav * 4));
        d_wav = h->ws_wav.as<float>();
    }
    // the prepared mel and its tile maxima stay in the handle for pk_hfg_debug_read
    PK_TRY(h->ws_mel.reserve((nmel + (size_t)h->ntiles[0] + 64) * 4));
    float* d_mel = h->ws_mel.as<float>();
    float* d_mel_amax = d_mel + (nmel + 63) / 64 * 64;
    const int* itab = h->ws_itab.as<int>();
    PK_LAUNCH(ctx, "hfg_prep", k_hfg_prep, dim3(h->ntiles[0]), dim3(HFG_THREADS), 0, d_in, d_mel, h->d_mu.as<float>(),
              h->d_sigma.as<float>(), (h->use_norm && (flags & PK_APPLY_NORMALIZER)) ? 1 : 0, itab + h->o_lens[0],
              h->ws_ltab.as<long>() + h->o_offs[0], itab + h->o_tile0[0], itab + h->o_tileb[0], c.in_channels, d_mel_amax);
    PK_TRY(hfg_chain(h, d_mel, d_mel_amax, d_wav, -1, nullptr));
    h->last_valid = true;
    if (host) {
        PK_HIP(hipMemcpyAsync(wav_out, d_wav, nwav * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

// the same kernels over utterance b of the last call alone (its tiles and scales are those of the batch), stopped after
// stage `stage` (>= 0) or after launch `launch` (>= 0): -> the buffer written last, its channels and positions
static int hfg_debug_run(pk_hfg* h, const char* who, int stage, int launch, int b, const float** ptr, int* C, long* len) {
    if (!h->last_valid || !h->finalized) PK_FAIL(PK_ESTATE, "%s: no pk_hfg_infer since the parameters were set", who);
    const pk_hfg_cfg& c = h->cfg;
    if (b < 0 || b >= (int)h->last_frames.size()) PK_FAIL(PK_EINVAL, "%s: utterance out of range", who);
    const std::vector<int> keep_frames = h->last_frames;
    const std::vector<long> keep_off = h->last_off;
    const int32_t one = keep_frames[b];
    // the utterance's first tile in the batch's rate-0 table: the tile maxima follow the mel in ws_mel
    long tile_first = 0, total = 0;
    for (int q = 0; q < b; ++q) tile_first += (keep_frames[q] + HFG_TILE - 1) / HFG_TILE;
    for (size_t q = 0; q < keep_frames.size(); ++q) total += keep_frames[q];
    const size_t nmel = (size_t)total * c.in_channels;
    float* d_mel_all = h->ws_mel.as<float>();
    float* d_amax_all = d_mel_all + (nmel + 63) / 64 * 64;
    int st;
    try {
        st = hfg_tables(h, who, &one, 1);
    } catch (const std::exception& e) {
        pk_set_error("%s: host tables: %s", who, e.what());
        st = PK_ENOMEM;
    }
    PK_TRY(st);
    // From here the handle's device tables, ntiles and sumL are those of this ONE utterance, not of the batch (last_frames /
    // last_off keep the batch on the host): every entry point rebuilds them before it launches, and nothing may read
    // h->ntiles / h->sumL for the batch after a tap.
    const float* d_stage = nullptr;
    h->dbg_stop = launch;
    st = hfg_chain(h, d_mel_all + keep_off[b] * c.in_channels, d_amax_all + tile_first, nullptr, stage, &d_stage);
    h->dbg_stop = -1;
    PK_TRY(st);
    if (launch >= 0) {
        if (!h->dbg_ptr) PK_FAIL(PK_EINVAL, "%s: launch %d out of range (the model has %d before tanh)", who, launch, h->dbg_count);
        *ptr = h->dbg_ptr;
        *C = h->dbg_C;
        *len = h->sumL[h->dbg_rate];
        h->dbg_ptr = nullptr;
    } else {
        *ptr = d_stage;
        *C = hfg_ch(c, stage + 1);
        *len = h->sumL[stage + 1];
    }
    return PK_OK;
}

extern "C" int pk_hfg_debug_read(pk_hfg* h, int32_t stage, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_hfg_debug_read: NULL argument");
    if (stage < 0 || stage >= h->cfg.n_upsample)
        PK_FAIL(PK_EINVAL, "pk_hfg_debug_read: stage %d out of range (the model has %d)", stage, h->cfg.n_upsample);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const float* p = nullptr;
    int C = 0;
    long len = 0;
    PK_TRY(hfg_debug_run(h, "pk_hfg_debug_read", stage, -1, b, &p, &C, &len));
    if (n_floats != (int64_t)C * len) PK_FAIL(PK_ESHAPE, "pk_hfg_debug_read: expected %ld floats", (long)C * len);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    PK_HIP(hipMemcpy(host_out, p, (size_t)C * len * 4, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_hfg_debug_conv(pk_hfg* h, int32_t launch, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_hfg_debug_conv: NULL argument");
    if (launch < 0 || launch + 1 >= (int)h->convs.size())   // the last one is the output convolution: pk_hfg_infer's wav
        PK_FAIL(PK_EINVAL, "pk_hfg_debug_conv: launch %d out of range (the model has %d before the output convolution)", launch,
                (int)h->convs.size() - 1);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const float* p = nullptr;
    int C = 0;
    long len = 0;
    PK_TRY(hfg_debug_run(h, "pk_hfg_debug_conv", -1, launch, b, &p, &C, &len));
    if (n_floats != (int64_t)C * len) PK_FAIL(PK_ESHAPE, "pk_hfg_debug_conv: expected %ld floats", (long)C * len);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    PK_HIP(hipMemcpy(host_out, p, (size_t)C * len * 4, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" void pk_hfg_destroy(pk_hfg* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    if (h->stage) (void)hipHostFree(h->stage);
    if (h->stage_done) (void)hipEventDestroy(h->stage_done);
    pk_dbuf* bufs[] = {&h->d_w32, &h->d_w16, &h->d_bias, &h->d_mu, &h->d_sigma, &h->ws_itab, &h->ws_ltab, &h->ws_mel,
                       &h->ws_act, &h->ws_amax, &h->ws_wav, &h->ws_hostmel};
    for (auto* b : bufs) b->release();
    delete h;
}
