// pk_hfg_conv.h -- the MFMA convolution kernel of the GAN vocoders and its host helpers, shared by hifigan.hip and melgan.hip.
// Everything is in an anonymous namespace: each including file instantiates and registers its own kernels.
//
// k_hfg_conv: out[co, t] = epi(bias[co] + sum_(tap, ci) W[co, ci, tap] * leaky_s(in[ci, t + t0 + tap * step])).  One workgroup
// takes HFG_TILE positions of one utterance (tiles start at utterance-relative multiples of the tile) and 32 * CT output
// channels.  The input window (tile + 2 * halo) is staged in LDS slab by slab of 32 input channels, [position][channel]:
// LeakyReLU is applied and the value split into its fp16 pair ONCE there, so a tap's B operand is one 16-byte LDS read and
// nothing is split inside the k-loop.  The weights are the A operand, packed as fragments at finalize and read
// through the caches; each of the four waves owns two 32-position tiles per fragment.
//
// The boundary rule is the compile-time parameter BND:
//   HFG_BND_ZERO     positions outside the utterance (and channels past C_in) are written as 0 by a select.
//   HFG_BND_REFLECT  a window position g outside [0, len) is staged from -g when g < 0 and from 2 (len - 1) - g when g >= len
//                    (ReflectionPad1d).  A reflected source is a copy of an in-range value, so the maximum the producer
//                    measured over the utterance still bounds what is staged.  Positions whose reflected source would still
//                    fall outside [0, len) are never read by an in-range output (the caller guarantees pad < len) and are
//                    written as 0.  Either way LDS never holds an undefined value.
//   Transposed and 1x1 convolutions use HFG_BND_ZERO.
//
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
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pk_common.h"
#include "pk_hifigan.h"
#include "pk_mfma.h"

namespace {

enum { HFG_EPI_STORE = 0, HFG_EPI_RES = 1, HFG_EPI_SUM = 2, HFG_EPI_TANH = 3 };
enum { HFG_BND_ZERO = 0, HFG_BND_REFLECT = 1 };

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

template <int MATH, int CT, int BND>
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
            int g = g0 + p;
            if (BND == HFG_BND_REFLECT) g = g < 0 ? -g : (g >= len ? 2 * (len - 1) - g : g);
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
// maximum of a tile of 256 frames for the input convolution's scale.
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

// What the launches of a stack need: the packed weights, the tables of the running call, the launch tap.  A model's handle
// derives from it.
struct hfg_engine {
    pk_ctx* ctx = nullptr;
    int math = PK_PWG_MATH_F16X3;
    pk_dbuf d_w32, d_w16, d_bias;
    pk_dbuf ws_itab, ws_ltab;
    // pinned staging of a call's tables (int part, then the long part) and the event after their copies: the upload does not
    // block the host, and the next call waits for this event alone before it overwrites the staging
    void* stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t stage_done = nullptr;
    bool stage_busy = false;
    // tables of the running call (offsets into ws_itab / ws_ltab per rate)
    std::vector<size_t> o_lens, o_tile0, o_tileb, o_offs;
    std::vector<int> ntiles;
    std::vector<long> sumL;
    // the launch tap: stop after launch dbg_stop (-1: never); what it wrote
    int dbg_stop = -1, dbg_count = 0, dbg_C = 0, dbg_rate = 0;
    const float* dbg_ptr = nullptr;
};

// Fragments of one convolution: at(phase, co, ci, tap) is W in the kernel's orientation (zero past C_out / C_in).
template <class F>
void hfg_pack(hfg_conv& cv, int phases, int ntaps, F at, std::vector<float>& f32, std::vector<uint16_t>& f16) {
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

// One convolution `name` of a parameter map, packed behind what f32 / f16 / bias already hold (Conv1D (C_out, C_in, k), or
// the transposed one (C_in, C_out, 2 s) in its s phases of two taps).  Returns the most maxima one of its tiles writes.
inline int hfg_add_conv(const pk_param_map& params, std::vector<hfg_conv>& convs, std::vector<float>& f32, std::vector<uint16_t>& f16,
                        std::vector<float>& bias, const std::string& name, int Cin, int Cout, int k, int dil, bool transposed,
                        int s, int* slots) {
    std::vector<float> w, bv;
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
    if (transposed) PK_TRY(pk_get_weight(params, name, {Cin, Cout, k}, w));
    else PK_TRY(pk_get_weight(params, name, {Cout, Cin, k}, w));
    PK_TRY(pk_get_vector(params, name + ".bias", Cout, bv));
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
    *slots = cv.CTtot / cv.CT * (transposed ? s : 1);
    convs.push_back(cv);
    return PK_OK;
}

// per rate r = 0 ... R - 1 (rate r is rate r - 1 times scales[r - 1]): lens | tile0 | tile_b and offs of one call onto the device
inline int hfg_tables(hfg_engine* h, const char* who, const int32_t* frames, int B, const int32_t* scales, int R) {
    pk_ctx* ctx = h->ctx;
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
        if (r) mul *= scales[r - 1];
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

// one convolution: `in` at rate r -> `out` (rate r, or r + 1 for the transposed one), under the boundary rule BND
template <int BND>
int hfg_launch(hfg_engine* h, const hfg_conv& cv, int r, const hfg_act& in, hfg_act& out, const float* res, int mode,
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
#define HFG_GO(M, CTV) PK_LAUNCH(ctx, "hfg_conv", (k_hfg_conv<M, CTV, BND>), grid, block, 0, a)
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

inline void hfg_engine_release(hfg_engine* h) {
    if (h->stage) (void)hipHostFree(h->stage);
    if (h->stage_done) (void)hipEventDestroy(h->stage_done);
    pk_dbuf* bufs[] = {&h->d_w32, &h->d_w16, &h->d_bias, &h->ws_itab, &h->ws_ltab};
    for (auto* b : bufs) b->release();
}

}  // namespace
