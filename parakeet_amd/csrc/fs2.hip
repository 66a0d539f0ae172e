// fs2.hip -- FastSpeech2 inference on gfx950: kernels + pk_fs2_* entry points.
//
// Reference: parakeet/models/fastspeech2/fastspeech2.py FastSpeech2.inference :468-558
// (_forward(is_inference=True) :377-466) and the modules listed in SURVEY.md 8a
// (encoder.py, encoder_layer.py, attention.py, embedding.py, multi_layer_conv.py,
// duration_predictor.py, variance_predictor.py, length_regulator.py, layer_norm.py,
// tacotron2/decoder.py Postnet, normalizer.py).
//
// The row timeline, the FFT blocks, the postnet and the speaker integration are pk_fft.h (fft.hip).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "pk_fft.h"
#include "pk_ffn_planes.h"
#include "pk_gemm.h"

namespace {

// Predictor heads: Linear(C -> 1) per row (+ masked_fill) and, for the duration
// predictor in inference, clip(round(exp(x) - offset), min=0) and the alpha speed
// scaling round(d * alpha)  (duration_predictor.py:95-103, length_regulator.py:85-88;
// paddle.round = half away from zero).
__device__ __forceinline__ float round_half_away(float x) { return copysignf(floorf(fabsf(x) + 0.5f), x); }

__global__ __launch_bounds__(256) void k_rowdot(const float* __restrict__ h, int C, const float* __restrict__ w,
                                                float bias, const int* __restrict__ row_utt, int rows,
                                                int duration_mode, float offset, float alpha,
                                                float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    if (row_utt[r] < 0) {
        if (lane == 0) out[r] = 0.f;
        return;
    }
    const float* x = h + (long)r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(x[c], w[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    s += bias;
    if (duration_mode) {
        s = fmaxf(round_half_away(expf(s) - offset), 0.f);
        if (alpha != 1.0f) s = round_half_away(s * alpha);
    }
    if (lane == 0) out[r] = s;
}

// Inclusive prefix sum of the integer durations of each utterance; frames[b] = total.
__global__ __launch_bounds__(256) void k_cumsum(const float* __restrict__ dur, const int* __restrict__ seg_start,
                                                const int* __restrict__ seg_len, int* __restrict__ cum,
                                                int* __restrict__ frames) {
    __shared__ int sh[256];
    const int b = blockIdx.x, start = seg_start[b], len = seg_len[b];
    int carry = 0;
    for (int base = 0; base < len; base += 256) {
        const int t = base + threadIdx.x;
        int v = (t < len) ? (int)dur[start + t] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            int add = ((int)threadIdx.x >= o) ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < len) cum[start + t] = carry + sh[threadIdx.x];
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) frames[b] = carry;
}

// Length regulator + variance embeddings + decoder positional encoding, fused:
//   hs2  = hs + (e * w_e + b_e) + (p * w_p + b_p)            fastspeech2.py:426-430 (k=1 convs)
//   up[l] = hs2[token(l)]                                    length_regulator.py:46-66 (row repeat)
//   x[l]  = up[l] * xscale + alpha_dec * PE[l]               decoder embed, fastspeech2.py:250-266
// token(l) = first t with cum[t] > l (binary search in the utterance's prefix sums).
__global__ __launch_bounds__(128) void k_regulate(
    const float* __restrict__ hs, const float* __restrict__ p_out, const float* __restrict__ e_out,
    const float* __restrict__ wp, const float* __restrict__ bp, const float* __restrict__ we,
    const float* __restrict__ be, const int* __restrict__ cum, const int* __restrict__ tseg_start,
    const int* __restrict__ tseg_len, const int* __restrict__ frow_utt, const int* __restrict__ frow_pos,
    const float* __restrict__ pe, float alpha_dec, float xscale, int d, float* __restrict__ x,
    float* __restrict__ hs_up_dbg) {
    const int r = blockIdx.x;
    const int b = frow_utt[r];
    float* xo = x + (long)r * d;
    if (b < 0) {
        for (int c = threadIdx.x; c < d; c += blockDim.x) xo[c] = 0.f;
        return;
    }
    const int l = frow_pos[r];
    const int* cu = cum + tseg_start[b];
    int lo = 0, hi = tseg_len[b] - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] > l) hi = mid; else lo = mid + 1;
    }
    const int tr = tseg_start[b] + lo;
    const float pv = p_out[tr], ev = e_out[tr];
    const float* src = hs + (long)tr * d;
    const float* pp = pe + (long)l * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        const float e_emb = fmaf(ev, we[c], be[c]);
        const float p_emb = fmaf(pv, wp[c], bp[c]);
        const float up = (src[c] + e_emb) + p_emb;
        if (hs_up_dbg) hs_up_dbg[(long)r * d + c] = up;
        xo[c] = up * xscale + alpha_dec * pp[c];
    }
}

}  // namespace

// reduction_factor r > 1: feat_out gives r frames per decoder row ([frame 0 | ... | frame r-1], fastspeech2.py:457:
// .reshape((B, -1, odim))).  Frame row q of the frame timeline (utterance u, position p) takes columns (p % r) * O .. of
// decoder row dec_seg_start[u] + p / r; gap rows are zeroed when rowmap == NULL (the postnet convolves over them).
__global__ __launch_bounds__(128) void k_fs2_unfold_r(const float* __restrict__ wide, int O, int r,
                                                      const int* __restrict__ dec_seg_start, const int* __restrict__ row_utt,
                                                      const int* __restrict__ row_pos, const int* __restrict__ rowmap,
                                                      const float* __restrict__ cscale, const float* __restrict__ cshift,
                                                      float* __restrict__ dst) {
    const long q = blockIdx.x;
    const int u = row_utt[q];
    const long o = rowmap ? rowmap[q] : q;
    if (o < 0) return;
    if (u < 0) {
        if (!rowmap)
            for (int c = threadIdx.x; c < O; c += blockDim.x) dst[o * O + c] = 0.f;
        return;
    }
    const int p = row_pos[q];
    const float* s = wide + ((long)(dec_seg_start[u] + p / r) * r + p % r) * O;
    for (int c = threadIdx.x; c < O; c += blockDim.x) {
        float v = s[c];
        if (cscale) v = v * cscale[c] + cshift[c];
        dst[o * O + c] = v;
    }
}

// hs[r] += ptone[tone[r]] on the rows of the timeline that belong to an utterance
__global__ __launch_bounds__(256) void k_add_tone(float* __restrict__ hs, const float* __restrict__ ptone,
                                                  const int* __restrict__ tone, const int* __restrict__ row_utt,
                                                  int A) {
    const int r = blockIdx.x;
    if (row_utt[r] < 0) return;
    const float* src = ptone + (long)tone[r] * A;
    for (int c = threadIdx.x; c < A; c += blockDim.x) hs[(long)r * A + c] += src[c];
}

// dst[rowmap[q]] = src[q] for the timeline rows that belong to an utterance: a timeline tensor, packed by utterance
__global__ __launch_bounds__(128) void k_fs2_pack_rows(const float* __restrict__ src, int O, const int* __restrict__ rowmap,
                                                       float* __restrict__ dst) {
    const long q = blockIdx.x;
    const long o = rowmap[q];
    if (o < 0) return;
    for (int c = threadIdx.x; c < O; c += blockDim.x) dst[o * O + c] = src[q * O + c];
}

typedef pk_fft_dense Dense;
typedef pk_fft_layer FftLayer;
typedef pk_fft_timeline Timeline;

struct Predictor {
    std::vector<Dense> conv;
    std::vector<size_t> ln_g, ln_b;
    size_t lin_w;
    float lin_b;
    int chans;
};

struct pk_fs2 : pk_fft_core {
    pk_fs2_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int gapr = 2;
    // weights (arena, math mode, positional table and the FFT-stack buffers: pk_fft_core)
    size_t emb_table = 0, enc_after_g = 0, enc_after_b = 0, dec_after_g = 0, dec_after_b = 0;
    float alpha_enc = 1.f, alpha_dec = 1.f, xscale = 1.f;
    std::vector<FftLayer> enc, dec;
    Predictor dur, pitch, energy;
    size_t pitch_w = 0, pitch_b = 0, energy_w = 0, energy_b = 0;
    Dense feat_out;
    std::vector<Dense> postnet;
    size_t tone_table = 0;                         // [num_tones][A]: tone_projection(normalize(embedding row))
    std::vector<long long> cond_tone;              // conditioning of the next encode (pk_fs2_set_tones)
    pk_dbuf d_tone;
    size_t spk_table = 0, spk_w = 0, spk_b = 0;   // embedding table, [D][A] speaker part of spk_projection, bias
    Dense spk_hs;                                  // "concat": the [A][A] hidden-state part of spk_projection
    std::vector<long long> cond_spk;               // conditioning of the next encode (pk_fs2_set_speakers)
    std::vector<float> cond_emb;
    int cond_B = 0;
    pk_dbuf d_spk_id, d_spk_emb, d_spk_vec;
    // targets of the next encode (pk_fs2_set_targets): given durations / pitch / energy, packed by utterance
    std::vector<long long> cond_dur;
    std::vector<float> cond_pitch, cond_energy;
    long cond_tgt_n = 0;
    bool cond_has_dur = false, cond_has_pitch = false, cond_has_energy = false;
    pk_dbuf d_tdur, d_tpitch, d_tenergy;           // ... on the token timeline, what k_cumsum / k_regulate read in their place
    const float* reg_pitch = nullptr;              // pitch / energy of the last encode that k_regulate embeds
    const float* reg_energy = nullptr;
    bool decoded = false;                          // before_outs of the last encode is on the device
    size_t out_scale = 0, out_shift = 0;
    bool has_out_affine = false;
    std::vector<float> h_out_scale, h_out_shift;
    // per-call state
    Timeline tl_tok, tl_frm, tl_frm2;   // tokens, decoder rows, mel frames (= decoder rows unless reduction_factor > 1)
    pk_dbuf d_wide, d_rowmap2;
    pk_dbuf d_pamax;   // row maxima of the predictors' LayerNorm outputs
    pk_dbuf d_hsp, d_hsam, d_pp, d_ppam;   // planes path of the predictors: the encoder output as planes, a layer's work planes
    char* hsp = nullptr;
    unsigned* hsam = nullptr;
    bool hs_planes_valid = false;           // ... converted once per pk_fs2_encode
    pk_dbuf d_tok, d_p1, d_p2, d_hs, d_pout, d_eout, d_dout, d_cum, d_frames,
        d_before, d_q1, d_q2, d_rowmap, d_dbg_up, d_zs, d_mel_stage;
    std::vector<int> frames;   // per utterance, result of encode
    bool encoded = false;
    bool debug = false;
};

extern "C" int pk_fs2_create(pk_ctx* ctx, const pk_fs2_cfg* cfg, pk_fs2** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_fs2_create: NULL argument");
    *out = nullptr;
    const pk_fs2_cfg& c = *cfg;
    if (c.idim <= 0 || c.odim <= 0 || c.adim <= 0 || c.aheads <= 0)
        PK_FAIL(PK_EINVAL, "FastSpeech2: idim/odim/adim/aheads must be positive");
    if (c.adim % c.aheads != 0) PK_FAIL(PK_ESHAPE, "FastSpeech2: adim %% aheads != 0 (attention.py:40)");
    const int dk = c.adim / c.aheads;
    if (dk != 64 && dk != 96 && dk != 128 && dk != 192)
        PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: head size %d not built (64/96/128/192)", dk);
    if (c.adim % 64 != 0 || c.adim > 64 * PK_FFT_LN_MAXPER)
        PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: adim must be a multiple of 64, <= %d", 64 * PK_FFT_LN_MAXPER);
    if (c.reduction_factor < 1 || c.reduction_factor > 16) PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: reduction_factor must be in [1, 16]");
    if (c.pitch_embed_kernel_size != 1 || c.energy_embed_kernel_size != 1)
        PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: pitch/energy_embed_kernel_size must be 1 (all reference recipes)");
    if (c.tone_embed_dim < 0 || c.num_tones < 0) PK_FAIL(PK_EINVAL, "FastSpeech2: negative tone sizes");
    if (c.tone_embed_dim > 0 && c.num_tones <= 0) PK_FAIL(PK_EINVAL, "FastSpeech2: tone_embed_dim needs num_tones");
    if (c.tone_embed_dim > 0 && c.tone_embed_integration_type != 0)
        PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: tone_embed_integration_type 'concat' is not implemented "
                                 "(the reference's branch cannot broadcast 1-D tone ids, fastspeech2.py:606-610)");
    if (c.positionwise_layer_type < 0 || c.positionwise_layer_type > 2)
        PK_FAIL(PK_EUNSUPPORTED, "Support only linear or conv1d. (encoder.py:169)");
    if (c.spk_embed_dim < 0 || c.num_speakers < 0) PK_FAIL(PK_EINVAL, "FastSpeech2: negative speaker sizes");
    if (c.spk_embed_dim > 0 && c.spk_embed_integration_type != 0 && c.spk_embed_integration_type != 1)
        PK_FAIL(PK_EUNSUPPORTED, "support only add or concat. (fastspeech2.py:584)");
    if (c.spk_embed_dim > 8192) PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: spk_embed_dim > 8192");
    if (c.postnet_layers > 0 && !c.use_batch_norm)
        PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: postnet without batch norm not implemented");
    const int ks[] = {c.positionwise_conv_kernel_size, c.duration_predictor_kernel_size,
                      c.pitch_predictor_kernel_size, c.energy_predictor_kernel_size,
                      c.postnet_layers > 0 ? c.postnet_filts : 1};
    int gapr = 1;
    for (int k : ks) {
        if (k < 1 || k % 2 == 0 || k > 15) PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: conv kernel size %d unsupported", k);
        gapr = std::max(gapr, (k - 1) / 2);
    }
    const int chans[] = {c.adim, c.eunits, c.dunits, c.duration_predictor_chans, c.pitch_predictor_chans,
                         c.energy_predictor_chans, c.postnet_layers > 0 ? c.postnet_chans : 16, c.odim};
    for (int ch : chans)
        if (ch % PK_GEMM_BK != 0) PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: channel count %d not a multiple of 16", ch);
    const int pch[] = {c.duration_predictor_chans, c.pitch_predictor_chans, c.energy_predictor_chans};
    for (int ch : pch)
        if (ch % 64 != 0 || ch > 64 * PK_FFT_LN_MAXPER)
            PK_FAIL(PK_EUNSUPPORTED, "FastSpeech2: predictor channels must be a multiple of 64, <= %d", 64 * PK_FFT_LN_MAXPER);
    pk_fs2* h = new pk_fs2();
    h->ctx = ctx;
    h->cfg = c;
    h->adim = c.adim;
    h->aheads = c.aheads;
    h->attn_lds = pk_prof_env("PK_FS2_ATTN_NO_LDS") == nullptr;
    h->no_bounds = pk_prof_env("PK_FS2_NO_BOUNDS") != nullptr;
    h->gapr = gapr;
    h->ffn_planes_min_blocks = FFNP_MIN_BLOCKS;
    if (const char* e = pk_prof_env("PK_FS2_FFN_PLANES")) h->ffn_planes = e[0] != '0';
    if (const char* e = pk_prof_env("PK_FS2_FFN_PLANES_MIN_BLOCKS")) h->ffn_planes_min_blocks = atoi(e);
    if (const char* e = pk_prof_env("PK_FFNP_VARIANT")) h->ffnp_variant = atoi(e);
    if (const char* e = pk_prof_env("PK_FS2_ATTN_WAVES")) h->attn_waves = atoi(e);
    if (const char* e = pk_prof_env("PK_FS2_MATH")) h->math = strcmp(e, "f32") == 0 ? PK_GEMM_MATH_F32 : PK_GEMM_MATH_F16X3;
    if (gapr > PK_FFT_LEAD) { delete h; PK_FAIL(PK_EUNSUPPORTED, "conv kernel too wide"); }
    *out = h;
    return PK_OK;
}

extern "C" int pk_fs2_set_param(pk_fs2* h, const char* name, const float* data, const int64_t* shape,
                                int32_t ndim) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_param: handle is NULL");
    h->finalized = false;
    return pk_store_param(h->params, name, data, shape, ndim);
}

extern "C" int pk_fs2_set_normalizer(pk_fs2* h, const float* mu, const float* sigma, int32_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_normalizer: handle is NULL");
    if (!mu && !sigma) {
        h->has_out_affine = false;
    } else {
        if (!mu || !sigma || n != h->cfg.odim) PK_FAIL(PK_ESHAPE, "normalizer needs mu and sigma of odim elements");
        h->h_out_scale.assign(sigma, sigma + n);
        h->h_out_shift.assign(mu, mu + n);
        h->has_out_affine = true;
    }
    h->finalized = false;
    return PK_OK;
}

typedef pk_fft_arena Arena;

namespace {
int add_predictor(Arena& ar, const pk_param_map& P, const std::string& prefix, int n_layers, int A, int chans,
                  int k, Predictor& pr) {
    pr.conv.resize(n_layers);
    pr.ln_g.resize(n_layers);
    pr.ln_b.resize(n_layers);
    pr.chans = chans;
    for (int j = 0; j < n_layers; ++j) {
        const std::string p = prefix + ".conv." + std::to_string(j);
        PK_TRY(pk_fft_add_conv(ar, P, p + ".0", chans, j == 0 ? A : chans, k, true, pr.conv[j]));
        PK_TRY(pk_fft_add_vec(ar, P, p + ".2.weight", chans, pr.ln_g[j]));
        PK_TRY(pk_fft_add_vec(ar, P, p + ".2.bias", chans, pr.ln_b[j]));
    }
    PK_TRY(pk_fft_add_vec(ar, P, prefix + ".linear.weight", chans, pr.lin_w));
    std::vector<float> b;
    PK_TRY(pk_get_vector(P, prefix + ".linear.bias", 1, b));
    pr.lin_b = b[0];
    return PK_OK;
}
}  // namespace

extern "C" int pk_fs2_finalize(pk_fs2* h) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_finalize: handle is NULL");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_fs2_cfg& c = h->cfg;
    const pk_param_map& P = h->params;
    const int A = c.adim;
    h->arena_h.clear();
    h->arena16_h.clear();
    Arena ar{h->arena_h, &h->arena16_h};
    {
        std::vector<float> t;
        PK_TRY(pk_get_weight(P, "encoder.embed.0", {c.idim, A}, t));
        for (int i = 0; i < A; ++i) t[i] = 0.f;  // nn.Embedding(padding_idx=0): id 0 -> zero row
        h->emb_table = ar.put(t);
    }
    std::vector<float> al;
    if (c.use_scaled_pos_enc) {
        PK_TRY(pk_get_vector(P, "encoder.embed.1.alpha", 1, al));
        h->alpha_enc = al[0];
        PK_TRY(pk_get_vector(P, "decoder.embed.0.alpha", 1, al));
        h->alpha_dec = al[0];
        h->xscale = 1.f;
    } else {
        h->alpha_enc = h->alpha_dec = 1.f;
        h->xscale = std::sqrt((float)A);  // PositionalEncoding.forward embedding.py:78
    }
    PK_TRY(pk_fft_add_stack(ar, P, "encoder", c.elayers, A, c.eunits, c.positionwise_conv_kernel_size, c.positionwise_layer_type, c.aheads, h->enc,
                         h->enc_after_g, h->enc_after_b, c.encoder_normalize_before != 0, c.encoder_concat_after != 0));
    PK_TRY(pk_fft_add_stack(ar, P, "decoder", c.dlayers, A, c.dunits, c.positionwise_conv_kernel_size, c.positionwise_layer_type, c.aheads, h->dec,
                         h->dec_after_g, h->dec_after_b, c.decoder_normalize_before != 0, c.decoder_concat_after != 0));
    PK_TRY(add_predictor(ar, P, "duration_predictor", c.duration_predictor_layers, A, c.duration_predictor_chans,
                         c.duration_predictor_kernel_size, h->dur));
    PK_TRY(add_predictor(ar, P, "pitch_predictor", c.pitch_predictor_layers, A, c.pitch_predictor_chans,
                         c.pitch_predictor_kernel_size, h->pitch));
    PK_TRY(add_predictor(ar, P, "energy_predictor", c.energy_predictor_layers, A, c.energy_predictor_chans,
                         c.energy_predictor_kernel_size, h->energy));
    PK_TRY(pk_fft_add_vec(ar, P, "pitch_embed.0.weight", A, h->pitch_w));
    PK_TRY(pk_fft_add_vec(ar, P, "pitch_embed.0.bias", A, h->pitch_b));
    PK_TRY(pk_fft_add_vec(ar, P, "energy_embed.0.weight", A, h->energy_w));
    PK_TRY(pk_fft_add_vec(ar, P, "energy_embed.0.bias", A, h->energy_b));
    {
        std::vector<float> w, b;
        const int OR = c.odim * c.reduction_factor;   // feat_out: adim -> odim * reduction_factor (fastspeech2.py:271)
        PK_TRY(pk_get_weight(P, "feat_out", {A, OR}, w));
        PK_TRY(pk_get_vector(P, "feat_out.bias", OR, b));
        PK_TRY(pk_fft_add_dense_kn(ar, w, &b, A, 1, OR, h->feat_out));
    }
    PK_TRY(pk_fft_add_postnet(ar, P, "postnet", c.postnet_layers, c.odim, c.postnet_chans, c.postnet_filts, h->postnet));
    if (c.tone_embed_dim > 0) {
        // "add": hs[t] += Linear(F.normalize(E[tone[t]])) is a function of the tone id alone -> one table
        const int Dt = c.tone_embed_dim;
        std::vector<float> e, w, b, tab((size_t)c.num_tones * A);
        PK_TRY(pk_get_weight(P, "tone_embedding_table", {c.num_tones, Dt}, e));
        PK_TRY(pk_get_weight(P, "tone_projection", {Dt, A}, w));
        PK_TRY(pk_get_vector(P, "tone_projection.bias", A, b));
        for (int k = 0; k < c.num_tones; ++k) {
            double ss = 0.0;
            if (k != 0)   // nn.Embedding(padding_idx=0) returns zeros for id 0
                for (int i = 0; i < Dt; ++i) ss += (double)e[(size_t)k * Dt + i] * e[(size_t)k * Dt + i];
            const double inv = 1.0 / std::max(std::sqrt(ss), 1e-12);
            for (int o = 0; o < A; ++o) {
                double acc = 0.0;
                if (k != 0)
                    for (int i = 0; i < Dt; ++i) acc += (double)e[(size_t)k * Dt + i] * inv * w[(size_t)i * A + o];
                tab[(size_t)k * A + o] = (float)(acc + b[o]);
            }
        }
        h->tone_table = ar.put(tab);
    }
    if (c.spk_embed_dim > 0) {
        const int D = c.spk_embed_dim;
        std::vector<float> t, w, b;
        if (c.num_speakers > 0) {
            PK_TRY(pk_get_weight(P, "spk_embedding_table", {c.num_speakers, D}, t));
            h->spk_table = ar.put(t);
        }
        PK_TRY(pk_get_vector(P, "spk_projection.bias", A, b));
        h->spk_b = ar.put(b);
        if (c.spk_embed_integration_type == 0) {
            PK_TRY(pk_get_weight(P, "spk_projection", {D, A}, w));
            h->spk_w = ar.put(w);
        } else {
            // Linear(adim + D -> adim) on concat([hs, e]) = hs . W[:adim] + e . W[adim:] (+ bias, added with e's part)
            PK_TRY(pk_get_weight(P, "spk_projection", {A + D, A}, w));
            std::vector<float> whs(w.begin(), w.begin() + (size_t)A * A), wsp(w.begin() + (size_t)A * A, w.end());
            PK_TRY(pk_fft_add_dense_kn(ar, whs, nullptr, A, 1, A, h->spk_hs));
            h->spk_w = ar.put(wsp);
        }
    }
    if (h->has_out_affine) {
        h->out_scale = ar.put(h->h_out_scale);
        h->out_shift = ar.put(h->h_out_shift);
    }
    PK_TRY(pk_upload(ctx, h->arena, h->arena_h.data(), h->arena_h.size() * sizeof(float)));
    h->arena_h.clear();
    h->arena_h.shrink_to_fit();
    if (!h->arena16_h.empty())
        PK_TRY(pk_upload(ctx, h->arena16, h->arena16_h.data(), h->arena16_h.size() * sizeof(uint16_t)));
    h->arena16_h.clear();
    h->arena16_h.shrink_to_fit();
    PK_TRY(pk_fft_ensure_pe(h, 1024));
    h->finalized = true;
    h->encoded = false;
    return PK_OK;
}

static int run_predictor(pk_fs2* h, const Predictor& pr, const Timeline& tl, const float* hs, int duration_mode,
                         float alpha, float* out) {
    const int A = h->cfg.adim;
    PK_TRY(pk_fft_act_reserve(h->d_p1, tl.rows, pr.chans));
    PK_TRY(pk_fft_act_reserve(h->d_p2, tl.rows, pr.chans));
    float* p1 = pk_fft_act_ptr(h->d_p1, pr.chans);
    float* p2 = pk_fft_act_ptr(h->d_p2, pr.chans);
    const float* in = hs;
    int ldin = A;
    // operand scales of the split-fp16 convs: the row maxima come out of the LayerNorm that produces the rows (no pass of
    // their own: 6 of the 9 k_row_amax launches of a batch); the buffer is zero outside the rows it writes (margins, padding)
    float* pam = nullptr;
    if (h->math == PK_GEMM_MATH_F16X3) {
        PK_TRY(pk_fft_act_reserve(h->d_pamax, tl.rows, 1));
        PK_HIP(hipMemsetAsync(h->d_pamax.p, 0, h->d_pamax.cap, h->ctx->stream));
        pam = pk_fft_act_ptr(h->d_pamax, 1);
    }
    // Round 4: the convs on the planes kernel (csrc/ffn_planes.hip, 384 | 256 -> 256 channels, k = 3 | 5): encoder output ->
    // planes once per batch (shared by the three predictors), conv -> fp32 rows (ReLU), LayerNorm -> planes for the next conv
    // (k_ffn_ln_planes) or -> fp32 rows for the head after the last one.  Same arithmetic class as the tile GEMM path
    // (block-scaled split-fp16, one scale per row), half its time.
    bool planes = h->math == PK_GEMM_MATH_F16X3 && h->ffn_planes && tl.rows_alloc % FFNP_BLK == 0 && !pr.conv.empty();
    for (const Dense& d : pr.conv) planes = planes && d.wp != (size_t)-1 && d.wps != (size_t)-1;
    if (planes) {
        const int nblk = tl.rows_alloc / FFNP_BLK;
        const int* rv = tl.d_row_utt();
        if (!h->hs_planes_valid) {
            PK_TRY(pk_fft_planes_buf(h, h->d_hsp, h->d_hsam, nblk, A, &h->hsp, &h->hsam));
            PK_TRY(ffnp_layernorm_launch(h->ctx, hs, nullptr, nullptr, rv, nblk, A, 0.f, h->hsp, h->hsam));
            h->hs_planes_valid = true;
        }
        char* pp = nullptr;
        unsigned* ppam = nullptr;
        PK_TRY(pk_fft_planes_buf(h, h->d_pp, h->d_ppam, nblk, pr.chans, &pp, &ppam));
        const void* cin = h->hsp;
        const unsigned* cam = h->hsam;
        for (size_t j = 0; j < pr.conv.size(); ++j) {
            FfnpConv c = pk_fft_conv256_args(h, pr.conv[j], nblk, rv, cin, cam);
            c.x = p1;
            c.ldx = pr.chans;
            PK_TRY(ffnp_conv256_launch(h->ctx, "fs2_conv_predictor_planes", c, pr.conv[j].taps, 2));
            if (j + 1 < pr.conv.size()) {
                PK_TRY(ffnp_layernorm_launch(h->ctx, p1, h->W(pr.ln_g[j]), h->W(pr.ln_b[j]), rv, nblk, pr.chans, 1e-5f, pp, ppam));
                cin = pp;
                cam = ppam;
            } else {
                PK_TRY(pk_fft_run_layernorm(h, p1, pr.ln_g[j], pr.ln_b[j], tl, pr.chans, p2));
            }
        }
        in = p2;
        ldin = pr.chans;
    }
    const float* in_amax = nullptr;
    for (size_t j = 0; j < pr.conv.size() && !planes; ++j) {
        PK_TRY(pk_fft_run_dense(h, "fs2_conv_predictor", pr.conv[j], in, ldin, p1, pr.chans, tl.rows, PK_ACT_RELU, nullptr, 0,
                         nullptr, in_amax));
        PK_TRY(pk_fft_run_layernorm(h, p1, pr.ln_g[j], pr.ln_b[j], tl, pr.chans, p2, pam));
        in = p2;
        ldin = pr.chans;
        in_amax = pam;
    }
    PK_LAUNCH(h->ctx, "fs2_rowdot", k_rowdot, dim3(pk_div_up(tl.rows, 4)), dim3(256), 0, in, ldin, h->W(pr.lin_w),
              pr.lin_b, tl.d_row_utt(), tl.rows, duration_mode, 1.0f, alpha, out);
    return PK_OK;
}

extern "C" int pk_fs2_encode(pk_fs2* h, const int64_t* ids, const int32_t* tok_lens, int32_t B, float alpha,
                             int32_t* out_frames) {
    if (!h || !ids || !tok_lens || !out_frames) PK_FAIL(PK_EINVAL, "pk_fs2_encode: NULL argument");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_fs2_encode: call pk_fs2_finalize first");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_fs2_encode: batch size must be positive");
    if (!(alpha > 0.f)) PK_FAIL(PK_ESHAPE, "LengthRegulator: alpha must be > 0 (length_regulator.py:86)");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_fs2_cfg& c = h->cfg;
    const int A = c.adim;
    int maxT = 0;
    long sumT = 0;
    for (int b = 0; b < B; ++b) {
        if (tok_lens[b] <= 0) PK_FAIL(PK_EINVAL, "pk_fs2_encode: utterance %d has %d tokens", b, tok_lens[b]);
        maxT = std::max(maxT, tok_lens[b]);
        sumT += tok_lens[b];
    }
    h->encoded = false;
    // Per-call conditioning (pk_fs2_set_speakers / pk_fs2_set_tones) is taken off the handle FIRST, so that no
    // exit path -- error or success -- leaves it behind for an unrelated later encode, and its counts are
    // validated before anything is launched.
    const int condB = h->cond_B;
    std::vector<long long> cond_spk, cond_tone;
    std::vector<float> cond_emb;
    cond_spk.swap(h->cond_spk);
    cond_emb.swap(h->cond_emb);
    cond_tone.swap(h->cond_tone);
    h->cond_B = 0;
    std::vector<long long> tgt_dur;
    std::vector<float> tgt_pitch, tgt_energy;
    tgt_dur.swap(h->cond_dur);
    tgt_pitch.swap(h->cond_pitch);
    tgt_energy.swap(h->cond_energy);
    const bool has_dur = h->cond_has_dur, has_pitch = h->cond_has_pitch, has_energy = h->cond_has_energy;
    const long tgt_n = h->cond_tgt_n;
    h->cond_has_dur = h->cond_has_pitch = h->cond_has_energy = false;
    h->cond_tgt_n = 0;
    h->decoded = false;
    if ((has_dur || has_pitch || has_energy) && tgt_n != sumT)
        PK_FAIL(PK_ESHAPE, "pk_fs2_encode: targets were set for %ld tokens, batch has %ld", tgt_n, sumT);
    if (c.spk_embed_dim > 0 && condB > 0 && condB != B)
        PK_FAIL(PK_ESHAPE, "pk_fs2_encode: speakers were set for %d utterances, batch has %d", condB, B);
    if (c.tone_embed_dim > 0 && !cond_tone.empty() && (long)cond_tone.size() != sumT)
        PK_FAIL(PK_ESHAPE, "pk_fs2_encode: %zu tone ids for %ld tokens", cond_tone.size(), sumT);
    PK_TRY(pk_fft_build_timeline(ctx, h->tl_tok, tok_lens, B, h->gapr));
    Timeline& tl = h->tl_tok;
    PK_TRY(pk_fft_ensure_pe(h, maxT));
    // token ids on the row timeline
    {
        std::vector<int> tok(tl.rows_alloc, 0);
        long o = 0;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < tok_lens[b]; ++t, ++o) {
                const int64_t id = ids[o];
                if (id < 0 || id >= c.idim) PK_FAIL(PK_EINVAL, "pk_fs2_encode: token id %lld out of [0,%d)", (long long)id, c.idim);
                tok[tl.seg_start[b] + t] = (int)id;
            }
        PK_TRY(pk_upload(ctx, h->d_tok, tok.data(), tok.size() * sizeof(int)));
    }
    PK_TRY(pk_fft_act_reserve(h->d_x, tl.rows, A));
    PK_TRY(pk_fft_act_reserve(h->d_hs, tl.rows, A));
    float* x = pk_fft_act_ptr(h->d_x, A);
    float* hs = pk_fft_act_ptr(h->d_hs, A);
    PK_TRY(pk_fft_embed(h, "fs2_embed", h->d_tok.as<int>(), tl, h->emb_table, h->alpha_enc, h->xscale, x));
    PK_TRY(pk_fft_run_stack(h, h->enc, h->enc_after_g, h->enc_after_b, tl, c.eunits, hs, c.encoder_normalize_before != 0));
    // speaker embedding (:396-402)
    if (c.spk_embed_dim > 0 && condB > 0) {
        const int D = c.spk_embed_dim;
        const bool ext = !cond_emb.empty();
        const long long* d_id = nullptr;
        const float* d_emb = nullptr;
        if (ext) {
            PK_TRY(pk_upload(ctx, h->d_spk_emb, cond_emb.data(), cond_emb.size() * sizeof(float)));
            d_emb = h->d_spk_emb.as<float>();
        } else {
            PK_TRY(pk_upload(ctx, h->d_spk_id, cond_spk.data(), cond_spk.size() * sizeof(long long)));
            d_id = h->d_spk_id.as<long long>();
        }
        PK_TRY(pk_fft_run_speaker(h, tl, d_id, d_emb, h->spk_table, h->spk_w, h->spk_b,
                                  c.spk_embed_integration_type == 1 ? &h->spk_hs : nullptr, D, h->d_spk_vec, hs, x));
    }
    // tone embedding (:404-408)
    if (c.tone_embed_dim > 0 && !cond_tone.empty()) {
        const std::vector<long long>& ct = cond_tone;
        std::vector<int> tn(tl.rows_alloc, 0);
        long o = 0;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < tok_lens[b]; ++t, ++o) tn[tl.seg_start[b] + t] = (int)ct[o];
        PK_TRY(pk_upload(ctx, h->d_tone, tn.data(), tn.size() * sizeof(int)));
        PK_LAUNCH(ctx, "fs2_add_tone", k_add_tone, dim3(tl.rows), dim3(256), 0, hs, h->W(h->tone_table),
                  h->d_tone.as<int>(), tl.d_row_utt(), A);
    }
    // variance adaptor
    PK_TRY(h->d_pout.reserve((size_t)tl.rows_alloc * 4));
    PK_TRY(h->d_eout.reserve((size_t)tl.rows_alloc * 4));
    PK_TRY(h->d_dout.reserve((size_t)tl.rows_alloc * 4));
    PK_TRY(h->d_cum.reserve((size_t)tl.rows_alloc * 4));
    PK_TRY(h->d_frames.reserve((size_t)B * 4));
    h->hs_planes_valid = false;
    // given durations / pitch / energy (pk_fs2_set_targets; _forward's is_inference=False branch :433-442) go onto the token
    // timeline and stand in for the predictor's output where it is consumed; the predictors run all the same
    const float* dur_src = h->d_dout.as<float>();
    h->reg_pitch = h->d_pout.as<float>();
    h->reg_energy = h->d_eout.as<float>();
    if (has_dur || has_pitch || has_energy) {
        std::vector<float> row(tl.rows_alloc);
        auto place = [&](pk_dbuf& dst, auto&& value) -> int {
            std::fill(row.begin(), row.end(), 0.f);
            long o = 0;
            for (int b = 0; b < B; ++b)
                for (int t = 0; t < tok_lens[b]; ++t, ++o) row[tl.seg_start[b] + t] = value(o);
            return pk_upload(ctx, dst, row.data(), row.size() * sizeof(float));
        };
        if (has_dur) {
            PK_TRY(place(h->d_tdur, [&](long o) { return (float)tgt_dur[o]; }));
            dur_src = h->d_tdur.as<float>();
        }
        if (has_pitch) {
            PK_TRY(place(h->d_tpitch, [&](long o) { return tgt_pitch[o]; }));
            h->reg_pitch = h->d_tpitch.as<float>();
        }
        if (has_energy) {
            PK_TRY(place(h->d_tenergy, [&](long o) { return tgt_energy[o]; }));
            h->reg_energy = h->d_tenergy.as<float>();
        }
    }
    PK_TRY(run_predictor(h, h->pitch, tl, hs, 0, 1.f, h->d_pout.as<float>()));
    PK_TRY(run_predictor(h, h->energy, tl, hs, 0, 1.f, h->d_eout.as<float>()));
    // with given durations the head writes DurationPredictor.forward: log domain, masked, unrounded (duration_predictor.py:85-103)
    PK_TRY(run_predictor(h, h->dur, tl, hs, has_dur ? 0 : 1, alpha, h->d_dout.as<float>()));
    PK_LAUNCH(ctx, "fs2_cumsum", k_cumsum, dim3(B), dim3(256), 0, dur_src, tl.d_seg_start(),
              tl.d_seg_len(), h->d_cum.as<int>(), h->d_frames.as<int>());
    h->frames.resize(B);
    PK_HIP(hipMemcpyAsync(h->frames.data(), h->d_frames.p, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b) out_frames[b] = h->frames[b] * c.reduction_factor;   // mel frames; h->frames: decoder rows
    h->encoded = true;
    return PK_OK;
}

extern "C" int pk_fs2_decode(pk_fs2* h, float* mel_out, int32_t flags) {
    if (!h || !mel_out) PK_FAIL(PK_EINVAL, "pk_fs2_decode: NULL argument");
    if (!h->encoded) PK_FAIL(PK_ESTATE, "pk_fs2_decode: call pk_fs2_encode first");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_fs2_cfg& c = h->cfg;
    const int A = c.adim, B = h->tl_tok.B;
    // frame timeline; utterances with 0 frames get an empty segment
    std::vector<int> lens(h->frames);
    int maxL = 0;
    long sumL = 0;
    for (int b = 0; b < B; ++b) {
        maxL = std::max(maxL, lens[b]);
        sumL += lens[b];
    }
    if (sumL == 0) return PK_OK;
    PK_TRY(pk_fft_build_timeline(ctx, h->tl_frm, lens.data(), B, h->gapr));
    Timeline& tl = h->tl_frm;
    PK_TRY(pk_fft_ensure_pe(h, maxL));
    // packed output row of each timeline row
    {
        std::vector<int> rowmap(tl.rows_alloc, -1);
        int o = 0;
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < lens[b]; ++l) rowmap[tl.seg_start[b] + l] = o++;
        PK_TRY(pk_upload(ctx, h->d_rowmap, rowmap.data(), rowmap.size() * sizeof(int)));
    }
    // d_hs keeps the encoder output (token rate) until k_regulate has consumed it; d_x was the
    // encoder's residual stream and is free for the decoder.
    PK_TRY(pk_fft_act_reserve(h->d_x, tl.rows, A));
    float* x = pk_fft_act_ptr(h->d_x, A);
    const float* hs_tok = pk_fft_act_ptr(h->d_hs, A);
    float* up_dbg = nullptr;
    if (h->debug) {
        PK_TRY(pk_fft_act_reserve(h->d_dbg_up, tl.rows, A));
        up_dbg = pk_fft_act_ptr(h->d_dbg_up, A);
    }
    PK_LAUNCH(ctx, "fs2_regulate", k_regulate, dim3(tl.rows), dim3(128), 0, hs_tok, h->reg_pitch,
              h->reg_energy, h->W(h->pitch_w), h->W(h->pitch_b), h->W(h->energy_w), h->W(h->energy_b),
              h->d_cum.as<int>(), h->tl_tok.d_seg_start(), h->tl_tok.d_seg_len(), tl.d_row_utt(), tl.d_row_pos(),
              h->d_pe.as<float>(), h->alpha_dec, h->xscale, A, x, up_dbg);
    PK_TRY(pk_fft_act_reserve(h->d_zs, tl.rows, A));
    float* zs = pk_fft_act_ptr(h->d_zs, A);
    PK_TRY(pk_fft_run_stack(h, h->dec, h->dec_after_g, h->dec_after_b, tl, c.dunits, zs, c.decoder_normalize_before != 0));
    // feat_out (+ row mask: the postnet convolves over it)
    PK_TRY(pk_fft_act_reserve(h->d_before, tl.rows, c.odim));
    float* before = pk_fft_act_ptr(h->d_before, c.odim);
    float* d_out = mel_out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->d_mel_stage.reserve((size_t)sumL * c.odim * 4));
        d_out = h->d_mel_stage.as<float>();
    }
    const bool denorm = h->has_out_affine && (flags & PK_APPLY_NORMALIZER);   // FastSpeech2Inference (:668-671)
    const float* cs = denorm ? h->W(h->out_scale) : nullptr;
    const float* ch = denorm ? h->W(h->out_shift) : nullptr;
    if (c.reduction_factor > 1) {
        // feat_out -> (rows, odim * r), unfolded onto a timeline of rows * r frames for the postnet (:457-464)
        const int RF = c.reduction_factor, O = c.odim;
        PK_TRY(pk_fft_act_reserve(h->d_wide, tl.rows, O * RF));
        float* wide = pk_fft_act_ptr(h->d_wide, O * RF);
        PK_TRY(pk_fft_run_dense(h, "fs2_gemm_feat_out", h->feat_out, zs, A, wide, O * RF, tl.rows, PK_ACT_NONE, nullptr, 0, nullptr));
        std::vector<int> flens(B);
        long sumF = 0;
        for (int b = 0; b < B; ++b) {
            flens[b] = lens[b] * RF;
            sumF += flens[b];
        }
        PK_TRY(pk_fft_build_timeline(ctx, h->tl_frm2, flens.data(), B, h->gapr));
        Timeline& tf = h->tl_frm2;
        {
            std::vector<int> rowmap(tf.rows_alloc, -1);
            int o = 0;
            for (int b = 0; b < B; ++b)
                for (int l = 0; l < flens[b]; ++l) rowmap[tf.seg_start[b] + l] = o++;
            PK_TRY(pk_upload(ctx, h->d_rowmap2, rowmap.data(), rowmap.size() * sizeof(int)));
        }
        if (flags & PK_HOST_IO) {
            PK_TRY(h->d_mel_stage.reserve((size_t)sumF * O * 4));
            d_out = h->d_mel_stage.as<float>();
        }
        if (c.postnet_layers == 0) {
            PK_LAUNCH(ctx, "fs2_unfold", k_fs2_unfold_r, dim3(tf.rows), dim3(128), 0, wide, O, RF, tl.d_seg_start(), tf.d_row_utt(),
                      tf.d_row_pos(), h->d_rowmap2.as<int>(), cs, ch, d_out);
        } else {
            PK_TRY(pk_fft_act_reserve(h->d_before, tf.rows, O));
            float* before2 = pk_fft_act_ptr(h->d_before, O);
            PK_LAUNCH(ctx, "fs2_unfold", k_fs2_unfold_r, dim3(tf.rows), dim3(128), 0, wide, O, RF, tl.d_seg_start(), tf.d_row_utt(),
                      tf.d_row_pos(), (const int*)nullptr, (const float*)nullptr, (const float*)nullptr, before2);
            PK_TRY(pk_fft_run_postnet(h, "fs2_conv_postnet", h->postnet, before2, O, c.postnet_chans, tf, h->d_q1, h->d_q2, d_out,
                                      h->d_rowmap2.as<int>(), cs, ch));
        }
        if (flags & PK_HOST_IO) {
            PK_HIP(hipMemcpyAsync(mel_out, d_out, (size_t)sumF * O * 4, hipMemcpyDeviceToHost, ctx->stream));
            PK_HIP(hipStreamSynchronize(ctx->stream));
        }
        h->decoded = true;
        return PK_OK;
    }
    if (c.postnet_layers == 0) {
        pk_gemm_args g;
        g.A = zs; g.lda = A; g.Wp = h->W(h->feat_out.w); g.bias = h->W(h->feat_out.b);
        g.Wh = h->feat_out.wh == (size_t)-1 ? nullptr : h->arena16.as<uint16_t>() + h->feat_out.wh; g.math = h->math;
        g.C = d_out; g.ldc = c.odim; g.rowvalid = tl.d_row_utt(); g.cscale = cs; g.cshift = ch;
        g.out_rowmap = h->d_rowmap.as<int>(); g.M = tl.rows; g.N = c.odim; g.Cin = A; g.taps = 1; g.pad = 0;
        PK_TRY(pk_gemm_launch(ctx, "fs2_gemm_feat_out", g));
    } else {
        PK_TRY(pk_fft_run_dense(h, "fs2_gemm_feat_out", h->feat_out, zs, A, before, c.odim, tl.rows, PK_ACT_NONE, nullptr, 0,
                         tl.d_row_utt()));
        // after = before + postnet(before)  (:463-464), then ZScore.inverse (FastSpeech2Inference :670)
        PK_TRY(pk_fft_run_postnet(h, "fs2_conv_postnet", h->postnet, before, c.odim, c.postnet_chans, tl, h->d_q1, h->d_q2,
                                  d_out, h->d_rowmap.as<int>(), cs, ch));
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(mel_out, d_out, (size_t)sumL * c.odim * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    h->decoded = true;
    return PK_OK;
}

extern "C" int pk_fs2_read_before(pk_fs2* h, float* before_out, int32_t flags) {
    if (!h || !before_out) PK_FAIL(PK_EINVAL, "pk_fs2_read_before: NULL argument");
    if (!h->encoded) PK_FAIL(PK_ESTATE, "pk_fs2_read_before: call pk_fs2_encode and pk_fs2_decode first");
    const pk_fs2_cfg& c = h->cfg;
    if (c.postnet_layers == 0)
        PK_FAIL(PK_ESTATE, "pk_fs2_read_before: the model has no postnet, before_outs is the mel of pk_fs2_decode (fastspeech2.py:460-461)");
    long sumF = 0;
    for (int f : h->frames) sumF += (long)f * c.reduction_factor;
    if (sumF == 0) return PK_OK;
    if (!h->decoded) PK_FAIL(PK_ESTATE, "pk_fs2_read_before: call pk_fs2_decode first");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const bool wide = c.reduction_factor > 1;
    const Timeline& tl = wide ? h->tl_frm2 : h->tl_frm;
    const int* rowmap = wide ? h->d_rowmap2.as<int>() : h->d_rowmap.as<int>();
    float* d_out = before_out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->d_mel_stage.reserve((size_t)sumF * c.odim * 4));
        d_out = h->d_mel_stage.as<float>();
    }
    PK_LAUNCH(ctx, "fs2_pack_before", k_fs2_pack_rows, dim3(tl.rows), dim3(128), 0, pk_fft_act_ptr(h->d_before, c.odim), c.odim,
              rowmap, d_out);
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(before_out, d_out, (size_t)sumF * c.odim * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_fs2_set_targets(pk_fs2* h, const int64_t* durations, const float* pitch, const float* energy, int64_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_targets: handle is NULL");
    h->cond_dur.clear();
    h->cond_pitch.clear();
    h->cond_energy.clear();
    h->cond_has_dur = h->cond_has_pitch = h->cond_has_energy = false;
    h->cond_tgt_n = 0;
    if (!durations && !pitch && !energy) return PK_OK;
    if (n <= 0) PK_FAIL(PK_EINVAL, "pk_fs2_set_targets: n must be positive");
    if (durations)
        for (int64_t i = 0; i < n; ++i) {
            if (durations[i] < 0) PK_FAIL(PK_EINVAL, "pk_fs2_set_targets: duration %lld of token %lld is negative", (long long)durations[i], (long long)i);
            if (durations[i] > (1 << 20)) PK_FAIL(PK_EINVAL, "pk_fs2_set_targets: duration %lld of token %lld exceeds 2^20 frames", (long long)durations[i], (long long)i);
        }
    if (durations) h->cond_dur.assign(durations, durations + n);
    if (pitch) h->cond_pitch.assign(pitch, pitch + n);
    if (energy) h->cond_energy.assign(energy, energy + n);
    h->cond_has_dur = durations != nullptr;
    h->cond_has_pitch = pitch != nullptr;
    h->cond_has_energy = energy != nullptr;
    h->cond_tgt_n = (long)n;
    return PK_OK;
}

extern "C" int pk_fs2_read_predictions(pk_fs2* h, float* d_outs, float* p_outs, float* e_outs, int64_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_read_predictions: handle is NULL");
    if (!h->encoded) PK_FAIL(PK_ESTATE, "pk_fs2_read_predictions: call pk_fs2_encode first");
    const Timeline& tl = h->tl_tok;
    long sumT = 0;
    for (int b = 0; b < tl.B; ++b) sumT += tl.seg_len[b];
    if (n != sumT) PK_FAIL(PK_ESHAPE, "pk_fs2_read_predictions: expected %ld floats per array, got %lld", sumT, (long long)n);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<float> row(tl.rows);
    float* const dst[3] = {d_outs, p_outs, e_outs};
    const float* const src[3] = {h->d_dout.as<float>(), h->d_pout.as<float>(), h->d_eout.as<float>()};
    for (int k = 0; k < 3; ++k) {
        if (!dst[k]) continue;
        PK_HIP(hipMemcpy(row.data(), src[k], (size_t)tl.rows * sizeof(float), hipMemcpyDeviceToHost));
        long o = 0;
        for (int b = 0; b < tl.B; ++b)
            for (int t = 0; t < tl.seg_len[b]; ++t, ++o) dst[k][o] = row[tl.seg_start[b] + t];
    }
    return PK_OK;
}

extern "C" int pk_fs2_set_speakers(pk_fs2* h, const int64_t* spk_id, const float* spembs, int32_t B) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_speakers: handle is NULL");
    h->cond_B = 0;
    h->cond_spk.clear();
    h->cond_emb.clear();
    if (!spk_id && !spembs) return PK_OK;
    const pk_fs2_cfg& c = h->cfg;
    if (c.spk_embed_dim <= 0) return PK_OK;   // a single-speaker model ignores speakers, like the reference (:396)
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_fs2_set_speakers: batch size must be positive");
    if (spembs) {
        h->cond_emb.assign(spembs, spembs + (size_t)B * c.spk_embed_dim);
    } else {
        if (c.num_speakers <= 0) PK_FAIL(PK_ESTATE, "pk_fs2_set_speakers: the model has no spk_embedding_table");
        for (int b = 0; b < B; ++b)
            if (spk_id[b] < 0 || spk_id[b] >= c.num_speakers)
                PK_FAIL(PK_EINVAL, "pk_fs2_set_speakers: speaker id %lld out of [0,%d)", (long long)spk_id[b], c.num_speakers);
        h->cond_spk.assign(spk_id, spk_id + B);
    }
    h->cond_B = B;
    return PK_OK;
}

extern "C" int pk_fs2_set_tones(pk_fs2* h, const int64_t* tone_id, int64_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_tones: handle is NULL");
    h->cond_tone.clear();
    if (!tone_id || h->cfg.tone_embed_dim <= 0) return PK_OK;   // a model without tones ignores them (:404)
    if (n <= 0) PK_FAIL(PK_EINVAL, "pk_fs2_set_tones: n must be positive");
    for (int64_t i = 0; i < n; ++i)
        if (tone_id[i] < 0 || tone_id[i] >= h->cfg.num_tones)
            PK_FAIL(PK_EINVAL, "pk_fs2_set_tones: tone id %lld out of [0,%d)", (long long)tone_id[i], h->cfg.num_tones);
    h->cond_tone.assign(tone_id, tone_id + n);
    return PK_OK;
}

extern "C" int pk_fs2_set_math(pk_fs2* h, int32_t mode) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_math: handle is NULL");
    if (mode != PK_GEMM_MATH_F32 && mode != PK_GEMM_MATH_F16X3) PK_FAIL(PK_EINVAL, "pk_fs2_set_math: unknown mode %d", mode);
    h->math = mode;
    return PK_OK;
}

extern "C" int pk_fs2_set_option(pk_fs2* h, const char* key, int64_t value) {
    return pk_fft_set_option(h, key, value, "pk_fs2_set_option");
}

extern "C" int pk_fs2_set_debug(pk_fs2* h, int32_t on) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_fs2_set_debug: handle is NULL");
    h->debug = on != 0;
    return PK_OK;
}

extern "C" int pk_fs2_debug_read(pk_fs2* h, int32_t what, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_fs2_debug_read: NULL argument");
    if (!h->encoded) PK_FAIL(PK_ESTATE, "pk_fs2_debug_read: nothing has run");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const int A = h->cfg.adim;
    const Timeline* tl = &h->tl_tok;
    const float* src = nullptr;
    int C = A;
    switch (what) {
        case 0: src = pk_fft_act_ptr(h->d_hs, A); break;                           // encoder output hs (T, adim)
        case 1: src = h->d_pout.as<float>(); C = 1; break;                  // pitch (T,)
        case 2: src = h->d_eout.as<float>(); C = 1; break;                  // energy (T,)
        case 3: src = h->d_dout.as<float>(); C = 1; break;                  // durations (T,)
        case 4: tl = &h->tl_frm; src = pk_fft_act_ptr(h->d_dbg_up, A); break;      // length-regulated hs (L, adim)
        case 5: tl = &h->tl_frm; src = pk_fft_act_ptr(h->d_zs, A); break;      // decoder output zs (L, adim)
        case 6: tl = h->cfg.reduction_factor > 1 ? &h->tl_frm2 : &h->tl_frm; src = pk_fft_act_ptr(h->d_before, h->cfg.odim); C = h->cfg.odim; break;  // before_outs
        default: PK_FAIL(PK_EINVAL, "pk_fs2_debug_read: unknown tap %d", what);
    }
    if (b < 0 || b >= tl->B) PK_FAIL(PK_EINVAL, "pk_fs2_debug_read: utterance out of range");
    if (what == 4 && !h->debug) PK_FAIL(PK_ESTATE, "pk_fs2_debug_read: tap 4 needs pk_fs2_set_debug(1) before decode");
    const long n = (long)tl->seg_len[b] * C;
    if (n_floats != n) PK_FAIL(PK_ESHAPE, "pk_fs2_debug_read: expected %ld floats, got %lld", n, (long long)n_floats);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    if (n > 0)
        PK_HIP(hipMemcpy(host_out, src + (long)tl->seg_start[b] * C, n * sizeof(float), hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" void pk_fs2_destroy(pk_fs2* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->release_core();
    pk_dbuf* bufs[] = {&h->d_hsp, &h->d_hsam, &h->d_pp, &h->d_ppam, &h->d_pamax, &h->d_tok, &h->d_p1, &h->d_p2, &h->d_hs, &h->d_pout, &h->d_eout, &h->d_dout, &h->d_cum, &h->d_frames,
                       &h->d_tone, &h->d_spk_id, &h->d_spk_emb, &h->d_spk_vec, &h->d_before, &h->d_q1, &h->d_q2, &h->d_rowmap, &h->d_dbg_up, &h->d_zs, &h->d_mel_stage,
                       &h->d_wide, &h->d_rowmap2, &h->d_tdur, &h->d_tpitch, &h->d_tenergy};
    for (auto* b : bufs) b->release();
    h->tl_tok.release();
    h->tl_frm.release();
    h->tl_frm2.release();
    delete h;
}
