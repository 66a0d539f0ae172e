// hifigan.hip -- the HiFi-GAN generator (Kong et al. 2020) on gfx950: every convolution of the stack on one MFMA kernel.
//
// Structure (restated from the paper with the module layout of the usual HiFiGANGenerator; include/pk_synth.h has the
// parameter names): input_conv, then per stage a transposed convolution (stride s, kernel 2 s) and nb residual blocks whose
// outputs are averaged, then LeakyReLU(0.01), output_conv and tanh.  Every convolution zero-pads its own input at the two
// ends of the utterance.
//
// The kernel k_hfg_conv, its boundary rule, epilogues and math are described in pk_hfg_conv.h, which MelGAN (melgan.hip) shares;
// this file uses its zero-padding instantiation alone.
//
// Plain launches only: no grid barrier, no persistent loop, no spinning.  An utterance's samples are the same bits alone, in
// any batch and at any position in it: nothing a workgroup computes depends on another utterance.
#include <cmath>
#include <exception>
#include <string>
#include <vector>

#include "pk_hfg_conv.h"

struct pk_hfg : hfg_engine {
    pk_hfg_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int hop = 1;
    bool use_norm = false;
    std::vector<hfg_conv> convs;   // input_conv | per stage: upsample, then blocks x dilations x (convs1[, convs2]) | output_conv
    pk_dbuf d_mu, d_sigma;
    pk_dbuf ws_mel, ws_act, ws_amax, ws_wav, ws_hostmel;
    int max_slots = 1;   // the most maxima one tile's producers write (output-channel groups x phases), over the model's convolutions
    // the last call, for pk_hfg_debug_read
    std::vector<int> last_frames;
    std::vector<long> last_off;
    bool last_valid = false;
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


static int hfg_finalize(pk_hfg* h) {
    pk_ctx* ctx = h->ctx;
    const pk_hfg_cfg& c = h->cfg;
    std::vector<float> f32, bias;
    std::vector<uint16_t> f16;
    h->convs.clear();
    h->max_slots = 1;
    auto add = [&](const std::string& name, int Cin, int Cout, int k, int dil, bool transposed, int s) -> int {
        int slots = 1;
        PK_TRY(hfg_add_conv(h->params, h->convs, f32, f16, bias, name, Cin, Cout, k, dil, transposed, s, &slots));
        h->max_slots = std::max(h->max_slots, slots);
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
    HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], 0, mel, *P, nullptr, HFG_EPI_STORE, 0, 1.f, 1.f, 1, true));
    for (int i = 0; i < S; ++i) {
        const int r = i + 1;
        HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], i, *P, *X, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
        const float inv_nb = 1.f / (float)c.n_blocks;
        for (int j = 0; j < c.n_blocks; ++j) {
            hfg_act* cur = X;
            const int nd = c.n_dilations[j];
            for (int n = 0; n < nd; ++n) {
                const bool last = n == nd - 1, fin = last && j == c.n_blocks - 1;
                if (c.use_additional_convs) {
                    HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], r, *cur, *T, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
                    hfg_act* dst = last ? Sm : Y;   // Y in place when cur is Y: a thread reads res[o], then writes out[o]
                    HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], r, *T, *dst, cur->p, last ? HFG_EPI_SUM : HFG_EPI_RES, j == 0, inv_nb,
                                      slope, 0, last ? fin : true));
                    cur = Y;
                } else {
                    hfg_act* dst = last ? Sm : (cur == Y ? T : Y);
                    HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], r, *cur, *dst, cur->p, last ? HFG_EPI_SUM : HFG_EPI_RES, j == 0, inv_nb,
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
    HFG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], S, *P, wav, nullptr, HFG_EPI_TANH, 0, 1.f, HFG_OUTPUT_SLOPE, 0, false));
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
        PK_TRY(hfg_tables(h, "pk_hfg_infer", frames, B, h->cfg.upsample_scales, h->cfg.n_upsample + 1));
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
        st = hfg_tables(h, who, &one, 1, c.upsample_scales, c.n_upsample + 1);
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
    hfg_engine_release(h);
    pk_dbuf* bufs[] = {&h->d_mu, &h->d_sigma, &h->ws_mel, &h->ws_act, &h->ws_amax, &h->ws_wav, &h->ws_hostmel};
    for (auto* b : bufs) b->release();
    delete h;
}
