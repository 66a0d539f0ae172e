// melgan.hip -- the MelGAN / multi-band MelGAN generator on gfx950: every convolution of the stack on the MFMA kernel that
// HiFi-GAN runs on (pk_hfg_conv.h), the padded ones under its reflecting boundary rule.
//
// Structure (the module layout of the usual MelGANGenerator, AS RECALLED: NEITHER THE PARAMETER NAMES NOR THE LAYOUT COULD BE
// CHECKED AGAINST A RELEASED CHECKPOINT; include/pk_synth.h has both): a reflection-padded input convolution; per stage
// LeakyReLU, a transposed convolution (stride s, kernel 2 s) and S residual stacks; LeakyReLU, a reflection-padded output
// convolution to out_channels, tanh.  A residual stack x -> Conv1x1(a(Conv_(k, d)(R(a(x))))) + Conv1x1_skip(x) is three
// launches of the kernel:
//   1. t = the dilated convolution of a(x), HFG_BND_REFLECT
//   2. sk = the skip convolution of x: slope 1, under which the kernel's LeakyReLU select is the identity
//   3. x' = the 1x1 convolution of a(t), its residual epilogue adding sk; written in place of sk (a thread reads res[o], then
//      writes out[o])
// Transposed and 1x1 convolutions run in HFG_BND_ZERO: they read no position outside the utterance (the transposed one's
// two out-of-range neighbours ARE zero in its definition).
//
// Reflection needs pad < length at every padded convolution; min_frames is the smallest frame count for which that holds,
// and a shorter utterance is refused -- never clamped.
//
// With a PQMF bank attached (pk_mgan_set_pqmf) the sub-bands (out_channels, L) of an utterance, which the output convolution
// writes channel-major, are the synthesis kernel's input as they lie; its tables are one more rate of this call's tables.
//
// Plain launches only, no atomics.  An utterance's samples are the same bits alone, in any batch and at any position in it.
#include <cmath>
#include <exception>
#include <string>
#include <vector>

#include "pk_hfg_conv.h"
#include "pk_pqmf.h"

struct pk_mgan : hfg_engine {
    pk_mgan_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int hop = 1, min_frames = 1;
    bool use_norm = false;
    pk_pqmf* pqmf = nullptr;
    std::vector<hfg_conv> convs;   // input | per stage: transposed, then stacks x (dilated, skip, 1x1) | output
    pk_dbuf d_mu, d_sigma;
    pk_dbuf ws_mel, ws_act, ws_amax, ws_out, ws_sub, ws_hostmel;
    int max_slots = 1;
    int32_t rates[PK_MGAN_MAX_STAGES + 1];   // the scales, then out_channels: the last rate is the bank's output
    std::vector<int> last_frames;
    std::vector<long> last_off;
    bool last_valid = false;
};

static int mg_ch(const pk_mgan_cfg& c, int i) { return c.channels >> i; }

static int mg_pad(const pk_mgan_cfg& c, int j) {   // the reflection pad of stack j
    int d = 1;
    for (int q = 0; q < j; ++q) d *= c.stack_kernel_size;
    return (c.stack_kernel_size - 1) / 2 * d;
}

extern "C" int pk_mgan_create(pk_ctx* ctx, const pk_mgan_cfg* cfg, pk_mgan** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_mgan_create: NULL argument");
    *out = nullptr;
    const pk_mgan_cfg& c = *cfg;
    if (c.in_channels < 1 || c.in_channels > 512) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: in_channels must be 1 ... 512 (got %d)", c.in_channels);
    if (c.out_channels < 1 || c.out_channels > 16) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: out_channels must be 1 ... 16 (got %d)", c.out_channels);
    if (c.kernel_size < 3 || c.kernel_size > 11 || c.kernel_size % 2 == 0)
        PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: kernel_size must be odd, 3 ... 11 (got %d)", c.kernel_size);
    if (c.n_upsample < 1 || c.n_upsample > PK_MGAN_MAX_STAGES)
        PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: 1 ... %d upsample stages (got %d)", PK_MGAN_MAX_STAGES, c.n_upsample);
    long hop = 1;
    for (int i = 0; i < c.n_upsample; ++i) {
        const int s = c.upsample_scales[i];
        if (s < 2 || s > 16) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: upsample_scales must be 2 ... 16 (got %d)", s);
        hop *= s;
    }
    if (c.channels < 8 || c.channels > 512) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: channels must be 8 ... 512 (got %d)", c.channels);
    for (int i = 0; i <= c.n_upsample; ++i)
        if (mg_ch(c, i) < 8 || mg_ch(c, i) % 8 != 0 || (mg_ch(c, i) << i) != c.channels)
            PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: channels >> %d = %d must be a multiple of 8 in 8 ... 512 (channels %d)", i,
                    mg_ch(c, i), c.channels);
    if (c.stacks < 1 || c.stacks > 6) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: stacks must be 1 ... 6 (got %d)", c.stacks);
    if (c.stack_kernel_size < 3 || c.stack_kernel_size > 7 || c.stack_kernel_size % 2 == 0)
        PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: stack_kernel_size must be odd, 3 ... 7 (got %d)", c.stack_kernel_size);
    {
        long pad = (c.stack_kernel_size - 1) / 2;
        for (int j = 1; j < c.stacks; ++j) pad *= c.stack_kernel_size;
        if (pad > HFG_MAX_HALO)
            PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator: (stack_kernel_size - 1) / 2 * stack_kernel_size^(stacks - 1) must be at most %d "
                    "(kernel %d, %d stacks: %ld)", HFG_MAX_HALO, c.stack_kernel_size, c.stacks, pad);
    }
    if (!c.bias) PK_FAIL(PK_EUNSUPPORTED, "MelGANGenerator(bias=False) is not implemented");
    if (!std::isfinite(c.negative_slope)) PK_FAIL(PK_EINVAL, "MelGANGenerator: negative_slope is not finite");
    pk_mgan* h = new pk_mgan();
    h->ctx = ctx;
    h->cfg = c;
    h->hop = (int)hop;
    // the smallest frame count with every reflection pad below the length it pads
    long need = (c.kernel_size - 1) / 2 + 1, mul = 1;
    for (int i = 0; i < c.n_upsample; ++i) {
        mul *= c.upsample_scales[i];
        h->rates[i] = c.upsample_scales[i];
        need = std::max(need, (mg_pad(c, c.stacks - 1) + 1 + mul - 1) / mul);
    }
    need = std::max(need, ((c.kernel_size - 1) / 2 + 1 + mul - 1) / mul);
    h->rates[c.n_upsample] = c.out_channels;
    h->min_frames = (int)need;
    *out = h;
    return PK_OK;
}

extern "C" int pk_mgan_set_param(pk_mgan* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mgan_set_param: handle is NULL");
    h->finalized = false;
    h->last_valid = false;
    return pk_store_param(h->params, name, data, shape, ndim);
}

extern "C" int pk_mgan_set_math(pk_mgan* h, int32_t mode) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mgan_set_math: handle is NULL");
    if (mode == PK_PWG_MATH_BF16X3) PK_FAIL(PK_EUNSUPPORTED, "pk_mgan_set_math: the MelGAN generator has no split-bf16 variant");
    if (mode != PK_PWG_MATH_F32 && mode != PK_PWG_MATH_F16X3) PK_FAIL(PK_EINVAL, "pk_mgan_set_math: unknown mode %d", mode);
    h->math = mode;
    return PK_OK;
}

extern "C" int pk_mgan_set_normalizer(pk_mgan* h, const float* mu, const float* sigma, int32_t n) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mgan_set_normalizer: handle is NULL");
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

extern "C" int32_t pk_mgan_min_frames(const pk_mgan* h) { return h ? h->min_frames : 0; }

extern "C" int pk_mgan_set_pqmf(pk_mgan* h, pk_pqmf* pqmf) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mgan_set_pqmf: handle is NULL");
    if (pqmf && pk_pqmf_subbands(pqmf) != h->cfg.out_channels)
        PK_FAIL(PK_EINVAL, "pk_mgan_set_pqmf: the bank has %d subbands, the generator %d output channels", pk_pqmf_subbands(pqmf),
                h->cfg.out_channels);
    h->pqmf = pqmf;
    h->last_valid = false;
    return PK_OK;
}

static int mg_finalize(pk_mgan* h) {
    pk_ctx* ctx = h->ctx;
    const pk_mgan_cfg& c = h->cfg;
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
    const int S = c.stacks;
    PK_TRY(add("melgan.1", c.in_channels, c.channels, c.kernel_size, 1, false, 1));
    for (int i = 0; i < c.n_upsample; ++i) {
        const int q = 2 + i * (2 + S), C = mg_ch(c, i + 1);
        PK_TRY(add("melgan." + std::to_string(q + 1), mg_ch(c, i), C, 2 * c.upsample_scales[i], 1, true, c.upsample_scales[i]));
        int d = 1;
        for (int j = 0; j < S; ++j) {
            const std::string base = "melgan." + std::to_string(q + 2 + j);
            PK_TRY(add(base + ".stack.2", C, C, c.stack_kernel_size, d, false, 1));
            PK_TRY(add(base + ".skip_layer", C, C, 1, 1, false, 1));
            PK_TRY(add(base + ".stack.4", C, C, 1, 1, false, 1));
            d *= c.stack_kernel_size;
        }
    }
    PK_TRY(add("melgan." + std::to_string(2 + c.n_upsample * (2 + S) + 2), mg_ch(c, c.n_upsample), c.out_channels, c.kernel_size, 1,
               false, 1));
    PK_TRY(pk_upload(ctx, h->d_w32, f32.data(), f32.size() * sizeof(float)));
    PK_TRY(pk_upload(ctx, h->d_w16, f16.data(), f16.size() * sizeof(uint16_t)));
    PK_TRY(pk_upload(ctx, h->d_bias, bias.data(), bias.size() * sizeof(float)));
    h->finalized = true;
    return PK_OK;
}

extern "C" int pk_mgan_finalize(pk_mgan* h) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mgan_finalize: handle is NULL");
    PK_DEVICE(h->ctx->device);
    try {
        return mg_finalize(h);
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_mgan_finalize: host tables: %s", e.what());
    }
}

// The stack over the call whose tables are on the device, from the prepared mel `d_mel` (its tile maxima in d_mel_amax).
// upto < 0: through the output convolution into d_out; else stop after stage `upto` and return its output buffer.
#define MG_STEP(call)                     \
    do {                                  \
        PK_TRY(call);                     \
        if (h->dbg_ptr) return PK_OK;     \
    } while (0)
static int mg_chain(pk_mgan* h, const float* d_mel, float* d_mel_amax, float* d_out, int upto, const float** stage_out) {
    const pk_mgan_cfg& c = h->cfg;
    const int n = c.n_upsample;
    size_t maxsz = (size_t)c.channels * h->sumL[0];
    for (int i = 0; i < n; ++i) maxsz = std::max(maxsz, (size_t)mg_ch(c, i + 1) * h->sumL[i + 1]);
    maxsz = (maxsz + 63) / 64 * 64;
    if ((long)(maxsz * 4 * sizeof(float)) > HFG_WORKSPACE_CAP)
        PK_FAIL(PK_ENOMEM, "pk_mgan_infer: the call needs %zu MiB of activations, more than the %ld MiB a call may take: split the batch",
                maxsz * 4 * sizeof(float) >> 20, HFG_WORKSPACE_CAP >> 20);
    const size_t asz = (size_t)h->ntiles[n] * h->max_slots;   // a producer's grid has at most the last convolution rate's tiles
    PK_TRY(h->ws_act.reserve(maxsz * 4 * sizeof(float)));
    PK_TRY(h->ws_amax.reserve(asz * 4 * sizeof(float)));
    hfg_act buf[4];
    for (int i = 0; i < 4; ++i) {
        buf[i].p = h->ws_act.as<float>() + maxsz * i;
        buf[i].amax = h->ws_amax.as<float>() + asz * i;
    }
    hfg_act *P = &buf[0], *X = &buf[1], *T = &buf[2], *Y = &buf[3];
    hfg_act mel;
    mel.p = const_cast<float*>(d_mel);
    mel.amax = d_mel_amax;
    mel.nsl = 1;
    mel.grate = 0;
    const float slope = c.negative_slope;
    size_t ci = 0;
    h->dbg_count = 0;
    h->dbg_ptr = nullptr;
    MG_STEP(hfg_launch<HFG_BND_REFLECT>(h, h->convs[ci++], 0, mel, *P, nullptr, HFG_EPI_STORE, 0, 1.f, 1.f, 1, true));
    for (int i = 0; i < n; ++i) {
        const int r = i + 1;
        MG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], i, *P, *X, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
        for (int j = 0; j < c.stacks; ++j) {
            MG_STEP(hfg_launch<HFG_BND_REFLECT>(h, h->convs[ci++], r, *X, *T, nullptr, HFG_EPI_STORE, 0, 1.f, slope, 0, true));
            MG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], r, *X, *Y, nullptr, HFG_EPI_STORE, 0, 1.f, 1.f, 0, false));
            MG_STEP(hfg_launch<HFG_BND_ZERO>(h, h->convs[ci++], r, *T, *Y, Y->p, HFG_EPI_RES, 0, 1.f, slope, 0, true));
            std::swap(X, Y);
        }
        std::swap(P, X);   // the last stack's output is the next stage's input
        if (upto == i) {
            *stage_out = P->p;
            return PK_OK;
        }
    }
    hfg_act o;
    o.p = d_out;
    MG_STEP(hfg_launch<HFG_BND_REFLECT>(h, h->convs[ci++], n, *P, o, nullptr, c.use_final_nonlinear_activation ? HFG_EPI_TANH : HFG_EPI_STORE,
                                        0, 1.f, slope, 0, false));
    return PK_OK;
}
#undef MG_STEP

extern "C" int pk_mgan_infer(pk_mgan* h, const float* mel, const int32_t* frames, int32_t B, float* out, int32_t flags) {
    if (!h || !mel || !frames || !out) PK_FAIL(PK_EINVAL, "pk_mgan_infer: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_mgan_infer: batch size must be positive");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_mgan_infer: call pk_mgan_finalize first");
    for (int b = 0; b < B; ++b)
        if (frames[b] < h->min_frames)
            PK_FAIL(PK_EINVAL, "pk_mgan_infer: utterance %d has %d frames; reflection padding needs at least min_frames = %d", b, frames[b],
                    h->min_frames);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    h->last_valid = false;
    const pk_mgan_cfg& c = h->cfg;
    const int n = c.n_upsample;
    try {
        PK_TRY(hfg_tables(h, "pk_mgan_infer", frames, B, h->rates, n + 2));
        h->last_frames.assign(frames, frames + B);
        h->last_off.assign(B, 0);
        for (int b = 1; b < B; ++b) h->last_off[b] = h->last_off[b - 1] + frames[b - 1];
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "pk_mgan_infer: host tables: %s", e.what());
    }
    const bool host = (flags & PK_HOST_IO) != 0;
    const size_t nmel = (size_t)h->sumL[0] * c.in_channels, nout = (size_t)h->sumL[n + 1];   // = sumL[n] * out_channels either way
    const float* d_in = mel;
    float* d_out = out;
    if (host) {
        PK_TRY(h->ws_hostmel.reserve(nmel * 4));
        PK_HIP(hipMemcpyAsync(h->ws_hostmel.p, mel, nmel * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = h->ws_hostmel.as<float>();
        PK_TRY(h->ws_out.reserve(nout * 4));
        d_out = h->ws_out.as<float>();
    }
    float* d_sub = d_out;   // what the output convolution writes
    if (h->pqmf) {
        PK_TRY(h->ws_sub.reserve(nout * 4));
        d_sub = h->ws_sub.as<float>();
    }
    // the prepared mel and its tile maxima stay in the handle for the test taps
    PK_TRY(h->ws_mel.reserve((nmel + (size_t)h->ntiles[0] + 64) * 4));
    float* d_mel = h->ws_mel.as<float>();
    float* d_mel_amax = d_mel + (nmel + 63) / 64 * 64;
    const int* itab = h->ws_itab.as<int>();
    PK_LAUNCH(ctx, "mgan_prep", k_hfg_prep, dim3(h->ntiles[0]), dim3(HFG_THREADS), 0, d_in, d_mel, h->d_mu.as<float>(),
              h->d_sigma.as<float>(), (h->use_norm && (flags & PK_APPLY_NORMALIZER)) ? 1 : 0, itab + h->o_lens[0],
              h->ws_ltab.as<long>() + h->o_offs[0], itab + h->o_tile0[0], itab + h->o_tileb[0], c.in_channels, d_mel_amax);
    PK_TRY(mg_chain(h, d_mel, d_mel_amax, d_sub, -1, nullptr));
    if (h->pqmf) {
        static_assert(PQMF_TILE == HFG_TILE, "the bank's tiles are this call's tables of the last rate");
        PK_TRY(pk_pqmf_launch_synthesis(h->pqmf, ctx, d_sub, itab + h->o_lens[n + 1], h->ws_ltab.as<long>() + h->o_offs[n + 1],
                                        itab + h->o_tile0[n + 1], itab + h->o_tileb[n + 1], h->ntiles[n + 1], d_out));
    }
    h->last_valid = true;
    if (host) {
        PK_HIP(hipMemcpyAsync(out, d_out, nout * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

// the same kernels over utterance b of the last call alone (its tiles and scales are those of the batch), stopped after
// stage `stage` (>= 0) or after launch `launch` (>= 0): -> the buffer written last, its channels and positions
static int mg_debug_run(pk_mgan* h, const char* who, int stage, int launch, int b, const float** ptr, int* C, long* len) {
    if (!h->last_valid || !h->finalized) PK_FAIL(PK_ESTATE, "%s: no pk_mgan_infer since the parameters were set", who);
    const pk_mgan_cfg& c = h->cfg;
    if (b < 0 || b >= (int)h->last_frames.size()) PK_FAIL(PK_EINVAL, "%s: utterance out of range", who);
    const std::vector<int> keep_frames = h->last_frames;
    const std::vector<long> keep_off = h->last_off;
    const int32_t one = keep_frames[b];
    long tile_first = 0, total = 0;
    for (int q = 0; q < b; ++q) tile_first += (keep_frames[q] + HFG_TILE - 1) / HFG_TILE;
    for (size_t q = 0; q < keep_frames.size(); ++q) total += keep_frames[q];
    const size_t nmel = (size_t)total * c.in_channels;
    float* d_mel_all = h->ws_mel.as<float>();
    float* d_amax_all = d_mel_all + (nmel + 63) / 64 * 64;
    int st;
    try {
        st = hfg_tables(h, who, &one, 1, h->rates, c.n_upsample + 2);
    } catch (const std::exception& e) {
        pk_set_error("%s: host tables: %s", who, e.what());
        st = PK_ENOMEM;
    }
    PK_TRY(st);
    // From here the handle's device tables, ntiles and sumL are those of this ONE utterance (last_frames / last_off keep the
    // batch on the host): every entry point rebuilds them before it launches.
    PK_TRY(h->ws_sub.reserve((size_t)h->sumL[c.n_upsample + 1] * 4));
    const float* d_stage = nullptr;
    h->dbg_stop = launch;
    st = mg_chain(h, d_mel_all + keep_off[b] * c.in_channels, d_amax_all + tile_first, h->ws_sub.as<float>(), stage, &d_stage);
    h->dbg_stop = -1;
    PK_TRY(st);
    if (launch >= 0) {
        if (!h->dbg_ptr) PK_FAIL(PK_EINVAL, "%s: launch %d out of range (the model has %d)", who, launch, h->dbg_count);
        *ptr = h->dbg_ptr;
        *C = h->dbg_C;
        *len = h->sumL[h->dbg_rate];
        h->dbg_ptr = nullptr;
    } else {
        *ptr = d_stage;
        *C = mg_ch(c, stage + 1);
        *len = h->sumL[stage + 1];
    }
    return PK_OK;
}

extern "C" int pk_mgan_debug_read(pk_mgan* h, int32_t stage, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_mgan_debug_read: NULL argument");
    if (stage < 0 || stage >= h->cfg.n_upsample)
        PK_FAIL(PK_EINVAL, "pk_mgan_debug_read: stage %d out of range (the model has %d)", stage, h->cfg.n_upsample);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const float* p = nullptr;
    int C = 0;
    long len = 0;
    PK_TRY(mg_debug_run(h, "pk_mgan_debug_read", stage, -1, b, &p, &C, &len));
    if (n_floats != (int64_t)C * len) PK_FAIL(PK_ESHAPE, "pk_mgan_debug_read: expected %ld floats", (long)C * len);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    PK_HIP(hipMemcpy(host_out, p, (size_t)C * len * 4, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" int pk_mgan_debug_conv(pk_mgan* h, int32_t launch, int32_t b, float* host_out, int64_t n_floats) {
    if (!h || !host_out) PK_FAIL(PK_EINVAL, "pk_mgan_debug_conv: NULL argument");
    if (launch < 0 || launch >= (int)h->convs.size())
        PK_FAIL(PK_EINVAL, "pk_mgan_debug_conv: launch %d out of range (the model has %d)", launch, (int)h->convs.size());
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const float* p = nullptr;
    int C = 0;
    long len = 0;
    PK_TRY(mg_debug_run(h, "pk_mgan_debug_conv", -1, launch, b, &p, &C, &len));
    if (n_floats != (int64_t)C * len) PK_FAIL(PK_ESHAPE, "pk_mgan_debug_conv: expected %ld floats", (long)C * len);
    PK_HIP(hipStreamSynchronize(ctx->stream));
    PK_HIP(hipMemcpy(host_out, p, (size_t)C * len * 4, hipMemcpyDeviceToHost));
    return PK_OK;
}

extern "C" void pk_mgan_destroy(pk_mgan* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    hfg_engine_release(h);
    pk_dbuf* bufs[] = {&h->d_mu, &h->d_sigma, &h->ws_mel, &h->ws_act, &h->ws_amax, &h->ws_out, &h->ws_sub, &h->ws_hostmel};
    for (auto* b : bufs) b->release();
    delete h;
}
