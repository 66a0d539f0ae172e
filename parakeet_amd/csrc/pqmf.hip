// pqmf.hip -- the pseudo-QMF analysis / synthesis bank of multi-band MelGAN on gfx950.  pk_pqmf.h defines the filters and
// the arithmetic (every product one fmaf, a fixed order); this file is its two vector-FMA kernels and the C ABI.
//
// Plain launches, no atomics; a workgroup computes PQMF_TILE outputs of ONE utterance from a window it staged in LDS itself:
// nothing depends on another utterance.
#include <cmath>
#include <exception>
#include <vector>

#include "pk_common.h"
#include "pk_pqmf.h"

namespace {

__device__ __forceinline__ int fdiv(int a, int b) {   // floor(a / b), b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// bands[k, m] = sum_n ana[k][n] * x[m K + n - h]
__global__ __launch_bounds__(PQMF_THREADS) void k_pqmf_analysis(const float* __restrict__ wav, float* __restrict__ bands,
                                                                const float* __restrict__ filt, const int* __restrict__ lensL,
                                                                const long* __restrict__ offL, const long* __restrict__ offB,
                                                                const int* __restrict__ tile0, const int* __restrict__ tile_b,
                                                                int K, int taps) {
    __shared__ float s_f[PQMF_LDS_FILT];
    __shared__ float s_w[PQMF_LDS_WIN_A];
    const int tid = threadIdx.x, tb = blockIdx.x, b = tile_b[tb];
    const int L = lensL[b], M = L / K, N = taps + 1, h = taps / 2;
    const int m0 = (tb - tile0[b]) * PQMF_TILE;
    const float* x = wav + offL[b];
    for (int i = tid; i < K * N; i += PQMF_THREADS) s_f[i] = filt[i];
    const int w0 = m0 * K - h, nw = (PQMF_TILE - 1) * K + N;   // <= PQMF_LDS_WIN_A
    for (int i = tid; i < nw; i += PQMF_THREADS) {
        const int g = w0 + i;
        s_w[i] = (unsigned)g < (unsigned)L ? x[g] : 0.f;
    }
    __syncthreads();
    const int m = m0 + tid;
    if (m >= M) return;
    float* out = bands + offB[b];
    for (int k = 0; k < K; ++k) {
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc = fmaf(s_f[k * N + n], s_w[tid * K + n], acc);
        out[(long)k * M + m] = acc;
    }
}

// wav[t] = K * sum_k sum_m syn[k][m K - t + h] * bands[k, m]
__global__ __launch_bounds__(PQMF_THREADS) void k_pqmf_synthesis(const float* __restrict__ bands, float* __restrict__ wav,
                                                                 const float* __restrict__ filt, const int* __restrict__ lens,
                                                                 const long* __restrict__ offs, const int* __restrict__ tile0,
                                                                 const int* __restrict__ tile_b, int K, int taps) {
    __shared__ float s_f[PQMF_LDS_FILT];
    __shared__ float s_w[PQMF_LDS_WIN_S];
    const int tid = threadIdx.x, tb = blockIdx.x, b = tile_b[tb];
    const int len = lens[b], M = len / K, N = taps + 1, h = taps / 2;
    const long off = offs[b];
    const int t0 = (tb - tile0[b]) * PQMF_TILE;
    for (int i = tid; i < K * N; i += PQMF_THREADS) s_f[i] = filt[i];
    const int mlo = fdiv(t0 - h + K - 1, K), mhi = fdiv(t0 + PQMF_TILE - 1 + h, K), nm = mhi - mlo + 1;   // nm K <= 255 + 2 h + 2 K
    const float* in = bands + off;
    for (int i = tid; i < K * nm; i += PQMF_THREADS) {
        const int k = i / nm, m = mlo + (i - k * nm);
        s_w[i] = (unsigned)m < (unsigned)M ? in[(long)k * M + m] : 0.f;
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t >= len) return;
    const int ma = fdiv(t - h + K - 1, K), mb = fdiv(t + h, K);
    float acc = 0.f;
    for (int k = 0; k < K; ++k)
        for (int m = ma; m <= mb; ++m) acc = fmaf(s_f[k * N + m * K - t + h], s_w[k * nm + m - mlo], acc);
    wav[off + t] = (float)K * acc;
}

}  // namespace

struct pk_pqmf {
    pk_ctx* ctx = nullptr;
    pk_pqmf_cfg cfg;
    std::vector<float> ana, syn;
    pk_dbuf d_ana, d_syn, ws_itab, ws_ltab, ws_in, ws_out;
};

extern "C" int pk_pqmf_create(pk_ctx* ctx, const pk_pqmf_cfg* cfg, pk_pqmf** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_pqmf_create: NULL argument");
    *out = nullptr;
    const pk_pqmf_cfg& c = *cfg;
    if (c.subbands < 2 || c.subbands > PQMF_MAX_K) PK_FAIL(PK_EUNSUPPORTED, "PQMF: subbands must be 2 ... %d (got %d)", PQMF_MAX_K, c.subbands);
    if (c.taps < 4 || c.taps > PQMF_MAX_TAPS || c.taps % 2 != 0)
        PK_FAIL(PK_EUNSUPPORTED, "PQMF: taps must be even, 4 ... %d (got %d)", PQMF_MAX_TAPS, c.taps);
    if (!(c.cutoff_ratio > 0.f && c.cutoff_ratio < 0.5f)) PK_FAIL(PK_EUNSUPPORTED, "PQMF: cutoff_ratio must lie in (0, 0.5) (got %g)", c.cutoff_ratio);
    if (!(c.beta >= 0.f) || !std::isfinite(c.beta) || c.beta > 700.f)
        PK_FAIL(PK_EUNSUPPORTED, "PQMF: beta must be 0 ... 700, where I0(beta) still is a float64 (got %g)", c.beta);
    pk_pqmf* q = nullptr;
    try {
        q = new pk_pqmf();
        q->ctx = ctx;
        q->cfg = c;
        pqmf_design(c.subbands, c.taps, (double)c.cutoff_ratio, (double)c.beta, q->ana, q->syn);
    } catch (const std::exception& e) {
        delete q;
        PK_FAIL(PK_ENOMEM, "pk_pqmf_create: %s", e.what());
    }
    PK_DEVICE(ctx->device);
    int st = pk_upload(ctx, q->d_ana, q->ana.data(), q->ana.size() * sizeof(float));
    if (st == PK_OK) st = pk_upload(ctx, q->d_syn, q->syn.data(), q->syn.size() * sizeof(float));
    if (st != PK_OK) {
        q->d_ana.release();
        q->d_syn.release();
        delete q;
        return st;
    }
    *out = q;
    return PK_OK;
}

extern "C" int pk_pqmf_filters(pk_pqmf* q, float* analysis_out, float* synthesis_out, int64_t n_floats) {
    if (!q || !analysis_out || !synthesis_out) PK_FAIL(PK_EINVAL, "pk_pqmf_filters: NULL argument");
    if (n_floats != (int64_t)q->ana.size()) PK_FAIL(PK_ESHAPE, "pk_pqmf_filters: expected %zu floats each", q->ana.size());
    memcpy(analysis_out, q->ana.data(), q->ana.size() * sizeof(float));
    memcpy(synthesis_out, q->syn.data(), q->syn.size() * sizeof(float));
    return PK_OK;
}

int pk_pqmf_subbands(const pk_pqmf* q) { return q->cfg.subbands; }

int pk_pqmf_launch_synthesis(pk_pqmf* q, pk_ctx* ctx, const float* bands, const int* lens, const long* offs, const int* tile0,
                             const int* tile_b, int ntiles, float* wav) {
    static_assert(PQMF_TILE - 1 + PQMF_MAX_TAPS + 2 * PQMF_MAX_K <= PQMF_LDS_WIN_S, "synthesis window");
    PK_LAUNCH(ctx, "pqmf_synthesis", k_pqmf_synthesis, dim3(ntiles), dim3(PQMF_THREADS), 0, bands, wav, q->d_syn.as<float>(), lens,
              offs, tile0, tile_b, q->cfg.subbands, q->cfg.taps);
    return PK_OK;
}

// tables of one call: ints lensL [B] | tile0 [B + 1] | tile_b [tiles]; longs offA [B] | offB [B].  `per_tile`: outputs an
// utterance of lens[b] input units produces; offA counts input units, offB output units.
static int pqmf_run(pk_pqmf* q, const char* who, bool analysis, const float* in, const int32_t* lens, int32_t B, float* out,
                    int32_t flags) {
    if (!q || !in || !lens || !out) PK_FAIL(PK_EINVAL, "%s: NULL argument", who);
    if (B <= 0) PK_FAIL(PK_EINVAL, "%s: batch size must be positive", who);
    pk_ctx* ctx = q->ctx;
    PK_DEVICE(ctx->device);
    const int K = q->cfg.subbands;
    std::vector<int> itab;
    std::vector<long> ltab;
    long nin = 0, nout = 0;
    int ntiles = 0;
    try {
        std::vector<int> lensT(B), tile0(B + 1);
        std::vector<long> offA(B), offB(B);
        for (int b = 0; b < B; ++b) {
            if (analysis ? lens[b] < K : lens[b] < 1)
                PK_FAIL(PK_EINVAL, analysis ? "%s: utterance %d is shorter than one band sample (%d samples, %d subbands)"
                                            : "%s: utterance %d has no band samples (%d; %d subbands)", who, b, lens[b], K);
            const long M = analysis ? lens[b] / K : lens[b];
            offA[b] = nin;
            offB[b] = nout;
            nin += analysis ? lens[b] : M * K;
            nout += M * K;
            if (nin > 0x3fffffffL) PK_FAIL(PK_EUNSUPPORTED, "%s: more than 2^30 samples in one call", who);
            lensT[b] = analysis ? lens[b] : (int)(M * K);     // analysis: L; synthesis: the output length K M
            tile0[b] = ntiles;
            ntiles += (int)(((analysis ? M : M * K) + PQMF_TILE - 1) / PQMF_TILE);
        }
        tile0[B] = ntiles;
        itab = lensT;
        itab.insert(itab.end(), tile0.begin(), tile0.end());
        for (int b = 0; b < B; ++b) itab.insert(itab.end(), (size_t)(tile0[b + 1] - tile0[b]), b);
        ltab = offA;
        ltab.insert(ltab.end(), offB.begin(), offB.end());
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "%s: host tables: %s", who, e.what());
    }
    PK_TRY(pk_upload(ctx, q->ws_itab, itab.data(), itab.size() * sizeof(int)));
    PK_TRY(pk_upload(ctx, q->ws_ltab, ltab.data(), ltab.size() * sizeof(long)));
    const bool host = (flags & PK_HOST_IO) != 0;
    const float* d_in = in;
    float* d_out = out;
    if (host) {
        PK_TRY(q->ws_in.reserve(nin * 4));
        PK_TRY(q->ws_out.reserve(nout * 4));
        PK_HIP(hipMemcpyAsync(q->ws_in.p, in, nin * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = q->ws_in.as<float>();
        d_out = q->ws_out.as<float>();
    }
    const int* it = q->ws_itab.as<int>();
    const long* lt = q->ws_ltab.as<long>();
    if (analysis) {
        static_assert((PQMF_TILE - 1) * PQMF_MAX_K + PQMF_MAX_TAPS + 1 <= PQMF_LDS_WIN_A, "analysis window");
        PK_LAUNCH(ctx, "pqmf_analysis", k_pqmf_analysis, dim3(ntiles), dim3(PQMF_THREADS), 0, d_in, d_out, q->d_ana.as<float>(), it,
                  lt, lt + B, it + B, it + 2 * B + 1, K, q->cfg.taps);
    } else {
        // bands and wav of an utterance start at the same offset (K M_b units each): offA == offB
        PK_TRY(pk_pqmf_launch_synthesis(q, ctx, d_in, it, lt + B, it + B, it + 2 * B + 1, ntiles, d_out));
    }
    if (host) {
        PK_HIP(hipMemcpyAsync(out, d_out, nout * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_pqmf_analysis(pk_pqmf* q, const float* wav, const int32_t* lens, int32_t B, float* bands_out, int32_t flags) {
    return pqmf_run(q, "pk_pqmf_analysis", true, wav, lens, B, bands_out, flags);
}

extern "C" int pk_pqmf_synthesis(pk_pqmf* q, const float* bands, const int32_t* band_lens, int32_t B, float* wav_out, int32_t flags) {
    return pqmf_run(q, "pk_pqmf_synthesis", false, bands, band_lens, B, wav_out, flags);
}

extern "C" void pk_pqmf_destroy(pk_pqmf* q) {
    if (!q) return;
    pk_device_guard _dg(q->ctx->device);
    (void)hipStreamSynchronize(q->ctx->stream);
    pk_dbuf* bufs[] = {&q->d_ana, &q->d_syn, &q->ws_itab, &q->ws_ltab, &q->ws_in, &q->ws_out};
    for (auto* b : bufs) b->release();
    delete q;
}
