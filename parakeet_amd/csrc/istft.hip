// istft.hip -- inverse STFT and fast Griffin-Lim on gfx950 (the way back from mel.hip).
//
// Reference: parakeet/audio/audio.py AudioProcessor.istft :86-93, which is librosa.istft: every frame is
// irfft(D[:, f], n_fft) * window, frames are overlap-added at stride hop, every sample is divided by the overlap-added
// window^2 where that envelope exceeds FLT_MIN, and with center n_fft/2 samples are cut from both ends.  The Griffin-Lim loop
// is librosa.griffinlim (Perraudin, Balazs, Sondergaard, "A fast Griffin-Lim algorithm", WASPAA 2013).
//
// The inverse real DFT with the synthesis window folded in is a GEMM: [frames x K] . [K x n_fft], K = 2*n_bin padded to 16,
// A rows = re | im of a frame, on the exact-fp32 k_gemm like the forward transform.  The product leaves a (frames, n_fft)
// buffer; k_istft_ola GATHERS it: a thread owns four consecutive output samples and adds up the at most ceil(n_fft / hop)
// frames that overlap them in ascending frame order -- no atomics, a fixed order, nothing shared between utterances, so an
// utterance's samples do not depend on the batch they are computed in.
//
// Under PK_TRANSFORM_FFT (pk_istft_set_transform) the frame buffer comes from the inverse radix FFT of rfft.hip instead of the
// product, and the Griffin-Lim loop's forward transform from its forward kernel; every other kernel here is the same.
#include <cfloat>
#include <cmath>
#include <vector>

#include "pk_gemm.h"
#include "pk_mel.h"
#include "pk_mfma.h"
#include "pk_philox.h"
#include "pk_rfft.h"

namespace {

constexpr unsigned PK_GL_STREAM = 0x474C5048u;   // "GLPH": counter word 3 of the initial-phase stream
constexpr int OLA_SPT = 4;                        // samples per thread (one 16-byte access)
constexpr int OLA_BLOCK = 256;

struct istft_utt {
    long ooff;     // where sample `trim` of the overlap-added signal goes in the output
    int row0;      // first row of the utterance in the frame buffer
    int frames;
};

// A[r][c] = spec[r][c] with im(DC), im(Nyquist) and the K padding zeroed (numpy.fft.irfft ignores the two; a NaN there
// must not reach the product through a zero basis row)
__global__ void k_istft_pack(const float* __restrict__ spec, int nb, float* __restrict__ A, int K) {
    const long r = blockIdx.x;
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= K) return;
    float v = 0.f;
    if (c < 2 * nb && c != nb && c != 2 * nb - 1) v = spec[r * (2 * nb) + c];
    A[r * K + c] = v;
}

// Overlap-add as a gather.  blockIdx.y = utterance, a block covers 1024 consecutive samples, a wave 256 of them: for every
// frame its 64 lanes read 1 KiB of consecutive floats of that frame's row.  n counts samples of the untrimmed signal
// (n_fft + hop * (frames - 1) long); n, hop, n_fft and trim are multiples of 4, so the four samples of a thread share
// their frame range [ceil((n - n_fft + 1) / hop), floor(n / hop)] and every access is 16-byte aligned.
__global__ __launch_bounds__(OLA_BLOCK) void k_istft_ola(const float* __restrict__ fr, const float* __restrict__ window,
                                                         const istft_utt* __restrict__ tab, int N, int hop, int trim,
                                                         int vec_store, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float w2[];   // window^2
    for (int i = threadIdx.x; i < N; i += OLA_BLOCK) {
        const float w = window[i];
        w2[i] = w * w;
    }
    __syncthreads();
    const istft_utt u = tab[blockIdx.y];
    const long total = (long)N + (long)hop * (u.frames - 1);
    const long n = trim + ((long)blockIdx.x * OLA_BLOCK + threadIdx.x) * OLA_SPT;
    if (n >= total - trim) return;
    const int f_hi = n / hop < u.frames ? (int)(n / hop) : u.frames - 1;
    const int f_lo = n < N ? 0 : (int)((n - N + hop) / hop);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, env = {0.f, 0.f, 0.f, 0.f};
    int k = (int)(n - (long)f_lo * hop);                          // position inside frame f_lo; < n_fft
    const float* p = fr + ((long)u.row0 + f_lo) * N + k;
    for (int f = f_lo; f <= f_hi; ++f) {
        acc += *reinterpret_cast<const f32x4*>(p);
        env += *reinterpret_cast<const f32x4*>(w2 + k);
        p += N - hop;
        k -= hop;
    }
#pragma unroll
    for (int j = 0; j < OLA_SPT; ++j)
        if (env[j] > FLT_MIN) acc[j] = acc[j] / env[j];
    float* o = out + u.ooff + (n - trim);
    if (vec_store) {
        *reinterpret_cast<f32x4*>(o) = acc;
    } else {
#pragma unroll
        for (int j = 0; j < OLA_SPT; ++j) o[j] = acc[j];
    }
}

// Reflect padding of the forward STFT (F.pad mode='reflect'), in place on the padded-signal axis: k_istft_ola has written
// the L centre samples of utterance b at ooff[b]; the n_fft/2 samples on either side mirror them.
__global__ void k_gl_reflect_edges(float* __restrict__ xpad, const istft_utt* __restrict__ tab, int hop, int pad) {
    const istft_utt u = tab[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * pad) return;
    const long L = (long)hop * (u.frames - 1);
    float* y = xpad + u.ooff;                                     // y[s], s in [0, L): the signal itself
    const long s = j < pad ? (long)j - pad : L + (j - pad);
    y[s] = y[s < 0 ? -s : 2 * (L - 1) - s];
}

// A[r] = S[r] * angles[r] as re | im.  angles == NULL: exp(2 pi i u), u = word * 2^-32, word (bin & 3) of the Philox block
// with counter (frame inside its utterance, bin >> 2, 0, "GLPH") and the utterance's seed as the key.
__global__ void k_gl_apply(const float* __restrict__ S, const float* __restrict__ angles, const int* __restrict__ rowframe,
                           const int* __restrict__ rowutt, const unsigned long long* __restrict__ seeds, int nb,
                           float* __restrict__ A, int K) {
    const long r = blockIdx.x;
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    float cs, sn;
    if (angles) {
        cs = angles[r * (2 * nb) + k];
        sn = angles[r * (2 * nb) + nb + k];
    } else {
        const unsigned long long seed = seeds[rowutt[r]];
        unsigned c[4] = {(unsigned)rowframe[r], (unsigned)(k >> 2), 0u, PK_GL_STREAM};
        philox4x32_10(c[0], c[1], c[2], c[3], (unsigned)seed, (unsigned)(seed >> 32));
        const unsigned w = (k & 3) == 0 ? c[0] : ((k & 3) == 1 ? c[1] : ((k & 3) == 2 ? c[2] : c[3]));
        sincospif(2.0f * ((float)w * 2.3283064365386963e-10f), &sn, &cs);
    }
    const float s = S[r * nb + k];
    A[r * K + k] = s * cs;
    A[r * K + nb + k] = (k == 0 || k == nb - 1) ? 0.f : s * sn;
}

// The phase update of fast Griffin-Lim and the next iterate in one pass: a = rebuilt - coef * previous (previous == NULL:
// 0, the first iteration), a /= |a| + 1e-16, A[r] = S[r] * a as re | im.  `previous = rebuilt` is a swap of two buffers on
// the host side; the phases themselves are never stored.
__global__ void k_gl_phase(const float* __restrict__ R, const float* __restrict__ P, const float* __restrict__ S, float coef,
                           int nb, float* __restrict__ A, int K) {
    const long r = blockIdx.x;
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    float re = R[r * (2 * nb) + k], im = R[r * (2 * nb) + nb + k];
    if (P) {
        re -= coef * P[r * (2 * nb) + k];
        im -= coef * P[r * (2 * nb) + nb + k];
    }
    const float m = hypotf(re, im) + 1e-16f;
    const float s = S[r * nb + k];
    A[r * K + k] = s * (re / m);
    A[r * K + nb + k] = (k == 0 || k == nb - 1) ? 0.f : s * (im / m);
}

}  // namespace

struct pk_istft {
    pk_ctx* ctx = nullptr;
    pk_istft_cfg cfg;
    int n_bin = 0, K = 0;
    int transform = PK_TRANSFORM_DENSE;
    pk_dbuf d_basis, d_window;
    pk_dbuf ws_tab, ws_itab, ws_in, ws_in2, ws_out, ws_A, ws_frames, ws_xpad, ws_r[2];
    long last_rows = 0;   // pk_gl_debug_read: frames of the last pk_gl_run and the buffer its last forward STFT wrote (-1: none)
    int last_r = -1;
};

namespace {

struct istft_layout {
    std::vector<int> row0, len;     // first frame row, samples returned
    std::vector<long> woff;         // offset in the packed output
    long sumF = 0, sumS = 0;
    int maxlen = 0;
};

int make_layout(const pk_istft* h, const int32_t* frames, int B, const char* who, istft_layout& L) {
    const long N = h->cfg.n_fft, hop = h->cfg.hop_length;
    L.row0.resize(B);
    L.len.resize(B);
    L.woff.resize(B);
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) PK_FAIL(PK_EINVAL, "%s: utterance %d has %d frames, at least 1 is needed", who, b, (int)frames[b]);
        const long n = hop * (frames[b] - 1) + (h->cfg.center ? 0 : N);
        if (n + N > 0x7fffffffL) PK_FAIL(PK_EINVAL, "%s: utterance %d is longer than 2^31 samples", who, b);
        L.row0[b] = (int)L.sumF;
        L.len[b] = (int)n;
        L.woff[b] = L.sumS;
        L.sumF += frames[b];
        L.sumS += n;
        L.maxlen = n > L.maxlen ? (int)n : L.maxlen;
    }
    if (L.sumF > 0x7fffffffL - PK_GEMM_BM) PK_FAIL(PK_EINVAL, "%s: more than 2^31 frames", who);
    return PK_OK;
}

// frames = A . basis, then the gather into `out` (tab[b].ooff); A holds sumF rows of K floats.  Under PK_TRANSFORM_FFT the
// frames are the inverse radix FFT of the rows at `spec` (leading dimension ld), times the window: A or the caller's spectrum
int synth_and_ola(pk_istft* h, long sumF, const istft_utt* d_tab, int B, int maxlen, float* out, const char* gemm_name,
                  const char* ola_name, const float* spec = nullptr, long ld = 0) {
    pk_ctx* ctx = h->ctx;
    const int N = h->cfg.n_fft, hop = h->cfg.hop_length;
    if (h->transform == PK_TRANSFORM_FFT) {
        PK_TRY(pk_rfft_inverse(ctx, gemm_name, spec ? spec : h->ws_A.as<float>(), spec ? ld : (long)h->K,
                               h->d_window.as<float>(), sumF, N, h->ws_frames.as<float>()));
    } else {
        pk_gemm_args g;
        g.A = h->ws_A.as<float>();
        g.lda = h->K;
        g.Cin = h->K;
        g.taps = 1;
        g.pad = 0;
        g.Wp = h->d_basis.as<float>();
        g.M = (int)sumF;
        g.N = N;
        g.C = h->ws_frames.as<float>();
        g.ldc = N;
        PK_TRY(pk_gemm_launch(ctx, gemm_name, g));
    }
    if (maxlen > 0) {
        const int vec = ((uintptr_t)out % 16) == 0 ? 1 : 0;
        PK_LAUNCH(ctx, ola_name, k_istft_ola, dim3(pk_div_up(maxlen, OLA_BLOCK * OLA_SPT), B), dim3(OLA_BLOCK),
                  (size_t)N * sizeof(float), h->ws_frames.as<float>(), h->d_window.as<float>(), d_tab, N, hop,
                  h->cfg.center ? N / 2 : 0, vec, out);
    }
    return PK_OK;
}

int reserve_product(pk_istft* h, long sumF) {
    const long rows_alloc = ((sumF + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    PK_TRY(h->ws_A.reserve((size_t)rows_alloc * h->K * 4));
    PK_TRY(h->ws_frames.reserve((size_t)sumF * h->cfg.n_fft * 4));
    return PK_OK;
}

}  // namespace

extern "C" int pk_istft_create(pk_ctx* ctx, const pk_istft_cfg* cfg, const float* window, pk_istft** out) {
    if (!ctx || !cfg || !window || !out) PK_FAIL(PK_EINVAL, "pk_istft_create: NULL argument");
    *out = nullptr;
    const pk_istft_cfg& c = *cfg;
    if (c.n_fft <= 0 || c.n_fft % PK_GEMM_BK != 0) PK_FAIL(PK_EUNSUPPORTED, "ISTFT: n_fft must be a multiple of 16");
    if (c.n_fft > 16384) PK_FAIL(PK_EUNSUPPORTED, "ISTFT: n_fft above 16384 (the overlap-add kernel keeps the window in LDS)");
    if (c.hop_length <= 0 || c.hop_length % 4 != 0) PK_FAIL(PK_EUNSUPPORTED, "ISTFT: hop_length must be a multiple of 4");
    PK_DEVICE(ctx->device);
    pk_istft* h = new pk_istft();
    h->ctx = ctx;
    h->cfg = c;
    const int N = c.n_fft, nb = 1 + N / 2;
    h->n_bin = nb;
    h->K = ((2 * nb + PK_GEMM_BK - 1) / PK_GEMM_BK) * PK_GEMM_BK;
    // synthesis basis [K = re(k) | im(k) | padding][n]: irfft with the window folded in.  x[n] = (1/N) (X_0 + (-1)^n X_{N/2})
    // + (2/N) sum_{0 < k < N/2} (re X_k cos(2 pi k n / N) - im X_k sin(2 pi k n / N)); rows im(0), im(N/2) and the padding are 0
    {
        std::vector<float> kn((size_t)h->K * N, 0.f), packed;
        for (int k = 0; k < nb; ++k) {
            const bool edge = k == 0 || k == N / 2;
            const double s = (edge ? 1.0 : 2.0) / N;
            for (int n = 0; n < N; ++n) {
                const double ang = 2.0 * M_PI * (double)(((long)n * k) % N) / N;
                kn[(size_t)k * N + n] = (float)(s * std::cos(ang) * (double)window[n]);
                if (!edge) kn[(size_t)(nb + k) * N + n] = (float)(-s * std::sin(ang) * (double)window[n]);
            }
        }
        pk_gemm_pack(kn.data(), h->K, N, packed);
        int s = pk_upload(ctx, h->d_basis, packed.data(), packed.size() * sizeof(float));
        if (s == PK_OK) s = pk_upload(ctx, h->d_window, window, (size_t)N * sizeof(float));
        if (s != PK_OK) { pk_istft_destroy(h); return s; }
    }
    *out = h;
    return PK_OK;
}

extern "C" int pk_istft_num_samples(pk_istft* h, int32_t frames, int32_t* n) {
    if (!h || !n) PK_FAIL(PK_EINVAL, "pk_istft_num_samples: NULL argument");
    if (frames < 1) PK_FAIL(PK_EINVAL, "pk_istft_num_samples: at least 1 frame is needed");
    const long v = (long)h->cfg.hop_length * (frames - 1) + (h->cfg.center ? 0 : h->cfg.n_fft);
    if (v + h->cfg.n_fft > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_istft_num_samples: longer than 2^31 samples");
    *n = (int32_t)v;
    return PK_OK;
}

extern "C" int pk_istft_run(pk_istft* h, const float* spec, const int32_t* frames, int32_t B, float* wav_out, int32_t flags) {
    if (!h || !spec || !frames || !wav_out) PK_FAIL(PK_EINVAL, "pk_istft_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_istft_run: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    istft_layout L;
    PK_TRY(make_layout(h, frames, B, "pk_istft_run", L));
    const int nb = h->n_bin;
    std::vector<istft_utt> tab(B);
    for (int b = 0; b < B; ++b) tab[b] = {L.woff[b], L.row0[b], frames[b]};
    PK_TRY(h->ws_tab.reserve(tab.size() * sizeof(istft_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_tab.p, tab.data(), tab.size() * sizeof(istft_utt), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    const float* d_spec = spec;
    float* d_out = wav_out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)L.sumF * 2 * nb * 4));
        PK_TRY(h->ws_out.reserve((size_t)(L.sumS > 0 ? L.sumS : 1) * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, spec, (size_t)L.sumF * 2 * nb * 4, hipMemcpyHostToDevice, ctx->stream));
        d_spec = h->ws_in.as<float>();
        d_out = h->ws_out.as<float>();
    }
    PK_TRY(reserve_product(h, L.sumF));
    if (h->transform == PK_TRANSFORM_FFT) {
        // the inverse FFT reads the caller's rows where they are and never looks at im(DC), im(Nyquist): nothing to pack
        PK_TRY(synth_and_ola(h, L.sumF, h->ws_tab.as<istft_utt>(), B, L.maxlen, d_out, "istft_fft", "istft_ola", d_spec,
                             2 * nb));
    } else {
        PK_LAUNCH(ctx, "istft_pack", k_istft_pack, dim3((unsigned)L.sumF, pk_div_up(h->K, 256)), dim3(256), 0, d_spec, nb,
                  h->ws_A.as<float>(), h->K);
        PK_TRY(synth_and_ola(h, L.sumF, h->ws_tab.as<istft_utt>(), B, L.maxlen, d_out, "istft_gemm", "istft_ola"));
    }
    if (flags & PK_HOST_IO) {
        if (L.sumS > 0) PK_HIP(hipMemcpyAsync(wav_out, d_out, (size_t)L.sumS * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_gl_run(pk_istft* h, pk_mel* stft, const float* mag, const int32_t* frames, int32_t B, int32_t n_iter,
                         float momentum, const uint64_t* seeds, const float* angles, float* wav_out, int32_t flags) {
    if (!h || !stft || !mag || !frames || !wav_out) PK_FAIL(PK_EINVAL, "pk_gl_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_gl_run: batch size must be positive");
    if (n_iter < 0) PK_FAIL(PK_EINVAL, "pk_gl_run: n_iter must not be negative (got %d)", (int)n_iter);
    if (!(momentum >= 0.f && momentum < 1.f)) PK_FAIL(PK_EINVAL, "pk_gl_run: momentum must be in [0, 1) (got %g)", (double)momentum);
    const pk_mel_cfg& mc = *pk_mel_config(stft);
    const pk_istft_cfg& c = h->cfg;
    if (mc.n_fft != c.n_fft || mc.hop_length != c.hop_length || (mc.center != 0) != (c.center != 0))
        PK_FAIL(PK_EINVAL, "pk_gl_run: the STFT handle (n_fft %d, hop %d, center %d) does not match the ISTFT handle (%d, %d, %d)",
                (int)mc.n_fft, (int)mc.hop_length, (int)mc.center, (int)c.n_fft, (int)c.hop_length, (int)c.center);
    if (pk_mel_context(stft) != h->ctx) PK_FAIL(PK_EINVAL, "pk_gl_run: the two handles belong to different contexts");
    if (pk_mel_transform(stft) != h->transform)
        PK_FAIL(PK_EINVAL, "pk_gl_run: the STFT handle's transform (%d) differs from the ISTFT handle's (%d); set both with "
                "pk_mel_set_transform / pk_istft_set_transform", pk_mel_transform(stft), h->transform);
    const bool fft = h->transform == PK_TRANSFORM_FFT;
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    istft_layout L;
    PK_TRY(make_layout(h, frames, B, "pk_gl_run", L));
    const int N = c.n_fft, hop = c.hop_length, nb = h->n_bin, pad = c.center ? N / 2 : 0;
    // the forward STFT's padded-sample axis, as pk_mel_run lays it out: utterances at hop-aligned offsets, every hop
    // position a candidate row, rowmap[row] = packed frame or -1
    std::vector<long> poff(B);
    long p = 0;
    for (int b = 0; b < B; ++b) {
        if (n_iter > 0 && L.len[b] <= pad)
            PK_FAIL(PK_EINVAL, "pk_gl_run: utterance %d (%d frames) is too short: the forward STFT reflect-pads n_fft/2 = %d "
                    "samples and needs hop * (frames - 1) above that", b, (int)frames[b], pad);
        poff[b] = p;
        const long padded = (long)L.len[b] + 2 * pad;
        p += ((padded + hop - 1) / hop) * hop;
    }
    const long rows = p / hop;
    if (rows > 0x7fffffffL - PK_GEMM_BM) PK_FAIL(PK_EINVAL, "pk_gl_run: more than 2^31 rows");
    const long rows_alloc = ((rows + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    // tables: [0, B) the loop's (into xpad), [B, 2B) the last inverse's (into wav_out); then three int tables and the seeds
    std::vector<istft_utt> tab(2 * B);
    for (int b = 0; b < B; ++b) {
        tab[b] = {poff[b] + pad, L.row0[b], frames[b]};
        tab[B + b] = {L.woff[b], L.row0[b], frames[b]};
    }
    std::vector<int> itab((size_t)rows_alloc + 2 * L.sumF, -1);
    int* rowmap = itab.data();
    int* rowframe = rowmap + rows_alloc;
    int* rowutt = rowframe + L.sumF;
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < frames[b]; ++f) {
            rowmap[poff[b] / hop + f] = L.row0[b] + f;
            rowframe[L.row0[b] + f] = f;
            rowutt[L.row0[b] + f] = b;
        }
    std::vector<unsigned long long> sd(B, 0ull);
    if (seeds)
        for (int b = 0; b < B; ++b) sd[b] = seeds[b];
    const size_t tab_bytes = tab.size() * sizeof(istft_utt), seed_bytes = (size_t)B * 8;
    PK_TRY(h->ws_tab.reserve(tab_bytes + seed_bytes));
    PK_TRY(h->ws_itab.reserve(itab.size() * sizeof(int)));
    PK_HIP(hipMemcpyAsync(h->ws_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync((char*)h->ws_tab.p + tab_bytes, sd.data(), seed_bytes, hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->ws_itab.p, itab.data(), itab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    const istft_utt* d_tab = h->ws_tab.as<istft_utt>();
    const unsigned long long* d_seeds = reinterpret_cast<const unsigned long long*>((char*)h->ws_tab.p + tab_bytes);
    const int* d_rowmap = h->ws_itab.as<int>();
    const int* d_rowframe = d_rowmap + rows_alloc;
    const int* d_rowutt = d_rowframe + L.sumF;

    const float* d_mag = mag;
    const float* d_ang = angles;
    float* d_out = wav_out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)L.sumF * nb * 4));
        PK_TRY(h->ws_out.reserve((size_t)(L.sumS > 0 ? L.sumS : 1) * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, mag, (size_t)L.sumF * nb * 4, hipMemcpyHostToDevice, ctx->stream));
        d_mag = h->ws_in.as<float>();
        d_out = h->ws_out.as<float>();
        if (angles) {
            PK_TRY(h->ws_in2.reserve((size_t)L.sumF * 2 * nb * 4));
            PK_HIP(hipMemcpyAsync(h->ws_in2.p, angles, (size_t)L.sumF * 2 * nb * 4, hipMemcpyHostToDevice, ctx->stream));
            d_ang = h->ws_in2.as<float>();
        }
    }
    PK_TRY(reserve_product(h, L.sumF));
    h->last_rows = L.sumF;
    h->last_r = n_iter > 0 ? (n_iter - 1) & 1 : -1;
    const dim3 egrid((unsigned)L.sumF, pk_div_up(nb, 256));
    // the K padding of A is written here once; the kernels below write columns [0, 2 * n_bin) only
    PK_HIP(hipMemsetAsync(h->ws_A.p, 0, (size_t)L.sumF * h->K * 4, ctx->stream));
    PK_LAUNCH(ctx, "gl_apply", k_gl_apply, egrid, dim3(256), 0, d_mag, d_ang, d_rowframe, d_rowutt, d_seeds, nb,
              h->ws_A.as<float>(), h->K);
    if (n_iter > 0) {
        const size_t xpad_floats = (size_t)rows_alloc * hop + N + 64;   // + slack: the last row tile reads n_fft samples
        PK_TRY(h->ws_xpad.reserve(xpad_floats * 4));
        PK_TRY(h->ws_r[0].reserve((size_t)L.sumF * 2 * nb * 4));
        if (n_iter > 1) PK_TRY(h->ws_r[1].reserve((size_t)L.sumF * 2 * nb * 4));
        PK_HIP(hipMemsetAsync(h->ws_xpad.p, 0, xpad_floats * 4, ctx->stream));
        pk_gemm_args g;
        g.A = h->ws_xpad.as<float>();
        g.lda = hop;
        g.Cin = N;
        g.taps = 1;
        g.pad = 0;
        g.Wp = pk_mel_dft_packed(stft);
        g.M = (int)rows;
        g.N = 2 * nb;
        g.ldc = 2 * nb;
        g.out_rowmap = d_rowmap;
        const float coef = momentum / (1.f + momentum);
        // every iteration is enqueued on the stream; the host does not wait inside the loop
        for (int it = 0; it < n_iter; ++it) {
            PK_TRY(synth_and_ola(h, L.sumF, d_tab, B, L.maxlen, h->ws_xpad.as<float>(), fft ? "gl_istft_fft" : "gl_istft_gemm",
                                 "gl_istft_ola"));
            if (pad > 0)
                PK_LAUNCH(ctx, "gl_reflect", k_gl_reflect_edges, dim3(pk_div_up(2 * pad, 256), B), dim3(256), 0,
                          h->ws_xpad.as<float>(), d_tab, hop, pad);
            g.C = h->ws_r[it & 1].as<float>();
            if (fft)
                PK_TRY(pk_rfft_forward(ctx, "gl_stft_fft", g.A, hop, pk_mel_window(stft), d_rowmap, rows, N, g.C, g.ldc));
            else
                PK_TRY(pk_gemm_launch(ctx, "gl_stft_gemm", g));
            PK_LAUNCH(ctx, "gl_phase", k_gl_phase, egrid, dim3(256), 0, h->ws_r[it & 1].as<float>(),
                      it > 0 ? h->ws_r[(it - 1) & 1].as<float>() : (const float*)nullptr, d_mag, coef, nb,
                      h->ws_A.as<float>(), h->K);
        }
    }
    PK_TRY(synth_and_ola(h, L.sumF, d_tab + B, B, L.maxlen, d_out, fft ? "istft_fft" : "istft_gemm", "istft_ola"));
    if (flags & PK_HOST_IO) {
        if (L.sumS > 0) PK_HIP(hipMemcpyAsync(wav_out, d_out, (size_t)L.sumS * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_istft_set_transform(pk_istft* h, int32_t transform) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_istft_set_transform: NULL argument");
    if (transform != PK_TRANSFORM_DENSE && transform != PK_TRANSFORM_FFT)
        PK_FAIL(PK_EINVAL, "pk_istft_set_transform: transform must be PK_TRANSFORM_DENSE (0) or PK_TRANSFORM_FFT (1), got %d",
                (int)transform);
    if (transform == PK_TRANSFORM_FFT) {
        if (!pk_rfft_size_ok(h->cfg.n_fft))
            PK_FAIL(PK_EUNSUPPORTED, "ISTFT: PK_TRANSFORM_FFT needs an n_fft that is " PK_RFFT_SIZES " (got %d); the dense "
                    "transform takes any multiple of 16", (int)h->cfg.n_fft);
        PK_DEVICE(h->ctx->device);
        PK_TRY(pk_rfft_prepare(h->ctx, h->cfg.n_fft));
    }
    h->transform = transform;
    return PK_OK;
}

extern "C" int pk_gl_debug_read(pk_istft* h, int32_t what, float* out, int64_t n) {
    if (!h || !out) PK_FAIL(PK_EINVAL, "pk_gl_debug_read: NULL argument");
    if (h->last_rows <= 0) PK_FAIL(PK_ESTATE, "pk_gl_debug_read: no pk_gl_run has completed on this handle");
    const size_t row = (size_t)2 * h->n_bin * 4;
    if (n != h->last_rows * 2 * h->n_bin) PK_FAIL(PK_ESHAPE, "pk_gl_debug_read: expected %ld floats", h->last_rows * 2 * h->n_bin);
    PK_DEVICE(h->ctx->device);
    PK_HIP(hipStreamSynchronize(h->ctx->stream));
    if (what == 0) {
        if (h->last_r < 0) PK_FAIL(PK_ESTATE, "pk_gl_debug_read: the last pk_gl_run had n_iter = 0, nothing was rebuilt");
        PK_HIP(hipMemcpy(out, h->ws_r[h->last_r].p, row * h->last_rows, hipMemcpyDeviceToHost));
    } else if (what == 1) {
        PK_HIP(hipMemcpy2D(out, row, h->ws_A.p, (size_t)h->K * 4, row, h->last_rows, hipMemcpyDeviceToHost));
    } else {
        PK_FAIL(PK_EINVAL, "pk_gl_debug_read: what must be 0 (rebuilt spectrum) or 1 (last iterate)");
    }
    return PK_OK;
}

extern "C" void pk_istft_destroy(pk_istft* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->d_basis, &h->d_window, &h->ws_tab, &h->ws_itab, &h->ws_in, &h->ws_in2, &h->ws_out, &h->ws_A,
                       &h->ws_frames, &h->ws_xpad, &h->ws_r[0], &h->ws_r[1]};
    for (auto* b : bufs) b->release();
    delete h;
}
