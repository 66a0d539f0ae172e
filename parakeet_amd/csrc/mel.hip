// mel.hip -- STFT -> magnitude/power -> mel -> log on gfx950 (feature / metric path).
//
// Reference: parakeet/modules/audio.py STFT.forward :161-200 (reflect pad + F.conv1d with the
// windowed DFT basis [2*n_bin, 1, n_fft], stride hop), power :198-200, magnitude :202-215,
// MelScale.forward :226-229; host twin parakeet/data/get_feats.py LogMelFBank :56-88
// (log10(clip(mel_basis . |STFT|, 1e-10))).
//
// The strided conv IS a GEMM whose A operand is the padded signal itself with leading dimension
// = hop: row r (frame r) = xpad[r*hop .. r*hop + n_fft).  Utterances sit on one padded-sample axis
// at hop-aligned offsets, so every frame of every utterance is one row of a single GEMM
// (frames that straddle two utterances are computed and dropped by the row map).
//
// Under PK_TRANSFORM_FFT (pk_mel_set_transform) the same re | im rows come from the radix FFT of rfft.hip: it reads the same
// padded-sample axis at stride hop, multiplies by the fp32 window and writes through the same row map.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pk_gemm.h"
#include "pk_mel.h"
#include "pk_rfft.h"

namespace {

// xpad[poff[b] + i] = x[reflect(i - pad)] for i in [0, len + 2*pad)   (F.pad mode='reflect', :175-179)
__global__ void k_reflect_pad(const float* __restrict__ wav, const int* __restrict__ woff,
                              const int* __restrict__ wlen, const long* __restrict__ poff, int pad,
                              float* __restrict__ xpad) {
    const int b = blockIdx.y;
    const int n = wlen[b];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + 2 * pad) return;
    int s = i - pad;
    if (pad > 0) {
        if (s < 0) s = -s;
        if (s >= n) s = 2 * (n - 1) - s;
    }
    xpad[poff[b] + i] = wav[(long)woff[b] + s];
}

// spec[r][k] = re^2 + im^2 (power) or its sqrt (magnitude); columns [n_bin, ld) zeroed (GEMM K padding)
__global__ void k_magnitude(const float* __restrict__ reim, int ld_in, int n_bin, int rows, int power,
                            float* __restrict__ spec, int ld_out) {
    const int r = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows || k >= ld_out) return;
    float v = 0.f;
    if (k < n_bin) {
        const float re = reim[(long)r * ld_in + k], im = reim[(long)r * ld_in + n_bin + k];
        v = re * re + im * im;
        if (!power) v = sqrtf(v);
    }
    spec[(long)r * ld_out + k] = v;
}

// y = log_base(max(y, floor))   (np.clip(mel, a_min=1e-10) + log10 / log, get_feats.py:82-87)
__global__ void k_clip_log(float* __restrict__ y, long n, float floor_v, int base10) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = fmaxf(y[i], floor_v);
    y[i] = base10 ? log10f(v) : logf(v);
}

// Frame energy (get_feats.py Energy._calculate_energy :196-203): energy[rowmap[r]] = sqrt(max(sum_k re^2 + im^2, floor)).
// One wave per frame, over the re | im row the STFT GEMM left: the power spectrum lives in registers only, no (frames, n_bin)
// tensor is written or read back.
__global__ __launch_bounds__(256) void k_frame_energy(const float* __restrict__ reim, int ld_in, int n_bin, int rows,
                                                      const int* __restrict__ rowmap, float floor_v,
                                                      float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int o = rowmap[r];
    if (o < 0) return;
    const int lane = threadIdx.x & 63;
    const float* x = reim + (long)r * ld_in;
    float s = 0.f;
    for (int k = lane; k < n_bin; k += 64) {
        const float re = x[k], im = x[n_bin + k];
        s += re * re + im * im;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) out[o] = sqrtf(fmaxf(s, floor_v));
}

// out[t][c] = mean of x[start[t] .. start[t + 1])[c], 0 for an empty span (get_feats.py _average_by_duration :205-214).
// One wave per token; start is the prefix sum of the durations, clamped to the number of frames like a numpy slice.
__global__ __launch_bounds__(64) void k_average_by_duration(const float* __restrict__ x, int C, const int* __restrict__ start,
                                                            float* __restrict__ out) {
    const int t = blockIdx.x;
    const int lo = start[t], n = start[t + 1] - lo;
    const int lane = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int f = lane; f < n; f += 64) s += x[(long)(lo + f) * C + c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) out[(long)t * C + c] = n > 0 ? s / (float)n : 0.f;
    }
}

}  // namespace

struct pk_mel {
    pk_ctx* ctx = nullptr;
    pk_mel_cfg cfg;
    int n_bin = 0, ldspec = 0;
    int transform = PK_TRANSFORM_DENSE;
    std::vector<float> window;      // as given; d_window holds it once PK_TRANSFORM_FFT has been asked for
    pk_dbuf d_dft, d_melw, d_window;   // packed GEMM weights
    pk_dbuf ws_tab, ws_ltab, ws_wav, ws_xpad, ws_reim, ws_spec, ws_out;
};

extern "C" int pk_mel_create(pk_ctx* ctx, const pk_mel_cfg* cfg, const float* window, const float* mel_basis,
                             pk_mel** out) {
    if (!ctx || !cfg || !window || !out) PK_FAIL(PK_EINVAL, "pk_mel_create: NULL argument");
    *out = nullptr;
    const pk_mel_cfg& c = *cfg;
    if (c.n_fft <= 0 || c.n_fft % PK_GEMM_BK != 0) PK_FAIL(PK_EUNSUPPORTED, "STFT: n_fft must be a multiple of 16");
    if (c.hop_length <= 0 || c.hop_length % 4 != 0) PK_FAIL(PK_EUNSUPPORTED, "STFT: hop_length must be a multiple of 4");
    if (c.n_mels < 0 || (c.n_mels > 0 && !mel_basis)) PK_FAIL(PK_EINVAL, "pk_mel_create: mel basis missing");
    PK_DEVICE(ctx->device);
    pk_mel* h = new pk_mel();
    h->ctx = ctx;
    h->cfg = c;
    const int N = c.n_fft, nb = 1 + N / 2;
    h->n_bin = nb;
    h->window.assign(window, window + N);
    h->ldspec = ((nb + PK_GEMM_BK - 1) / PK_GEMM_BK) * PK_GEMM_BK;
    // windowed DFT basis, np.fft.fft(np.eye(n_fft))[:n_bin] * window (:146-153): [K = n][N = re(k) | im(k)]
    {
        std::vector<float> kn((size_t)N * 2 * nb), packed;
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < nb; ++k) {
                const double ang = -2.0 * M_PI * (double)(((long)n * k) % N) / N;
                kn[(size_t)n * 2 * nb + k] = (float)(std::cos(ang) * (double)window[n]);
                kn[(size_t)n * 2 * nb + nb + k] = (float)(std::sin(ang) * (double)window[n]);
            }
        pk_gemm_pack(kn.data(), N, 2 * nb, packed);
        int s = pk_upload(ctx, h->d_dft, packed.data(), packed.size() * sizeof(float));
        if (s != PK_OK) { delete h; return s; }
    }
    if (c.n_mels > 0) {
        std::vector<float> kn((size_t)h->ldspec * c.n_mels, 0.f), packed;   // [K = bin][N = mel]
        for (int m = 0; m < c.n_mels; ++m)
            for (int k = 0; k < nb; ++k) kn[(size_t)k * c.n_mels + m] = mel_basis[(size_t)m * nb + k];
        pk_gemm_pack(kn.data(), h->ldspec, c.n_mels, packed);
        int s = pk_upload(ctx, h->d_melw, packed.data(), packed.size() * sizeof(float));
        if (s != PK_OK) { delete h; return s; }
    }
    *out = h;
    return PK_OK;
}

const pk_mel_cfg* pk_mel_config(const pk_mel* h) { return &h->cfg; }
pk_ctx* pk_mel_context(const pk_mel* h) { return h->ctx; }
const float* pk_mel_dft_packed(const pk_mel* h) { return h->d_dft.as<float>(); }
int pk_mel_transform(const pk_mel* h) { return h->transform; }
const float* pk_mel_window(const pk_mel* h) { return h->d_window.as<float>(); }

extern "C" int pk_mel_set_transform(pk_mel* h, int32_t transform) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_mel_set_transform: NULL argument");
    if (transform != PK_TRANSFORM_DENSE && transform != PK_TRANSFORM_FFT)
        PK_FAIL(PK_EINVAL, "pk_mel_set_transform: transform must be PK_TRANSFORM_DENSE (0) or PK_TRANSFORM_FFT (1), got %d",
                (int)transform);
    if (transform == PK_TRANSFORM_FFT) {
        if (!pk_rfft_size_ok(h->cfg.n_fft))
            PK_FAIL(PK_EUNSUPPORTED, "STFT: PK_TRANSFORM_FFT needs an n_fft that is " PK_RFFT_SIZES " (got %d); the dense "
                    "transform takes any multiple of 16", (int)h->cfg.n_fft);
        PK_DEVICE(h->ctx->device);
        PK_TRY(pk_rfft_prepare(h->ctx, h->cfg.n_fft));
        if (!h->d_window.p) PK_TRY(pk_upload(h->ctx, h->d_window, h->window.data(), h->window.size() * sizeof(float)));
    }
    h->transform = transform;
    return PK_OK;
}

extern "C" int pk_mel_num_frames(pk_mel* h, int32_t n_samples, int32_t* frames) {
    if (!h || !frames) PK_FAIL(PK_EINVAL, "pk_mel_num_frames: NULL argument");
    const int pad = h->cfg.center ? h->cfg.n_fft / 2 : 0;
    const long padded = (long)n_samples + 2 * pad;
    *frames = padded < h->cfg.n_fft ? 0 : (int32_t)(1 + (padded - h->cfg.n_fft) / h->cfg.hop_length);
    return PK_OK;
}

extern "C" int pk_mel_run(pk_mel* h, const float* wav, const int32_t* lens, int32_t B, float* out,
                          int32_t what, int32_t flags) {
    if (!h || !wav || !lens || !out) PK_FAIL(PK_EINVAL, "pk_mel_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_mel_run: batch size must be positive");
    if (what < 0 || what > 3) PK_FAIL(PK_EINVAL, "pk_mel_run: what must be 0 (re|im), 1 (spectrum), 2 (mel) or 3 (energy)");
    if (what == 2 && h->cfg.n_mels <= 0) PK_FAIL(PK_ESTATE, "pk_mel_run: no mel basis was given");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_mel_cfg& c = h->cfg;
    const int N = c.n_fft, hop = c.hop_length, nb = h->n_bin, pad = c.center ? N / 2 : 0;
    std::vector<int> woff(B), nfr(B), row0(B);
    std::vector<long> poff(B);
    long p = 0, sumS = 0;
    int sumF = 0, maxlen = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] <= pad) PK_FAIL(PK_EINVAL, "pk_mel_run: utterance %d too short for reflect padding", b);
        woff[b] = (int)sumS;
        sumS += lens[b];
        maxlen = lens[b] > maxlen ? lens[b] : maxlen;
        const long padded = (long)lens[b] + 2 * pad;
        nfr[b] = padded < N ? 0 : (int)(1 + (padded - N) / hop);
        poff[b] = p;
        row0[b] = (int)(p / hop);
        p += ((padded + hop - 1) / hop) * hop;   // next utterance starts hop-aligned
        sumF += nfr[b];
    }
    if (sumF == 0) return PK_OK;
    const int rows = (int)(p / hop);             // every hop position is a candidate row
    const int rows_alloc = ((rows + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    std::vector<int> rowmap(rows_alloc, -1), tab;
    {
        int o = 0;
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < nfr[b]; ++f) rowmap[row0[b] + f] = o++;
    }
    tab.insert(tab.end(), woff.begin(), woff.end());
    tab.insert(tab.end(), lens, lens + B);
    tab.insert(tab.end(), rowmap.begin(), rowmap.end());
    PK_TRY(h->ws_tab.reserve(tab.size() * sizeof(int)));
    PK_TRY(h->ws_ltab.reserve(poff.size() * sizeof(long)));
    PK_HIP(hipMemcpyAsync(h->ws_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->ws_ltab.p, poff.data(), poff.size() * sizeof(long), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    const int* d_tab = h->ws_tab.as<int>();
    const float* d_wav = wav;
    const int out_cols = what == 0 ? 2 * nb : (what == 1 ? nb : (what == 2 ? c.n_mels : 1));
    float* d_out = out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_wav.reserve((size_t)sumS * 4));
        PK_TRY(h->ws_out.reserve((size_t)sumF * out_cols * 4));
        PK_HIP(hipMemcpyAsync(h->ws_wav.p, wav, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
        d_wav = h->ws_wav.as<float>();
        d_out = h->ws_out.as<float>();
    }
    // padded signal (+ one tile of slack so the last GEMM row tile can read n_fft samples)
    const size_t xpad_floats = (size_t)rows_alloc * hop + N + 64;
    PK_TRY(h->ws_xpad.reserve(xpad_floats * 4));
    PK_HIP(hipMemsetAsync(h->ws_xpad.p, 0, xpad_floats * 4, ctx->stream));
    PK_LAUNCH(ctx, "mel_reflect_pad", k_reflect_pad, dim3(pk_div_up(maxlen + 2 * pad, 256), B), dim3(256), 0, d_wav,
              d_tab, d_tab + B, h->ws_ltab.as<long>(), pad, h->ws_xpad.as<float>());
    // STFT GEMM: [rows x n_fft] (lda = hop) x [n_fft x 2*n_bin]; under PK_TRANSFORM_FFT the radix FFT writes the same rows
    const bool fft = h->transform == PK_TRANSFORM_FFT;
    pk_gemm_args g;
    g.A = h->ws_xpad.as<float>();
    g.lda = hop;
    g.Cin = N;
    g.taps = 1;
    g.pad = 0;
    g.Wp = h->d_dft.as<float>();
    g.M = rows;
    g.N = 2 * nb;
    if (what == 0) {
        g.C = d_out;
        g.ldc = 2 * nb;
        g.out_rowmap = d_tab + 2 * B;
        if (fft)
            PK_TRY(pk_rfft_forward(ctx, "mel_stft_fft", g.A, hop, h->d_window.as<float>(), g.out_rowmap, rows, N, g.C, g.ldc));
        else
            PK_TRY(pk_gemm_launch(ctx, "mel_stft_gemm", g));
    } else {
        PK_TRY(h->ws_reim.reserve((size_t)rows_alloc * 2 * nb * 4));
        g.C = h->ws_reim.as<float>();
        g.ldc = 2 * nb;
        if (fft)
            PK_TRY(pk_rfft_forward(ctx, "mel_stft_fft", g.A, hop, h->d_window.as<float>(), nullptr, rows, N, g.C, g.ldc));
        else
            PK_TRY(pk_gemm_launch(ctx, "mel_stft_gemm", g));
        if (what == 3) {
            PK_LAUNCH(ctx, "mel_frame_energy", k_frame_energy, dim3(pk_div_up(rows, 4)), dim3(256), 0, h->ws_reim.as<float>(),
                      2 * nb, nb, rows, d_tab + 2 * B, c.log_floor, d_out);
        } else if (what == 1) {
            // spectrum straight into the packed output (row map applied by a tiny second pass: reuse k_magnitude
            // on timeline rows, then gather) -- keep it simple: compute on the timeline, gather rows with a GEMM-free copy
            PK_TRY(h->ws_spec.reserve((size_t)rows_alloc * h->ldspec * 4));
            PK_LAUNCH(ctx, "mel_magnitude", k_magnitude, dim3(pk_div_up(h->ldspec, 256), rows), dim3(256), 0,
                      h->ws_reim.as<float>(), 2 * nb, nb, rows, c.power ? 1 : 0, h->ws_spec.as<float>(), h->ldspec);
            for (int b = 0, o = 0; b < B; ++b) {
                if (nfr[b] > 0)
                    PK_HIP(hipMemcpy2DAsync(d_out + (size_t)o * nb, (size_t)nb * 4,
                                            h->ws_spec.as<float>() + (size_t)row0[b] * h->ldspec, (size_t)h->ldspec * 4,
                                            (size_t)nb * 4, nfr[b], hipMemcpyDeviceToDevice, ctx->stream));
                o += nfr[b];
            }
        } else {
            PK_TRY(h->ws_spec.reserve((size_t)(rows_alloc + 8) * h->ldspec * 4));
            PK_LAUNCH(ctx, "mel_magnitude", k_magnitude, dim3(pk_div_up(h->ldspec, 256), rows), dim3(256), 0,
                      h->ws_reim.as<float>(), 2 * nb, nb, rows, c.power ? 1 : 0, h->ws_spec.as<float>(), h->ldspec);
            pk_gemm_args m;
            m.A = h->ws_spec.as<float>();
            m.lda = h->ldspec;
            m.Cin = h->ldspec;
            m.taps = 1;
            m.pad = 0;
            m.Wp = h->d_melw.as<float>();
            m.C = d_out;
            m.ldc = c.n_mels;
            m.out_rowmap = d_tab + 2 * B;
            m.M = rows;
            m.N = c.n_mels;
            PK_TRY(pk_gemm_launch(ctx, "mel_filterbank_gemm", m));
            if (c.log_base != 0) {
                const long n = (long)sumF * c.n_mels;
                PK_LAUNCH(ctx, "mel_clip_log", k_clip_log, dim3(pk_div_up(n, 256)), dim3(256), 0, d_out, n, c.log_floor,
                          c.log_base == 10 ? 1 : 0);
            }
        }
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(out, d_out, (size_t)sumF * out_cols * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_op_average_by_duration(pk_ctx* ctx, const float* x, int64_t frames, int32_t C, const int64_t* durations,
                                         int32_t T, float* out) {
    if (!ctx || !durations || !out || (!x && frames > 0)) PK_FAIL(PK_EINVAL, "pk_op_average_by_duration: NULL argument");
    if (frames < 0 || frames > 0x7fffffff || C <= 0 || T <= 0) PK_FAIL(PK_EINVAL, "average_by_duration: bad shape");
    PK_DEVICE(ctx->device);
    std::vector<int> start(T + 1, 0);
    int64_t k = 0;
    for (int t = 0; t < T; ++t) {
        if (durations[t] < 0) PK_FAIL(PK_EINVAL, "average_by_duration: negative duration at token %d", t);
        k = std::min<int64_t>(k + durations[t], frames);   // x[start:end] past the last frame is an empty slice
        start[t + 1] = (int)k;
    }
    pk_dbuf d_start;
    int rc = pk_upload(ctx, d_start, start.data(), start.size() * sizeof(int));
    if (rc == PK_OK) {
        hipLaunchKernelGGL(k_average_by_duration, dim3(T), dim3(64), 0, ctx->stream, x, C, d_start.as<int>(), out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // d_start is released below
        if (e != hipSuccess) { d_start.release(); PK_FAIL(PK_EHIP, "pk_op_average_by_duration: %s", hipGetErrorString(e)); }
    }
    d_start.release();
    return rc;
}

extern "C" void pk_mel_destroy(pk_mel* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->d_dft, &h->d_melw, &h->d_window, &h->ws_tab, &h->ws_ltab, &h->ws_wav, &h->ws_xpad, &h->ws_reim,
                       &h->ws_spec, &h->ws_out};
    for (auto* b : bufs) b->release();
    delete h;
}
