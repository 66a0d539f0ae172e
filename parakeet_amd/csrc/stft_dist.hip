// stft_dist.hip -- multi-resolution STFT distance of two signals on gfx950, at any hop length.
//
// Reference: parakeet/modules/stft_loss.py stft :20-67 (sqrt(clip(re^2 + im^2, 1e-7))), SpectralConvergenceLoss :70-92,
// LogSTFTMagnitudeLoss :95-118, MultiResolutionSTFTLoss :163-219 (the evaluator of Parallel WaveGAN,
// parallel_wavegan_updater.py:204-211).
//
// The transform is the exact-fp32 GEMM of mel.hip: the A operand is the reflect-padded signal itself, row = frame.  That
// kernel loads A 16 bytes at a time, so a row must start on a multiple of 4 floats -- mel.hip therefore wants hop % 4 == 0.
// Here the hop is free.  With P = 4 / gcd(hop, 4) (1, 2 or 4), frames r = j (mod P) start P * hop floats apart, a multiple
// of 4: the padded timeline is kept in P copies, copy j shifted by (-j * hop) mod 4 floats so that frame j -- and with it
// every frame of its residue class -- is 16-byte aligned, and one GEMM per class runs with lda = P * hop and a row map onto
// packed frames.  P copies of the padded signal are written, never a framed (frames, n_fft) copy.
//
// The columns of the basis are interleaved, re(k) at 2k and im(k) at 2k + 1, and a row of the product has n_fft + 4 floats:
// a lane of the reduction reads two whole bins of a frame with one 16-byte load.  x and y go through the same launches as
// one batch of 2B signals; frame i of x is row i, the same frame of y is row sum(frames) + i.  One wave per frame pair
// forms X, Y and the three terms and leaves three partials per frame; a second kernel folds the partials of an utterance in
// a fixed order in fp64.  No atomics, nothing shared between utterances: an utterance's sums are bit-identical in any batch
// and at any position in it.  Magnitudes are stored only by pk_stftd_magnitude.
#include <cmath>
#include <exception>
#include <vector>

#include "pk_gemm.h"

namespace {

// copy j: xc[j * copy_floats + shift[j] + poff[s] + i] = src_s[reflect(i - pad)], s = group * B + b, group 0 = x, 1 = y
__global__ void k_stftd_pad(const float* __restrict__ x, const float* __restrict__ y, int B,
                            const long* __restrict__ woff, const int* __restrict__ wlen, const long* __restrict__ poff,
                            int pad, int hop, long copy_floats, float* __restrict__ xc) {
    const int s = blockIdx.y, j = blockIdx.z;
    const int b = s < B ? s : s - B;
    const int n = wlen[b];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + 2 * pad) return;
    int t = i - pad;
    if (pad > 0) {
        if (t < 0) t = -t;
        if (t >= n) t = 2 * (n - 1) - t;
    }
    const float* src = s < B ? x : y;
    const int shift = (4 - (int)(((long)j * hop) & 3)) & 3;
    xc[(long)j * copy_floats + shift + poff[s] + i] = src[woff[b] + t];
}

__device__ __forceinline__ float stftd_mag(float re, float im, float pfloor) {
    return sqrtf(fmaxf(re * re + im * im, pfloor));
}

// One wave per frame pair: rows r (x) and rows + r (y) of the interleaved re, im product.
// part[r] = { sum_k (Y - X)^2, sum_k Y^2, sum_k |ln max(Y, lfloor) - ln max(X, lfloor)| }
__global__ __launch_bounds__(256) void k_stftd_reduce(const float* __restrict__ reim, int ld, int n_bin, int rows,
                                                      float pfloor, float lfloor, float* __restrict__ part) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4* xr = reinterpret_cast<const float4*>(reim + (long)r * ld);
    const float4* yr = reinterpret_cast<const float4*>(reim + ((long)rows + r) * ld);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    auto term = [&](float xre, float xim, float yre, float yim) {
        const float X = stftd_mag(xre, xim, pfloor), Y = stftd_mag(yre, yim, pfloor);
        const float d = Y - X;
        s0 += d * d;
        s1 += Y * Y;
        s2 += fabsf(logf(fmaxf(Y, lfloor)) - logf(fmaxf(X, lfloor)));
    };
    const int npair = (n_bin + 1) >> 1;
    for (int p = lane; p < npair; p += 64) {
        const float4 a = xr[p], b = yr[p];
        term(a.x, a.y, b.x, b.y);
        if (2 * p + 1 < n_bin) term(a.z, a.w, b.z, b.w);   // the last pair of an odd n_bin holds one bin
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s0 += __shfl_xor(s0, d);
        s1 += __shfl_xor(s1, d);
        s2 += __shfl_xor(s2, d);
    }
    if (lane == 0) {
        part[(long)r * 3 + 0] = s0;
        part[(long)r * 3 + 1] = s1;
        part[(long)r * 3 + 2] = s2;
    }
}

// One block per utterance: out[(b * R + res) * 3 + c] = sum over its frames of part[.][c].  Thread t adds frames t, t + 256,
// ... in ascending order, then a tree over the 256 threads: the order depends on the utterance's frame count alone.
__global__ __launch_bounds__(256) void k_stftd_fold(const float* __restrict__ part, const int* __restrict__ f0,
                                                    int R, int res, double* __restrict__ out) {
    __shared__ double sh[3][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int lo = f0[b], n = f0[b + 1] - lo;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int f = t; f < n; f += 256) {
        const float* p = part + (long)(lo + f) * 3;
        a0 += (double)p[0];
        a1 += (double)p[1];
        a2 += (double)p[2];
    }
    sh[0][t] = a0;
    sh[1][t] = a1;
    sh[2][t] = a2;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            sh[0][t] += sh[0][t + d];
            sh[1][t] += sh[1][t + d];
            sh[2][t] += sh[2][t + d];
        }
        __syncthreads();
    }
    if (t < 3) out[((long)b * R + res) * 3 + t] = sh[t][0];
}

// out[r][k] = sqrt(max(re^2 + im^2, pfloor)), packed (rows, n_bin)
__global__ void k_stftd_magnitude(const float* __restrict__ reim, int ld, int n_bin, int rows, float pfloor,
                                  float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * n_bin) return;
    const long r = i / n_bin;
    const int k = (int)(i - r * n_bin);
    const float2 v = *reinterpret_cast<const float2*>(reim + r * ld + 2 * k);
    out[i] = stftd_mag(v.x, v.y, pfloor);
}

struct stftd_res {
    int n_fft = 0, hop = 0, center = 0, n_bin = 0, ld = 0, P = 1;
    pk_dbuf d_dft;   // pk_gemm_pack of the windowed DFT basis [K = n_fft][N = re(0), im(0), re(1), ...]
};

// Where the signals of one call sit for one resolution (host side), and where its tables sit in the uploaded blobs.
struct stftd_plan {
    int sumF = 0, rows = 0, Mj = 0, Mj_alloc = 0, maxlen = 0;
    long copy_floats = 0;
    size_t itab_rowmap = 0, itab_f0 = 0, ltab_poff = 0;   // offsets (elements) into the int / long tables
};

}  // namespace

struct pk_stftd {
    pk_ctx* ctx = nullptr;
    pk_stftd_cfg cfg;
    std::vector<stftd_res> res;
    pk_dbuf ws_itab, ws_ltab, ws_wav, ws_xpad, ws_reim, ws_part, ws_out;
};

extern "C" int pk_stftd_create(pk_ctx* ctx, const pk_stftd_cfg* cfg, const pk_stftd_resolution* res,
                               const float* windows, pk_stftd** out) {
    if (!ctx || !cfg || !res || !windows || !out) PK_FAIL(PK_EINVAL, "pk_stftd_create: NULL argument");
    *out = nullptr;
    if (cfg->n_res <= 0) PK_FAIL(PK_EINVAL, "pk_stftd_create: at least one resolution is needed");
    if (!(cfg->power_floor >= 0.f) || !(cfg->log_floor > 0.f))
        PK_FAIL(PK_EINVAL, "pk_stftd_create: power_floor must be >= 0 and log_floor > 0");
    for (int r = 0; r < cfg->n_res; ++r) {
        if (res[r].n_fft <= 0 || res[r].n_fft % PK_GEMM_BK != 0)
            PK_FAIL(PK_EUNSUPPORTED, "STFT distance: n_fft must be a multiple of 16 (resolution %d has %d)", r, res[r].n_fft);
        if (res[r].hop_length < 1) PK_FAIL(PK_EINVAL, "STFT distance: hop_length must be >= 1 (resolution %d)", r);
    }
    PK_DEVICE(ctx->device);
    pk_stftd* h = new pk_stftd();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->res.resize(cfg->n_res);
    const float* window = windows;
    for (int r = 0; r < cfg->n_res; ++r) {
        stftd_res& s = h->res[r];
        const int N = res[r].n_fft, nb = 1 + N / 2;
        s.n_fft = N;
        s.hop = res[r].hop_length;
        s.center = res[r].center ? 1 : 0;
        s.n_bin = nb;
        s.ld = N + 4;   // 2 * n_bin = n_fft + 2 columns, rounded up to whole 16-byte loads
        const int g = (s.hop % 4 == 0) ? 4 : ((s.hop % 2 == 0) ? 2 : 1);
        s.P = 4 / g;
        // np.fft.fft(np.eye(n_fft))[:n_bin] * window, as pk_mel_create builds it (double, rounded once), columns interleaved
        std::vector<float> kn((size_t)N * 2 * nb), packed;
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < nb; ++k) {
                const double ang = -2.0 * M_PI * (double)(((long)n * k) % N) / N;
                kn[(size_t)n * 2 * nb + 2 * k] = (float)(std::cos(ang) * (double)window[n]);
                kn[(size_t)n * 2 * nb + 2 * k + 1] = (float)(std::sin(ang) * (double)window[n]);
            }
        pk_gemm_pack(kn.data(), N, 2 * nb, packed);
        int st = pk_upload(ctx, s.d_dft, packed.data(), packed.size() * sizeof(float));
        if (st != PK_OK) {
            pk_stftd_destroy(h);
            return st;
        }
        window += N;
    }
    *out = h;
    return PK_OK;
}

static int stftd_frames(const stftd_res& s, long n_samples) {
    const long padded = n_samples + (s.center ? s.n_fft : 0);
    return padded < s.n_fft ? 0 : (int)(1 + (padded - s.n_fft) / s.hop);
}

extern "C" int pk_stftd_num_frames(pk_stftd* h, int32_t r, int32_t n_samples, int32_t* frames) {
    if (!h || !frames) PK_FAIL(PK_EINVAL, "pk_stftd_num_frames: NULL argument");
    if (r < 0 || r >= (int)h->res.size()) PK_FAIL(PK_EINVAL, "pk_stftd_num_frames: no resolution %d", r);
    *frames = stftd_frames(h->res[r], n_samples);
    return PK_OK;
}

// Lay `groups` x B signals (group 0 = x, 1 = y) on one timeline for resolution s and append its tables to itab / ltab.
// Every utterance starts on a multiple of P * hop, so frame f of any utterance falls into residue class f % P.
// Sizes are formed in long and refused before anything is sized by them (hop 1 puts a candidate frame on every sample).
static int stftd_plan_one(const stftd_res& s, const char* who, const int32_t* lens, int B, int groups, std::vector<int>& itab,
                          std::vector<long>& ltab, stftd_plan& pl) {
    const int N = s.n_fft, hop = s.hop, pad = s.center ? N / 2 : 0, P = s.P;
    const long step = (long)P * hop;
    std::vector<long> poff(B);
    std::vector<int> nfr(B);
    long p = 0, sumF = 0;
    pl.maxlen = 0;
    for (int b = 0; b < B; ++b) {
        const long padded = (long)lens[b] + 2 * pad;
        nfr[b] = stftd_frames(s, lens[b]);
        poff[b] = p;
        p += ((padded + step - 1) / step) * step;
        sumF += nfr[b];
        if (lens[b] > pl.maxlen) pl.maxlen = lens[b];
    }
    const long G = p;                                   // one group's stretch of the timeline, a multiple of P * hop
    const long rows = groups * G / hop;                 // every hop position is a candidate frame; a multiple of P
    if (rows + (long)P * PK_GEMM_BM > 0x3fffffffL || groups * sumF > 0x3fffffffL)
        PK_FAIL(PK_EUNSUPPORTED, "%s: too many frames in one call (%ld candidate rows at n_fft %d, hop %d; the limit is 2^30)",
                who, rows, N, hop);
    pl.rows = (int)rows;
    pl.Mj = pl.rows / P;                                // rows of each residue class' GEMM
    pl.sumF = 0;
    pl.itab_f0 = itab.size();
    for (int b = 0; b < B; ++b) {
        itab.push_back(pl.sumF);
        pl.sumF += nfr[b];
    }
    itab.push_back(pl.sumF);
    pl.Mj_alloc = ((pl.Mj + PK_GEMM_BM - 1) / PK_GEMM_BM) * PK_GEMM_BM;
    // the last row tile of class P - 1 reads up to (P - 1) * hop + 3 + (Mj_alloc - 1) * P * hop + n_fft floats into its copy
    pl.copy_floats = ((groups * G + (long)PK_GEMM_BM * step + N + 8 + 3) / 4) * 4;
    pl.ltab_poff = ltab.size();
    pl.itab_rowmap = itab.size();
    itab.resize(itab.size() + (size_t)P * pl.Mj_alloc, -1);
    int* rowmap = itab.data() + pl.itab_rowmap;
    for (int g = 0; g < groups; ++g)
        for (int b = 0; b < B; ++b) {
            ltab.push_back(g * G + poff[b]);
            const long t0 = (g * G + poff[b]) / hop;
            const int o0 = g * pl.sumF + itab[pl.itab_f0 + b];
            for (int f = 0; f < nfr[b]; ++f) {
                const long t = t0 + f;
                rowmap[(size_t)(t % P) * pl.Mj_alloc + t / P] = o0 + f;
            }
        }
    return PK_OK;
}

// re, im rows of resolution r for the planned signals into h->ws_reim (packed, ld floats each)
static int stftd_transform(pk_stftd* h, int r, const stftd_plan& pl, const float* d_x, const float* d_y, int B, int groups) {
    pk_ctx* ctx = h->ctx;
    const stftd_res& s = h->res[r];
    const int N = s.n_fft, pad = s.center ? N / 2 : 0;
    const int* itab = h->ws_itab.as<int>();
    const long* ltab = h->ws_ltab.as<long>();
    // gaps between utterances are left as they are: only frames that lie inside one padded utterance are stored
    PK_TRY(h->ws_xpad.reserve((size_t)s.P * pl.copy_floats * 4));
    PK_TRY(h->ws_reim.reserve((size_t)groups * pl.sumF * s.ld * 4));
    PK_LAUNCH(ctx, "stftd_reflect_pad", k_stftd_pad, dim3(pk_div_up(pl.maxlen + 2 * pad, 256), groups * B, s.P), dim3(256), 0,
              d_x, d_y, B, ltab, itab, ltab + pl.ltab_poff, pad, s.hop, pl.copy_floats, h->ws_xpad.as<float>());
    for (int j = 0; j < s.P; ++j) {
        const int shift = (4 - (int)(((long)j * s.hop) & 3)) & 3;
        pk_gemm_args g;
        g.A = h->ws_xpad.as<float>() + (size_t)j * pl.copy_floats + shift + (long)j * s.hop;   // 16-byte aligned
        g.lda = s.P * s.hop;
        g.Cin = N;
        g.taps = 1;
        g.pad = 0;
        g.Wp = s.d_dft.as<float>();
        g.M = pl.Mj;
        g.N = 2 * s.n_bin;
        g.C = h->ws_reim.as<float>();
        g.ldc = s.ld;
        g.out_rowmap = itab + pl.itab_rowmap + (size_t)j * pl.Mj_alloc;
        PK_TRY(pk_gemm_launch(ctx, "stftd_stft_gemm", g));
    }
    return PK_OK;
}

// Shared front of the two entry points: checks, plans for resolutions [r0, r1), one upload of the tables.
// The int table starts with lens[B], the long table with the sample offsets woff[B].
static int stftd_prepare_tables(pk_stftd* h, const char* who, const int32_t* lens, int B, int groups, int r0, int r1,
                                std::vector<stftd_plan>& plans, long& sumS) {
    std::vector<int> itab(lens, lens + B);
    std::vector<long> ltab(B);
    sumS = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] <= 0) PK_FAIL(PK_EINVAL, "%s: utterance %d is empty", who, b);
        for (int r = r0; r < r1; ++r)
            if (h->res[r].center && lens[b] <= h->res[r].n_fft / 2)
                PK_FAIL(PK_EINVAL, "%s: utterance %d (%d samples) too short for reflect padding at n_fft %d", who, b,
                        lens[b], h->res[r].n_fft);
        ltab[b] = sumS;
        sumS += lens[b];
    }
    if (sumS > 0x3fffffffL) PK_FAIL(PK_EUNSUPPORTED, "%s: more than 2^30 samples in one call", who);
    plans.resize(r1 - r0);
    for (int r = r0; r < r1; ++r) PK_TRY(stftd_plan_one(h->res[r], who, lens, B, groups, itab, ltab, plans[r - r0]));
    pk_ctx* ctx = h->ctx;
    PK_TRY(h->ws_itab.reserve(itab.size() * sizeof(int)));
    PK_TRY(h->ws_ltab.reserve(ltab.size() * sizeof(long)));
    PK_HIP(hipMemcpyAsync(h->ws_itab.p, itab.data(), itab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->ws_ltab.p, ltab.data(), ltab.size() * sizeof(long), hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));   // the host tables go out of scope
    return PK_OK;
}

// No exception crosses the C ABI: a host table that cannot be allocated is PK_ENOMEM.
static int stftd_prepare(pk_stftd* h, const char* who, const int32_t* lens, int B, int groups, int r0, int r1,
                         std::vector<stftd_plan>& plans, long& sumS) {
    try {
        return stftd_prepare_tables(h, who, lens, B, groups, r0, r1, plans, sumS);
    } catch (const std::exception& e) {
        PK_FAIL(PK_ENOMEM, "%s: host tables: %s", who, e.what());
    }
}

extern "C" int pk_stftd_run(pk_stftd* h, const float* x, const float* y, const int32_t* lens, int32_t B,
                            double* sums_out, int32_t flags) {
    if (!h || !x || !y || !lens || !sums_out) PK_FAIL(PK_EINVAL, "pk_stftd_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_stftd_run: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const int R = (int)h->res.size();
    std::vector<stftd_plan> plans;
    long sumS = 0;
    PK_TRY(stftd_prepare(h, "pk_stftd_run", lens, B, 2, 0, R, plans, sumS));
    const float *d_x = x, *d_y = y;
    double* d_out = sums_out;
    const size_t out_bytes = (size_t)B * R * 3 * sizeof(double);
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_wav.reserve((size_t)sumS * 2 * 4));
        PK_TRY(h->ws_out.reserve(out_bytes));
        PK_HIP(hipMemcpyAsync(h->ws_wav.p, x, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
        PK_HIP(hipMemcpyAsync(h->ws_wav.as<float>() + sumS, y, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
        d_x = h->ws_wav.as<float>();
        d_y = d_x + sumS;
        d_out = h->ws_out.as<double>();
    }
    for (int r = 0; r < R; ++r) {
        const stftd_plan& pl = plans[r];
        const stftd_res& s = h->res[r];
        if (pl.sumF > 0) {
            PK_TRY(stftd_transform(h, r, pl, d_x, d_y, B, 2));
            PK_TRY(h->ws_part.reserve((size_t)pl.sumF * 3 * 4));
            PK_LAUNCH(ctx, "stftd_reduce", k_stftd_reduce, dim3(pk_div_up(pl.sumF, 4)), dim3(256), 0, h->ws_reim.as<float>(),
                      s.ld, s.n_bin, pl.sumF, h->cfg.power_floor, h->cfg.log_floor, h->ws_part.as<float>());
        } else {
            PK_TRY(h->ws_part.reserve(16));
        }
        PK_LAUNCH(ctx, "stftd_fold", k_stftd_fold, dim3(B), dim3(256), 0, h->ws_part.as<float>(),
                  h->ws_itab.as<int>() + pl.itab_f0, R, r, d_out);
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(sums_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_stftd_magnitude(pk_stftd* h, int32_t r, const float* wav, const int32_t* lens, int32_t B, float* out,
                                  int32_t flags) {
    if (!h || !wav || !lens || !out) PK_FAIL(PK_EINVAL, "pk_stftd_magnitude: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_stftd_magnitude: batch size must be positive");
    if (r < 0 || r >= (int)h->res.size()) PK_FAIL(PK_EINVAL, "pk_stftd_magnitude: no resolution %d", r);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    std::vector<stftd_plan> plans;
    long sumS = 0;
    PK_TRY(stftd_prepare(h, "pk_stftd_magnitude", lens, B, 1, r, r + 1, plans, sumS));
    const stftd_plan& pl = plans[0];
    const stftd_res& s = h->res[r];
    if (pl.sumF == 0) return PK_OK;
    const float* d_wav = wav;
    float* d_out = out;
    const size_t out_bytes = (size_t)pl.sumF * s.n_bin * 4;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_wav.reserve((size_t)sumS * 4));
        PK_TRY(h->ws_out.reserve(out_bytes));
        PK_HIP(hipMemcpyAsync(h->ws_wav.p, wav, (size_t)sumS * 4, hipMemcpyHostToDevice, ctx->stream));
        d_wav = h->ws_wav.as<float>();
        d_out = h->ws_out.as<float>();
    }
    PK_TRY(stftd_transform(h, r, pl, d_wav, d_wav, B, 1));
    PK_LAUNCH(ctx, "stftd_magnitude", k_stftd_magnitude, dim3(pk_div_up((long)pl.sumF * s.n_bin, 256)), dim3(256), 0,
              h->ws_reim.as<float>(), s.ld, s.n_bin, pl.sumF, h->cfg.power_floor, d_out);
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" void pk_stftd_destroy(pk_stftd* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (auto& s : h->res) s.d_dft.release();
    pk_dbuf* bufs[] = {&h->ws_itab, &h->ws_ltab, &h->ws_wav, &h->ws_xpad, &h->ws_reim, &h->ws_part, &h->ws_out};
    for (auto* b : bufs) b->release();
    delete h;
}
