// pvoc.hip -- the phase vocoder over ragged batches of packed (frames, 2 n_bin) re | im rows, in float64 without any
// transcendental function, on gfx950.  The definition and the plan: pk_pvoc.h.  This file is compiled without
// contraction and without the SLP vectoriser (build.py): every float64 operation is the separate operation the header writes,
// and the re / im chains of a lane stay scalar lines.
//
// A call uploads its table of utterances (pk_upload synchronises, as everywhere), enqueues one kernel on the context's stream
// and reads nothing back.
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_pvoc.h"

namespace {

struct pvoc_utt {
    long soff;      // first row in the packed input
    long ooff;      // first row in the packed output
    double rate;
    int F;          // input frames, >= 1
    int T;          // output frames, >= 1
};
static_assert(sizeof(pvoc_utt) % 8 == 0, "tables are arrays of pvoc_utt");

// m(z) and u(z) of pk_pvoc.h
__device__ __forceinline__ void pv_polar(double re, double im, double& m, double& ur, double& ui) {
    m = sqrt(re * re + im * im);
    const bool nz = m > 0.0;
    const double d = nz ? m : 1.0;
    const double a = re / d, b = im / d;
    ur = nz ? a : 1.0;
    ui = nz ? b : 0.0;
}

// the rows of step t of an utterance: (re, im) of D[k_t] and of D[k_t + 1] for this lane's bin, and a_t.  The loads are
// unconditional, from a row clamped into the utterance (a load under a branch is followed by its own wait); a row at or
// beyond F is selected to zero.  t is clamped to T - 1: a step beyond the last is loaded and not used
struct pv_rows {
    float re0, im0, re1, im1;
    double a;
};

__device__ __forceinline__ pv_rows pv_load(const float* __restrict__ su, long ld, int n_bin, const pvoc_utt& u, long t) {
    const long tc = t < u.T ? t : u.T - 1;
    const double step = (double)tc * u.rate, kf = floor(step);
    const long k = (long)kf, F = u.F;
    const long r0 = k < F ? k : F - 1, r1 = k + 1 < F ? k + 1 : F - 1;
    const float a0 = su[r0 * ld], b0 = su[r0 * ld + n_bin], a1 = su[r1 * ld], b1 = su[r1 * ld + n_bin];
    pv_rows r;
    r.re0 = k < F ? a0 : 0.f;
    r.im0 = k < F ? b0 : 0.f;
    r.re1 = k + 1 < F ? a1 : 0.f;
    r.im1 = k + 1 < F ? b1 : 0.f;
    r.a = step - kf;
    return r;
}

__global__ __launch_bounds__(PVOC_THREADS) void k_pvoc(const float* __restrict__ spec, const pvoc_utt* __restrict__ utts, int n_bin,
                                                       float* __restrict__ out) {
    const pvoc_utt u = utts[blockIdx.y];
    const int bin = blockIdx.x * PVOC_THREADS + threadIdx.x;
    if (bin >= n_bin) return;
    const long ld = 2L * n_bin, T = u.T;
    const float* su = spec + u.soff * ld + bin;
    float* ou = out + u.ooff * ld + bin;
    double pr, pi;
    {
        double m;
        pv_polar((double)su[0], (double)su[n_bin], m, pr, pi);      // p_0 = u(D[0])
    }
    pv_rows cur[PVOC_AHEAD], nxt[PVOC_AHEAD];
#pragma unroll
    for (int j = 0; j < PVOC_AHEAD; ++j) cur[j] = pv_load(su, ld, n_bin, u, j);
    for (long t0 = 0; t0 < T; t0 += PVOC_AHEAD) {
#pragma unroll
        for (int j = 0; j < PVOC_AHEAD; ++j) nxt[j] = pv_load(su, ld, n_bin, u, t0 + PVOC_AHEAD + j);   // beside this stretch's chain
#pragma unroll
        for (int j = 0; j < PVOC_AHEAD; ++j) {
            const long t = t0 + j;
            if (t < T) {                                   // (uniform)
                const pv_rows r = cur[j];
                double m0, a, b, m1, c, d;
                pv_polar((double)r.re0, (double)r.im0, m0, a, b);
                pv_polar((double)r.re1, (double)r.im1, m1, c, d);
                const double mag = (1.0 - r.a) * m0 + r.a * m1;
                ou[t * ld] = (float)(mag * pr);
                ou[t * ld + n_bin] = (float)(mag * pi);
                const double wr = c * a + d * b, wi = d * a - c * b;
                const double qr = pr * wr - pi * wi, qi = pr * wi + pi * wr;
                const double mq = sqrt(qr * qr + qi * qi);
                pr = qr / mq;
                pi = qi / mq;
            }
        }
#pragma unroll
        for (int j = 0; j < PVOC_AHEAD; ++j) cur[j] = nxt[j];
    }
}

}  // namespace

extern "C" int pk_pvoc_num_frames(int64_t frames, double rate, int64_t* out_frames) {
    if (!out_frames) PK_FAIL(PK_EINVAL, "pk_pvoc_num_frames: NULL argument");
    if (frames < 1) PK_FAIL(PK_EINVAL, "pk_pvoc_num_frames: %lld frames; a spectrogram has at least one", (long long)frames);
    if (!std::isfinite(rate) || !(rate > 0.0)) PK_FAIL(PK_EINVAL, "pk_pvoc_num_frames: rate = %g must be finite and > 0", rate);
    const double T = pvoc_num_frames(frames, rate);
    if (!(T < (double)PVOC_MAX_FRAMES))
        PK_FAIL(PK_EINVAL, "pk_pvoc_num_frames: %lld frames at rate %g give %g frames; the limit is below 2^31", (long long)frames, rate, T);
    *out_frames = (int64_t)T;
    return PK_OK;
}

extern "C" int pk_pvoc_run(pk_ctx* ctx, const float* spec, const int32_t* frames, int32_t B, int32_t n_bin, const double* rates,
                           float* out) {
    if (!ctx || !spec || !frames || !rates || !out) PK_FAIL(PK_EINVAL, "pk_pvoc_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pvoc_run: batch size must be positive");
    if (n_bin < 1) PK_FAIL(PK_EINVAL, "pk_pvoc_run: n_bin = %d; a row has at least one bin", (int)n_bin);
    if (B > PVOC_MAX_BATCH) PK_FAIL(PK_EUNSUPPORTED, "pk_pvoc_run: %d utterances; the engine's envelope is %d in a call", (int)B, PVOC_MAX_BATCH);
    std::vector<pvoc_utt> tab(B);
    long soff = 0, ooff = 0;
    for (int b = 0; b < B; ++b) {
        int64_t T = 0;
        if (frames[b] < 1) PK_FAIL(PK_EINVAL, "pk_pvoc_run: utterance %d has %d frames; a spectrogram has at least one", b, (int)frames[b]);
        if (!std::isfinite(rates[b]) || !(rates[b] > 0.0))
            PK_FAIL(PK_EINVAL, "pk_pvoc_run: utterance %d has rate = %g; a rate must be finite and > 0", b, rates[b]);
        PK_TRY(pk_pvoc_num_frames(frames[b], rates[b], &T));
        tab[b] = {soff, ooff, rates[b], (int)frames[b], (int)T};
        soff += frames[b];
        ooff += T;
    }
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    PK_TRY(pk_upload(ctx, sc->pvoc_tab, tab.data(), tab.size() * sizeof(pvoc_utt)));
    PK_LAUNCH(ctx, "pvoc", k_pvoc, dim3((unsigned)pk_div_up(n_bin, PVOC_THREADS), (unsigned)B), dim3(PVOC_THREADS), 0, spec,
              (const pvoc_utt*)sc->pvoc_tab.as<pvoc_utt>(), (int)n_bin, out);
    return PK_OK;
}
