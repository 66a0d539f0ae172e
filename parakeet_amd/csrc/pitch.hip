// pitch.hip -- frame-level f0 of ragged batches on gfx950: the estimator of DESIGN.md 4.5e (difference function, cumulative-mean
// normalisation, absolute threshold, parabolic refinement -- NOT pyworld's DIO + StoneMask), and the reference's
// continuous-f0 / log step for f0 from any estimator.  Geometry: pk_pitch.h.
//
// k_pitch: one workgroup owns one tile of F frames of one utterance.  It stages the tile's samples in LDS (samples outside the
// utterance are zeros by a select, the packed buffer's neighbours are never read).  Phase 1: a work item (frame, lag group)
// sums (x[s + j] - x[s + j + tau])^2 over j ascending, one fp32 FMA chain per lag, R lags per item; d goes to LDS.  Phase 2:
// one wave per frame turns its row of d into d' (a prefix sum over tau in chunks of 64 lags: a shuffle scan inside the
// chunk, then the carry of the chunks before it), finds the first lag under the threshold and the end of the descent that
// follows as min-reductions over the lanes, and lane 0 refines.  Every sum has one fixed order that involves neither the
// batch, nor the tile's position, nor the grid: a frame's result is the same bits wherever it is computed.
//
// k_cont_f0: one workgroup per utterance walks its track in chunks of 256 frames, forwards with a max-scan of "last voiced
// index" (kept per frame in a workspace), then backwards with a min-scan of "next voiced index", and writes the result.
#include <vector>

#include "pk_common.h"
#include "pk_pitch.h"

namespace {

struct pt_utt {
    long xoff;      // first sample of the utterance in the packed input
    long foff;      // first frame in the packed outputs
    int n_in;
    int n_frames;
};

constexpr int PT_NONE = 0x7fffffff;

__device__ __forceinline__ int pt_wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(PT_THREADS) void k_pitch(const float* __restrict__ x, const pt_utt* __restrict__ utts,
                                                      float* __restrict__ f0_out, int* __restrict__ lag_out,
                                                      float* __restrict__ cmnd_out, int hop, int tau_min, int tau_max, int W,
                                                      int G, int F, int span, float threshold, double sr) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int R = PT_R;
    float* xs = lds;                       // span staged samples: xs[k] = x~[fr0 * hop - L / 2 + k]
    float* dl = lds + span;                // F rows of tau_max + 1: d, then d'
    const pt_utt u = utts[blockIdx.y];
    const int fr0 = blockIdx.x * F;        // the tile's first frame
    if (fr0 >= u.n_frames) return;         // (uniform over the workgroup)
    const int nf = u.n_frames - fr0 < F ? u.n_frames - fr0 : F;
    const int row = tau_max + 1;
    const long m0 = (long)fr0 * hop - (W + tau_max) / 2;
    const float* xu = x + u.xoff;
    for (int s = threadIdx.x; s < span; s += PT_THREADS) {
        const long m = m0 + s;
        xs[s] = (m >= 0 && m < u.n_in) ? xu[m] : 0.f;
    }
    __syncthreads();
    // ---- phase 1: the difference function
    const int n_items = nf * G;
    for (int it = threadIdx.x; it < n_items; it += PT_THREADS) {
        const int f = it / G, g = it - f * G;
        const int tau0 = 1 + g * R;
        const float* xr = xs + f * hop;    // xr[j] = x~[s + j]
        const float* xw = xr + tau0;       // xw[j + q] = x~[s + j + tau0 + q]
        float acc[R], w[R];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = 0.f;
#pragma unroll
        for (int q = 0; q < R - 1; ++q) w[q] = xw[q];
        w[R - 1] = 0.f;
        int j = 0;
        for (; j + R <= W; j += R) {
#pragma unroll
            for (int t = 0; t < R; ++t) {              // step j + t: the window's slot (t + q) % R holds xw[j + t + q]
                w[(t + R - 1) % R] = xw[j + t + R - 1];
                const float r = xr[j + t];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float e = r - w[(t + q) % R];
                    acc[q] = __builtin_fmaf(e, e, acc[q]);
                }
            }
        }
        for (; j < W; ++j) {                           // the last W % R steps: the same chain, read directly
            const float r = xr[j];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float e = r - xw[j + q];
                acc[q] = __builtin_fmaf(e, e, acc[q]);
            }
        }
        float* dr = dl + f * row;
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (tau0 + q <= tau_max) dr[tau0 + q] = acc[q];
    }
    __syncthreads();
    // ---- phase 2: one wave per frame
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int fb = 0; fb < F; fb += PT_THREADS / 64) {  // (uniform trip count: the barriers below are reached by every wave)
        const int f = fb + wave;
        const bool live = f < nf;
        float* dr = dl + (live ? f : 0) * row;
        if (live) {
            float carry = 0.f;
            for (int base = 0; base < tau_max; base += 64) {
                const int tau = base + lane + 1;
                const float d = tau <= tau_max ? dr[tau] : 0.f;
                float s = d;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float o = __shfl_up(s, off, 64);
                    if (lane >= off) s += o;
                }
                const float c = carry + s;
                carry = __shfl(c, 63, 64);
                if (tau <= tau_max) dr[tau] = c > 0.f ? (d * (float)tau) / c : 1.f;
            }
            if (lane == 0) dr[0] = 1.f;
        }
        __syncthreads();
        if (live) {
            const long fr = u.foff + fr0 + f;
            if (cmnd_out)
                for (int t = lane; t < row; t += 64) cmnd_out[fr * row + t] = dr[t];
            int t0 = PT_NONE;
            for (int t = tau_min + lane; t <= tau_max - 1; t += 64)
                if (dr[t] < threshold) {
                    t0 = t;
                    break;
                }
            t0 = pt_wave_min(t0);
            int ts = PT_NONE;
            if (t0 != PT_NONE) {                       // (uniform over the wave)
                for (int t = t0 + lane; t <= tau_max - 1; t += 64)
                    if (!(t + 1 <= tau_max - 1 && dr[t + 1] < dr[t])) {
                        ts = t;
                        break;
                    }
                ts = pt_wave_min(ts);                  // tau_max - 1 always stops: ts is a lag
            }
            if (lane == 0) {
                float f0 = 0.f;
                int lag = 0;
                if (ts != PT_NONE) {
                    const double a = dr[ts - 1], b = dr[ts], c = dr[ts + 1];
                    const double den = a - 2.0 * b + c;
                    const double delta = (a >= b && c >= b && den > 0.0) ? (a - c) / (2.0 * den) : 0.0;
                    f0 = (float)(sr / ((double)ts + delta));
                    lag = ts;
                }
                f0_out[fr] = f0;
                if (lag_out) lag_out[fr] = lag;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PT_SCAN_CHUNK) void k_cont_f0(const float* __restrict__ f0, const pt_utt* __restrict__ utts,
                                                           int* __restrict__ prev, float* __restrict__ out, int log_flag) {
    __shared__ int sm[PT_SCAN_CHUNK];
    const pt_utt u = utts[blockIdx.x];
    const float* f = f0 + u.foff;
    float* o = out + u.foff;
    int* pv = prev + u.foff;
    const int n = u.n_frames, tid = threadIdx.x;
    const int chunks = (n + PT_SCAN_CHUNK - 1) / PT_SCAN_CHUNK;
    if (log_flag & 2) {                                // no filling (uniform): the log step alone
        for (int i = tid; i < n; i += PT_SCAN_CHUNK) {
            float v = f[i];
            if ((log_flag & 1) && v != 0.f) v = (float)log((double)v);
            o[i] = v;
        }
        return;
    }
    int carry = -1;                                    // the last voiced frame before the chunk
    for (int ch = 0; ch < chunks; ++ch) {
        const int i = ch * PT_SCAN_CHUNK + tid;
        sm[tid] = (i < n && f[i] != 0.f) ? i : -1;
        __syncthreads();
        for (int off = 1; off < PT_SCAN_CHUNK; off <<= 1) {
            const int v = tid >= off ? sm[tid - off] : -1;
            __syncthreads();
            if (v > sm[tid]) sm[tid] = v;
            __syncthreads();
        }
        if (i < n) pv[i] = sm[tid] > carry ? sm[tid] : carry;
        const int last = sm[PT_SCAN_CHUNK - 1];
        carry = last > carry ? last : carry;
        __syncthreads();
    }
    if (carry < 0) {                                   // no voiced frame (uniform): the track as it is
        for (int i = tid; i < n; i += PT_SCAN_CHUNK) o[i] = f[i];
        return;
    }
    carry = PT_NONE;                                   // the first voiced frame after the chunk
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int i = ch * PT_SCAN_CHUNK + tid;
        sm[tid] = (i < n && f[i] != 0.f) ? i : PT_NONE;
        __syncthreads();
        for (int off = 1; off < PT_SCAN_CHUNK; off <<= 1) {
            const int v = tid + off < PT_SCAN_CHUNK ? sm[tid + off] : PT_NONE;
            __syncthreads();
            if (v < sm[tid]) sm[tid] = v;
            __syncthreads();
        }
        if (i < n) {                                   // (prev[i] was written by this very thread)
            const int a = pv[i], b = sm[tid] < carry ? sm[tid] : carry;
            float v;
            if (a < 0) v = f[b];
            else if (b == PT_NONE) v = f[a];
            else if (a == b) v = f[i];
            else {
                const double fa = f[a], fb = f[b];
                v = (float)(fa + (fb - fa) * (double)(i - a) / (double)(b - a));
            }
            if ((log_flag & 1) && v != 0.f) v = (float)log((double)v);
            o[i] = v;
        }
        const int first = sm[0];
        carry = first < carry ? first : carry;
        __syncthreads();
    }
}

}  // namespace

struct pk_pitch {
    pk_ctx* ctx = nullptr;
    pk_pitch_cfg cfg;
    pt_plan plan;
    pk_dbuf ws_utt, ws_in, ws_f0, ws_lag, ws_cmnd;
};

extern "C" int pk_pitch_create(pk_ctx* ctx, const pk_pitch_cfg* cfg, pk_pitch** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_pitch_create: NULL argument");
    *out = nullptr;
    const pk_pitch_cfg& c = *cfg;
    if (c.sr < 1) PK_FAIL(PK_EINVAL, "pitch: sr = %d must be positive", (int)c.sr);
    if (!(c.threshold == c.threshold)) PK_FAIL(PK_EINVAL, "pitch: the threshold is not a number");
    if (c.tau_max > PT_MAX_TAU || c.tau_max < 4)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: tau_max = %d; the engine's envelope is 4 ... %d lags", (int)c.tau_max, PT_MAX_TAU);
    if (c.tau_min < 2 || c.tau_min > c.tau_max - 2)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: tau_min = %d; it must be in 2 ... tau_max - 2 = %d", (int)c.tau_min, (int)c.tau_max - 2);
    if (c.win < 1 || c.win > 2 * c.tau_max)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: a window of %d samples; the limit is 1 ... 2 * tau_max = %d", (int)c.win,
                2 * (int)c.tau_max);
    if (c.hop < 1 || c.hop > PT_MAX_HOP) PK_FAIL(PK_EUNSUPPORTED, "pitch: hop = %d; the limit is 1 ... %d", (int)c.hop, PT_MAX_HOP);
    pk_pitch* h = new pk_pitch();
    h->ctx = ctx;
    h->cfg = c;
    h->plan = pt_make_plan(c.hop, c.tau_max, c.win);
    *out = h;
    return PK_OK;
}

extern "C" int pk_pitch_frames(pk_pitch* h, int64_t n_samples, int32_t* frames) {
    if (!h || !frames) PK_FAIL(PK_EINVAL, "pk_pitch_frames: NULL argument");
    if (n_samples < 0 || n_samples > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_pitch_frames: n_samples must be in 0 ... 2^31 - 1");
    *frames = (int32_t)(n_samples / h->cfg.hop + 1);
    return PK_OK;
}

extern "C" int pk_pitch_tile_frames(pk_pitch* h, int32_t* tile) {
    if (!h || !tile) PK_FAIL(PK_EINVAL, "pk_pitch_tile_frames: NULL argument");
    *tile = h->plan.F;
    return PK_OK;
}

extern "C" int pk_pitch_run(pk_pitch* h, const float* wav, const int32_t* lens, int32_t B, float* f0_out, int32_t* lag_out,
                            float* cmnd_out, int32_t flags) {
    if (!h || !wav || !lens || !f0_out) PK_FAIL(PK_EINVAL, "pk_pitch_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pitch_run: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pt_plan& p = h->plan;
    const pk_pitch_cfg& c = h->cfg;
    std::vector<pt_utt> tab(B);
    long sum_in = 0, sum_fr = 0, max_tiles = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "pk_pitch_run: utterance %d is empty (%d samples)", b, (int)lens[b]);
        const int nf = lens[b] / c.hop + 1;
        tab[b] = {sum_in, sum_fr, lens[b], nf};
        sum_in += lens[b];
        sum_fr += nf;
        const long tiles = (nf + p.F - 1) / p.F;
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    PK_TRY(h->ws_utt.reserve(tab.size() * sizeof(pt_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utt.p, tab.data(), tab.size() * sizeof(pt_utt), hipMemcpyHostToDevice, ctx->stream));
    const float* d_in = wav;
    float* d_f0 = f0_out;
    int* d_lag = lag_out;
    float* d_cm = cmnd_out;
    const size_t cm_bytes = (size_t)sum_fr * p.row * 4;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)sum_in * 4));
        PK_TRY(h->ws_f0.reserve((size_t)sum_fr * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, wav, (size_t)sum_in * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = h->ws_in.as<float>();
        d_f0 = h->ws_f0.as<float>();
        if (lag_out) {
            PK_TRY(h->ws_lag.reserve((size_t)sum_fr * 4));
            d_lag = h->ws_lag.as<int>();
        }
        if (cmnd_out) {
            PK_TRY(h->ws_cmnd.reserve(cm_bytes));
            d_cm = h->ws_cmnd.as<float>();
        }
    }
    PK_HIP(hipStreamSynchronize(ctx->stream));             // `tab` leaves scope with this call
    const size_t lds = ((size_t)p.span + (size_t)p.F * p.row) * sizeof(float);
    constexpr int GRID_Y = 32768;                          // utterances per launch (grid.y is a 16-bit quantity)
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        PK_LAUNCH(ctx, "pitch", k_pitch, dim3((unsigned)max_tiles, (unsigned)nb), dim3(PT_THREADS), lds, d_in,
                  h->ws_utt.as<pt_utt>() + b0, d_f0, d_lag, d_cm, (int)c.hop, (int)c.tau_min, (int)c.tau_max, (int)c.win, p.G, p.F,
                  p.span, c.threshold, (double)c.sr);
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(f0_out, d_f0, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (lag_out) PK_HIP(hipMemcpyAsync(lag_out, d_lag, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (cmnd_out) PK_HIP(hipMemcpyAsync(cmnd_out, d_cm, cm_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" void pk_pitch_destroy(pk_pitch* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->ws_utt, &h->ws_in, &h->ws_f0, &h->ws_lag, &h->ws_cmnd};
    for (auto* b : bufs) b->release();
    delete h;
}

extern "C" int pk_op_continuous_f0(pk_ctx* ctx, const float* f0, const int32_t* frames, int32_t B, int32_t log_flag,
                                   float* out) {
    if (!ctx || !f0 || !frames || !out) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: batch size must be positive");
    if (log_flag < 0 || log_flag > 3) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: log_flag = %d is not in 0 ... 3", (int)log_flag);
    PK_DEVICE(ctx->device);
    std::vector<pt_utt> tab(B);
    long sum = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: track %d is empty (%d frames)", b, (int)frames[b]);
        tab[b] = {0, sum, 0, frames[b]};
        sum += frames[b];
    }
    pk_dbuf d_tab, d_prev;
    int rc = pk_upload(ctx, d_tab, tab.data(), tab.size() * sizeof(pt_utt));
    if (rc == PK_OK) rc = d_prev.reserve((size_t)sum * sizeof(int));
    constexpr int GRID_X = 1 << 20;
    for (int b0 = 0; rc == PK_OK && b0 < B; b0 += GRID_X) {
        const int nb = B - b0 < GRID_X ? B - b0 : GRID_X;
        hipLaunchKernelGGL(k_cont_f0, dim3(nb), dim3(PT_SCAN_CHUNK), 0, ctx->stream, f0, d_tab.as<pt_utt>() + b0,
                           d_prev.as<int>(), out, (int)log_flag);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            pk_set_error("pk_op_continuous_f0: %s", hipGetErrorString(e));
            rc = PK_EHIP;
        }
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // the two buffers are released below
    if (e != hipSuccess && rc == PK_OK) {
        pk_set_error("pk_op_continuous_f0: %s", hipGetErrorString(e));
        rc = PK_EHIP;
    }
    d_tab.release();
    d_prev.release();
    return rc;
}
