// stoi.hip -- short-time objective intelligibility (STOI / ESTOI) of ragged batches on gfx950: silent-frame
// removal, one-third-octave band magnitudes on the radix FFT of rfft.hip, and the 30-frame segment correlations in float64.
// The definition, the buffers' geometry and every summation order: pk_stoi.h.  This file is compiled without contraction
// (build.py): a fused multiply-add appears only where it is written (__builtin_fmaf).
//
// Every stage is enqueued on the context's stream; the kept-frame counts never reach the host (buffers and grids are sized by
// the frame counts F(L), which the host knows).  A call uploads its table of utterances first (pk_upload synchronises, as
// everywhere) and reads nothing back: the results stay on the device for the caller to fetch once.
#include <vector>

#include "pk_common.h"
#include "pk_rfft.h"
#include "pk_stoi.h"

namespace {

struct st_utt {
    long xoff;      // first sample in the packed signals
    long foff;      // first frame in the packed per-frame arrays (energies, flags, index list)
    long roff;      // first row (of 128 floats) of the utterance's region in the padded buffers
    long boff;      // first row in the packed band / spectrum arrays
    long soff;      // first segment value
    int L;          // samples
    int F;          // frames of the signal, F(L)
    int nb;         // band rows the host knows of: F(L) for a given signal; the upper bound max(F - 1, 0) in the pipeline
    int pad_;
};
static_assert(sizeof(st_utt) % 8 == 0, "tables are arrays of st_utt");

constexpr int ST_WAVES = STOI_THREADS / 64;

__global__ __launch_bounds__(STOI_THREADS) void k_stoi_energy(const float* __restrict__ x, const st_utt* __restrict__ utts,
                                                              const float* __restrict__ win, float* __restrict__ ss) {
    const st_utt u = utts[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (f >= u.F) return;                              // (uniform over the wave; no barrier below)
    const float* xf = x + u.xoff + f * STOI_HOP;       // f * 128 + 255 < L by the frame rule
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < STOI_FRAME / 64; ++q) {        // THE ORDER of pk_stoi.h
        const float p = win[lane + 64 * q] * xf[lane + 64 * q];
        acc = __builtin_fmaf(p, p, acc);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) ss[u.foff + f] = acc;
}

__device__ __forceinline__ double st_db(float ss) { return 20.0 * log10(sqrt((double)ss) + STOI_EPS); }

__global__ __launch_bounds__(STOI_THREADS) void k_stoi_mask(const float* __restrict__ ss, const st_utt* __restrict__ utts,
                                                            float* __restrict__ energy_out, unsigned char* __restrict__ keep_out,
                                                            int* __restrict__ idx, int* __restrict__ kept) {
    __shared__ float smf[ST_WAVES];
    __shared__ int swv[ST_WAVES];
    const st_utt u = utts[blockIdx.x];
    const float* s = ss + u.foff;
    const int n = u.F, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = 0.f;                                    // ss >= 0; a NaN never becomes the maximum and is never kept
    for (int i = tid; i < n; i += STOI_THREADS) mx = fmaxf(mx, s[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) smf[wave] = mx;
    __syncthreads();
    mx = smf[0];
#pragma unroll
    for (int k = 1; k < ST_WAVES; ++k) mx = fmaxf(mx, smf[k]);
    const double emax = st_db(mx);
    int carry = 0;                                     // kept frames before the chunk
    for (int k0 = 0; k0 < n; k0 += STOI_THREADS) {
        const int i = k0 + tid;
        bool keep = false;
        double e = 0.0;
        if (i < n) {
            e = st_db(s[i]);
            keep = emax - STOI_RANGE_DB - e < 0.0;
        }
        int incl = keep ? 1 : 0;                       // kept frames of the wave up to and including this lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        __syncthreads();                               // swv of the previous chunk has been read
        if (lane == 63) swv[wave] = incl;
        __syncthreads();
        int base = carry, total = 0;
#pragma unroll
        for (int v = 0; v < ST_WAVES; ++v) {
            base += v < wave ? swv[v] : 0;
            total += swv[v];
        }
        if (i < n) {
            if (keep) idx[u.foff + base + incl - 1] = i;
            if (energy_out) energy_out[u.foff + i] = (float)e;
            if (keep_out) keep_out[u.foff + i] = keep ? 1 : 0;
        }
        carry += total;
    }
    if (tid == 0) kept[blockIdx.x] = carry;
}

// raw != 0: the signals as they are (x alone), zeros behind them, every frame of them transformed.
// raw == 0: stage 2 of pk_stoi.h for x and y through idx / kept.
// pad: the two padded buffers one after the other (y's rows start at TR); rowmap: 2 TR entries (TR under raw).
__global__ __launch_bounds__(STOI_THREADS) void k_stoi_rebuild(const float* __restrict__ x, const float* __restrict__ y,
                                                               const st_utt* __restrict__ utts, const float* __restrict__ win,
                                                               const int* __restrict__ idx, const int* __restrict__ kept,
                                                               float* __restrict__ pad, int* __restrict__ rowmap, long TR,
                                                               long TB, int raw) {
    const st_utt u = utts[blockIdx.y];
    const long n = (long)blockIdx.x * STOI_THREADS + threadIdx.x;
    const long region = ((long)u.F + 3) * STOI_HOP;
    if (n >= region) return;
    const long c = n / STOI_HOP;
    const int r = (int)(n % STOI_HOP);
    float vx = 0.f, vy = 0.f;
    long rows;                                         // frames of this utterance that are transformed
    if (raw) {
        if (n < u.L) vx = x[u.xoff + n];
        rows = u.F;
    } else {
        const int K = kept[blockIdx.y];
        const int* ix = idx + u.foff;
        if (c >= 1 && c <= K) {                        // the earlier frame first
            const long s = u.xoff + (long)ix[c - 1] * STOI_HOP + r + STOI_HOP;
            const float w = win[r + STOI_HOP];
            vx = w * x[s];
            vy = w * y[s];
        }
        if (c < K) {
            const long s = u.xoff + (long)ix[c] * STOI_HOP + r;
            const float w = win[r];
            vx = vx + w * x[s];
            vy = vy + w * y[s];
        }
        rows = K > 1 ? K - 1 : 0;
    }
    const long o = u.roff * STOI_HOP + n;
    pad[o] = vx;
    if (!raw) pad[TR * STOI_HOP + o] = vy;
    if (r == 0) {
        rowmap[u.roff + c] = c < rows ? (int)(u.boff + c) : -1;
        if (!raw) rowmap[TR + u.roff + c] = c < rows ? (int)(TB + u.boff + c) : -1;
    }
}

struct st_edges {
    int lo[STOI_BANDS], hi[STOI_BANDS];
};

// spec: rows of re | im (257 floats each); a row the transform skipped is not read.  valid[g * TB + boff + m] rows: m below the
// utterance's count.
__global__ __launch_bounds__(STOI_THREADS) void k_stoi_bands(const float* __restrict__ spec, const st_utt* __restrict__ utts,
                                                             const int* __restrict__ kept, st_edges ed, long TB, int nsig,
                                                             float* __restrict__ bands) {
    const st_utt u = utts[blockIdx.y];
    const long t = (long)blockIdx.x * STOI_THREADS + threadIdx.x;
    const long m = t >> 4;
    const int j = (int)(t & 15);
    long rows = u.nb;
    if (kept) {
        const int K = kept[blockIdx.y];
        rows = K > 1 ? K - 1 : 0;
    }
    if (m >= rows || j >= STOI_BANDS) return;
    for (int g = 0; g < nsig; ++g) {
        const long row = g * TB + u.boff + m;
        const float* re = spec + row * (STOI_NFFT + 2);
        const float* im = re + (STOI_NFFT / 2 + 1);
        float s = 0.f;
        for (int k = ed.lo[j]; k < ed.hi[j]; ++k) s = s + (re[k] * re[k] + im[k] * im[k]);
        bands[row * STOI_BANDS + j] = sqrtf(s);
    }
}

constexpr int ST_RUN_FRAMES = STOI_RUN + STOI_SEG - 1;         // 33
constexpr int ST_RUN_FLOATS = ST_RUN_FRAMES * STOI_BANDS;      // 495

__global__ __launch_bounds__(64 * STOI_SEG_WAVES) void k_stoi_segments(const float* __restrict__ bx, const float* __restrict__ by,
                                                                      const st_utt* __restrict__ utts,
                                                                      const int* __restrict__ kept, int extended,
                                                                      double* __restrict__ dseg) {
    __shared__ float sx[STOI_SEG_WAVES][ST_RUN_FLOATS + 1];
    __shared__ float sy[STOI_SEG_WAVES][ST_RUN_FLOATS + 1];
    __shared__ double rs[STOI_SEG_WAVES][STOI_RUN][STOI_BANDS][4];   // ESTOI: a row's mean_x, den_x, mean_y, den_y
    __shared__ double part[STOI_SEG_WAVES][STOI_RUN][32];
    const st_utt u = utts[blockIdx.y];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long rows = u.nb;
    if (kept) {
        const int K = kept[blockIdx.y];
        rows = K > 1 ? K - 1 : 0;
    }
    const long S = rows - (STOI_SEG - 1);
    const long m0 = ((long)blockIdx.x * STOI_SEG_WAVES + w) * STOI_RUN;
    const int ns = m0 < S ? (int)(S - m0 < STOI_RUN ? S - m0 : STOI_RUN) : 0;     // segments of this wave's run (uniform)
    if (ns > 0) {
        const int nfl = (ns + STOI_SEG - 1) * STOI_BANDS;                        // frames m0 ... m0 + ns + 28 < rows
        const float* gx = bx + (u.boff + m0) * STOI_BANDS;
        const float* gy = by + (u.boff + m0) * STOI_BANDS;
        for (int i = lane; i < nfl; i += 64) {
            sx[w][i] = gx[i];
            sy[w][i] = gy[i];
        }
    }
    __syncthreads();
    const float* X = sx[w];
    const float* Y = sy[w];
    {
        const int s = lane >> 4, j = lane & 15;
        if (s < ns && j < STOI_BANDS) {
            const float* xr = X + s * STOI_BANDS + j;                            // value n of the row: xr[n * 15]
            const float* yr = Y + s * STOI_BANDS + j;
            if (!extended) {
                double nx2 = 0.0, ny2 = 0.0, sumx = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    const double a = (double)xr[n * STOI_BANDS], b = (double)yr[n * STOI_BANDS];
                    nx2 = nx2 + a * a;
                    ny2 = ny2 + b * b;
                    sumx = sumx + a;
                }
                const double alpha = sqrt(nx2) / (sqrt(ny2) + STOI_EPS);
                double sumy = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    const double a = (double)xr[n * STOI_BANDS], b = (double)yr[n * STOI_BANDS];
                    sumy = sumy + fmin(alpha * b, a * STOI_CLIP);
                }
                const double mxv = sumx / (double)STOI_SEG, myv = sumy / (double)STOI_SEG;
                double vx2 = 0.0, vy2 = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    const double a = (double)xr[n * STOI_BANDS], b = (double)yr[n * STOI_BANDS];
                    const double xc = a - mxv, yc = fmin(alpha * b, a * STOI_CLIP) - myv;
                    vx2 = vx2 + xc * xc;
                    vy2 = vy2 + yc * yc;
                }
                const double dx = sqrt(vx2) + STOI_EPS, dy = sqrt(vy2) + STOI_EPS;
                double c = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    const double a = (double)xr[n * STOI_BANDS], b = (double)yr[n * STOI_BANDS];
                    const double xh = (a - mxv) / dx, yh = (fmin(alpha * b, a * STOI_CLIP) - myv) / dy;
                    c = c + xh * yh;
                }
                part[w][s][j] = c;
            } else {
                double sumx = 0.0, sumy = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    sumx = sumx + (double)xr[n * STOI_BANDS];
                    sumy = sumy + (double)yr[n * STOI_BANDS];
                }
                const double mxv = sumx / (double)STOI_SEG, myv = sumy / (double)STOI_SEG;
                double vx2 = 0.0, vy2 = 0.0;
                for (int n = 0; n < STOI_SEG; ++n) {
                    const double xc = (double)xr[n * STOI_BANDS] - mxv, yc = (double)yr[n * STOI_BANDS] - myv;
                    vx2 = vx2 + xc * xc;
                    vy2 = vy2 + yc * yc;
                }
                rs[w][s][j][0] = mxv;
                rs[w][s][j][1] = sqrt(vx2) + STOI_EPS;
                rs[w][s][j][2] = myv;
                rs[w][s][j][3] = sqrt(vy2) + STOI_EPS;
            }
        }
    }
    __syncthreads();
    if (extended) {
#pragma unroll
        for (int step = 0; step < STOI_RUN / 2; ++step) {
            const int s = 2 * step + (lane >> 5), n = lane & 31;
            if (s < ns && n < STOI_SEG) {
                const float* xc = X + (s + n) * STOI_BANDS;                      // column n of segment s: its 15 bands
                const float* yc = Y + (s + n) * STOI_BANDS;
                double vx[STOI_BANDS], vy[STOI_BANDS];
                double sumx = 0.0, sumy = 0.0;
#pragma unroll
                for (int j = 0; j < STOI_BANDS; ++j) {
                    vx[j] = ((double)xc[j] - rs[w][s][j][0]) / rs[w][s][j][1];
                    vy[j] = ((double)yc[j] - rs[w][s][j][2]) / rs[w][s][j][3];
                    sumx = sumx + vx[j];
                    sumy = sumy + vy[j];
                }
                const double mxv = sumx / (double)STOI_BANDS, myv = sumy / (double)STOI_BANDS;
                double vx2 = 0.0, vy2 = 0.0;
#pragma unroll
                for (int j = 0; j < STOI_BANDS; ++j) {
                    vx[j] = vx[j] - mxv;
                    vy[j] = vy[j] - myv;
                    vx2 = vx2 + vx[j] * vx[j];
                    vy2 = vy2 + vy[j] * vy[j];
                }
                const double dx = sqrt(vx2) + STOI_EPS, dy = sqrt(vy2) + STOI_EPS;
                double c = 0.0;
#pragma unroll
                for (int j = 0; j < STOI_BANDS; ++j) c = c + (vx[j] / dx) * (vy[j] / dy);
                part[w][s][n] = c;
            }
        }
    }
    __syncthreads();
    if (lane < ns) {                                                             // lane s: the segment's value, ascending
        const int cnt = extended ? STOI_SEG : STOI_BANDS;
        double d = 0.0;
        for (int i = 0; i < cnt; ++i) d = d + part[w][lane][i];
        dseg[u.soff + m0 + lane] = d;
    }
}

__global__ __launch_bounds__(STOI_RED_THREADS) void k_stoi_reduce(const double* __restrict__ dseg, const st_utt* __restrict__ utts,
                                                                  const int* __restrict__ kept, int extended,
                                                                  pk_stoi_result* __restrict__ res, double* __restrict__ d_out,
                                                                  int* __restrict__ seg_out) {
    __shared__ double a[STOI_RED_THREADS];
    const st_utt u = utts[blockIdx.x];
    const int t = threadIdx.x;
    long rows = u.nb;
    int K = u.F;
    if (kept) {
        K = kept[blockIdx.x];
        rows = K > 1 ? K - 1 : 0;
    }
    long S = rows - (STOI_SEG - 1);
    S = S > 0 ? S : 0;
    double acc = 0.0;
    for (long i = t; i < S; i += STOI_RED_THREADS) acc = acc + dseg[u.soff + i];
    a[t] = acc;
    __syncthreads();
    for (int h = STOI_RED_THREADS / 2; h >= 1; h >>= 1) {                        // THE ORDER of pk_stoi.h
        if (t < h) a[t] = a[t] + a[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const double den = (double)(extended ? STOI_SEG : STOI_BANDS) * (double)S;
        const double d = S > 0 ? a[0] / den : __builtin_nan("");
        if (res) {
            res[blockIdx.x].d = d;
            res[blockIdx.x].segments = (int)S;
            res[blockIdx.x].kept = K;
            res[blockIdx.x].frames = u.F;
        }
        if (d_out) d_out[blockIdx.x] = d;
        if (seg_out) seg_out[blockIdx.x] = (int)S;
    }
}

// ------------------------------------------------------------------------------------------------ host side
size_t st_align(size_t b) { return (b + 255) / 256 * 256; }

struct st_plan {
    std::vector<st_utt> tab;
    long TF = 0, TR = 0, TB = 0, TS = 0, maxF = 0, maxS = 0, maxB = 0;
};

// offs: B + 1 ascending sample offsets (utterance b is [offs[b], offs[b + 1])).  pipeline: band rows are the upper bound F - 1
int st_table(const char* who, const int64_t* offs, int B, bool pipeline, st_plan& p) {
    if (B <= 0) PK_FAIL(PK_EINVAL, "%s: batch size must be positive", who);
    if (B > STOI_MAX_BATCH) PK_FAIL(PK_EUNSUPPORTED, "%s: %d utterances; the engine's envelope is %d in a call", who, B, STOI_MAX_BATCH);
    if (offs[0] < 0) PK_FAIL(PK_EINVAL, "%s: a negative offset", who);
    p.tab.resize(B);
    for (int b = 0; b < B; ++b) {
        const int64_t L = offs[b + 1] - offs[b];
        if (L < 0) PK_FAIL(PK_EINVAL, "%s: the offsets of utterance %d descend", who, b);
        if (L > STOI_MAX_SAMPLES)
            PK_FAIL(PK_EUNSUPPORTED, "%s: utterance %d has %lld samples; the engine's envelope is %ld", who, b, (long long)L, STOI_MAX_SAMPLES);
        const long F = stoi_frames(L);
        const long nb = pipeline ? (F > 1 ? F - 1 : 0) : F;
        const long Smax = nb - (STOI_SEG - 1) > 0 ? nb - (STOI_SEG - 1) : 0;
        p.tab[b] = {offs[b], p.TF, p.TR, p.TB, p.TS, (int)L, (int)F, (int)nb, 0};
        p.TF += F;
        p.TR += F + 3;
        p.TB += nb;
        p.TS += Smax;
        p.maxF = F > p.maxF ? F : p.maxF;
        p.maxB = nb > p.maxB ? nb : p.maxB;
        p.maxS = Smax > p.maxS ? Smax : p.maxS;
    }
    if (2 * p.TR > 0x3fffffffL) PK_FAIL(PK_EUNSUPPORTED, "%s: more than 2^29 frames in a call", who);
    return PK_OK;
}

// carve the context's grow-only workspace
struct st_ws {
    float* ss;
    unsigned char* keep;
    int* idx;
    int* kept;
    float* pad;
    int* rowmap;
    float* spec;
    float* bands;
    double* dseg;
};

int st_reserve(pk_ctx_scratch* sc, const st_plan& p, int B, int nsig, st_ws& w) {
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += st_align(bytes ? bytes : 1);
        return at;
    };
    const size_t o_ss = take((size_t)p.TF * 4), o_keep = take((size_t)p.TF), o_idx = take((size_t)p.TF * 4), o_kept = take((size_t)B * 4),
                 o_pad = take((size_t)nsig * p.TR * STOI_HOP * 4), o_map = take((size_t)nsig * p.TR * 4),
                 o_spec = take((size_t)nsig * p.TB * (STOI_NFFT + 2) * 4), o_bands = take((size_t)nsig * p.TB * STOI_BANDS * 4),
                 o_dseg = take((size_t)p.TS * 8);
    PK_TRY(sc->stoi_ws.reserve(o));
    unsigned char* base = sc->stoi_ws.as<unsigned char>();
    w.ss = reinterpret_cast<float*>(base + o_ss);
    w.keep = base + o_keep;
    w.idx = reinterpret_cast<int*>(base + o_idx);
    w.kept = reinterpret_cast<int*>(base + o_kept);
    w.pad = reinterpret_cast<float*>(base + o_pad);
    w.rowmap = reinterpret_cast<int*>(base + o_map);
    w.spec = reinterpret_cast<float*>(base + o_spec);
    w.bands = reinterpret_cast<float*>(base + o_bands);
    w.dseg = reinterpret_cast<double*>(base + o_dseg);
    return PK_OK;
}

// w followed by 256 zeros, float32 from float64: uploaded when this stream's scratch first needs it
int st_window(pk_ctx* ctx, pk_ctx_scratch* sc, const float** win) {
    if (!sc->stoi_win.p) {
        std::vector<float> h(STOI_NFFT, 0.f);
        for (int n = 0; n < STOI_FRAME; ++n)            // numpy.hanning(258)[n + 1]
            h[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(n + 1) / (double)(STOI_FRAME + 1)));
        PK_TRY(pk_upload(ctx, sc->stoi_win, h.data(), h.size() * sizeof(float)));
    }
    *win = sc->stoi_win.as<float>();
    return PK_OK;
}

st_edges st_edge_table() {
    st_edges e;
    stoi_edges(e.lo, e.hi);
    return e;
}

unsigned st_blocks(long items, long per) { return (unsigned)((items + per - 1) / per); }

int st_launch_mask(pk_ctx* ctx, const float* clean, const st_utt* dtab, const st_plan& p, int B, const float* win, const st_ws& w,
                   float* energy_out, unsigned char* keep_out, int* idx, int* kept) {
    if (p.maxF > 0)
        PK_LAUNCH(ctx, "stoi_energy", k_stoi_energy, dim3(st_blocks(p.maxF, ST_WAVES), B), dim3(STOI_THREADS), 0, clean, dtab, win, w.ss);
    PK_LAUNCH(ctx, "stoi_mask", k_stoi_mask, dim3(B), dim3(STOI_THREADS), 0, (const float*)w.ss, dtab, energy_out, keep_out, idx, kept);
    return PK_OK;
}

// the padded buffers -> band magnitudes (nsig signals of TB rows each)
int st_launch_bands(pk_ctx* ctx, const st_utt* dtab, const st_plan& p, int B, int nsig, const float* win, const int* kept,
                    const st_ws& w, float* bands) {
    if (p.maxB == 0) return PK_OK;
    PK_TRY(pk_rfft_forward(ctx, "stoi_rfft", w.pad, STOI_HOP, win, w.rowmap, (long)nsig * p.TR, STOI_NFFT, w.spec, STOI_NFFT + 2));
    PK_LAUNCH(ctx, "stoi_bands", k_stoi_bands, dim3(st_blocks(p.maxB * 16, STOI_THREADS), B), dim3(STOI_THREADS), 0,
              (const float*)w.spec, dtab, kept, st_edge_table(), p.TB, nsig, bands);
    return PK_OK;
}

int st_launch_segments(pk_ctx* ctx, const float* bx, const float* by, const st_utt* dtab, const st_plan& p, int B, const int* kept,
                       int extended, const st_ws& w, pk_stoi_result* res, double* d_out, int* seg_out) {
    if (p.maxS > 0)
        PK_LAUNCH(ctx, "stoi_segments", k_stoi_segments, dim3(st_blocks(p.maxS, STOI_RUN * STOI_SEG_WAVES), B),
                  dim3(64 * STOI_SEG_WAVES), 0, bx, by, dtab, kept, extended, w.dseg);
    PK_LAUNCH(ctx, "stoi_reduce", k_stoi_reduce, dim3(B), dim3(STOI_RED_THREADS), 0, (const double*)w.dseg, dtab, kept, extended, res,
              d_out, seg_out);
    return PK_OK;
}

}  // namespace

extern "C" int pk_stoi_band_edges(int32_t* lo, int32_t* hi) {
    if (!lo || !hi) PK_FAIL(PK_EINVAL, "pk_stoi_band_edges: NULL argument");
    const st_edges e = st_edge_table();
    for (int j = 0; j < STOI_BANDS; ++j) lo[j] = e.lo[j], hi[j] = e.hi[j];
    return PK_OK;
}

extern "C" int pk_stoi_num_frames(int64_t n_samples, int64_t* frames) {
    if (!frames) PK_FAIL(PK_EINVAL, "pk_stoi_num_frames: NULL argument");
    if (n_samples < 0) PK_FAIL(PK_EINVAL, "pk_stoi_num_frames: a negative length");
    *frames = stoi_frames(n_samples);
    return PK_OK;
}

extern "C" int pk_stoi_mask(pk_ctx* ctx, const float* clean, const int64_t* offs, int32_t B, float* energy_out, uint8_t* keep_out,
                            int32_t* index_out, int32_t* kept_out) {
    if (!ctx || !clean || !offs || !kept_out) PK_FAIL(PK_EINVAL, "pk_stoi_mask: NULL argument");
    st_plan p;
    PK_TRY(st_table("pk_stoi_mask", offs, B, false, p));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    const float* win;
    PK_TRY(st_window(ctx, sc, &win));
    st_ws w;
    PK_TRY(st_reserve(sc, p, B, 0, w));
    PK_TRY(pk_upload(ctx, sc->stoi_tab, p.tab.data(), p.tab.size() * sizeof(st_utt)));
    return st_launch_mask(ctx, clean, sc->stoi_tab.as<st_utt>(), p, B, win, w, energy_out, keep_out, index_out ? index_out : w.idx,
                          kept_out);
}

extern "C" int pk_stoi_bands(pk_ctx* ctx, const float* x, const int64_t* offs, int32_t B, float* bands_out) {
    if (!ctx || !x || !offs || !bands_out) PK_FAIL(PK_EINVAL, "pk_stoi_bands: NULL argument");
    st_plan p;
    PK_TRY(st_table("pk_stoi_bands", offs, B, false, p));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    const float* win;
    PK_TRY(st_window(ctx, sc, &win));
    PK_TRY(pk_rfft_prepare(ctx, STOI_NFFT));
    st_ws w;
    PK_TRY(st_reserve(sc, p, B, 1, w));
    PK_TRY(pk_upload(ctx, sc->stoi_tab, p.tab.data(), p.tab.size() * sizeof(st_utt)));
    const st_utt* dtab = sc->stoi_tab.as<st_utt>();
    PK_LAUNCH(ctx, "stoi_pad", k_stoi_rebuild, dim3(st_blocks((p.maxF + 3) * STOI_HOP, STOI_THREADS), B), dim3(STOI_THREADS), 0, x,
              (const float*)nullptr, dtab, win, (const int*)nullptr, (const int*)nullptr, w.pad, w.rowmap, p.TR, p.TB, 1);
    return st_launch_bands(ctx, dtab, p, B, 1, win, nullptr, w, bands_out);
}

extern "C" int pk_stoi_segments(pk_ctx* ctx, const float* bands_x, const float* bands_y, const int32_t* frames, int32_t B,
                                int32_t extended, double* d_out, int32_t* segments_out) {
    if (!ctx || !bands_x || !bands_y || !frames || !d_out) PK_FAIL(PK_EINVAL, "pk_stoi_segments: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_stoi_segments: batch size must be positive");
    if (B > STOI_MAX_BATCH)
        PK_FAIL(PK_EUNSUPPORTED, "pk_stoi_segments: %d utterances; the engine's envelope is %d in a call", (int)B, STOI_MAX_BATCH);
    st_plan p;
    p.tab.resize(B);
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 0) PK_FAIL(PK_EINVAL, "pk_stoi_segments: utterance %d has a negative frame count", b);
        const long nb = frames[b], Smax = nb - (STOI_SEG - 1) > 0 ? nb - (STOI_SEG - 1) : 0;
        p.tab[b] = {0, 0, 0, p.TB, p.TS, 0, (int)nb, (int)nb, 0};
        p.TB += nb;
        p.TS += Smax;
        p.maxS = Smax > p.maxS ? Smax : p.maxS;
    }
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    st_ws w;
    PK_TRY(st_reserve(sc, p, B, 0, w));
    PK_TRY(pk_upload(ctx, sc->stoi_tab, p.tab.data(), p.tab.size() * sizeof(st_utt)));
    return st_launch_segments(ctx, bands_x, bands_y, sc->stoi_tab.as<st_utt>(), p, B, nullptr, extended ? 1 : 0, w, nullptr, d_out,
                              segments_out);
}

extern "C" int pk_stoi_run(pk_ctx* ctx, const float* clean, const float* degraded, const int64_t* offs, int32_t B, int32_t extended,
                           pk_stoi_result* result_out) {
    if (!ctx || !clean || !degraded || !offs || !result_out) PK_FAIL(PK_EINVAL, "pk_stoi_run: NULL argument");
    st_plan p;
    PK_TRY(st_table("pk_stoi_run", offs, B, true, p));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    const float* win;
    PK_TRY(st_window(ctx, sc, &win));
    PK_TRY(pk_rfft_prepare(ctx, STOI_NFFT));
    st_ws w;
    PK_TRY(st_reserve(sc, p, B, 2, w));
    PK_TRY(pk_upload(ctx, sc->stoi_tab, p.tab.data(), p.tab.size() * sizeof(st_utt)));
    const st_utt* dtab = sc->stoi_tab.as<st_utt>();
    PK_TRY(st_launch_mask(ctx, clean, dtab, p, B, win, w, nullptr, nullptr, w.idx, w.kept));
    PK_LAUNCH(ctx, "stoi_rebuild", k_stoi_rebuild, dim3(st_blocks((p.maxF + 3) * STOI_HOP, STOI_THREADS), B), dim3(STOI_THREADS), 0,
              clean, degraded, dtab, win, (const int*)w.idx, (const int*)w.kept, w.pad, w.rowmap, p.TR, p.TB, 0);
    PK_TRY(st_launch_bands(ctx, dtab, p, B, 2, win, w.kept, w, w.bands));
    return st_launch_segments(ctx, w.bands, w.bands + p.TB * STOI_BANDS, dtab, p, B, w.kept, extended ? 1 : 0, w, result_out, nullptr,
                              nullptr);
}
