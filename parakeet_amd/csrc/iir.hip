// iir.hip -- cascades of biquads over ragged batches in float64, gated loudness (BS.1770, mono) on the same passes, and a
// per-utterance gain, on gfx950.  The definition, the chunk plan and every summation order: pk_iir.h.  This
// file is compiled without contraction and without the SLP vectoriser (build.py): every float64 operation of the recurrence
// is the separate operation the header writes, and the sections' independent chains stay scalar lines.
//
// A filter handle keeps its coefficients on the host (they reach the kernels as launch arguments) and the transition matrix P
// on the device.  A call uploads its table of utterances (pk_upload synchronises, as everywhere), enqueues its kernels on the
// context's stream and reads nothing back.
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_iir.h"

struct pk_iir {
    pk_ctx* ctx = nullptr;
    int S = 0;
    double sos[IIR_MAX_SECTIONS][6];
    pk_dbuf P;          // (2 S, 2 S) double, row-major
};

namespace {

struct iir_coef {
    double b0[IIR_MAX_SECTIONS], b1[IIR_MAX_SECTIONS], b2[IIR_MAX_SECTIONS], a1[IIR_MAX_SECTIONS], a2[IIR_MAX_SECTIONS];
};

struct iir_utt {
    long xoff;      // first sample in the packed signals
    long coff;      // first chunk in the per-chunk arrays
    long goff;      // first hop segment (loudness)
    int L;          // samples
    int nch;        // chunks, the partial one included
    int G;          // hop segments (loudness)
    float gain;     // k_gain
};
static_assert(sizeof(iir_utt) % 8 == 0, "tables are arrays of iir_utt");

// the recurrence of pk_iir.h: one sample through the S sections; returns the last section's output
template <int S>
__device__ __forceinline__ double iir_step(const iir_coef& k, double (&z)[2 * S], double v) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double o = k.b0[s] * v + z[2 * s];
        z[2 * s] = (k.b1[s] * v - k.a1[s] * o) + z[2 * s + 1];
        z[2 * s + 1] = k.b2[s] * v - k.a2[s] * o;
        v = o;
    }
    return v;
}

template <int S>
__global__ __launch_bounds__(64) void k_iir_transition(iir_coef k, double* __restrict__ P) {
    constexpr int n = 2 * S;
    const int j = threadIdx.x;
    if (j >= n) return;
    double z[n];
#pragma unroll
    for (int i = 0; i < n; ++i) z[i] = i == j ? 1.0 : 0.0;
    const float zero = 0.f;
    for (int t = 0; t < IIR_CHUNK; ++t) (void)iir_step<S>(k, z, (double)zero);
#pragma unroll
    for (int i = 0; i < n; ++i) P[i * n + j] = z[i];
}

// one stage of the wave's 64 chunks into the tile: row r = samples [64 sub, 64 sub + 64) of chunk cbase + r; zeros at or
// beyond `lim` samples of the utterance (lim >= 1).  The loads are unconditional, from an index clamped into the utterance, so
// that a row does not wait for the one before it (a load under a branch is followed by its own wait)
__device__ __forceinline__ void iir_stage_in(float* tile, const float* __restrict__ xu, long cbase, int sub, long lim, int lane) {
#pragma unroll 16
    for (int r = 0; r < IIR_LANES; ++r) {
        const long idx = (cbase + r) * IIR_CHUNK + sub * IIR_STAGE + lane;
        const float v = xu[idx < lim ? idx : lim - 1];
        tile[r * IIR_TILE_LD + lane] = idx < lim ? v : 0.f;
    }
}

template <int S>
__global__ __launch_bounds__(IIR_LANES) void k_iir_local(const float* __restrict__ x, const iir_utt* __restrict__ utts, iir_coef k,
                                                         double* __restrict__ q, long TC) {
    constexpr int n = 2 * S;
    __shared__ float tile[IIR_LANES * IIR_TILE_LD];
    const iir_utt u = utts[blockIdx.y];
    const int lane = threadIdx.x;
    const long nfull = u.L / IIR_CHUNK, cbase = (long)blockIdx.x * IIR_LANES, c = cbase + lane;
    if (cbase >= nfull) return;                        // (uniform over the workgroup)
    const float* xu = x + u.xoff;
    double z[n];
#pragma unroll
    for (int i = 0; i < n; ++i) z[i] = 0.0;
    for (int sub = 0; sub < IIR_CHUNK / IIR_STAGE; ++sub) {
        iir_stage_in(tile, xu, cbase, sub, nfull * IIR_CHUNK, lane);
        __syncthreads();
        if (c < nfull) {
            const float* row = tile + lane * IIR_TILE_LD;
            for (int t = 0; t < IIR_STAGE; ++t) (void)iir_step<S>(k, z, (double)row[t]);
        }
        __syncthreads();
    }
    if (c < nfull) {
#pragma unroll
        for (int i = 0; i < n; ++i) q[i * TC + u.coff + c] = z[i];
    }
}

__device__ __forceinline__ double iir_lane_read(double v, int j) {       // the value lane j holds (j uniform)
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// sb[i][c] = s_c[i] for every chunk of the utterance (s_0 = 0)
template <int S>
__global__ __launch_bounds__(64) void k_iir_carry(const iir_utt* __restrict__ utts, const double* __restrict__ P,
                                                  const double* __restrict__ q, double* __restrict__ sb, long TC) {
    constexpr int n = 2 * S;
    const iir_utt u = utts[blockIdx.x];
    const int lane = threadIdx.x;
    const bool own = lane < n;
    const int i = own ? lane : 0;                      // the other lanes shadow lane 0 and store nothing
    double Pr[n];
#pragma unroll
    for (int j = 0; j < n; ++j) Pr[j] = P[i * n + j];
    const long nfull = u.L / IIR_CHUNK, nch = u.nch;
    if (nch == 0) return;                              // an empty utterance owns no entry of q or sb
    const double* qi = q + i * TC + u.coff;
    double* si = sb + i * TC + u.coff;
    double s = 0.0;
    double qa[IIR_CARRY_AHEAD], qn[IIR_CARRY_AHEAD];
    // q is loaded unconditionally from an index clamped into the utterance's entries (a load under a branch is followed by its
    // own wait); an entry no full chunk wrote is read and not used
#pragma unroll
    for (int m = 0; m < IIR_CARRY_AHEAD; ++m) {
        const double v = qi[m < nch ? m : nch - 1];
        qa[m] = m < nfull ? v : 0.0;
    }
    for (long c0 = 0; c0 < nch; c0 += IIR_CARRY_AHEAD) {
#pragma unroll
        for (int m = 0; m < IIR_CARRY_AHEAD; ++m) {    // the next stretch's q, loaded beside this stretch's chain
            const long c = c0 + IIR_CARRY_AHEAD + m;
            const double v = qi[c < nch ? c : nch - 1];
            qn[m] = c < nfull ? v : 0.0;
        }
        double sv[IIR_CARRY_AHEAD];                    // the stretch's start states, stored behind its chain: memory operations
#pragma unroll                                         // complete in order, and a store between two steps would make the chain
        for (int m = 0; m < IIR_CARRY_AHEAD; ++m) {    // wait for the loads issued just above
            const long c = c0 + m;
            sv[m] = s;
            if (c < nfull) {                           // (uniform)
                double a = 0.0;
#pragma unroll
                for (int j = 0; j < n; ++j) a = a + Pr[j] * iir_lane_read(s, j);
                s = a + qa[m];
            }
        }
#pragma unroll
        for (int m = 0; m < IIR_CARRY_AHEAD; ++m) {
            if (c0 + m < nch && own) si[c0 + m] = sv[m];
            qa[m] = qn[m];
        }
    }
}

// LOUD == false: y = the filtered samples.  LOUD == true: piece[0 / 1][c], cpeak[c] (pk_iir.h), nothing else is stored.
template <int S, bool LOUD>
__global__ __launch_bounds__(IIR_LANES) void k_iir_apply(const float* __restrict__ x, const iir_utt* __restrict__ utts, iir_coef k,
                                                         const double* __restrict__ sb, long TC, float* __restrict__ y, int h,
                                                         double* __restrict__ piece, float* __restrict__ cpeak) {
    constexpr int n = 2 * S;
    __shared__ float tile[IIR_LANES * IIR_TILE_LD];
    const iir_utt u = utts[blockIdx.y];
    const int lane = threadIdx.x;
    const long L = u.L, nch = u.nch, cbase = (long)blockIdx.x * IIR_LANES, c = cbase + lane;
    if (cbase >= nch) return;                          // (uniform over the workgroup)
    const bool active = c < nch;
    const float* xu = x + u.xoff;
    const long left = L - c * IIR_CHUNK;
    const int nc = !active ? 0 : left < IIR_CHUNK ? (int)left : IIR_CHUNK;      // samples of this lane's chunk
    double z[n];
#pragma unroll
    for (int i = 0; i < n; ++i) z[i] = sb[i * TC + u.coff + (active ? c : nch - 1)];      // (unconditional loads; idle lanes store nothing)
    int tb = IIR_CHUNK;                                // samples of the chunk before hop segment g0 + 1
    double acc0 = 0.0, acc1 = 0.0;
    float pk = 0.f;
    if (LOUD && active) {
        const long g0 = c * IIR_CHUNK / h, edge = (g0 + 1) * h - c * IIR_CHUNK;
        tb = edge < IIR_CHUNK ? (int)edge : IIR_CHUNK;
    }
    for (int sub = 0; sub < IIR_CHUNK / IIR_STAGE; ++sub) {
        iir_stage_in(tile, xu, cbase, sub, L, lane);
        __syncthreads();
        float* row = tile + lane * IIR_TILE_LD;
        for (int t = 0; t < IIR_STAGE; ++t) {
            const int tt = sub * IIR_STAGE + t;
            if (tt < nc) {
                const float xv = row[t];
                const double o = iir_step<S>(k, z, (double)xv);
                if (LOUD) {
                    const double zz = o * o;
                    if (tt < tb) acc0 = acc0 + zz;
                    else acc1 = acc1 + zz;
                    pk = fmaxf(pk, fabsf(xv));
                } else {
                    row[t] = (float)o;
                }
            }
        }
        __syncthreads();
        if (!LOUD) {
#pragma unroll 8
            for (int r = 0; r < IIR_LANES; ++r) {
                const long idx = (cbase + r) * IIR_CHUNK + sub * IIR_STAGE + lane;
                if (idx < L) y[u.xoff + idx] = tile[r * IIR_TILE_LD + lane];
            }
            __syncthreads();
        }
    }
    if (LOUD && active) {
        piece[u.coff + c] = acc0;
        piece[TC + u.coff + c] = acc1;
        cpeak[u.coff + c] = pk;
    }
}

__global__ __launch_bounds__(LOUD_THREADS) void k_loud_segments(const double* __restrict__ piece, const iir_utt* __restrict__ utts,
                                                                long TC, int h, double* __restrict__ seg) {
    const iir_utt u = utts[blockIdx.y];
    const long g = (long)blockIdx.x * LOUD_THREADS + threadIdx.x;
    if (g >= u.G) return;
    const long c_lo = g * h / IIR_CHUNK, c_hi = ((g + 1) * h - 1) / IIR_CHUNK;   // (g + 1) h <= L: c_hi < nch
    double acc = 0.0;
    for (long c = c_lo; c <= c_hi; ++c) {
        const long g0 = c * IIR_CHUNK / h;             // g or g - 1
        acc = acc + piece[(g0 == g ? 0 : TC) + u.coff + c];
    }
    seg[u.goff + g] = acc;
}

// THE ORDER over blocks: a[] holds every item's partial sum; returns a_0 to every item
__device__ __forceinline__ double loud_tree(double* a, int t, double v) {
    __syncthreads();                                   // the previous use of a[] has been read
    a[t] = v;
    __syncthreads();
    for (int hh = LOUD_THREADS / 2; hh >= 1; hh >>= 1) {
        if (t < hh) a[t] = a[t] + a[t + hh];
        __syncthreads();
    }
    return a[0];
}

__device__ __forceinline__ int loud_count(int* a, int t, int v) {
    __syncthreads();
    a[t] = v;
    __syncthreads();
    for (int hh = LOUD_THREADS / 2; hh >= 1; hh >>= 1) {
        if (t < hh) a[t] = a[t] + a[t + hh];
        __syncthreads();
    }
    return a[0];
}

__global__ __launch_bounds__(LOUD_THREADS) void k_loud_gate(const double* __restrict__ seg, const float* __restrict__ cpeak,
                                                            const iir_utt* __restrict__ utts, int h, double* __restrict__ mean_out,
                                                            double* __restrict__ rel_out, float* __restrict__ peak_out,
                                                            int* __restrict__ counts_out) {
    __shared__ double a[LOUD_THREADS];
    __shared__ int cn[LOUD_THREADS];
    __shared__ float pm[LOUD_THREADS];
    const iir_utt u = utts[blockIdx.x];
    const int t = threadIdx.x;
    const long J = u.G > 3 ? u.G - 3 : 0;
    const double den = (double)(4 * h);
    const double* sg = seg + u.goff;
    double acc = 0.0;
    int cnt = 0;
    for (long j = t; j < J; j += LOUD_THREADS) {
        const double p = (((sg[j] + sg[j + 1]) + sg[j + 2]) + sg[j + 3]) / den;
        if (p > LOUD_ABS) {
            acc = acc + p;
            ++cnt;
        }
    }
    const double sum1 = loud_tree(a, t, acc);
    const int n1 = loud_count(cn, t, cnt);
    const double rel = n1 > 0 ? 0.1 * (sum1 / (double)n1) : 0.0;
    acc = 0.0;
    cnt = 0;
    for (long j = t; j < J; j += LOUD_THREADS) {
        const double p = (((sg[j] + sg[j + 1]) + sg[j + 2]) + sg[j + 3]) / den;
        if (p > LOUD_ABS && p > rel) {
            acc = acc + p;
            ++cnt;
        }
    }
    const double sum2 = loud_tree(a, t, acc);
    const int n2 = loud_count(cn, t, cnt);
    float pk = 0.f;
    for (long c = t; c < u.nch; c += LOUD_THREADS) pk = fmaxf(pk, cpeak[u.coff + c]);
    pm[t] = pk;
    __syncthreads();
    for (int hh = LOUD_THREADS / 2; hh >= 1; hh >>= 1) {
        if (t < hh) pm[t] = fmaxf(pm[t], pm[t + hh]);
        __syncthreads();
    }
    if (t == 0) {
        mean_out[blockIdx.x] = n2 > 0 ? sum2 / (double)n2 : 0.0;
        rel_out[blockIdx.x] = rel;
        peak_out[blockIdx.x] = pm[0];
        counts_out[3 * blockIdx.x + 0] = n2;
        counts_out[3 * blockIdx.x + 1] = n1;
        counts_out[3 * blockIdx.x + 2] = (int)J;
    }
}

constexpr int IIR_GAIN_THREADS = 256;

__global__ __launch_bounds__(IIR_GAIN_THREADS) void k_gain(const float* __restrict__ x, const iir_utt* __restrict__ utts,
                                                           float* __restrict__ y) {
    const iir_utt u = utts[blockIdx.y];
    const long i = (long)blockIdx.x * IIR_GAIN_THREADS + threadIdx.x;
    if (i < u.L) y[u.xoff + i] = x[u.xoff + i] * u.gain;
}

// ------------------------------------------------------------------------------------------------ host side
size_t iir_align(size_t b) { return (b + 255) / 256 * 256; }

struct iir_plan {
    std::vector<iir_utt> tab;
    long TC = 0, TG = 0, maxL = 0, maxfull = 0, maxch = 0, maxG = 0;
};

// h: samples of a hop segment (0: no loudness); gains: NULL or (B)
int iir_table(const char* who, const int32_t* lens, int B, int h, const float* gains, iir_plan& p) {
    if (B <= 0) PK_FAIL(PK_EINVAL, "%s: batch size must be positive", who);
    if (B > IIR_MAX_BATCH) PK_FAIL(PK_EUNSUPPORTED, "%s: %d utterances; the engine's envelope is %d in a call", who, B, IIR_MAX_BATCH);
    p.tab.resize(B);
    long xoff = 0;
    for (int b = 0; b < B; ++b) {
        const long L = lens[b];
        if (L < 0) PK_FAIL(PK_EINVAL, "%s: utterance %d has a negative length (%ld)", who, b, L);
        if (L > IIR_MAX_SAMPLES)
            PK_FAIL(PK_EUNSUPPORTED, "%s: utterance %d has %ld samples; the engine's envelope is %ld", who, b, L, IIR_MAX_SAMPLES);
        const long nch = iir_chunks(L), nfull = iir_full_chunks(L), G = h > 0 ? L / h : 0;
        p.tab[b] = {xoff, p.TC, p.TG, (int)L, (int)nch, (int)G, gains ? gains[b] : 1.f};
        xoff += L;
        p.TC += nch;
        p.TG += G;
        p.maxL = L > p.maxL ? L : p.maxL;
        p.maxfull = nfull > p.maxfull ? nfull : p.maxfull;
        p.maxch = nch > p.maxch ? nch : p.maxch;
        p.maxG = G > p.maxG ? G : p.maxG;
    }
    return PK_OK;
}

struct iir_ws {
    double* q;       // (2 S, TC)
    double* sb;      // (2 S, TC)
    double* piece;   // (2, TC)
    float* cpeak;    // (TC)
    double* seg;     // (TG)
};

int iir_reserve(pk_ctx_scratch* sc, const iir_plan& p, int n, bool loud, iir_ws& w) {
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += iir_align(bytes ? bytes : 1);
        return at;
    };
    const size_t o_q = take((size_t)n * p.TC * 8), o_s = take((size_t)n * p.TC * 8), o_p = take(loud ? (size_t)2 * p.TC * 8 : 0),
                 o_k = take(loud ? (size_t)p.TC * 4 : 0), o_g = take(loud ? (size_t)p.TG * 8 : 0);
    PK_TRY(sc->iir_ws.reserve(o));
    unsigned char* base = sc->iir_ws.as<unsigned char>();
    w.q = reinterpret_cast<double*>(base + o_q);
    w.sb = reinterpret_cast<double*>(base + o_s);
    w.piece = reinterpret_cast<double*>(base + o_p);
    w.cpeak = reinterpret_cast<float*>(base + o_k);
    w.seg = reinterpret_cast<double*>(base + o_g);
    return PK_OK;
}

iir_coef iir_coefs(const pk_iir* h) {
    iir_coef k;
    for (int s = 0; s < IIR_MAX_SECTIONS; ++s) {
        const bool in = s < h->S;
        k.b0[s] = in ? h->sos[s][0] : 0.0;
        k.b1[s] = in ? h->sos[s][1] : 0.0;
        k.b2[s] = in ? h->sos[s][2] : 0.0;
        k.a1[s] = in ? h->sos[s][4] : 0.0;
        k.a2[s] = in ? h->sos[s][5] : 0.0;
    }
    return k;
}

unsigned iir_blocks(long items, long per) { return (unsigned)((items + per - 1) / per); }

#define IIR_FOR_S(S_, CALL)          \
    switch (S_) {                    \
        case 1: { constexpr int S = 1; CALL; } break; \
        case 2: { constexpr int S = 2; CALL; } break; \
        case 3: { constexpr int S = 3; CALL; } break; \
        case 4: { constexpr int S = 4; CALL; } break; \
        case 5: { constexpr int S = 5; CALL; } break; \
        case 6: { constexpr int S = 6; CALL; } break; \
        case 7: { constexpr int S = 7; CALL; } break; \
        default: { constexpr int S = 8; CALL; } break; \
    }

template <int S>
int iir_launch_transition(pk_iir* h, const iir_coef& k) {
    PK_LAUNCH(h->ctx, "iir_transition", k_iir_transition<S>, dim3(1), dim3(64), 0, k, h->P.as<double>());
    return PK_OK;
}

// the three passes; y != NULL: filter mode, else loudness mode (pieces and peaks into the workspace)
template <int S>
int iir_launch_passes(pk_iir* h, const float* x, const iir_utt* dtab, const iir_plan& p, int B, const iir_ws& w, float* y, int hop) {
    pk_ctx* ctx = h->ctx;
    const iir_coef k = iir_coefs(h);
    if (p.maxch == 0) return PK_OK;                    // nothing but empty utterances
    if (p.maxfull > 0)
        PK_LAUNCH(ctx, "iir_local", k_iir_local<S>, dim3(iir_blocks(p.maxfull, IIR_LANES), B), dim3(IIR_LANES), 0, x, dtab, k, w.q, p.TC);
    PK_LAUNCH(ctx, "iir_carry", k_iir_carry<S>, dim3(B), dim3(64), 0, dtab, (const double*)h->P.as<double>(), (const double*)w.q,
              w.sb, p.TC);
    if (y)
        PK_LAUNCH(ctx, "iir_apply", (k_iir_apply<S, false>), dim3(iir_blocks(p.maxch, IIR_LANES), B), dim3(IIR_LANES), 0, x, dtab, k,
                  (const double*)w.sb, p.TC, y, 0, (double*)nullptr, (float*)nullptr);
    else
        PK_LAUNCH(ctx, "iir_apply_loud", (k_iir_apply<S, true>), dim3(iir_blocks(p.maxch, IIR_LANES), B), dim3(IIR_LANES), 0, x, dtab,
                  k, (const double*)w.sb, p.TC, (float*)nullptr, hop, w.piece, w.cpeak);
    return PK_OK;
}

}  // namespace

extern "C" int pk_iir_create(pk_ctx* ctx, const double* sos, int32_t n_sections, pk_iir** out) {
    if (!ctx || !sos || !out) PK_FAIL(PK_EINVAL, "pk_iir_create: NULL argument");
    if (n_sections < 1) PK_FAIL(PK_EINVAL, "pk_iir_create: %d sections; a filter has at least one", (int)n_sections);
    if (n_sections > IIR_MAX_SECTIONS)
        PK_FAIL(PK_EUNSUPPORTED, "pk_iir_create: %d sections; the engine's envelope is 1 ... %d", (int)n_sections, IIR_MAX_SECTIONS);
    for (int s = 0; s < n_sections; ++s) {
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(sos[6 * s + i])) PK_FAIL(PK_EINVAL, "pk_iir_create: section %d has a coefficient that is not finite", s);
        if (sos[6 * s + 3] != 1.0)
            PK_FAIL(PK_EINVAL, "pk_iir_create: section %d has a0 = %g; sections are normalised to a0 = 1", s, sos[6 * s + 3]);
    }
    PK_DEVICE(ctx->device);
    pk_iir* h = new pk_iir();
    h->ctx = ctx;
    h->S = n_sections;
    for (int s = 0; s < n_sections; ++s)
        for (int i = 0; i < 6; ++i) h->sos[s][i] = sos[6 * s + i];
    const int n = 2 * n_sections;
    int st = h->P.reserve((size_t)n * n * sizeof(double));
    if (st == PK_OK) {
        const iir_coef k = iir_coefs(h);
        IIR_FOR_S(h->S, st = iir_launch_transition<S>(h, k));
    }
    if (st == PK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        pk_set_error("pk_iir_create: the transition kernel failed");
        st = PK_EHIP;
    }
    if (st != PK_OK) {
        h->P.release();
        delete h;
        return st;
    }
    *out = h;
    return PK_OK;
}

extern "C" void pk_iir_destroy(pk_iir* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->P.release();
    delete h;
}

extern "C" int pk_iir_transition(pk_iir* h, double* P_out) {
    if (!h || !P_out) PK_FAIL(PK_EINVAL, "pk_iir_transition: NULL argument");
    PK_DEVICE(h->ctx->device);
    const int n = 2 * h->S;
    PK_HIP(hipMemcpyAsync(P_out, h->P.p, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    PK_HIP(hipStreamSynchronize(h->ctx->stream));
    return PK_OK;
}

extern "C" int pk_iir_run(pk_iir* h, const float* x, const int32_t* lens, int32_t B, float* y) {
    if (!h || !x || !lens || !y) PK_FAIL(PK_EINVAL, "pk_iir_run: NULL argument");
    iir_plan p;
    PK_TRY(iir_table("pk_iir_run", lens, B, 0, nullptr, p));
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    iir_ws w;
    PK_TRY(iir_reserve(sc, p, 2 * h->S, false, w));
    PK_TRY(pk_upload(ctx, sc->iir_tab, p.tab.data(), p.tab.size() * sizeof(iir_utt)));
    const iir_utt* dtab = sc->iir_tab.as<iir_utt>();
    int st = PK_OK;
    IIR_FOR_S(h->S, st = iir_launch_passes<S>(h, x, dtab, p, B, w, y, 0));
    return st;
}

extern "C" int pk_loudness_run(pk_iir* h, const float* x, const int32_t* lens, int32_t B, int32_t sr, double* mean_out,
                               double* rel_out, float* peak_out, int32_t* counts_out) {
    if (!h || !x || !lens || !mean_out || !rel_out || !peak_out || !counts_out) PK_FAIL(PK_EINVAL, "pk_loudness_run: NULL argument");
    if (sr < LOUD_SR_MIN || sr > LOUD_SR_MAX || sr % 10 != 0)
        PK_FAIL(PK_EUNSUPPORTED, "pk_loudness_run: sr = %d; blocks lie on a 100 ms sample grid, which takes a multiple of 10 in %d ... %d "
                "(resample first)", (int)sr, LOUD_SR_MIN, LOUD_SR_MAX);
    const int hop = sr / 10;
    iir_plan p;
    PK_TRY(iir_table("pk_loudness_run", lens, B, hop, nullptr, p));
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    iir_ws w;
    PK_TRY(iir_reserve(sc, p, 2 * h->S, true, w));
    PK_TRY(pk_upload(ctx, sc->iir_tab, p.tab.data(), p.tab.size() * sizeof(iir_utt)));
    const iir_utt* dtab = sc->iir_tab.as<iir_utt>();
    int st = PK_OK;
    IIR_FOR_S(h->S, st = iir_launch_passes<S>(h, x, dtab, p, B, w, nullptr, hop));
    PK_TRY(st);
    if (p.maxG > 0)
        PK_LAUNCH(ctx, "loud_segments", k_loud_segments, dim3(iir_blocks(p.maxG, LOUD_THREADS), B), dim3(LOUD_THREADS), 0,
                  (const double*)w.piece, dtab, p.TC, hop, w.seg);
    PK_LAUNCH(ctx, "loud_gate", k_loud_gate, dim3(B), dim3(LOUD_THREADS), 0, (const double*)w.seg, (const float*)w.cpeak, dtab, hop,
              mean_out, rel_out, peak_out, counts_out);
    return PK_OK;
}

extern "C" int pk_gain_run(pk_ctx* ctx, const float* x, const int32_t* lens, int32_t B, const float* gains, float* y) {
    if (!ctx || !x || !lens || !gains || !y) PK_FAIL(PK_EINVAL, "pk_gain_run: NULL argument");
    iir_plan p;
    PK_TRY(iir_table("pk_gain_run", lens, B, 0, gains, p));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    PK_TRY(pk_upload(ctx, sc->iir_tab, p.tab.data(), p.tab.size() * sizeof(iir_utt)));
    if (p.maxL > 0)
        PK_LAUNCH(ctx, "gain", k_gain, dim3(iir_blocks(p.maxL, IIR_GAIN_THREADS), B), dim3(IIR_GAIN_THREADS), 0, x,
                  (const iir_utt*)sc->iir_tab.as<iir_utt>(), y);
    return PK_OK;
}
