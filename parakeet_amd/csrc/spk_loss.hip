// spk_loss.hip -- the GE2E similarity matrix and softmax loss (parakeet/models/lstm_speaker_encoder.py similarity_matrix
// :55-104, loss :122-134), forward only.
//
// embeds (N speakers, M utterances each, C dimensions), not assumed unit-norm.  Three launches:
//   k_ge2e_centroids  one workgroup per speaker: S[n] = sum_m e[n, m] (m ascending), the inclusive centroid S / M, its norm,
//                     and the normalised centroid written TRANSPOSED, cT[c][n], so that a lane per speaker reads it coalesced.
//   k_ge2e_rows<R>    one workgroup per R utterances (rows of the matrix), their embeddings in LDS.
//                     Exclusive centroid: one wave per row, x = (S[n] - e) / (M - 1), its norm, p2 = sum_c e_c (x_c / |x|);
//                     lanes stride over c, an xor butterfly joins them.
//                     p1: lane j owns speaker j (then j + 256, ...): C sequential fmas in four chains by c mod 4, joined as
//                     (a0 + a1) + (a2 + a3); the centroid column is loaded once for the R rows.
//                     p = (own speaker ? p2 : p1) * w + b; the row's log-sum-exp runs online in float64 (running maximum,
//                     rescaled sum) per lane, the lanes are joined under the row's exact maximum by a butterfly and a fixed
//                     tree over the four waves; row term = max + log(sum) - p[own speaker].
//   k_ge2e_fold       one workgroup: thread t adds rows t, t + 256, ... in float64, a tree over the threads, / (N M).
// Every summation order is a function of (M, C) alone -- of N M for the fold -- and no atomics are used: a row's p, p1, p2
// depend on that utterance and the centroids only, so permuting the speakers of a batch permutes them bit for bit.  (The
// row TERM sums over speakers in lane order and is reproducible, not permutation-invariant.)
// A speaker whose centroid (or an utterance whose exclusive centroid) has zero norm gives NaN, as in the reference.
#include <algorithm>
#include <cmath>

#include "pk_spk_loss.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// S [N][Cp], cT [Cp][N]; columns C .. Cp - 1 are zero in both
__global__ __launch_bounds__(256) void k_ge2e_centroids(const float* __restrict__ e, int N, int M, int C, int Cp,
                                                        float* __restrict__ S, float* __restrict__ cT) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* base = e + (long)n * M * C;
    float* Sn = S + (long)n * Cp;
    const float fm = (float)M;
    float ss = 0.f;
    for (int c = tid; c < Cp; c += 256) {
        float s = 0.f;
        if (c < C)
            for (int m = 0; m < M; ++m) s += base[(long)m * C + c];
        Sn[c] = s;
        const float ci = s / fm;
        ss = fmaf(ci, ci, ss);
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float nrm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    for (int c = tid; c < Cp; c += 256) cT[(long)c * N + n] = c < C ? (Sn[c] / fm) / nrm : 0.f;   // Sn[c]: this thread's own store
}

template <int R>
__global__ __launch_bounds__(256) void k_ge2e_rows(const float* __restrict__ e, const float* __restrict__ S,
                                                   const float* __restrict__ cT, int N, int M, int C, int Cp, float w, float b,
                                                   float* __restrict__ sim, float* __restrict__ p1, float* __restrict__ p2,
                                                   double* __restrict__ nll) {
    extern __shared__ float es[];   // [R][Cp]
    __shared__ float p2s[R];
    __shared__ float mred[4][R];
    __shared__ double sred[4][R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long NM = (long)N * M, r0 = (long)blockIdx.x * R;

    for (int i = tid; i < R * Cp; i += 256) {
        const int r = i / Cp, c = i - r * Cp;
        const long row = r0 + r;
        es[i] = (row < NM && c < C) ? e[row * C + c] : 0.f;
    }
    __syncthreads();

    // ---- exclusive centroid and p2: one wave per row
    const float fm1 = (float)(M - 1);
    for (int r = wave; r < R; r += 4) {
        const long row = r0 + r;
        if (row >= NM) break;   // wave-uniform
        const float* Sn = S + (row / M) * Cp;
        const float* er = es + r * Cp;
        float ss = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float x = (Sn[c] - er[c]) / fm1;
            ss = fmaf(x, x, ss);
        }
        const float nrm = sqrtf(wave_sum(ss));
        float d = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float x = (Sn[c] - er[c]) / fm1;
            d = fmaf(er[c], x / nrm, d);
        }
        d = wave_sum(d);
        if (lane == 0) {
            p2s[r] = d;
            if (p2) p2[row] = d;
        }
    }
    __syncthreads();

    // ---- p1, p and the online log-sum-exp: one lane per speaker
    float lm[R];
    double ls[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        lm[r] = -INFINITY;
        ls[r] = 0.0;
    }
    for (int j = tid; j < N; j += 256) {
        float a[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r][0] = a[r][1] = a[r][2] = a[r][3] = 0.f;
        const float* cj = cT + j;
        for (int c = 0; c < Cp; c += 4) {
            const float c0 = cj[(long)c * N], c1 = cj[(long)(c + 1) * N], c2 = cj[(long)(c + 2) * N], c3 = cj[(long)(c + 3) * N];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 ev = *reinterpret_cast<const float4*>(es + r * Cp + c);
                a[r][0] = fmaf(ev.x, c0, a[r][0]);
                a[r][1] = fmaf(ev.y, c1, a[r][1]);
                a[r][2] = fmaf(ev.z, c2, a[r][2]);
                a[r][3] = fmaf(ev.w, c3, a[r][3]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long row = r0 + r;
            if (row < NM) {
                const float d = (a[r][0] + a[r][1]) + (a[r][2] + a[r][3]);
                if (p1) p1[row * N + j] = d;
                const float s = j == (int)(row / M) ? p2s[r] : d;
                const float v = fmaf(s, w, b);
                if (sim) sim[row * N + j] = v;
                if (v > lm[r]) {
                    ls[r] = ls[r] * exp((double)lm[r] - (double)v) + 1.0;
                    lm[r] = v;
                } else {
                    ls[r] += exp((double)v - (double)lm[r]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float m = lm[r];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) mred[wave][r] = m;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float mx = fmaxf(fmaxf(mred[0][r], mred[1][r]), fmaxf(mred[2][r], mred[3][r]));
        double s = ls[r] == 0.0 ? 0.0 : ls[r] * exp((double)lm[r] - (double)mx);   // a lane without a speaker adds nothing
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) sred[wave][r] = s;
    }
    __syncthreads();
    if (tid < R && r0 + tid < NM) {
        const int r = tid;
        const float mx = fmaxf(fmaxf(mred[0][r], mred[1][r]), fmaxf(mred[2][r], mred[3][r]));
        const double tot = (sred[0][r] + sred[1][r]) + (sred[2][r] + sred[3][r]);
        const float own = fmaf(p2s[r], w, b);   // the same operation as the matrix entry: the same bits
        nll[r0 + r] = (double)mx + log(tot) - (double)own;
    }
}

__global__ __launch_bounds__(256) void k_ge2e_fold(const double* __restrict__ nll, long NM, double* __restrict__ loss) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double a = 0.0;
    for (long i = t; i < NM; i += 256) a += nll[i];
    sh[t] = a;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) loss[0] = sh[0] / (double)NM;
}

// cosine similarity of U pairs of C-vectors, one wave per pair: a . b / (max(|a|, eps) max(|b|, eps)), eps = 1e-12 as F.normalize
__global__ __launch_bounds__(64) void k_spk_cosine(const float* __restrict__ a, const float* __restrict__ b, int C,
                                                   float* __restrict__ out) {
    const long u = blockIdx.x;
    const int lane = threadIdx.x;
    const float *pa = a + u * C, *pb = b + u * C;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float x = pa[c], y = pb[c];
        ab = fmaf(x, y, ab);
        aa = fmaf(x, x, aa);
        bb = fmaf(y, y, bb);
    }
    ab = wave_sum(ab);
    aa = wave_sum(aa);
    bb = wave_sum(bb);
    if (lane == 0) out[u] = ab / (fmaxf(sqrtf(aa), 1e-12f) * fmaxf(sqrtf(bb), 1e-12f));
}

}  // namespace

int pk_spk_cosine_run(pk_ctx* ctx, const float* a, const float* b, int U, int C, float* out) {
    if (!ctx || !a || !b || !out) PK_FAIL(PK_EINVAL, "pk_spk_cosine: NULL argument");
    if (U < 1 || C < 1) PK_FAIL(PK_ESHAPE, "pk_spk_cosine: %d pairs of %d dimensions", U, C);
    PK_DEVICE(ctx->device);
    PK_LAUNCH(ctx, "spk_cosine", k_spk_cosine, dim3(U), dim3(64), 0, a, b, C, out);
    return PK_OK;
}

int pk_spk_loss_run(pk_ctx* ctx, pk_dbuf& ws, float w, float b, const float* embeds, int N, int M, int C, float* sim, float* p1,
                    float* p2, double* row_nll, double* loss) {
    if (!ctx || !embeds) PK_FAIL(PK_EINVAL, "pk_spk_ge2e: NULL argument");
    if (N < 2 || M < 2 || C < 1)
        PK_FAIL(PK_ESHAPE, "pk_spk_ge2e: embeds (%d, %d, %d): the GE2E loss takes at least 2 speakers of at least 2 utterances "
                           "(the exclusive centroid divides by M - 1) and 1 dimension", N, M, C);
    const long NM = (long)N * M;
    if (N > PK_GE2E_MAX_N || C > PK_GE2E_MAX_C || NM > PK_GE2E_MAX_ROWS || NM * N > PK_GE2E_MAX_SCORES)
        PK_FAIL(PK_EUNSUPPORTED, "pk_spk_ge2e: embeds (%d, %d, %d) exceed the envelope: N <= %d, C <= %d, N M <= %ld, N M N <= %ld",
                N, M, C, PK_GE2E_MAX_N, PK_GE2E_MAX_C, PK_GE2E_MAX_ROWS, PK_GE2E_MAX_SCORES);
    PK_DEVICE(ctx->device);
    const int Cp = (C + 3) / 4 * 4;
    // workspace: [row terms NM doubles][S N * Cp][cT Cp * N]
    const size_t nll_bytes = ((size_t)NM * sizeof(double) + 15) & ~(size_t)15, mat = (size_t)N * Cp * sizeof(float);
    PK_TRY(ws.reserve(nll_bytes + 2 * mat));
    double* nll = row_nll ? row_nll : ws.as<double>();
    float* S = reinterpret_cast<float*>(ws.as<char>() + nll_bytes);
    float* cT = S + (size_t)N * Cp;
    PK_LAUNCH(ctx, "ge2e_centroids", k_ge2e_centroids, dim3(N), dim3(256), 0, embeds, N, M, C, Cp, S, cT);
    if (Cp <= PK_GE2E_WIDE_MAX_C) {
        constexpr int R = PK_GE2E_ROWS_WIDE;
        PK_LAUNCH(ctx, "ge2e_rows", k_ge2e_rows<R>, dim3(pk_div_up(NM, R)), dim3(256), (size_t)R * Cp * sizeof(float), embeds, S,
                  cT, N, M, C, Cp, w, b, sim, p1, p2, nll);
    } else {
        constexpr int R = PK_GE2E_ROWS_NARROW;
        PK_LAUNCH(ctx, "ge2e_rows", k_ge2e_rows<R>, dim3(pk_div_up(NM, R)), dim3(256), (size_t)R * Cp * sizeof(float), embeds, S,
                  cT, N, M, C, Cp, w, b, sim, p1, p2, nll);
    }
    if (loss) PK_LAUNCH(ctx, "ge2e_fold", k_ge2e_fold, dim3(1), dim3(256), 0, nll, NM, loss);
    return PK_OK;
}
