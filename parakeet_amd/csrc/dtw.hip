// dtw.hip -- dynamic time warping of ragged batches and the statistics along its path on gfx950: what the
// scores of free-running synthesis (mel-cepstral distortion, log-F0 RMSE: parakeet_amd/metrics.py) are taken along.  The
// definition, the decision words' layout, the order of the sums and the envelope: pk_dtw.h.  The definition is this project's
// own (unconstrained, squared Euclidean local cost); it is not any other toolkit's.
//
// k_dtw_cost:       feature mode's float32 cost matrix, a DTW_TILE x DTW_TILE tile per workgroup, the x and y tiles in LDS.
// k_dtw<R>:         one wave per pair, R rows per lane, lanes skewed by one column, the neighbour's bottom value by a DPP wave
//                   shift, one 32-bit decision word per lane and column (LDS or a global workspace), then the backtrack by
//                   every lane alike over decision words read from LDS.
// k_dtw_path_stats: one workgroup per pair, float64 sums in the fixed order of pk_dtw.h.
#pragma clang fp contract(off)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_dtw.h"

namespace {

typedef unsigned int u32;

struct dtw_pair {
    long off;         // first cost of the pair (floats) in the matrix the search reads
    long row_stride;  // floats between its rows
    long path_off;    // first path entry (sum of N + M - 1 before it)
    long bits_off;    // first decision word in the global workspace; -1: LDS
    long carry_off;   // first double of the pair's two carry rows (pairs of several passes)
    long rev_off;     // first word of the pair's reversed path
    int N, M;
    int b, pad_;      // the pair's number in the call
};

struct dtw_feat {     // a pair's feature streams (k_dtw_cost, k_dtw_path_stats)
    long xoff, yoff;  // first float of x, of y
    long xs, ys;      // floats between rows
    long coff;        // k_dtw_cost: first float of the pair's cost matrix in the output
    long path_off;    // k_dtw_path_stats: first path entry, first mask bytes
    long mx_off, my_off;
    int N, M;
    int b, pad_;
};

constexpr double POS_INF = __builtin_huge_val();

// lane l receives lane l - 1's x; lane 0 receives fill (DPP wave_shr:1, two 32-bit moves)
__device__ __forceinline__ double dtw_from_left(double x, double fill) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// s of pk_dtw.h for one cell: K columns from xr and yr
__device__ __forceinline__ double dtw_sq_dist(const float* __restrict__ xr, const float* __restrict__ yr, int K) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        const double d = (double)xr[k] - (double)yr[k];
        const double dd = d * d;
        s = s + dd;
    }
    return s;
}

__global__ __launch_bounds__(DTW_COST_THREADS) void k_dtw_cost(const float* __restrict__ x, const float* __restrict__ y,
                                                               const dtw_feat* __restrict__ pairs, int k0, int K,
                                                               float* __restrict__ out) {
    constexpr int LD = DTW_TILE + 1;
    __shared__ float xt[DTW_MAX_DIM * LD];             // [k][row of the tile]
    __shared__ float yt[DTW_MAX_DIM * LD];
    const dtw_feat u = pairs[blockIdx.z];
    const int i0 = blockIdx.y * DTW_TILE, j0 = blockIdx.x * DTW_TILE, tid = threadIdx.x;
    if (i0 >= u.N || j0 >= u.M) return;                // (uniform: the grid is sized for the launch's largest pair)
    for (int e = tid; e < DTW_TILE * K; e += DTW_COST_THREADS) {
        const int r = e / K, k = e - r * K;
        xt[k * LD + r] = i0 + r < u.N ? x[u.xoff + (long)(i0 + r) * u.xs + k0 + k] : 0.f;
        yt[k * LD + r] = j0 + r < u.M ? y[u.yoff + (long)(j0 + r) * u.ys + k0 + k] : 0.f;
    }
    __syncthreads();
    constexpr int ROWS = DTW_TILE * DTW_TILE / DTW_COST_THREADS, STEP = DTW_COST_THREADS / DTW_TILE;
    const int tj = tid % DTW_TILE, ti = tid / DTW_TILE;
    double s[ROWS];
#pragma unroll
    for (int c = 0; c < ROWS; ++c) s[c] = 0.0;
    for (int k = 0; k < K; ++k) {
        const double yv = (double)yt[k * LD + tj];
#pragma unroll
        for (int c = 0; c < ROWS; ++c) {
            const double d = (double)xt[k * LD + ti + c * STEP] - yv;
            const double dd = d * d;
            s[c] = s[c] + dd;
        }
    }
#pragma unroll
    for (int c = 0; c < ROWS; ++c) {
        const int i = i0 + ti + c * STEP, j = j0 + tj;
        if (i < u.N && j < u.M) out[u.coff + (long)i * u.M + j] = (float)s[c];
    }
}

template <int R>
__global__ __launch_bounds__(64) void k_dtw(const float* __restrict__ cost, const dtw_pair* __restrict__ pairs,
                                            int* __restrict__ ix, int* __restrict__ iy, int* __restrict__ plen,
                                            double* __restrict__ cost_out, int* __restrict__ status, u32* __restrict__ gbits,
                                            double* __restrict__ gcarry, u32* __restrict__ grev) {
    constexpr int A = DTW_AHEAD(R);
    constexpr int RS = R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : 4;
    static_assert((1 << RS) == R && R <= DTW_MAX_STRIP, "a strip is 1, 2, 4, 8 or 16 rows");
    extern __shared__ u32 lbits[];                     // the decision words (LDS store) or the stage of a global store
    const dtw_pair u = pairs[blockIdx.x];
    const int N = u.N, M = u.M, lane = threadIdx.x;
    const int G = (N + R - 1) / R;                     // strips
    const bool global_store = u.bits_off >= 0;         // (uniform)
    u32* bits = global_store ? gbits + u.bits_off : lbits;
    const int npass = (G + 63) / 64;
    const int g_last = (N - 1) >> RS, r_last = (N - 1) & (R - 1);
    int bad = 0;
    double score = 0.0;

    for (int pass = 0; pass < npass; ++pass) {
        const int g = pass * 64 + lane, i0 = g * R;    // the lane's strip and its first row
        const bool strip = g < G;
        const int lanes = G - pass * 64 < 64 ? G - pass * 64 : 64;
        const int steps = M + lanes - 1;
        const float* src = cost + u.off + (long)i0 * u.row_stride;
        const double* cin = pass > 0 ? gcarry + u.carry_off + (long)((pass - 1) & 1) * M : nullptr;
        double* cout = pass + 1 < npass ? gcarry + u.carry_off + (long)(pass & 1) * M : nullptr;
        const bool takes_carry = lane == 0 && pass > 0;

        double q[R];                                   // Q(i0 + r, j - 1)
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] = POS_INF;
        double bot = POS_INF;                          // Q(i0 + R - 1, j - 1): what lane + 1 takes next step
        double diag_in = pass == 0 && lane == 0 ? -0.0 : POS_INF;   // Q(i0 - 1, j - 1); c + -0.0 = c makes Q(0, 0) = c(0, 0)
        float cur[A][R], nxt[A][R];
        double ccur[A], cnxt[A];                       // lane 0: the row above the pass
        auto load = [&](float(&dst)[A][R], double(&cd)[A], int t0) {
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const int j = t0 + a - lane;
                const bool in = j >= 0 && j < M;
#pragma unroll
                for (int r = 0; r < R; ++r) dst[a][r] = (in && i0 + r < N) ? src[(long)r * u.row_stride + j] : 0.f;
                cd[a] = (in && takes_carry) ? cin[j] : POS_INF;
            }
        };
        load(cur, ccur, 0);
        for (int t0 = 0; t0 < steps; t0 += A) {
            load(nxt, cnxt, t0 + A);                   // (nothing outside the N x M matrix is read)
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const int j = t0 + a - lane;
                const bool in = strip && j >= 0 && j < M;
                double up_in = dtw_from_left(bot, POS_INF);
                up_in = lane == 0 ? ccur[a] : up_in;
                double nq[R];
                u32 w = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double d = r == 0 ? diag_in : q[r > 0 ? r - 1 : 0];
                    const double up = r == 0 ? up_in : nq[r > 0 ? r - 1 : 0];
                    const double lf = q[r];
                    const float c = cur[a][r];
                    if (in && i0 + r < N && !(fabsf(c) <= 3.402823466e+38f)) bad = 1;
                    // the smallest of d, up, lf; ties to d, then up.  min(d, lf) does not wait for the cell above
                    const bool lf_d = lf < d;
                    const double pre = lf_d ? lf : d;
                    const bool take_up = lf_d ? up <= pre : up < pre;
                    const double m = take_up ? up : pre;
                    const u32 dec = take_up ? 1u : (lf_d ? 2u : 0u);
                    nq[r] = (double)c + m;
                    w |= dec << (2 * r);
                }
                if (in) {
#pragma unroll
                    for (int r = 0; r < R; ++r) q[r] = nq[r];
                    bot = nq[R - 1];
                    bits[(long)j * G + g] = w;
                    if (cout && lane == 63) cout[j] = bot;
                    if (j == M - 1 && g == g_last) {
                        double sc = nq[0];
#pragma unroll
                        for (int r = 1; r < R; ++r) sc = r == r_last ? nq[r] : sc;
                        score = sc;
                    }
                }
                diag_in = up_in;
            }
#pragma unroll
            for (int a = 0; a < A; ++a) {
                ccur[a] = cnxt[a];
#pragma unroll
                for (int r = 0; r < R; ++r) cur[a][r] = nxt[a][r];
            }
        }
        if (cout) {                                    // (uniform) lane 0 of the next pass reads what lane 63 wrote
            __threadfence();
            __syncthreads();
        }
    }
    if (cost_out && lane == (g_last & 63)) cost_out[u.b] = score;
    {
        const unsigned long long any_bad = __ballot(bad != 0);
        if (status && lane == 0) status[u.b] = any_bad ? 1 : 0;
    }
    if (global_store) __threadfence();
    __syncthreads();                                   // one wave: the words written above are read by other lanes below

    // the backtrack: every lane walks alike.  Lane (k & 63) keeps the k-th entry from the end; 64 entries leave in one store.
    u32* rev = grev + u.rev_off;
    const int CB = DTW_LDS_WORDS / G;                  // whole columns a stage holds (G <= 256: at least 48)
    int i = N - 1, j = M - 1, k = 0;
    u32 kept = 0;
    bool done = false;
    while (!done) {
        int j_lo = 0;
        const u32* rd = lbits;                         // rd[j * G + g]
        if (global_store) {
            j_lo = j - CB + 1 > 0 ? j - CB + 1 : 0;
            const int n = (j - j_lo + 1) * G;
            const u32* gsrc = bits + (long)j_lo * G;
            for (int e = lane; e < n; e += 64) lbits[e] = gsrc[e];
            __syncthreads();
            rd = lbits - (long)j_lo * G;
        }
        for (;;) {
            kept = lane == (k & 63) ? ((u32)i << 16 | (u32)j) : kept;
            if ((k & 63) == 63) rev[k - 63 + lane] = kept;
            ++k;
            if (i == 0 && j == 0) {
                done = true;
                break;
            }
            int dec;
            if (i == 0) dec = 2;                       // row 0 and column 0: pk_dtw.h
            else if (j == 0) dec = 1;
            else dec = __builtin_amdgcn_readfirstlane((int)((rd[(long)j * G + (i >> RS)] >> (2 * (i & (R - 1)))) & 3u));
            if (dec == 0) {
                --i;
                --j;
            } else if (dec == 1) {
                --i;
            } else {
                --j;
            }
            if (j < j_lo) break;
        }
        if (global_store) __syncthreads();             // the stage is overwritten next
    }
    const int P = k;
    if (lane < (P & 63)) rev[(P & ~63) + lane] = kept;
    __threadfence();
    __syncthreads();
    int* pix = ix + u.path_off;
    int* piy = iy + u.path_off;
    for (int p = lane; p < P; p += 64) {
        const u32 v = rev[P - 1 - p];
        pix[p] = (int)(v >> 16);
        piy[p] = (int)(v & 0xffffu);
    }
    if (lane == 0) plen[u.b] = P;
}

__global__ __launch_bounds__(DTW_STATS_THREADS) void k_dtw_path_stats(const int* __restrict__ ix, const int* __restrict__ iy,
                                                                      const int* __restrict__ plen, const float* __restrict__ x,
                                                                      const float* __restrict__ y,
                                                                      const unsigned char* __restrict__ mx,
                                                                      const unsigned char* __restrict__ my,
                                                                      const dtw_feat* __restrict__ pairs, int k0, int K,
                                                                      double* __restrict__ sums, long long* __restrict__ counts,
                                                                      int* __restrict__ status) {
    constexpr int T = DTW_STATS_THREADS;
    __shared__ double a_sq[T];
    __shared__ double a_rt[T];
    __shared__ long long a_n[4 * T];
    __shared__ int s_bad[1];
    const dtw_feat u = pairs[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0) s_bad[0] = 0;
    int P = plen[u.b];
    bool bad = P < 1 || P > u.N + u.M - 1;
    if (bad) P = 0;
    double sq = 0.0, rt = 0.0;
    long long n[4] = {0, 0, 0, 0};
    for (int p = t; p < P; p += T) {                   // THE ORDER of pk_dtw.h
        const int i = ix[u.path_off + p], j = iy[u.path_off + p];
        if (i < 0 || i >= u.N || j < 0 || j >= u.M) {
            bad = true;
            continue;
        }
        const bool vx = mx ? mx[u.mx_off + i] != 0 : true, vy = my ? my[u.my_off + j] != 0 : true;
        const int cls = (vx ? 0 : 2) + (vy ? 0 : 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) n[c] += cls == c ? 1 : 0;
        if (vx && vy) {
            const double s = dtw_sq_dist(x + u.xoff + (long)i * u.xs + k0, y + u.yoff + (long)j * u.ys + k0, K);
            sq = sq + s;
            rt = rt + sqrt(s);
        }
    }
    a_sq[t] = sq;
    a_rt[t] = rt;
#pragma unroll
    for (int c = 0; c < 4; ++c) a_n[c * T + t] = n[c];
    __syncthreads();
    if (bad) s_bad[0] = 1;
    for (int h = T / 2; h >= 1; h >>= 1) {
        if (t < h) {
            a_sq[t] = a_sq[t] + a_sq[t + h];
            a_rt[t] = a_rt[t] + a_rt[t + h];
#pragma unroll
            for (int c = 0; c < 4; ++c) a_n[c * T + t] += a_n[c * T + t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        sums[2 * u.b] = a_sq[0];
        sums[2 * u.b + 1] = a_rt[0];
#pragma unroll
        for (int c = 0; c < 4; ++c) counts[4 * u.b + c] = a_n[c * T];
        if (status) status[u.b] = s_bad[0] ? 2 : 0;
    }
}

template <int R>
int dtw_launch(pk_ctx* ctx, int n, size_t lds, const float* cost, const dtw_pair* pairs, int* ix, int* iy, int* plen,
               double* cost_out, int* status, u32* gbits, double* gcarry, u32* grev) {
    PK_LAUNCH(ctx, "dtw", (k_dtw<R>), dim3(n), dim3(64), lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
    return PK_OK;
}

int dtw_launch_r(int R, pk_ctx* ctx, int n, size_t lds, const float* cost, const dtw_pair* pairs, int* ix, int* iy, int* plen,
                 double* cost_out, int* status, u32* gbits, double* gcarry, u32* grev) {
    switch (R) {
        case 1: return dtw_launch<1>(ctx, n, lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
        case 2: return dtw_launch<2>(ctx, n, lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
        case 4: return dtw_launch<4>(ctx, n, lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
        case 8: return dtw_launch<8>(ctx, n, lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
        default: return dtw_launch<16>(ctx, n, lds, cost, pairs, ix, iy, plen, cost_out, status, gbits, gcarry, grev);
    }
}

std::atomic<long> g_cost_cap{DTW_COST_CAP_BYTES};

// the checks every entry point shares; `who` names it
int dtw_check(const char* who, int32_t mode, const void* x, const void* y, const int64_t* offs_x, const int64_t* offs_y,
              int64_t stride_x, int64_t stride_y, int32_t D, int32_t k0, int32_t k1, const int32_t* rows, const int32_t* cols,
              int32_t B) {
    if (!x || !rows || !cols || (mode == 1 && !y)) PK_FAIL(PK_EINVAL, "%s: NULL argument", who);
    if (B <= 0) PK_FAIL(PK_EINVAL, "%s: batch size must be positive", who);
    if (B > 65535) PK_FAIL(PK_EUNSUPPORTED, "%s: %d pairs; the engine's envelope is 65535 in a call", who, (int)B);
    if (stride_x < 0 || stride_y < 0) PK_FAIL(PK_EINVAL, "%s: negative stride", who);
    if ((!offs_x && stride_x) || (mode == 1 && !offs_y && stride_y))
        PK_FAIL(PK_EINVAL, "%s: a stride needs the pairs' offsets (NULL offsets mean contiguous pairs)", who);
    if (mode == 1) {
        if (D < 1) PK_FAIL(PK_EINVAL, "%s: feature dimension %d must be positive", who, (int)D);
        if (k0 < 0 || k1 <= k0 || k1 > D) PK_FAIL(PK_EINVAL, "%s: column range [%d, %d) does not lie in [0, %d)", who, (int)k0, (int)k1, (int)D);
        if (D > DTW_MAX_DIM) PK_FAIL(PK_EUNSUPPORTED, "%s: feature dimension %d; the engine's envelope is 1 ... %d", who, (int)D, DTW_MAX_DIM);
        if ((stride_x && stride_x < D) || (stride_y && stride_y < D)) PK_FAIL(PK_EINVAL, "%s: a row stride below the feature dimension %d", who, (int)D);
    }
    for (int b = 0; b < B; ++b) {
        if (rows[b] < 1 || cols[b] < 1) PK_FAIL(PK_EINVAL, "%s: pair %d is empty (%d rows x %d columns)", who, b, rows[b], cols[b]);
        if (rows[b] > DTW_MAX_ROWS) PK_FAIL(PK_EUNSUPPORTED, "%s: pair %d has %d rows; the engine's envelope is 1 ... %d", who, b, rows[b], DTW_MAX_ROWS);
        if (cols[b] > DTW_MAX_COLS) PK_FAIL(PK_EUNSUPPORTED, "%s: pair %d has %d columns; the engine's envelope is 1 ... %d", who, b, cols[b], DTW_MAX_COLS);
        if (mode == 0 && stride_x && stride_x < cols[b])
            PK_FAIL(PK_EINVAL, "%s: pair %d: row stride %ld below its %d columns", who, b, (long)stride_x, cols[b]);
        if ((offs_x && offs_x[b] < 0) || (mode == 1 && offs_y && offs_y[b] < 0)) PK_FAIL(PK_EINVAL, "%s: pair %d has a negative offset", who, b);
    }
    return PK_OK;
}

// the feature table of a call: where every pair's x and y start
void dtw_feat_table(std::vector<dtw_feat>& tab, const int64_t* offs_x, const int64_t* offs_y, int64_t stride_x, int64_t stride_y,
                    int32_t D, const int32_t* rows, const int32_t* cols, int32_t B) {
    tab.resize(B);
    long ox = 0, oy = 0, op = 0, omx = 0, omy = 0;
    for (int b = 0; b < B; ++b) {
        const long xs = stride_x ? stride_x : D, ys = stride_y ? stride_y : D;
        tab[b] = dtw_feat{offs_x ? offs_x[b] : ox, offs_y ? offs_y[b] : oy, xs, ys, 0, op, omx, omy, rows[b], cols[b], b, 0};
        ox += rows[b] * xs;
        oy += cols[b] * ys;
        op += rows[b] + cols[b] - 1;
        omx += rows[b];
        omy += cols[b];
    }
}

int dtw_cost_launch(pk_ctx* ctx, const float* x, const float* y, const dtw_feat* dev_tab, const dtw_feat* host_tab, int n, int k0,
                    int K, float* out) {
    int mi = 1, mj = 1;
    for (int b = 0; b < n; ++b) {
        mi = std::max(mi, pk_div_up(host_tab[b].N, DTW_TILE));
        mj = std::max(mj, pk_div_up(host_tab[b].M, DTW_TILE));
    }
    PK_LAUNCH(ctx, "dtw_cost", k_dtw_cost, dim3(mj, mi, n), dim3(DTW_COST_THREADS), 0, x, y, dev_tab, k0, K, out);
    return PK_OK;
}

}  // namespace

extern "C" int pk_dtw_lds_words(int32_t* words) {
    if (!words) PK_FAIL(PK_EINVAL, "pk_dtw_lds_words: NULL argument");
    *words = DTW_LDS_WORDS;
    return PK_OK;
}

extern "C" int pk_dtw_cost_cap(int64_t set_bytes, int64_t* bytes_out) {
    if (set_bytes < 0) PK_FAIL(PK_EINVAL, "pk_dtw_cost_cap: a negative cap");
    if (set_bytes) g_cost_cap.store((long)set_bytes);
    if (bytes_out) *bytes_out = g_cost_cap.load();
    return PK_OK;
}

extern "C" int pk_dtw_cost(pk_ctx* ctx, const float* x, const float* y, const int64_t* offs_x, const int64_t* offs_y,
                           int64_t stride_x, int64_t stride_y, int32_t D, int32_t k0, int32_t k1, const int32_t* rows,
                           const int32_t* cols, int32_t B, float* cost_out) {
    if (!ctx || !cost_out) PK_FAIL(PK_EINVAL, "pk_dtw_cost: NULL argument");
    PK_TRY(dtw_check("pk_dtw_cost", 1, x, y, offs_x, offs_y, stride_x, stride_y, D, k0, k1, rows, cols, B));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    std::vector<dtw_feat> tab;
    dtw_feat_table(tab, offs_x, offs_y, stride_x, stride_y, D, rows, cols, B);
    long oc = 0;
    for (auto& u : tab) {
        u.coff = oc;
        oc += (long)u.N * u.M;
    }
    PK_TRY(pk_upload(ctx, sc->dtw_tab, tab.data(), tab.size() * sizeof(dtw_feat)));
    return dtw_cost_launch(ctx, x, y, sc->dtw_tab.as<dtw_feat>(), tab.data(), B, k0, k1 - k0, cost_out);
}

extern "C" int pk_dtw_run(pk_ctx* ctx, int32_t mode, const float* x_or_cost, const float* y, const int64_t* offs_x,
                          const int64_t* offs_y, int64_t stride_x, int64_t stride_y, int32_t D, int32_t k0, int32_t k1,
                          const int32_t* rows, const int32_t* cols, int32_t B, int32_t* ix_out, int32_t* iy_out, int32_t* len_out,
                          double* cost_out, int32_t* status_out) {
    if (!ctx || !ix_out || !iy_out || !len_out) PK_FAIL(PK_EINVAL, "pk_dtw_run: NULL argument");
    if (mode != 0 && mode != 1) PK_FAIL(PK_EINVAL, "pk_dtw_run: mode = %d is neither 0 (cost matrix) nor 1 (features)", (int)mode);
    PK_TRY(dtw_check("pk_dtw_run", mode, x_or_cost, y, offs_x, offs_y, stride_x, stride_y, D, k0, k1, rows, cols, B));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);

    // launches: consecutive pairs in the caller's order whose cost matrices fit the cap together (feature mode); one otherwise
    std::vector<dtw_feat> feat;
    std::vector<int> first{0};                         // first pair of every launch, then B
    long cost_floats = 0;
    if (mode == 1) {
        dtw_feat_table(feat, offs_x, offs_y, stride_x, stride_y, D, rows, cols, B);
        const long cap = g_cost_cap.load() / (long)sizeof(float);
        long oc = 0;
        for (int b = 0; b < B; ++b) {
            const long sz = (long)rows[b] * cols[b];
            if (oc && oc + sz > cap) {
                first.push_back(b);
                oc = 0;
            }
            feat[b].coff = oc;
            oc += sz;
            cost_floats = std::max(cost_floats, oc);
        }
    }
    first.push_back(B);

    // the search's table: inside a launch ordered by rows per strip (one grid per value that occurs); outputs in the call's order
    std::vector<dtw_pair> tab(B);
    long o = 0, op = 0, gwords = 0, gcarry = 0, grev = 0;
    for (int b = 0; b < B; ++b) {
        const int N = rows[b], M = cols[b];
        dtw_pair u{};
        if (mode == 1) {
            u.off = feat[b].coff;
            u.row_stride = M;
        } else {
            u.row_stride = stride_x ? stride_x : M;
            u.off = offs_x ? offs_x[b] : o;
            o += (long)N * u.row_stride;
        }
        u.path_off = op;
        op += N + M - 1;
        u.bits_off = -1;
        if (dtw_words(N, M) > DTW_LDS_WORDS) {         // 128-byte aligned per pair
            u.bits_off = gwords;
            gwords += (dtw_words(N, M) + 31) / 32 * 32;
        }
        u.carry_off = gcarry;
        if (dtw_strips(N) > 64) gcarry += 2L * M;
        u.rev_off = grev;
        grev += (N + M - 1 + 63) / 64 * 64;
        u.N = N;
        u.M = M;
        u.b = b;
        tab[b] = u;
    }
    for (size_t c = 0; c + 1 < first.size(); ++c)
        std::stable_sort(tab.begin() + first[c], tab.begin() + first[c + 1],
                         [](const dtw_pair& a, const dtw_pair& c2) { return dtw_strip_rows(a.N) < dtw_strip_rows(c2.N); });
    if (cost_floats) PK_TRY(sc->dtw_cost.reserve((size_t)cost_floats * sizeof(float)));
    if (gwords) PK_TRY(sc->dtw_bits.reserve((size_t)gwords * sizeof(u32)));
    if (gcarry) PK_TRY(sc->dtw_carry.reserve((size_t)gcarry * sizeof(double)));
    PK_TRY(sc->dtw_rev.reserve((size_t)grev * sizeof(u32)));
    // one upload: the search's table, then feature mode's
    const size_t tab_bytes = tab.size() * sizeof(dtw_pair), feat_bytes = feat.size() * sizeof(dtw_feat);
    std::vector<unsigned char> blob(tab_bytes + feat_bytes);
    std::memcpy(blob.data(), tab.data(), tab_bytes);
    if (feat_bytes) std::memcpy(blob.data() + tab_bytes, feat.data(), feat_bytes);
    PK_TRY(pk_upload(ctx, sc->dtw_tab, blob.data(), blob.size()));
    const dtw_pair* dtab = sc->dtw_tab.as<dtw_pair>();
    const dtw_feat* dfeat = reinterpret_cast<const dtw_feat*>(sc->dtw_tab.as<unsigned char>() + tab_bytes);
    static_assert(sizeof(dtw_pair) % 8 == 0 && sizeof(dtw_feat) % 8 == 0, "the tables follow one another in one buffer");
    const float* src = mode == 1 ? sc->dtw_cost.as<float>() : x_or_cost;

    for (size_t c = 0; c + 1 < first.size(); ++c) {
        const int lo = first[c], hi = first[c + 1];
        if (mode == 1) PK_TRY(dtw_cost_launch(ctx, x_or_cost, y, dfeat + lo, feat.data() + lo, hi - lo, k0, k1 - k0, sc->dtw_cost.as<float>()));
        for (int i = lo; i < hi;) {
            const int R = dtw_strip_rows(tab[i].N);
            int j = i;
            size_t lds = 0;
            for (; j < hi && dtw_strip_rows(tab[j].N) == R; ++j) {
                const size_t need = (tab[j].bits_off >= 0 ? (size_t)DTW_LDS_WORDS : (size_t)dtw_words(tab[j].N, tab[j].M)) * sizeof(u32);
                lds = std::max(lds, need);
            }
            PK_TRY(dtw_launch_r(R, ctx, j - i, lds, src, dtab + i, ix_out, iy_out, len_out, cost_out, status_out,
                                sc->dtw_bits.as<u32>(), sc->dtw_carry.as<double>(), sc->dtw_rev.as<u32>()));
            i = j;
        }
    }
    return PK_OK;
}

extern "C" int pk_dtw_path_stats(pk_ctx* ctx, const int32_t* ix, const int32_t* iy, const int32_t* len, const float* x,
                                 const float* y, const int64_t* offs_x, const int64_t* offs_y, int64_t stride_x, int64_t stride_y,
                                 int32_t D, int32_t k0, int32_t k1, const int32_t* rows, const int32_t* cols, int32_t B,
                                 const uint8_t* mask_x, const uint8_t* mask_y, double* sums_out, int64_t* counts_out,
                                 int32_t* status_out) {
    if (!ctx || !ix || !iy || !len || !sums_out || !counts_out) PK_FAIL(PK_EINVAL, "pk_dtw_path_stats: NULL argument");
    PK_TRY(dtw_check("pk_dtw_path_stats", 1, x, y, offs_x, offs_y, stride_x, stride_y, D, k0, k1, rows, cols, B));
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    std::vector<dtw_feat> tab;
    dtw_feat_table(tab, offs_x, offs_y, stride_x, stride_y, D, rows, cols, B);
    PK_TRY(pk_upload(ctx, sc->dtw_tab, tab.data(), tab.size() * sizeof(dtw_feat)));
    PK_LAUNCH(ctx, "dtw_path_stats", k_dtw_path_stats, dim3(B), dim3(DTW_STATS_THREADS), 0, ix, iy, len, x, y, mask_x, mask_y,
              sc->dtw_tab.as<dtw_feat>(), k0, k1 - k0, sums_out, reinterpret_cast<long long*>(counts_out), status_out);
    return PK_OK;
}
