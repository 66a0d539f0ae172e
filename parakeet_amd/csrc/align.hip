// align.hip -- durations from a teacher's attention on gfx950: the monotonic alignment search of ragged
// batches (the best monotonic path through a score matrix, the dynamic programme of Glow-TTS's maximum_path) and the focus
// rate of attention maps (FastSpeech, 3.3).  The definition, the decision words' layout, the order of the focus rate's sum
// and the envelope: pk_align.h.  This is NOT the Montreal Forced Aligner.
//
// k_mas<C, ATT>:  one wave per utterance, C = ceil(T / 64) columns per lane, the previous row of Q in registers, the left
//                 neighbour's value by a DPP wave shift, one ballot per owned column for the decision bits (LDS or a global
//                 workspace), then the backtrack by every lane alike over decision words read from LDS.
// k_focus_rate:   one workgroup per map: a wave takes a row's maximum, float64 sums in the fixed order of pk_align.h.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pk_align.h"
#include "pk_common.h"

namespace {

typedef unsigned long long u64;

struct mas_utt {
    long off;         // first score of the utterance (floats)
    long row_stride;  // floats between rows
    long dur_off;     // first duration in the packed output (sum of T before it)
    long path_off;    // first path entry (sum of S before it)
    long v_off;       // first entry of the packed scores_out (sum of S * T before it)
    long bits_off;    // first 64-bit decision word in the global workspace; -1: LDS
    int S, T;
    int b, pad_;      // the utterance's number in the call
};

struct fr_map {
    long off, row_stride;
    int S, T;
};

constexpr double NEG_INF = -__builtin_huge_val();

// lane l receives lane l - 1's x; lane 0 receives fill (DPP wave_shr:1, two 32-bit moves)
__device__ __forceinline__ double mas_from_left(double x, double fill) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(x), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

template <int C, bool ATT>
__global__ __launch_bounds__(64) void k_mas(const float* __restrict__ in, const mas_utt* __restrict__ utts, float eps,
                                            int* __restrict__ dur, int* __restrict__ path, double* __restrict__ score,
                                            int* __restrict__ status, float* __restrict__ vout, u64* __restrict__ gbits) {
    constexpr int R = MAS_ROWS(C);
    extern __shared__ u64 lbits[];                     // the decision words (LDS store) or the stage of a global store
    const mas_utt u = utts[blockIdx.x];
    const int S = u.S, T = u.T, lane = threadIdx.x;
    const int t0 = lane * C;                           // the lane's first column
    const bool global_store = u.bits_off >= 0;         // (uniform)
    u64* bits = global_store ? gbits + u.bits_off : lbits;
    const float* src = in + u.off + t0;
    float* vdst = (ATT && vout) ? vout + u.v_off + t0 : nullptr;

    double q[C];                                       // Q(s - 1, t0 + c)
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = NEG_INF;
    int bad = 0;
    float cur[R][C], nxt[R][C];
    auto load = [&](float(&dst)[R][C], int s0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < C; ++c) dst[r][c] = (s0 + r < S && t0 + c < T) ? src[(long)(s0 + r) * u.row_stride + c] : 0.f;
    };
    load(cur, 0);
    for (int s0 = 0; s0 < S; s0 += R) {
        load(nxt, s0 + R);                             // (nothing past row S - 1 is read)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int s = s0 + r;
            if (s < S) {                               // (uniform)
                const double in_left = mas_from_left(q[C - 1], NEG_INF);
                double nq[C];
                u64 mine = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double left = c == 0 ? in_left : q[c - 1], up = q[c];
                    const bool stay = up >= left;      // ties stay
                    const double m = stay ? up : left;
                    float x = cur[r][c];
                    if (ATT) x = logf(x < eps ? eps : x);
                    const int col = t0 + c;
                    if (ATT && vdst && col < T) vdst[(long)s * T + c] = x;
                    const bool inside = col < T && col <= s;
                    if (inside && !(fabsf(x) <= 3.402823466e+38f)) bad = 1;
                    nq[c] = inside ? (s == 0 ? (double)x : (double)x + m) : NEG_INF;
                    const u64 w = __ballot(!stay);
                    mine = lane == c ? w : mine;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) q[c] = nq[c];
                if (lane < C) bits[(long)s * C + lane] = mine;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < C; ++c) cur[r][c] = nxt[r][c];
    }
    {
        const int lt = (T - 1) / C, ct = (T - 1) % C;
        double sc = q[0];
#pragma unroll
        for (int c = 1; c < C; ++c) sc = c == ct ? q[c] : sc;
        if (score && lane == lt) score[u.b] = sc;
        const u64 any_bad = __ballot(bad != 0);
        if (status && lane == 0) status[u.b] = any_bad ? 1 : 0;
    }
    if (global_store) __threadfence();
    __syncthreads();                                   // one wave: the words written above are read by other lanes below

    // the backtrack: every lane walks alike.  Lane (s & 63) keeps path[s]; 64 entries leave in one store.
    int t = T - 1, run_end = S - 1, kept = 0;
    int* pdst = path ? path + u.path_off : nullptr;
    int* ddst = dur + u.dur_off;
    constexpr int STAGE_ROWS = MAS_STAGE_WORDS64 / C;
    int s_hi = S - 1;
    while (s_hi >= 1) {
        int s_lo = 1;
        const u64* rd = lbits;                         // rd[s * C + c]: word c of row s
        if (global_store) {
            s_lo = s_hi - STAGE_ROWS + 1 > 1 ? s_hi - STAGE_ROWS + 1 : 1;
            const int n = (s_hi - s_lo + 1) * C;
            const u64* g = bits + (long)s_lo * C;
            for (int i = lane; i < n; i += 64) lbits[i] = g[i];
            __syncthreads();
            rd = lbits - (long)s_lo * C;
        }
        for (int s = s_hi; s >= s_lo; --s) {
            kept = lane == (s & 63) ? t : kept;
            if ((s & 63) == 0 && pdst && s + lane < S) pdst[s + lane] = kept;
            const u64 w = rd[(long)s * C + t % C];
            const int mv = __builtin_amdgcn_readfirstlane((int)((w >> (t / C)) & 1));
            if (mv && t > 0) {                         // (t > 0 always holds on finite scores)
                if (lane == 0) ddst[t] = run_end - s + 1;
                run_end = s - 1;
                --t;
            }
        }
        if (global_store) __syncthreads();
        s_hi = s_lo - 1;
    }
    kept = lane == 0 ? t : kept;                       // row 0
    if (pdst && lane < S) pdst[lane] = kept;
    if (lane == 0) ddst[t] = run_end + 1;
}

__global__ __launch_bounds__(FR_THREADS) void k_focus_rate(const float* __restrict__ att, const fr_map* __restrict__ maps,
                                                           double* __restrict__ out) {
    __shared__ double part[FR_WAVES];
    const fr_map m = maps[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int s = wave; s < m.S; s += FR_WAVES) {       // THE ORDER of pk_align.h
        const float* row = att + m.off + (long)s * m.row_stride;
        float mx = -__builtin_huge_valf();
        for (int t = lane; t < m.T; t += 64) mx = fmaxf(mx, row[t]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        acc += (double)mx;
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    static_assert(FR_WAVES == 4, "the fold below");
    if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + (part[2] + part[3])) / (double)m.S;
}

template <int C>
int mas_launch(pk_ctx* ctx, int n, size_t lds, int mode, const float* in, const mas_utt* utts, float eps, int* dur, int* path,
               double* score, int* status, float* vout, u64* gbits) {
    if (mode)
        PK_LAUNCH(ctx, "mas_att", (k_mas<C, true>), dim3(n), dim3(64), lds, in, utts, eps, dur, path, score, status, vout, gbits);
    else
        PK_LAUNCH(ctx, "mas", (k_mas<C, false>), dim3(n), dim3(64), lds, in, utts, eps, dur, path, score, status, vout, gbits);
    return PK_OK;
}

typedef int (*mas_launch_fn)(pk_ctx*, int, size_t, int, const float*, const mas_utt*, float, int*, int*, double*, int*, float*,
                             u64*);
const mas_launch_fn MAS_LAUNCH[MAS_MAX_C] = {mas_launch<1>,  mas_launch<2>,  mas_launch<3>,  mas_launch<4>,
                                            mas_launch<5>,  mas_launch<6>,  mas_launch<7>,  mas_launch<8>,
                                            mas_launch<9>,  mas_launch<10>, mas_launch<11>, mas_launch<12>,
                                            mas_launch<13>, mas_launch<14>, mas_launch<15>, mas_launch<16>};

}  // namespace

extern "C" int pk_mas_lds_words(int32_t* words) {
    if (!words) PK_FAIL(PK_EINVAL, "pk_mas_lds_words: NULL argument");
    *words = MAS_LDS_WORDS;
    return PK_OK;
}

extern "C" int pk_mas_run(pk_ctx* ctx, const float* scores_or_att, const int64_t* offs, int64_t row_stride, const int32_t* rows,
                          const int32_t* cols, int32_t B, int32_t mode, float eps, int32_t* durations_out, int32_t* path_out,
                          double* score_out, int32_t* status_out, float* scores_out) {
    if (!ctx || !scores_or_att || !rows || !cols || !durations_out) PK_FAIL(PK_EINVAL, "pk_mas_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_mas_run: batch size must be positive");
    if (mode != 0 && mode != 1) PK_FAIL(PK_EINVAL, "pk_mas_run: mode = %d is neither 0 (scores) nor 1 (attention)", (int)mode);
    if (mode == 1 && (!(eps > 0.f) || std::isinf(eps))) PK_FAIL(PK_EINVAL, "pk_mas_run: eps %g must be positive and finite", (double)eps);
    if (mode == 0 && scores_out) PK_FAIL(PK_EINVAL, "pk_mas_run: scores_out is written in attention mode only");
    if (row_stride < 0) PK_FAIL(PK_EINVAL, "pk_mas_run: negative stride");
    if (!offs && row_stride) PK_FAIL(PK_EINVAL, "pk_mas_run: a stride needs the utterances' offsets (NULL offsets mean contiguous maps)");
    for (int b = 0; b < B; ++b) {
        if (rows[b] < 1 || cols[b] < 1) PK_FAIL(PK_EINVAL, "pk_mas_run: utterance %d is empty (%d rows x %d tokens)", b, rows[b], cols[b]);
        if (cols[b] > rows[b])
            PK_FAIL(PK_EINVAL, "pk_mas_run: utterance %d has more tokens (%d) than rows (%d): no monotonic path gives every token a row",
                    b, cols[b], rows[b]);
        if (cols[b] > MAS_MAX_COLS)
            PK_FAIL(PK_EUNSUPPORTED, "pk_mas_run: utterance %d has %d tokens; the engine's envelope is 1 ... %d", b, cols[b], MAS_MAX_COLS);
        if (rows[b] > MAS_MAX_ROWS)
            PK_FAIL(PK_EUNSUPPORTED, "pk_mas_run: utterance %d has %d rows; the engine's envelope is 1 ... %d", b, rows[b], MAS_MAX_ROWS);
        if (row_stride && row_stride < cols[b])
            PK_FAIL(PK_EINVAL, "pk_mas_run: utterance %d: row stride %ld below its %d tokens", b, (long)row_stride, cols[b]);
        if (offs && offs[b] < 0) PK_FAIL(PK_EINVAL, "pk_mas_run: utterance %d has a negative offset", b);
    }
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    // the table, ordered by columns per lane (one launch per value that occurs); the outputs stay in the call's order
    std::vector<mas_utt> tab(B);
    long o = 0, od = 0, op = 0, ov = 0;
    for (int b = 0; b < B; ++b) {
        const long ss = row_stride ? row_stride : cols[b];
        tab[b] = mas_utt{offs ? offs[b] : o, ss, od, op, ov, -1, rows[b], cols[b], b, 0};
        o += (long)rows[b] * ss;
        od += cols[b];
        op += rows[b];
        ov += (long)rows[b] * cols[b];
    }
    std::stable_sort(tab.begin(), tab.end(),
                     [](const mas_utt& a, const mas_utt& c) { return mas_cols_per_lane(a.T) < mas_cols_per_lane(c.T); });
    long gwords = 0;                                   // 64-bit words of the global workspace, 128-byte aligned per utterance
    for (auto& u : tab)
        if (mas_words(u.S, u.T) > MAS_LDS_WORDS) {
            u.bits_off = gwords;
            gwords += ((long)u.S * mas_cols_per_lane(u.T) + 15) / 16 * 16;
        }
    if (gwords) PK_TRY(sc->mas_bits.reserve((size_t)gwords * sizeof(u64)));
    PK_TRY(pk_upload(ctx, sc->mas_tab, tab.data(), tab.size() * sizeof(mas_utt)));
    for (int i = 0; i < B;) {
        const int C = mas_cols_per_lane(tab[i].T);
        int j = i;
        size_t lds = 0;
        for (; j < B && mas_cols_per_lane(tab[j].T) == C; ++j) {
            const size_t need = tab[j].bits_off >= 0 ? (size_t)MAS_STAGE_WORDS64 * sizeof(u64) : (size_t)tab[j].S * C * sizeof(u64);
            lds = need > lds ? need : lds;
        }
        PK_TRY(MAS_LAUNCH[C - 1](ctx, j - i, lds, mode, scores_or_att, sc->mas_tab.as<mas_utt>() + i, eps, durations_out, path_out,
                                 score_out, status_out, scores_out, sc->mas_bits.as<u64>()));
        i = j;
    }
    return PK_OK;
}

extern "C" int pk_focus_rate_run(pk_ctx* ctx, const float* att, const int64_t* offs, int64_t map_stride, int64_t row_stride,
                                 const int32_t* maps, const int32_t* rows, const int32_t* cols, int32_t B, double* rates_out) {
    if (!ctx || !att || !maps || !rows || !cols || !rates_out) PK_FAIL(PK_EINVAL, "pk_focus_rate_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_focus_rate_run: batch size must be positive");
    if (map_stride < 0 || row_stride < 0) PK_FAIL(PK_EINVAL, "pk_focus_rate_run: negative stride");
    if (!offs && (map_stride || row_stride))
        PK_FAIL(PK_EINVAL, "pk_focus_rate_run: strides need the utterances' offsets (NULL offsets mean contiguous maps)");
    long n_map = 0;
    for (int b = 0; b < B; ++b) {
        if (maps[b] < 1 || rows[b] < 1 || cols[b] < 1)
            PK_FAIL(PK_EINVAL, "pk_focus_rate_run: utterance %d: %d maps of %d x %d", b, maps[b], rows[b], cols[b]);
        const long ss = row_stride ? row_stride : cols[b];
        if (ss < cols[b]) PK_FAIL(PK_EINVAL, "pk_focus_rate_run: utterance %d: row stride %ld below its %d columns", b, ss, cols[b]);
        if (map_stride && map_stride < (rows[b] - 1) * ss + cols[b])
            PK_FAIL(PK_EINVAL, "pk_focus_rate_run: utterance %d: map stride %ld below one map", b, (long)map_stride);
        if (offs && offs[b] < 0) PK_FAIL(PK_EINVAL, "pk_focus_rate_run: utterance %d has a negative offset", b);
        n_map += maps[b];
    }
    if (n_map > (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_focus_rate_run: %ld maps; the engine's envelope is 2^30", n_map);
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    std::vector<fr_map> tab;
    tab.reserve((size_t)n_map);
    long o = 0;
    for (int b = 0; b < B; ++b) {
        const long ss = row_stride ? row_stride : cols[b], gs = map_stride ? map_stride : rows[b] * ss;
        const long ob = offs ? offs[b] : o;
        for (int g = 0; g < maps[b]; ++g) tab.push_back(fr_map{ob + g * gs, ss, rows[b], cols[b]});
        o += maps[b] * gs;
    }
    PK_TRY(pk_upload(ctx, sc->mas_tab, tab.data(), tab.size() * sizeof(fr_map)));
    PK_LAUNCH(ctx, "focus_rate", k_focus_rate, dim3((unsigned)n_map), dim3(FR_THREADS), 0, att, sc->mas_tab.as<fr_map>(), rates_out);
    return PK_OK;
}
