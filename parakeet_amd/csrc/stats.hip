// stats.hip -- streaming mean / variance of ragged feature matrices on gfx950: the accumulator behind
// normalizer.FeatureStats, which writes the (2, D) *_stats.npy files every model and vocoder here reads.  The definition,
// THE ORDER of every sum and the envelope: pk_stats.h.  Memory-bound: every input byte is read once.
//
// k_stats_tile:  one workgroup per row tile of one utterance: CW column slots x G row slots (pk_stats.h: lanes over columns
//                for wide D, over (row, column) pairs for narrow D), float64 partials, a halving tree over the row slots in
//                LDS; the tile's 2 D partial sums go to a workspace.
// k_stats_utt:   one workgroup per utterance adds its tiles' partials in ascending order -> U (B x 2 D float64).
// k_stats_fold:  adds U_0, U_1, ... to the state in call order (staged through LDS 256 utterances at a time).
// No atomics anywhere: they would break the order.
#include <vector>

#include "pk_common.h"
#include "pk_stats.h"

namespace {

struct st_tile {
    long row0;   // first row of the tile in the packed input
    int rows;    // 1 ... R
    int pad_;
};
struct st_utt {
    long tile0;  // the utterance's first tile in the workspace
    int ntiles;
    int pad_;
};

__global__ __launch_bounds__(STATS_THREADS) void k_stats_tile(const float* __restrict__ x, const float* __restrict__ K,
                                                              const st_tile* __restrict__ tiles, int D, int cw_log2,
                                                              double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double p1[STATS_THREADS], p2[STATS_THREADS];
    const st_tile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, CW = 1 << cw_log2, G = STATS_THREADS >> cw_log2;
    const int j = tid & (CW - 1), g = tid >> cw_log2;
    const float* base = x + t.row0 * D;
    double* out = part + (long)blockIdx.x * 2 * D;
    for (int c0 = 0; c0 < D; c0 += CW) {               // (uniform)
        const int c = c0 + j;
        double a1 = 0.0, a2 = 0.0;
        if (c < D) {
            const double k = (double)K[c];
            const float* col = base + c;
            int r = g;
            for (; r + (STATS_UNROLL - 1) * G < t.rows; r += STATS_UNROLL * G) {   // THE ORDER of pk_stats.h: rows ascending
                float v[STATS_UNROLL];
#pragma unroll
                for (int i = 0; i < STATS_UNROLL; ++i) v[i] = col[(long)(r + i * G) * D];
#pragma unroll
                for (int i = 0; i < STATS_UNROLL; ++i) {
                    const double d = (double)v[i] - k;
                    const double q = d * d;
                    a1 = a1 + d;
                    a2 = a2 + q;
                }
            }
            for (; r < t.rows; r += G) {
                const double d = (double)col[(long)r * D] - k;
                const double q = d * d;
                a1 = a1 + d;
                a2 = a2 + q;
            }
        }
        p1[tid] = a1;
        p2[tid] = a2;
        __syncthreads();
        for (int s = G >> 1; s >= 1; s >>= 1) {        // the halving tree over the row slots
            if (g < s) {
                p1[tid] = p1[tid] + p1[tid + (s << cw_log2)];
                p2[tid] = p2[tid] + p2[tid + (s << cw_log2)];
            }
            __syncthreads();
        }
        if (g == 0 && c < D) {
            out[c] = p1[tid];
            out[D + c] = p2[tid];
        }
        __syncthreads();                               // the next chunk of columns writes p1, p2 again
    }
}

__global__ __launch_bounds__(STATS_THREADS) void k_stats_utt(const double* __restrict__ part, const st_utt* __restrict__ utts,
                                                             int D2, double* __restrict__ U) {
    const st_utt u = utts[blockIdx.x];
    for (int v = threadIdx.x; v < D2; v += STATS_THREADS) {
        const double* p = part + u.tile0 * D2 + v;
        double a = 0.0;
        for (int i = 0; i < u.ntiles; ++i) a = a + p[(long)i * D2];   // ascending tiles
        U[(long)blockIdx.x * D2 + v] = a;
    }
}

// One workgroup per STATS_FOLD_COLS of the 2 D sums: its work items stage STATS_FOLD_ROWS utterances' values in LDS with all
// their loads in flight at once, then one work item per value adds them in call order.  The chain of B additions per value
// is the definition; staging only keeps it from waiting for memory once per utterance.
__global__ __launch_bounds__(STATS_THREADS) void k_stats_fold(const double* __restrict__ U, int B, int D2,
                                                              double* __restrict__ state) {
    constexpr int LOADERS = STATS_THREADS / STATS_FOLD_COLS, PER = STATS_FOLD_ROWS / LOADERS;
    __shared__ double stage[STATS_FOLD_ROWS][STATS_FOLD_COLS];
    const int vv = threadIdx.x % STATS_FOLD_COLS, rl = threadIdx.x / STATS_FOLD_COLS;
    const int v = blockIdx.x * STATS_FOLD_COLS + vv;
    const bool live = v < D2;
    double s = (live && rl == 0) ? state[v] : 0.0;
    for (int b0 = 0; b0 < B; b0 += STATS_FOLD_ROWS) {  // (uniform)
        const int nb = B - b0 < STATS_FOLD_ROWS ? B - b0 : STATS_FOLD_ROWS;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = rl + i * LOADERS;
            if (live && r < nb) stage[r][vv] = U[(long)(b0 + r) * D2 + v];
        }
        __syncthreads();
        if (live && rl == 0) {                         // call order; the LDS reads of 16 utterances are issued before their additions
            int r = 0;
            for (; r + 16 <= nb; r += 16) {
                double t[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) t[i] = stage[r + i][vv];
#pragma unroll
                for (int i = 0; i < 16; ++i) s = s + t[i];
            }
            for (; r < nb; ++r) s = s + stage[r][vv];
        }
        __syncthreads();
    }
    if (live && rl == 0) state[v] = s;
}

}  // namespace

struct pk_stats {
    pk_ctx* ctx = nullptr;
    int D = 0;
    bool have_k = false;
    int64_t n = 0;
    pk_dbuf d_k, d_state;                  // K (D floats); S1 | S2 (2 D doubles)
    pk_dbuf ws_tiles, ws_utts, ws_part, ws_u;
};

extern "C" int pk_stats_tile_rows(int32_t D, int32_t* rows) {
    if (!rows) PK_FAIL(PK_EINVAL, "pk_stats_tile_rows: NULL argument");
    if (D < 1 || D > STATS_MAX_DIM)
        PK_FAIL(PK_EUNSUPPORTED, "pk_stats_tile_rows: feature dimension %d; the engine's envelope is 1 ... %d", (int)D, STATS_MAX_DIM);
    *rows = stats_tile_rows(D);
    return PK_OK;
}

extern "C" int pk_stats_create(pk_ctx* ctx, int32_t D, pk_stats** out) {
    if (!ctx || !out) PK_FAIL(PK_EINVAL, "pk_stats_create: NULL argument");
    if (D < 1 || D > STATS_MAX_DIM)
        PK_FAIL(PK_EUNSUPPORTED, "pk_stats_create: feature dimension %d; the engine's envelope is 1 ... %d", (int)D, STATS_MAX_DIM);
    PK_DEVICE(ctx->device);
    pk_stats* h = new pk_stats();
    h->ctx = ctx;
    h->D = D;
    int s = h->d_k.reserve((size_t)D * sizeof(float));
    if (s == PK_OK) s = h->d_state.reserve((size_t)2 * D * sizeof(double));
    if (s == PK_OK && hipMemsetAsync(h->d_k.p, 0, (size_t)D * sizeof(float), ctx->stream) != hipSuccess) s = PK_EHIP;
    if (s == PK_OK && hipMemsetAsync(h->d_state.p, 0, (size_t)2 * D * sizeof(double), ctx->stream) != hipSuccess) s = PK_EHIP;
    if (s != PK_OK) {
        if (s == PK_EHIP) pk_set_error("pk_stats_create: hipMemsetAsync failed");
        h->d_k.release();
        h->d_state.release();
        delete h;
        return s;
    }
    *out = h;
    return PK_OK;
}

extern "C" void pk_stats_destroy(pk_stats* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->d_k, &h->d_state, &h->ws_tiles, &h->ws_utts, &h->ws_part, &h->ws_u};
    for (auto* b : bufs) b->release();
    delete h;
}

extern "C" int pk_stats_reset(pk_stats* h, const float* shift) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_stats_reset: NULL argument");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    h->n = 0;
    h->have_k = shift != nullptr;
    PK_HIP(hipMemsetAsync(h->d_state.p, 0, (size_t)2 * h->D * sizeof(double), ctx->stream));
    if (shift) PK_HIP(hipMemcpyAsync(h->d_k.p, shift, (size_t)h->D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    else PK_HIP(hipMemsetAsync(h->d_k.p, 0, (size_t)h->D * sizeof(float), ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));         // the caller's shift may leave scope
    return PK_OK;
}

extern "C" int pk_stats_update(pk_stats* h, const float* rows, const int64_t* lens, int32_t B, double* moments_out,
                               int32_t flags) {
    if (!h || !lens) PK_FAIL(PK_EINVAL, "pk_stats_update: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_stats_update: batch size must be positive");
    if (flags & ~PK_STATS_MOMENTS_ONLY) PK_FAIL(PK_EINVAL, "pk_stats_update: unknown flags %d", (int)flags);
    const bool only = (flags & PK_STATS_MOMENTS_ONLY) != 0;
    if (only && !moments_out) PK_FAIL(PK_EINVAL, "pk_stats_update: PK_STATS_MOMENTS_ONLY without moments_out");
    const int D = h->D, D2 = 2 * D, R = stats_tile_rows(D);
    long total = 0, ntiles = 0;
    int first = -1;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0) PK_FAIL(PK_EINVAL, "pk_stats_update: utterance %d has a negative length", b);
        if (lens[b] > 0x7fffffffL)
            PK_FAIL(PK_EUNSUPPORTED, "pk_stats_update: utterance %d has %ld rows; the engine's envelope is 2^31 - 1", b, (long)lens[b]);
        if (first < 0 && lens[b] > 0) first = b;
        total += lens[b];
        ntiles += (lens[b] + R - 1) / R;
        if (ntiles > STATS_MAX_TILES)
            PK_FAIL(PK_EUNSUPPORTED, "pk_stats_update: more than %ld tiles of %d rows in one update; split the call", STATS_MAX_TILES, R);
    }
    if (total > 0 && !rows) PK_FAIL(PK_EINVAL, "pk_stats_update: NULL rows");
    if (only && !h->have_k) PK_FAIL(PK_ESTATE, "pk_stats_update: PK_STATS_MOMENTS_ONLY before the shift is fixed");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    if (total == 0) {                                  // nothing to add; the shift stays open
        if (moments_out) PK_HIP(hipMemsetAsync(moments_out, 0, (size_t)B * D2 * sizeof(double), ctx->stream));
        return PK_OK;
    }
    std::vector<st_tile> tiles;
    tiles.reserve((size_t)ntiles);
    std::vector<st_utt> utts(B);
    long row = 0, first_row = 0;
    for (int b = 0; b < B; ++b) {
        if (b == first) first_row = row;
        utts[b] = st_utt{(long)tiles.size(), (int)((lens[b] + R - 1) / R), 0};
        for (long r = 0; r < lens[b]; r += R) tiles.push_back(st_tile{row + r, (int)(lens[b] - r < R ? lens[b] - r : R), 0});
        row += lens[b];
    }
    if (!h->have_k) {                                  // the first row the accumulator ever sees
        PK_HIP(hipMemcpyAsync(h->d_k.p, rows + first_row * D, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        h->have_k = true;
    }
    PK_TRY(h->ws_part.reserve((size_t)ntiles * D2 * sizeof(double)));
    double* U = moments_out;
    if (!U) {
        PK_TRY(h->ws_u.reserve((size_t)B * D2 * sizeof(double)));
        U = h->ws_u.as<double>();
    }
    PK_TRY(h->ws_utts.reserve(utts.size() * sizeof(st_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utts.p, utts.data(), utts.size() * sizeof(st_utt), hipMemcpyHostToDevice, ctx->stream));
    PK_TRY(pk_upload(ctx, h->ws_tiles, tiles.data(), tiles.size() * sizeof(st_tile)));   // (synchronises: both tables have left the host)
    int cw_log2 = 0;
    while ((1 << cw_log2) < stats_col_width(D)) ++cw_log2;
    PK_LAUNCH(ctx, "stats_tile", k_stats_tile, dim3((unsigned)ntiles), dim3(STATS_THREADS), 0, rows, h->d_k.as<float>(),
              h->ws_tiles.as<st_tile>(), D, cw_log2, h->ws_part.as<double>());
    PK_LAUNCH(ctx, "stats_utt", k_stats_utt, dim3((unsigned)B), dim3(STATS_THREADS), 0, h->ws_part.as<double>(),
              h->ws_utts.as<st_utt>(), D2, U);
    if (!only) {
        PK_LAUNCH(ctx, "stats_fold", k_stats_fold, dim3((unsigned)pk_div_up(D2, STATS_FOLD_COLS)), dim3(STATS_THREADS), 0, U, (int)B,
                  D2, h->d_state.as<double>());
        h->n += total;
    }
    return PK_OK;
}

extern "C" int pk_stats_get(pk_stats* h, int64_t* n, int32_t* have_shift, float* shift, double* s1, double* s2) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_stats_get: NULL argument");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const size_t nb = (size_t)h->D * sizeof(double);
    if (shift) PK_HIP(hipMemcpyAsync(shift, h->d_k.p, (size_t)h->D * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (s1) PK_HIP(hipMemcpyAsync(s1, h->d_state.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (s2) PK_HIP(hipMemcpyAsync(s2, h->d_state.as<char>() + nb, nb, hipMemcpyDeviceToHost, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    if (n) *n = h->n;
    if (have_shift) *have_shift = h->have_k ? 1 : 0;
    return PK_OK;
}

extern "C" int pk_stats_set(pk_stats* h, int64_t n, const float* shift, const double* s1, const double* s2) {
    if (!h || !s1 || !s2) PK_FAIL(PK_EINVAL, "pk_stats_set: NULL argument");
    if (n < 0) PK_FAIL(PK_EINVAL, "pk_stats_set: negative row count");
    if (n > 0 && !shift) PK_FAIL(PK_EINVAL, "pk_stats_set: a state that has seen rows has a shift");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const size_t nb = (size_t)h->D * sizeof(double);
    if (shift) PK_HIP(hipMemcpyAsync(h->d_k.p, shift, (size_t)h->D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    else PK_HIP(hipMemsetAsync(h->d_k.p, 0, (size_t)h->D * sizeof(float), ctx->stream));
    PK_HIP(hipMemcpyAsync(h->d_state.p, s1, nb, hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipMemcpyAsync(h->d_state.as<char>() + nb, s2, nb, hipMemcpyHostToDevice, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    h->n = n;
    h->have_k = shift != nullptr;
    return PK_OK;
}
