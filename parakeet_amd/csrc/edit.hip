// edit.hip -- the edit (Levenshtein) distance of ragged batches of token sequences and its alignment on gfx950 (DESIGN.md
// 4.7c): what word, character and phone error rates are counted from (parakeet_amd/utils/error_rate.py).  The definition, the op
// words' layout and the envelope: pk_edit.h.  The recurrence is that of parakeet/utils/error_rate.py; the alignment (which
// of several minimal edit scripts is returned) is this project's own.
//
// k_edit<R, MODE>: one wave per pair, R rows per lane, lanes skewed by one column, the neighbour's bottom value by one DPP wave
//                  shift; MODE 1 keeps one 32-bit op word per lane and column (LDS or a global workspace) and walks back over
//                  them, every lane alike.  Integer arithmetic on ids: there is no cost matrix to read.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pk_common.h"
#include "pk_edit.h"

namespace {

typedef unsigned int u32;

struct edit_pair {
    long ref_off, hyp_off;   // first id of the pair's ref, of its hyp
    long ops_off;            // first op (sum of N + M before it)
    long bits_off;           // first op word in the global workspace; -1: LDS
    long carry_off;          // first int of the pair's two carry rows (pairs of several passes)
    long rev_off;            // first word of the pair's reversed ops
    int N, M;
    int b, pad_;             // the pair's number in the call
};

// lane l receives lane l - 1's x; lane 0 receives fill (DPP wave_shr:1)
__device__ __forceinline__ int edit_from_left(int x, int fill) {
    return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xf, 0xf, false);
}

template <int R, int MODE>
__global__ __launch_bounds__(64) void k_edit(const int* __restrict__ ref, const int* __restrict__ hyp,
                                             const edit_pair* __restrict__ pairs, int* __restrict__ dist_out,
                                             int* __restrict__ counts_out, unsigned char* __restrict__ ops_out,
                                             int* __restrict__ len_out, u32* __restrict__ gbits, int* __restrict__ gcarry,
                                             u32* __restrict__ grev) {
    constexpr int A = EDIT_AHEAD;
    constexpr int RS = R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : 4;
    static_assert((1 << RS) == R && R <= EDIT_MAX_STRIP, "a strip is 1, 2, 4, 8 or 16 rows");
    extern __shared__ u32 lbits[];                     // MODE 1: the op words (LDS store) or the stage of a global store
    const edit_pair u = pairs[blockIdx.x];
    const int N = u.N, M = u.M, lane = threadIdx.x;
    const int G = (N + R - 1) / R;                     // strips
    const bool global_store = MODE == 1 && u.bits_off >= 0;   // (uniform)
    u32* bits = global_store ? gbits + u.bits_off : lbits;
    const int npass = (N > 0 && M > 0) ? (G + 63) / 64 : 0;   // an empty side: D(N, 0) = N, D(0, M) = M, nothing to compute
    const int g_last = N > 0 ? (N - 1) >> RS : 0, r_last = (N - 1) & (R - 1);
    int score = N == 0 ? M : N;
    const int* rp = ref + u.ref_off;
    const int* hp = hyp + u.hyp_off;

    // rows and columns are counted from 0 below: row i is D's row i + 1 (ref id i), column j is D's column j + 1 (hyp id j)
    for (int pass = 0; pass < npass; ++pass) {
        const int g = pass * 64 + lane, i0 = g * R;    // the lane's strip and its first row
        const bool strip = g < G;
        const int lanes = G - pass * 64 < 64 ? G - pass * 64 : 64;
        const int steps = M + lanes - 1;
        const int* cin = pass > 0 ? gcarry + u.carry_off + (long)((pass - 1) & 1) * M : nullptr;
        int* cout = pass + 1 < npass ? gcarry + u.carry_off + (long)(pass & 1) * M : nullptr;
        const bool takes_carry = lane == 0 && pass > 0;

        int rt[R], q[R];                               // the strip's ref ids; D(i0 + r + 1, j) of the previous column
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rt[r] = i0 + r < N ? rp[i0 + r] : 0;
            q[r] = i0 + r + 1;                         // D(i, 0) = i
        }
        int bot = 0;                                   // D(i0 + R, j): what lane + 1 takes next step
        int diag_in = i0;                              // D(i0, j): the row above the strip, one column back
        int hcur[A], hnxt[A], ccur[A], cnxt[A];        // hyp ids; lane 0: the row above the pass
        auto load = [&](int(&hd)[A], int(&cd)[A], int t0) {
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const int j = t0 + a - lane;
                const bool in = j >= 0 && j < M;
                hd[a] = in ? hp[j] : 0;
                cd[a] = (in && takes_carry) ? cin[j] : j + 1;    // pass 0: D(0, j + 1) = j + 1
            }
        };
        load(hcur, ccur, 0);
        for (int t0 = 0; t0 < steps; t0 += A) {
            load(hnxt, cnxt, t0 + A);                  // (nothing outside the pair's M ids is read)
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const int j = t0 + a - lane;
                const bool in = strip && j >= 0 && j < M;
                int up_in = edit_from_left(bot, 0);
                up_in = lane == 0 ? ccur[a] : up_in;
                const int h = hcur[a];
                int nq[R];
                u32 w = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int d = r == 0 ? diag_in : q[r > 0 ? r - 1 : 0];
                    const int up = r == 0 ? up_in : nq[r > 0 ? r - 1 : 0];
                    const int lf = q[r];
                    const bool eq = rt[r] == h;
                    // e does not wait for the cell above; on equal ids d <= up + 1 (pk_edit.h), so min(e, up + 1) is d there
                    const bool lf_d = lf < d;
                    const int pre = lf_d ? lf : d;
                    const int e = eq ? d : pre + 1;
                    const int up1 = up + 1;
                    nq[r] = up1 < e ? up1 : e;
                    if (MODE == 1) {
                        // the op the walk back takes: a hit, else the smallest of d, up, lf; ties to d, then up
                        const bool take_up = lf_d ? up <= pre : up < pre;
                        const u32 op = eq ? 0u : (take_up ? 2u : (lf_d ? 3u : 1u));
                        w |= op << (2 * r);
                    }
                }
                if (in) {
#pragma unroll
                    for (int r = 0; r < R; ++r) q[r] = nq[r];
                    bot = nq[R - 1];
                    if (MODE == 1) bits[(long)j * G + g] = w;
                    if (cout && lane == 63) cout[j] = bot;
                    if (j == M - 1 && g == g_last) {
                        int sc = nq[0];
#pragma unroll
                        for (int r = 1; r < R; ++r) sc = r == r_last ? nq[r] : sc;
                        score = sc;
                    }
                }
                diag_in = j >= 0 ? up_in : i0;         // D(i0, 0) = i0 until the lane's first column
            }
#pragma unroll
            for (int a = 0; a < A; ++a) {
                hcur[a] = hnxt[a];
                ccur[a] = cnxt[a];
            }
        }
        if (cout) {                                    // (uniform) lane 0 of the next pass reads what lane 63 wrote
            __threadfence();
            __syncthreads();
        }
    }
    if (lane == (g_last & 63)) dist_out[u.b] = score;  // (with an empty side every lane holds the score)
    if (MODE == 0) return;

    if (global_store) __threadfence();
    __syncthreads();                                   // one wave: the words written above are read by other lanes below

    // the walk back: every lane walks alike.  Lane (k & 63) keeps the k-th op from the end; 64 ops leave in one store.
    u32* rev = grev + u.rev_off;
    const int CB = G > 0 ? EDIT_LDS_WORDS / G : 1;     // whole columns a stage holds (G <= 256: at least 48)
    int i = N, j = M, k = 0;                           // the cell of D
    int n_hit = 0, n_sub = 0, n_del = 0, n_ins = 0;
    u32 kept = 0;
    while (i > 0 || j > 0) {
        int j_lo = 0;                                  // the first column (from 0) the stage holds
        const u32* rd = lbits;                         // rd[j * G + g]
        const bool stage = global_store && i > 0 && j > 0;    // (uniform)
        if (stage) {
            j_lo = j - CB > 0 ? j - CB : 0;
            const int n = (j - j_lo) * G;
            const u32* gsrc = bits + (long)j_lo * G;
            for (int e = lane; e < n; e += 64) lbits[e] = gsrc[e];
            __syncthreads();
            rd = lbits - (long)j_lo * G;
        }
        for (;;) {
            int op;
            if (i == 0) op = 3;                        // row 0 and column 0: pk_edit.h
            else if (j == 0) op = 2;
            else {
                const int ri = i - 1;
                op = __builtin_amdgcn_readfirstlane((int)((rd[(long)(j - 1) * G + (ri >> RS)] >> (2 * (ri & (R - 1)))) & 3u));
            }
            kept = lane == (k & 63) ? (u32)op : kept;
            if ((k & 63) == 63) rev[k - 63 + lane] = kept;
            ++k;
            n_hit += op == 0;
            n_sub += op == 1;
            n_del += op == 2;
            n_ins += op == 3;
            i -= op != 3;
            j -= op != 2;
            if (i == 0 && j == 0) break;
            if (i > 0 && j > 0 && j - 1 < j_lo) break;         // the next word is in an earlier block of columns
        }
        if (stage) __syncthreads();                    // the stage is overwritten next
    }
    const int P = k;
    if (lane < (P & 63)) rev[(P & ~63) + lane] = kept;
    __threadfence();
    __syncthreads();
    unsigned char* po = ops_out + u.ops_off;
    for (int p = lane; p < P; p += 64) po[p] = (unsigned char)rev[P - 1 - p];
    if (lane == 0) {
        len_out[u.b] = P;
        counts_out[4 * u.b] = n_hit;
        counts_out[4 * u.b + 1] = n_sub;
        counts_out[4 * u.b + 2] = n_del;
        counts_out[4 * u.b + 3] = n_ins;
    }
}

template <int R, int MODE>
int edit_launch(pk_ctx* ctx, int n, size_t lds, const int* ref, const int* hyp, const edit_pair* pairs, int* dist, int* counts,
                unsigned char* ops, int* plen, u32* gbits, int* gcarry, u32* grev) {
    PK_LAUNCH(ctx, "edit", (k_edit<R, MODE>), dim3(n), dim3(64), lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
    return PK_OK;
}

template <int MODE>
int edit_launch_r(int R, pk_ctx* ctx, int n, size_t lds, const int* ref, const int* hyp, const edit_pair* pairs, int* dist,
                  int* counts, unsigned char* ops, int* plen, u32* gbits, int* gcarry, u32* grev) {
    switch (R) {
        case 1: return edit_launch<1, MODE>(ctx, n, lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
        case 2: return edit_launch<2, MODE>(ctx, n, lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
        case 4: return edit_launch<4, MODE>(ctx, n, lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
        case 8: return edit_launch<8, MODE>(ctx, n, lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
        default: return edit_launch<16, MODE>(ctx, n, lds, ref, hyp, pairs, dist, counts, ops, plen, gbits, gcarry, grev);
    }
}

}  // namespace

extern "C" int pk_edit_lds_words(int32_t* words) {
    if (!words) PK_FAIL(PK_EINVAL, "pk_edit_lds_words: NULL argument");
    *words = EDIT_LDS_WORDS;
    return PK_OK;
}

extern "C" int pk_edit_run(pk_ctx* ctx, const int32_t* ref, const int32_t* hyp, const int64_t* offs_ref, const int64_t* offs_hyp,
                           const int32_t* n, const int32_t* m, int32_t B, int32_t mode, int32_t* dist_out, int32_t* counts_out,
                           uint8_t* ops_out, int32_t* len_out) {
    if (!ctx || !ref || !hyp || !n || !m || !dist_out) PK_FAIL(PK_EINVAL, "pk_edit_run: NULL argument");
    if (mode != 0 && mode != 1) PK_FAIL(PK_EINVAL, "pk_edit_run: mode = %d is neither 0 (distance) nor 1 (distance, counts and ops)", (int)mode);
    if (mode == 1 && (!counts_out || !ops_out || !len_out)) PK_FAIL(PK_EINVAL, "pk_edit_run: NULL argument (mode 1 writes counts, ops and their number)");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_edit_run: batch size must be positive");
    if (B > 65535) PK_FAIL(PK_EUNSUPPORTED, "pk_edit_run: %d pairs; the engine's envelope is 65535 in a call", (int)B);
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0 || m[b] < 0) PK_FAIL(PK_EINVAL, "pk_edit_run: pair %d has a negative length (%d ref ids, %d hyp ids)", b, n[b], m[b]);
        if (n[b] > EDIT_MAX_LEN) PK_FAIL(PK_EUNSUPPORTED, "pk_edit_run: pair %d has %d ref ids; the engine's envelope is 0 ... %d", b, n[b], EDIT_MAX_LEN);
        if (m[b] > EDIT_MAX_LEN) PK_FAIL(PK_EUNSUPPORTED, "pk_edit_run: pair %d has %d hyp ids; the engine's envelope is 0 ... %d", b, m[b], EDIT_MAX_LEN);
        if ((offs_ref && offs_ref[b] < 0) || (offs_hyp && offs_hyp[b] < 0)) PK_FAIL(PK_EINVAL, "pk_edit_run: pair %d has a negative offset", b);
    }
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);

    // the table: ordered by rows per strip (one grid per value that occurs); outputs in the call's order
    std::vector<edit_pair> tab(B);
    long o_ref = 0, o_hyp = 0, o_ops = 0, gwords = 0, gcarry = 0, grev = 0;
    for (int b = 0; b < B; ++b) {
        const int N = n[b], M = m[b];
        edit_pair u{};
        u.ref_off = offs_ref ? offs_ref[b] : o_ref;
        u.hyp_off = offs_hyp ? offs_hyp[b] : o_hyp;
        o_ref += N;
        o_hyp += M;
        u.ops_off = o_ops;
        o_ops += N + M;
        u.bits_off = -1;
        if (mode == 1 && edit_words(N, M) > EDIT_LDS_WORDS) {  // 128-byte aligned per pair
            u.bits_off = gwords;
            gwords += (edit_words(N, M) + 31) / 32 * 32;
        }
        u.carry_off = gcarry;
        if (edit_strips(N) > 64) gcarry += 2L * M;
        u.rev_off = grev;
        if (mode == 1) grev += (N + M + 63) / 64 * 64;
        u.N = N;
        u.M = M;
        u.b = b;
        tab[b] = u;
    }
    std::stable_sort(tab.begin(), tab.end(), [](const edit_pair& a, const edit_pair& c) { return edit_strip_rows(a.N) < edit_strip_rows(c.N); });
    if (gwords) PK_TRY(sc->edit_bits.reserve((size_t)gwords * sizeof(u32)));
    if (gcarry) PK_TRY(sc->edit_carry.reserve((size_t)gcarry * sizeof(int)));
    if (grev) PK_TRY(sc->edit_rev.reserve((size_t)grev * sizeof(u32)));
    PK_TRY(pk_upload(ctx, sc->edit_tab, tab.data(), tab.size() * sizeof(edit_pair)));
    const edit_pair* dtab = sc->edit_tab.as<edit_pair>();

    for (int i = 0; i < B;) {
        const int R = edit_strip_rows(tab[i].N);
        int j = i;
        size_t lds = 0;
        for (; j < B && edit_strip_rows(tab[j].N) == R; ++j) {
            const size_t need = (tab[j].bits_off >= 0 ? (size_t)EDIT_LDS_WORDS : (size_t)edit_words(tab[j].N, tab[j].M)) * sizeof(u32);
            lds = std::max(lds, need);
        }
        if (mode == 1)
            PK_TRY(edit_launch_r<1>(R, ctx, j - i, lds, ref, hyp, dtab + i, dist_out, counts_out, ops_out, len_out,
                                    sc->edit_bits.as<u32>(), sc->edit_carry.as<int>(), sc->edit_rev.as<u32>()));
        else
            PK_TRY(edit_launch_r<0>(R, ctx, j - i, 0, ref, hyp, dtab + i, dist_out, nullptr, nullptr, nullptr, nullptr,
                                    sc->edit_carry.as<int>(), nullptr));
        i = j;
    }
    return PK_OK;
}
