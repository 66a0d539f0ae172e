// seq_loss.hip -- the per-utterance sums behind the evaluator criteria of FastSpeech2, TransformerTTS and Tacotron2:
//   pk_pair_loss_run    sum |p - t| and sum (p - t)^2 of ragged pairs of fp32 rectangles (nn.L1Loss / nn.MSELoss under
//                       make_non_pad_mask, fastspeech2.py:754-781, transformer_tts.py:829-848, tacotron2.py:960-961);
//   pk_bce_logits_run   sum of the binary_cross_entropy_with_logits term under a pos_weight (transformer_tts.py:798, :849,
//                       tacotron2.py:906, :970);
//   pk_guided_attn_run  sum W * A and sum A of each utterance's attention maps under the guide
//                       W[s, t] = 1 - exp(-(t / T - s / S)^2 / (2 sigma^2))
//                       (transformer_tts.py:984-989 with s over olen, t over ilen; modules/losses.py:34-39 likewise).
//
// The convention is mel_loss.hip's: the device leaves per-utterance sums in float64, the host forms the means.  One workgroup
// per tile of one utterance; every term is formed in fp32 exactly as the reference forms it (the stop-token term in fp64) and
// enters a float64 accumulator at once (PK_SEQ_LOSS_F32_CHAIN = 0).  Lanes are combined by an xor butterfly, the four waves
// in a fixed tree, an utterance's tiles by k_seq_loss_fold in a fixed order: no atomics, nothing shared between utterances.
// The decomposition into tiles and lanes follows the utterance's own index space (never its address), so its sums are the
// same bits alone, in any batch, at any position, packed or inside a padded rectangle.
//
// Loads are 16 bytes per lane where the utterance's layout allows (contiguous rows, offsets and strides that are multiples of
// four floats, an aligned base); otherwise the same lane reads the same four entries one by one, in the same order.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_seq_loss.h"

namespace {

constexpr int VEC = PK_SEQ_LOSS_VEC;
constexpr int PAIR_ITERS = PK_SEQ_LOSS_PAIR_ITERS;
constexpr long PAIR_TILE = PK_SEQ_LOSS_PAIR_TILE;
constexpr int GR = PK_SEQ_LOSS_GUIDE_ROWS, GC = PK_SEQ_LOSS_GUIDE_COLS;
static_assert(VEC == 4, "a lane's entries are one float4");
static_assert(GR * (GC / VEC) == 256, "one lane per row and column quad of the guide tile");

struct seq_tile {
    int b, idx;   // utterance, number of the tile within it
};
struct seq_fold {
    int tile0, ntile;
};
struct pair_utt {
    long p_off, t_off;   // first entry in pred / target (floats)
    long n;              // rows * W
    int vec, pad_;
};
struct bce_utt {
    long x_off, y_off;
    long n;
};
struct guide_utt {
    long off, g_stride, s_stride;   // floats
    int G, S, T, ntt;               // maps, rows, columns, column tiles
    int vec, pad_;
};

// the workgroup's two float64 sums -> part[2 * block]
__device__ __forceinline__ void block_sum2(double a0, double a1, double* __restrict__ part) {
    __shared__ double red[8];
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a0 += __shfl_xor(a0, d);
        a1 += __shfl_xor(a1, d);
    }
    if ((tid & 63) == 0) {
        red[(tid >> 6) * 2] = a0;
        red[(tid >> 6) * 2 + 1] = a1;
    }
    __syncthreads();
    if (tid == 0) {
        part[(long)blockIdx.x * 2] = (red[0] + red[2]) + (red[4] + red[6]);
        part[(long)blockIdx.x * 2 + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

__global__ __launch_bounds__(256) void k_pair_loss_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const pair_utt* __restrict__ utt, const seq_tile* __restrict__ tile,
                                                        int W, long p_stride, long t_stride, double* __restrict__ part) {
    const int tid = threadIdx.x;
    const seq_tile tv = tile[blockIdx.x];
    const pair_utt u = utt[tv.b];
    const long e0 = (long)tv.idx * PAIR_TILE;
    double a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int it = 0; it < PAIR_ITERS; ++it) {
        const long e = e0 + ((long)it * 256 + tid) * VEC;
        if (e >= u.n) break;
        float pv[VEC], tg[VEC];
        if (u.vec && e + VEC <= u.n) {
            const float4 a = *reinterpret_cast<const float4*>(pred + u.p_off + e);
            const float4 b = *reinterpret_cast<const float4*>(target + u.t_off + e);
            pv[0] = a.x, pv[1] = a.y, pv[2] = a.z, pv[3] = a.w;
            tg[0] = b.x, tg[1] = b.y, tg[2] = b.z, tg[3] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const long ek = e + k;
                pv[k] = tg[k] = 0.f;
                if (ek < u.n) {
                    const long row = ek / W, col = ek - row * W;
                    pv[k] = pred[u.p_off + row * p_stride + col];
                    tg[k] = target[u.t_off + row * t_stride + col];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float d = pv[k] - tg[k];   // the reference's fp32 difference
            a1 += (double)fabsf(d);
            a2 += (double)d * (double)d;     // exact product
        }
    }
    block_sum2(a1, a2, part);
}

// Paddle's binary_cross_entropy_with_logits, reduction "none":
//   (1 - y) x + (1 + (pos_weight - 1) y) (log1p(exp(-|x|)) + max(-x, 0))
// in this form, which never exponentiates a positive number.  The data is one float per decoder frame: the term is evaluated
// in float64, where x + softplus(-x) keeps the digits an fp32 evaluation loses below -17.
__global__ __launch_bounds__(256) void k_bce_logits_tile(const float* __restrict__ x, const float* __restrict__ y,
                                                         const bce_utt* __restrict__ utt, const seq_tile* __restrict__ tile,
                                                         double pwm1, double* __restrict__ part) {
    const int tid = threadIdx.x;
    const seq_tile tv = tile[blockIdx.x];
    const bce_utt u = utt[tv.b];
    const long e0 = (long)tv.idx * PAIR_TILE;
    double acc = 0.0;
    for (int it = 0; it < PAIR_ITERS * VEC; ++it) {
        const long e = e0 + (long)it * 256 + tid;
        if (e >= u.n) break;
        const double xv = (double)x[u.x_off + e], yv = (double)y[u.y_off + e];
        const double sp = log1p(exp(-fabs(xv))) + fmax(-xv, 0.0);
        acc += (1.0 - yv) * xv + (1.0 + pwm1 * yv) * sp;
    }
    block_sum2(acc, 0.0, part);
}

// den = 2 sigma^2 rounded to fp32.  The guide of a lane's four columns is formed once and stays in registers while the
// utterance's G maps pass under it.
__global__ __launch_bounds__(256) void k_guided_attn_tile(const float* __restrict__ att, const guide_utt* __restrict__ utt,
                                                          const seq_tile* __restrict__ tile, float den,
                                                          double* __restrict__ part) {
    const int tid = threadIdx.x;
    const seq_tile tv = tile[blockIdx.x];
    const guide_utt u = utt[tv.b];
    const int ts = tv.idx / u.ntt, tt = tv.idx - ts * u.ntt;
    const int s = ts * GR + (tid >> 4), t0 = tt * GC + (tid & 15) * VEC;
    double wa = 0.0, sa = 0.0;
    if (s < u.S && t0 < u.T) {
        float w[VEC];
        {
            // the reference's order in fp32: two quotients, their difference, its square, the division, the exponential
#pragma clang fp contract(off)
            const float fs = (float)s / (float)u.S;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float ft = (float)(t0 + k) / (float)u.T;
                const float d = ft - fs;
                const float z = (d * d) / den;
                w[k] = 1.f - expf(-z);
            }
        }
        const int nk = min(VEC, u.T - t0);
        const float* q = att + u.off + (long)s * u.s_stride + t0;
        for (int g = 0; g < u.G; ++g, q += u.g_stride) {
            float a[VEC];
            if (u.vec && nk == VEC) {
                const float4 v = *reinterpret_cast<const float4*>(q);
                a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) a[k] = k < nk ? q[k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                wa = fma((double)w[k], (double)a[k], wa);   // exact product, one rounding in float64
                sa += (double)a[k];
            }
        }
    }
    block_sum2(wa, sa, part);
}

// One block per utterance: out[b * nv + j] = sum of its tiles' j-th numbers.  Thread t adds tiles t, t + 256, ... in ascending
// order, then a tree over the 256 threads: the order depends on the utterance alone.
__global__ __launch_bounds__(256) void k_seq_loss_fold(const double* __restrict__ part, const seq_fold* __restrict__ fold,
                                                       int nv, double* __restrict__ out) {
    __shared__ double sh[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const seq_fold f = fold[b];
    double a0 = 0.0, a1 = 0.0;
    for (int i = t; i < f.ntile; i += 256) {
        const double* p = part + (long)(f.tile0 + i) * 2;
        a0 += p[0];
        a1 += p[1];
    }
    sh[0][t] = a0;
    sh[1][t] = a1;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            sh[0][t] += sh[0][t + d];
            sh[1][t] += sh[1][t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[(long)b * nv] = sh[0][0];
        if (nv > 1) out[(long)b * nv + 1] = sh[1][0];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The tables of one call in one upload: [utt B][seq_fold B][seq_tile n_tile], each part 16-byte aligned.
template <class U>
struct seq_tables {
    std::vector<char> blob;
    size_t off_fold = 0, off_tile = 0;
    U* utt = nullptr;
    seq_fold* fold = nullptr;
    seq_tile* tile = nullptr;
    void layout(int B, long n_tile) {
        off_fold = ((size_t)B * sizeof(U) + 15) & ~(size_t)15;
        off_tile = (off_fold + (size_t)B * sizeof(seq_fold) + 15) & ~(size_t)15;
        blob.assign(off_tile + (size_t)(n_tile + 1) * sizeof(seq_tile), 0);
        utt = reinterpret_cast<U*>(blob.data());
        fold = reinterpret_cast<seq_fold*>(blob.data() + off_fold);
        tile = reinterpret_cast<seq_tile*>(blob.data() + off_tile);
    }
};

// Stage host operands of a PK_HOST_IO call behind the (B, nv) sums in sc->seq_io; returns the device pointers.
int stage_host(pk_ctx* ctx, pk_ctx_scratch* sc, size_t out_bytes, const float* a, size_t na, const float* b, size_t nb,
               double** d_out, const float** d_a, const float** d_b) {
    const size_t o = (out_bytes + 15) & ~(size_t)15, oa = (na * 4 + 15) & ~(size_t)15;
    PK_TRY(sc->seq_io.reserve(o + oa + nb * 4 + 16));
    char* base = sc->seq_io.as<char>();
    *d_out = reinterpret_cast<double*>(base);
    float* da = reinterpret_cast<float*>(base + o);
    float* db = reinterpret_cast<float*>(base + o + oa);
    if (na) PK_HIP(hipMemcpyAsync(da, a, na * 4, hipMemcpyHostToDevice, ctx->stream));
    if (nb) PK_HIP(hipMemcpyAsync(db, b, nb * 4, hipMemcpyHostToDevice, ctx->stream));
    *d_a = da;
    if (d_b) *d_b = db;
    return PK_OK;
}

}  // namespace

extern "C" int pk_pair_loss_run(pk_ctx* ctx, const float* pred, const float* target, const int64_t* pred_offs,
                                const int64_t* target_offs, int64_t pred_stride, int64_t target_stride, const int32_t* rows,
                                int32_t B, int32_t W, double* sums_out, int32_t flags) {
    if (!ctx || !pred || !target || !rows || !sums_out) PK_FAIL(PK_EINVAL, "pk_pair_loss_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pair_loss_run: batch size must be positive");
    if (W < 1) PK_FAIL(PK_EINVAL, "pk_pair_loss_run: width %d", W);
    if (W > PK_SEQ_LOSS_MAX_W) PK_FAIL(PK_EUNSUPPORTED, "pk_pair_loss_run: width %d exceeds %d", W, PK_SEQ_LOSS_MAX_W);
    const long ps = pred_stride ? pred_stride : W, tst = target_stride ? target_stride : W;
    if (ps < W || tst < W) PK_FAIL(PK_EINVAL, "pk_pair_loss_run: row strides %ld, %ld below the width %d", ps, tst, W);
    if ((!pred_offs && ps != W) || (!target_offs && tst != W))
        PK_FAIL(PK_EINVAL, "pk_pair_loss_run: a row stride other than W needs the operand's offsets");
    long n_tile = 0;
    for (int b = 0; b < B; ++b) {
        if (rows[b] < 0) PK_FAIL(PK_EINVAL, "pk_pair_loss_run: pair %d has %d rows", b, rows[b]);
        if ((pred_offs && pred_offs[b] < 0) || (target_offs && target_offs[b] < 0))
            PK_FAIL(PK_EINVAL, "pk_pair_loss_run: pair %d has a negative offset", b);
        n_tile += ((long)rows[b] * W + PAIR_TILE - 1) / PAIR_TILE;
    }
    if (n_tile > (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_pair_loss_run: %ld tiles", n_tile);
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    seq_tables<pair_utt> tb;
    tb.layout(B, n_tile);
    const bool host = (flags & PK_HOST_IO) != 0;
    // a staged operand starts on a 16-byte boundary, as a caller's device pointer may or may not
    const bool base_ok = host || (aligned16(pred) && aligned16(target));
    long po = 0, to = 0, r = 0, p_ext = 0, t_ext = 0;
    for (int b = 0; b < B; ++b) {
        const long n = (long)rows[b] * W, nt = (n + PAIR_TILE - 1) / PAIR_TILE;
        const long pb = pred_offs ? pred_offs[b] : po, tb_ = target_offs ? target_offs[b] : to;
        const int vec = base_ok && ps == W && tst == W && pb % VEC == 0 && tb_ % VEC == 0;
        tb.utt[b] = pair_utt{pb, tb_, n, vec, 0};
        tb.fold[b] = seq_fold{(int)r, (int)nt};
        for (long i = 0; i < nt; ++i) tb.tile[r++] = seq_tile{b, (int)i};
        if (rows[b] > 0) {
            p_ext = std::max(p_ext, pb + (rows[b] - 1) * ps + W);
            t_ext = std::max(t_ext, tb_ + (rows[b] - 1) * tst + W);
        }
        po += n;
        to += n;
    }
    PK_TRY(pk_upload(ctx, sc->seq_tab, tb.blob.data(), tb.blob.size()));
    const char* dt = sc->seq_tab.as<char>();
    PK_TRY(sc->seq_part.reserve((size_t)(n_tile + 1) * 2 * sizeof(double)));
    const float *d_pred = pred, *d_target = target;
    double* d_out = sums_out;
    const size_t out_bytes = (size_t)B * 2 * sizeof(double);
    if (host) PK_TRY(stage_host(ctx, sc, out_bytes, pred, (size_t)p_ext, target, (size_t)t_ext, &d_out, &d_pred, &d_target));
    if (n_tile > 0)
        PK_LAUNCH(ctx, "pair_loss_tile", k_pair_loss_tile, dim3((unsigned)n_tile), dim3(256), 0, d_pred, d_target,
                  reinterpret_cast<const pair_utt*>(dt), reinterpret_cast<const seq_tile*>(dt + tb.off_tile), W, ps, tst,
                  sc->seq_part.as<double>());
    PK_LAUNCH(ctx, "seq_loss_fold", k_seq_loss_fold, dim3(B), dim3(256), 0, sc->seq_part.as<double>(),
              reinterpret_cast<const seq_fold*>(dt + tb.off_fold), 2, d_out);
    if (host) {
        PK_HIP(hipMemcpyAsync(sums_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_bce_logits_run(pk_ctx* ctx, const float* logits, const float* labels, const int64_t* logit_offs,
                                 const int64_t* label_offs, const int32_t* lens, int32_t B, float pos_weight,
                                 double* sums_out, int32_t flags) {
    if (!ctx || !logits || !labels || !lens || !sums_out) PK_FAIL(PK_EINVAL, "pk_bce_logits_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_bce_logits_run: batch size must be positive");
    if (!(pos_weight >= 0.f) || std::isinf(pos_weight))
        PK_FAIL(PK_EINVAL, "pk_bce_logits_run: pos_weight %g must be finite and not negative", (double)pos_weight);
    long n_tile = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0) PK_FAIL(PK_EINVAL, "pk_bce_logits_run: row %d has %d entries", b, lens[b]);
        if ((logit_offs && logit_offs[b] < 0) || (label_offs && label_offs[b] < 0))
            PK_FAIL(PK_EINVAL, "pk_bce_logits_run: row %d has a negative offset", b);
        n_tile += (lens[b] + PAIR_TILE - 1) / PAIR_TILE;
    }
    if (n_tile > (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_bce_logits_run: %ld tiles", n_tile);
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    seq_tables<bce_utt> tb;
    tb.layout(B, n_tile);
    long xo = 0, yo = 0, r = 0, x_ext = 0, y_ext = 0;
    for (int b = 0; b < B; ++b) {
        const long n = lens[b], nt = (n + PAIR_TILE - 1) / PAIR_TILE;
        const long xb = logit_offs ? logit_offs[b] : xo, yb = label_offs ? label_offs[b] : yo;
        tb.utt[b] = bce_utt{xb, yb, n};
        tb.fold[b] = seq_fold{(int)r, (int)nt};
        for (long i = 0; i < nt; ++i) tb.tile[r++] = seq_tile{b, (int)i};
        if (n > 0) {
            x_ext = std::max(x_ext, xb + n);
            y_ext = std::max(y_ext, yb + n);
        }
        xo += n;
        yo += n;
    }
    PK_TRY(pk_upload(ctx, sc->seq_tab, tb.blob.data(), tb.blob.size()));
    const char* dt = sc->seq_tab.as<char>();
    PK_TRY(sc->seq_part.reserve((size_t)(n_tile + 1) * 2 * sizeof(double)));
    const float *d_x = logits, *d_y = labels;
    double* d_out = sums_out;
    const size_t out_bytes = (size_t)B * sizeof(double);
    const bool host = (flags & PK_HOST_IO) != 0;
    if (host) PK_TRY(stage_host(ctx, sc, out_bytes, logits, (size_t)x_ext, labels, (size_t)y_ext, &d_out, &d_x, &d_y));
    if (n_tile > 0)
        PK_LAUNCH(ctx, "bce_logits_tile", k_bce_logits_tile, dim3((unsigned)n_tile), dim3(256), 0, d_x, d_y,
                  reinterpret_cast<const bce_utt*>(dt), reinterpret_cast<const seq_tile*>(dt + tb.off_tile),
                  (double)pos_weight - 1.0, sc->seq_part.as<double>());
    PK_LAUNCH(ctx, "seq_loss_fold", k_seq_loss_fold, dim3(B), dim3(256), 0, sc->seq_part.as<double>(),
              reinterpret_cast<const seq_fold*>(dt + tb.off_fold), 1, d_out);
    if (host) {
        PK_HIP(hipMemcpyAsync(sums_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_guided_attn_run(pk_ctx* ctx, const float* att, const int64_t* offs, int64_t map_stride, int64_t row_stride,
                                  const int32_t* maps, const int32_t* rows, const int32_t* cols, int32_t B, double sigma,
                                  double* sums_out, int32_t flags) {
    if (!ctx || !att || !maps || !rows || !cols || !sums_out) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: batch size must be positive");
    if (!(sigma > 0.0) || std::isinf(sigma)) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: sigma %g must be positive and finite", sigma);
    const float den = (float)(2.0 * sigma * sigma);   // the one rounding of 2 sigma^2
    if (!(den > 0.f) || std::isinf(den)) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: 2 sigma^2 = %g is not an fp32 number", (double)den);
    if (map_stride < 0 || row_stride < 0) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: negative stride");
    if (!offs && (map_stride || row_stride))
        PK_FAIL(PK_EINVAL, "pk_guided_attn_run: strides need the utterances' offsets (NULL offsets mean contiguous maps)");
    long n_tile = 0;
    for (int b = 0; b < B; ++b) {
        if (maps[b] < 1 || rows[b] < 1 || cols[b] < 1)
            PK_FAIL(PK_EINVAL, "pk_guided_attn_run: utterance %d: %d maps of %d x %d", b, maps[b], rows[b], cols[b]);
        if (maps[b] > PK_SEQ_LOSS_MAX_MAPS)
            PK_FAIL(PK_EUNSUPPORTED, "pk_guided_attn_run: utterance %d: %d maps exceed %d", b, maps[b], PK_SEQ_LOSS_MAX_MAPS);
        const long ss = row_stride ? row_stride : cols[b];
        if (ss < cols[b]) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: utterance %d: row stride %ld below its %d columns", b, ss, cols[b]);
        if (map_stride && map_stride < (rows[b] - 1) * ss + cols[b])
            PK_FAIL(PK_EINVAL, "pk_guided_attn_run: utterance %d: map stride %ld below one map", b, (long)map_stride);
        if (offs && offs[b] < 0) PK_FAIL(PK_EINVAL, "pk_guided_attn_run: utterance %d has a negative offset", b);
        n_tile += (long)((rows[b] + GR - 1) / GR) * ((cols[b] + GC - 1) / GC);
    }
    if (n_tile > (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_guided_attn_run: %ld tiles", n_tile);
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    seq_tables<guide_utt> tb;
    tb.layout(B, n_tile);
    const bool host = (flags & PK_HOST_IO) != 0;
    const bool base_ok = host || aligned16(att);
    long o = 0, r = 0, ext = 0;
    for (int b = 0; b < B; ++b) {
        const long ss = row_stride ? row_stride : cols[b], gs = map_stride ? map_stride : rows[b] * ss;
        const long ob = offs ? offs[b] : o;
        const int ntt = (cols[b] + GC - 1) / GC;
        const long nt = (long)((rows[b] + GR - 1) / GR) * ntt;
        const int vec = base_ok && ob % VEC == 0 && ss % VEC == 0 && gs % VEC == 0;
        tb.utt[b] = guide_utt{ob, gs, ss, maps[b], rows[b], cols[b], ntt, vec, 0};
        tb.fold[b] = seq_fold{(int)r, (int)nt};
        for (long i = 0; i < nt; ++i) tb.tile[r++] = seq_tile{b, (int)i};
        ext = std::max(ext, ob + (maps[b] - 1) * gs + (rows[b] - 1) * ss + cols[b]);
        o += maps[b] * gs;
    }
    PK_TRY(pk_upload(ctx, sc->seq_tab, tb.blob.data(), tb.blob.size()));
    const char* dt = sc->seq_tab.as<char>();
    PK_TRY(sc->seq_part.reserve((size_t)(n_tile + 1) * 2 * sizeof(double)));
    const float* d_att = att;
    double* d_out = sums_out;
    const size_t out_bytes = (size_t)B * 2 * sizeof(double);
    if (host) PK_TRY(stage_host(ctx, sc, out_bytes, att, (size_t)ext, nullptr, 0, &d_out, &d_att, nullptr));
    PK_LAUNCH(ctx, "guided_attn_tile", k_guided_attn_tile, dim3((unsigned)n_tile), dim3(256), 0, d_att,
              reinterpret_cast<const guide_utt*>(dt), reinterpret_cast<const seq_tile*>(dt + tb.off_tile), den,
              sc->seq_part.as<double>());
    PK_LAUNCH(ctx, "seq_loss_fold", k_seq_loss_fold, dim3(B), dim3(256), 0, sc->seq_part.as<double>(),
              reinterpret_cast<const seq_fold*>(dt + tb.off_fold), 2, d_out);
    if (host) {
        PK_HIP(hipMemcpyAsync(sums_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}
