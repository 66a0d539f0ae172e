// mel_loss.hip -- masked L1 and SSIM of pairs of mel spectrograms in one pass over both images: the two spectrogram terms
// of the SpeedySpeech evaluator (speedyspeech_updater.py:119-140) and the reference's ssim as a metric of its own.
//
// Reference: parakeet/modules/ssim.py:21-61 with channel = 1 (gaussian window of sigma 1.5, zero padding of window_size / 2 on
// all four sides, C1 = 0.01^2, C2 = 0.03^2), parakeet/modules/losses.py:60-100 (weighted_mean, masked_l1_loss) under a frame
// mask of prefix form: rows at or past lens[b] read as zero in both images (decoded * spec_mask, target * spec_mask), the
// absolute error counts on the rows below lens[b] only.
//
// k_mel_loss_tile: one workgroup per tile of PK_MEL_LOSS_ROWS rows x cols columns of one utterance's map.  It stages the tile
// of both images with a halo of window_size / 2 rows and columns in LDS, filters the five moments x, y, x^2, y^2, xy
// horizontally from LDS into LDS and vertically from there (the 2-D window is the outer product of the 1-D one), evaluates the
// map and leaves one fp32 pair per tile: sum |p - t| of its valid entries, sum (map - 1) of its map entries.  k_mel_loss_fold
// adds an utterance's pairs in fixed order in fp64 (as k_stftd_fold) and puts the number of map entries back.  No atomics,
// nothing shared between utterances: a pair's sums are the same bits alone and in any batch.
//
// Arithmetic of the variances.  E[x^2] - mu^2 in fp32 loses what the mean takes: on raw log-mels (mean -6, deviation 2) x^2 is
// 40 where the variance is 4.  The moments are therefore taken of x - c and y - c, c being the mean of the target over the
// staged tile, the zeros of the padding and of the masked rows included (one constant per tile: what the tile's windows hold
// on average; exactly 0 for a tile no valid row reaches).  The zeros shift with the rest (they become -c), so with S = the sum
// of the 2-D window
//     mu_x        = m_x + c S
//     sigma_x^2   = (q_x  - m_x^2)   + (1 - S) (2 c m_x + c^2 S)
//     sigma_xy    = (q_xy - m_x m_y) + (1 - S) (c (m_x + m_y) + c^2 S)
// hold exactly (m, q: the windowed moments of the shifted images).  S differs from 1 by the rounding of the fp32 window; the
// terms in (1 - S) keep the result that of the reference's window, not of a normalised one.
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_mel_loss.h"

namespace {

struct mel_utt {
    long in_off;    // first row of the pair in pred / target
    long map_off;   // first row of its map in ssim_map_out
    int len, plen;  // valid rows, map rows
    int tile0, ntile;   // its tiles in the partial array
};

struct mel_rowtile {
    int b, t0;
};

constexpr int TR = PK_MEL_LOSS_ROWS;

__global__ __launch_bounds__(256) void k_mel_loss_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const mel_utt* __restrict__ utt, const mel_rowtile* __restrict__ rtile,
                                                       const float* __restrict__ win, int W, int cols, int ntw, int halo,
                                                       float S, float oms, float* __restrict__ part,
                                                       float* __restrict__ map_out) {
    extern __shared__ float smem[];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ws = 2 * halo + 1;
    const int rt = blockIdx.x / ntw, tw = blockIdx.x - rt * ntw;
    const mel_rowtile rtv = rtile[rt];
    const mel_utt u = utt[rtv.b];
    const int t0 = rtv.t0, c0 = tw * cols, ncol = min(cols, W - c0);
    const int SR = TR + 2 * halo, SC = cols + 2 * halo;
    float* sx = smem;
    float* sy = sx + SR * SC;
    float* hm = sy + SR * SC;
    float* sw = hm + 5 * SR * cols;
    if (tid < ws) sw[tid] = win[tid];
    float l1 = 0.f, tsum = 0.f;
    for (int idx = tid; idx < SR * SC; idx += 256) {
        const int sr = idx / SC, sc = idx - sr * SC;
        const int gr = t0 - halo + sr, gc = c0 - halo + sc;
        float p = 0.f, t = 0.f;
        if (gr >= 0 && gr < u.len && gc >= 0 && gc < W) {
            const long o = (u.in_off + gr) * W + gc;
            p = pred[o];
            t = target[o];
            if (sr >= halo && sr < halo + TR && sc >= halo && sc < halo + ncol) l1 += fabsf(p - t);
        }
        sx[idx] = p;
        sy[idx] = t;
        tsum += t;
    }
    // the tile's centre: the mean of the staged target, zeros of the padding and of the masked rows included
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) tsum += __shfl_xor(tsum, d);
    if (lane == 0) red[tid >> 6] = tsum;
    __syncthreads();
    const float c = ((red[0] + red[1]) + (red[2] + red[3])) / (float)(SR * SC);
    for (int idx = tid; idx < SR * SC; idx += 256) {
        sx[idx] -= c;
        sy[idx] -= c;
    }
    __syncthreads();
    const int plane = SR * cols;
    for (int idx = tid; idx < plane; idx += 256) {
        const int sr = idx / cols, j = idx - sr * cols;
        const float* px = sx + sr * SC + j;
        const float* py = sy + sr * SC + j;
        float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
        for (int k = 0; k < ws; ++k) {
            const float a = px[k], b = py[k];
            const float wa = sw[k] * a, wb = sw[k] * b;
            m1 += wa;
            m2 += wb;
            q1 = fmaf(wa, a, q1);
            q2 = fmaf(wb, b, q2);
            q12 = fmaf(wa, b, q12);
        }
        hm[idx] = m1;
        hm[plane + idx] = m2;
        hm[2 * plane + idx] = q1;
        hm[3 * plane + idx] = q2;
        hm[4 * plane + idx] = q12;
    }
    __syncthreads();
    float sm = 0.f;
    for (int idx = tid; idx < TR * cols; idx += 256) {
        const int i = idx / cols, j = idx - i * cols;
        const int t = t0 + i;
        if (t < u.plen && j < ncol) {
            // no contraction in the map's evaluation: where both images are equal in a window (the rows no valid row reaches:
            // both are -c) the two factors of the numerator are the bits of the two of the denominator, the map is exactly 1
#pragma clang fp contract(off)
            const float* p = hm + i * cols + j;
            float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
            for (int k = 0; k < ws; ++k) {
                const float w = sw[k];
                const float* q = p + k * cols;
                m1 = fmaf(w, q[0], m1);
                m2 = fmaf(w, q[plane], m2);
                q1 = fmaf(w, q[2 * plane], q1);
                q2 = fmaf(w, q[3 * plane], q2);
                q12 = fmaf(w, q[4 * plane], q12);
            }
            const float ccs = c * c * S;
            const float mu1 = fmaf(c, S, m1), mu2 = fmaf(c, S, m2);
            const float s1 = (q1 - m1 * m1) + oms * (2.f * c * m1 + ccs);
            const float s2 = (q2 - m2 * m2) + oms * (2.f * c * m2 + ccs);
            const float s12 = (q12 - m1 * m2) + oms * (c * (m1 + m2) + ccs);
            const float C1 = 1e-4f, C2 = 9e-4f;
            const float v = ((2.f * mu1 * mu2 + C1) * (2.f * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
            if (map_out) map_out[(u.map_off + t) * W + c0 + j] = v;
            sm += v - 1.f;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        l1 += __shfl_xor(l1, d);
        sm += __shfl_xor(sm, d);
    }
    if (lane == 0) {
        red[(tid >> 6) * 2] = l1;
        red[(tid >> 6) * 2 + 1] = sm;
    }
    __syncthreads();
    if (tid == 0) {
        part[(long)blockIdx.x * 2] = (red[0] + red[2]) + (red[4] + red[6]);
        part[(long)blockIdx.x * 2 + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

// One block per utterance: out[b] = (sum of its tiles' first numbers, sum of the second ones + its map entries).  Thread t adds
// tiles t, t + 256, ... in ascending order, then a tree over the 256 threads: the order depends on the utterance alone.
__global__ __launch_bounds__(256) void k_mel_loss_fold(const float* __restrict__ part, const mel_utt* __restrict__ utt, int W,
                                                       double* __restrict__ out) {
    __shared__ double sh[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const mel_utt u = utt[b];
    double a0 = 0.0, a1 = 0.0;
    for (int i = t; i < u.ntile; i += 256) {
        const float* p = part + (long)(u.tile0 + i) * 2;
        a0 += (double)p[0];
        a1 += (double)p[1];
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
        out[(long)b * 2] = sh[0][0];
        out[(long)b * 2 + 1] = sh[1][0] + (double)u.plen * (double)W;
    }
}

}  // namespace

// The reference's 1-D window (ssim.py:21-26): exp in double, rounded to fp32, divided in fp32 by the fp32 sum.  The sum is the
// correctly rounded one (formed in double): it equals the sum a pairwise or vectorised fp32 reduction gives for the window
// sizes in use (1, 3, 11), where a strictly sequential fp32 sum is one unit off at 11.
static void mel_loss_window(int ws, std::vector<float>& w, double& S) {
    w.resize(ws);
    double sum = 0.0;
    for (int k = 0; k < ws; ++k) {
        const int d = k - ws / 2;
        w[k] = (float)std::exp(-(double)(d * d) / (2.0 * 1.5 * 1.5));
        sum += (double)w[k];
    }
    const float fsum = (float)sum;
    double s1 = 0.0;
    for (int k = 0; k < ws; ++k) {
        w[k] = w[k] / fsum;
        s1 += (double)w[k];
    }
    S = s1 * s1;
}

extern "C" int pk_mel_loss_run(pk_ctx* ctx, const float* pred, const float* target, const int32_t* lens,
                               const int32_t* padded_lens, int32_t B, int32_t W, int32_t window_size, double* sums_out,
                               float* ssim_map_out, int32_t flags) {
    if (!ctx || !pred || !target || !lens || !sums_out) PK_FAIL(PK_EINVAL, "pk_mel_loss_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_mel_loss_run: batch size must be positive");
    if (W < 1) PK_FAIL(PK_EINVAL, "pk_mel_loss_run: width %d", W);
    if (W > PK_MEL_LOSS_MAX_W) PK_FAIL(PK_EUNSUPPORTED, "pk_mel_loss_run: width %d exceeds %d", W, PK_MEL_LOSS_MAX_W);
    if (window_size < 1 || window_size % 2 == 0)
        PK_FAIL(PK_EINVAL, "pk_mel_loss_run: window_size %d must be odd and at least 1 (an even window changes the size of the "
                           "reference's map)", window_size);
    if (window_size > PK_MEL_LOSS_MAX_WINDOW)
        PK_FAIL(PK_EUNSUPPORTED, "pk_mel_loss_run: window_size %d exceeds %d", window_size, PK_MEL_LOSS_MAX_WINDOW);
    const int halo = window_size / 2;
    long sum_len = 0, sum_plen = 0, n_rt = 0;
    for (int b = 0; b < B; ++b) {
        const int pl = padded_lens ? padded_lens[b] : lens[b];
        if (lens[b] < 0) PK_FAIL(PK_EINVAL, "pk_mel_loss_run: pair %d has %d rows", b, lens[b]);
        if (pl < lens[b]) PK_FAIL(PK_EINVAL, "pk_mel_loss_run: pair %d: padded_lens %d is below lens %d", b, pl, lens[b]);
        sum_len += lens[b];
        sum_plen += pl;
        n_rt += (pl + TR - 1) / TR;
    }
    // the widest column tile the LDS budget admits, then equal tiles
    int max_cols = PK_MEL_LOSS_MAX_COLS;
    while (max_cols > 1 && pk_mel_loss_lds_floats(max_cols, halo) * 4 > PK_MEL_LOSS_LDS_BUDGET) --max_cols;
    const int ntw = (W + max_cols - 1) / max_cols, cols = (W + ntw - 1) / ntw;
    if (n_rt * ntw > (1L << 30)) PK_FAIL(PK_EUNSUPPORTED, "pk_mel_loss_run: %ld tiles", n_rt * ntw);
    PK_DEVICE(ctx->device);
    pk_ctx_scratch* sc = pk_ctx_get_scratch(ctx);
    // one blob: [mel_utt B][mel_rowtile n_rt][window]
    const size_t off_rt = (size_t)B * sizeof(mel_utt), off_win = off_rt + (size_t)n_rt * sizeof(mel_rowtile);
    std::vector<char> blob(off_win + (size_t)window_size * sizeof(float));
    mel_utt* hu = reinterpret_cast<mel_utt*>(blob.data());
    mel_rowtile* hr = reinterpret_cast<mel_rowtile*>(blob.data() + off_rt);
    {
        long io = 0, mo = 0;
        int r = 0;
        for (int b = 0; b < B; ++b) {
            const int pl = padded_lens ? padded_lens[b] : lens[b];
            const int nr = (pl + TR - 1) / TR;
            hu[b] = mel_utt{io, mo, lens[b], pl, r * ntw, nr * ntw};
            for (int i = 0; i < nr; ++i) hr[r++] = mel_rowtile{b, i * TR};
            io += lens[b];
            mo += pl;
        }
    }
    std::vector<float> w;
    double S;
    mel_loss_window(window_size, w, S);
    memcpy(blob.data() + off_win, w.data(), (size_t)window_size * sizeof(float));
    PK_TRY(pk_upload(ctx, sc->mel_tab, blob.data(), blob.size()));
    const mel_utt* d_utt = sc->mel_tab.as<mel_utt>();
    const mel_rowtile* d_rt = reinterpret_cast<const mel_rowtile*>(sc->mel_tab.as<char>() + off_rt);
    const float* d_win = reinterpret_cast<const float*>(sc->mel_tab.as<char>() + off_win);
    PK_TRY(sc->mel_part.reserve((size_t)(n_rt * ntw + 1) * 2 * sizeof(float)));
    const float *d_pred = pred, *d_target = target;
    double* d_out = sums_out;
    float* d_map = ssim_map_out;
    const size_t in_bytes = (size_t)sum_len * W * 4, map_bytes = (size_t)sum_plen * W * 4, out_bytes = (size_t)B * 2 * sizeof(double);
    if (flags & PK_HOST_IO) {
        // [sums B x 2 double][pred][target][map]
        PK_TRY(sc->mel_io.reserve(out_bytes + 2 * in_bytes + (ssim_map_out ? map_bytes : 0) + 16));
        char* base = sc->mel_io.as<char>();
        d_out = reinterpret_cast<double*>(base);
        float* dp = reinterpret_cast<float*>(base + out_bytes);
        float* dt = dp + (size_t)sum_len * W;
        if (in_bytes) {
            PK_HIP(hipMemcpyAsync(dp, pred, in_bytes, hipMemcpyHostToDevice, ctx->stream));
            PK_HIP(hipMemcpyAsync(dt, target, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        d_pred = dp;
        d_target = dt;
        if (ssim_map_out) d_map = dt + (size_t)sum_len * W;
    }
    if (n_rt > 0) {
        const size_t lds = (size_t)pk_mel_loss_lds_floats(cols, halo) * 4;
        PK_LAUNCH(ctx, "mel_loss_tile", k_mel_loss_tile, dim3((unsigned)(n_rt * ntw)), dim3(256), lds, d_pred, d_target, d_utt,
                  d_rt, d_win, W, cols, ntw, halo, (float)S, (float)(1.0 - S), sc->mel_part.as<float>(), d_map);
    }
    PK_LAUNCH(ctx, "mel_loss_fold", k_mel_loss_fold, dim3(B), dim3(256), 0, sc->mel_part.as<float>(), d_utt, W, d_out);
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(sums_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (ssim_map_out && map_bytes) PK_HIP(hipMemcpyAsync(ssim_map_out, d_map, map_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}
