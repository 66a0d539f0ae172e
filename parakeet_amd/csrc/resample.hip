// resample.hip -- rational-ratio resampling of ragged batches on gfx950: a generic polyphase FIR.
//
//   y[n] = sum_k table[(n * down) mod up][k] * x[floor(n * down / up) - (taps - 1) / 2 + k],   x = 0 outside 0 ... N - 1
//
// The phase table comes from the host (parakeet_amd/audio.py resample_filter: a Kaiser-windowed sinc in float64, rounded to
// fp32 once), so nothing here knows about windows or rates.  Geometry: pk_resample.h.  One workgroup owns one tile of one
// utterance: it stages the tile's input span in LDS (samples outside the utterance are zeros by a select, the packed
// buffer's neighbours are never read), then every work item walks its input samples in ascending order with one fp32 FMA
// per sample and output: A * R accumulators, per step R samples from LDS (each used for A outputs) and A coefficients from
// the table (each used for R outputs).  The device copy of the table is laid out [step][residue group][a] with the rows of
// a group shifted onto common input samples and padded with zeros; an output's own taps still arrive in ascending order,
// the padding adds 0 * x (x finite) before and after them.  Work items are dealt to the lanes so that the 32 lanes of a
// half wave start on 32 different LDS banks wherever the shape has that many.  Nothing is shared between tiles or
// utterances and the order of every sum is fixed: an utterance's output is the same bits alone, in any batch, at any
// position of the batch.
#include <vector>

#include "pk_common.h"
#include "pk_resample.h"

namespace {

struct rs_utt {
    long xoff;      // first sample of the utterance in the packed input
    long yoff;      // first output in the packed output
    long n_out;
    int n_in;
    int pad_;
};

struct rs_item {
    int xoff;       // LDS index of the item's first input sample (q = 0, step 0)
    int i0;         // tile-relative index of its first output: residue A * g, q = 0
    int g;          // residue group: the table column
    int na;         // residues of the group that exist (< A only for the last group of an odd `up`)
};

typedef float rs_f32x2 __attribute__((ext_vector_type(2)));

template <int R, int A>
__global__ __launch_bounds__(RS_THREADS) void k_resample(const float* __restrict__ x, const float* __restrict__ tab,
                                                         const rs_item* __restrict__ items, const rs_utt* __restrict__ utts,
                                                         float* __restrict__ y, int up, int down, int lead, int steps, int G,
                                                         int n_items, int CR, int span) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const rs_utt u = utts[blockIdx.y];
    const long n0 = (long)blockIdx.x * CR * up;            // the tile's first output: phase 0, input base tile * CR * down
    if (n0 >= u.n_out) return;                             // (uniform over the workgroup)
    const long m0 = (long)blockIdx.x * CR * down - lead;   // the input sample xs[0] stands for; lead = (taps - 1) / 2
    const float* xu = x + u.xoff;
    for (int s = threadIdx.x; s < span; s += RS_THREADS) {
        const long m = m0 + s;
        xs[s] = (m >= 0 && m < u.n_in) ? xu[m] : 0.f;
    }
    __syncthreads();
    float* yu = y + u.yoff + n0;
    const long left = u.n_out - n0;                        // outputs of this utterance from n0 on
    for (int it = threadIdx.x; it < n_items; it += RS_THREADS) {
        const rs_item item = items[it];
        if (item.i0 >= left) continue;                     // not even the item's first output exists
        const float* xp = xs + item.xoff;
        const float* tp = tab + item.g * A;
        float acc[A][R];
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int q = 0; q < R; ++q) acc[a][q] = 0.f;
#pragma unroll 4
        for (int j = 0; j < steps; ++j) {
            float w[A];
            if constexpr (A == 2) {
                const rs_f32x2 w2 = *reinterpret_cast<const rs_f32x2*>(tp + (long)j * G * 2);
                w[0] = w2[0];
                w[1] = w2[1];
            } else {
                w[0] = tp[(long)j * G];
            }
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float xv = xp[q * down + j];
#pragma unroll
                for (int a = 0; a < A; ++a) acc[a][q] = __builtin_fmaf(w[a], xv, acc[a][q]);
            }
        }
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int i = item.i0 + a + q * up;
                if (a < item.na && i < left) yu[i] = acc[a][q];
            }
    }
}

}  // namespace

struct pk_resample {
    pk_ctx* ctx = nullptr;
    pk_resample_cfg cfg;
    rs_plan plan;
    int n_items = 0;
    pk_dbuf d_tab, d_items, ws_utt, ws_in, ws_out;
};

static long rs_out_len(const pk_resample* h, long n_in) { return (n_in * h->cfg.up + h->cfg.down - 1) / h->cfg.down; }

extern "C" int pk_resample_create(pk_ctx* ctx, const pk_resample_cfg* cfg, const float* table, pk_resample** out) {
    if (!ctx || !cfg || !table || !out) PK_FAIL(PK_EINVAL, "pk_resample_create: NULL argument");
    *out = nullptr;
    const pk_resample_cfg& c = *cfg;
    if (c.up < 1 || c.up > RS_MAX_RATIO || c.down < 1 || c.down > RS_MAX_RATIO)
        PK_FAIL(PK_EUNSUPPORTED, "resample: up = %d, down = %d; both must be in 1 ... %d (the ratio in lowest terms)", (int)c.up,
                (int)c.down, RS_MAX_RATIO);
    if (c.taps < 1 || c.taps > RS_MAX_TAPS)
        PK_FAIL(PK_EUNSUPPORTED, "resample: %d taps per phase; the limit is 1 ... %d", (int)c.taps, RS_MAX_TAPS);
    if ((long)c.up * c.taps > RS_MAX_TABLE)
        PK_FAIL(PK_EUNSUPPORTED, "resample: a table of up * taps = %ld coefficients; the limit is %ld", (long)c.up * c.taps,
                RS_MAX_TABLE);
    PK_DEVICE(ctx->device);
    pk_resample* h = new pk_resample();
    h->ctx = ctx;
    h->cfg = c;
    h->plan = rs_make_plan(c.up, c.down, c.taps);
    const rs_plan& p = h->plan;
    // the table as the kernel walks it: [step j][group g][a]; residue r = A * g + a has phase (r * down) mod up and its tap k
    // at step k + (o_r - o_{A g}), o_r = floor(r * down / up) its input base inside a period; zeros elsewhere
    std::vector<float> t((size_t)p.steps * p.G * p.A, 0.f);
    for (int r = 0; r < c.up; ++r) {
        const int g = r / p.A, a = r % p.A;
        const int shift = (int)(((long)r * c.down) / c.up - ((long)g * p.A * c.down) / c.up);
        const float* row = table + (size_t)(((long)r * c.down) % c.up) * c.taps;
        for (int k = 0; k < c.taps; ++k) t[((size_t)(k + shift) * p.G + g) * p.A + a] = row[k];
    }
    // the work items (g, chunk), dealt to the lanes half wave by half wave: each takes one item from as many different LDS
    // banks (ds_read_b32: word address mod 32; every lane adds the same q * down + j) as still have items
    std::vector<rs_item> all, order;
    for (int ch = 0; ch < p.C; ++ch)
        for (int g = 0; g < p.G; ++g) {
            const int r0 = g * p.A;
            all.push_back({(int)(((long)r0 * c.down) / c.up) + ch * p.R * c.down, r0 + ch * p.R * c.up, g,
                           c.up - r0 < p.A ? c.up - r0 : p.A});
        }
    std::vector<std::vector<rs_item>> bank(32);
    for (auto it = all.rbegin(); it != all.rend(); ++it) bank[it->xoff & 31].push_back(*it);     // pop_back() takes them in order
    while (order.size() < all.size()) {
        int taken = 0;
        for (int pass = 0; pass < 32 && taken < 32; ++pass)       // pass 0: one from every bank; later passes fill the half wave
            for (int b = 0; b < 32 && taken < 32; ++b)
                if (!bank[b].empty()) {
                    order.push_back(bank[b].back());
                    bank[b].pop_back();
                    ++taken;
                }
        if (taken == 0) break;
    }
    h->n_items = (int)order.size();
    int s = pk_upload(ctx, h->d_tab, t.data(), t.size() * sizeof(float));
    if (s == PK_OK) s = pk_upload(ctx, h->d_items, order.data(), order.size() * sizeof(rs_item));
    if (s != PK_OK) {
        pk_resample_destroy(h);
        return s;
    }
    *out = h;
    return PK_OK;
}

extern "C" int pk_resample_out_len(pk_resample* h, int64_t n_in, int64_t* n_out) {
    if (!h || !n_out) PK_FAIL(PK_EINVAL, "pk_resample_out_len: NULL argument");
    if (n_in < 0 || n_in > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_resample_out_len: n_in must be in 0 ... 2^31 - 1");
    *n_out = rs_out_len(h, n_in);
    return PK_OK;
}

extern "C" int pk_resample_tile_samples(pk_resample* h, int32_t* tile) {
    if (!h || !tile) PK_FAIL(PK_EINVAL, "pk_resample_tile_samples: NULL argument");
    *tile = h->plan.tile;
    return PK_OK;
}

extern "C" int pk_resample_run(pk_resample* h, const float* wav, const int32_t* lens, int32_t B, float* out, int32_t flags) {
    if (!h || !wav || !lens || !out) PK_FAIL(PK_EINVAL, "pk_resample_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_resample_run: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const rs_plan& p = h->plan;
    std::vector<rs_utt> tab(B);
    long sum_in = 0, sum_out = 0, max_tiles = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "pk_resample_run: utterance %d is empty (%d samples)", b, (int)lens[b]);
        const long n_out = rs_out_len(h, lens[b]);
        tab[b] = {sum_in, sum_out, n_out, lens[b], 0};
        sum_in += lens[b];
        sum_out += n_out;
        const long tiles = (n_out + p.tile - 1) / p.tile;
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    if (max_tiles > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_resample_run: an utterance of more than 2^31 tiles");
    PK_TRY(h->ws_utt.reserve(tab.size() * sizeof(rs_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utt.p, tab.data(), tab.size() * sizeof(rs_utt), hipMemcpyHostToDevice, ctx->stream));
    const float* d_in = wav;
    float* d_out = out;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)sum_in * 4));
        PK_TRY(h->ws_out.reserve((size_t)sum_out * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, wav, (size_t)sum_in * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = h->ws_in.as<float>();
        d_out = h->ws_out.as<float>();
    }
    PK_HIP(hipStreamSynchronize(ctx->stream));             // `tab` leaves scope with this call
    const size_t lds = (size_t)p.span * sizeof(float);
    constexpr int GRID_Y = 32768;                          // utterances per launch (grid.y is a 16-bit quantity)
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        const dim3 grid((unsigned)max_tiles, (unsigned)nb);
        const rs_utt* d_utt = h->ws_utt.as<rs_utt>() + b0;
#define RS_LAUNCH(R_, A_)                                                                                                 \
    PK_LAUNCH(ctx, "resample", (k_resample<R_, A_>), grid, dim3(RS_THREADS), lds, d_in, h->d_tab.as<float>(),                \
              h->d_items.as<rs_item>(), d_utt, d_out, (int)h->cfg.up, (int)h->cfg.down, ((int)h->cfg.taps - 1) / 2, p.steps, \
              p.G, h->n_items, p.C * p.R, p.span)
        switch (p.R * 4 + p.A) {
            case 8 * 4 + 2: RS_LAUNCH(8, 2); break;
            case 4 * 4 + 2: RS_LAUNCH(4, 2); break;
            case 2 * 4 + 2: RS_LAUNCH(2, 2); break;
            case 1 * 4 + 2: RS_LAUNCH(1, 2); break;
            case 8 * 4 + 1: RS_LAUNCH(8, 1); break;
            case 4 * 4 + 1: RS_LAUNCH(4, 1); break;
            case 2 * 4 + 1: RS_LAUNCH(2, 1); break;
            default: RS_LAUNCH(1, 1); break;
        }
#undef RS_LAUNCH
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(out, d_out, (size_t)sum_out * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" void pk_resample_destroy(pk_resample* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->d_tab, &h->d_items, &h->ws_utt, &h->ws_in, &h->ws_out};
    for (auto* b : bufs) b->release();
    delete h;
}
