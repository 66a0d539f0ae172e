// spk.hip -- the GE2E speaker encoder (parakeet/models/lstm_speaker_encoder.py LSTMSpeakerEncoder :24-53) on gfx950:
// kernels + pk_spk_* entry points.
//
// embed_sequences (:40-48): nn.LSTM(n_mels, H, num_layers) over a batch of P partial utterances of T frames, h[-1] of the
// last layer -> relu(linear) -> F.normalize; with reduce (embed_utterance, :50-53) the mean of an utterance's partials,
// normalised again.
//
// Per layer:
//   XG = X . W_ih^T + (b_ih + b_hh) for every (partial, step) row: ONE launch of the dense GEMM (pk_fft_run_dense; layer 0
//   reads the mel frames zero-padded to a multiple of 32 channels, so that the split-fp16 GEMM takes any n_mels; above
//   SPK_GEMM_MAX_IN channels k_spk_proj_wide sums layer 0 in fp64 instead).
//   k_spk_lstm_rec: one workgroup owns a tile of SPK_M = 32 partials and walks all T steps; no communication between
//   workgroups.  Per step the tile's 32 x 4H gate block h(t-1) . W_hh^T runs on the matrix cores, W_hh^T streamed from L2
//   in the MFMA operand layout packed at finalize.  Wave w owns the 32-unit blocks ub = w, w + 8, ...: it accumulates the
//   FOUR gate tiles i | f | g | o of those units (columns q H + 32 ub .. + 31), so the cell (c, h) finishes in registers;
//   c stays in registers for the whole sequence, h(t) goes to LDS as the next step's A operand (and to the next layer's
//   GEMM input; the last layer keeps h(T) only).
//   Math: PK_GEMM_MATH_F16X3 (default) = the engine's 3-term split-fp16 on v_mfma_f32_32x32x16_f16 (pk_split.h);
//   W_hh carries one exponent per tensor, h one per ROW (partial): |h(t)| < 1 for t >= 1 (o * tanh(c)) takes the fixed
//   2^14, the caller's h0 the row's own block maximum -- a partial's result never depends on the batch it rides in.
//   PK_GEMM_MATH_F32 = exact fp32 on v_mfma_f32_32x32x2f32.
// k_spk_head: relu(h(T) . W + b), normalise; optionally the per-utterance mean of the partials and a second normalise.
//
// pk_spk_ge2e: the GE2E similarity matrix and softmax loss over resident embeddings (similarity_matrix :55-104, loss
// :122-134) -- kernels in spk_loss.hip; similarity_weight / similarity_bias ([1] each, 10 and -5 unless set) live here.
//
// LSTM semantics [paddle-semantics, from Paddle's API documentation]: gate order i, f, g, o along the 4H axis, zero
// initial states unless given, c' = sigmoid(f) c + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c').
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pk_fft.h"
#include "pk_mfma.h"
#include "pk_split.h"
#include "pk_spk_loss.h"

namespace {
typedef pk_fft_dense Dense;

constexpr int SPK_M = 32;          // partials per workgroup (one MFMA row block)
constexpr int SPK_WAVES = 8;
constexpr int SPK_MAX_H = 512;
constexpr int SPK_GEMM_MAX_IN = 512;   // layer 0 above this many mel channels: k_spk_proj_wide instead of the tile GEMM
constexpr int SPK_WIDE_ROWS = 8;

struct RecArgs {
    const float* xg;      // [P * T][4H]: x W_ih^T + b_ih + b_hh, row p * T + t
    const void* w;        // W_hh^T packed at pk_spk_finalize (F32: floats, F16X3: halves)
    int kw;               // F16X3: exponent folded into the packed weights
    const float* h0;      // [P][H] or NULL (zeros)
    const float* c0;      // [P][H] or NULL
    float* hseq;          // [P * T][H]: h(t) of every step, or NULL
    float* hlast;         // [P][H]: h(T), or NULL
    int P, T, H;
};

// LDS: h(t-1) as A operands, 32 rows.  F32: float hs[k][32], row slot swizzled by k (conflict-free column writes);
// F16X3: f16x8 blocks [part hi | lo][k / 8][32 rows], row slot swizzled by k / 8.  Both H * 128 bytes, then 32 ints.
template <int MATH, int UBW>   // UBW: 32-unit blocks per wave (H <= 256: 1)
__global__ __launch_bounds__(SPK_WAVES * 64) void k_spk_lstm_rec(RecArgs a) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hi = lane >> 5;
    const int H = a.H, G = 4 * H, T = a.T, nub = H / 32, p0 = blockIdx.x * SPK_M;
    const long P = a.P;
    constexpr bool SPLIT = MATH == PK_GEMM_MATH_F16X3;
    _Float16* hb = reinterpret_cast<_Float16*>(sm);          // F16X3 view
    int* rexp = reinterpret_cast<int*>(sm + (long)H * 32);    // [32]: the rows' exponents of the t = 0 operand
    const long part_halves = (long)H * 32;                     // halves of one part (hi or lo)

    // ---- t = 0 operand: h0 (row exponent from the row's maximum) or zeros; c0 into registers
    {
        // 16 threads per row: the row's maximum by a 16-lane reduction, then each writes its share of the row
        const int row = tid >> 4, sub = tid & 15;
        const bool valid = p0 + row < P && a.h0 != nullptr;
        const float* src = a.h0 + (long)(p0 + row) * H;
        float m = 0.f;
        if (valid)
            for (int k = sub; k < H; k += 16) m = fmaxf(m, fabsf(src[k]));
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const int kr = a.h0 ? blk_scale_exp(__float_as_uint(m)) : PK_UNIT_EXP;
        const float s = pow2f(kr);
        for (int k = sub; k < H; k += 16) {
            const float v = valid ? src[k] : 0.f;
            if constexpr (SPLIT) {
                const int kb = k >> 3;
                const long o = ((long)kb * 32 + (row ^ (kb & 31))) * 8 + (k & 7);
                const _Float16 vh = (_Float16)(v * s);
                hb[o] = vh;
                hb[part_halves + o] = (_Float16)(v * s - (float)vh);
            } else {
                sm[(long)k * 32 + (row ^ (k & 31))] = v;
            }
        }
        if (sub == 0) rexp[row] = kr;
    }
    __syncthreads();
    float cst[UBW][16], hnew[UBW][16];
#pragma unroll
    for (int s = 0; s < UBW; ++s) {
        const int ub = wave + s * SPK_WAVES;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long p = p0 + mfma_row(r, hi);
            cst[s][r] = (ub < nub && a.c0 && p < P) ? a.c0[p * H + ub * 32 + j] : 0.f;
            hnew[s][r] = 0.f;
        }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int s = 0; s < UBW; ++s) {
            const int ub = wave + s * SPK_WAVES;
            if (ub >= nub) break;   // wave-uniform
            // the accumulators start at zero and this step's input projection is added once, behind the matrix loop.  (Seeded
            // with xg, each of the H / 2 (F32) or 3 H / 16 (F16X3) accumulation steps rounded at the magnitude of xg + partial sum
            // instead of the partial sum's: 2.5 x the error at H = 512, tests/test_spk_lstm_gpu.py.)
            f32x16 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
            if constexpr (SPLIT) {
                const int KC = H / 16;
                const f16x8* wb = reinterpret_cast<const f16x8*>(a.w) + (long)ub * KC * 8 * 64 + lane;
                const f16x8* ab = reinterpret_cast<const f16x8*>(hb);
                const long lo_off = part_halves / 8;
#pragma unroll 2
                for (int kc = 0; kc < KC; ++kc) {
                    f16x8 bh[4], bl[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        bh[q] = wb[((long)kc * 8 + q * 2 + 0) * 64];
                        bl[q] = wb[((long)kc * 8 + q * 2 + 1) * 64];
                    }
                    const int kb = kc * 2 + hi;
                    const int slot = kb * 32 + (j ^ (kb & 31));
                    const f16x8 ah = ab[slot], al = ab[lo_off + slot];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[q], acc[q], 0, 0, 0);
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[q], acc[q], 0, 0, 0);
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[q], acc[q], 0, 0, 0);
                    }
                }
            } else {
                const int KP = H / 2;
                const f32x4* wb = reinterpret_cast<const f32x4*>(a.w) + (long)ub * KP * 64 + lane;
#pragma unroll 4
                for (int kp = 0; kp < KP; ++kp) {
                    const f32x4 b = wb[(long)kp * 64];
                    const int k = kp * 2 + hi;
                    const float av = sm[k * 32 + (j ^ (k & 31))];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[q], acc[q], 0, 0, 0);
                }
            }
            // the cell, in registers
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, hi);
                // rows behind P read the last partial's xg: unconditional loads that the compiler may issue together (behind a
                // guard each waited for its own latency); what those rows compute is never stored and feeds no other row.
                // (32-bit offsets: pk_spk_embed admits at most 2^30 elements of xg; they halve the address registers)
                const long p = p0 + row < P ? p0 + row : P - 1;
                const float* xr = a.xg + (unsigned)((p * T + t) * G + ub * 32 + j);
                // the products come back from their scale by a power of two (exact)
                const float sc = SPLIT ? pow2f(-((t == 0 ? rexp[row] : PK_UNIT_EXP) + a.kw)) : 1.f;
                float g4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) g4[q] = acc[q][r] * sc + xr[q * H];
                const float gi = sigmoidf_(g4[0]);
                const float gf = sigmoidf_(g4[1]);
                const float gg = tanhf(g4[2]);
                const float go = sigmoidf_(g4[3]);
                const float c = gf * cst[s][r] + gi * gg;
                cst[s][r] = c;
                hnew[s][r] = go * tanhf(c);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long p = p0 + mfma_row(r, hi);
                if (p >= P) continue;
                if (a.hseq) a.hseq[(p * T + t) * H + ub * 32 + j] = hnew[s][r];
                if (a.hlast && t == T - 1) a.hlast[p * H + ub * 32 + j] = hnew[s][r];
            }
        }
        __syncthreads();   // every wave has read h(t-1)
#pragma unroll
        for (int s = 0; s < UBW; ++s) {
            const int ub = wave + s * SPK_WAVES;
            if (ub >= nub) break;
            const int u = ub * 32 + j;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, hi);
                const float v = hnew[s][r];
                if constexpr (SPLIT) {
                    const int kb = u >> 3;
                    const long o = ((long)kb * 32 + (row ^ (kb & 31))) * 8 + (u & 7);
                    const _Float16 vh = (_Float16)(v * PK_UNIT_SCALE);
                    hb[o] = vh;
                    hb[part_halves + o] = (_Float16)(v * PK_UNIT_SCALE - (float)vh);
                } else {
                    sm[u * 32 + (row ^ j)] = v;   // (u & 31) == j
                }
            }
        }
        __syncthreads();
    }
}

// One workgroup per utterance (cu != NULL: partials cu[u] .. cu[u + 1] - 1, mean + normalise) or per partial.
// LDS: h row [H] | e [O] | m [O] | 4 partial sums.
__global__ __launch_bounds__(256) void k_spk_head(const float* __restrict__ hlast, const float* __restrict__ W,
                                                  const float* __restrict__ bias, const int* __restrict__ cu, int H, int O,
                                                  float* __restrict__ out) {
    extern __shared__ float shd[];
    float* hrow = shd;
    float* e = shd + H;
    float* m = e + O;
    float* red = m + O;
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pb = cu ? cu[u] : u, pe = cu ? cu[u + 1] : u + 1;
    auto block_sum = [&](float v) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave] = v;
        __syncthreads();
        const float s = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
        return s;
    };
    for (int o = tid; o < O; o += 256) m[o] = 0.f;
    for (int p = pb; p < pe; ++p) {
        for (int k = tid; k < H; k += 256) hrow[k] = hlast[(long)p * H + k];
        __syncthreads();
        float ss = 0.f;
        for (int o = tid; o < O; o += 256) {
            float v0 = 0.f, v1 = 0.f;
            int k = 0;
            for (; k + 1 < H; k += 2) {
                v0 = fmaf(hrow[k], W[(long)k * O + o], v0);
                v1 = fmaf(hrow[k + 1], W[(long)(k + 1) * O + o], v1);
            }
            if (k < H) v0 = fmaf(hrow[k], W[(long)k * O + o], v0);
            const float v = fmaxf(v0 + v1 + bias[o], 0.f);
            e[o] = v;
            ss = fmaf(v, v, ss);
        }
        const float nrm = fmaxf(sqrtf(block_sum(ss)), 1e-12f);   // F.normalize: x / max(||x||, eps)
        for (int o = tid; o < O; o += 256) m[o] += e[o] / nrm;
    }
    if (cu) {
        const float n = (float)(pe - pb);
        float ss = 0.f;
        for (int o = tid; o < O; o += 256) {
            const float v = m[o] / n;
            m[o] = v;
            ss = fmaf(v, v, ss);
        }
        const float nrm = fmaxf(sqrtf(block_sum(ss)), 1e-12f);
        for (int o = tid; o < O; o += 256) out[(long)u * O + o] = m[o] / nrm;
    } else {
        for (int o = tid; o < O; o += 256) out[(long)u * O + o] = m[o];
    }
}

// (P * T) rows of C channels -> rows of Cp >= C channels, the extra columns zero
__global__ __launch_bounds__(256) void k_spk_pad_in(const float* __restrict__ in, long rows, int C, int Cp, float* __restrict__ x) {
    const long n = rows * Cp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / Cp;
        const int c = (int)(i - r * Cp);
        x[i] = c < C ? in[r * C + c] : 0.f;
    }
}

// Layer 0 for n_mels > SPK_GEMM_MAX_IN: xg = in . W_ih^T + b with fp64 accumulators.  The tile GEMM sums K products in one fp32
// accumulator, k ascending; a power mel spreads over decades, the partial sums of thousands of terms reach 50 - 100 and every
// step rounds at that magnitude (n_mels 4096: 2.6 - 3.1 x the bar of tests/test_spk_lstm_gpu.py, reproduced by an fp32
// restatement summed one k at a time).  One thread per gate column and SPK_WIDE_ROWS rows; kn is W_ih^T [n_mels][G].
__global__ __launch_bounds__(256) void k_spk_proj_wide(const float* __restrict__ in, long rows, int C, const float* __restrict__ kn,
                                                       const float* __restrict__ bias, int G, float* __restrict__ xg) {
    const int g = blockIdx.y * 256 + threadIdx.x;
    const long r0 = (long)blockIdx.x * SPK_WIDE_ROWS;
    if (g >= G) return;
    double acc[SPK_WIDE_ROWS];
    const float* src[SPK_WIDE_ROWS];
#pragma unroll
    for (int i = 0; i < SPK_WIDE_ROWS; ++i) {
        acc[i] = 0.0;
        src[i] = in + (r0 + i < rows ? r0 + i : rows - 1) * C;   // rows behind the end repeat the last one and are not stored
    }
    for (int k = 0; k < C; ++k) {
        const double w = kn[(long)k * G + g];
#pragma unroll
        for (int i = 0; i < SPK_WIDE_ROWS; ++i) acc[i] = fma((double)src[i][k], w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < SPK_WIDE_ROWS; ++i)
        if (r0 + i < rows) xg[(r0 + i) * G + g] = (float)(acc[i] + (double)bias[g]);
}

uint16_t f32_to_f16_bits(float v) {
    const _Float16 h = (_Float16)v;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
float f16_bits_to_f32(uint16_t b) {
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}
}  // namespace

struct pk_spk : pk_fft_core {
    pk_spk_cfg cfg;
    pk_param_map params;
    bool finalized = false;
    int cin0 = 0;                       // n_mels padded to a multiple of 32
    std::vector<Dense> xin;             // per layer: input projection + both biases
    std::vector<size_t> whh32, whh16;   // per layer: packed W_hh^T (F32 floats / F16X3 halves)
    std::vector<int> kw;                // per layer: exponent of the split weights
    size_t lin_w = 0, lin_b = 0;
    size_t wide_kn = 0, wide_b = 0;     // n_mels > SPK_GEMM_MAX_IN: W_ih^T [n_mels][4H] and b_ih + b_hh of layer 0, fp32
    pk_dbuf d_x, d_xg, d_hseq, d_hlast, d_cu;
    pk_dbuf d_ge2e;                     // pk_spk_ge2e: row terms, speaker sums, transposed centroids
    std::vector<int32_t> cu_h;          // host copy of the last call's utterance bounds (source of its async copy)
    hipEvent_t cu_ev = nullptr;         // recorded after that copy
};

namespace {
int find_param(const pk_param_map& P, const std::vector<std::string>& names, int64_t n, const std::vector<float>** out) {
    for (const std::string& nm : names) {
        auto it = P.find(nm);
        if (it == P.end()) continue;
        if (it->second.numel() != n)
            PK_FAIL(PK_ESHAPE, "LSTMSpeakerEncoder: parameter %s has %lld elements, expected %lld", nm.c_str(),
                    (long long)it->second.numel(), (long long)n);
        *out = &it->second.data;
        return PK_OK;
    }
    PK_FAIL(PK_ESTATE, "LSTMSpeakerEncoder: parameter %s was never set", names.front().c_str());
}

size_t rec_lds_bytes(int H) { return (size_t)H * 128 + SPK_M * sizeof(int); }
}  // namespace

extern "C" int pk_spk_create(pk_ctx* ctx, const pk_spk_cfg* cfg, pk_spk** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_spk_create: NULL argument");
    *out = nullptr;
    const pk_spk_cfg& c = *cfg;
    if (c.n_mels <= 0 || c.num_layers <= 0) PK_FAIL(PK_EINVAL, "LSTMSpeakerEncoder: n_mels and num_layers must be positive");
    if (c.hidden_size <= 0 || c.hidden_size % 32 != 0 || c.hidden_size > SPK_MAX_H)
        PK_FAIL(PK_EUNSUPPORTED, "LSTMSpeakerEncoder: hidden_size %d unsupported (a multiple of 32 up to %d)", c.hidden_size,
                SPK_MAX_H);
    if (c.output_size <= 0 || c.output_size % 32 != 0 || c.output_size > 4096)
        PK_FAIL(PK_EUNSUPPORTED, "LSTMSpeakerEncoder: output_size %d unsupported (a multiple of 32 up to 4096)", c.output_size);
    if (c.n_mels > 4096) PK_FAIL(PK_EUNSUPPORTED, "LSTMSpeakerEncoder: n_mels %d unsupported (at most 4096)", c.n_mels);
    pk_spk* h = new pk_spk();
    h->ctx = ctx;
    h->cfg = c;
    h->cin0 = (c.n_mels + 31) / 32 * 32;
    *out = h;
    return PK_OK;
}

extern "C" int pk_spk_set_param(pk_spk* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_spk_set_param: handle is NULL");
    if (name && (!strcmp(name, "similarity_weight") || !strcmp(name, "similarity_bias"))) {
        // the GE2E scale and offset (:29-32): read by pk_spk_ge2e, no part of the packed weights
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape ? shape[i] : 0;
        if (!data || !shape || ndim < 1 || n != 1) PK_FAIL(PK_ESHAPE, "LSTMSpeakerEncoder: parameter %s must have shape [1]", name);
        return pk_store_param(h->params, name, data, shape, ndim);
    }
    h->finalized = false;
    return pk_store_param(h->params, name, data, shape, ndim);
}

extern "C" int pk_spk_set_math(pk_spk* h, int32_t mode) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_spk_set_math: handle is NULL");
    if (mode != PK_GEMM_MATH_F32 && mode != PK_GEMM_MATH_F16X3) PK_FAIL(PK_EINVAL, "pk_spk_set_math: unknown mode %d", mode);
    h->math = mode;
    return PK_OK;
}

extern "C" int pk_spk_finalize(pk_spk* h) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_spk_finalize: handle is NULL");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_spk_cfg& c = h->cfg;
    const int H = c.hidden_size, G = 4 * H, L = c.num_layers, O = c.output_size;
    h->arena_h.clear();
    h->arena16_h.clear();
    pk_fft_arena ar{h->arena_h, &h->arena16_h};
    h->xin.assign(L, Dense());
    h->whh32.assign(L, 0);
    h->whh16.assign(L, 0);
    h->kw.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        // nn.LSTM registers each parameter twice: "lstm.weight_ih_l{k}" and "lstm.{k}.cell.weight_ih"
        const std::string a = "lstm.", cl = a + std::to_string(l) + ".cell.", sl = std::to_string(l);
        const int in = l == 0 ? c.n_mels : H, cin = l == 0 ? h->cin0 : H;
        const std::vector<float>*wih, *whh, *bih, *bhh;
        PK_TRY(find_param(h->params, {a + "weight_ih_l" + sl, cl + "weight_ih"}, (int64_t)G * in, &wih));
        PK_TRY(find_param(h->params, {a + "weight_hh_l" + sl, cl + "weight_hh"}, (int64_t)G * H, &whh));
        PK_TRY(find_param(h->params, {a + "bias_ih_l" + sl, cl + "bias_ih"}, G, &bih));
        PK_TRY(find_param(h->params, {a + "bias_hh_l" + sl, cl + "bias_hh"}, G, &bhh));
        std::vector<float> kn((size_t)cin * G, 0.f), bias(G);
        for (int g = 0; g < G; ++g) {
            for (int k = 0; k < in; ++k) kn[(size_t)k * G + g] = (*wih)[(size_t)g * in + k];
            bias[g] = (*bih)[g] + (*bhh)[g];
        }
        if (l == 0 && c.n_mels > SPK_GEMM_MAX_IN) {
            h->wide_kn = ar.put(kn);
            h->wide_b = ar.put(bias);
        } else {
            PK_TRY(pk_fft_add_dense_kn(ar, kn, &bias, cin, 1, G, h->xin[l]));
        }
        // W_hh^T in the operand layouts of k_spk_lstm_rec: lane (j, hi) of the wave owning unit block ub, gate q
        const std::vector<float>& W = *whh;   // [4H][H]
        const int nub = H / 32;
        std::vector<float> p32((size_t)G * H);
        for (int ub = 0; ub < nub; ++ub)
            for (int kp = 0; kp < H / 2; ++kp)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 4; ++q) {
                        const int k = kp * 2 + (lane >> 5), n = q * H + ub * 32 + (lane & 31);
                        p32[(((size_t)ub * (H / 2) + kp) * 64 + lane) * 4 + q] = W[(size_t)n * H + k];
                    }
        h->whh32[l] = ar.put(p32);
        const int kw = pk_weight_scale_exp(W.data(), W.size());
        h->kw[l] = kw;
        std::vector<uint16_t> p16((size_t)G * H * 2);
        for (int ub = 0; ub < nub; ++ub)
            for (int kc = 0; kc < H / 16; ++kc)
                for (int q = 0; q < 4; ++q)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int k = kc * 16 + (lane >> 5) * 8 + e, n = q * H + ub * 32 + (lane & 31);
                            const float w = std::ldexp(W[(size_t)n * H + k], kw);
                            const uint16_t hb = f32_to_f16_bits(w), lb = f32_to_f16_bits(w - f16_bits_to_f32(hb));
                            const size_t base = ((((size_t)ub * (H / 16) + kc) * 4 + q) * 2) * 64;
                            p16[((base + 0 * 64) + lane) * 8 + e] = hb;
                            p16[((base + 1 * 64) + lane) * 8 + e] = lb;
                        }
        h->whh16[l] = ar.put16(p16);
    }
    {
        std::vector<float> w, b;
        PK_TRY(pk_get_weight(h->params, "linear", {H, O}, w));   // paddle Linear.weight [in, out]
        PK_TRY(pk_get_vector(h->params, "linear.bias", O, b));
        h->lin_w = ar.put(w);
        h->lin_b = ar.put(b);
    }
    PK_TRY(pk_upload(ctx, h->arena, h->arena_h.data(), h->arena_h.size() * sizeof(float)));
    h->arena_h.clear();
    h->arena_h.shrink_to_fit();
    PK_TRY(pk_upload(ctx, h->arena16, h->arena16_h.data(), h->arena16_h.size() * sizeof(uint16_t)));
    h->arena16_h.clear();
    h->arena16_h.shrink_to_fit();
    h->finalized = true;
    return PK_OK;
}

extern "C" int pk_spk_embed(pk_spk* h, const float* partials, int32_t P, int32_t T, const float* h0, const float* c0,
                            const int32_t* cu_partials, int32_t U, float* out) {
    if (!h || !partials || !out) PK_FAIL(PK_EINVAL, "pk_spk_embed: NULL argument");
    if (!h->finalized) PK_FAIL(PK_ESTATE, "pk_spk_embed: call pk_spk_finalize first");
    if (P <= 0 || T <= 0) PK_FAIL(PK_EINVAL, "pk_spk_embed: %d partials of %d frames", P, T);
    if ((h0 == nullptr) != (c0 == nullptr)) PK_FAIL(PK_EINVAL, "pk_spk_embed: initial states come as a pair (h0, c0)");
    if (cu_partials) {
        if (U <= 0) PK_FAIL(PK_EINVAL, "pk_spk_embed: %d utterances", U);
        if (cu_partials[0] != 0 || cu_partials[U] != P)
            PK_FAIL(PK_EINVAL, "pk_spk_embed: cu_partials must run from 0 to P = %d", P);
        for (int u = 0; u < U; ++u)
            if (cu_partials[u + 1] <= cu_partials[u]) PK_FAIL(PK_EINVAL, "pk_spk_embed: utterance %d has no partial", u);
    } else if (U != P) {
        PK_FAIL(PK_EINVAL, "pk_spk_embed: without cu_partials there is one output row per partial (U = P)");
    }
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pk_spk_cfg& c = h->cfg;
    const int H = c.hidden_size, G = 4 * H, L = c.num_layers, O = c.output_size;
    const long rows = (long)P * T;
    if (rows > (1L << 30) / std::max(G, h->cin0)) PK_FAIL(PK_EUNSUPPORTED, "pk_spk_embed: %ld frames in one call exceed 2^30 elements", rows);
    // utterance bounds: an asynchronous copy from a host copy the handle keeps alive until the copy has run (the call
    // stays asynchronous; the next call waits on the event before it overwrites the host copy)
    const int* dcu = nullptr;
    if (cu_partials) {
        if (h->cu_ev) PK_HIP(hipEventSynchronize(h->cu_ev));
        else PK_HIP(hipEventCreateWithFlags(&h->cu_ev, hipEventDisableTiming));
        h->cu_h.assign(cu_partials, cu_partials + U + 1);
        PK_TRY(h->d_cu.reserve((size_t)(U + 1) * sizeof(int32_t)));
        PK_HIP(hipMemcpyAsync(h->d_cu.p, h->cu_h.data(), (size_t)(U + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        PK_HIP(hipEventRecord(h->cu_ev, ctx->stream));
        dcu = h->d_cu.as<int>();
    }
    const bool wide = c.n_mels > SPK_GEMM_MAX_IN;   // layer 0 reads the partials themselves (k_spk_proj_wide)
    if (!wide) PK_TRY(pk_fft_act_reserve(h->d_x, (int)rows, h->cin0));
    PK_TRY(pk_fft_act_reserve(h->d_xg, (int)rows, G));
    if (L > 1) PK_TRY(pk_fft_act_reserve(h->d_hseq, (int)rows, H));
    PK_TRY(h->d_hlast.reserve((size_t)P * H * sizeof(float)));
    float* x = wide ? nullptr : pk_fft_act_ptr(h->d_x, h->cin0);
    float* xg = pk_fft_act_ptr(h->d_xg, G);
    float* hseq = L > 1 ? pk_fft_act_ptr(h->d_hseq, H) : nullptr;
    // the GEMM tiles read rows up to the next multiple of 128 beyond P * T: only that tail is cleared (the rows below are
    // written first, by k_spk_pad_in / each layer's recurrence; the tail only feeds output rows that are discarded)
    auto clear_tail = [&](pk_dbuf& buf, float* base, int C) -> int {
        const size_t off = (size_t)((char*)(base + rows * C) - (char*)buf.p);
        if (off < buf.cap) PK_HIP(hipMemsetAsync((char*)buf.p + off, 0, buf.cap - off, ctx->stream));
        return PK_OK;
    };
    if (!wide) PK_TRY(clear_tail(h->d_x, x, h->cin0));
    if (L > 1) PK_TRY(clear_tail(h->d_hseq, hseq, H));
    if (!wide) {
        const long n = rows * h->cin0;
        const int grid = (int)std::min<long>((n + 255) / 256, 16384);
        PK_LAUNCH(ctx, "spk_pad_in", k_spk_pad_in, dim3(grid), dim3(256), 0, partials, rows, c.n_mels, h->cin0, x);
    }
    for (int l = 0; l < L; ++l) {
        const float* A = l == 0 ? x : hseq;
        if (l == 0 && wide) {
            PK_LAUNCH(ctx, "spk_proj_wide", k_spk_proj_wide, dim3((unsigned)pk_div_up(rows, (long)SPK_WIDE_ROWS), pk_div_up(G, 256)),
                      dim3(256), 0, partials, rows, c.n_mels, h->W(h->wide_kn), h->W(h->wide_b), G, xg);
        } else {
            PK_TRY(pk_fft_run_dense(h, "spk_gemm_xg", h->xin[l], A, l == 0 ? h->cin0 : H, xg, G, (int)rows, PK_ACT_NONE, nullptr, 0,
                                    nullptr));
        }
        RecArgs ra;
        ra.xg = xg;
        ra.kw = h->kw[l];
        ra.h0 = h0 ? h0 + (long)l * P * H : nullptr;
        ra.c0 = c0 ? c0 + (long)l * P * H : nullptr;
        ra.hseq = l + 1 < L ? hseq : nullptr;
        ra.hlast = l + 1 < L ? nullptr : h->d_hlast.as<float>();
        ra.P = P;
        ra.T = T;
        ra.H = H;
        const dim3 grid(pk_div_up(P, SPK_M)), block(SPK_WAVES * 64);
        static const char* names[3] = {"spk_lstm_rec_l0", "spk_lstm_rec_l1", "spk_lstm_rec_l2+"};
        const char* nm = names[std::min(l, 2)];
        const bool split = h->math == PK_GEMM_MATH_F16X3;
        ra.w = split ? (const void*)(h->arena16.as<uint16_t>() + h->whh16[l]) : (const void*)h->W(h->whh32[l]);
        const size_t lds = rec_lds_bytes(H);
        if (split && H <= 256)
            PK_LAUNCH(ctx, nm, (k_spk_lstm_rec<PK_GEMM_MATH_F16X3, 1>), grid, block, lds, ra);
        else if (split)
            PK_LAUNCH(ctx, nm, (k_spk_lstm_rec<PK_GEMM_MATH_F16X3, 2>), grid, block, lds, ra);
        else if (H <= 256)
            PK_LAUNCH(ctx, nm, (k_spk_lstm_rec<PK_GEMM_MATH_F32, 1>), grid, block, lds, ra);
        else
            PK_LAUNCH(ctx, nm, (k_spk_lstm_rec<PK_GEMM_MATH_F32, 2>), grid, block, lds, ra);
    }
    PK_LAUNCH(ctx, "spk_head", k_spk_head, dim3(U), dim3(256), (size_t)(H + 2 * O + 4) * sizeof(float), h->d_hlast.as<float>(),
              h->W(h->lin_w), h->W(h->lin_b), dcu, H, O, out);
    return PK_OK;
}

extern "C" int pk_spk_ge2e(pk_spk* h, const float* embeds, int32_t N, int32_t M, int32_t C, float* sim, float* p1, float* p2,
                           double* row_nll, double* loss) {
    if (!h || !embeds) PK_FAIL(PK_EINVAL, "pk_spk_ge2e: NULL argument");
    float wb[2] = {10.f, -5.f};   // I.Constant(10.), I.Constant(-5.) (:29-32)
    const char* names[2] = {"similarity_weight", "similarity_bias"};
    for (int i = 0; i < 2; ++i) {
        auto it = h->params.find(names[i]);
        if (it != h->params.end()) wb[i] = it->second.data[0];
    }
    return pk_spk_loss_run(h->ctx, h->d_ge2e, wb[0], wb[1], embeds, N, M, C, sim, p1, p2, row_nll, loss);
}

extern "C" int pk_spk_cosine(pk_spk* h, const float* a, const float* b, int32_t U, int32_t C, float* out) {
    if (!h) PK_FAIL(PK_EINVAL, "pk_spk_cosine: handle is NULL");
    return pk_spk_cosine_run(h->ctx, a, b, U, C, out);
}

extern "C" void pk_spk_destroy(pk_spk* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->release_core();
    pk_dbuf* bufs[] = {&h->d_x, &h->d_xg, &h->d_hseq, &h->d_hlast, &h->d_cu, &h->d_ge2e};
    for (auto* b : bufs) b->release();
    if (h->cu_ev) (void)hipEventDestroy(h->cu_ev);
    delete h;
}
