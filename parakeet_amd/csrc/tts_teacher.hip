// tts_teacher.hip -- kernels of TransformerTTS.inference(..., use_teacher_forcing=True) on gfx950 (pk_tts_teacher.h).
//
// Reference: parakeet/models/transformer_tts/transformer_tts.py _forward :462-500 (teacher-forced branch of inference
// :567-579), Decoder.forward decoder.py:163-195, DecoderLayer.forward decoder_layer.py:74-158, MultiHeadedAttention
// attention.py:88-156.
//
// With teacher forcing every decoder input row is known up front, so the decoder runs as ONE pass over all rows of all
// utterances: the GEMMs are the tile GEMMs of gemm.hip on a row timeline, and the two attentions are the flash-style kernels
// below, one wave per (utterance, head, 32 query rows), scores and probabilities in registers:
//   S^T = K . Q^T    (A = 32 key rows, B = 32 query rows; the accumulator of lane (j, hi) holds query j's scores of keys
//                     mfma_row(r, hi))
//   online softmax per query = per lane (no cross-lane traffic besides one swap of the two lane halves)
//   O^T += V^T . P^T (A = V rows, B = the probabilities straight from the S registers)
// Two maths, as every kernel of the engine: exact fp32 (v_mfma_f32_32x32x2f32) and split-fp16 (v_mfma_f32_32x32x16_f16, three
// terms, operands block-scaled per (utterance, head), pk_split.h).  Every scale comes from the utterance's own rows, so the
// result of an utterance does not depend on the batch it is in.
// Causal self-attention: query tile i reads key tiles 0 .. i only; the key mask is applied in the diagonal tile.
// Encoder-decoder attention: with att != NULL a second pass over the keys recomputes the scores and writes the normalised
// weights; without it that traffic does not exist.
#include <algorithm>
#include <cmath>

#include "pk_gemm.h"
#include "pk_mfma.h"
#include "pk_philox.h"
#include "pk_split.h"
#include "pk_tts_teacher.h"

namespace {

// x = hi + lo: hi = fp16 round toward zero, lo = fp16_rne(x - hi) (plain C here; pk_mfma.h split8 is the same split through v_fma_mix_f32)
__device__ __forceinline__ void tt_split8(const float (&v)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const pkh2 h = __builtin_amdgcn_cvt_pkrtz(v[2 * p], v[2 * p + 1]);
        const float h0 = (float)h[0], h1 = (float)h[1];
        hi[2 * p] = (_Float16)h[0];
        hi[2 * p + 1] = (_Float16)h[1];
        lo[2 * p] = (_Float16)(v[2 * p] - h0);
        lo[2 * p + 1] = (_Float16)(v[2 * p + 1] - h1);
    }
}
__device__ __forceinline__ void tt_split8s(const float (&v)[8], float s, f16x8& hi, f16x8& lo) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = v[e] * s;
    tt_split8(t, hi, lo);
}
__device__ __forceinline__ f32x16 tt_mfma3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
}
// O^T tile rows are value channels, columns queries: this lane's query row goes out as 4-float pieces
template <int DT>
__device__ __forceinline__ void tt_store_out(const f32x16 (&O)[DT], float f, float* o_row, int hi) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            f32x4 v = {O[dt][4 * rq] * f, O[dt][4 * rq + 1] * f, O[dt][4 * rq + 2] * f, O[dt][4 * rq + 3] * f};
            *reinterpret_cast<f32x4*>(o_row + 32 * dt + 8 * rq + 4 * hi) = v;   // channels mfma_row(4 rq .. 4 rq + 3, hi)
        }
}

// keys of this lane's query: causal -> 0 .. q (within the segment), else all nk; -inf beyond.  Uniform test first: only the
// tiles that reach past the wave's smallest limit are masked.
__device__ __forceinline__ void tt_mask(f32x16& S, int k0, int hi, int klim_wave, int klim) {
    if (k0 + 32 > klim_wave) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (k0 + mfma_row(r, hi) >= klim) S[r] = -INFINITY;
    }
}

// ---- exact fp32
template <int DK>
__global__ __launch_bounds__(256, 1) void k_tt_attn_f32(pk_tt_attn a) {
    constexpr int KH = DK / 2;   // k-steps of S^T = K . Q^T (d = hi * KH + step)
    constexpr int DT = DK / 32;
    const int b = blockIdx.z, h = blockIdx.y;
    const int nq = a.q_len[b], nk = a.k_len[b];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    if (q0 >= nq) return;
    const int j = lane & 31, hi = lane >> 5;
    const float* qb = a.q + (long)a.q_start[b] * a.ldq + h * DK;
    const float* kb = a.k + (long)a.k_start[b] * a.ldkv + h * DK;
    const float* vb = a.v + (long)a.k_start[b] * a.ldkv + h * DK;
    const int kend = a.causal ? min(nk, q0 + 32) : nk;
    const int klim_wave = a.causal ? min(nk, q0 + 1) : nk;
    const int klim = a.causal ? min(nk, q0 + j + 1) : nk;

    float qf[KH];
    {
        const float* qp = qb + (long)min(q0 + j, nq - 1) * a.ldq + hi * KH;
#pragma unroll
        for (int c = 0; c < KH / 4; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 4 * c);
            qf[4 * c] = v[0]; qf[4 * c + 1] = v[1]; qf[4 * c + 2] = v[2]; qf[4 * c + 3] = v[3];
        }
    }
    auto scores = [&](int k0) {
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.f;
        const float* kp = kb + (long)min(k0 + j, nk - 1) * a.ldkv + hi * KH;
#pragma unroll
        for (int c = 0; c < KH / 4; ++c) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[e], qf[4 * c + e], S, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] *= a.scale;
        tt_mask(S, k0, hi, klim_wave, klim);
        return S;
    };
    f32x16 O[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    for (int k0 = 0; k0 < kend; k0 += 32) {
        f32x16 S = scores(k0);
        float mloc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, S[r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);   // (finite: key 0 is in every query's first tile)
        const float alpha = expf(m_run - m_new);
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            S[r] = expf(S[r] - m_new);
            lsum += S[r];
        }
        lsum += __shfl_xor(lsum, 32);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
        const float* vp = vb + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vrow = vp + (long)min(k0 + mfma_row(r, hi), nk - 1) * a.ldkv;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * dt], S[r], O[dt], 0, 0, 0);
        }
    }
    const int q = q0 + j;
    if (q < nq) tt_store_out<DT>(O, 1.f / l_run, a.out + (long)(a.q_start[b] + q) * a.ldo + h * DK, hi);
    if (a.att) {
        const float inv = 1.f / l_run;
        float* ap = a.att + a.att_off[b] + (((long)a.layer * a.heads + h) * nq + q) * nk;
        for (int k0 = 0; k0 < nk; k0 += 32) {
            const f32x16 S = scores(k0);
            if (q < nq)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + mfma_row(r, hi);
                    if (key < nk) ap[key] = expf(S[r] - m_run) * inv;
                }
        }
    }
}

// ---- split-fp16 (default math)
template <int DK>
__global__ __launch_bounds__(256, 1) void k_tt_attn_h3(pk_tt_attn a) {
    constexpr int KS = DK / 16;
    constexpr int DT = DK / 32;
    const int b = blockIdx.z, h = blockIdx.y;
    const int nq = a.q_len[b], nk = a.k_len[b];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    if (q0 >= nq) return;
    const int j = lane & 31, hi = lane >> 5;
    const float* qb = a.q + (long)a.q_start[b] * a.ldq + h * DK;
    const float* kb = a.k + (long)a.k_start[b] * a.ldkv + h * DK;
    const float* vb = a.v + (long)a.k_start[b] * a.ldkv + h * DK;
    const int kend = a.causal ? min(nk, q0 + 32) : nk;
    const int klim_wave = a.causal ? min(nk, q0 + 1) : nk;
    const int klim = a.causal ? min(nk, q0 + j + 1) : nk;
    // block scales of this (utterance, head): operands to [2^13, 2^14), the accumulators brought back in the softmax / epilogue
    const unsigned* mx = a.amax + ((long)b * a.heads + h) * 3;
    const int eq = blk_scale_exp(mx[0]), ek = blk_scale_exp(mx[1]), ev = blk_scale_exp(mx[2]);
    const float sq = pow2f(eq), sk = pow2f(ek), sv = pow2f(ev);
    const float c2 = a.scale * pow2f(-eq) * pow2f(-ek) * 1.4426950408889634f;   // accumulator -> logit in log2 units
    const float co = pow2f(-ev);

    f16x8 qh[KS], ql[KS];
    {
        const float* qp = qb + (long)min(q0 + j, nq - 1) * a.ldq + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(qp + 16 * ks);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(qp + 16 * ks + 4);
            const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            tt_split8s(v, sq, qh[ks], ql[ks]);
        }
    }
    auto scores = [&](int k0) {   // logits in log2 units
        f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.f;
        const float* kp = kb + (long)min(k0 + j, nk - 1) * a.ldkv + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(kp + 16 * ks);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(kp + 16 * ks + 4);
            const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            f16x8 kh, kl;
            tt_split8s(v, sk, kh, kl);
            S = tt_mfma3(kh, kl, qh[ks], ql[ks], S);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] *= c2;
        tt_mask(S, k0, hi, klim_wave, klim);
        return S;
    };
    f32x16 O[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    for (int k0 = 0; k0 < kend; k0 += 32) {
        f32x16 S = scores(k0);
        float mloc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, S[r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        const float off = (float)PK_UNIT_EXP - m_new;   // P operand = 2^14 p (p <= 1: the fixed block scale)
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            S[r] = __builtin_amdgcn_exp2f(S[r] + off);
            lsum += S[r];
        }
        lsum += __shfl_xor(lsum, 32);
        l_run = fmaf(l_run, alpha, lsum);
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
        const float* vp = vb + j;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float pv[8];
            long voff[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                pv[e] = S[8 * s2 + e];
                voff[e] = (long)min(k0 + mfma_row(8 * s2 + e, hi), nk - 1) * a.ldkv;
            }
            f16x8 ph, pl;
            tt_split8(pv, ph, pl);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                float vv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) vv[e] = vp[voff[e] + 32 * dt];
                f16x8 vh, vl;
                tt_split8s(vv, sv, vh, vl);
                O[dt] = tt_mfma3(vh, vl, ph, pl, O[dt]);   // O^T += V^T P^T
            }
        }
    }
    const int q = q0 + j;
    if (q < nq)   // O^T = 2^14 2^ev sum p v, l_run = 2^14 sum p
        tt_store_out<DT>(O, co / l_run, a.out + (long)(a.q_start[b] + q) * a.ldo + h * DK, hi);
    if (a.att) {
        const float inv = 1.f / l_run;
        const float off = (float)PK_UNIT_EXP - m_run;
        float* ap = a.att + a.att_off[b] + (((long)a.layer * a.heads + h) * nq + q) * nk;
        for (int k0 = 0; k0 < nk; k0 += 32) {
            const f32x16 S = scores(k0);
            if (q < nq)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + mfma_row(r, hi);
                    if (key < nk) ap[key] = __builtin_amdgcn_exp2f(S[r] + off) * inv;
                }
        }
    }
}

// block maxima: grid (ceil(maxlen / 32), heads, B), 4 waves x 8 rows
__global__ __launch_bounds__(256) void k_tt_amax(const float* __restrict__ x, int ld, const int* __restrict__ seg_start,
                                                 const int* __restrict__ seg_len, int dk, int nparts, int pstride, int slot0,
                                                 unsigned* __restrict__ amax) {
    const int b = blockIdx.z, h = blockIdx.y;
    const int len = seg_len[b], start = seg_start[b];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = blockIdx.x * 32 + wave * 8;
    if (r0 >= len) return;
    const int r1 = min(r0 + 8, len);
    for (int p = 0; p < nparts; ++p) {
        const float* src = x + (long)start * ld + p * pstride + h * dk;
        float m = 0.f;
        for (int r = r0; r < r1; ++r)
            for (int c = lane; c < dk; c += 64) m = fmaxf(m, fabsf(src[(long)r * ld + c]));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) atomicMax(amax + ((long)b * gridDim.y + h) * 3 + slot0 + p, __float_as_uint(m));
    }
}

__global__ __launch_bounds__(128) void k_tt_ys_in(const float* __restrict__ speech, const long* __restrict__ off, int O, int r,
                                                  const int* __restrict__ row_utt, const int* __restrict__ row_pos,
                                                  float* __restrict__ out) {
    const long q = blockIdx.x;
    const int u = row_utt[q];
    const int p = u >= 0 ? row_pos[q] : 0;
    const float* s = speech + (off[u < 0 ? 0 : u] + (long)p * r - 1) * O;
    for (int c = threadIdx.x; c < O; c += blockDim.x) out[q * O + c] = p > 0 ? s[c] : 0.f;
}

__global__ __launch_bounds__(256) void k_tt_dropout(float* __restrict__ x, int ld, int rows, int U, const int* __restrict__ row_utt,
                                                    const int* __restrict__ row_pos, const int* __restrict__ seg_len, int J, int j,
                                                    const unsigned long long* __restrict__ seeds, unsigned thr, float scale) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const int per_row = U >> 2;
    if (q >= (long)rows * per_row) return;
    const int r = (int)(q / per_row), u4 = (int)(q - (long)r * per_row) * 4;
    const int b = row_utt[r];
    if (b < 0) return;
    const unsigned long long s = (unsigned long long)seg_len[b];
    const unsigned long long e = ((s * (s - 1) / 2ull + (unsigned long long)row_pos[r]) * (unsigned long long)J +
                                  (unsigned long long)j) * (unsigned long long)U + (unsigned long long)u4;
    unsigned w[4];
    pk_dropout_words(e, seeds ? seeds[b] : 0ull, w);
    float4* p = reinterpret_cast<float4*>(x + (long)r * ld + u4);
    float4 v = *p;
    v.x = w[0] >= thr ? v.x * scale : 0.f;
    v.y = w[1] >= thr ? v.y * scale : 0.f;
    v.z = w[2] >= thr ? v.z * scale : 0.f;
    v.w = w[3] >= thr ? v.w * scale : 0.f;
    *p = v;
}

__global__ __launch_bounds__(128) void k_tt_scatter(const float* __restrict__ src, int C, const int* __restrict__ row_utt,
                                                    const int* __restrict__ row_pos, int B, int off, float* __restrict__ dst) {
    const long q = blockIdx.x;
    const int u = row_utt[q];
    if (u < 0) return;
    float* d = dst + ((long)(row_pos[q] + off) * B + u) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) d[c] = src[q * C + c];
}

// one wave per row
__global__ __launch_bounds__(256) void k_tt_probs(const float* __restrict__ z, int A, const float* __restrict__ w,
                                                  const float* __restrict__ bias, int r, const int* __restrict__ row_utt,
                                                  const int* __restrict__ row_pos, int rows, int B, float* __restrict__ probs,
                                                  float* __restrict__ logits) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= rows) return;
    const int u = row_utt[q];
    if (u < 0) return;
    for (int k = 0; k < r; ++k) {
        float s = 0.f;
        for (int c = lane; c < A; c += 64) s = fmaf(z[(long)q * A + c], w[(long)c * r + k], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            const long o = ((long)row_pos[q] * B + u) * r + k;
            const float lg = s + bias[k];
            probs[o] = 1.f / (1.f + expf(-lg));
            logits[o] = lg;   // what the stop criterion takes (a saturated probability does not give it back)
        }
    }
}
}  // namespace

int pk_tt_attention(pk_ctx* ctx, const pk_tt_attn& a, int dk, int math, int B, int maxq) {
    if (a.att && a.causal) PK_FAIL(PK_EINVAL, "pk_tt_attention: attention weights are kept for the encoder-decoder attention only");
    if (math == PK_GEMM_MATH_F16X3 && !a.amax) PK_FAIL(PK_EINVAL, "pk_tt_attention: split-fp16 needs block maxima");
    if (maxq <= 0 || B <= 0) return PK_OK;
    const dim3 grid(pk_div_up(maxq, 128), a.heads, B);
    if (math == PK_GEMM_MATH_F16X3) {
        switch (dk) {
            case 64: PK_LAUNCH(ctx, "tts_teacher_attn_h3", k_tt_attn_h3<64>, grid, dim3(256), 0, a); break;
            case 96: PK_LAUNCH(ctx, "tts_teacher_attn_h3", k_tt_attn_h3<96>, grid, dim3(256), 0, a); break;
            case 128: PK_LAUNCH(ctx, "tts_teacher_attn_h3", k_tt_attn_h3<128>, grid, dim3(256), 0, a); break;
            case 192: PK_LAUNCH(ctx, "tts_teacher_attn_h3", k_tt_attn_h3<192>, grid, dim3(256), 0, a); break;
            default: PK_FAIL(PK_EUNSUPPORTED, "teacher attention: head size %d", dk);
        }
        return PK_OK;
    }
    switch (dk) {
        case 64: PK_LAUNCH(ctx, "tts_teacher_attn", k_tt_attn_f32<64>, grid, dim3(256), 0, a); break;
        case 96: PK_LAUNCH(ctx, "tts_teacher_attn", k_tt_attn_f32<96>, grid, dim3(256), 0, a); break;
        case 128: PK_LAUNCH(ctx, "tts_teacher_attn", k_tt_attn_f32<128>, grid, dim3(256), 0, a); break;
        case 192: PK_LAUNCH(ctx, "tts_teacher_attn", k_tt_attn_f32<192>, grid, dim3(256), 0, a); break;
        default: PK_FAIL(PK_EUNSUPPORTED, "teacher attention: head size %d", dk);
    }
    return PK_OK;
}

int pk_tt_amax(pk_ctx* ctx, const float* x, int ld, const int* seg_start, const int* seg_len, int B, int heads, int dk,
               int nparts, int pstride, int slot0, int maxlen, unsigned* amax) {
    if (maxlen <= 0) return PK_OK;
    PK_LAUNCH(ctx, "tts_teacher_amax", k_tt_amax, dim3(pk_div_up(maxlen, 32), heads, B), dim3(256), 0, x, ld, seg_start, seg_len,
              dk, nparts, pstride, slot0, amax);
    return PK_OK;
}

int pk_tt_ys_in(pk_ctx* ctx, const float* speech, const long* off, int O, int r, const int* row_utt, const int* row_pos,
                int rows, float* out) {
    PK_LAUNCH(ctx, "tts_teacher_ys_in", k_tt_ys_in, dim3(rows), dim3(128), 0, speech, off, O, r, row_utt, row_pos, out);
    return PK_OK;
}

int pk_tt_dropout(pk_ctx* ctx, float* x, int ld, int rows, int U, const int* row_utt, const int* row_pos, const int* seg_len,
                  int J, int j, const unsigned long long* seeds, unsigned thr, float scale) {
    if (U % 4 != 0) PK_FAIL(PK_EUNSUPPORTED, "teacher dropout: units %% 4 != 0");
    PK_LAUNCH(ctx, "tts_teacher_dropout", k_tt_dropout, dim3(pk_div_up((long)rows * (U / 4), 256)), dim3(256), 0, x, ld, rows, U,
              row_utt, row_pos, seg_len, J, j, seeds, thr, scale);
    return PK_OK;
}

int pk_tt_scatter(pk_ctx* ctx, const float* src, int C, const int* row_utt, const int* row_pos, int rows, int B, int off,
                  float* dst) {
    PK_LAUNCH(ctx, "tts_teacher_scatter", k_tt_scatter, dim3(rows), dim3(128), 0, src, C, row_utt, row_pos, B, off, dst);
    return PK_OK;
}

int pk_tt_probs(pk_ctx* ctx, const float* z, int A, const float* w, const float* bias, int r, const int* row_utt,
                const int* row_pos, int rows, int B, float* probs, float* logits) {
    PK_LAUNCH(ctx, "tts_teacher_probs", k_tt_probs, dim3(pk_div_up(rows, 4)), dim3(256), 0, z, A, w, bias, r, row_utt, row_pos,
              rows, B, probs, logits);
    return PK_OK;
}
