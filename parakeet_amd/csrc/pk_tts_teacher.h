// pk_tts_teacher.h -- kernels of TransformerTTS's teacher-forced decoder pass (tts_teacher.hip), used by pk_tts_teacher
// (tts.hip).  The pass runs the whole decoder on a row timeline of the decoder inputs (pk_fft.h): utterance b's L_b / r rows
// are one segment, its T_b + 1 encoder rows one segment of the token timeline.
#pragma once
#include "pk_common.h"

// Multi-head attention of every query row of an utterance's segment at once (attention.py:133-156):
//   causal = 1: keys 0 .. query of the same segment (the decoder self-attention under _target_mask, transformer_tts.py:692-723)
//   causal = 0: every key row of the key segment (the encoder-decoder attention; the reference's memory mask is all ones)
// q rows [q_start[b], + q_len[b]) with head h at column h * dk (ld ldq); k / v rows [k_start[b], + k_len[b]) (ld ldkv).
// att != NULL (causal = 0 only): the softmax weights go to att[att_off[b] + ((layer * heads + h) * q_len[b] + i) * k_len[b] + j],
// i.e. pk_tts_read's (dlayers, heads, L_in, T_b) block of the utterance.
struct pk_tt_attn {
    const float* q = nullptr;
    int ldq = 0;
    const float* k = nullptr;
    const float* v = nullptr;
    int ldkv = 0;
    const int *q_start = nullptr, *q_len = nullptr, *k_start = nullptr, *k_len = nullptr;
    int causal = 0;
    float scale = 1.f;
    const unsigned* amax = nullptr;   // split-fp16: fp32 bits of max|q|, max|k|, max|v| per (utterance, head) [B][heads][3]
    float* out = nullptr;
    int ldo = 0;
    float* att = nullptr;
    const long* att_off = nullptr;
    int layer = 0, heads = 0;
};

// math: PK_GEMM_MATH_F32 or PK_GEMM_MATH_F16X3 (a.amax required); dk 64 / 96 / 128 / 192; maxq: the longest query segment
int pk_tt_attention(pk_ctx* ctx, const pk_tt_attn& a, int dk, int math, int B, int maxq);
// amax[(b * heads + h) * 3 + slot0 + p] = max(., max |x[r][p * pstride + h * dk + c]|) over the rows of segment b, p < nparts
// (atomicMax on fp32 bits: amax must be zeroed by the caller)
int pk_tt_amax(pk_ctx* ctx, const float* x, int ld, const int* seg_start, const int* seg_len, int B, int heads, int dk,
               int nparts, int pstride, int slot0, int maxlen, unsigned* amax);
// decoder inputs (transformer_tts.py:484-492): row pos of utterance u = 0 for pos 0, else speech[off[u] + pos * r - 1]
// (the last frame of the previous group of r); gap rows 0.  speech packed (sum L_b, O).
int pk_tt_ys_in(pk_ctx* ctx, const float* speech, const long* off, int O, int r, const int* row_utt, const int* row_pos,
                int rows, float* out);
// prenet dropout on timeline rows (include/pk_synth.h "dropout stream"): the prenet sees all L_in rows of an utterance in ONE
// call, the AR decode's call at step s = L_in: element ((s (s - 1) / 2 + pos) * J + j) * U + u, s = seg_len[utterance]
int pk_tt_dropout(pk_ctx* ctx, float* x, int ld, int rows, int U, const int* row_utt, const int* row_pos, const int* seg_len,
                  int J, int j, const unsigned long long* seeds, unsigned thr, float scale);
// timeline row (u, pos) -> row (pos + off) * B + u of a position-major array (pk_tts_read's layout of the AR decode)
int pk_tt_scatter(pk_ctx* ctx, const float* src, int C, const int* row_utt, const int* row_pos, int rows, int B, int off,
                  float* dst);
// prob_out + sigmoid per timeline row: probs[(pos * B + u) * r + k] = sigmoid(z[row] . w[:, k] + bias[k]) (w [A][r]);
// logits, in the same layout, keeps the sigmoid's argument
int pk_tt_probs(pk_ctx* ctx, const float* z, int A, const float* w, const float* bias, int r, const int* row_utt,
                const int* row_pos, int rows, int B, float* probs, float* logits);
