// pk_spk_loss.h -- the GE2E similarity matrix and softmax loss (spk_loss.hip), called by pk_spk_ge2e (spk.hip).
#pragma once
#include "pk_common.h"

// The envelope (beyond it: PK_EUNSUPPORTED, nothing is truncated)
#define PK_GE2E_MAX_N 4096
#define PK_GE2E_MAX_C 2048
#define PK_GE2E_MAX_ROWS (1L << 20)     // N * M
#define PK_GE2E_MAX_SCORES (1L << 28)   // N * M * N
// utterances (rows of the similarity matrix) per workgroup: 8 while their C floats each fit 32 KB of LDS, else 4.  A row's
// numbers do not depend on the tile it rides in.
#define PK_GE2E_ROWS_WIDE 8
#define PK_GE2E_ROWS_NARROW 4
#define PK_GE2E_WIDE_MAX_C 1024

// embeds (N, M, C) on the device; w, b: similarity_weight / similarity_bias; ws: the handle's workspace.  Every output is a
// nullable device pointer: sim (N*M, N), p1 (N*M*N), p2 (N*M), row_nll (N*M) double, loss (1) double.
int pk_spk_loss_run(pk_ctx* ctx, pk_dbuf& ws, float w, float b, const float* embeds, int N, int M, int C, float* sim, float* p1,
                    float* p2, double* row_nll, double* loss);

// out[u] = cosine similarity of rows u of a and b, both (U, C) on the device
int pk_spk_cosine_run(pk_ctx* ctx, const float* a, const float* b, int U, int C, float* out);
