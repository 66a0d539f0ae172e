// pk_rfft.h -- the radix FFT of rfft.hip as the other translation units see it (mel.hip and istft.hip run their frames on it
// under PK_TRANSFORM_FFT; pk_op_rfft / pk_op_irfft are the public primitive).
//
// THE PLAN (tests/rfft_ref.py restates it and counts its roundings for the error bound; change one, change the other).
// A real transform of n points, n = 2^5 ... 2^12, is a complex transform of M = n / 2 points z[m] = x[2m] + i x[2m+1] plus a
// split pass:
//   1. Stockham autosort passes over two LDS buffers, decimation in time, sub-transform length Ns = 1, 4, 16, ...:
//      floor(log2(M) / 2) radix-4 passes; where log2(M) is odd ONE radix-2 pass follows them (Ns = M / 2).
//        radix-4 pass, butterfly j in [0, M/4), k = j mod Ns:  v_q = in[j + q M/4] * T[q k n/(4 Ns)]  (q = 1, 2, 3; v_0 = in[j]),
//                      out[(j - k) 4 + k + r Ns] = sum_q v_q (-i)^(r q)   as two levels of additions
//        radix-2 pass, butterfly j in [0, M/2):                v_1 = in[j + M/2] * T[2 j],  out[j] = v_0 + v_1, out[j + M/2] = v_0 - v_1
//      The first pass (Ns = 1, k = 0) multiplies by T[0] = 1 like every other: one code path, the product is exact.
//   2. split pass, k in [0, M]:  A = Z[k] + conj(Z[M-k]),  B = -i (Z[k] - conj(Z[M-k])),  X[k] = (A + T[k] B) / 2   (Z[M] = Z[0])
//   The inverse builds Z[k] = (X[k] + conj(X[M-k])) + i conj(T[k]) (X[k] - conj(X[M-k])) for k in [0, M) -- im X[0] and
//   im X[M] are never read --, runs the same passes on conj(Z) and conjugates back, scales by the exact 1/n, then multiplies
//   by the window.
// T[t] = exp(-2 pi i t / n), t in [0, n): computed in fp64 on the host, rounded once to fp32, uploaded when the context first
// needs that n.  No sine or cosine is evaluated on the device.
//
// One workgroup of 256 threads owns PK_RFFT rows(n) whole frames: min(256, M/4) threads per frame, one or two radix-4
// butterflies per thread and pass.  Nothing is shared between frames, there are no atomics, the order is fixed: a frame's
// result does not depend on the batch around it.
#pragma once
#include "pk_common.h"

static inline bool pk_rfft_size_ok(int n) { return n >= 32 && n <= 4096 && (n & (n - 1)) == 0; }
#define PK_RFFT_SIZES "a power of two from 32 to 4096"
// frames per workgroup
static inline int pk_rfft_rows_per_block(int n) { return n / 8 >= 256 ? 1 : 256 / (n / 8); }

// Builds and uploads T for n on first need (synchronises the stream then); later calls do nothing.
int pk_rfft_prepare(pk_ctx* ctx, int n);
// Forward: frame `row` is the n floats at x + row * stride (stride in floats, the start 8-byte aligned), times window[0..n)
// where window != NULL.  Writes re | im (n/2 + 1 floats each) at out + o * ldc, o = rowmap ? rowmap[row] : row; rows with a
// negative map entry are skipped.  pk_rfft_prepare(ctx, n) must have succeeded.
int pk_rfft_forward(pk_ctx* ctx, const char* name, const float* x, long stride, const float* window, const int* rowmap,
                    long rows, int n, float* out, long ldc);
// Inverse: row r reads re | im at spec + r * ld (the imaginary parts of DC and Nyquist are not read), writes n floats at
// out + r * n (8-byte aligned): irfft * window (window == NULL: 1).
int pk_rfft_inverse(pk_ctx* ctx, const char* name, const float* spec, long ld, const float* window, long rows, int n,
                    float* out);
