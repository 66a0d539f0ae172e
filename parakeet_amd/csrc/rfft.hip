// rfft.hip -- real FFT / inverse real FFT of whole frames in LDS on gfx950: the plan of pk_rfft.h.
//
// Reference semantics: numpy.fft.rfft / numpy.fft.irfft (what librosa.stft / librosa.istft, the reference's transforms, call
// per frame).  The dense products of mel.hip / istft.hip stay the default; this is the path of PK_TRANSFORM_FFT.
//
// LDS.  A frame's M = n/2 complex points live in two ping-pong buffers of float2 (Stockham: a pass reads one, writes the
// other, one barrier per pass); 256 threads hold max(1024, M) points per buffer, 2 x 8 KiB up to n = 2048 and 2 x 16 KiB at
// 4096.  Every access moves one float2 (ds_read_b64 / ds_write_b64).  A pass READS point j + q M/4 for consecutive j
// (consecutive lanes, conflict-free as it stands) and WRITES point (j - k) 4 + k + r Ns: stride 4 points in the first pass,
// runs of 4 at stride 16 in the second, runs of Ns >= 16 after that.  A 32-lane ds_write_b64 covers two 128-byte bank rows
// (modulus 32 dwords = 16 points), so 2 lanes per 8-byte slot is the floor; unswizzled the first pass puts 8 lanes on a slot
// and so does the second.  The index swizzle
//     swz(i) = i ^ (((i >> 4) & 3) << 2) ^ ((i >> 5) & 3)
// changes the low four bits of a point's index by bits 4..6 only: a bijection inside every aligned block of 16, so runs of
// 16 and the aligned 32-point reads (modulus 64 dwords = 32 points; bit 4 is untouched) stay conflict-free, while the
// stride-4 writes land on slots 4 ((j & 3) ^ (j >> 2 & 3)) + (r ^ (j >> 3 & 3)) -- all 16, twice each -- and the runs of 4
// on (t ^ (q >> 1 & 3)) + 4 (r ^ (q & 3)) -- again all 16, twice each.  Frames of fewer than 128 points share a 32-lane group
// and read 2-way; they are the small transforms.
#include <cmath>
#include <vector>

#include "pk_rfft.h"

namespace {

constexpr int RFFT_BLOCK = 256;

__device__ __forceinline__ int swz(int i) { return i ^ (((i >> 4) & 3) << 2) ^ ((i >> 5) & 3); }

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int LOG2N>
struct plan {
    static constexpr int N = 1 << LOG2N;
    static constexpr int M = N / 2;
    static constexpr int LOG2M = LOG2N - 1;
    static constexpr int TPF = M / 4 < RFFT_BLOCK ? M / 4 : RFFT_BLOCK;   // threads per frame
    static constexpr int ROWS = RFFT_BLOCK / TPF;                         // frames per workgroup
    static constexpr int R4 = LOG2M / 2;                                  // radix-4 passes
    static constexpr bool R2 = (LOG2M & 1) != 0;                          // ... and one radix-2 pass
    static constexpr int LDS_POINTS = ROWS * M;                           // per buffer
};

// The passes over one frame: `a` holds the input in swizzled order, the result is in natural order (swizzled) in the
// buffer returned.  t: the thread's index inside its frame.  Every thread of the workgroup must call it (barriers).
template <int LOG2N>
__device__ __forceinline__ float2* fft_passes(float2* a, float2* b, const float2* __restrict__ tw, int t) {
    using P = plan<LOG2N>;
    constexpr int M = P::M, Q = M / 4;
#pragma unroll
    for (int p = 0; p < P::R4; ++p) {
        const int Ns = 1 << (2 * p);
        const int tstep = P::N / (4 * Ns);
        __syncthreads();
#pragma unroll
        for (int j = t; j < Q; j += P::TPF) {
            const int k = j & (Ns - 1);
            const int s = k * tstep;
            const float2 v0 = a[swz(j)];
            const float2 v1 = cmul(a[swz(j + Q)], tw[s]);
            const float2 v2 = cmul(a[swz(j + 2 * Q)], tw[2 * s]);
            const float2 v3 = cmul(a[swz(j + 3 * Q)], tw[3 * s]);
            const float2 b0 = cadd(v0, v2), b1 = csub(v0, v2), b2 = cadd(v1, v3), d = csub(v1, v3);
            const float2 b3 = make_float2(d.y, -d.x);                      // -i (v1 - v3)
            const int j0 = ((j - k) << 2) + k;
            b[swz(j0)] = cadd(b0, b2);
            b[swz(j0 + Ns)] = cadd(b1, b3);
            b[swz(j0 + 2 * Ns)] = csub(b0, b2);
            b[swz(j0 + 3 * Ns)] = csub(b1, b3);
        }
        float2* x = a;
        a = b;
        b = x;
    }
    if (P::R2) {
        constexpr int H = M / 2;
        __syncthreads();
#pragma unroll
        for (int j = t; j < H; j += P::TPF) {
            const float2 v0 = a[swz(j)];
            const float2 v1 = cmul(a[swz(j + H)], tw[2 * j]);
            b[swz(j)] = cadd(v0, v1);
            b[swz(j + H)] = csub(v0, v1);
        }
        float2* x = a;
        a = b;
        b = x;
    }
    __syncthreads();
    return a;
}

template <int LOG2N>
__global__ __launch_bounds__(RFFT_BLOCK) void k_rfft_fwd(const float* __restrict__ x, long stride,
                                                         const float* __restrict__ window, const float2* __restrict__ tw,
                                                         const int* __restrict__ rowmap, long rows, float* __restrict__ out,
                                                         long ldc) {
    using P = plan<LOG2N>;
    constexpr int M = P::M;
    __shared__ float2 lds[2 * P::LDS_POINTS];
    const int f = threadIdx.x / P::TPF, t = threadIdx.x % P::TPF;
    const long row = (long)blockIdx.x * P::ROWS + f;
    long o = -1;
    if (row < rows) o = rowmap ? (long)rowmap[row] : row;
    float2* a = lds + f * M;
    float2* b = lds + P::LDS_POINTS + f * M;
    if (o >= 0) {
        const float2* src = reinterpret_cast<const float2*>(x + row * stride);
        const float2* w2 = reinterpret_cast<const float2*>(window);
#pragma unroll
        for (int m = t; m < M; m += P::TPF) {
            float2 v = src[m];
            if (window) {
                const float2 w = w2[m];
                v.x *= w.x;
                v.y *= w.y;
            }
            a[swz(m)] = v;
        }
    }
    const float2* Z = fft_passes<LOG2N>(a, b, tw, t);
    if (o < 0) return;
    float* re = out + o * ldc;
    float* im = re + (M + 1);
    for (int k = t; k <= M; k += P::TPF) {
        const float2 zk = Z[swz(k & (M - 1))];
        float2 zc = Z[swz((M - k) & (M - 1))];
        zc.y = -zc.y;
        const float2 A = cadd(zk, zc), d = csub(zk, zc);
        const float2 B = make_float2(d.y, -d.x);
        const float2 X = cadd(A, cmul(B, tw[k]));
        re[k] = 0.5f * X.x;
        im[k] = 0.5f * X.y;
    }
}

template <int LOG2N>
__global__ __launch_bounds__(RFFT_BLOCK) void k_rfft_inv(const float* __restrict__ spec, long ld,
                                                         const float* __restrict__ window, const float2* __restrict__ tw,
                                                         long rows, float* __restrict__ out) {
    using P = plan<LOG2N>;
    constexpr int M = P::M;
    __shared__ float2 lds[2 * P::LDS_POINTS];
    const int f = threadIdx.x / P::TPF, t = threadIdx.x % P::TPF;
    const long row = (long)blockIdx.x * P::ROWS + f;
    const bool live = row < rows;
    float2* a = lds + f * M;
    float2* b = lds + P::LDS_POINTS + f * M;
    if (live) {
        const float* re = spec + row * ld;
        const float* im = re + (M + 1);
        for (int k = t; k < M; k += P::TPF) {
            // X[k] and conj(X[M - k]); the imaginary parts of bins 0 and M are not part of a real signal's spectrum
            const float2 xk = make_float2(re[k], k == 0 ? 0.f : im[k]);
            const float2 xc = make_float2(re[M - k], k == 0 ? 0.f : -im[M - k]);
            const float2 w = tw[k];
            const float2 A = cadd(xk, xc);
            const float2 C = cmul(csub(xk, xc), make_float2(w.x, -w.y));
            // conj(Z[k]), Z[k] = A + i C
            a[swz(k)] = make_float2(A.x - C.y, -(A.y + C.x));
        }
    }
    const float2* z = fft_passes<LOG2N>(a, b, tw, t);
    if (!live) return;
    constexpr float scale = 1.0f / (float)P::N;
    float2* dst = reinterpret_cast<float2*>(out + row * P::N);
    const float2* w2 = reinterpret_cast<const float2*>(window);
#pragma unroll
    for (int m = t; m < M; m += P::TPF) {
        const float2 v = z[swz(m)];
        float2 y = make_float2(v.x * scale, -v.y * scale);
        if (window) {
            const float2 w = w2[m];
            y.x *= w.x;
            y.y *= w.y;
        }
        dst[m] = y;
    }
}

int log2_of(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

}  // namespace

int pk_rfft_prepare(pk_ctx* ctx, int n) {
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "rfft: n = %d; the radix FFT takes " PK_RFFT_SIZES, n);
    void*& slot = ctx->rfft_tw[log2_of(n) - 5];
    if (slot) return PK_OK;
    std::vector<float> t((size_t)2 * n);
    for (int i = 0; i < n; ++i) {
        const double ang = -2.0 * M_PI * (double)i / (double)n;
        t[2 * i] = (float)std::cos(ang);
        t[2 * i + 1] = (float)std::sin(ang);
        if ((4 * i) % n == 0) {   // the four axis points exactly: libm's cos(pi / 2) is 6e-17, not 0
            const int q = 4 * i / n;
            t[2 * i] = q == 0 ? 1.f : (q == 2 ? -1.f : 0.f);
            t[2 * i + 1] = q == 1 ? -1.f : (q == 3 ? 1.f : 0.f);
        }
    }
    pk_dbuf buf;
    PK_TRY(pk_upload(ctx, buf, t.data(), t.size() * sizeof(float)));
    slot = buf.p;   // owned by the context from here on (pk_ctx_destroy frees it)
    return PK_OK;
}

#define RFFT_DISPATCH(L2, CALL) \
    switch (L2) {               \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        case 8: CALL(8); break; \
        case 9: CALL(9); break; \
        case 10: CALL(10); break; \
        case 11: CALL(11); break; \
        default: CALL(12); break; \
    }

int pk_rfft_forward(pk_ctx* ctx, const char* name, const float* x, long stride, const float* window, const int* rowmap,
                    long rows, int n, float* out, long ldc) {
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "rfft: n = %d; the radix FFT takes " PK_RFFT_SIZES, n);
    const int l2 = log2_of(n);
    const float2* tw = static_cast<const float2*>(ctx->rfft_tw[l2 - 5]);
    if (!tw) PK_FAIL(PK_ESTATE, "rfft: no twiddle table for n = %d (pk_rfft_prepare was not called)", n);
    if (rows <= 0) return PK_OK;
    const long blocks = (rows + pk_rfft_rows_per_block(n) - 1) / pk_rfft_rows_per_block(n);
    if (blocks > 0x7fffffffL) PK_FAIL(PK_EINVAL, "rfft: more than 2^31 workgroups");
#define CALL(L) \
    PK_LAUNCH(ctx, name, k_rfft_fwd<L>, dim3((unsigned)blocks), dim3(RFFT_BLOCK), 0, x, stride, window, tw, rowmap, rows, out, ldc)
    RFFT_DISPATCH(l2, CALL)
#undef CALL
    return PK_OK;
}

int pk_rfft_inverse(pk_ctx* ctx, const char* name, const float* spec, long ld, const float* window, long rows, int n,
                    float* out) {
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "irfft: n = %d; the radix FFT takes " PK_RFFT_SIZES, n);
    const int l2 = log2_of(n);
    const float2* tw = static_cast<const float2*>(ctx->rfft_tw[l2 - 5]);
    if (!tw) PK_FAIL(PK_ESTATE, "irfft: no twiddle table for n = %d (pk_rfft_prepare was not called)", n);
    if (rows <= 0) return PK_OK;
    const long blocks = (rows + pk_rfft_rows_per_block(n) - 1) / pk_rfft_rows_per_block(n);
    if (blocks > 0x7fffffffL) PK_FAIL(PK_EINVAL, "irfft: more than 2^31 workgroups");
#define CALL(L) \
    PK_LAUNCH(ctx, name, k_rfft_inv<L>, dim3((unsigned)blocks), dim3(RFFT_BLOCK), 0, spec, ld, window, tw, rows, out)
    RFFT_DISPATCH(l2, CALL)
#undef CALL
    return PK_OK;
}

extern "C" int pk_rfft_supported(int32_t n) { return pk_rfft_size_ok(n) ? 1 : 0; }

extern "C" int pk_rfft_tile_rows(int32_t n, int32_t* rows) {
    if (!rows) PK_FAIL(PK_EINVAL, "pk_rfft_tile_rows: NULL argument");
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "pk_rfft_tile_rows: n = %d; the radix FFT takes " PK_RFFT_SIZES, (int)n);
    *rows = pk_rfft_rows_per_block(n);
    return PK_OK;
}

extern "C" int pk_op_rfft(pk_ctx* ctx, const float* x, int64_t rows, int32_t n, float* out) {
    if (!ctx || !out || (!x && rows > 0)) PK_FAIL(PK_EINVAL, "pk_op_rfft: NULL argument");
    if (rows < 0) PK_FAIL(PK_EINVAL, "pk_op_rfft: rows must not be negative");
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "pk_op_rfft: n = %d; the radix FFT takes " PK_RFFT_SIZES, (int)n);
    if (((uintptr_t)x | (uintptr_t)out) % 8 != 0) PK_FAIL(PK_EINVAL, "pk_op_rfft: x and out must be 8-byte aligned");
    PK_DEVICE(ctx->device);
    PK_TRY(pk_rfft_prepare(ctx, n));
    return pk_rfft_forward(ctx, "op_rfft", x, n, nullptr, nullptr, rows, n, out, n + 2);
}

extern "C" int pk_op_irfft(pk_ctx* ctx, const float* spec, int64_t rows, int32_t n, float* out) {
    if (!ctx || !out || (!spec && rows > 0)) PK_FAIL(PK_EINVAL, "pk_op_irfft: NULL argument");
    if (rows < 0) PK_FAIL(PK_EINVAL, "pk_op_irfft: rows must not be negative");
    if (!pk_rfft_size_ok(n)) PK_FAIL(PK_EUNSUPPORTED, "pk_op_irfft: n = %d; the radix FFT takes " PK_RFFT_SIZES, (int)n);
    if ((uintptr_t)out % 8 != 0) PK_FAIL(PK_EINVAL, "pk_op_irfft: out must be 8-byte aligned");
    PK_DEVICE(ctx->device);
    PK_TRY(pk_rfft_prepare(ctx, n));
    return pk_rfft_inverse(ctx, "op_irfft", spec, n + 2, nullptr, rows, n, out);
}
