// trim.hip -- silence trimming of ragged batches on gfx950: framed power, the non-silent frame test of
// librosa.effects.trim / split with (start, end) per utterance, the steps of the reference's trim_long_silences after its
// voice detector (moving average, rounding, dilation, gather) with an energy detector of this project's own in front
// (NOT webrtcvad), and peak normalisation.  Geometry, the accumulation order of a frame's power and the envelope: pk_trim.h.
//
// k_frame_power: one workgroup stages a tile of T frames of one utterance in LDS (16-byte global reads where the source
// is aligned; the edges by reflection or zeros, the packed buffer's neighbours are never read); one wave sums a frame.
// k_trim_utt:    one workgroup per utterance: the maximum of P, then the non-silent flags, the first and the last of them.
// k_vad_mask:    one workgroup per utterance walks its windows in chunks of 256 with a carry: voice flags (from the window
//                powers or from the caller), the windowed count, the mask, the dilation, an exclusive scan of the kept windows.
// k_vad_gather:  one wave copies a kept window to its place in the packed output.
// k_peak_max / k_peak_div: max |y| per utterance (an integer maximum of the bit patterns: exact in any order), then y / max.
#include <vector>

#include "pk_common.h"
#include "pk_trim.h"

namespace {

struct tr_utt {
    long xoff;      // first sample of the utterance in the packed input
    long foff;      // first frame (window) in the packed per-frame arrays
    long ooff;      // first sample in the packed output of the gather
    int n_in;
    int n_frames;
};

constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_NONE = 0x7fffffff;
constexpr double TR_AMIN = 1e-10;       // librosa's amin of power_to_db

// v op'ed over the workgroup; sm holds TR_WAVES values and may be reused right after the call
template <class V, class Op>
__device__ __forceinline__ V tr_block_reduce(V v, Op op, V* sm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    V r = sm[0];
#pragma unroll
    for (int k = 1; k < TR_WAVES; ++k) r = op(r, sm[k]);
    return r;
}

// the number of leading floats before p reaches a 16-byte boundary, at most n
__device__ __forceinline__ int tr_head(const float* p, long n) {
    const long h = (long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return (int)(h < n ? h : n);
}

__global__ __launch_bounds__(TR_THREADS) void k_frame_power(const float* __restrict__ x, const tr_utt* __restrict__ utts,
                                                            float* __restrict__ P, int Lf, int hop, int mode, int T, int rms) {
    extern __shared__ __attribute__((aligned(16))) float xs[];   // xs[s] = x~[fr0 * hop - pad + s]
    const tr_utt u = utts[blockIdx.y];
    const int fr0 = blockIdx.x * T;                    // the tile's first frame
    if (fr0 >= u.n_frames) return;                     // (uniform over the workgroup)
    const int nf = u.n_frames - fr0 < T ? u.n_frames - fr0 : T;
    const int span = (nf - 1) * hop + Lf;              // <= (T - 1) * hop + Lf floats, the launch's LDS
    const int pad = mode == TR_PAD_NONE ? 0 : Lf / 2;
    const long N = u.n_in;
    const long m0 = (long)fr0 * hop - pad;             // xs[s] is sample m0 + s
    const float* xu = x + u.xoff;
    const int tid = threadIdx.x;
    // [lo, hi): the staged samples inside the utterance
    long lo_l = m0 < 0 ? -m0 : 0;
    lo_l = lo_l < span ? lo_l : span;
    long hi_l = N - m0;
    hi_l = hi_l > span ? span : hi_l;
    hi_l = hi_l < lo_l ? lo_l : hi_l;
    const int lo = (int)lo_l, hi = (int)hi_l;
    const int n_edge = lo + (span - hi);
    for (int e = tid; e < n_edge; e += TR_THREADS) {
        const int s = e < lo ? e : hi + (e - lo);
        long m = m0 + s;
        m = m < 0 ? -m : 2 * (N - 1) - m;              // numpy's reflect: the edge sample is not repeated
        xs[s] = (mode == TR_PAD_REFLECT && m >= 0 && m < N) ? xu[m] : 0.f;
    }
    {
        const int n = hi - lo;
        const float* src = xu + (m0 + lo);
        float* dst = xs + lo;
        const int head = tr_head(src, n);
        if (tid < head) dst[tid] = src[tid];
        const int nv = (n - head) >> 2;
        const float4* sv = reinterpret_cast<const float4*>(src + head);
        for (int v = tid; v < nv; v += TR_THREADS) {
            const float4 q = sv[v];
            float* d = dst + head + 4 * v;
            d[0] = q.x;
            d[1] = q.y;
            d[2] = q.z;
            d[3] = q.w;
        }
        const int i = head + 4 * nv + tid;
        if (i < n) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < nf; f += TR_WAVES) {        // THE ORDER of pk_trim.h
        const float* xf = xs + f * hop;
        float acc = 0.f;
        for (int j = lane; j < Lf; j += 64) {
            const float v = xf[j];
            acc = __builtin_fmaf(v, v, acc);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) {
            const float p = acc / (float)Lf;               // (IEEE division and square root: hipcc's default)
            P[u.foff + fr0 + f] = rms ? sqrtf(p) : p;
        }
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_trim_utt(const float* __restrict__ P, const tr_utt* __restrict__ utts,
                                                         unsigned char* __restrict__ flags, int* __restrict__ bounds, int hop,
                                                         double factor) {
    __shared__ float smf[TR_WAVES];
    __shared__ int smi[TR_WAVES];
    const tr_utt u = utts[blockIdx.x];
    const float* p = P + u.foff;
    const int n = u.n_frames, tid = threadIdx.x;
    float mx = 0.f;                                    // P >= 0
    for (int i = tid; i < n; i += TR_THREADS) mx = fmaxf(mx, p[i]);
    mx = tr_block_reduce(mx, [](float a, float b) { return fmaxf(a, b); }, smf);
    const double thr = fmax(TR_AMIN, (double)mx) * factor;
    int first = TR_NONE, last = -1;
    for (int i = tid; i < n; i += TR_THREADS) {
        const bool ns = fmax(TR_AMIN, (double)p[i]) > thr;
        if (flags) flags[u.foff + i] = ns ? 1 : 0;
        if (ns) {
            first = i < first ? i : first;
            last = i;
        }
    }
    first = tr_block_reduce(first, [](int a, int b) { return a < b ? a : b; }, smi);
    last = tr_block_reduce(last, [](int a, int b) { return a > b ? a : b; }, smi);
    if (tid == 0 && bounds) {
        const long end = ((long)last + 1) * hop;
        bounds[2 * blockIdx.x] = last < 0 ? 0 : (int)((long)first * hop);
        bounds[2 * blockIdx.x + 1] = last < 0 ? 0 : (int)(end < u.n_in ? end : u.n_in);
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_vad_mask(const float* __restrict__ Q, const unsigned char* __restrict__ given,
                                                         const tr_utt* __restrict__ utts, unsigned char* __restrict__ flags_out,
                                                         int* __restrict__ pos, int* __restrict__ counts, int W, int S, double rel,
                                                         double floor_p) {
    constexpr int CH = TR_SCAN_CHUNK;
    static_assert(CH == TR_THREADS, "one window per thread");
    __shared__ unsigned char sf[CH + 4 * TR_HALO];     // voice flags of windows k0 - 64 ... k0 + CH + 63
    __shared__ unsigned char sm[CH + 2 * TR_HALO];     // mask of windows k0 - 32 ... k0 + CH + 31
    __shared__ float smf[TR_WAVES];
    __shared__ int swv[TR_WAVES];
    const tr_utt u = utts[blockIdx.x];
    const int n = u.n_frames, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* q = Q ? Q + u.foff : nullptr;
    const unsigned char* gv = given ? given + u.foff : nullptr;
    double thr = 0.0;
    if (q) {                                           // (uniform)
        float mx = 0.f;
        for (int i = tid; i < n; i += TR_THREADS) mx = fmaxf(mx, q[i]);
        mx = tr_block_reduce(mx, [](float a, float b) { return fmaxf(a, b); }, smf);
        thr = fmax((double)mx * rel, floor_p);
    }
    const int a_lo = (W - 1) / 2, a_hi = W / 2;        // the count reads flags k - a_lo ... k + a_hi
    const int L = S + 1;
    const int d_lo = L - 1 - L / 2, d_hi = L / 2;      // the dilation reads the mask k - d_lo ... k + d_hi
    int carry = 0;                                     // kept windows before the chunk
    for (int k0 = 0; k0 < n; k0 += CH) {
        for (int e = tid; e < CH + 4 * TR_HALO; e += TR_THREADS) {
            const int k = k0 - 2 * TR_HALO + e;
            unsigned char f = 0;
            if (k >= 0 && k < n) f = q ? ((double)q[k] > thr ? 1 : 0) : (gv[k] != 0 ? 1 : 0);
            sf[e] = f;
        }
        __syncthreads();
        for (int e = tid; e < CH + 2 * TR_HALO; e += TR_THREADS) {
            const int k = k0 - TR_HALO + e;
            int c = 0;
            for (int d = -a_lo; d <= a_hi; ++d) c += sf[e + TR_HALO + d];
            sm[e] = (k >= 0 && k < n && 2 * c > W) ? 1 : 0;
        }
        __syncthreads();
        const int k = k0 + tid;
        bool keep = false;
        for (int d = -d_lo; d <= d_hi; ++d) keep = keep || sm[tid + TR_HALO + d] != 0;
        keep = keep && k < n;
        int incl = keep ? 1 : 0;                       // kept windows of the wave up to and including this lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const int before = incl - (keep ? 1 : 0);
        if (lane == 63) swv[wave] = incl;
        __syncthreads();
        int base = carry, total = 0;
#pragma unroll
        for (int v = 0; v < TR_WAVES; ++v) {
            base += v < wave ? swv[v] : 0;
            total += swv[v];
        }
        if (k < n) {
            pos[u.foff + k] = keep ? base + before : -1;
            if (flags_out) flags_out[u.foff + k] = sf[tid + 2 * TR_HALO];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(TR_THREADS) void k_vad_gather(const float* __restrict__ x, const tr_utt* __restrict__ utts,
                                                           const int* __restrict__ pos, float* __restrict__ out, int w) {
    const tr_utt u = utts[blockIdx.y];
    const int k0 = blockIdx.x * TR_GATHER_WINDOWS;
    if (k0 >= u.n_frames) return;
    const int k1 = k0 + TR_GATHER_WINDOWS < u.n_frames ? k0 + TR_GATHER_WINDOWS : u.n_frames;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = k0 + wave; k < k1; k += TR_WAVES) {
        const int p = pos[u.foff + k];                 // (uniform over the wave)
        if (p < 0) continue;
        const float* src = x + u.xoff + (long)k * w;
        float* dst = out + u.ooff + (long)p * w;
        if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) != 0) {   // not aligned alike: 4-byte accesses
            for (int i = lane; i < w; i += 64) dst[i] = src[i];
            continue;
        }
        const int head = tr_head(src, w);
        if (lane < head) dst[lane] = src[lane];
        const int nv = (w - head) >> 2;
        const float4* sv = reinterpret_cast<const float4*>(src + head);
        float4* dv = reinterpret_cast<float4*>(dst + head);
        for (int v = lane; v < nv; v += 64) dv[v] = sv[v];
        const int i = head + 4 * nv + lane;
        if (i < w) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_peak_max(const float* __restrict__ x, const tr_utt* __restrict__ utts,
                                                         unsigned* __restrict__ amax) {
    __shared__ unsigned smu[TR_WAVES];
    const tr_utt u = utts[blockIdx.y];
    const long t0 = (long)blockIdx.x * TR_NORM_TILE;
    if (t0 >= u.n_in) return;
    const int n = (int)(u.n_in - t0 < TR_NORM_TILE ? u.n_in - t0 : TR_NORM_TILE);
    const float* src = x + u.xoff + t0;
    const int tid = threadIdx.x;
    const unsigned ABS = 0x7fffffffu;                  // |y| as its bit pattern: ordered like the value, a NaN above all
    unsigned m = 0;
    const int head = tr_head(src, n);
    if (tid < head) m = __float_as_uint(src[tid]) & ABS;
    const int nv = (n - head) >> 2;
    const float4* sv = reinterpret_cast<const float4*>(src + head);
    for (int v = tid; v < nv; v += TR_THREADS) {
        const float4 q = sv[v];
        const unsigned a = __float_as_uint(q.x) & ABS, b = __float_as_uint(q.y) & ABS, c = __float_as_uint(q.z) & ABS,
                       d = __float_as_uint(q.w) & ABS;
        const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
        const unsigned e = ab > cd ? ab : cd;
        m = e > m ? e : m;
    }
    const int i = head + 4 * nv + tid;
    if (i < n) {
        const unsigned a = __float_as_uint(src[i]) & ABS;
        m = a > m ? a : m;
    }
    m = tr_block_reduce(m, [](unsigned a, unsigned b) { return a > b ? a : b; }, smu);
    if (tid == 0) atomicMax(amax + blockIdx.y, m);
}

__global__ __launch_bounds__(TR_THREADS) void k_peak_div(const float* __restrict__ x, const tr_utt* __restrict__ utts,
                                                         const unsigned* __restrict__ amax, float* __restrict__ out) {
    const tr_utt u = utts[blockIdx.y];
    const long t0 = (long)blockIdx.x * TR_NORM_TILE;
    if (t0 >= u.n_in) return;
    const int n = (int)(u.n_in - t0 < TR_NORM_TILE ? u.n_in - t0 : TR_NORM_TILE);
    const float* src = x + u.xoff + t0;
    float* dst = out + u.xoff + t0;
    const int tid = threadIdx.x;
    const float m = __uint_as_float(amax[blockIdx.y]);
    const bool leave = m < 1.17549435e-38f;            // below the smallest normal number: the utterance as it is
    auto f = [&](float v) { return leave ? v : v / m; };
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) != 0) {
        for (int i = tid; i < n; i += TR_THREADS) dst[i] = f(src[i]);
        return;
    }
    const int head = tr_head(src, n);
    if (tid < head) dst[tid] = f(src[tid]);
    const int nv = (n - head) >> 2;
    const float4* sv = reinterpret_cast<const float4*>(src + head);
    float4* dv = reinterpret_cast<float4*>(dst + head);
    for (int v = tid; v < nv; v += TR_THREADS) {
        float4 q = sv[v];
        q.x = f(q.x);
        q.y = f(q.y);
        q.z = f(q.z);
        q.w = f(q.w);
        dv[v] = q;
    }
    const int i = head + 4 * nv + tid;
    if (i < n) dst[i] = f(src[i]);
}

constexpr int GRID_Y = 32768;                          // utterances per launch (grid.y is a 16-bit quantity)
constexpr int GRID_X = 1 << 20;

}  // namespace

struct pk_trim {
    pk_ctx* ctx = nullptr;
    pk_dbuf ws_utt, ws_pow, ws_cnt;
};

// the table of a call: offsets of every utterance in the packed arrays; uploaded, and the stream synchronised (the host
// vector leaves scope with the caller)
static int tr_upload(pk_trim* h, const std::vector<tr_utt>& tab) {
    PK_TRY(h->ws_utt.reserve(tab.size() * sizeof(tr_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utt.p, tab.data(), tab.size() * sizeof(tr_utt), hipMemcpyHostToDevice, h->ctx->stream));
    PK_HIP(hipStreamSynchronize(h->ctx->stream));
    return PK_OK;
}

static int tr_check_frames(const char* who, int Lf, int hop, int mode) {
    if (mode != TR_PAD_NONE && mode != TR_PAD_REFLECT && mode != TR_PAD_CONSTANT)
        PK_FAIL(PK_EINVAL, "%s: pad_mode = %d is not one of 0 (no padding), 1 (reflect), 2 (constant)", who, mode);
    if (Lf < 1 || Lf > TR_MAX_FRAME)
        PK_FAIL(PK_EUNSUPPORTED, "%s: a frame of %d samples; the engine's envelope is 1 ... %d", who, Lf, TR_MAX_FRAME);
    if (hop < 1 || hop > Lf) PK_FAIL(PK_EUNSUPPORTED, "%s: hop = %d; the engine's envelope is 1 ... frame_length = %d", who, hop, Lf);
    return PK_OK;
}

static int tr_frame_table(const char* who, const int32_t* lens, int B, int Lf, int hop, int mode, std::vector<tr_utt>& tab,
                          long& sum_fr, long& max_fr) {
    long sum_in = 0;
    sum_fr = max_fr = 0;
    tab.resize(B);
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "%s: utterance %d is empty (%d samples)", who, b, (int)lens[b]);
        if (mode == TR_PAD_REFLECT && lens[b] <= Lf / 2)
            PK_FAIL(PK_EINVAL, "%s: utterance %d has %d samples; reflect padding needs more than frame_length / 2 = %d", who, b,
                    (int)lens[b], Lf / 2);
        const long nf = tr_num_frames(lens[b], Lf, hop, mode);
        if (nf > 0x7fffffffL) PK_FAIL(PK_EINVAL, "%s: utterance %d has more than 2^31 - 1 frames", who, b);
        tab[b] = {sum_in, sum_fr, 0, lens[b], (int)nf};
        sum_in += lens[b];
        sum_fr += nf;
        max_fr = nf > max_fr ? nf : max_fr;
    }
    return PK_OK;
}

static int tr_launch_power(pk_trim* h, const float* wav, int B, int Lf, int hop, int mode, long max_fr, float* power, int rms) {
    if (max_fr == 0) return PK_OK;
    pk_ctx* ctx = h->ctx;
    const int T = tr_tile_frames(Lf, hop);
    const size_t lds = ((size_t)(T - 1) * hop + Lf) * sizeof(float);
    const long tiles = (max_fr + T - 1) / T;
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        PK_LAUNCH(ctx, "trim_power", k_frame_power, dim3((unsigned)tiles, (unsigned)nb), dim3(TR_THREADS), lds, wav,
                  h->ws_utt.as<tr_utt>() + b0, power, Lf, hop, mode, T, rms);
    }
    return PK_OK;
}

extern "C" int pk_trim_create(pk_ctx* ctx, pk_trim** out) {
    if (!ctx || !out) PK_FAIL(PK_EINVAL, "pk_trim_create: NULL argument");
    pk_trim* h = new pk_trim();
    h->ctx = ctx;
    *out = h;
    return PK_OK;
}

extern "C" void pk_trim_destroy(pk_trim* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->ws_utt, &h->ws_pow, &h->ws_cnt};
    for (auto* b : bufs) b->release();
    delete h;
}

extern "C" int pk_trim_num_frames(int64_t n_samples, int32_t frame_length, int32_t hop, int32_t pad_mode, int64_t* frames) {
    if (!frames) PK_FAIL(PK_EINVAL, "pk_trim_num_frames: NULL argument");
    PK_TRY(tr_check_frames("pk_trim_num_frames", frame_length, hop, pad_mode));
    if (n_samples < 0 || n_samples > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_trim_num_frames: n_samples must be in 0 ... 2^31 - 1");
    *frames = tr_num_frames(n_samples, frame_length, hop, pad_mode);
    return PK_OK;
}

extern "C" int pk_trim_tile_frames(int32_t frame_length, int32_t hop, int32_t* tile) {
    if (!tile) PK_FAIL(PK_EINVAL, "pk_trim_tile_frames: NULL argument");
    PK_TRY(tr_check_frames("pk_trim_tile_frames", frame_length, hop, TR_PAD_NONE));
    *tile = tr_tile_frames(frame_length, hop);
    return PK_OK;
}

extern "C" int pk_trim_run(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t frame_length, int32_t hop,
                           int32_t pad_mode, double factor, int32_t rms, float* power_out, uint8_t* flags_out,
                           int32_t* bounds_out) {
    if (!h || !wav || !lens) PK_FAIL(PK_EINVAL, "pk_trim_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_trim_run: batch size must be positive");
    if (!power_out && !flags_out && !bounds_out) PK_FAIL(PK_EINVAL, "pk_trim_run: no output is asked for");
    if (rms && (flags_out || bounds_out)) PK_FAIL(PK_EINVAL, "pk_trim_run: the frame test reads the power, not its square root");
    if ((flags_out || bounds_out) && !(factor == factor)) PK_FAIL(PK_EINVAL, "pk_trim_run: the threshold factor is not a number");
    PK_TRY(tr_check_frames("pk_trim_run", frame_length, hop, pad_mode));
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    std::vector<tr_utt> tab;
    long sum_fr, max_fr;
    PK_TRY(tr_frame_table("pk_trim_run", lens, B, frame_length, hop, pad_mode, tab, sum_fr, max_fr));
    float* d_pow = power_out;
    if (!d_pow) {
        PK_TRY(h->ws_pow.reserve((size_t)(sum_fr > 0 ? sum_fr : 1) * sizeof(float)));
        d_pow = h->ws_pow.as<float>();
    }
    PK_TRY(tr_upload(h, tab));
    PK_TRY(tr_launch_power(h, wav, B, frame_length, hop, pad_mode, max_fr, d_pow, rms));
    if (flags_out || bounds_out) {
        for (int b0 = 0; b0 < B; b0 += GRID_X) {
            const int nb = B - b0 < GRID_X ? B - b0 : GRID_X;
            PK_LAUNCH(ctx, "trim_utt", k_trim_utt, dim3(nb), dim3(TR_THREADS), 0, d_pow, h->ws_utt.as<tr_utt>() + b0, flags_out,
                      bounds_out ? bounds_out + 2 * (long)b0 : nullptr, hop, factor);
        }
    }
    return PK_OK;
}

extern "C" int pk_vad_mask(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t window, int32_t avg_width,
                           int32_t max_silence, const uint8_t* voice_flags, double rel, double floor_power, float* power_out,
                           uint8_t* flags_out, int32_t* pos_out, int32_t* kept) {
    if (!h || !lens || !pos_out || !kept) PK_FAIL(PK_EINVAL, "pk_vad_mask: NULL argument");
    if (!wav && !voice_flags) PK_FAIL(PK_EINVAL, "pk_vad_mask: neither samples nor voice flags");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_vad_mask: batch size must be positive");
    if (window < 1 || window > TR_MAX_FRAME)
        PK_FAIL(PK_EUNSUPPORTED, "vad: a window of %d samples; the engine's envelope is 1 ... %d", (int)window, TR_MAX_FRAME);
    if (avg_width < 1 || avg_width > TR_MAX_AVG)
        PK_FAIL(PK_EUNSUPPORTED, "vad: a moving average over %d windows; the engine's envelope is 1 ... %d", (int)avg_width,
                TR_MAX_AVG);
    if (max_silence < 0 || max_silence > TR_MAX_SILENCE)
        PK_FAIL(PK_EUNSUPPORTED, "vad: max_silence_length = %d windows; the engine's envelope is 0 ... %d", (int)max_silence,
                TR_MAX_SILENCE);
    if (!voice_flags && !(rel == rel && floor_power == floor_power)) PK_FAIL(PK_EINVAL, "vad: a threshold is not a number");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    std::vector<tr_utt> tab;
    long sum_fr, max_fr;
    PK_TRY(tr_frame_table("pk_vad_mask", lens, B, window, window, TR_PAD_NONE, tab, sum_fr, max_fr));
    float* d_pow = nullptr;
    if (!voice_flags) {
        d_pow = power_out;
        if (!d_pow) {
            PK_TRY(h->ws_pow.reserve((size_t)(sum_fr > 0 ? sum_fr : 1) * sizeof(float)));
            d_pow = h->ws_pow.as<float>();
        }
    }
    PK_TRY(h->ws_cnt.reserve((size_t)B * sizeof(int)));
    PK_TRY(tr_upload(h, tab));
    if (d_pow) PK_TRY(tr_launch_power(h, wav, B, window, window, TR_PAD_NONE, max_fr, d_pow, 0));
    for (int b0 = 0; b0 < B; b0 += GRID_X) {
        const int nb = B - b0 < GRID_X ? B - b0 : GRID_X;
        PK_LAUNCH(ctx, "vad_mask", k_vad_mask, dim3(nb), dim3(TR_THREADS), 0, (const float*)d_pow, voice_flags,
                  h->ws_utt.as<tr_utt>() + b0, flags_out, pos_out, h->ws_cnt.as<int>() + b0, (int)avg_width, (int)max_silence, rel,
                  floor_power);
    }
    PK_HIP(hipMemcpyAsync(kept, h->ws_cnt.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PK_HIP(hipStreamSynchronize(ctx->stream));
    return PK_OK;
}

extern "C" int pk_vad_gather(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t window, const int32_t* pos,
                             const int32_t* kept, float* out) {
    if (!h || !wav || !lens || !pos || !kept || !out) PK_FAIL(PK_EINVAL, "pk_vad_gather: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_vad_gather: batch size must be positive");
    if (window < 1 || window > TR_MAX_FRAME)
        PK_FAIL(PK_EUNSUPPORTED, "vad: a window of %d samples; the engine's envelope is 1 ... %d", (int)window, TR_MAX_FRAME);
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    std::vector<tr_utt> tab;
    long sum_fr, max_fr;
    PK_TRY(tr_frame_table("pk_vad_gather", lens, B, window, window, TR_PAD_NONE, tab, sum_fr, max_fr));
    long sum_out = 0;
    for (int b = 0; b < B; ++b) {
        if (kept[b] < 0 || kept[b] > tab[b].n_frames)
            PK_FAIL(PK_EINVAL, "pk_vad_gather: utterance %d keeps %d of %d windows", b, (int)kept[b], tab[b].n_frames);
        tab[b].ooff = sum_out;
        sum_out += (long)kept[b] * window;
    }
    if (max_fr == 0 || sum_out == 0) return PK_OK;
    PK_TRY(tr_upload(h, tab));
    const long tiles = (max_fr + TR_GATHER_WINDOWS - 1) / TR_GATHER_WINDOWS;
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        PK_LAUNCH(ctx, "vad_gather", k_vad_gather, dim3((unsigned)tiles, (unsigned)nb), dim3(TR_THREADS), 0, wav,
                  h->ws_utt.as<tr_utt>() + b0, pos, out, (int)window);
    }
    return PK_OK;
}

extern "C" int pk_peak_normalize(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, float* out) {
    if (!h || !wav || !lens || !out) PK_FAIL(PK_EINVAL, "pk_peak_normalize: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_peak_normalize: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    std::vector<tr_utt> tab(B);
    long sum_in = 0, max_in = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "pk_peak_normalize: utterance %d is empty (%d samples)", b, (int)lens[b]);
        tab[b] = {sum_in, 0, 0, lens[b], 0};
        sum_in += lens[b];
        max_in = lens[b] > max_in ? lens[b] : max_in;
    }
    PK_TRY(h->ws_cnt.reserve((size_t)B * sizeof(unsigned)));
    PK_TRY(tr_upload(h, tab));
    PK_HIP(hipMemsetAsync(h->ws_cnt.p, 0, (size_t)B * sizeof(unsigned), ctx->stream));
    const long tiles = (max_in + TR_NORM_TILE - 1) / TR_NORM_TILE;
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        PK_LAUNCH(ctx, "peak_max", k_peak_max, dim3((unsigned)tiles, (unsigned)nb), dim3(TR_THREADS), 0, wav,
                  h->ws_utt.as<tr_utt>() + b0, h->ws_cnt.as<unsigned>() + b0);
        PK_LAUNCH(ctx, "peak_div", k_peak_div, dim3((unsigned)tiles, (unsigned)nb), dim3(TR_THREADS), 0, wav,
                  h->ws_utt.as<tr_utt>() + b0, (const unsigned*)(h->ws_cnt.as<unsigned>() + b0), out);
    }
    return PK_OK;
}
