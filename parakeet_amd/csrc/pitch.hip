// pitch.hip -- frame-level f0 of ragged batches on gfx950: the estimator of DESIGN.md 4.5e (difference function, cumulative-mean
// normalisation, absolute threshold, parabolic refinement -- NOT pyworld's DIO + StoneMask), and the reference's
// continuous-f0 / log step for f0 from any estimator.  Geometry: pk_pitch.h.
//
// k_pitch: one workgroup owns one tile of F frames of one utterance.  It stages the tile's samples in LDS (samples outside the
// utterance are zeros by a select, the packed buffer's neighbours are never read).  Phase 1: a work item (frame, lag group)
// sums (x[s + j] - x[s + j + tau])^2 over j ascending, one fp32 FMA chain per lag, R lags per item; d goes to LDS.  Phase 2:
// one wave per frame turns its row of d into d' (a prefix sum over tau in chunks of 64 lags: a shuffle scan inside the
// chunk, then the carry of the chunks before it), finds the first lag under the threshold and the end of the descent that
// follows as min-reductions over the lanes, and lane 0 refines.  Every sum has one fixed order that involves neither the
// batch, nor the tile's position, nor the grid: a frame's result is the same bits wherever it is computed.
//
// k_cont_f0: one workgroup per utterance walks its track in chunks of 256 frames, forwards with a max-scan of "last voiced
// index" (kept per frame in a workspace), then backwards with a min-scan of "next voiced index", and writes the result.
//
// k_pitch_cand, k_pitch_viterbi: a second decision stage on the d' rows k_pitch wrote -- a frame's local minima as candidates
// and the cheapest path over them ("Viterbi tracking over candidates"); described where they stand below.
#include <cmath>
#include <vector>

#include "pk_common.h"
#include "pk_pitch.h"

namespace {

struct pt_utt {
    long xoff;      // first sample of the utterance in the packed input
    long foff;      // first frame in the packed outputs
    int n_in;
    int n_frames;
};

constexpr int PT_NONE = 0x7fffffff;

__device__ __forceinline__ int pt_wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(PT_THREADS) void k_pitch(const float* __restrict__ x, const pt_utt* __restrict__ utts,
                                                      float* __restrict__ f0_out, int* __restrict__ lag_out,
                                                      float* __restrict__ cmnd_out, int hop, int tau_min, int tau_max, int W,
                                                      int G, int F, int span, float threshold, double sr) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int R = PT_R;
    float* xs = lds;                       // span staged samples: xs[k] = x~[fr0 * hop - L / 2 + k]
    float* dl = lds + span;                // F rows of tau_max + 1: d, then d'
    const pt_utt u = utts[blockIdx.y];
    const int fr0 = blockIdx.x * F;        // the tile's first frame
    if (fr0 >= u.n_frames) return;         // (uniform over the workgroup)
    const int nf = u.n_frames - fr0 < F ? u.n_frames - fr0 : F;
    const int row = tau_max + 1;
    const long m0 = (long)fr0 * hop - (W + tau_max) / 2;
    const float* xu = x + u.xoff;
    for (int s = threadIdx.x; s < span; s += PT_THREADS) {
        const long m = m0 + s;
        xs[s] = (m >= 0 && m < u.n_in) ? xu[m] : 0.f;
    }
    __syncthreads();
    // ---- phase 1: the difference function
    const int n_items = nf * G;
    for (int it = threadIdx.x; it < n_items; it += PT_THREADS) {
        const int f = it / G, g = it - f * G;
        const int tau0 = 1 + g * R;
        const float* xr = xs + f * hop;    // xr[j] = x~[s + j]
        const float* xw = xr + tau0;       // xw[j + q] = x~[s + j + tau0 + q]
        float acc[R], w[R];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = 0.f;
#pragma unroll
        for (int q = 0; q < R - 1; ++q) w[q] = xw[q];
        w[R - 1] = 0.f;
        int j = 0;
        for (; j + R <= W; j += R) {
#pragma unroll
            for (int t = 0; t < R; ++t) {              // step j + t: the window's slot (t + q) % R holds xw[j + t + q]
                w[(t + R - 1) % R] = xw[j + t + R - 1];
                const float r = xr[j + t];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float e = r - w[(t + q) % R];
                    acc[q] = __builtin_fmaf(e, e, acc[q]);
                }
            }
        }
        for (; j < W; ++j) {                           // the last W % R steps: the same chain, read directly
            const float r = xr[j];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float e = r - xw[j + q];
                acc[q] = __builtin_fmaf(e, e, acc[q]);
            }
        }
        float* dr = dl + f * row;
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (tau0 + q <= tau_max) dr[tau0 + q] = acc[q];
    }
    __syncthreads();
    // ---- phase 2: one wave per frame
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int fb = 0; fb < F; fb += PT_THREADS / 64) {  // (uniform trip count: the barriers below are reached by every wave)
        const int f = fb + wave;
        const bool live = f < nf;
        float* dr = dl + (live ? f : 0) * row;
        if (live) {
            float carry = 0.f;
            for (int base = 0; base < tau_max; base += 64) {
                const int tau = base + lane + 1;
                const float d = tau <= tau_max ? dr[tau] : 0.f;
                float s = d;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float o = __shfl_up(s, off, 64);
                    if (lane >= off) s += o;
                }
                const float c = carry + s;
                carry = __shfl(c, 63, 64);
                if (tau <= tau_max) dr[tau] = c > 0.f ? (d * (float)tau) / c : 1.f;
            }
            if (lane == 0) dr[0] = 1.f;
        }
        __syncthreads();
        if (live) {
            const long fr = u.foff + fr0 + f;
            if (cmnd_out)
                for (int t = lane; t < row; t += 64) cmnd_out[fr * row + t] = dr[t];
            int t0 = PT_NONE;
            for (int t = tau_min + lane; t <= tau_max - 1; t += 64)
                if (dr[t] < threshold) {
                    t0 = t;
                    break;
                }
            t0 = pt_wave_min(t0);
            int ts = PT_NONE;
            if (t0 != PT_NONE) {                       // (uniform over the wave)
                for (int t = t0 + lane; t <= tau_max - 1; t += 64)
                    if (!(t + 1 <= tau_max - 1 && dr[t + 1] < dr[t])) {
                        ts = t;
                        break;
                    }
                ts = pt_wave_min(ts);                  // tau_max - 1 always stops: ts is a lag
            }
            if (lane == 0) {
                float f0 = 0.f;
                int lag = 0;
                if (ts != PT_NONE) {
                    const double a = dr[ts - 1], b = dr[ts], c = dr[ts + 1];
                    const double den = a - 2.0 * b + c;
                    const double delta = (a >= b && c >= b && den > 0.0) ? (a - c) / (2.0 * den) : 0.0;
                    f0 = (float)(sr / ((double)ts + delta));
                    lag = ts;
                }
                f0_out[fr] = f0;
                if (lag_out) lag_out[fr] = lag;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PT_SCAN_CHUNK) void k_cont_f0(const float* __restrict__ f0, const pt_utt* __restrict__ utts,
                                                           int* __restrict__ prev, float* __restrict__ out, int log_flag) {
    __shared__ int sm[PT_SCAN_CHUNK];
    const pt_utt u = utts[blockIdx.x];
    const float* f = f0 + u.foff;
    float* o = out + u.foff;
    int* pv = prev + u.foff;
    const int n = u.n_frames, tid = threadIdx.x;
    const int chunks = (n + PT_SCAN_CHUNK - 1) / PT_SCAN_CHUNK;
    if (log_flag & 2) {                                // no filling (uniform): the log step alone
        for (int i = tid; i < n; i += PT_SCAN_CHUNK) {
            float v = f[i];
            if ((log_flag & 1) && v != 0.f) v = (float)log((double)v);
            o[i] = v;
        }
        return;
    }
    int carry = -1;                                    // the last voiced frame before the chunk
    for (int ch = 0; ch < chunks; ++ch) {
        const int i = ch * PT_SCAN_CHUNK + tid;
        sm[tid] = (i < n && f[i] != 0.f) ? i : -1;
        __syncthreads();
        for (int off = 1; off < PT_SCAN_CHUNK; off <<= 1) {
            const int v = tid >= off ? sm[tid - off] : -1;
            __syncthreads();
            if (v > sm[tid]) sm[tid] = v;
            __syncthreads();
        }
        if (i < n) pv[i] = sm[tid] > carry ? sm[tid] : carry;
        const int last = sm[PT_SCAN_CHUNK - 1];
        carry = last > carry ? last : carry;
        __syncthreads();
    }
    if (carry < 0) {                                   // no voiced frame (uniform): the track as it is
        for (int i = tid; i < n; i += PT_SCAN_CHUNK) o[i] = f[i];
        return;
    }
    carry = PT_NONE;                                   // the first voiced frame after the chunk
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int i = ch * PT_SCAN_CHUNK + tid;
        sm[tid] = (i < n && f[i] != 0.f) ? i : PT_NONE;
        __syncthreads();
        for (int off = 1; off < PT_SCAN_CHUNK; off <<= 1) {
            const int v = tid + off < PT_SCAN_CHUNK ? sm[tid + off] : PT_NONE;
            __syncthreads();
            if (v < sm[tid]) sm[tid] = v;
            __syncthreads();
        }
        if (i < n) {                                   // (prev[i] was written by this very thread)
            const int a = pv[i], b = sm[tid] < carry ? sm[tid] : carry;
            float v;
            if (a < 0) v = f[b];
            else if (b == PT_NONE) v = f[a];
            else if (a == b) v = f[i];
            else {
                const double fa = f[a], fb = f[b];
                v = (float)(fa + (fb - fa) * (double)(i - a) / (double)(b - a));
            }
            if ((log_flag & 1) && v != 0.f) v = (float)log((double)v);
            o[i] = v;
        }
        const int first = sm[0];
        carry = first < carry ? first : carry;
        __syncthreads();
    }
}

// ---- the tracker ("Viterbi tracking over candidates").  Everything below reads the d' rows k_pitch wrote.
constexpr unsigned long long PTK_NOKEY = ~0ull;

// fp32 -> 32 bits that order as the values do (for d' >= 0 these are the value's own bits with the sign bit set; the map also
// orders negative values, which only rows handed to pk_pitch_track_from_cmnd can hold; -0 is +0)
__device__ __forceinline__ unsigned ptk_order_bits(float v) {
    const unsigned b = __float_as_uint(v + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// k_pitch_cand: one wave per frame.  Lane l looks at the lags tau_min + l + 64 j: a local minimum under theta_c becomes the key
// (order bits of d' << 32 | tau), anything else PTK_NOKEY.  K rounds of a wave-wide minimum pick the K smallest keys (a key is
// unique: it holds its lag), lane r keeps the winner of round r; the winners' ranks by lag are their slots.
__global__ __launch_bounds__(PT_THREADS) void k_pitch_cand(const float* __restrict__ cmnd, long total, int row, int tau_min,
                                                           int tau_max, int K, float theta_c, int* __restrict__ cand_lag,
                                                           float* __restrict__ cand_cost) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long fr = (long)blockIdx.x * (PT_THREADS / 64) + wave;
    if (fr >= total) return;                               // (uniform over the wave; the kernel has no barrier)
    const float* r = cmnd + fr * row;
    unsigned long long key[PTK_SLOTS];
#pragma unroll
    for (int j = 0; j < PTK_SLOTS; ++j) {
        const int tau = tau_min + lane + 64 * j;
        unsigned long long k = PTK_NOKEY;
        if (tau <= tau_max - 1) {
            const float a = r[tau - 1], b = r[tau], c = r[tau + 1];
            if (b < a && b <= c && b < theta_c) k = ((unsigned long long)ptk_order_bits(b) << 32) | (unsigned)tau;
        }
        key[j] = k;
    }
    unsigned long long mine = PTK_NOKEY;
    for (int round = 0; round < K; ++round) {              // (K is uniform)
        unsigned long long m = PTK_NOKEY;
#pragma unroll
        for (int j = 0; j < PTK_SLOTS; ++j) m = key[j] < m ? key[j] : m;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off, 64);
            m = o < m ? o : m;
        }
        if (lane == round) mine = m;
#pragma unroll
        for (int j = 0; j < PTK_SLOTS; ++j)
            if (key[j] == m) key[j] = PTK_NOKEY;           // (no effect once m is PTK_NOKEY)
    }
    const unsigned my_tau = (unsigned)(mine & 0xffffffffu);   // 0xffffffff without a candidate
    int rank = 0;
    for (int i = 0; i < K; ++i) {
        const unsigned o = __shfl(my_tau, i, 64);
        rank += o < my_tau ? 1 : 0;
    }
    if (lane < K) {
        const bool have = mine != PTK_NOKEY;               // c winners fill the slots 0 ... c - 1 by rank, the lanes c ... K - 1 the rest
        const int slot = have ? rank : lane;
        cand_lag[fr * K + slot] = have ? (int)my_tau : 0;
        cand_cost[fr * K + slot] = have ? r[my_tau] : __uint_as_float(0x7f800000u);
    }
}

// lane exchanges of the tracker's frame loop: DPP moves (no LDS traffic, a few cycles each).  0xB1 / 0x4E: quad_perm [1,0,3,2] /
// [2,3,0,1] (lane ^ 1, lane ^ 2); 0x141: row_half_mirror (lane -> 7 - lane within 8 lanes: the other quad)
template <int CTRL>
__device__ __forceinline__ double ptk_dpp(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// the minimum of x over the 8 lanes that share lane >> 3, in all 8 of them (the inputs are never NaN)
__device__ __forceinline__ double ptk_min8(double x) {
    double o = ptk_dpp<0xB1>(x);
    x = o < x ? o : x;
    o = ptk_dpp<0x4E>(x);
    x = o < x ? o : x;
    o = ptk_dpp<0x141>(x);
    return o < x ? o : x;
}

// k_pitch_viterbi: one wave per utterance.  Lane l owns the pair (predecessor p = l & 7, state s = l >> 3) of voiced slots; the
// unvoiced state (index 8 here, whatever K is: it is the last state either way) is carried by every lane.  The candidates of
// PTK_CH frames are staged in LDS as (log2 of the lag, cost) in float64, the next chunk's global loads are issued before the
// chunk's frames are walked and land in LDS after them, and a frame's three LDS reads are issued one frame ahead: the loop
// waits for no global load.  A frame's backpointers are one 64-bit word (4 bits x 9 states) in LDS, or in `bp_ws` when the
// utterance has more than `bp_lds` frames.  The minimum over p is three DPP steps on the value; which p attained it is read
// off a ballot afterwards, beside the chain that the next frame waits for.  The backtrack takes 64 frames at a time: lane j
// loads the word of frame base + j, the walk reads the words lane by lane into scalar registers (lane j keeps the state of its
// frame), then the 64 lanes refine their frames.
__global__ __launch_bounds__(64) void k_pitch_viterbi(const float* __restrict__ cmnd, const pt_utt* __restrict__ utts,
                                                      const int* __restrict__ cand_lag, const float* __restrict__ cand_cost,
                                                      const double* __restrict__ logtau, unsigned long long* __restrict__ bp_ws,
                                                      float* __restrict__ f0_out, int* __restrict__ lag_out,
                                                      double* __restrict__ score_out, int row, int K, int bp_lds, double lambda,
                                                      double cu, double sw, double sr) {
#pragma clang fp contract(off)
    __shared__ double T[PT_MAX_TAU + 1];
    __shared__ double lt[PTK_CH][8];
    __shared__ double ob[PTK_CH][8];
    __shared__ uint64_t bp[PTK_BP_LDS];
    const pt_utt u = utts[blockIdx.x];
    const int nf = u.n_frames, lane = threadIdx.x, p = lane & 7, s = lane >> 3;
    const bool use_ws = nf > bp_lds;                       // (uniform)
    unsigned long long* bpw = bp_ws + u.foff;
    const double inf = (double)__uint_as_float(0x7f800000u);
    for (int t = lane; t < row; t += 64) T[t] = logtau[t];
    // staging: lane l holds slot l & 7 of the frames (l >> 3) + 8 q of a chunk
    int plag[PTK_CH / 8];
    float pcost[PTK_CH / 8];
    auto fetch = [&](int c) {
#pragma unroll
        for (int q = 0; q < PTK_CH / 8; ++q) {
            const int i = c * PTK_CH + s + 8 * q;
            const bool have = i < nf && p < K;
            const long at = (u.foff + (have ? i : 0)) * K + (have ? p : 0);
            const int l = cand_lag[at];
            const float v = cand_cost[at];
            plag[q] = have ? l : 0;
            pcost[q] = have ? v : __uint_as_float(0x7f800000u);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < PTK_CH / 8; ++q) {
            lt[s + 8 * q][p] = T[plag[q]];
            ob[s + 8 * q][p] = (double)pcost[q];
        }
    };
    fetch(0);
    __syncthreads();                                       // T is written
    stage();
    __syncthreads();
    const int chunks = (nf + PTK_CH - 1) / PTK_CH;
    double Dv = inf, Du = cu, ltp_prev = 0.0;
    for (int c = 0; c < chunks; ++c) {
        if (c + 1 < chunks) fetch(c + 1);                  // (uniform)
        const int n = nf - c * PTK_CH < PTK_CH ? nf - c * PTK_CH : PTK_CH;
        double n_lts = lt[0][s], n_ltp = lt[0][p], n_o = ob[0][s];
        for (int f = 0; f < n; ++f) {
            const int i = c * PTK_CH + f;
            const double lts = n_lts, ltp = n_ltp, o = n_o;
            if (f + 1 < n) {
                n_lts = lt[f + 1][s];
                n_ltp = lt[f + 1][p];
                n_o = ob[f + 1][s];
            }
            if (i == 0) {                                  // (uniform)
                Dv = o;
                Du = cu;
            } else {
                const double Dp = __shfl(Dv, p * 8, 64);   // D(i - 1)[p]: the lanes of group p hold it
                const double tr = lambda * fabs(lts - ltp_prev);
                const double v0 = Dp + tr, w0 = Dp + sw;   // into voiced state s / into the unvoiced state, from voiced p
                double v = ptk_min8(v0), w = ptk_min8(w0);
                // the predecessor: the smallest p that attains the minimum (a ballot: byte s holds the p's of state s); the
                // unvoiced predecessor is the last one, it wins only if smaller
                const unsigned long long mv = __ballot(v0 == v), mw = __ballot(w0 == w);
                const unsigned bv = (unsigned)(mv >> (8 * s)) & 0xffu, bw = (unsigned)mw & 0xffu;
                int a = bv ? __builtin_ctz(bv) : 8, aw = bw ? __builtin_ctz(bw) : 8;
                const double vu = Du + sw;
                a = vu < v ? 8 : a;
                v = vu < v ? vu : v;
                aw = Du < w ? 8 : aw;
                w = Du < w ? Du : w;
                Dv = v + o;
                Du = w + cu;
                // the frame's word: every lane of group s holds a << 4 s; OR over the groups by row_ror:8, row_bcast:15 into
                // rows 1 and 3, row_bcast:31 into rows 2 and 3: lane 63 has all eight nibbles
                int nib = a << (4 * s);
                nib |= __builtin_amdgcn_update_dpp(0, nib, 0x128, 0xf, 0xf, false);
                nib |= __builtin_amdgcn_update_dpp(0, nib, 0x142, 0xa, 0xf, false);
                nib |= __builtin_amdgcn_update_dpp(0, nib, 0x143, 0xc, 0xf, false);
                const unsigned long long word = (unsigned long long)(unsigned)nib | ((unsigned long long)aw << 32);
                if (lane == 63) {
                    if (use_ws) bpw[i] = word;
                    else bp[i] = word;
                }
            }
            ltp_prev = ltp;
        }
        __syncthreads();                                   // the chunk is read, the backpointers are written
        if (c + 1 < chunks) {
            stage();
            __syncthreads();
        }
    }
    // the last state: the smallest s of minimal D
    double best = __shfl(Dv, 0, 64);
    int st = 0;
    for (int q = 1; q < 8; ++q) {
        const double d = __shfl(Dv, q * 8, 64);
        if (d < best) {
            best = d;
            st = q;
        }
    }
    if (Du < best) {
        best = Du;
        st = 8;
    }
    if (lane == 0 && score_out) score_out[blockIdx.x] = best;
    st = __builtin_amdgcn_readfirstlane(st);               // (the same in every lane)
    for (int base = (nf - 1) / 64 * 64; base >= 0; base -= 64) {
        const int hi = (nf < base + 64 ? nf : base + 64) - 1;
        unsigned long long mw = 0ull;                      // lane j: the word of frame base + j
        if (base + lane < nf && base + lane > 0) mw = use_ws ? bpw[base + lane] : bp[base + lane];   // (frame 0 has none)
        const int wlo = (int)(unsigned)mw, whi = (int)(unsigned)(mw >> 32);
        int mine = 8;
#pragma unroll
        for (int j = 63; j >= 0; --j) {
            if (base + j <= hi) {                          // (uniform)
                mine = lane == j ? st : mine;
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane(wlo, j), up = (unsigned)__builtin_amdgcn_readlane(whi, j);
                if (base + j > 0) st = (int)(((((unsigned long long)up << 32) | lo) >> (4 * st)) & 15ull);
            }
        }
        const int i = base + lane;
        if (i < nf) {
            const long fr = u.foff + i;
            float f0 = 0.f;
            int lag = mine < K ? cand_lag[fr * K + mine] : 0;
            if (lag >= 1 && lag <= row - 2) {
                const float* dr = cmnd + fr * row;
                const double a = dr[lag - 1], b = dr[lag], c = dr[lag + 1];
                const double den = a - 2.0 * b + c;
                const double delta = (a >= b && c >= b && den > 0.0) ? (a - c) / (2.0 * den) : 0.0;
                f0 = (float)(sr / ((double)lag + delta));
            } else {
                lag = 0;
            }
            if (f0_out) f0_out[fr] = f0;
            if (lag_out) lag_out[fr] = lag;
        }
    }
}

}  // namespace

struct pk_pitch {
    pk_ctx* ctx = nullptr;
    pk_pitch_cfg cfg;
    pt_plan plan;
    pk_dbuf ws_utt, ws_in, ws_f0, ws_lag, ws_cmnd;
    // the tracker: the table of log2(tau), candidates, backpointer words of long tracks, scores and the staging of a host call
    pk_dbuf ws_logtau, ws_clag, ws_ccost, ws_bp, ws_score, ws_tcm;
    bool logtau_ready = false;
    int bp_lds = PTK_BP_LDS;
};

extern "C" int pk_pitch_create(pk_ctx* ctx, const pk_pitch_cfg* cfg, pk_pitch** out) {
    if (!ctx || !cfg || !out) PK_FAIL(PK_EINVAL, "pk_pitch_create: NULL argument");
    *out = nullptr;
    const pk_pitch_cfg& c = *cfg;
    if (c.sr < 1) PK_FAIL(PK_EINVAL, "pitch: sr = %d must be positive", (int)c.sr);
    if (!(c.threshold == c.threshold)) PK_FAIL(PK_EINVAL, "pitch: the threshold is not a number");
    if (c.tau_max > PT_MAX_TAU || c.tau_max < 4)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: tau_max = %d; the engine's envelope is 4 ... %d lags", (int)c.tau_max, PT_MAX_TAU);
    if (c.tau_min < 2 || c.tau_min > c.tau_max - 2)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: tau_min = %d; it must be in 2 ... tau_max - 2 = %d", (int)c.tau_min, (int)c.tau_max - 2);
    if (c.win < 1 || c.win > 2 * c.tau_max)
        PK_FAIL(PK_EUNSUPPORTED, "pitch: a window of %d samples; the limit is 1 ... 2 * tau_max = %d", (int)c.win,
                2 * (int)c.tau_max);
    if (c.hop < 1 || c.hop > PT_MAX_HOP) PK_FAIL(PK_EUNSUPPORTED, "pitch: hop = %d; the limit is 1 ... %d", (int)c.hop, PT_MAX_HOP);
    pk_pitch* h = new pk_pitch();
    h->ctx = ctx;
    h->cfg = c;
    h->plan = pt_make_plan(c.hop, c.tau_max, c.win);
    *out = h;
    return PK_OK;
}

extern "C" int pk_pitch_frames(pk_pitch* h, int64_t n_samples, int32_t* frames) {
    if (!h || !frames) PK_FAIL(PK_EINVAL, "pk_pitch_frames: NULL argument");
    if (n_samples < 0 || n_samples > 0x7fffffffL) PK_FAIL(PK_EINVAL, "pk_pitch_frames: n_samples must be in 0 ... 2^31 - 1");
    *frames = (int32_t)(n_samples / h->cfg.hop + 1);
    return PK_OK;
}

extern "C" int pk_pitch_tile_frames(pk_pitch* h, int32_t* tile) {
    if (!h || !tile) PK_FAIL(PK_EINVAL, "pk_pitch_tile_frames: NULL argument");
    *tile = h->plan.F;
    return PK_OK;
}

extern "C" int pk_pitch_run(pk_pitch* h, const float* wav, const int32_t* lens, int32_t B, float* f0_out, int32_t* lag_out,
                            float* cmnd_out, int32_t flags) {
    if (!h || !wav || !lens || !f0_out) PK_FAIL(PK_EINVAL, "pk_pitch_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pitch_run: batch size must be positive");
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    const pt_plan& p = h->plan;
    const pk_pitch_cfg& c = h->cfg;
    std::vector<pt_utt> tab(B);
    long sum_in = 0, sum_fr = 0, max_tiles = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "pk_pitch_run: utterance %d is empty (%d samples)", b, (int)lens[b]);
        const int nf = lens[b] / c.hop + 1;
        tab[b] = {sum_in, sum_fr, lens[b], nf};
        sum_in += lens[b];
        sum_fr += nf;
        const long tiles = (nf + p.F - 1) / p.F;
        max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
    PK_TRY(h->ws_utt.reserve(tab.size() * sizeof(pt_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utt.p, tab.data(), tab.size() * sizeof(pt_utt), hipMemcpyHostToDevice, ctx->stream));
    const float* d_in = wav;
    float* d_f0 = f0_out;
    int* d_lag = lag_out;
    float* d_cm = cmnd_out;
    const size_t cm_bytes = (size_t)sum_fr * p.row * 4;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)sum_in * 4));
        PK_TRY(h->ws_f0.reserve((size_t)sum_fr * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, wav, (size_t)sum_in * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = h->ws_in.as<float>();
        d_f0 = h->ws_f0.as<float>();
        if (lag_out) {
            PK_TRY(h->ws_lag.reserve((size_t)sum_fr * 4));
            d_lag = h->ws_lag.as<int>();
        }
        if (cmnd_out) {
            PK_TRY(h->ws_cmnd.reserve(cm_bytes));
            d_cm = h->ws_cmnd.as<float>();
        }
    }
    PK_HIP(hipStreamSynchronize(ctx->stream));             // `tab` leaves scope with this call
    const size_t lds = ((size_t)p.span + (size_t)p.F * p.row) * sizeof(float);
    constexpr int GRID_Y = 32768;                          // utterances per launch (grid.y is a 16-bit quantity)
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        const int nb = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        PK_LAUNCH(ctx, "pitch", k_pitch, dim3((unsigned)max_tiles, (unsigned)nb), dim3(PT_THREADS), lds, d_in,
                  h->ws_utt.as<pt_utt>() + b0, d_f0, d_lag, d_cm, (int)c.hop, (int)c.tau_min, (int)c.tau_max, (int)c.win, p.G, p.F,
                  p.span, c.threshold, (double)c.sr);
    }
    if (flags & PK_HOST_IO) {
        PK_HIP(hipMemcpyAsync(f0_out, d_f0, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (lag_out) PK_HIP(hipMemcpyAsync(lag_out, d_lag, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (cmnd_out) PK_HIP(hipMemcpyAsync(cmnd_out, d_cm, cm_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

extern "C" int pk_pitch_set_option(pk_pitch* h, const char* key, int64_t value) {
    if (!h || !key) PK_FAIL(PK_EINVAL, "pk_pitch_set_option: NULL argument");
    if (!strcmp(key, "track_lds_frames")) {
        if (value < 1 || value > PTK_BP_LDS)
            PK_FAIL(PK_EINVAL, "pk_pitch_set_option: track_lds_frames = %lld is not in 1 ... %d", (long long)value, PTK_BP_LDS);
        h->bp_lds = (int)value;
    } else PK_FAIL(PK_EINVAL, "pk_pitch_set_option: unknown option '%s'", key);
    return PK_OK;
}

namespace {

int ptk_check_cfg(const char* who, const pk_pitch_track_cfg* c) {
    if (c->K < 1 || c->K > PTK_MAX_K) PK_FAIL(PK_EINVAL, "%s: K = %d candidates; it must be in 1 ... %d", who, (int)c->K, PTK_MAX_K);
    if (!(c->theta_c == c->theta_c)) PK_FAIL(PK_EINVAL, "%s: the candidate threshold is not a number", who);
    const double costs[] = {c->lambda, c->unvoiced_cost, c->switch_cost};
    const char* names[] = {"lambda", "unvoiced_cost", "switch_cost"};
    for (int i = 0; i < 3; ++i)
        if (!(costs[i] >= 0.0) || costs[i] > 1.7976931348623157e308)
            PK_FAIL(PK_EINVAL, "%s: %s = %g must be a finite number >= 0", who, names[i], costs[i]);
    return PK_OK;
}

// stages 1-5 on the d' rows at d_cm (device); h->ws_utt holds the call's table (foff and n_frames are read)
int ptk_run(pk_pitch* h, const float* d_cm, long sum_fr, int B, const pk_pitch_track_cfg* cfg, float* f0_out, int32_t* lag_out,
            double* score_out, int32_t* cand_lag_out, float* cand_cost_out, int32_t flags) {
    pk_ctx* ctx = h->ctx;
    const pk_pitch_cfg& c = h->cfg;
    const int row = h->plan.row, K = cfg->K;
    const bool host = (flags & PK_HOST_IO) != 0;
    if (!h->logtau_ready) {                                // float64 log2(tau), T[0] = 0: the device calls no transcendental
        std::vector<double> T(row);
        T[0] = 0.0;
        for (int t = 1; t < row; ++t) T[t] = std::log2((double)t);
        PK_TRY(pk_upload(ctx, h->ws_logtau, T.data(), T.size() * sizeof(double)));
        PK_HIP(hipStreamSynchronize(ctx->stream));
        h->logtau_ready = true;
    }
    const size_t n_c = (size_t)sum_fr * K;
    int* d_cl = cand_lag_out;
    float* d_cc = cand_cost_out;
    if (host || !d_cl) {
        PK_TRY(h->ws_clag.reserve(n_c * 4));
        d_cl = h->ws_clag.as<int>();
    }
    if (host || !d_cc) {
        PK_TRY(h->ws_ccost.reserve(n_c * 4));
        d_cc = h->ws_ccost.as<float>();
    }
    float* d_f0 = f0_out;
    int* d_lag = lag_out;
    double* d_sc = score_out;
    if (host) {
        if (f0_out) {
            PK_TRY(h->ws_f0.reserve((size_t)sum_fr * 4));
            d_f0 = h->ws_f0.as<float>();
        }
        if (lag_out) {
            PK_TRY(h->ws_lag.reserve((size_t)sum_fr * 4));
            d_lag = h->ws_lag.as<int>();
        }
        if (score_out) {
            PK_TRY(h->ws_score.reserve((size_t)B * 8));
            d_sc = h->ws_score.as<double>();
        }
    }
    PK_TRY(h->ws_bp.reserve((size_t)sum_fr * 8));          // (read and written by utterances of more than bp_lds frames only)
    const long waves = PT_THREADS / 64;
    PK_LAUNCH(ctx, "pitch_cand", k_pitch_cand, dim3((unsigned)((sum_fr + waves - 1) / waves)), dim3(PT_THREADS), 0, d_cm, sum_fr, row,
              (int)c.tau_min, (int)c.tau_max, K, cfg->theta_c, d_cl, d_cc);
    constexpr int GRID_X = 1 << 20;
    for (int b0 = 0; b0 < B; b0 += GRID_X) {
        const int nb = B - b0 < GRID_X ? B - b0 : GRID_X;
        PK_LAUNCH(ctx, "pitch_viterbi", k_pitch_viterbi, dim3((unsigned)nb), dim3(64), 0, d_cm, h->ws_utt.as<pt_utt>() + b0, d_cl, d_cc,
                  h->ws_logtau.as<double>(), h->ws_bp.as<unsigned long long>(), d_f0, d_lag, d_sc ? d_sc + b0 : nullptr, row, K,
                  h->bp_lds, cfg->lambda, cfg->unvoiced_cost, cfg->switch_cost, (double)c.sr);
    }
    if (host) {
        if (f0_out) PK_HIP(hipMemcpyAsync(f0_out, d_f0, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (lag_out) PK_HIP(hipMemcpyAsync(lag_out, d_lag, (size_t)sum_fr * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (score_out) PK_HIP(hipMemcpyAsync(score_out, d_sc, (size_t)B * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (cand_lag_out) PK_HIP(hipMemcpyAsync(cand_lag_out, d_cl, n_c * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (cand_cost_out) PK_HIP(hipMemcpyAsync(cand_cost_out, d_cc, n_c * 4, hipMemcpyDeviceToHost, ctx->stream));
        PK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PK_OK;
}

}  // namespace

extern "C" int pk_pitch_track_run(pk_pitch* h, const float* wav, const int32_t* lens, int32_t B, const pk_pitch_track_cfg* cfg,
                                  float* f0_out, int32_t* lag_out, double* score_out, int32_t* cand_lag_out, float* cand_cost_out,
                                  int32_t flags) {
    if (!h || !wav || !lens || !cfg) PK_FAIL(PK_EINVAL, "pk_pitch_track_run: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pitch_track_run: batch size must be positive");
    PK_TRY(ptk_check_cfg("pk_pitch_track_run", cfg));
    long sum_in = 0, sum_fr = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) PK_FAIL(PK_EINVAL, "pk_pitch_track_run: utterance %d is empty (%d samples)", b, (int)lens[b]);
        const long nf = lens[b] / h->cfg.hop + 1;
        if (nf > PTK_MAX_FRAMES)
            PK_FAIL(PK_EUNSUPPORTED, "pk_pitch_track_run: utterance %d has %ld frames; the tracker's envelope is %d", b, nf, PTK_MAX_FRAMES);
        sum_in += lens[b];
        sum_fr += nf;
    }
    PK_DEVICE(h->ctx->device);
    const float* d_in = wav;
    if (flags & PK_HOST_IO) {
        PK_TRY(h->ws_in.reserve((size_t)sum_in * 4));
        PK_HIP(hipMemcpyAsync(h->ws_in.p, wav, (size_t)sum_in * 4, hipMemcpyHostToDevice, h->ctx->stream));
        d_in = h->ws_in.as<float>();
    }
    // the estimator's own call on device pointers: d' into the handle's workspace (its per-frame f0 is not wanted: it goes to the
    // same workspace the tracker's own f0 of a host call overwrites afterwards, in stream order); it leaves the call's table in ws_utt
    PK_TRY(h->ws_tcm.reserve((size_t)sum_fr * h->plan.row * 4));
    PK_TRY(h->ws_f0.reserve((size_t)sum_fr * 4));
    PK_TRY(pk_pitch_run(h, d_in, lens, B, h->ws_f0.as<float>(), nullptr, h->ws_tcm.as<float>(), 0));
    return ptk_run(h, h->ws_tcm.as<float>(), sum_fr, B, cfg, f0_out, lag_out, score_out, cand_lag_out, cand_cost_out, flags);
}

extern "C" int pk_pitch_track_from_cmnd(pk_pitch* h, const float* cmnd, const int32_t* frames, int32_t B, const pk_pitch_track_cfg* cfg,
                                        float* f0_out, int32_t* lag_out, double* score_out, int32_t* cand_lag_out,
                                        float* cand_cost_out, int32_t flags) {
    if (!h || !cmnd || !frames || !cfg) PK_FAIL(PK_EINVAL, "pk_pitch_track_from_cmnd: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_pitch_track_from_cmnd: batch size must be positive");
    PK_TRY(ptk_check_cfg("pk_pitch_track_from_cmnd", cfg));
    std::vector<pt_utt> tab(B);
    long sum_fr = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) PK_FAIL(PK_EINVAL, "pk_pitch_track_from_cmnd: track %d is empty (%d frames)", b, (int)frames[b]);
        if (frames[b] > PTK_MAX_FRAMES)
            PK_FAIL(PK_EUNSUPPORTED, "pk_pitch_track_from_cmnd: track %d has %d frames; the tracker's envelope is %d", b, (int)frames[b],
                    PTK_MAX_FRAMES);
        tab[b] = {0, sum_fr, 0, frames[b]};
        sum_fr += frames[b];
    }
    pk_ctx* ctx = h->ctx;
    PK_DEVICE(ctx->device);
    PK_TRY(h->ws_utt.reserve(tab.size() * sizeof(pt_utt)));
    PK_HIP(hipMemcpyAsync(h->ws_utt.p, tab.data(), tab.size() * sizeof(pt_utt), hipMemcpyHostToDevice, ctx->stream));
    const float* d_cm = cmnd;
    if (flags & PK_HOST_IO) {
        const size_t bytes = (size_t)sum_fr * h->plan.row * 4;
        PK_TRY(h->ws_tcm.reserve(bytes));
        PK_HIP(hipMemcpyAsync(h->ws_tcm.p, cmnd, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_cm = h->ws_tcm.as<float>();
    }
    PK_HIP(hipStreamSynchronize(ctx->stream));             // `tab` leaves scope with this call
    return ptk_run(h, d_cm, sum_fr, B, cfg, f0_out, lag_out, score_out, cand_lag_out, cand_cost_out, flags);
}

extern "C" void pk_pitch_destroy(pk_pitch* h) {
    if (!h) return;
    pk_device_guard _dg(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    pk_dbuf* bufs[] = {&h->ws_utt,    &h->ws_in,   &h->ws_f0,    &h->ws_lag, &h->ws_cmnd, &h->ws_logtau,
                       &h->ws_clag,   &h->ws_ccost, &h->ws_bp,   &h->ws_score, &h->ws_tcm};
    for (auto* b : bufs) b->release();
    delete h;
}

extern "C" int pk_op_continuous_f0(pk_ctx* ctx, const float* f0, const int32_t* frames, int32_t B, int32_t log_flag,
                                   float* out) {
    if (!ctx || !f0 || !frames || !out) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: NULL argument");
    if (B <= 0) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: batch size must be positive");
    if (log_flag < 0 || log_flag > 3) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: log_flag = %d is not in 0 ... 3", (int)log_flag);
    PK_DEVICE(ctx->device);
    std::vector<pt_utt> tab(B);
    long sum = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) PK_FAIL(PK_EINVAL, "pk_op_continuous_f0: track %d is empty (%d frames)", b, (int)frames[b]);
        tab[b] = {0, sum, 0, frames[b]};
        sum += frames[b];
    }
    pk_dbuf d_tab, d_prev;
    int rc = pk_upload(ctx, d_tab, tab.data(), tab.size() * sizeof(pt_utt));
    if (rc == PK_OK) rc = d_prev.reserve((size_t)sum * sizeof(int));
    constexpr int GRID_X = 1 << 20;
    for (int b0 = 0; rc == PK_OK && b0 < B; b0 += GRID_X) {
        const int nb = B - b0 < GRID_X ? B - b0 : GRID_X;
        hipLaunchKernelGGL(k_cont_f0, dim3(nb), dim3(PT_SCAN_CHUNK), 0, ctx->stream, f0, d_tab.as<pt_utt>() + b0,
                           d_prev.as<int>(), out, (int)log_flag);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            pk_set_error("pk_op_continuous_f0: %s", hipGetErrorString(e));
            rc = PK_EHIP;
        }
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // the two buffers are released below
    if (e != hipSuccess && rc == PK_OK) {
        pk_set_error("pk_op_continuous_f0: %s", hipGetErrorString(e));
        rc = PK_EHIP;
    }
    d_tab.release();
    d_prev.release();
    return rc;
}
