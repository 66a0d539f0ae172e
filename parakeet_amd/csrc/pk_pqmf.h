// pk_pqmf.h -- the pseudo-QMF bank (pqmf.hip): its filters and its arithmetic.  tests/pqmf_ref.py restates both.
//
// Filters, computed once on the host in float64 and rounded ONCE to float32.  K = subbands, n = 0 ... taps, c = n - taps / 2:
//   proto[n]       = sin(pi cutoff c) / (pi c) * kaiser(taps + 1, beta)[n],   the centre tap (c = 0) is cutoff * kaiser = cutoff
//   kaiser(M, b)[n] = I0(b sqrt(1 - ((n - (M - 1) / 2) / ((M - 1) / 2))^2)) / I0(b),   I0(x) = sum_j ((x / 2)^j / j!)^2
//   analysis_k[n]  = 2 proto[n] cos((2 k + 1) pi / (2 K) c + (-1)^k pi / 4)
//   synthesis_k[n] = 2 proto[n] cos((2 k + 1) pi / (2 K) c - (-1)^k pi / 4)
//
// Operations over packed ragged batches, h = taps / 2:
//   analysis   wav (L) -> bands (K, M), M = floor(L / K) (L >= K):
//                bands[k, m] = sum_(n = 0 ... taps) analysis_k[n] * x[m K + n - h],  x = 0 outside [0, L)
//              acc = 0, then acc = fmaf(analysis_k[n], x, acc) for n ASCENDING over all taps + 1 taps (those outside the
//              utterance multiply a staged 0).
//   synthesis  bands (K, M) -> wav (K M): zeros inserted, scaled by K, zero-padded by h, correlated with synthesis_k and
//              summed over k -- in its polyphase form
//                wav[t] = K * sum_k sum_m synthesis_k[m K - t + h] * bands[k, m],  over the m with 0 <= m K - t + h <= taps
//              acc = 0, then acc = fmaf(synthesis_k[n], bands[k, m], acc) for k ASCENDING and, within a band, m ASCENDING
//              from ceil((t - h) / K) to floor((t + h) / K) (at most ceil((taps + 1) / K) of them; an m outside [0, M)
//              multiplies a staged 0); wav[t] = (float)K * acc, one more rounding (none for a power of two).
// THE PRODUCTS ARE CONTRACTED: every step is one fmaf, one rounding.  The order is fixed and depends on nothing but the
// utterance-relative position, so a sample is the same bits alone, in any batch and at any position in it.  No atomics.
//
// Kernels: one workgroup of PQMF_THREADS takes PQMF_TILE outputs (band positions m for analysis, samples t for synthesis) of
// one utterance; the filters (K (taps + 1) floats) and the tile's input window are staged in LDS.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

struct pk_ctx;
struct pk_pqmf;

constexpr int PQMF_THREADS = 256;
constexpr int PQMF_TILE = 256;
constexpr int PQMF_MAX_K = 16;
constexpr int PQMF_MAX_TAPS = 254;
// LDS of a workgroup, in floats: the filters, then the window
constexpr int PQMF_LDS_FILT = PQMF_MAX_K * (PQMF_MAX_TAPS + 1);                          // 4080
constexpr int PQMF_LDS_WIN_A = (PQMF_TILE - 1) * PQMF_MAX_K + PQMF_MAX_TAPS + 1;         // analysis: 4335 wav samples at most
constexpr int PQMF_LDS_WIN_S = ((PQMF_TILE + PQMF_MAX_TAPS) / 2 + 2) * PQMF_MAX_K;       // synthesis: (band positions) x K, K >= 2

inline double pqmf_i0(double x) {
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < 2000; ++j) {
        term *= q / ((double)j * (double)j);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// analysis and synthesis (K, taps + 1) float32 each
inline void pqmf_design(int K, int taps, double cutoff, double beta, std::vector<float>& ana, std::vector<float>& syn) {
    const double pi = 3.14159265358979323846;
    const int N = taps + 1;
    const double alpha = taps / 2.0, i0b = pqmf_i0(beta);
    std::vector<double> proto(N);
    for (int n = 0; n < N; ++n) {
        const double c = n - alpha, r = c / alpha;
        const double win = pqmf_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
        proto[n] = (c == 0.0 ? cutoff : std::sin(pi * cutoff * c) / (pi * c)) * win;
    }
    ana.assign((size_t)K * N, 0.f);
    syn.assign((size_t)K * N, 0.f);
    for (int k = 0; k < K; ++k) {
        const double sgn = (k % 2 == 0) ? 1.0 : -1.0;
        for (int n = 0; n < N; ++n) {
            const double ph = (2 * k + 1) * pi / (2.0 * K) * (n - alpha);
            ana[(size_t)k * N + n] = (float)(2.0 * proto[n] * std::cos(ph + sgn * pi / 4.0));
            syn[(size_t)k * N + n] = (float)(2.0 * proto[n] * std::cos(ph - sgn * pi / 4.0));
        }
    }
}

// pqmf.hip, for melgan.hip: the synthesis kernel over tables that are already on the device, on ctx's stream.  lens / offs /
// tile0 / tile_b describe the OUTPUT rate (lens[b] = K M_b samples, offs[b] samples before utterance b; bands of utterance b
// start at K-channel-major offset offs[b]); tiles of PQMF_TILE samples.
int pk_pqmf_launch_synthesis(pk_pqmf* q, pk_ctx* ctx, const float* bands, const int* lens, const long* offs, const int* tile0,
                             const int* tile_b, int ntiles, float* wav);
int pk_pqmf_subbands(const pk_pqmf* q);
