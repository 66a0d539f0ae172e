"""Cases of the multi-resolution STFT loss tests (a plain module, not a conftest; shared by tests/test_stft_loss_cpu.py,
tests/test_stft_loss_gpu.py and tools/make_golden_stft_loss.py).

Resolutions (n_fft, hop, win_length): the smallest that take every path of csrc/stft_dist.hip -- the four residues of the hop
modulo 4 (1, 2 or 4 shifted copies of the timeline, 1, 2 or 4 GEMMs), a window shorter than the transform at an odd offset,
and the three resolutions of every Parallel WaveGAN recipe.  Every case is a ragged batch of three pairs: the shortest
utterance reflect padding allows (n_fft / 2 + 1 samples), one of about 4 900 samples and one in between; the predicted
signal of the middle pair is all zeros, so the floor is engaged on every entry of it.

Signals.  Band noise plus a tone, a component at the Nyquist frequency and one click.  The click and the Nyquist component
are there for the mutant tests: a stationary signal has the same magnitudes when every frame starts one sample late, and a
signal without energy at the Nyquist frequency loses nothing with that bin; the worst-case bound (which grows with n_fft) must
still tell such a result from the right one.
"""
import collections
import zlib

import numpy as np

Res = collections.namedtuple("Res", "n_fft hop win")

RESOLUTIONS = [
    Res(64, 16, 64),        # aligned baseline
    Res(32, 6, 20),         # hop = 2 mod 4: two copies
    Res(64, 5, 64),         # hop = 1 mod 4: four copies
    Res(64, 7, 30),         # hop = 3 mod 4, window offset 17 (odd)
    Res(512, 50, 240), Res(1024, 120, 600), Res(2048, 240, 1200),   # the recipe's three
]
RECIPE = [Res(1024, 120, 600), Res(2048, 240, 1200), Res(512, 50, 240)]   # in the reference's default order
GEMM_BM = 128     # PK_GEMM_BM


def res_id(r):
    return f"{r.n_fft}-{r.hop}-{r.win}"


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def num_frames(r, n):
    return 1 + n // r.hop          # centred: 1 + (n + n_fft - n_fft) // hop


def signal(n, key, click=8.0):
    g = rng_for("stft_loss", key)
    t = np.arange(n, dtype=np.float64)
    x = 0.1 * g.standard_normal(n) + 0.05 * np.sin(2 * np.pi * 0.0371 * t + g.uniform(0, 6)) + 0.1 * (-1.0) ** t
    x[int(n * 0.6)] += click
    return x.astype(np.float32)


def lengths(r):
    """Three lengths whose frame counts, summed, are a multiple of neither 4 nor the GEMM's row tile -- for the batch and
    for the batch of 2B signals the distance runs."""
    lens = [r.n_fft // 2 + 1, 2600, 4897]
    while True:
        F = sum(num_frames(r, n) for n in lens)
        if F % 4 != 0 and (2 * F) % 4 != 0 and F % GEMM_BM != 0 and (2 * F) % GEMM_BM != 0:
            return lens
        lens[1] += 1


def batch(r):
    """-> xs, ys: lists of three float32 signals; xs[1] is silence."""
    lens = lengths(r)
    ys = [signal(n, ("y", res_id(r), i)) for i, n in enumerate(lens)]
    xs = [(y + 0.3 * signal(n, ("d", res_id(r), i), click=2.0)).astype(np.float32)
          for i, (y, n) in enumerate(zip(ys, lens))]
    xs[1] = np.zeros(lens[1], np.float32)
    return xs, ys


def golden_batch(T=1400):
    """The (B, T) pair the reference's own MultiResolutionSTFTLoss scores for tests/golden/stft_loss.npz."""
    y = np.stack([signal(T, ("golden-y", i)) for i in range(2)])
    x = (y + 0.3 * np.stack([signal(T, ("golden-d", i), click=2.0) for i in range(2)])).astype(np.float32)
    return x, y


def loud_batch(r):
    """For the scaling test: broadband signals around 2^20, so that at 2^-20 times their size no entry is near the floor."""
    lens = lengths(r)
    ys = [(2.0 ** 20 * 4.0 * signal(n, ("ly", res_id(r), i))).astype(np.float32) for i, n in enumerate(lens)]
    xs = [(2.0 ** 20 * 4.0 * signal(n, ("lx", res_id(r), i))).astype(np.float32) for i, n in enumerate(lens)]
    return xs, ys
