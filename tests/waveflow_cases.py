"""Cases, inputs and float64 references of the WaveFlow sweep (tests/test_waveflow_sweep_cpu.py, tests/test_waveflow_sweep_gpu.py):
every family of configuration ``pk_wf_create`` admits, at the widths where the kernels change behaviour.  A plain module, not a
conftest.

What decides the code path (read from csrc/waveflow.hip and csrc/wf_layer.hip):

    channels 64 / 128 and 64 < n_mels < 96   the fused layer kernel (wf_layer / wf_row): 32-position blocks, the condition as fp16
                                             planes in blocks [pos / 32][96][32]; maths "f16x3" and "f16"
    anything else, or math "f32"             the GEMM path (wf_gemm_conv_gate...): 128-row tiles, the condition as [pos][mp] with
                                             mp = n_mels rounded up to 32 and the pad channels zero
    upsample_factors                         1 .. 4 launches of k_wf_upsample, 256 // n_mels time steps per block, intermediate
                                             layers in two ping-pong buffers, the last layer folds into the condition rows
    n_group                                  rows per position; 32 / 64 / 128 have height-dilated layers (rings deeper than 3 rows)

An utterance of T frames has cond_len(T) latent samples, ``pruned = cond_len // n_group * n_group`` waveform samples and
``width = pruned // n_group`` positions.  With ``[16, 16]`` and n_group 16 -- the one point the older tests run -- cond_len is a
multiple of 16 and width is 16 T - 17.  ``[4, 4]`` gives cond_len 16 T - 20, width T - 2 and 12 trimmed samples per utterance, so
the ragged offsets of z (counted in cond_len) and of the waveform (counted in pruned) differ from the second utterance on.

Inputs: ``syn.waveflow_state(cfg, seed, weight_norm=True)``, mels and z as tests/test_waveflow_gpu.py::_run.  Forward: audio 0.3 N(0, 1)
of ``pruned + r`` samples, r < n_group chosen per utterance so that ``frames x hop - len`` is not a multiple of n_group (the same
widths as infer; the samples past ``pruned`` are the ones _trim cuts).

Bars: the project's existing ones (INFER_BAR, tests/test_waveflow_forward_gpu.py's Z_BAR / LD_BAR / *_F16).  tests/test_waveflow_sweep_cpu.py
asserts that the float32 oracle alone stays inside them on every case.

``n_group=8`` with ``[16, 16]`` has width 32 T - 34, never 32 or 64: its batch has 30, 62 (across a block edge) and 94.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp32_bounds as fb                              # noqa: E402
import waveflow_forward_ref as fref                   # noqa: E402
from oracle import waveflow_ref as ref                # noqa: E402
from oracle.nn_ref import Weights, fold_weight_norm   # noqa: E402
from parakeet_amd import synthetic as syn             # noqa: E402

INFER_BAR = {"f32": 1e-5, "f16x3": 1e-5, "f16": 2e-3}           # of the waveform's peak (tests/test_waveflow_gpu.py)
Z_BAR, LD_BAR, Z_BAR_F16, LD_BAR_F16 = 1e-5, 1e-6, 2e-3, 2e-3   # tests/test_waveflow_forward_gpu.py (not its *_REG bars)
MAX_N_MELS = 256                                                # pk_wf_create: the upsampling kernel's block

Case = collections.namedtuple("Case", "name group over frames seed maths dirs waves fused widths")
# over:   overrides of syn.WAVEFLOW_LJSPEECH (n_flows 2 unless given: flow 0 and flow 1 are the two permutation kinds)
# frames: one ragged batch;  maths: set_math modes to run;  dirs: "infer" / "forward";  waves: layer_waves values that must give
# the same bits as the default;  fused: the kernel family expected for "f16x3" / "f16";  widths: widths the case claims to contain

_A, _B = (3, 34, 35, 131, 66), (33, 129, 130, 65, 4)
_BOTH = ("infer", "forward")


def _c(name, group, over, frames, seed, maths=("f16x3",), dirs=_BOTH, waves=(), fused=False, widths=()):
    return Case(name, group, dict({"n_flows": 2}, **over), tuple(frames), seed, tuple(maths), tuple(dirs), tuple(waves), fused,
                tuple(widths))


CASES = [
    # ---- fused kernel, width edges: [4, 4] gives width T - 2 and cond_len - pruned = 12 for every utterance
    _c("fw_c64_a", "fused_width", dict(channels=64, upsample_factors=[4, 4]), _A, 101, ("f16x3", "f16"), waves=(8, 12, 6), fused=True,
       widths=(1, 32, 33, 129, 64)),
    _c("fw_c64_b_4flows", "fused_width", dict(channels=64, upsample_factors=[4, 4], n_flows=4), _B, 102, ("f16x3", "f16"), waves=(8, 12, 6), fused=True,
       widths=(31, 127, 128, 63, 2)),
    _c("fw_c128_a", "fused_width", dict(channels=128, upsample_factors=[4, 4]), _A, 103, ("f16x3", "f16"), fused=True,
       widths=(1, 32, 33, 129, 64)),
    _c("fw_c128_b", "fused_width", dict(channels=128, upsample_factors=[4, 4]), _B, 104, ("f16x3", "f16"), fused=True,
       widths=(31, 127, 128, 63, 2)),
    # ---- n_group against the factors: a width below 32, one of exactly 32, one past it
    _c("ng8_f2", "n_group", dict(channels=64, n_group=8, upsample_factors=[2]), (6, 130, 133), 111, ("f16x3", "f16"), fused=True,
       widths=(1, 32, 33)),
    _c("ng8_f16x16", "n_group", dict(channels=64, n_group=8), (2, 3, 4), 112, fused=True, widths=(30, 62, 94)),
    _c("ng32_f4x4", "n_group", dict(channels=64, n_group=32, upsample_factors=[4, 4]), (5, 66, 68), 113, fused=True, widths=(1, 32, 33)),
    _c("ng64_f4x4", "n_group", dict(channels=64, n_group=64, upsample_factors=[4, 4]), (6, 130, 134), 115, fused=True,
       widths=(1, 32, 33)),
    _c("ng128_f64", "n_group", dict(channels=64, n_group=128, upsample_factors=[64]), (3, 65, 67), 114, fused=True, widths=(1, 32, 33)),
    # ---- unfused widths: 192 and 256 channels (always the GEMM path; "f16" refused)
    _c("c192_f4x4", "unfused_width", dict(channels=192, upsample_factors=[4, 4]), (4, 35, 131), 121, ("f32", "f16x3"), widths=(2, 33, 129)),
    _c("c256_f16x16", "unfused_width", dict(channels=256), (4, 3), 122, ("f32", "f16x3"), widths=(47, 31)),
    _c("c256_f4x4", "unfused_width", dict(channels=256, upsample_factors=[4, 4]), (34, 3, 131), 123, dirs=("infer",), widths=(32, 1, 129)),
    # ---- unfused n_mels: mp = 32 (16), 64 (48, 64), 128 (112, 128), 192 (176: one time step per upsampling block, 80 threads of it
    # idle), 256 (256: the largest the upsampling launch serves)
    _c("m16", "unfused_n_mels", dict(channels=64, n_mels=16, upsample_factors=[4, 4]), (3, 35, 10), 131, ("f32", "f16x3"), widths=(1, 33, 8)),
    _c("m48", "unfused_n_mels", dict(channels=64, n_mels=48, upsample_factors=[4, 4]), (3, 35, 10), 132, widths=(1, 33, 8)),
    _c("m64", "unfused_n_mels", dict(channels=64, n_mels=64, upsample_factors=[4, 4]), (3, 35, 10), 133, dirs=("infer",), widths=(1, 33, 8)),
    _c("m112", "unfused_n_mels", dict(channels=64, n_mels=112, upsample_factors=[4, 4]), (3, 35, 10), 134, ("f32", "f16x3"), widths=(1, 33, 8)),
    _c("m128", "unfused_n_mels", dict(channels=64, n_mels=128, upsample_factors=[4, 4]), (3, 35, 10), 135, dirs=("infer",), widths=(1, 33, 8)),
    _c("m176", "unfused_n_mels", dict(channels=64, n_mels=176, upsample_factors=[4, 4]), (3, 35, 10), 139, dirs=("infer",), widths=(1, 33, 8)),
    _c("m256", "unfused_n_mels", dict(channels=64, n_mels=256, upsample_factors=[4, 4]), (3, 35, 10), 136, widths=(1, 33, 8)),
    _c("c192_m48", "unfused_n_mels", dict(channels=192, n_mels=48), (4,), 137, widths=(47,)),
    _c("c128_m16_8flows_f8x4x2", "unfused_n_mels", dict(channels=128, n_mels=16, n_flows=8, upsample_factors=[8, 4, 2]), (5, 3), 138,
       dirs=("infer",), widths=(15, 7)),
    # ---- upsample stacks: one layer (which also folds), four layers (both ping-pong buffers twice), the factor extremes
    _c("up_2", "upsample", dict(channels=64, upsample_factors=[2]), (9, 257, 265), 141, fused=True, widths=(1, 32, 33)),
    _c("up_64_m256", "upsample", dict(channels=64, n_mels=256, upsample_factors=[64]), (2, 9, 10), 142, widths=(4, 32, 36)),
    _c("up_2x2x2x2", "upsample", dict(channels=64, upsample_factors=[2, 2, 2, 2]), (20, 3, 34, 35), 143, fused=True, widths=(18, 1, 32, 33)),
    _c("up_8x4x2_m112", "upsample", dict(channels=64, n_mels=112, upsample_factors=[8, 4, 2]), (2, 9, 10), 144, widths=(3, 31, 35)),
    _c("up_2x64_c128", "upsample", dict(channels=128, upsample_factors=[2, 64]), (2, 5, 6), 145, fused=True, widths=(4, 28, 36)),
    _c("up_64x2_m256", "upsample", dict(channels=64, n_mels=256, upsample_factors=[64, 2]), (2, 5, 6), 146, widths=(7, 31, 39)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the cases whose condition is read back on its own: every upsample stack and every n_mels, in both layouts
COND_CASES = [c.name for c in CASES if c.group in ("upsample", "unfused_n_mels")] + ["fw_c64_a", "ng8_f2", "ng128_f64"]


def cfg_of(case):
    return dict(syn.WAVEFLOW_LJSPEECH, **case.over)


def lengths(cfg, t_mel):
    """(cond_len, pruned) of an utterance of t_mel frames: what ``ConditionalWaveFlow.lengths`` answers."""
    n = ref.cond_length(t_mel, cfg["upsample_factors"])
    return n, n // cfg["n_group"] * cfg["n_group"]


def widths(case):
    cfg = cfg_of(case)
    return tuple(lengths(cfg, T)[1] // cfg["n_group"] for T in case.frames)


def hop(cfg):
    return int(np.prod(cfg["upsample_factors"]))


def audio_len(cfg, b, t_mel):
    """pruned + r: the first r from 1 + 2 b on (mod n_group) that fits under frames x hop with a shortfall that is no multiple of
    n_group."""
    G, full = cfg["n_group"], t_mel * hop(cfg)
    pruned = lengths(cfg, t_mel)[1]
    for k in range(G):
        n = pruned + (1 + 2 * b + k) % G
        if n <= full and (full - n) % G != 0:
            return n
    raise AssertionError((cfg, t_mel))


def mp_of(n_mels):
    return (n_mels + 31) // 32 * 32


def fused(case, math):
    return case.fused and math in ("f16x3", "f16")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state, mels, zs, audios) of a case; computed once, never modified."""
    case = BY_NAME[name]
    cfg = cfg_of(case)
    state = syn.waveflow_state(cfg, seed=case.seed, weight_norm=True)
    rng = np.random.default_rng(case.seed + 1)
    mels = [np.maximum(rng.normal(-4, 2, size=(cfg["n_mels"], T)), np.log(1e-5)).astype(np.float32) for T in case.frames]
    zs = [rng.normal(size=(lengths(cfg, T)[0],)).astype(np.float32) for T in case.frames]
    audios = [(0.3 * rng.normal(size=audio_len(cfg, b, T))).astype(np.float32) for b, T in enumerate(case.frames)]
    return state, mels, zs, audios


_DTYPE = {"f64": torch.float64, "f32": torch.float32}


def oracle_infer(state, mel, z, cfg, dtype="f64"):
    with torch.no_grad():
        return ref.infer(state, torch.from_numpy(mel)[None], torch.from_numpy(z)[None], cfg, _DTYPE[dtype])[0].numpy()


@functools.lru_cache(maxsize=None)
def infer_ref(name, dtype="f64"):
    """The oracle's waveform of every utterance of the case, each on its own (an utterance does not depend on its batch)."""
    case = BY_NAME[name]
    state, mels, zs, _ = inputs(name)
    return [oracle_infer(state, m, z, cfg_of(case), dtype) for m, z in zip(mels, zs)]


@functools.lru_cache(maxsize=None)
def forward_ref(name, dtype="f64"):
    """[(z, logdet)] per utterance."""
    case = BY_NAME[name]
    state, mels, _, audios = inputs(name)
    out = []
    for m, a in zip(mels, audios):
        z, ld = fref.forward(state, a[None], m[None], cfg_of(case), _DTYPE[dtype])
        out.append((z[0].numpy(), float(ld[0])))
    return out


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (np.abs(want).max() + 1e-30))


# ---------------------------------------------------------------- the upsampler on its own
def upsample_with_bound(state, mel, factors, trim):
    """(cond, bound), both (n_mels, T') float64: ``ref.upsample`` and an a-priori bound on an fp32 evaluation of it.

    A layer's output is bias + at most 6 products (3 mel taps x 2 input steps; kernel 2f, stride f) and then a leaky ReLU:
        bound_out = dot_bound((|in| + bound_in) (*) |w|, 6, bias)     the layer's own roundings, any order (fp32_bounds.dot_bound)
                  + bound_in (*) |w|                                  the input's error through the same transposed convolution
                  + 2 u |out|                                         the product with the slope 0.4f (its rounding, and 0.4f's)
    The leaky ReLU has slope <= 1, so it does not grow an error.  The weights are the fp32 rounding of the same fp64 fold on both
    sides (oracle/nn_ref.py fold_weight_norm, csrc/pk_ctx.cpp pk_get_weight): dot_bound's operand rounding covers the last bit."""
    import torch.nn.functional as F
    W = Weights(fold_weight_norm(state), torch.float64).sub("encoder.")
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(mel)).to(torch.float64)[None, None]
        bound = torch.zeros_like(x)
        for i, f in enumerate(factors):
            w, b = W[f"{i}.weight"], W[f"{i}.bias"]
            kw = dict(stride=(1, f), padding=(1, f // 2))
            y = F.conv_transpose2d(x, w, b, **kw)
            absdot = F.conv_transpose2d(x.abs() + bound, w.abs(), None, **kw)
            bound = torch.from_numpy(fb.dot_bound(absdot.numpy(), 6, float(b.abs()))) + F.conv_transpose2d(bound, w.abs(), None, **kw)
            if trim:
                y, bound = y[..., :-f], bound[..., :-f]
            x = F.leaky_relu(y, 0.4)
            bound = bound + 2.0 * fb.U * x.abs()
    return x[0, 0].numpy(), bound[0, 0].numpy()


@functools.lru_cache(maxsize=None)
def cond_ref(name, direction):
    """[(cond, bound)] per utterance as ``debug_tap("cond", b)`` returns it: after infer the trimmed upsampling cut to ``pruned``,
    after forward the untrimmed one cut to the length of z."""
    case = BY_NAME[name]
    cfg = cfg_of(case)
    state, mels, _, audios = inputs(name)
    out = []
    for b, m in enumerate(mels):
        c, bd = upsample_with_bound(state, m, cfg["upsample_factors"], trim=direction == "infer")
        n = lengths(cfg, case.frames[b])[1] if direction == "infer" else len(audios[b]) // cfg["n_group"] * cfg["n_group"]
        assert c.shape[1] >= n
        out.append((c[:, :n], bd[:, :n]))
    return out


def upsample_direct(state, mel, factors, trim, drop_second_tap=False):
    """The upsampler as the kernel states it (csrc/waveflow.hip k_wf_upsample), float64: out[c][t] = bias + sum over the input steps
    ix in {ix_hi, ix_hi - 1}, ix_hi = (t + f/2) // f, and ky in 0..2 of in[c + 1 - ky][ix] w[ky][t + f/2 - f ix].
    ``drop_second_tap``: the wrong kernel that forgets ix_hi - 1."""
    Wt = fold_weight_norm(state)
    x = np.asarray(mel, np.float64)
    for i, f in enumerate(factors):
        w = np.asarray(Wt[f"encoder.{i}.weight"], np.float64)[0, 0]
        bias = float(np.asarray(Wt[f"encoder.{i}.bias"])[0])
        M, Tin = x.shape
        Tout = f * Tin - f if trim else f * Tin
        xp = np.pad(x, ((1, 1), (0, 0)))
        y = np.full((M, Tout), bias)
        t = np.arange(Tout)
        for d in ((0,) if drop_second_tap else (0, 1)):
            ix = (t + f // 2) // f - d
            kx = t + f // 2 - f * ix
            ok = (ix >= 0) & (ix < Tin) & (kx < 2 * f)
            ixc = np.clip(ix, 0, Tin - 1)
            for ky in range(3):
                # in[c + 1 - ky] = xp[c + 2 - ky]
                y += np.where(ok, xp[2 - ky:2 - ky + M][:, ixc] * w[ky, np.clip(kx, 0, 2 * f - 1)], 0.0)
        x = np.where(y > 0, y, 0.4 * y)
    return x


def infer_from_cond(state, cond, z, cfg, dtype="f64"):
    """WaveFlow.inverse on a given condition (n_mels, >= len(z))."""
    W = Weights(fold_weight_norm(state), _DTYPE[dtype])
    with torch.no_grad():
        c = torch.from_numpy(np.asarray(cond))[None].to(_DTYPE[dtype])
        return ref.waveflow_inverse(W.sub("decoder."), torch.from_numpy(z)[None].to(_DTYPE[dtype]), c[:, :, :len(z)], cfg)[0].numpy()
