"""GPU parity: ConditionalWaveFlow at n_group 32, 64 and 128 -- residual layers with height dilations (Flow.dilations_dict,
waveflow.py:420-426; layer l of a flow looks back dh_l and 2 dh_l rows, kept in a ring of min(2 dh_l + 1, n_group) rows) -- in
both directions, against the fp64 oracles (oracle/waveflow_ref.py, tests/waveflow_forward_ref.py) and the vectors of the
reference's own source (tests/golden/waveflow_ngroup.npz).

Inputs: weights from ``syn.waveflow_state(cfg, seed, weight_norm=True)``, mels as in test_waveflow_gpu.py; forward's recordings
as in test_waveflow_forward_gpu.py (the fp64 inverse of a known z with 4 or 8 flows, 0.3 N(0, 1) with 2).

Bars -- the project's WaveFlow bars: infer within 1e-5 of the waveform's peak in the default math and "f32", 2e-3 in "f16";
forward z within 1e-5 of its peak and the log-determinant within 1e-6 nats per sample.
Measured on an MI355X: infer 9.4e-8 .. 2.5e-7 of the peak in the default math and "f32" over all the cases below
(golden vectors: 2.0e-7), 4.9e-5 in "f16"; forward z 9.9e-8 .. 1.7e-7, log-determinant 3e-10 .. 4.8e-9 nats per sample (golden
vectors: 1.6e-7 and 5.4e-9); the round trip returns z to 4.3e-7.  The regression bars are ten times the largest measured value."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import waveflow_forward_ref as fref
from oracle import waveflow_ref as ref
from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

WAV_BAR, WAV_BAR_F16, Z_BAR, LD_BAR = 1e-5, 2e-3, 1e-5, 1e-6
WAV_REG, WAV_REG_F16, Z_REG, LD_REG, TRIP_REG = 2.5e-6, 4.9e-4, 1.7e-6, 5.4e-8, 4.3e-6   # 10 x measured
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waveflow_ngroup.npz")


def _cfg(**over):
    return dict(syn.WAVEFLOW_LJSPEECH, **over)


def _key(cfg):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()))


def _unkey(cfg_key):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg_key}


def _mel(rng, n_mels, T):
    return np.maximum(rng.normal(-4, 2, size=(n_mels, T)), np.log(1e-5)).astype(np.float32)


def _cond_len(cfg, T):
    return ref.cond_length(T, cfg["upsample_factors"])


def _model(cfg, state, math=None, waves=0):
    from parakeet_amd.waveflow import ConditionalWaveFlow
    model = ConditionalWaveFlow(**cfg)
    model.set_state_dict(state)
    model.eval()
    if math:
        model.set_math(math)
    if waves:
        model.set_option("layer_waves", waves)
    return model


class _Kernels:
    """The kernel names a block launched (Context profiling, as test_waveflow_gpu.py)."""

    def __enter__(self):
        from parakeet_amd.runtime import Context
        self.ctx = Context.get()
        self.ctx.prof_enable(True)
        self.ctx.prof_reset()
        return self

    def __exit__(self, *exc):
        self.counts = {k: n for k, (n, _) in self.ctx.prof_dump().items() if n > 0}
        self.ctx.prof_enable(False)

    def check(self, present, absent):
        assert any(n.startswith(present) for n in self.counts) and not any(n.startswith(absent) for n in self.counts), self.counts


# ---------------------------------------------------------------- infer against oracle.waveflow_ref.infer (fp64)
@functools.lru_cache(maxsize=None)
def _infer_case(cfg_key, frames, seed):
    """(state, mels, zs, want) of a case, computed once and shared (never modified)."""
    cfg = _unkey(cfg_key)
    state = syn.waveflow_state(cfg, seed=seed, weight_norm=True)
    rng = np.random.default_rng(seed + 1)
    mels = [_mel(rng, cfg["n_mels"], T) for T in frames]
    zs = [rng.normal(size=(_cond_len(cfg, T),)).astype(np.float32) for T in frames]
    with torch.no_grad():
        want = [ref.infer(state, torch.from_numpy(m)[None], torch.from_numpy(z)[None], cfg, torch.float64)[0].numpy() for m, z in zip(mels, zs)]
    return state, mels, zs, want


def _run_infer(cfg_over, frames, seed, tol=WAV_BAR, math=None, expect_kernel=None):
    cfg = _cfg(**cfg_over)
    state, mels, zs, want = _infer_case(_key(cfg), tuple(frames), seed)
    model = _model(cfg, state, math)
    for T, z in zip(frames, zs):
        assert model.lengths(T)[0] == len(z) and model.lengths(T)[1] == len(z) // cfg["n_group"] * cfg["n_group"]
    with _Kernels() as k:
        outs = model.infer_batch(mels, zs)
    if expect_kernel:
        k.check(*expect_kernel)
    for b, (o, w) in enumerate(zip(outs, want)):
        got = o.numpy()
        assert got.shape == w.shape and got.dtype == np.float32
        err = np.abs(got - w).max() / np.abs(w).max()
        print(f"infer {cfg_over} math {math} utt {b} ({frames[b]} frames, {w.size // cfg['n_group']} positions): {err:.3g} of the peak")
        assert err < tol, f"utt {b}: rel err {err}"
        assert err < (WAV_REG_F16 if math == "f16" else WAV_REG), f"utt {b}: within the bar but ten times worse than measured: {err}"


def test_infer_n_group_32_ragged():
    """64 / 24 / 40 positions per row: tiles straddle utterances and gaps; rings of 3 / 5 / 9 rows wrap several times in 31 steps."""
    _run_infer(dict(channels=64, n_flows=2, n_group=32), [9, 4, 6], seed=31)


def test_infer_n_group_64_all_flows():
    """All 8 flows: both permutation kinds and their cumulative effect on the condition; the ring of 33 rows wraps in 63 steps."""
    _run_infer(dict(channels=64, n_group=64), [5, 3], seed=32)


def test_infer_n_group_128():
    """22 and 4 positions.  The dh = 64 layer never gets its first kernel row (at most 6 taps), the dh = 32 ring of 65 rows wraps."""
    _run_infer(dict(channels=64, n_flows=2, n_group=128), [12, 3], seed=33)


def test_infer_n_group_64_c128():
    _run_infer(dict(channels=128, n_flows=2, n_group=64), [4], seed=34)


def test_infer_n_group_32_96_mels_runs_unfused():
    _run_infer(dict(channels=64, n_flows=2, n_group=32, n_mels=96), [4, 3], seed=35,
               expect_kernel=("wf_gemm_conv_gate", ("wf_layer", "wf_row")))
    _run_infer(dict(channels=64, n_flows=2, n_group=32), [4, 3], seed=35, expect_kernel=("wf_layer", ("wf_gemm_conv_gate", "wf_row")))


def test_infer_n_group_64_exact_fp32_math():
    _run_infer(dict(channels=64, n_flows=2, n_group=64), [4, 3], seed=36, math="f32", expect_kernel=("wf_gemm_conv_gate", ("wf_layer", "wf_row")))


def test_infer_n_group_64_fp16_operand_mode():
    _run_infer(dict(channels=64, n_flows=2, n_group=64), [9, 4], seed=37, tol=WAV_BAR_F16, math="f16")


# ---------------------------------------------------------------- the reference source's vectors through the engine
@pytest.mark.parametrize("n_group", [32, 64, 128])
def test_golden_through_the_engine(n_group):
    g = np.load(GOLD)
    cfg = _cfg(channels=64, n_flows=2, n_group=n_group)
    model = _model(cfg, syn.waveflow_state(cfg, seed=int(g["seed"]), weight_norm=True))
    mel, want = g[f"mel_{n_group}"], g[f"wav_{n_group}"]
    wav = model.infer(mel, g[f"z_{n_group}"]).numpy()
    assert wav.shape == want.shape
    err = np.abs(wav - want).max() / np.abs(want).max()
    zw, lw = g[f"fz_{n_group}"], float(g[f"logdet_{n_group}"][0])
    z, ld = model(g[f"audio_{n_group}"], mel)
    z = z.numpy()
    assert z.shape == zw.shape
    ez = np.abs(z - zw).max() / np.abs(zw).max()
    el = abs(float(ld[0]) - lw) / zw.size
    print(f"golden n_group {n_group}: infer {err:.3g}, forward z {ez:.3g} of the peak, logdet {el:.3g} nats per sample")
    # (the vectors are fp32 results of the reference's source: their own distance to fp64 is part of these numbers, as in
    # test_golden_cpu.py -- same bars)
    assert err < WAV_BAR
    assert ez < Z_BAR
    assert el < LD_BAR + 1e-7 * abs(lw) / zw.size   # (+ the fp32 return value's rounding, as test_waveflow_forward_gpu.py)
    assert err < WAV_REG and ez < Z_REG and el < LD_REG + 1e-7 * abs(lw) / zw.size, f"ten times worse than measured: {err}, {ez}, {el}"


# ---------------------------------------------------------------- infer: determinism (no oracle)
def test_infer_n_group_64_deterministic_any_waves_any_batch():
    """8 flows, 160 / 40 / 7 frames (635 / 155 / 23 positions: several tiles per workgroup): the waveform is the same bit for bit
    with 8- and 12-wave workgroups and the launcher's choice, in three calls, and for every utterance alone."""
    cfg = _cfg(channels=64, n_group=64)
    model = _model(cfg, syn.waveflow_state(cfg, seed=77, weight_norm=True))
    rng = np.random.default_rng(78)
    frames = [160, 40, 7]
    mels = [_mel(rng, 80, T) for T in frames]
    zs = [rng.normal(size=(model.lengths(T)[0],)).astype(np.float32) for T in frames]
    outs = {}
    for w in (8, 12, 0):
        model.set_option("layer_waves", w)
        outs[w] = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
    assert all(np.isfinite(o).all() and np.abs(o).max() > 0 for o in outs[0])
    for w in (8, 12):
        for b, (a, o) in enumerate(zip(outs[0], outs[w])):
            assert np.array_equal(a, o), f"layer_waves {w}: utterance {b} differs from the launcher's choice"
    for r in range(2):
        for b, (a, o) in enumerate(zip(outs[0], model.infer_batch(mels, zs))):
            assert np.array_equal(a, o.numpy()), f"call {r + 2}: utterance {b} differs from the first call"
    for b in range(3):
        alone, = model.infer_batch([mels[b]], [zs[b]])
        assert np.array_equal(outs[0][b], alone.numpy()), f"utterance {b} alone differs from its result in the batch"


# ---------------------------------------------------------------- forward against waveflow_forward_ref.forward (fp64)
@functools.lru_cache(maxsize=None)
def _forward_case(cfg_key, frames, seed):
    """(state, mels, audios, want z, want logdet): recordings of T * 256 - 37 - 5 b samples -- not a multiple of n_group, shorter
    than the condition -- built as in test_waveflow_forward_gpu.py's _case.  Computed once and shared (never modified)."""
    cfg = _unkey(cfg_key)
    state = syn.waveflow_state(cfg, seed=seed, weight_norm=True)
    rng = np.random.default_rng(seed + 1)
    hop = int(np.prod(cfg["upsample_factors"]))
    mels, audios, zs, lds = [], [], [], []
    for i, T in enumerate(frames):
        mel = _mel(rng, cfg["n_mels"], T)
        n = T * hop - 37 - 5 * i
        if cfg["n_flows"] % 4 == 0:
            zn = rng.normal(size=(1, n))
            audio = fref.inverse(state, zn, mel[None], cfg, torch.float64)[0].numpy().astype(np.float32)
            audio = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])   # the samples _trim cuts
        else:
            audio = (0.3 * rng.normal(size=n)).astype(np.float32)
        z, ld = fref.forward(state, audio[None], mel[None], cfg, torch.float64)
        mels.append(mel)
        audios.append(audio)
        zs.append(z[0].numpy())
        lds.append(float(ld[0]))
    return state, mels, audios, zs, lds


def _check_forward(outs, zs, lds, tag):
    for b, ((z, ld), zw, lw) in enumerate(zip(outs, zs, lds)):
        z = z.numpy()
        assert z.shape == zw.shape and z.dtype == np.float32
        ez = np.abs(z - zw).max() / np.abs(zw).max()
        el = abs(float(ld) - lw) / zw.size
        print(f"forward {tag} utt {b}: z {ez:.3g} of the peak, logdet {el:.3g} nats per sample (logdet {float(ld):.4f}, {zw.size} samples)")
        assert ez < Z_BAR, f"utt {b}: z rel err {ez}"
        assert ez < TRIP_REG, f"utt {b}: within the bar but ten times worse than measured: {ez}"
        assert el < LD_BAR, f"utt {b}: logdet off by {el} nats per sample"
        assert ez < Z_REG and el < LD_REG, f"utt {b}: within the bars but ten times worse than measured: z {ez}, logdet {el}"


def _run_forward(cfg_over, frames, seed, math=None, expect_kernel=None):
    cfg = _cfg(**cfg_over)
    state, mels, audios, zs, lds = _forward_case(_key(cfg), tuple(frames), seed)
    model = _model(cfg, state, math)
    for T, a, zw in zip(frames, audios, zs):
        assert model.forward_length(T, len(a)) == len(zw) == len(a) // cfg["n_group"] * cfg["n_group"]
    with _Kernels() as k:
        outs = model.forward_batch(audios, mels)
    if expect_kernel:
        k.check(*expect_kernel)
    _check_forward(outs, zs, lds, f"{cfg_over} math {math}")


@pytest.mark.parametrize("n_group", [32, 64, 128])
def test_forward_four_flows_recovers_z(n_group):
    _run_forward(dict(channels=64, n_flows=4, n_group=n_group), [4, 3], seed=40 + n_group)


def test_forward_n_group_64_c128():
    _run_forward(dict(channels=128, n_flows=4, n_group=64), [4, 3], seed=51)


def test_forward_n_group_32_exact_fp32_math():
    _run_forward(dict(channels=64, n_flows=4, n_group=32), [4, 3], seed=52, math="f32", expect_kernel=("wf_gemm_conv_gate", ("wf_layer", "wf_row")))


def test_forward_n_group_64_96_mels_runs_unfused():
    _run_forward(dict(channels=64, n_flows=2, n_group=64, n_mels=96), [4, 3], seed=53, expect_kernel=("wf_gemm_conv_gate", ("wf_layer", "wf_row")))


@pytest.mark.parametrize("n_group", [64, 128])
def test_forward_layer_launches_do_not_grow_with_n_group(n_group):
    """A fused-path forward of 8 flows issues n_flows x n_layers = 64 layer launches at any n_group."""
    cfg = _cfg(channels=64, n_group=n_group)
    model = _model(cfg, syn.waveflow_state(cfg, seed=4, weight_norm=True))
    rng = np.random.default_rng(4)
    mel = _mel(rng, 80, 3)
    audio = (0.3 * rng.normal(size=700)).astype(np.float32)
    model.forward_batch([audio], [mel])
    with _Kernels() as k:
        model.forward_batch([audio], [mel])
    counts = k.counts
    assert counts.get("wf_layer") == 64, counts
    assert counts.get("wf_inproj_rows") == 8 and counts.get("wf_cond_planes_rows") == 8 and counts.get("wf_affine_rows") == 8, counts


def test_forward_n_group_64_batch_equals_single_calls_bit_for_bit():
    cfg = _cfg(channels=64, n_flows=4, n_group=64)
    model = _model(cfg, syn.waveflow_state(cfg, seed=77, weight_norm=True))
    rng = np.random.default_rng(5)
    frames = [40, 12, 7]
    mels = [_mel(rng, 80, T) for T in frames]
    audios = [(0.3 * rng.normal(size=T * 256 - 3 * i)).astype(np.float32) for i, T in enumerate(frames)]
    batch = model.forward_batch(audios, mels)
    for b in range(3):
        (z1, l1), = model.forward_batch([audios[b]], [mels[b]])
        assert np.isfinite(z1.numpy()).all()
        assert np.array_equal(batch[b][0].numpy(), z1.numpy()), f"utterance {b}: z differs between the batch and the single call"
        assert float(batch[b][1]) == float(l1), f"utterance {b}: logdet differs"


# ---------------------------------------------------------------- round trip and API
def test_round_trip_n_group_64_all_flows():
    """forward(infer(mel, z), mel) = z on the engine.  (infer's trimmed condition equals the untrimmed one on the samples it keeps.)"""
    cfg = _cfg(channels=64, n_group=64)
    model = _model(cfg, syn.waveflow_state(cfg, seed=61, weight_norm=True))
    rng = np.random.default_rng(62)
    frames = [6, 4]
    mels = [_mel(rng, 80, T) for T in frames]
    zs = [rng.normal(size=(model.lengths(T)[0],)).astype(np.float32) for T in frames]
    wavs = model.infer_batch(mels, zs)
    back = model.forward_batch([w.numpy() for w in wavs], mels)
    for b, ((z, ld), zw) in enumerate(zip(back, zs)):
        z = z.numpy()
        zw = zw[:len(z)]
        assert len(z) == model.lengths(frames[b])[1] and np.isfinite(float(ld))
        ez = np.abs(z - zw).max() / np.abs(zw).max()
        print(f"round trip utt {b}: z {ez:.3g} of the peak")
        assert ez < Z_BAR, f"utt {b}: z rel err {ez}"
        assert ez < TRIP_REG, f"utt {b}: within the bar but ten times worse than measured: {ez}"


def test_envelope_and_lengths():
    from parakeet_amd.waveflow import ConditionalWaveFlow
    cfg = _cfg(channels=64, n_flows=2)
    for g in (4, 24, 256):                        # even, but no key of Flow.dilations_dict (a KeyError in the reference)
        with pytest.raises(NotImplementedError):
            ConditionalWaveFlow(**dict(cfg, n_group=g))
    with pytest.raises(ValueError):
        ConditionalWaveFlow(**dict(cfg, n_group=6, n_flows=3))   # odd flows (waveflow.py:586-589)
    for g in (32, 64, 128):
        m = ConditionalWaveFlow(**dict(cfg, n_group=g))
        for T in (3, 7, 40):
            cond, wav = m.lengths(T)
            assert cond == ref.cond_length(T, cfg["upsample_factors"]) and wav == cond // g * g and wav % g == 0 and wav > 0
            n = m.forward_length(T, T * 256 - 37)
            assert n == (T * 256 - 37) // g * g and n % g == 0
        with pytest.raises(NotImplementedError):
            m.set_option("persistent", 1)


def test_from_pretrained_with_n_group_64(tmp_path):
    """A released-layout checkpoint (`<path>.pdparams`, config with `model` / `data` sections) whose config says n_group 64."""
    from parakeet_amd.waveflow import ConditionalWaveFlow

    class Node(dict):
        __getattr__ = dict.__getitem__
    wcfg = _cfg(channels=64, n_flows=2, n_group=64)
    config = Node(data=Node(n_mels=80, sample_rate=22050), model=Node({k: v for k, v in wcfg.items() if k != "n_mels"}))
    state = syn.waveflow_state(wcfg, seed=5, weight_norm=True)
    with open(tmp_path / "step-1.pdparams", "wb") as f:
        pickle.dump(dict(state), f, protocol=2)
    model = ConditionalWaveFlow.from_pretrained(config, str(tmp_path / "step-1"))
    assert model.n_group == 64
    model.eval()
    rng = np.random.default_rng(6)
    mel = _mel(rng, 80, 4)
    z = rng.normal(size=(model.lengths(4)[0],)).astype(np.float32)
    with torch.no_grad():
        want = ref.infer(state, torch.from_numpy(mel)[None], torch.from_numpy(z)[None], wcfg, torch.float64)[0].numpy()
    got = model.predict(mel, z)
    assert got.shape == want.shape == (model.lengths(4)[1],)
    assert np.abs(got - want).max() / np.abs(want).max() < WAV_BAR
