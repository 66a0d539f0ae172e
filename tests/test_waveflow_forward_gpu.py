"""GPU parity: ConditionalWaveFlow.forward / forward_batch / WaveFlowLoss / log_likelihood (HIP through the C ABI) against the
fp64 restatement of the reference (tests/waveflow_forward_ref.py).

Inputs: weights from ``syn.waveflow_state(..., weight_norm=True)``, mels as in test_waveflow_gpu.py.  With 4 or 8 flows the audio
is the fp64 ``waveflow_inverse`` of a seeded normal z under the untrimmed condition, so z is also the known answer; with 2 flows
(whose permutations do not compose to the identity, tests/test_waveflow_forward_cpu.py) it is 0.3 N(0, 1).

Bars (default math and "f32"): z within 1e-5 of its peak (the project's WaveFlow bar; the per-row arithmetic is infer's) and the
log-determinant within 1e-6 nats per sample (100 x the fp32 CPU restatement's own error, 1e-5 of the value).  "f16": 2e-3, the
project's bar for f16 infer.
Measured on an MI355X: z 9e-8 .. 2.6e-7, log-determinant 7e-11 .. 1.2e-8 nats per sample in the default math and
"f32"; "f16" at 2 x 160 frames: z 1.6e-4, log-determinant 4.0e-5.  The regression bars are ten times the largest measured value."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import waveflow_forward_ref as fref
from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Z_BAR, LD_BAR, Z_BAR_F16, LD_BAR_F16 = 1e-5, 1e-6, 2e-3, 2e-3
Z_REG, LD_REG, Z_REG_F16, LD_REG_F16 = 2.6e-6, 1.2e-7, 1.6e-3, 4.1e-4   # 10 x measured


def _cfg(**over):
    return dict(syn.WAVEFLOW_LJSPEECH, **over)


def _key(cfg):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()))


@functools.lru_cache(maxsize=None)
def _case(cfg_key, frames, seed, short):
    """(state, mels, audios, want z, want logdet) of a case, computed once and shared (never modified)."""
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg_key}
    state = syn.waveflow_state(cfg, seed=seed, weight_norm=True)
    rng = np.random.default_rng(seed + 1)
    hop = int(np.prod(cfg["upsample_factors"]))
    mels, audios, zs, lds = [], [], [], []
    for i, T in enumerate(frames):
        mel = np.maximum(rng.normal(-4, 2, size=(cfg["n_mels"], T)), np.log(1e-5)).astype(np.float32)
        n = T * hop - (37 + 5 * i if short else 0)      # not a multiple of n_group, shorter than frames x hop
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


def _check(outs, zs, lds, z_bar=Z_BAR, ld_bar=LD_BAR, tag="", z_reg=Z_REG, ld_reg=LD_REG):
    for b, ((z, ld), zw, lw) in enumerate(zip(outs, zs, lds)):
        z = z.numpy()
        assert z.shape == zw.shape and z.dtype == np.float32
        ez = np.abs(z - zw).max() / np.abs(zw).max()
        el = abs(float(ld) - lw) / zw.size
        print(f"{tag} utt {b}: z rel err {ez:.3g}, logdet err {el:.3g} nats/sample (logdet {float(ld):.4f}, {zw.size} samples)")
        assert ez < z_bar, f"utt {b}: z rel err {ez}"
        assert el < ld_bar, f"utt {b}: logdet off by {el} nats per sample"
        assert ez < z_reg and el < ld_reg, f"utt {b}: within the bars but ten times worse than measured: z {ez}, logdet {el}"


def _run(cfg_over, frames, seed, math=None, short=True, expect_kernel=None, **bars):
    cfg = _cfg(**cfg_over)
    state, mels, audios, zs, lds = _case(_key(cfg), tuple(frames), seed, short)
    model = _model(cfg, state, math)
    if expect_kernel:
        from parakeet_amd.runtime import Context
        ctx = Context.get()
        ctx.prof_enable(True)
        ctx.prof_reset()
    outs = model.forward_batch(audios, mels)
    if expect_kernel:
        names = {k for k, (n, _) in ctx.prof_dump().items() if n > 0}
        ctx.prof_enable(False)
        present, absent = expect_kernel
        assert any(n.startswith(present) for n in names) and not any(n.startswith(absent) for n in names), names
    _check(outs, zs, lds, tag=str(cfg_over), **bars)
    return model, outs


def test_forward_c64_two_flows_ragged():
    _run(dict(channels=64, n_flows=2), [4, 7, 3], seed=1)


def test_forward_c64_all_flows_recovers_z():
    _run(dict(channels=64), [5, 3], seed=2)


def test_forward_c128_four_flows():
    _run(dict(channels=128, n_flows=4), [4], seed=3)


def test_forward_96_mel_channels_runs_unfused():
    _run(dict(channels=64, n_flows=2, n_mels=96), [4, 3], seed=6, expect_kernel=("wf_gemm_conv_gate", ("wf_layer", "wf_row")))
    _run(dict(channels=64, n_flows=2), [4, 3], seed=6, expect_kernel=("wf_layer", "wf_gemm_conv_gate"))


def test_forward_exact_fp32_math():
    _run(dict(channels=64, n_flows=2), [4, 7, 3], seed=1, math="f32")


def test_forward_n_group_8():
    _run(dict(channels=64, n_flows=4, n_group=8), [4, 3], seed=8)


@pytest.mark.parametrize("waves", [8, 12])
def test_forward_every_wave_works_several_rounds_deterministic(waves):
    """2 x 160 frames: 160 position tiles x 15 rows, so every wave of a workgroup takes tiles and workgroups run more than one
    round.  Against fp64, and three calls equal bit for bit."""
    cfg = _cfg(channels=64)
    state, mels, audios, zs, lds = _case(_key(cfg), (160, 160), 77, False)
    model = _model(cfg, state, waves=waves)
    runs = [model.forward_batch(audios, mels) for _ in range(3)]
    _check(runs[0], zs, lds, tag=f"waves {waves}")
    for r in runs[1:]:
        for (z0, l0), (z1, l1) in zip(runs[0], r):
            assert np.array_equal(z0.numpy(), z1.numpy()) and float(l0) == float(l1)


def test_forward_batch_equals_single_calls_bit_for_bit():
    cfg = _cfg(channels=64)
    state = syn.waveflow_state(cfg, seed=77, weight_norm=True)
    rng = np.random.default_rng(5)
    frames = [160, 40, 7]
    mels = [np.maximum(rng.normal(-4, 2, size=(80, T)), np.log(1e-5)).astype(np.float32) for T in frames]
    audios = [(0.3 * rng.normal(size=T * 256 - 3 * i)).astype(np.float32) for i, T in enumerate(frames)]
    model = _model(cfg, state)
    batch = model.forward_batch(audios, mels)
    for b in range(3):
        (z1, l1), = model.forward_batch([audios[b]], [mels[b]])
        assert np.array_equal(batch[b][0].numpy(), z1.numpy()), f"utterance {b}: z differs between the batch and the single call"
        assert float(batch[b][1]) == float(l1), f"utterance {b}: logdet differs"


def test_forward_fp16_operand_mode():
    cfg = _cfg(channels=64)
    state, mels, audios, zs, lds = _case(_key(cfg), (160, 160), 77, False)
    model = _model(cfg, state, math="f16")
    _check(model.forward_batch(audios, mels), zs, lds, z_bar=Z_BAR_F16, ld_bar=LD_BAR_F16, tag="f16", z_reg=Z_REG_F16, ld_reg=LD_REG_F16)


def test_forward_errors():
    from parakeet_amd import _capi
    from parakeet_amd.waveflow import ConditionalWaveFlow
    cfg = _cfg(channels=64, n_flows=2)
    state = syn.waveflow_state(cfg, seed=5, weight_norm=True)
    model = _model(cfg, state)
    mel = np.random.default_rng(0).normal(-4, 1, size=(80, 4)).astype(np.float32)
    with pytest.raises(ValueError):
        model.forward_batch([np.zeros(4 * 256 + 1, np.float32)], [mel])     # longer than the condition
    with pytest.raises(ValueError):
        model.forward_batch([np.zeros(15, np.float32)], [mel])              # shorter than n_group
    fresh = ConditionalWaveFlow(**cfg)
    fresh.set_state_dict(state)                                             # ... but not finalized
    dev = torch.zeros(4 * 80 + 1024 + 1024, device="cuda")
    ld = torch.zeros(1, dtype=torch.float64, device="cuda")
    frames, alen = (C.c_int32 * 1)(4), (C.c_int32 * 1)(1024)
    st = fresh._ctx.lib.pk_wf_forward(fresh._h, C.c_void_p(dev.data_ptr()), frames, C.c_void_p(dev.data_ptr()), alen, 1,
                                      C.c_void_p(dev.data_ptr()), C.c_void_p(ld.data_ptr()), 0)
    assert st == -6, st                                                     # PK_ESTATE (include/pk_synth.h)
    with pytest.raises(RuntimeError):
        _capi.check(st)


def test_forward_api_shapes_loss_and_log_likelihood():
    from parakeet_amd.waveflow import ConditionalWaveFlow, WaveFlowLoss
    import parakeet_amd.waveflow as wfm
    assert "WaveFlowLoss" in wfm.__all__
    cfg = _cfg(channels=64, n_flows=2)
    state = syn.waveflow_state(cfg, seed=5, weight_norm=True)
    model = _model(cfg, state)
    rng = np.random.default_rng(9)
    mel = np.maximum(rng.normal(-4, 2, size=(2, 80, 4)), np.log(1e-5)).astype(np.float32)
    audio = (0.3 * rng.normal(size=(2, 1000))).astype(np.float32)
    z, ldj = model(audio, mel)
    assert tuple(z.shape) == (2, 992) and tuple(ldj.shape) == (1,) and ldj.dtype == torch.float32
    zw, lw = fref.forward(state, audio, mel, cfg, torch.float64)
    assert np.abs(z.numpy() - zw.numpy()).max() / np.abs(zw.numpy()).max() < Z_BAR
    assert abs(float(ldj[0]) - float(lw.sum())) / zw.numel() < LD_BAR + 1e-7 * abs(float(lw.sum())) / zw.numel()   # (+ the fp32 return value's rounding)
    for sigma in (1.0, 0.7):
        crit = WaveFlowLoss(sigma=sigma)
        assert abs(crit.const - (0.5 * np.log(2 * np.pi) + np.log(sigma))) < 1e-12
        got = float(crit(z, ldj))
        assert abs(got - fref.loss(zw.numpy(), lw.numpy(), sigma)) < 5e-6
        lls = model.log_likelihood([audio[0], audio[1]], [mel[0], mel[1]], sigma=sigma)
        for b in range(2):
            assert abs(lls[b] + fref.loss(zw[b].numpy(), lw[b].numpy(), sigma)) < 5e-6


@pytest.mark.parametrize("n_group", [8, 16])
def test_forward_layer_launches_do_not_grow_with_n_group(n_group):
    """A fused-path forward of 8 flows issues n_flows x n_layers = 64 layer launches, whatever n_group (infer: 64 x (n_group - 1))."""
    from parakeet_amd.runtime import Context
    cfg = _cfg(channels=64, n_group=n_group)
    model = _model(cfg, syn.waveflow_state(cfg, seed=4, weight_norm=True))
    rng = np.random.default_rng(4)
    mel = np.maximum(rng.normal(-4, 2, size=(80, 3)), np.log(1e-5)).astype(np.float32)
    audio = (0.3 * rng.normal(size=700)).astype(np.float32)
    model.forward_batch([audio], [mel])
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    model.forward_batch([audio], [mel])
    counts = {k: n for k, (n, _) in ctx.prof_dump().items() if n > 0}
    ctx.prof_enable(False)
    assert counts.get("wf_layer") == 64, counts
    assert counts.get("wf_inproj_rows") == 8 and counts.get("wf_cond_planes_rows") == 8 and counts.get("wf_affine_rows") == 8, counts
