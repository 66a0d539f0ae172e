"""ConditionalWaveFlow.forward, CPU side: the fp64 restatement (tests/waveflow_forward_ref.py) against the golden vectors the
reference's own ``ConditionalWaveFlow.forward`` / ``WaveFlowLoss`` produced (tools/make_golden_waveflow_forward.py ->
golden/waveflow_forward_c64.npz), and the fact the GPU tests' inputs rest on: WaveFlow.forward inverts WaveFlow.inverse only
when the flows' row permutations compose to the identity (n_flows a multiple of 4)."""
import os

import numpy as np
import pytest
import torch

import waveflow_forward_ref as fref
from parakeet_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")   # (the golden_source fixture points it at golden_paddle)
CFG = dict(syn.WAVEFLOW_LJSPEECH, channels=64)


@pytest.fixture(scope="module")
def state():
    return syn.waveflow_state(CFG, seed=314, weight_norm=True)


def _gold():
    return np.load(os.path.join(GOLD, "waveflow_forward_c64.npz"))


@pytest.mark.parametrize("b", [0, 1])
def test_restatement_matches_the_reference_forward(state, b):
    g = _gold()
    audio, mel = g[f"audio{b}"], g["mel"][b:b + 1]
    z, logdet = fref.forward(state, audio[None], mel, CFG, torch.float64)
    z, logdet = z[0].numpy(), float(logdet[0])
    assert z.shape == g[f"z{b}"].shape == (len(audio) // 16 * 16,)
    err = np.abs(z - g[f"z{b}"]).max() / np.abs(g[f"z{b}"]).max()
    print(f"utterance {b}: z rel err {err:.3g}, logdet {logdet:.6f} vs {float(g[f'logdet{b}'][0]):.6f}")
    assert err < 5e-6, err                                                   # measured 5.6e-7 (the golden is fp32)
    assert abs(logdet - float(g[f"logdet{b}"][0])) / z.size < 1e-6           # nats per sample


@pytest.mark.parametrize("b", [0, 1])
def test_loss_formula_matches_the_reference(b):
    g = _gold()
    for s, want in zip(g["sigmas"], g[f"loss{b}"]):
        got = fref.loss(g[f"z{b}"], g[f"logdet{b}"], float(s))
        assert abs(got - want) < 2e-6, (s, got, want)                        # the reference computes it in fp32 (value about 1)


@pytest.mark.parametrize("n_flows,inverts", [(4, True), (8, True), (2, False)])
def test_forward_inverts_inverse_only_when_the_permutations_compose_to_identity(n_flows, inverts):
    cfg = dict(CFG, n_flows=n_flows)
    st = syn.waveflow_state(cfg, seed=5, weight_norm=True)
    rng = np.random.default_rng(6)
    mel = np.maximum(rng.normal(-4, 2, size=(1, 80, 2)), np.log(1e-5))
    z = rng.normal(size=(1, 400))
    x = fref.inverse(st, z, mel, cfg, torch.float64)
    z2, _ = fref.forward(st, x, mel, cfg, torch.float64)
    err = float((z2 - torch.as_tensor(z)).abs().max())
    assert (err < 1e-9) if inverts else (err > 1e-3), err
