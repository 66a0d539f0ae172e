"""The two WaveFlow oracles at n_group 32, 64 and 128 -- residual layers with height dilations (Flow.dilations_dict,
waveflow.py:420-426) -- against vectors computed by the reference's own source (tools/make_golden_waveflow_ngroup.py):
``oracle.waveflow_ref.infer`` and ``waveflow_forward_ref.forward``, in fp32 as the goldens.

Bars: waveform and z within 1e-5 of the peak (the bar test_golden_cpu.py holds waveflow_c64.npz to), log-determinant within 1e-6
nats per sample."""
import os

import numpy as np
import pytest
import torch

import waveflow_forward_ref as fref
from oracle import waveflow_ref
from parakeet_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waveflow_ngroup.npz")
N_GROUPS = (32, 64, 128)


def _load(n_group):
    g = np.load(GOLD)
    assert tuple(int(v) for v in g["n_groups"]) == N_GROUPS
    cfg = dict(syn.WAVEFLOW_LJSPEECH, channels=64, n_flows=2, n_group=n_group)
    state = syn.waveflow_state(cfg, seed=int(g["seed"]), weight_norm=True)
    return g, cfg, state


@pytest.mark.parametrize("n_group", N_GROUPS)
def test_infer_oracle_matches_reference_source(n_group):
    g, cfg, state = _load(n_group)
    want = g[f"wav_{n_group}"]
    with torch.no_grad():
        wav = waveflow_ref.infer(state, torch.from_numpy(g[f"mel_{n_group}"]), torch.from_numpy(g[f"z_{n_group}"]), cfg).numpy()
    assert wav.shape == want.shape and want.shape[1] % n_group == 0 and want.shape[1] > 0
    err = np.abs(wav - want).max() / max(1.0, np.abs(want).max())
    print(f"n_group {n_group}: infer oracle vs reference source {err:.3g} of the peak")
    assert err < 1e-5


@pytest.mark.parametrize("n_group", N_GROUPS)
def test_forward_oracle_matches_reference_source(n_group):
    g, cfg, state = _load(n_group)
    want, want_ld = g[f"fz_{n_group}"], float(g[f"logdet_{n_group}"][0])
    z, ld = fref.forward(state, g[f"audio_{n_group}"], g[f"mel_{n_group}"], cfg, torch.float32)
    z = z.numpy()
    assert z.shape == want.shape and want.shape[1] == (3 * 256 - 37) // n_group * n_group
    err = np.abs(z - want).max() / max(1.0, np.abs(want).max())
    eld = abs(float(ld.sum()) - want_ld) / want.size
    print(f"n_group {n_group}: forward oracle vs reference source z {err:.3g} of the peak, logdet {eld:.3g} nats per sample")
    assert err < 1e-5
    assert eld < 1e-6
