"""The fp64 PWG oracle (oracle/pwg_ref.py) against the reference's own PWGGenerator at four non-default shapes
(tests/golden/pwg_sizes.npz, written by tools/make_golden_pwg_sizes.py): small 32/64/32, large 128/256/128, aux 64 with
kernel 5 at hop 300, and an uneven 96/160/32 with aux 100.  This pins the restatement the engine tests compare against to
the reference's source at shapes other than the LJSpeech recipe's.

The archive is the stand-in's (oracle/paddle_shim); tools/verify_with_paddle.py re-pins it under PaddlePaddle.  The
conftest's GOLDEN_MODULES list is not extended, so these tests always read the stand-in goldens."""
import os

import numpy as np
import pytest
import torch

from oracle import pwg_ref
from parakeet_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS, config = syn.PWG_SIZES, syn.pwg_size_config
GOLD = os.path.join(HERE, "golden", "pwg_sizes.npz")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_matches_reference_at_size(name):
    g = np.load(GOLD)
    cfg = config(name)
    state = {k: torch.from_numpy(v) for k, v in syn.pwg_state(cfg, seed=int(g[f"{name}_seed"]), weight_norm=True).items()}
    y = pwg_ref.generator_forward(state, torch.from_numpy(g[f"{name}_fwd_x"]), torch.from_numpy(g[f"{name}_fwd_c"]), cfg,
                                  torch.float64)
    assert y.shape == g[f"{name}_fwd_y"].shape
    assert _rel(y.numpy(), g[f"{name}_fwd_y"]) < 1e-5
    wav = pwg_ref.generator_inference(state, torch.from_numpy(g[f"{name}_inf_mel"]),
                                      torch.from_numpy(g[f"{name}_inf_noise"]), cfg, torch.float64)
    assert wav.shape == g[f"{name}_inf_wav"].shape
    assert _rel(wav.numpy(), g[f"{name}_inf_wav"]) < 1e-5


def test_golden_shapes_are_the_issue_configurations():
    g = np.load(GOLD)
    assert config("B")["residual_channels"] == 128 and config("B")["gate_channels"] == 256
    assert int(np.prod(config("C")["upsample_scales"])) == 300 and config("C")["kernel_size"] == 5
    assert g["C_fwd_x"].shape[-1] == 3 * 300 and g["D_fwd_c"].shape[1] == 100
    assert os.path.getsize(GOLD) < 1 << 20
