"""HiFi-GAN's waveforms are the bits they were before its convolution kernel moved into csrc/pk_hfg_conv.h and gained a
boundary parameter: tests/golden/hifigan_tiny_waveforms.npz holds the seven TINY waveforms in both maths, recorded on the
commit before the move."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import hifigan_ref as hr  # noqa: E402

from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hifigan_tiny_waveforms.npz")


@pytest.mark.parametrize("math", hr.MATHS)
def test_tiny_waveforms_are_the_recorded_bits(math):
    from parakeet_amd.hifigan import HiFiGANGenerator
    cfg = hr.CONFIGS["TINY"]
    g = HiFiGANGenerator(**hr.ctor_kwargs(cfg))
    g.set_state_dict(syn.hifigan_state(cfg, seed=hr.SEEDS["TINY"]))
    g.eval()
    g.set_math(math)
    mels = hr.make_mels("TINY")
    golden = np.load(GOLDEN)
    assert len(mels) == 7
    for b, o in enumerate(g.inference_batch(mels)):
        got = o.as_subclass(torch.Tensor).cpu().numpy()[:, 0]
        want = golden[f"{math}_{b}"]
        assert want.shape == (len(mels[b]) * 6,) and np.abs(want).max() > 0.1
        np.testing.assert_array_equal(got, want)
