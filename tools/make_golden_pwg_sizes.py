#!/usr/bin/env python
"""Generate tests/golden/pwg_sizes.npz: the reference's own PWGGenerator at four non-default shapes.

Runs parakeet/models/parallel_wavegan/parallel_wavegan.py over the paddle stand-in (oracle/paddle_shim) through
tools/ref_import.py, like golden_pwg() in tools/make_golden.py, with weight-norm pairs.  For every configuration it
records forward(x, c) on a batch of two and inference(mel) with the in-call randn replaced by a recorded draw.
Weights are not stored: parakeet_amd.synthetic.pwg_state regenerates them from the stored seed.
tools/verify_with_paddle.py runs this file under PaddlePaddle itself to re-pin the archive.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402

from parakeet_amd import synthetic as syn  # noqa: E402

OUT = ref_import.golden_dir()

CONFIGS = syn.PWG_SIZES
SEEDS = {"A": 101, "B": 102, "C": 103, "D": 104}


def config(name):
    return syn.pwg_size_config(name)


def golden_pwg_sizes():
    pw = ref_import.load("parakeet.models.parallel_wavegan.parallel_wavegan")
    out = {}
    for i, name in enumerate(CONFIGS):
        cfg = config(name)
        hop = int(np.prod(cfg["upsample_scales"]))
        aux, ctx = cfg["aux_channels"], cfg["aux_context_window"]
        state = syn.pwg_state(cfg, seed=SEEDS[name], weight_norm=True)
        gen = pw.PWGGenerator(**cfg)
        gen.set_state_dict(state)
        gen.remove_weight_norm()
        gen.eval()
        rng = np.random.default_rng(200 + i)
        x = rng.normal(size=(2, 1, 3 * hop)).astype(np.float32)
        c = rng.normal(size=(2, aux, 3 + 2 * ctx)).astype(np.float32)
        with paddle.no_grad():
            out[f"{name}_fwd_y"] = gen(paddle.to_tensor(x), paddle.to_tensor(c)).numpy().astype(np.float32)
        out[f"{name}_fwd_x"], out[f"{name}_fwd_c"] = x, c
        mel = rng.normal(size=(4, aux)).astype(np.float32)
        noise = rng.normal(size=(1, 1, 4 * hop)).astype(np.float32)
        with ref_import.fixed_randn(noise), paddle.no_grad():
            out[f"{name}_inf_wav"] = gen.inference(paddle.to_tensor(mel)).numpy().astype(np.float32)
        out[f"{name}_inf_mel"], out[f"{name}_inf_noise"] = mel, noise.reshape(-1)
        out[f"{name}_seed"] = np.array(SEEDS[name])
        print(f"pwg {name}:", out[f"{name}_fwd_y"].shape, out[f"{name}_inf_wav"].shape, flush=True)
    np.savez_compressed(os.path.join(OUT, "pwg_sizes.npz"), **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    golden_pwg_sizes()
