#!/usr/bin/env python
"""tests/golden/pwg_disc.npz: the REFERENCE's own PWGDiscriminator (parakeet/models/parallel_wavegan/parallel_wavegan.py
:523-630) run over the torch-backed stand-in of paddle (tools/ref_import.py), and the three MSE numbers the evaluator forms
of its logits (parallel_wavegan_updater.py:192-223, ``nn.MSELoss``), for the two configurations of
tests/pwg_disc_ref.golden_configs: (a) the recipes' shape on a (2, 1, 300) rectangle, (b) layers 5, 16 channels, kernel 5,
dilation_factor 2, no bias on (1, 1, 97).

Stored per configuration ``<n>``: the seeded weights in weight-norm form under ``<n>/<state-dict key>``, ``<n>_x`` (the batch
scored as generated audio) and ``<n>_y`` (the batch scored as real audio), their logits ``<n>_px`` / ``<n>_py`` and
``<n>_mse`` = [adversarial mse(px, 1), real mse(py, 1), fake mse(px, 0)].  tests/test_pwg_disc_cpu.py compares the fp64
restatement with these vectors, tests/test_pwg_disc_gpu.py the engine.  Needs the reference checkout.

For the full-size case of the GPU tests (one utterance of 163 840 samples, pwg_disc_ref.full_size_input, configuration a) the
archive also holds what the fp64 restatement gives: ``a_full_sums`` = [sum (p - 1)^2, sum p^2] and its derived bounds
``a_full_bound_f32`` / ``a_full_bound_f16x3`` (pwg_disc_ref.forward_long and sums_with_bound at the largest kernel window,
256 terms per fp32 sum), and the reference's own float32 logits reduced the same way, ``a_full_sums_reference``.

The stand-in's ``nn.MSELoss`` is a name without a forward; it is supplied here, on torch, with Paddle's documented semantics
(``reduction="mean"``: the mean of the squared differences)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402

import pwg_disc_ref as ref  # noqa: E402


def _supply():
    import torch

    def forward(self, input, label):   # noqa: A002  (Paddle's argument name)
        return paddle.to_tensor(torch.mean((input.as_subclass(torch.Tensor) - label.as_subclass(torch.Tensor)) ** 2))

    if "forward" not in vars(paddle.nn.MSELoss):
        paddle.nn.MSELoss.forward = forward


def main():
    if not ref_import.REAL:
        _supply()
    pw = ref_import.load("parakeet.models.parallel_wavegan.parallel_wavegan")
    mse = paddle.nn.MSELoss()
    out = {}
    for name, (cfg, seed, shape) in ref.golden_configs().items():
        state, x = ref.golden_inputs(name)
        y = np.random.default_rng(seed + 2000).normal(size=shape).astype(np.float32) * 0.5
        kw = {k: v for k, v in cfg.items() if k != "negative_slope"}
        model = pw.PWGDiscriminator(nonlinear_activation="LeakyReLU",
                                    nonlinear_activation_params={"negative_slope": cfg["negative_slope"]}, **kw)
        assert set(model.state_dict().keys()) == set(state.keys()), sorted(model.state_dict().keys())
        model.set_state_dict(state)
        model.eval()
        with paddle.no_grad():
            px, py = model(paddle.to_tensor(x)), model(paddle.to_tensor(y))
            nums = [float(mse(px, paddle.ones_like(px))), float(mse(py, paddle.ones_like(py))),
                    float(mse(px, paddle.zeros_like(px)))]
        for k, v in state.items():
            out[f"{name}/{k}"] = v
        out[f"{name}_x"], out[f"{name}_y"] = x, y
        out[f"{name}_px"] = np.asarray(px.numpy(), np.float32)
        out[f"{name}_py"] = np.asarray(py.numpy(), np.float32)
        out[f"{name}_mse"] = np.array(nums, np.float64)
        print(name, out[f"{name}_px"].shape, nums, flush=True)
        if name == "a":
            xf = ref.full_size_input()
            r = ref.forward_long(ref.Model(cfg, state), xf)
            for m in ref.MATHS:
                out["a_full_sums"], out[f"a_full_bound_{m}"] = ref.sums_with_bound(r["logits"], r["b_logits"][m], 256)
            with paddle.no_grad():
                pf = model(paddle.to_tensor(xf.reshape(1, 1, -1))).numpy().reshape(-1)
            out["a_full_sums_reference"] = ref.sums(pf)
            q = np.abs(out["a_full_sums_reference"] - out["a_full_sums"]) / out["a_full_bound_f32"]
            print("full size", out["a_full_sums"], out["a_full_bound_f32"], out["a_full_bound_f16x3"], "reference / bound", q)
            assert (q <= 1.0).all()
    path = os.path.join(ref_import.golden_dir(), "pwg_disc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
