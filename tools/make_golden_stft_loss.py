#!/usr/bin/env python
"""tests/golden/stft_loss.npz: the REFERENCE's own parakeet/modules/stft_loss.py run over the torch-backed stand-in of paddle
(tools/ref_import.py) on the small pair of tests/stft_loss_cases.golden_batch: the magnitudes ``stft`` returns for the
predicted signals at every resolution of stft_loss_cases.RESOLUTIONS, ``STFTLoss`` at each of them, and
``MultiResolutionSTFTLoss`` with its defaults.  tests/test_stft_loss_cpu.py compares the fp64 restatement with these vectors,
tests/test_stft_loss_gpu.py the engine.  Needs the reference checkout.

The stand-in lacks four things this module uses; they are supplied here, on torch, with Paddle's documented semantics:
``paddle.signal.stft`` (torch.stft, onesided, (B, n_bin, frames) complex) whose result answers ``.real()`` / ``.imag()`` as
methods, ``paddle.norm(x, p="fro")`` and ``paddle.nn.functional.l1_loss`` (mean reduction).  Reproducible: the inputs are
seeded and nothing else is random."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import ref_import  # noqa: E402
import stft_loss_cases as lc  # noqa: E402


class _Complex:
    def __init__(self, z):
        self.z = z

    def real(self):
        import paddle
        return paddle.to_tensor(self.z.real.contiguous())

    def imag(self):
        import paddle
        return paddle.to_tensor(self.z.imag.contiguous())


def _supply():
    import paddle
    import paddle.nn.functional as F

    def stft(x, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", normalized=False,
             onesided=True, name=None):
        x = x.as_subclass(torch.Tensor)
        w = None if window is None else window.as_subclass(torch.Tensor).to(x.dtype)
        return _Complex(torch.stft(x, n_fft, hop_length=hop_length, win_length=win_length, window=w, center=center,
                                   pad_mode=pad_mode, normalized=normalized, onesided=onesided, return_complex=True))

    def norm(x, p="fro", axis=None, keepdim=False, name=None):
        assert p == "fro" and axis is None
        return paddle.to_tensor(torch.linalg.vector_norm(x.as_subclass(torch.Tensor)))

    def l1_loss(input, label, reduction="mean", name=None):   # noqa: A002  (Paddle's argument name)
        assert reduction == "mean"
        return paddle.to_tensor(torch.mean(torch.abs(input.as_subclass(torch.Tensor) - label.as_subclass(torch.Tensor))))

    if not hasattr(paddle, "signal"):
        paddle.signal = types.SimpleNamespace(stft=stft)
    if not hasattr(paddle, "norm"):
        paddle.norm = norm
    if not hasattr(F, "l1_loss"):
        F.l1_loss = l1_loss


def main():
    ref_import.setup()
    import paddle
    if not ref_import.REAL:
        _supply()
    ref = ref_import.load("parakeet.modules.stft_loss")
    x, y = lc.golden_batch()
    px, py = paddle.to_tensor(x), paddle.to_tensor(y)
    out = {"x": x, "y": y}
    per = []
    for r in lc.RESOLUTIONS:
        out["mag_x_" + lc.res_id(r)] = np.asarray(ref.stft(px, r.n_fft, r.hop, r.win, "hann").numpy(), np.float32)
        sc, mag = ref.STFTLoss(r.n_fft, r.hop, r.win, "hann")(px, py)
        per.append([float(sc), float(mag)])
    out["stft_loss"] = np.array(per, np.float64)
    sc, mag = ref.MultiResolutionSTFTLoss()(px, py)
    out["multi_resolution"] = np.array([float(sc), float(mag)], np.float64)
    x3, y3 = x.reshape(1, 2, -1), y.reshape(1, 2, -1)
    sc, mag = ref.MultiResolutionSTFTLoss()(paddle.to_tensor(x3), paddle.to_tensor(y3))
    out["multi_resolution_bct"] = np.array([float(sc), float(mag)], np.float64)
    path = os.path.join(ref_import.golden_dir(), "stft_loss.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
