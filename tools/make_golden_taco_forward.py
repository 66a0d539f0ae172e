#!/usr/bin/env python
"""Generate tests/golden/tacotron2_forward.npz: Tacotron2 with teacher forcing, computed by the REFERENCE's own
``Tacotron2.forward`` (parakeet/models/tacotron2.py:691-778, decoder :419-472) run in eval mode over the torch-backed
paddle stand-in (oracle/paddle_shim, tools/ref_import.py).  The cases are tests/taco2_forward_cases.py.

The decoder prenet keeps its dropout on (:76-79); the mask is the engine's counter-based stream, injected through the
dropout hook of tools/make_golden_ar.py.  In ``forward`` the prenet sees all T_mel + 1 query rows of the batch in ONE
call per layer (:451), so the hook maps row s of utterance b to decoding step s of stream seed + b.

The frozen stand-in has two gaps on this path, filled here at run time by replacing attributes of the imported objects:
  * ``paddle.fluid.layers.sequence_mask`` raises: the name ``sequence_mask`` of the reference's tacotron2 module is rebound
    to the function below [paddle-semantics, from Paddle's API documentation: mask[i, j] = j < x[i], maxlen = max(x),
    dtype int64 unless given];
  * the stand-in's LSTM refuses ``sequence_length``: the encoder LSTM's forward drops it when every length equals the
    padded length, where it changes nothing (every case here has equal text lengths).

Stored are the recorded inputs and the reference's outputs.  The archive is written with fixed zip timestamps."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402
import torch  # noqa: E402

from oracle import tacotron2_ref as t2_ref  # noqa: E402

sys.path.insert(0, os.path.join(ref_import.ROOT, "tests"))
import taco2_forward_cases as cases  # noqa: E402
from make_golden_fs2_forward import save_npz_reproducible  # noqa: E402


def sequence_mask(x, maxlen=None, dtype="int64", name=None):
    lens = torch.as_tensor(np.asarray(x.numpy() if hasattr(x, "numpy") else x)).to(torch.int64)
    n = int(lens.max()) if maxlen is None else int(maxlen)
    mask = torch.arange(n).unsqueeze(0) < lens.unsqueeze(-1)
    if isinstance(dtype, str):
        dtype = getattr(torch, dtype)
    return paddle.to_tensor(mask.to(dtype).numpy())


def full_length_lstm(lstm):
    """``lstm(inputs=x, sequence_length=lens)`` with every length equal to x.shape[1] is ``lstm(inputs=x)``."""
    inner = lstm.forward

    def forward(inputs, initial_states=None, sequence_length=None):
        if sequence_length is not None:
            lens = np.asarray(sequence_length.numpy()).reshape(-1)
            assert (lens == int(inputs.shape[1])).all(), "only full-length batches: the stand-in's LSTM has no masking"
        return inner(inputs, initial_states)
    lstm.forward = forward


class ForwardDropout:
    """F.dropout hook for Tacotron2.forward: DecoderPreNet is called once on (B, T_mel + 1, d_prenet), its two layers are
    calls 0 and 1; row s is decoding step s."""

    def __init__(self, seeds, units, p):
        self.drops = [t2_ref.stream_dropout(s, units, p) for s in seeds]
        self.p, self.calls = p, 0

    def __call__(self, shape, p):
        assert p == self.p and len(shape) == 3 and shape[0] == len(self.drops) and self.calls < 2
        layer = self.calls
        self.calls += 1
        return np.stack([np.stack([np.asarray(d(s, layer, shape[2])) for s in range(shape[1])]) for d in self.drops])


def run_case(t2m, name, out):
    cfg = cases.case_cfg(name)
    model = t2m.Tacotron2(**cfg)
    model.set_state_dict(cases.case_state(name))
    model.eval()
    full_length_lstm(model.encoder.lstm)
    u = cases.case_inputs(name)
    B, T = u["ids"].shape
    opt = lambda v: None if v is None else paddle.to_tensor(v)     # noqa: E731
    hook = ForwardDropout(u["seeds"], cfg["d_prenet"], cfg["p_prenet_dropout"])
    with ref_import.dropout_hook(hook), paddle.no_grad():
        o = model.forward(paddle.to_tensor(u["ids"]), paddle.to_tensor(np.full(B, T, dtype=np.int64)),
                          paddle.to_tensor(u["mels"]), output_lens=opt(u["output_lens"]), tones=opt(u["tones"]),
                          global_condition=opt(u["global_condition"]))
    assert hook.calls == 2
    for k in ("ids", "tones", "global_condition", "mels", "output_lens"):
        if u[k] is not None:
            out[f"{name}_{k}"] = u[k]
    out[f"{name}_seeds"] = np.array(u["seeds"], dtype=np.int64)
    for k in cases.KEYS:
        if k in o:
            out[f"{name}_{k}"] = o[k].numpy().astype(np.float32)
    print("tacotron2_forward", name, {k: out[f"{name}_{k}"].shape for k in cases.KEYS if f"{name}_{k}" in out})


def main():
    t2m = ref_import.load("parakeet.models.tacotron2")
    t2m.sequence_mask = sequence_mask
    out = {}
    for name in cases.CASES:
        run_case(t2m, name, out)
    out["cases"] = np.array(",".join(cases.CASES))
    path = os.path.join(ref_import.golden_dir(), "tacotron2_forward.npz")
    save_npz_reproducible(path, out)
    print("tacotron2_forward:", list(cases.CASES), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
