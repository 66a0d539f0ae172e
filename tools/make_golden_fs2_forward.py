#!/usr/bin/env python
"""Generate tests/golden/fs2_forward.npz: FastSpeech2 with GIVEN durations, pitch and energy, computed by the REFERENCE's
own FastSpeech2 source (parakeet/models/fastspeech2/fastspeech2.py) run over the torch-backed paddle stand-in
(oracle/paddle_shim, tools/ref_import.py).  The cases are tests/fs2_forward_cases.py: ``_forward(..., is_inference=False)``
and ``forward`` per utterance (T = 1, 7, 40; add / concat speaker; reduction_factor 2; post-norm; "linear" FFN; zero
durations inside an utterance), one equal-length batch of 3 through ``forward``, and one T = 1 case through the reference's
own ``inference(use_teacher_forcing=True)`` -- its ``if durations:`` (:516) takes the truth value of the duration tensor,
which exists for one element only; if the stand-in refuses even that, the case is dropped and the tool says so.

Weights and targets come from seeds; stored are the targets and the reference's outputs.  The archive is written with
fixed zip timestamps: running the tool twice gives identical bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402

sys.path.insert(0, os.path.join(ref_import.ROOT, "tests"))
import fs2_forward_cases as cases  # noqa: E402


def save_npz_reproducible(path, arrays):
    """np.savez_compressed stamps every member with the current time; this writes the same archive with a fixed one."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def run_case(fsm, name, out):
    _, how, toks, spk = cases.CASES[name]
    cfg = cases.model_kwargs(name)
    model = fsm.FastSpeech2(idim=80, odim=80, **cfg)
    model.set_state_dict(cases.case_state(name))
    model.eval()
    utts = cases.case_inputs(name)
    B, T = len(utts), toks[0]
    xs = paddle.to_tensor(np.stack([u["ids"] for u in utts]))
    ilens = paddle.to_tensor(np.array([T] * B, dtype=np.int64))
    ds = paddle.to_tensor(np.stack([u["ds"] for u in utts]))
    ps = paddle.to_tensor(np.stack([u["ps"] for u in utts])[:, :, None])
    es = paddle.to_tensor(np.stack([u["es"] for u in utts])[:, :, None])
    olens = paddle.to_tensor(np.array([u["olen"] for u in utts], dtype=np.int64))
    kw = {}
    if spk == "spk_id":
        kw["spk_id"] = paddle.to_tensor(np.array([u["spk_id"] for u in utts], dtype=np.int64))
    elif spk == "spembs":
        kw["spembs"] = paddle.to_tensor(np.stack([u["spembs"] for u in utts]))
    with paddle.no_grad():
        if how == "_forward":
            before, after, d, p, e = model._forward(xs, ilens, olens, ds, ps, es, is_inference=False, **kw)
        elif how == "forward":
            ys = paddle.to_tensor(np.zeros((B, int(max(u["olen"] for u in utts)), 80), np.float32))
            before, after, d, p, e, ys_out, olens_out = model.forward(xs, ilens, ys, olens, ds, ps, es, **kw)
            out[f"{name}_olens_out"] = np.asarray(olens_out.numpy()).astype(np.int64).reshape(-1)
            out[f"{name}_ys_len"] = np.array(ys_out.shape[1], dtype=np.int64)
        else:
            after = model.inference(xs[0], durations=ds[0], pitch=ps[0], energy=es[0], use_teacher_forcing=True)
            after = after.unsqueeze(0)
            before = d = p = e = None
    for b, u in enumerate(utts):
        for k in ("ids", "ds", "ps", "es"):
            out[f"{name}_{k}{b}"] = u[k]
        out[f"{name}_olen{b}"] = np.array(u["olen"], dtype=np.int64)
        if "spk_id" in u:
            out[f"{name}_spk_id{b}"] = np.array(u["spk_id"], dtype=np.int64)
        if "spembs" in u:
            out[f"{name}_spembs{b}"] = u["spembs"]
        out[f"{name}_after{b}"] = after.numpy()[b].astype(np.float32)
        if before is not None:
            out[f"{name}_before{b}"] = before.numpy()[b].astype(np.float32)
            out[f"{name}_d_outs{b}"] = d.numpy()[b].astype(np.float32)
            out[f"{name}_p_outs{b}"] = p.numpy()[b, :, 0].astype(np.float32)
            out[f"{name}_e_outs{b}"] = e.numpy()[b, :, 0].astype(np.float32)


def main():
    fsm = ref_import.load("parakeet.models.fastspeech2.fastspeech2")
    out = {"seed": np.array(cases.SEED, dtype=np.int64)}
    done = []
    for name, (_, how, _, _) in cases.CASES.items():
        try:
            run_case(fsm, name, out)
            done.append(name)
        except Exception as exc:       # only the reference's own wrapper may be refused (tensor truth value)
            if how != "inference":
                raise
            print(f"{name}: dropped, the reference's inference(use_teacher_forcing=True) did not run: {exc!r}")
    out["cases"] = np.array(",".join(done))
    path = os.path.join(ref_import.golden_dir(), "fs2_forward.npz")
    save_npz_reproducible(path, out)
    print("fs2_forward:", done, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
