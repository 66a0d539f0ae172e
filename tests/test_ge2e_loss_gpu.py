"""GE2E similarity matrix, loss and EER on the device (csrc/spk_loss.hip through pk_spk_ge2e and the Python class) against
the fp64 restatement tests/ge2e_loss_ref.py, under the derived bounds of tests/ge2e_bounds.py (ratio = error / bound <= 1,
printed; DESIGN.md 4.6b lists the first hardware run).  All shapes are tiny; a shape's reference and bounds are computed
once and shared."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ge2e_bounds as gb  # noqa: E402
import ge2e_loss_ref as ref  # noqa: E402
from fp32_bounds import ratio  # noqa: E402

from parakeet_amd import synthetic as syn  # noqa: E402
from parakeet_amd.lstm_speaker_encoder import LSTMSpeakerEncoder, equal_error_rate  # noqa: E402

pytestmark = pytest.mark.gpu

SECOND = dict(n_mels=80, num_layers=2, hidden_size=128, output_size=64)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge2e_loss.npz")
# (N, M, C), unit rows.  (2, 2, 1): the smallest admitted (left un-normalised: unit rows of one dimension are all 1);
# (33, 7, 257): off every wave and tile multiple, rows that end inside a workgroup's tile of 8; (130, 3, 48): more speakers than a wave has lanes; (260, 2, 8): more speakers than a
# workgroup has threads (a lane owns two); (64, 10, 256): the recipe; (64, 40, 64): what forward feeds at the recipe;
# (3, 2, 1024) / (3, 2, 1025): the two sides of the switch from 8 to 4 rows per workgroup; (5, 3, 64) un-normalised too.
SHAPES = [((2, 2, 1), False), ((3, 2, 5), True), ((5, 3, 64), True), ((5, 3, 64), False), ((33, 7, 257), True),
          ((130, 3, 48), True), ((260, 2, 8), True), ((64, 10, 256), True), ((64, 40, 64), False), ((3, 2, 1024), True),
          ((3, 2, 1025), True)]
KEYS = ("p", "p1", "p2", "terms", "loss_f32")


def _id(s):
    return "x".join(str(v) for v in s[0]) + ("" if s[1] else "-raw")


@functools.lru_cache(maxsize=None)
def _model():
    return LSTMSpeakerEncoder(**SECOND).eval()


@functools.lru_cache(maxsize=None)
def _case(shape, unit, w=10.0, b=-5.0, seed=3):
    e = ref.embeddings(*shape, seed=seed, normalise=unit)
    return e, ref.loss(e, w, b), gb.bounds(e, w, b)


def _engine(m, e):
    """Everything the engine computes for embeds e, as numpy."""
    p, p1, p2 = m.similarity_matrix(e)
    terms = m.loss_terms(e)
    loss, eer = m.loss(e)
    assert p.dtype == torch.float32 and terms.dtype == torch.float64 and loss.dtype == torch.float32 and loss.dim() == 0
    assert isinstance(eer, float)
    N, M, _ = np.shape(e)
    assert tuple(p.shape) == (N * M, N) and tuple(p1.shape) == (N * M * N,) and tuple(p2.shape) == (N * M,)
    assert tuple(terms.shape) == (N, M)
    return {"p": p.cpu().numpy(), "p1": p1.cpu().numpy(), "p2": p2.cpu().numpy(), "terms": terms.cpu().numpy().reshape(-1),
            "loss_f32": float(loss.cpu()), "eer": eer}


def _ratios(got, want, bd):
    return {k: ratio(got[k], want["loss" if k == "loss_f32" else k], bd[k]) for k in KEYS}


def _show(tag, rs):
    print(f"GE2E {tag}: " + ", ".join(f"{k} {v:.4f}" for k, v in rs.items()))


@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_error_bounds(case):
    e, want, bd = _case(*case)
    got = _engine(_model(), e)
    rs = _ratios(got, want, bd)
    _show(_id(case), rs)
    assert max(rs.values()) <= 1.0, rs
    # the EER is that of the engine's OWN matrix (a score pair closer than the rounding error may swap against fp64)
    N, M, _ = e.shape
    assert got["eer"] == equal_error_rate(ref.labels(N, M), got["p"])


@pytest.mark.parametrize("case", [((3, 2, 5), True), ((33, 7, 257), True), ((130, 3, 48), True), ((260, 2, 8), True),
                                  ((3, 2, 1025), True)], ids=_id)
def test_speaker_permutation_is_bit_exact(case):
    e, _, _ = _case(*case)
    N, M, _ = e.shape
    perm = np.random.default_rng(11).permutation(N)
    assert (perm != np.arange(N)).any()
    m = _model()
    a = _engine(m, e)
    b = _engine(m, np.ascontiguousarray(e[perm]))
    rows = (perm[:, None] * M + np.arange(M)[None, :]).reshape(-1)        # row (n', m) of the permuted batch = (perm[n'], m)
    assert np.array_equal(b["p"], a["p"][rows][:, perm])
    assert np.array_equal(b["p1"].reshape(N * M, N), a["p1"].reshape(N * M, N)[rows][:, perm])
    assert np.array_equal(b["p2"], a["p2"][rows])


def test_two_identical_calls_agree_bit_for_bit():
    e, _, _ = _case((33, 7, 257), True)
    a, b = _engine(_model(), e), _engine(_model(), e)
    for k in ("p", "p1", "p2", "terms"):
        assert np.array_equal(a[k], b[k]), k
    assert a["loss_f32"] == b["loss_f32"] and a["eer"] == b["eer"]


def test_loss_is_the_mean_of_the_terms():
    e, _, _ = _case((33, 7, 257), True)
    got = _engine(_model(), e)
    mean = float(got["terms"].mean())
    assert abs(got["loss_f32"] - mean) <= 2.0 ** -23 * abs(mean)    # one rounding to float32, with a spare


def test_similarity_parameters_are_kept():
    e, want_default, _ = _case((5, 3, 64), True)
    m = LSTMSpeakerEncoder(**SECOND).eval()
    m.set_state_dict({"similarity_weight": np.array([7.5], np.float32), "similarity_bias": np.array([-2.0], np.float32)})
    _, want, bd = _case((5, 3, 64), True, 7.5, -2.0)
    got = _engine(m, e)
    rs = _ratios(got, want, bd)
    _show("5x3x64 w=7.5 b=-2", rs)
    assert max(rs.values()) <= 1.0, rs
    assert ratio(got["p"], want_default["p"], bd["p"]) > 1.0      # and it is not the default's matrix
    # p1 and p2 do not see the parameters
    base = _engine(_model(), e)
    assert np.array_equal(got["p1"], base["p1"]) and np.array_equal(got["p2"], base["p2"])
    with pytest.raises((ValueError, AssertionError)):
        m.set_state_dict({"similarity_weight": np.array([1.0, 2.0], np.float32)})


def test_forward_and_evaluate_batch():
    """forward keeps the reference's reshape([N, -1, N]); evaluate_batch is the (N, M, output_size) reading."""
    g = np.load(GOLD)      # the golden's model and 8 partials of 12 frames: no slice centroid vanishes there
    m = LSTMSpeakerEncoder(**SECOND)
    m.set_state_dict(syn.ge2e_state(SECOND, seed=int(g["fwd_seed"])))
    m.eval()
    x, N = g["fwd_x"], int(g["fwd_num_speakers"])
    M = x.shape[0] // N
    emb = m.embed_sequences(x)
    assert np.abs(emb.cpu().numpy() - g["fwd_seqs"]).max() < 1e-4
    for name, shape, call in (("forward", (N, -1, N), lambda: m.forward(x, N)),
                              ("call", (N, -1, N), lambda: m(x, N)),
                              ("evaluate_batch", (N, M, SECOND["output_size"]),
                               lambda: tuple(m.evaluate_batch(x, N)[k] for k in ("loss", "eer")))):
        loss, eer = call()
        e = emb.reshape(*shape)
        want_loss, want_eer = m.loss(e)
        assert torch.equal(loss, want_loss) and eer == want_eer, name
        e_np = e.cpu().numpy()
        r, bd = ref.loss(e_np, 10.0, -5.0), gb.bounds(e_np, 10.0, -5.0)
        rt = ratio(float(loss.cpu()), r["loss"], bd["loss_f32"])
        print(f"GE2E {name} {e_np.shape}: loss {float(loss.cpu()):.6f} err {eer:.6f}, loss ratio {rt:.4f}")
        assert rt <= 1.0
    assert m.loss(emb.reshape(N, -1, N))[0] != m.loss(emb.reshape(N, M, -1))[0]


@pytest.mark.parametrize("name", ["a", "b", "wb", "fwd"])
def test_reference_goldens_through_the_engine(name):
    g = np.load(GOLD)
    e = g[f"{name}_embeds"]
    w, b = (float(v) for v in g[f"{name}_wb"])
    m = LSTMSpeakerEncoder(**SECOND).eval()
    m.set_state_dict({"similarity_weight": np.array([w], np.float32), "similarity_bias": np.array([b], np.float32)})
    got = _engine(m, e)
    bd = gb.bounds(e, w, b)
    want = {"p": g[f"{name}_p"], "p1": g[f"{name}_p1"], "p2": g[f"{name}_p2"], "loss": float(g[f"{name}_loss"])}
    rs = {k: ratio(got[k], want["loss" if k == "loss_f32" else k], bd[k]) for k in ("p", "p1", "p2", "loss_f32")}
    _show(f"golden {name}", rs)
    assert max(rs.values()) <= 1.0, rs


def test_speaker_similarity():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((37, 257)).astype(np.float32)
    b = (a * 0.5 + rng.standard_normal((37, 257)) * np.exp(rng.normal(0, 1, size=(37, 1)))).astype(np.float32)
    got = _model().speaker_similarity(a, b)
    assert tuple(got.shape) == (37,) and got.is_cuda
    r = ratio(got.cpu().numpy(), ref.cosine(a, b), gb.cosine_bound(a, b))
    print(f"speaker_similarity: ratio {r:.4f}")
    assert r <= 1.0
    same = _model().speaker_similarity(a, a).cpu().numpy()
    assert np.abs(same - 1.0).max() <= gb.cosine_bound(a, a).max()
    with pytest.raises(ValueError):
        _model().speaker_similarity(a, b[:5])


def test_inv_argmax():
    row = _model().inv_argmax(2, 5)
    assert row.tolist() == [0, 0, 1, 0, 0] and row.dtype.kind == "i"


def test_errors():
    m = _model()
    with pytest.raises(ValueError):
        m.loss(np.ones((3, 1, 8), np.float32))              # M = 1: the exclusive centroid divides by zero
    with pytest.raises(ValueError):
        m.similarity_matrix(np.ones((1, 4, 8), np.float32))  # N = 1
    with pytest.raises(ValueError):
        m.loss_terms(np.ones((6, 8), np.float32))           # 2-d
    with pytest.raises(ValueError):
        m.similarity_matrix(np.ones((4097, 2, 1), np.float32))   # beyond the envelope: refused, never truncated
    # the C ABI refuses the same shapes itself
    lib, e = m._ctx.lib, torch.ones((3, 1, 8), device="cuda")
    assert lib.pk_spk_ge2e(m._h, C.c_void_p(e.data_ptr()), 3, 1, 8, None, None, None, None, None) == -2
    assert b"M - 1" in lib.pk_last_error()
    assert lib.pk_spk_ge2e(m._h, C.c_void_p(e.data_ptr()), 4097, 2, 1, None, None, None, None, None) == -3
    # forward: 3 partials x 64 dimensions do not reshape to (4, -1, 4)
    mm = LSTMSpeakerEncoder(**SECOND)
    mm.set_state_dict(syn.ge2e_state(SECOND, seed=12))
    x = np.full((3, 4, SECOND["n_mels"]), 0.1, np.float32)
    with pytest.raises(ValueError):
        mm.eval().forward(x, 5)
    with pytest.raises(ValueError):
        mm.evaluate_batch(x, 2)


def test_example_ge2e_verify(tmp_path, monkeypatch, capsys):
    """examples/ge2e_verify.py on a small corpus of mel files: the trainer's line per batch and the means, seeded (two runs
    print the same), and --literal goes through forward's reshape (other numbers)."""
    import importlib.util
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(root, "tools", "make_paddle_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    st = syn.ge2e_state(syn.GE2E_RELEASED, seed=27)
    mk.paddle_save({k: mk.VarBase(f"param_{i}", v) for i, (k, v) in enumerate(st.items())}, str(tmp_path / "step-7.pdparams"))
    rng = np.random.default_rng(3)
    for s in range(4):
        (tmp_path / "corpus" / f"spk{s}").mkdir(parents=True)
        for u in range(3):
            mel = np.exp(rng.normal(-2.0 + 0.5 * s, 2.0, size=(170 + 10 * u, 40))).astype(np.float32)
            np.save(tmp_path / "corpus" / f"spk{s}" / f"utt{u}.npy", mel)
        np.save(tmp_path / "corpus" / f"spk{s}" / "short.npy", np.ones((20, 40), np.float32))   # below a clip: left out
    spec = importlib.util.spec_from_file_location("ge2e_verify", os.path.join(root, "examples", "ge2e_verify.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)

    def run(*extra):
        monkeypatch.setattr(sys, "argv", ["ge2e_verify.py", "--input", str(tmp_path / "corpus"), "--checkpoint_path",
                                          str(tmp_path / "step-7"), "--speakers_per_batch", "4", "--utterances_per_speaker", "2",
                                          "--batches", "2", "--seed", "5", *extra])
        ex.main()
        return capsys.readouterr().out

    a, b, lit = run(), run(), run("--literal")
    assert a == b and a != lit
    assert "4 speakers, 12 utterances" in a
    rows = re.findall(r"^step: (\d+), loss: (\d+\.\d{6}) err: (\d\.\d{6})$", a, flags=re.M)
    assert [r[0] for r in rows] == ["0", "1"]
    mean = re.search(r"^mean loss: (\d+\.\d{6}) err: (\d\.\d{6})$", a, flags=re.M)
    assert mean and abs(float(mean.group(1)) - np.mean([float(r[1]) for r in rows])) < 2e-6
    assert all(0.0 <= float(r[2]) <= 1.0 for r in rows)
