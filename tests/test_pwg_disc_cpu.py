"""The Parallel WaveGAN discriminator without a device: the fp64 restatement (tests/pwg_disc_ref.py) against the reference's
own numbers (tests/golden/pwg_disc.npz) under its derived fp32 bound, the mutants that bound must reject, the Python class's
refusals and dilation schedule, checkpoint loading, and the evaluator's dictionary."""
import functools
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import pwg_disc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MAX_TILE = 256      # no kernel window is larger: the most terms one fp32 sum of the loss may hold


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "pwg_disc.npz")))


@functools.lru_cache(maxsize=None)
def _model(name):
    cfg = ref.golden_configs()[name][0]
    state = {k[len(name) + 1:]: v for k, v in _gold().items() if k.startswith(name + "/")}
    return cfg, state, ref.Model(cfg, state)


def _mkfix():
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(ROOT, "tools", "make_paddle_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_equals_the_golden_inside_the_fp32_bound(name):
    g, (cfg, state, model) = _gold(), _model(name)
    assert all(k.endswith(("weight_g", "weight_v", "bias")) for k in state)          # stored in weight-norm form
    assert g[f"{name}_x"].shape == ref.golden_configs()[name][2]
    nums, bnum, n = {}, {}, 0
    for tag in ("x", "y"):
        x, want = g[f"{name}_{tag}"], g[f"{name}_p{tag}"]
        rs = [ref.forward(model, x[i, 0], maths=("f32",), keep=False) for i in range(x.shape[0])]
        q = max(fb.ratio(want[i, 0], r["logits"], r["b_logits"]["f32"]) for i, r in enumerate(rs))
        print(f"SWEEP-RATIO pwg_disc restatement {name} golden logits {tag} {q:.4f}")
        assert q <= 1.0
        sb = [ref.sums_with_bound(r["logits"], r["b_logits"]["f32"], x.shape[2]) for r in rs]   # one mean over the rectangle
        n = x.size
        nums[tag], bnum[tag] = sum(s for s, _ in sb) / n, sum(b for _, b in sb) / n
    got = np.array([nums["x"][0], nums["y"][0], nums["x"][1]])
    # torch's mean of N x T float32 terms: pairwise or not, (N T + 8) u relative covers any order (as the sums' gamma)
    bound = (np.array([bnum["x"][0], bnum["y"][0], bnum["x"][1]]) + (n + 8) * fb.U * got)
    assert fb.ratio(g[f"{name}_mse"], got, bound) <= 1.0
    # the logits vary by much more than the bound: the comparison can tell a model that ignores its input from the right one
    assert g[f"{name}_px"].std() > 10 * max(r["b_logits"]["f32"].max() for r in rs)


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("math", ref.MATHS)
def test_every_mutant_falls_outside_the_bound(name, math):
    g, (cfg, _, model) = _gold(), _model(name)
    x = g[f"{name}_x"][0, 0]
    r = ref.forward(model, x, maths=(math,), keep=False)
    s, bs = ref.sums_with_bound(r["logits"], r["b_logits"][math], MAX_TILE)
    tile = MAX_TILE - 2 * model.halo
    mut = ref.mutants(model, x, tile=tile)
    # without biases LeakyReLU(0) = 0 and zero-extending the signal IS the right answer: "nozero" exists for (a) only
    assert set(mut) == ({"nozero", "dil", "lastact", "twice"} if cfg["bias"] else {"dil", "lastact", "twice"})
    for key, (p, ms) in mut.items():
        q = fb.ratio(ms, s, bs) if key == "twice" else fb.ratio(p, r["logits"], r["b_logits"][math])
        print(f"SWEEP-RATIO pwg_disc mutant {name} {math} {key} {q:.1f}")
        assert q > 1.0, key


def test_the_piecewise_restatement_of_a_long_utterance_is_the_whole_one():
    """pwg_disc_ref.forward_long, which made the golden's sums of the full-size utterance: the logits of ``forward``, and bounds
    that are never larger (the f16x3 scale comes from a piece's maximum instead of the utterance's)."""
    model = _model("a")[2]
    x = ref.full_size_input(2500)
    whole, long = ref.forward(model, x, keep=False), ref.forward_long(model, x, chunk=512)
    assert np.allclose(whole["logits"], long["logits"], rtol=0, atol=1e-13)
    for m in ref.MATHS:
        assert (long["b_logits"][m] <= whole["b_logits"][m] * (1 + 1e-9)).all() and (long["b_logits"][m] > 0).all()
    assert np.allclose(long["b_logits"]["f32"], whole["b_logits"]["f32"], rtol=1e-9, atol=0)
    g = _gold()
    assert g["a_full_sums"].shape == (2,) and g["a_full_bound_f32"].shape == g["a_full_bound_f16x3"].shape == (2,)
    assert (g["a_full_bound_f32"] < g["a_full_bound_f16x3"]).all() and (g["a_full_bound_f16x3"] < g["a_full_sums"]).all()


def test_constructor_refusals_and_defaults():
    from parakeet_amd.parallel_wavegan import PWGDiscriminator, ResidualPWGDiscriminator
    d = PWGDiscriminator()                                   # no device needed to build one
    assert (d.in_channels, d.out_channels, d.kernel_size, d.layers, d.conv_channels, d.dilation_factor, d.negative_slope,
            d.bias) == (1, 1, 3, 10, 64, 1, 0.2, True)
    for kw, word in ((dict(nonlinear_activation="ReLU"), "LeakyReLU"), (dict(layers=1), "layers"), (dict(layers=2), "590"),
                     (dict(in_channels=2), "in_channels"), (dict(out_channels=3), "out_channels"),
                     (dict(nonlinear_activation_params={"negative_slope": 0.1, "alpha": 1}), "alpha")):
        with pytest.raises(NotImplementedError, match=word):
            PWGDiscriminator(**kw)
    with pytest.raises(AssertionError):
        PWGDiscriminator(kernel_size=4)
    with pytest.raises(AssertionError):
        PWGDiscriminator(dilation_factor=0)
    with pytest.raises(NotImplementedError, match="DESIGN.md"):
        ResidualPWGDiscriminator()
    assert d.eval() is d and d.training is False and d.remove_weight_norm() is None
    with pytest.raises(NotImplementedError):
        d.set_math("bf16x3")


def test_dilation_schedule():
    from parakeet_amd.parallel_wavegan import PWGDiscriminator
    assert PWGDiscriminator().dilations == [1, 1, 2, 3, 4, 5, 6, 7, 8, 1]
    assert PWGDiscriminator(layers=6, dilation_factor=2).dilations == [1, 2, 4, 8, 16, 1]
    assert PWGDiscriminator(layers=5, dilation_factor=3).dilations == [1, 3, 9, 27, 1]
    for f in (1, 2, 3):
        assert PWGDiscriminator(layers=5, dilation_factor=f).dilations[:-1] == ref.dilations(5, f)
    # the recipes' receptive field: (k - 1) / 2 * (sum d_i + 1) = 38 samples per side
    assert ref.halo(dict(kernel_size=3, layers=10, dilation_factor=1)) == 38 == _model("a")[2].halo


@pytest.mark.parametrize("weight_norm", [True, False])
def test_load_pwg_discriminator_from_an_updater_archive(tmp_path, weight_norm):
    """A snapshot as StandardUpdater writes it (generator_params beside discriminator_params), through the writer of
    tools/make_paddle_fixture.py, in weight-norm and in folded form."""
    from parakeet_amd import checkpoint
    from parakeet_amd import synthetic as syn
    mk = _mkfix()
    cfg = dict(kernel_size=5, layers=4, conv_channels=16, dilation_factor=2, bias=True,
               nonlinear_activation_params={"negative_slope": 0.1})
    st = syn.pwg_disc_state(cfg, seed=9, weight_norm=weight_norm)
    wrap = lambda s, tag: {k: mk.VarBase(f"{tag}_{i}", v) for i, (k, v) in enumerate(s.items())}   # noqa: E731
    path = str(tmp_path / "snapshot_iter_7.pdz")
    mk.paddle_save({"epoch": 1, "iteration": 7, "generator_params": wrap({"first_conv.weight": np.ones((2, 1, 1), np.float32)}, "g"),
                    "discriminator_params": wrap(st, "d")}, path)
    model = checkpoint.load_pwg_discriminator({"generator_params": {}, "discriminator_params": cfg}, path)
    assert model.training is False and model.negative_slope == 0.1 and model.dilations == [1, 2, 4, 1]
    back = model.state_dict()
    assert set(back) == set(st) and all(np.array_equal(back[k], st[k]) for k in st)
    assert any(k.endswith("weight_g") for k in back) == weight_norm
    # the restatement folds what was loaded: a (16, 16, 5) weight per hidden block in either form
    assert ref.Model(dict(cfg, negative_slope=0.1), back).w[1].shape == (16, 16, 5)
    with open(tmp_path / "generator_only.pdz", "wb") as f:
        pickle.dump({"generator_params": {}, "discriminator_params": {}}, f, protocol=2)
    with pytest.raises(ValueError, match="empty"):
        checkpoint.load_pwg_discriminator({"discriminator_params": cfg}, str(tmp_path / "generator_only.pdz"))
    with pytest.raises(KeyError):
        checkpoint.load_pwg_discriminator({"generator_params": {}}, path)


class _StubDiscriminator:
    """PWGDiscriminator.scores by the restatement"""

    def __init__(self, model):
        self.model = model

    def scores(self, wavs):
        ps = [ref.forward(self.model, np.asarray(w, np.float64), maths=(), keep=False)["logits"] for w in wavs]
        return np.stack([ref.sums(p) for p in ps]), np.array([len(p) for p in ps], np.int64)


class _StubCriterion:
    def __call__(self, x, y):
        d = (np.asarray(x, np.float64) - np.asarray(y, np.float64))
        return torch.tensor(np.abs(d).mean(), dtype=torch.float32), torch.tensor((d ** 2).mean(), dtype=torch.float32)

    def per_utterance(self, xs, ys):
        return np.array([[[float(v) for v in self(x, y)]] * 3 for x, y in zip(xs, ys)])


def test_pwg_evaluate_forms_the_seven_numbers_as_the_evaluator_does():
    from parakeet_amd.losses import pwg_evaluate, pwg_evaluate_per_utterance
    g, (_, _, model) = _gold(), _model("b")
    wav, noise = g["b_y"], g["b_x"]
    wav = np.concatenate([wav, 0.5 * wav[:, :, ::-1]], 0)                 # (2, 1, 97)
    noise = np.concatenate([noise, -noise], 0)
    mel = np.zeros((2, 4, 3), np.float32)
    generator = lambda z, c: torch.from_numpy(np.tanh(z + c.mean()))      # noqa: E731  stands for PWGGenerator.forward
    lam = 2.5
    got = pwg_evaluate(generator, _StubDiscriminator(model), _StubCriterion(), wav, mel, noise, lam)
    fake = np.tanh(noise)
    logits = lambda rows: np.concatenate([ref.forward(model, r, maths=(), keep=False)["logits"] for r in rows[:, 0]])   # noqa: E731
    sc, mag = _StubCriterion()(fake, wav)
    want = ref.evaluate(logits(fake), logits(wav), float(sc), float(mag), lam)
    assert list(got) == ["eval/adversarial_loss", "eval/spectral_convergence_loss", "eval/log_stft_magnitude_loss",
                         "eval/generator_loss", "eval/real_loss", "eval/fake_loss", "eval/discriminator_loss"]
    for k in want:
        assert isinstance(got[k], float) and got[k] == pytest.approx(want[k], rel=1e-12), k
    assert got["eval/generator_loss"] == pytest.approx(lam * got["eval/adversarial_loss"] + float(sc) + float(mag), rel=1e-12)
    per = pwg_evaluate_per_utterance(_StubDiscriminator(model), _StubCriterion(), [fake[0, 0], fake[1, 0, :50]],
                                     [wav[0, 0], wav[1, 0, :50]], lam)
    one = ref.evaluate(logits(fake[:1]), logits(wav[:1]), *[float(v) for v in _StubCriterion()(fake[0, 0], wav[0, 0])], lam)
    for k in one:
        assert per[k].shape == (2,) and per[k][0] == pytest.approx(one[k], rel=1e-12), k
