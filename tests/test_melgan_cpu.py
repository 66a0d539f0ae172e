"""MelGAN / multi-band MelGAN generator without a device: the fp64 restatement (tests/melgan_ref.py) against an independent
torch chain, the min-frames arithmetic, the constructor's refusals, the checkpoint loader, and the proof that the derived
bound can tell wrong evaluations -- a zero-padded boundary among them -- from right ones."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import hifigan_ref as hr  # noqa: E402
import melgan_ref as mr  # noqa: E402

from parakeet_amd import synthetic as syn  # noqa: E402
from parakeet_amd.melgan import PQMF, MelGANGenerator, MelGANInference  # noqa: E402

_CACHE = {}


def model_of(name, weight_norm=False):
    key = (name, weight_norm)
    if key not in _CACHE:
        cfg = mr.CONFIGS[name]
        state = syn.melgan_state(cfg, seed=mr.SEEDS[name], weight_norm=weight_norm)
        _CACHE[key] = (state, mr.Model(cfg, state))
    return _CACHE[key]


@pytest.mark.parametrize("name", list(mr.SMALL))
def test_restatement_equals_torch_chain(name):
    """pad(mode="reflect") / conv1d / conv_transpose1d / leaky_relu in float64 state the same function, from the shortest
    admissible utterance (pad = length - 1 at the input convolution) on; lengths are exactly T' hop."""
    state, model = model_of(name)
    mf = mr.min_frames(mr.CONFIGS[name])
    mels = mr.make_mels(name, (mf, mf + 1, 7 + mf))
    chain = mr.torch_chain(mr.CONFIGS[name], state, mels)
    for mel, (stages, out) in zip(mels, chain):
        r = mr.forward(model, mel, maths=())
        assert r["out"].shape == (mr.CONFIGS[name]["out_channels"], len(mel) * model.hop) == out.shape
        for a, b in zip(r["stages"], stages):
            assert a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-11 * max(1.0, np.abs(b).max()))
        np.testing.assert_allclose(r["out"], out, rtol=0, atol=1e-11 * max(1.0, np.abs(out).max()))
        if model.tanh:
            assert np.abs(r["out"]).max() < 0.95


def test_full_width_restatement_equals_torch_chain():
    for name in ("FULL", "MB-FULL"):
        cfg = mr.CONFIGS[name]
        state = syn.melgan_state(cfg, seed=mr.SEEDS[name])
        mel = mr.make_mels(name, (4,))[0]
        want = mr.torch_chain(cfg, state, [mel])[0][1]
        got = mr.forward(mr.Model(cfg, state), mel, maths=())["out"]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-11)


def test_min_frames_arithmetic():
    """The smallest frame count with every reflection pad below the length it pads: the restatement, the constructor and a
    brute-force search over numpy's own reflect rule agree; one frame fewer makes numpy refuse the pad."""
    assert MelGANGenerator().min_frames == 4 == mr.min_frames(syn.MELGAN)
    assert mr.min_frames(syn.MB_MELGAN) == 4                       # stage 0 (x 8): pad 27 needs 28 positions, 4 frames
    cases = dict(mr.CONFIGS)
    cases["DEEP"] = dict(mr.CONFIGS["TINY"], upsample_scales=(2, 2), stacks=4, kernel_size=3)   # pad 27 at rate 2: 14 frames
    cases["K11"] = dict(mr.CONFIGS["TINY"], kernel_size=11)
    for name, cfg in cases.items():
        g = MelGANGenerator(**mr.ctor_kwargs(cfg))
        pads = []                                                    # (pad, rate) of every reflecting convolution
        k, sk, S = cfg["kernel_size"], cfg["stack_kernel_size"], cfg["stacks"]
        pads.append(((k - 1) // 2, 1))
        mul = 1
        for s in cfg["upsample_scales"]:
            mul *= s
            pads += [((sk - 1) // 2 * sk ** j, mul) for j in range(S)]
        pads.append(((k - 1) // 2, mul))
        brute = next(f for f in range(1, 200) if all(p < f * r for p, r in pads))
        assert g.min_frames == mr.min_frames(cfg) == brute, name
    assert MelGANGenerator(**mr.ctor_kwargs(cases["DEEP"])).min_frames == 14
    state, model = model_of("TINY")
    mf = mr.min_frames(mr.CONFIGS["TINY"])
    with pytest.raises((AssertionError, ValueError)):
        mr.forward(model, mr.make_mels("TINY", (mf - 1,))[0], maths=())


def test_weight_norm_folding():
    cfg = mr.CONFIGS["TINY"]
    state = syn.melgan_state(cfg, seed=5, weight_norm=True)
    assert "melgan.3.weight_g" in state and "melgan.3.weight" not in state and state["melgan.3.weight_v"].shape == (32, 16, 4)
    plain = {}
    for k_, v_ in state.items():
        if k_.endswith(".weight_g"):
            plain[k_[:-9] + ".weight"] = hr.folded(state, k_[:-9])
        elif not k_.endswith(".weight_v"):
            plain[k_] = v_
    mel = mr.make_mels("TINY", (5,))[0]
    a = mr.forward(mr.Model(cfg, state), mel, maths=())["out"]
    b = mr.forward(mr.Model(cfg, plain), mel, maths=())["out"]
    np.testing.assert_array_equal(a, b)


def test_parameter_names():
    """The layout of the docstring for the defaults: 4 stages of 3 stacks -> melgan.1 ... melgan.24."""
    st = syn.melgan_state()
    bases = sorted({k.rsplit(".", 1)[0] for k in st}, key=lambda s: (int(s.split(".")[1]), s))
    assert bases[0] == "melgan.1" and bases[-1] == "melgan.24"
    assert "melgan.3" in bases and "melgan.4.stack.2" in bases and "melgan.6.skip_layer" in bases and "melgan.8" in bases
    assert st["melgan.3.weight"].shape == (512, 256, 16) and st["melgan.24.weight"].shape == (1, 32, 7)
    assert len(bases) == 2 + 4 * (1 + 3 * 3)


REFUSED = [
    dict(use_causal_conv=True), dict(pad="ConstantPad1d"), dict(pad_params={"value": 0.0}), dict(nonlinear_activation="ReLU"),
    dict(nonlinear_activation_params={"negative_slope": 0.2, "x": 1}), dict(bias=False), dict(in_channels=0),
    dict(in_channels=513), dict(out_channels=0), dict(out_channels=17), dict(kernel_size=4), dict(kernel_size=13),
    dict(kernel_size=1), dict(upsample_scales=()), dict(upsample_scales=(2,) * 7, channels=512),
    dict(upsample_scales=(8, 8, 2, 1)), dict(upsample_scales=(17, 2)), dict(channels=64), dict(channels=1024),
    dict(channels=520), dict(channels=4), dict(stacks=0), dict(stacks=7), dict(stack_kernel_size=4), dict(stack_kernel_size=9),
    dict(stack_kernel_size=1), dict(stacks=5), dict(stack_kernel_size=5, stacks=4), dict(stack_kernel_size=7, stacks=3),
]


@pytest.mark.parametrize("kw", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals_need_no_device(kw):
    with pytest.raises(NotImplementedError):
        MelGANGenerator(**kw)


PQMF_REFUSED = [dict(subbands=1), dict(subbands=17), dict(taps=63), dict(taps=2), dict(taps=256), dict(cutoff_ratio=0.0),
                dict(cutoff_ratio=0.5), dict(beta=-1.0), dict(beta=float("nan"))]


@pytest.mark.parametrize("kw", PQMF_REFUSED, ids=[str(i) for i in range(len(PQMF_REFUSED))])
def test_pqmf_refusals_need_no_device(kw):
    with pytest.raises(NotImplementedError):
        PQMF(**kw)


def test_envelope_accepts_the_configurations():
    for name, cfg in mr.CONFIGS.items():
        g = MelGANGenerator(**mr.ctor_kwargs(cfg))
        assert g.upsample_factor == int(np.prod(cfg["upsample_scales"])) and g._h is None
    g = MelGANGenerator()
    assert g.upsample_factor == 256 and g.negative_slope == pytest.approx(0.2) and g.stacks == 3
    MelGANGenerator(stack_kernel_size=5, stacks=3)       # 2 * 25 = 50 <= 64
    MelGANGenerator(stack_kernel_size=3, stacks=4)       # 27
    with pytest.raises(ValueError):
        g.infer_packed(None, [4], noise=np.zeros(256))
    with pytest.raises(NotImplementedError):
        g.set_math("bf16x3")
    mb = MelGANGenerator(**syn.MB_MELGAN)
    assert mb.upsample_factor == 64
    voc = MelGANInference(None, mb, PQMF())
    assert mb.upsample_factor == 256 and voc.generator is mb and voc.pwg_generator is mb and mb._h is None
    with pytest.raises(ValueError):
        g.set_pqmf(PQMF())                               # 4 bands on a 1-channel generator


def test_load_melgan_round_trip(tmp_path):
    """yaml generator_params (+ pqmf_params) + the updaters' nested archive + stats.npy -> MelGANInference holding the same
    tensors, with and without weight norm; pqmf.* keys of the archive are ignored."""
    import yaml
    from parakeet_amd import checkpoint as ck
    for wn, name in ((True, "MB-TINY"), (False, "TINY")):
        cfg = mr.CONFIGS[name]
        state = syn.melgan_state(cfg, seed=3, weight_norm=wn)
        kw = mr.ctor_kwargs(cfg)
        conf = {"generator_params": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()},
                "n_mels": cfg["in_channels"], "pqmf_params": {"subbands": 4, "taps": 62, "cutoff_ratio": 0.142, "beta": 9.0}}
        d = tmp_path / name
        d.mkdir()
        (d / "default.yaml").write_text(yaml.safe_dump(conf))
        arch = {k: ("t_" + k, v) for k, v in state.items()}
        arch["pqmf.analysis_filter"] = ("t_pqmf", np.zeros((4, 1, 63), np.float32))
        arch["pqmf.updown_filter"] = ("t_pqmf2", np.zeros((4, 4, 4), np.float32))
        with open(d / "snapshot_iter_10.pdz", "wb") as f:
            pickle.dump({"epoch": 1, "iteration": 10, "generator_params": arch, "discriminator_params": {}}, f, protocol=2)
        stats = np.stack([np.linspace(-1, 1, cfg["in_channels"]), np.linspace(0.5, 2, cfg["in_channels"])]).astype(np.float32)
        np.save(d / "stats.npy", stats)
        voc = ck.load_melgan(str(d / "default.yaml"), str(d / "snapshot_iter_10.pdz"), str(d / "stats.npy"))
        assert isinstance(voc, MelGANInference) and voc.pwg_generator is voc.generator
        got = voc.generator.state_dict()
        assert set(got) == set(state)
        for k in state:
            np.testing.assert_array_equal(got[k], state[k])
        assert voc.generator.training is False
        if name == "MB-TINY":
            assert voc.pqmf.subbands == 4 and voc.pqmf.taps == 62 and voc.generator.upsample_factor == 24
        else:
            assert voc.pqmf is None and voc.generator.upsample_factor == 6
        np.testing.assert_array_equal(voc.normalizer.mu, stats[0])


MUTANTS = ("zero", "inzero", "askip", "dil", "noact")


@pytest.mark.parametrize("math", mr.MATHS)
def test_bound_is_not_vacuous(math):
    """Every mutant -- zero padding where the model reflects among them -- leaves the bound restarted at every launch (ratio
    > 1) on the GPU test's own TINY inputs, the shortest utterance included; the restatement rounded to float32 stays far
    inside it."""
    _, model = model_of("TINY")
    import fp32_bounds as fb  # noqa: F401
    for mel in mr.make_mels("TINY", (4, 22)):
        ref = mr.forward(model, mel, maths=(math,))
        s32 = [s.astype(np.float32) for s in ref["stages"]]
        o32 = ref["out"].astype(np.float32)
        own = mr.local_ratio(model, mel, s32, o32, math)
        own_c = mr.conv_ratios(model, mel, [t.astype(np.float32) for t in ref["taps"]], o32, math)
        print(f"MUTANT-RATIO melgan TINY {math} frames={len(mel)} exact-rounded: per-launch={max(own_c):.3g} per-stage={max(own):.3g} "
              f"whole-model bound/peak={float(ref['b_out'][math].max()) / np.abs(ref['out']).max():.3g}")
        assert max(own) < 0.5 and max(own_c) < 0.5
        for name in MUTANTS:
            stages, out, taps = mr.mutant(model, mel, name)
            per = mr.conv_ratios(model, mel, [t.astype(np.float32) for t in taps], out.astype(np.float32), math)
            print(f"MUTANT-RATIO melgan TINY {math} frames={len(mel)} {name}: per-launch={max(per):.3g}")
            assert max(per) > 1.0, (name, per)
