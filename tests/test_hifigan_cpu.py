"""HiFi-GAN generator without a device: the fp64 restatement (tests/hifigan_ref.py) against an independent torch chain,
weight-norm folding, the constructor's refusals, the checkpoint loader, and the proof that the derived bound can tell
wrong evaluations from right ones."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import fp32_bounds as fb  # noqa: E402
import hifigan_ref as hr  # noqa: E402

from parakeet_amd import synthetic as syn  # noqa: E402
from parakeet_amd.hifigan import HiFiGANGenerator, HiFiGANInference  # noqa: E402

_CACHE = {}


def model_of(name, weight_norm=False):
    key = (name, weight_norm)
    if key not in _CACHE:
        cfg = hr.CONFIGS[name]
        state = syn.hifigan_state(cfg, seed=hr.SEEDS[name], weight_norm=weight_norm)
        _CACHE[key] = (state, hr.Model(cfg, state))
    return _CACHE[key]


@pytest.mark.parametrize("name", list(hr.CONFIGS))
def test_restatement_equals_torch_chain(name):
    """conv1d / conv_transpose1d in float64 state the same function; lengths are exactly T' hop (odd scales too) and the
    waveform stays away from tanh's saturation."""
    state, model = model_of(name)
    frames = (1, 3) if name == "V1" else (1, 2, 7)
    mels = hr.make_mels(name, frames)
    chain = hr.torch_chain(hr.CONFIGS[name], state, mels)
    for mel, (stages, wav) in zip(mels, chain):
        r = hr.forward(model, mel, maths=())
        assert r["wav"].shape == (len(mel) * model.hop,) == wav.shape
        for a, b in zip(r["stages"], stages):
            assert a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-11 * max(1.0, np.abs(b).max()))
        np.testing.assert_allclose(r["wav"], wav, rtol=0, atol=1e-11)
        assert np.abs(r["wav"]).max() < 0.95


@pytest.mark.parametrize("s", [2, 3, 5, 8])
def test_transposed_identity(s):
    rng = np.random.default_rng(s)
    x, w = rng.standard_normal((6, 9)), rng.standard_normal((6, 4, 2 * s))
    want = torch.nn.functional.conv_transpose1d(torch.as_tensor(x)[None], torch.as_tensor(w), stride=s,
                                                padding=s // 2 + s % 2, output_padding=s % 2)[0].numpy()
    got = hr.conv_transpose(x, w, s)
    assert got.shape == (4, 9 * s)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    assert np.abs(hr.conv_transpose(x, w, s, swap=True) - want).max() > 0.1


def test_weight_norm_folding_both_layouts():
    cfg = hr.CONFIGS["TINY"]
    state = syn.hifigan_state(cfg, seed=5, weight_norm=True)
    for base, shape0 in (("blocks.0.convs1.0.1", 16), ("upsamples.0.1", 32)):   # Conv1D (C_out, ...), Conv1DTranspose (C_in, ...)
        g, v = state[base + ".weight_g"], state[base + ".weight_v"]
        assert v.shape[0] == shape0 and g.size == shape0
        want = np.empty(v.shape, np.float32)
        for o in range(shape0):
            want[o] = (v[o].astype(np.float64) * (float(g.reshape(-1)[o]) / np.sqrt((v[o].astype(np.float64) ** 2).sum()))
                       ).astype(np.float32)
        np.testing.assert_array_equal(hr.folded(state, base), want)
        flat = dict(state)
        flat[base + ".weight_g"] = g.reshape(-1)            # g of any shape with that many elements
        np.testing.assert_array_equal(hr.folded(flat, base), want)
    # the folded model is the model of the plain weights
    plain = {}
    for k_, v_ in state.items():
        if k_.endswith(".weight_g"):
            plain[k_[:-9] + ".weight"] = hr.folded(state, k_[:-9])
        elif not k_.endswith(".weight_v"):
            plain[k_] = v_
    mel = hr.make_mels("TINY", (5,))[0]
    a = hr.forward(hr.Model(cfg, state), mel, maths=())["wav"]
    b = hr.forward(hr.Model(cfg, plain), mel, maths=())["wav"]
    np.testing.assert_array_equal(a, b)


REFUSED = [
    dict(global_channels=256), dict(nonlinear_activation="ReLU"), dict(nonlinear_activation_params={"negative_slope": 0.1, "x": 1}),
    dict(bias=False), dict(in_channels=0), dict(in_channels=513), dict(out_channels=2), dict(kernel_size=4),
    dict(kernel_size=13), dict(kernel_size=1), dict(upsample_scales=(), upsample_kernel_sizes=()),
    dict(upsample_scales=(2,) * 7, upsample_kernel_sizes=(4,) * 7, channels=256),
    dict(upsample_scales=(8, 8, 2, 1), upsample_kernel_sizes=(16, 16, 4, 2)),
    dict(upsample_scales=(17, 2), upsample_kernel_sizes=(34, 4)), dict(upsample_kernel_sizes=(16, 16, 4, 8)),
    dict(upsample_kernel_sizes=(15, 16, 4, 4)), dict(upsample_scales=(2,), upsample_kernel_sizes=(4,)),
    dict(upsample_scales=(16, 16, 8), upsample_kernel_sizes=(32, 32, 16)), dict(channels=64), dict(channels=1024),
    dict(channels=520), dict(resblock_kernel_sizes=(), resblock_dilations=()),
    dict(resblock_kernel_sizes=(3,) * 5, resblock_dilations=((1,),) * 5), dict(resblock_kernel_sizes=(3, 4, 11)),
    dict(resblock_kernel_sizes=(3, 7, 13)), dict(resblock_dilations=((1, 3, 5), (1, 3, 5), ())),
    dict(resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 2, 3, 4, 5))), dict(resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 13))),
    dict(resblock_dilations=((1, 3, 5), (1, 3, 0), (1, 3, 5))), dict(resblock_dilations=((1, 3, 5), (1, 3, 5))),
]


@pytest.mark.parametrize("kw", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals_need_no_device(kw):
    with pytest.raises(NotImplementedError):
        HiFiGANGenerator(**kw)


def test_envelope_accepts_the_configurations():
    for name, cfg in hr.CONFIGS.items():
        g = HiFiGANGenerator(**hr.ctor_kwargs(cfg))
        assert g.upsample_factor == int(np.prod(cfg["upsample_scales"])) and g._h is None
    g = HiFiGANGenerator()
    assert g.upsample_factor == 256 and g.negative_slope == pytest.approx(0.1)
    with pytest.raises(ValueError):
        g.infer_packed(None, [1], noise=np.zeros(256))
    with pytest.raises(NotImplementedError):
        g.set_math("bf16x3")
    import parakeet_amd
    assert parakeet_amd.HiFiGANGenerator is HiFiGANGenerator and parakeet_amd.HiFiGANInference is HiFiGANInference


def test_load_hifigan_round_trip(tmp_path):
    """yaml generator_params + the updaters' nested archive + stats.npy -> HiFiGANInference holding the same tensors."""
    import yaml
    from parakeet_amd import checkpoint as ck
    cfg = hr.CONFIGS["TINY"]
    state = syn.hifigan_state(cfg, seed=3, weight_norm=True)
    kw = hr.ctor_kwargs(cfg)
    conf = {"generator_params": {k: (list(map(list, v)) if k == "resblock_dilations" else list(v) if isinstance(v, tuple) else v)
                                 for k, v in kw.items()}, "n_mels": cfg["in_channels"]}
    (tmp_path / "default.yaml").write_text(yaml.safe_dump(conf))
    with open(tmp_path / "snapshot_iter_10.pdz", "wb") as f:
        pickle.dump({"epoch": 1, "iteration": 10, "generator_params": {k: ("t_" + k, v) for k, v in state.items()},
                     "discriminator_params": {}}, f, protocol=2)
    stats = np.stack([np.linspace(-1, 1, cfg["in_channels"]), np.linspace(0.5, 2, cfg["in_channels"])]).astype(np.float32)
    np.save(tmp_path / "stats.npy", stats)
    voc = ck.load_hifigan(str(tmp_path / "default.yaml"), str(tmp_path / "snapshot_iter_10.pdz"), str(tmp_path / "stats.npy"))
    assert isinstance(voc, HiFiGANInference) and voc.pwg_generator is voc.generator
    got = voc.generator.state_dict()
    assert set(got) == set(state)
    for k in state:
        np.testing.assert_array_equal(got[k], state[k])
    assert voc.generator.upsample_factor == 6 and voc.generator.training is False
    np.testing.assert_array_equal(voc.normalizer.mu, stats[0])


MUTANTS = ("outslope", "nb_plus", "nb_minus", "tapswap", "abias", "dil")


@pytest.mark.parametrize("math", hr.MATHS)
def test_bound_is_not_vacuous(math):
    """Every mutant leaves the bound restarted at every convolution (ratio > 1) on the GPU test's own TINY inputs; the
    restatement rounded to float32 -- the best any fp32 evaluation can do -- stays far inside it.  The stage-restarted and
    the whole-model bound are printed beside it: carried through |W| over many layers they approach or exceed the signal
    (DESIGN.md 4.1d), which is why the restart exists."""
    _, model = model_of("TINY")
    for mel in hr.make_mels("TINY", (22, 43)):
        ref = hr.forward(model, mel, maths=(math,))
        assert np.abs(ref["wav"]).max() < 0.95
        s32 = [s.astype(np.float32) for s in ref["stages"]]
        w32 = ref["wav"].astype(np.float32)
        own = hr.local_ratio(model, mel, s32, w32, math)
        own_c = hr.conv_ratios(model, mel, [t.astype(np.float32) for t in ref["taps"]], w32, math)
        print(f"MUTANT-RATIO TINY {math} frames={len(mel)} exact-rounded: per-conv={max(own_c):.3g} per-stage={max(own):.3g} "
              f"whole-model bound/peak={float(ref['b_wav'][math].max()) / np.abs(ref['wav']).max():.3g}")
        assert max(own) < 0.5 and max(own_c) < 0.5
        for name in MUTANTS:
            stages, wav, taps = hr.mutant(model, mel, name)
            w32 = wav.astype(np.float32)
            per_conv = hr.conv_ratios(model, mel, [t.astype(np.float32) for t in taps], w32, math)
            loc = hr.local_ratio(model, mel, [s.astype(np.float32) for s in stages], w32, math)
            glo = hr.global_ratio(ref, stages, wav, math)
            print(f"MUTANT-RATIO TINY {math} frames={len(mel)} {name}: per-conv={max(per_conv):.3g} per-stage={max(loc):.3g} "
                  f"whole-model={glo:.3g}")
            assert max(per_conv) > 1.0, (name, per_conv)


def test_split_lo_terms_are_needed():
    """f16x3: output_conv through fb.split_emulation stays inside the bound of one convolution; with the lo terms dropped
    it leaves it."""
    _, model = model_of("TINY")
    mel = hr.make_mels("TINY", (43,))[0]
    x = hr.forward(model, mel, maths=())["stages"][-1].astype(np.float32)
    r = hr.forward(model, maths=("f16x3",), first=len(model.scales), x0=x)
    want, bound = r["pre"], r["b_pre"]["f16x3"]
    good = fb.ratio(hr.output_conv_split(model, x), want, bound)
    bad = fb.ratio(hr.output_conv_split(model, x, drop_lo=True), want, bound)
    print(f"MUTANT-RATIO TINY f16x3 output_conv split emulation: full={good:.3g} lo dropped={bad:.3g}")
    assert good <= 1.0 < bad
