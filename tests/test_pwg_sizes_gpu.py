"""GPU: Parallel WaveGAN generators of non-default channel widths and kernel sizes on the shape-generic kernels
(csrc/pwg_gen.hip), through the C ABI.

Goldens: tests/golden/pwg_sizes.npz (tools/make_golden_pwg_sizes.py: the reference's own PWGGenerator over the paddle
stand-in).  The conftest's GOLDEN_MODULES list is not extended, so these tests always read the stand-in goldens; the
fp64 oracle (oracle/pwg_ref.py) is pinned to them by tests/test_pwg_sizes_cpu.py.
"""
import json
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "pwg_sizes.npz")
FIX = os.path.join(HERE, "fixtures")
NAMES = sorted(syn.PWG_SIZES)
MATHS = ["f32", "f16x3", "bf16x3"]
# wav relative error: the north star, and the regression bars of the maths (measured on MI355X: at most 1.1e-5 in every
# mode and configuration, 6e-7 generic vs tuned at the default shape)
NORTH_STAR = 1e-4
BAR = {"f32": 5e-5, "f16x3": 5e-5, "bf16x3": 1e-4}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _gen(cfg, state, math_="f16x3", options=None):
    from parakeet_amd.parallel_wavegan import PWGGenerator
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(state)
    gen.remove_weight_norm()
    gen.eval()
    gen.set_math(math_)
    for k, v in (options or {}).items():
        gen.set_option(k, v)
    return gen


def _check(err, m):
    assert err < NORTH_STAR and err < BAR[m], f"{m}: rel err {err:.3e}"


@pytest.mark.parametrize("m", MATHS)
@pytest.mark.parametrize("name", NAMES)
def test_engine_matches_reference_golden(name, m):
    g = np.load(GOLD)
    cfg = syn.pwg_size_config(name)
    gen = _gen(cfg, syn.pwg_state(cfg, seed=int(g[f"{name}_seed"]), weight_norm=True), m)
    y = gen(torch.from_numpy(g[f"{name}_fwd_x"]), torch.from_numpy(g[f"{name}_fwd_c"])).cpu().numpy()
    assert y.shape == g[f"{name}_fwd_y"].shape
    e1 = _rel(y, g[f"{name}_fwd_y"])
    wav = gen.inference(g[f"{name}_inf_mel"], noise=g[f"{name}_inf_noise"]).cpu().numpy()
    assert wav.shape == g[f"{name}_inf_wav"].shape
    e2 = _rel(wav, g[f"{name}_inf_wav"])
    print(f"pwg_sizes golden {name} {m}: forward {e1:.3e} inference {e2:.3e}")
    _check(e1, m)
    _check(e2, m)


def _oracle_case(cfg, state, mels, noises, outs, gen, taps=True):
    from oracle import pwg_ref
    from oracle.nn_ref import fold_weight_norm
    errs = []
    for b in range(len(mels)):
        c = torch.from_numpy(mels[b]).transpose(0, 1).unsqueeze(0)
        c = torch.nn.functional.pad(c, (cfg["aux_context_window"],) * 2, mode="replicate")
        x = torch.from_numpy(noises[b]).reshape(1, 1, -1)
        ref, parts = pwg_ref.generator_forward(state, x, c, cfg, torch.float64, return_parts=True)
        if taps:
            wa = torch.as_tensor(fold_weight_norm(state)["conv_layers.0.conv1x1_aux.weight"]).double()
            aux0 = torch.nn.functional.conv1d(parts["c_up"], wa)[0].numpy()
            t0 = gen.debug_tap(0, b)
            assert t0.shape == (cfg["gate_channels"], mels[b].shape[0] * gen.upsample_factor)
            assert _rel(t0, aux0) < 1e-5
            assert _rel(gen.debug_tap(1, b), parts["x_last"][0].numpy()) < NORTH_STAR
            skips = gen.debug_tap(2, b) * math.sqrt(1.0 / cfg["layers"])
            assert _rel(skips, parts["skips"][0].numpy()) < NORTH_STAR
        errs.append(_rel(outs[b].cpu().numpy()[:, 0], ref[0, 0].numpy()))
    return max(errs)


def _inputs(cfg, frames, seed):
    rng = np.random.default_rng(seed)
    hop = int(np.prod(cfg["upsample_scales"]))
    mels = [rng.normal(size=(L, cfg["aux_channels"])).astype(np.float32) for L in frames]
    noises = [rng.normal(size=(L * hop,)).astype(np.float32) for L in frames]
    return mels, noises


@pytest.mark.parametrize("name", NAMES)
def test_ragged_batch_against_oracle_with_taps(name):
    cfg = syn.pwg_size_config(name)
    state = syn.pwg_state(cfg, seed=11, weight_norm=True)
    mels, noises = _inputs(cfg, [1, 3, 17, 64], seed=12)
    gen = _gen(cfg, state)
    outs = gen.inference_batch(mels, noises)
    err = _oracle_case(cfg, state, mels, noises, outs, gen)
    print(f"pwg_sizes ragged {name}: {err:.3e}")
    _check(err, "f16x3")


@pytest.mark.parametrize("name", ["A", "C"])
def test_batch_invariance_and_chunking_are_bitwise(name):
    cfg = syn.pwg_size_config(name)
    state = syn.pwg_state(cfg, seed=21)
    frames = [2, 9, 1, 5]
    mels, noises = _inputs(cfg, frames, seed=22)
    gen = _gen(cfg, state)
    batch = [o.cpu().numpy() for o in gen.inference_batch(mels, noises)]
    for b in range(len(frames)):
        alone = gen.inference_batch([mels[b]], [noises[b]])[0].cpu().numpy()
        assert np.array_equal(alone, batch[b]), f"utterance {b}"
    hop = gen.upsample_factor
    gen.set_chunk_samples(6 * hop)
    chunked = [o.cpu().numpy() for o in gen.inference_batch(mels, noises)]
    assert all(np.array_equal(a, c) for a, c in zip(batch, chunked))


def test_generic_kernel_on_default_shape():
    cfg = dict(syn.PWG_LJSPEECH)
    state = syn.pwg_state(cfg, seed=31, weight_norm=True)
    mels, noises = _inputs(cfg, [3, 7], seed=32)
    tuned = _gen(cfg, state)
    ref = [o.cpu().numpy() for o in tuned.inference_batch(mels, noises)]
    gen = _gen(cfg, state)
    gen.inference_batch(mels, noises)
    gen.set_option("generic_kernel", 1)           # marks the generator un-finalised: the next call re-packs
    got = [o.cpu().numpy() for o in gen.inference_batch(mels, noises)]
    for a, b in zip(got, ref):
        err = _rel(a, b)
        print(f"generic vs tuned (default shape): {err:.3e}")
        _check(err, "f16x3")
    assert _oracle_case(cfg, state, mels, noises, [torch.from_numpy(a) for a in got], gen) < BAR["f16x3"]
    with pytest.raises(RuntimeError):
        gen.scale_overshoot()                      # PK_ESTATE: the generic path has no scale guard
    for opt in ("planes", "scale_guard", "scale_guard_every", "noise_fed_first"):
        gen.set_option(opt, 0)                     # accepted, no effect
    assert all(np.array_equal(a, o.cpu().numpy()) for a, o in zip(got, gen.inference_batch(mels, noises)))
    # the recipe golden of the default shape
    g = np.load(os.path.join(HERE, "golden", "pwg_ljspeech.npz"))
    gen2 = _gen(cfg, syn.pwg_state(cfg, seed=int(g["seed"]), weight_norm=True), options={"generic_kernel": 1})
    y = gen2(torch.from_numpy(g["fwd_x"]), torch.from_numpy(g["fwd_c"])).cpu().numpy()
    _check(_rel(y, g["fwd_y"]), "f16x3")
    wav = gen2.inference(g["inf_mel"], noise=g["inf_noise"]).cpu().numpy()
    _check(_rel(wav, g["inf_wav"]), "f16x3")
    gen2.set_option("generic_kernel", 0)
    back = gen2.inference(g["inf_mel"], noise=g["inf_noise"]).cpu().numpy()
    tuned2 = _gen(cfg, syn.pwg_state(cfg, seed=int(g["seed"]), weight_norm=True))
    assert np.array_equal(back, tuned2.inference(g["inf_mel"], noise=g["inf_noise"]).cpu().numpy())


def test_large_shape_long_utterance():
    cfg = syn.pwg_size_config("B")
    state = syn.pwg_state(cfg, seed=41)
    mels, noises = _inputs(cfg, [640], seed=42)
    gen = _gen(cfg, state)
    err = _oracle_case(cfg, state, mels, noises, gen.inference_batch(mels, noises), gen, taps=False)
    print(f"pwg_sizes B 640 frames: {err:.3e}")
    _check(err, "f16x3")


def test_internal_noise_and_normalizer():
    from parakeet_amd.normalizer import ZScore
    from parakeet_amd.parallel_wavegan import PWGInference
    cfg = syn.pwg_size_config("D")
    state = syn.pwg_state(cfg, seed=51)
    gen = _gen(cfg, state)
    mu = np.linspace(-1, 1, 100).astype(np.float32)
    sigma = np.linspace(0.5, 2, 100).astype(np.float32)
    mel = np.random.default_rng(52).normal(size=(5, 100)).astype(np.float32)
    gen.set_seed(7)
    a = gen.inference(mel).cpu().numpy()
    gen.set_seed(7)
    b = gen.inference(mel).cpu().numpy()
    assert np.array_equal(a, b) and np.isfinite(a).all()
    noise = np.random.default_rng(53).normal(size=(5 * 256,)).astype(np.float32)
    n1 = PWGInference(ZScore(mu, sigma), gen)(mel * sigma + mu, noise=noise).cpu().numpy()
    n2 = gen.inference(mel, noise=noise).cpu().numpy()
    assert _rel(n1, n2) < 1e-5


def _write_pwg_a(tmp_path):
    cfg = syn.pwg_size_config("A")
    state = syn.pwg_state(cfg, seed=61, weight_norm=True)
    with open(tmp_path / "pwg_a.pdz", "wb") as f:
        pickle.dump({"generator_params": {k: ("g%d" % i, v) for i, (k, v) in enumerate(state.items())},
                     "discriminator_params": {}}, f, protocol=4)
    text = open(os.path.join(FIX, "pwg_ljspeech.yaml")).read()
    for key in ("residual_channels", "gate_channels", "skip_channels", "layers", "stacks"):
        default = syn.PWG_LJSPEECH[key]
        assert f"  {key}: {default}\n" in text
        text = text.replace(f"  {key}: {default}\n", f"  {key}: {cfg[key]}\n")
    (tmp_path / "pwg_a.yaml").write_text(text)
    np.save(tmp_path / "pwg_stats.npy", np.stack(syn.mel_stats(seed=6)))
    return cfg, state


def test_checkpoint_and_synthesizer_with_small_vocoder(tmp_path):
    from parakeet_amd import checkpoint as ck
    from parakeet_amd.fastspeech2 import FastSpeech2, FastSpeech2Inference
    from parakeet_amd.normalizer import ZScore
    from parakeet_amd.synthesize import Synthesizer
    cfg, state = _write_pwg_a(tmp_path)
    voc = ck.load_pwg(tmp_path / "pwg_a.yaml", tmp_path / "pwg_a.pdz", tmp_path / "pwg_stats.npy")
    assert voc.pwg_generator.gate_channels == 64 and voc.pwg_generator.layers == 10
    am = FastSpeech2(80, 80, **syn.FS2_LJSPEECH)
    am.set_state_dict(syn.fastspeech2_state(fixed_duration=2))
    am.eval()
    synth = Synthesizer(FastSpeech2Inference(ZScore(*syn.mel_stats(seed=5)), am), voc)
    texts = [syn.phoneme_ids(9, seed=3), syn.phoneme_ids(5, seed=4)]
    wav, frames = synth.synthesize_packed(texts)
    frames = [int(f) for f in frames]
    wav = wav.cpu().numpy()
    assert len(frames) == 2 and min(frames) > 0
    assert wav.shape == (sum(frames) * 256,) and np.isfinite(wav).all()
    # the vocoder on the acoustic model's own mel (the domain synthesize_packed hands it) against the oracle
    from oracle import pwg_ref
    mel = am.decode_packed(denormalize=True).as_subclass(torch.Tensor).cpu().numpy().reshape(-1, 80)[:frames[0]]
    noise = np.random.default_rng(62).normal(size=(frames[0] * 256,)).astype(np.float32)
    got = voc(mel, noise=noise).cpu().numpy()[:, 0]
    pmu, psd = syn.mel_stats(seed=6)
    ref = pwg_ref.pwg_inference({k: torch.from_numpy(v) for k, v in state.items()}, pmu, psd, torch.from_numpy(mel),
                                torch.from_numpy(noise), cfg, torch.float64).numpy()[:, 0]
    _check(_rel(got, ref), "f16x3")


def test_synthesize_vocoder_example_small_config(tmp_path):
    _write_pwg_a(tmp_path)
    rng = np.random.default_rng(71)
    with open(tmp_path / "meta.jsonl", "w") as f:
        for i, L in enumerate((4, 7)):
            np.save(tmp_path / f"u{i}.npy", rng.normal(size=(L, 80)).astype(np.float32))
            f.write(json.dumps({"utt_id": f"u{i}", "feats": f"u{i}.npy"}) + "\n")
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "synthesize_vocoder.py"), "parallel_wavegan",
                        "--config", str(tmp_path / "pwg_a.yaml"), "--checkpoint", str(tmp_path / "pwg_a.pdz"),
                        "--test-metadata", str(tmp_path / "meta.jsonl"), "--output-dir", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == ["u0.wav", "u1.wav"]


@pytest.mark.parametrize("over", [dict(out_channels=2), dict(gate_channels=66), dict(kernel_size=4),
                                  dict(residual_channels=24), dict(use_causal_conv=True), dict(aux_channels=513),
                                  dict(skip_channels=272)])
def test_outside_envelope_raises(over):
    from parakeet_amd.parallel_wavegan import PWGGenerator
    with pytest.raises(NotImplementedError):
        PWGGenerator(**dict(syn.PWG_LJSPEECH, **over))
