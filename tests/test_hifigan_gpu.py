"""HiFi-GAN generator on the engine (csrc/hifigan.hip) against the fp64 restatement of tests/hifigan_ref.py.

Every configuration of hifigan_ref.CONFIGS runs a ragged batch in both maths; the waveform and every stage tap must stay
within the derived whole-model bound, and -- the sharp checks -- within the same derivation restarted at every stage and at
every convolution from the engine's own taps (hifigan_ref.local_ratio / conv_ratios).  ``SWEEP-RATIO`` lines carry the
figures.  TINY's lengths (6 ... 258 samples) put utterance ends anywhere against the 256-sample tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import fp32_bounds as fb  # noqa: E402
import hifigan_ref as hr  # noqa: E402

from parakeet_amd import _capi  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-4   # README: the wav relative error bar of every vocoder test
_MODELS, _REFS = {}, {}


def setup(name):
    """(state, restatement model, mels) of a configuration; built once."""
    if name not in _MODELS:
        cfg = hr.CONFIGS[name]
        state = syn.hifigan_state(cfg, seed=hr.SEEDS[name])
        _MODELS[name] = (state, hr.Model(cfg, state), hr.make_mels(name))
    return _MODELS[name]


def reference(name, b):
    """forward() with the bounds of both maths for utterance b of the configuration's batch; computed once, never changed."""
    if (name, b) not in _REFS:
        _, model, mels = setup(name)
        r = hr.forward(model, mels[b], maths=hr.MATHS)
        assert np.abs(r["wav"]).max() < 0.95, "the oracle must stay away from tanh's saturation"
        _REFS[(name, b)] = r
    return _REFS[(name, b)]


def engine(name, math="f16x3", state=None):
    from parakeet_amd.hifigan import HiFiGANGenerator
    g = HiFiGANGenerator(**hr.ctor_kwargs(hr.CONFIGS[name]))
    g.set_state_dict(setup(name)[0] if state is None else state)
    g.remove_weight_norm()
    g.eval()
    g.set_math(math)
    return g


def host(t):
    return t.as_subclass(torch.Tensor).cpu().numpy()


@pytest.mark.parametrize("math", hr.MATHS)
@pytest.mark.parametrize("name", list(hr.CONFIGS))
def test_sweep_within_derived_bounds(name, math):
    _, model, mels = setup(name)
    g = engine(name, math)
    outs = g.inference_batch(mels)
    worst = {"whole": 0.0, "stage": 0.0, "conv": 0.0}
    for b, mel in enumerate(mels):
        wav = host(outs[b])[:, 0]
        assert wav.shape == (len(mel) * model.hop,)
        stages = g.debug_stages(b)
        taps = g.debug_convs(b)
        ref = reference(name, b)
        whole = hr.global_ratio(ref, stages, wav, math)
        per_stage = max(hr.local_ratio(model, mel, stages, wav, math))
        per_conv = hr.conv_ratios(model, mel, taps, wav, math)
        print(f"SWEEP-RATIO hifigan {name} {math} frames={len(mel)}: whole-model={whole:.3g} per-stage={per_stage:.3g} "
              f"per-conv={max(per_conv):.3g} (launch {int(np.argmax(per_conv))}) "
              f"err/peak={np.abs(wav - ref['wav']).max() / np.abs(ref['wav']).max():.3g}")
        worst = {"whole": max(worst["whole"], whole), "stage": max(worst["stage"], per_stage),
                 "conv": max(worst["conv"], max(per_conv))}
        # the last stage tap is what the output convolution read; the last launch's tap is the same buffer
        np.testing.assert_array_equal(taps[-1], stages[-1])
    print(f"SWEEP-RATIO hifigan {name} {math} worst: {worst}")
    assert worst["whole"] <= 1.0 and worst["stage"] <= 1.0 and worst["conv"] <= 1.0, worst


@pytest.mark.parametrize("name", ["TINY", "CS"])
def test_weight_norm_state_against_the_restatement(name):
    """weight_g / weight_v pairs handed to the engine as they are (g as (C, 1, 1), both layouts: Conv1D normalised over its
    output channels, Conv1DTranspose (C_in, C_out, k) over axis 0 too): its folding is the restatement's."""
    cfg = hr.CONFIGS[name]
    state = syn.hifigan_state(cfg, seed=hr.SEEDS[name] + 50, weight_norm=True)
    assert "upsamples.0.1.weight_g" in state and "upsamples.0.1.weight" not in state
    model = hr.Model(cfg, state)
    mels = hr.make_mels(name, (3, 9))
    g = engine(name, "f16x3", state)
    outs = g.inference_batch(mels)
    for b, mel in enumerate(mels):
        wav = host(outs[b])[:, 0]
        per_conv = hr.conv_ratios(model, mel, g.debug_convs(b), wav, "f16x3")
        print(f"SWEEP-RATIO hifigan {name} weight-norm state frames={len(mel)}: per-conv={max(per_conv):.3g}")
        assert max(per_conv) <= 1.0


@pytest.mark.parametrize("math", hr.MATHS)
@pytest.mark.parametrize("name", ["TINY", "CS"])
def test_same_bits_alone_in_any_batch_and_order(name, math):
    _, _, mels = setup(name)
    g = engine(name, math)
    batch = [host(o) for o in g.inference_batch(mels)]
    rev = [host(o) for o in g.inference_batch(mels[::-1])][::-1]
    for b, mel in enumerate(mels):
        alone = host(g.inference(mel))
        np.testing.assert_array_equal(alone, batch[b])
        np.testing.assert_array_equal(alone, rev[b])
    pair = [host(o) for o in g.inference_batch([mels[-1], mels[2], mels[-1]])]
    np.testing.assert_array_equal(pair[0], batch[-1])
    np.testing.assert_array_equal(pair[1], batch[2])
    np.testing.assert_array_equal(pair[2], batch[-1])


def test_entry_points_agree_bit_for_bit():
    _, model, _ = setup("TINY")
    g = engine("TINY")
    ctx = g._engine()
    mels = hr.make_mels("TINY", (11, 11))
    want = [host(o)[:, 0] for o in g.inference_batch(mels)]
    fwd = host(g.forward(np.stack([m.T for m in mels])))                     # (N, C_in, T') -> (N, 1, T' hop)
    assert fwd.shape == (2, 1, 11 * model.hop)
    packed = host(g.infer_packed(ctx.to_device(np.concatenate(mels)), [11, 11]))
    for b in range(2):
        np.testing.assert_array_equal(fwd[b, 0], want[b])
        np.testing.assert_array_equal(host(g.inference(mels[b]))[:, 0], want[b])
        np.testing.assert_array_equal(packed[b * 11 * model.hop:(b + 1) * 11 * model.hop], want[b])
    # host pointers through the C ABI
    flat = np.ascontiguousarray(np.concatenate(mels))
    frames = np.array([11, 11], np.int32)
    out = np.empty(22 * model.hop, np.float32)
    _capi.check(ctx.lib.pk_hfg_infer(g._h, _capi.fptr(flat), frames.ctypes.data_as(C.POINTER(C.c_int32)), 2, _capi.fptr(out),
                                     _capi.PK_HOST_IO))
    np.testing.assert_array_equal(out, np.concatenate(want))
    with pytest.raises(ValueError):
        g.infer_packed(ctx.to_device(flat), [11, 11], noise=np.zeros(4))
    # the C side's own refusals and states
    lib = ctx.lib
    cfg = g._cfg()
    cfg.upsample_kernel_sizes[0] = 5
    h = C.c_void_p()
    assert lib.pk_hfg_create(ctx.handle, C.byref(cfg), C.byref(h)) == -3 and not h
    cfg = g._cfg()
    cfg.bias = 0
    assert lib.pk_hfg_create(ctx.handle, C.byref(cfg), C.byref(h)) == -3
    assert lib.pk_hfg_set_math(g._h, _capi.PK_PWG_MATH_BF16X3) == -3 and lib.pk_hfg_set_math(g._h, 7) == -1
    buf = np.empty(4, np.float32)
    assert lib.pk_hfg_debug_read(g._h, 0, 0, _capi.fptr(buf), buf.size) == -2           # wrong size
    assert lib.pk_hfg_debug_read(g._h, 9, 0, _capi.fptr(buf), buf.size) == -1
    assert lib.pk_hfg_infer(g._h, _capi.fptr(flat), frames.ctypes.data_as(C.POINTER(C.c_int32)), 0, _capi.fptr(out), 1) == -1


def test_normalize_equals_normalising_on_the_host():
    from parakeet_amd.hifigan import HiFiGANInference
    from parakeet_amd.normalizer import ZScore
    _, _, mels = setup("TINY")
    rng = np.random.default_rng(4)
    mu = rng.normal(size=20).astype(np.float32)
    sigma = rng.uniform(0.5, 2.0, size=20).astype(np.float32)
    g = engine("TINY")
    voc = HiFiGANInference(ZScore(mu, sigma), g)
    raw = [(m * sigma + mu).astype(np.float32) for m in mels]
    on_host = [((r - mu) / sigma).astype(np.float32) for r in raw]
    want = g.inference_batch(on_host)
    got = g.inference_batch(raw, normalize=True)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(host(a), host(b))
    np.testing.assert_array_equal(host(voc(raw[3])), host(want[3]))


@pytest.mark.parametrize("math", hr.MATHS)
@pytest.mark.parametrize("e", [20, -20])
def test_internal_scale_does_not_matter(e, math):
    """input_conv's weight and every bias up to the last stage times 2^e, output_conv's weight times 2^-e: the same function
    (LeakyReLU is positively homogeneous; output_conv's own bias adds to the unscaled pre-activation and stays).  The
    result stays within the same bounds -- computed for the scaled model, whose exact result is the original's -- and
    the test prints whether it is the same bits."""
    state, model, mels = setup("TINY")
    scaled = {}
    for k, v in state.items():
        if k == "output_conv.1.weight":
            scaled[k] = np.ldexp(v, -e)
        elif k == "input_conv.weight" or (k.endswith(".bias") and k != "output_conv.1.bias"):
            scaled[k] = np.ldexp(v, e)
        else:
            scaled[k] = v
    m2 = hr.Model(hr.CONFIGS["TINY"], scaled)
    g, g2 = engine("TINY", math), engine("TINY", math, scaled)
    a, b = g.inference_batch(mels), g2.inference_batch(mels)
    same = True
    for i, mel in enumerate(mels):
        wav, wav2 = host(a[i])[:, 0], host(b[i])[:, 0]
        same = same and np.array_equal(wav, wav2)
        ref = reference("TINY", i)
        whole = fb.ratio(wav2, ref["wav"], ref["b_wav"][math])
        per_conv = max(hr.conv_ratios(m2, mel, g2.debug_convs(i), wav2, math))
        print(f"SWEEP-RATIO hifigan TINY {math} scaled 2^{e} frames={len(mel)}: whole-model={whole:.3g} per-conv={per_conv:.3g}")
        assert whole <= 1.0 and per_conv <= 1.0
    print(f"SWEEP-RATIO hifigan TINY {math} scaled 2^{e}: bit-equal to the unscaled model: {same}")


def test_synthesizer_fastspeech2_to_hifigan():
    from parakeet_amd.fastspeech2 import FastSpeech2, FastSpeech2Inference
    from parakeet_amd.hifigan import HiFiGANGenerator, HiFiGANInference
    from parakeet_amd.normalizer import ZScore
    from parakeet_amd.synthesize import Synthesizer
    cfg = hr.CONFIGS["V2"]
    g = HiFiGANGenerator(**hr.ctor_kwargs(cfg))
    g.set_state_dict(syn.hifigan_state(cfg, seed=21, weight_norm=True))
    g.eval()
    am = FastSpeech2(80, 80, **syn.FS2_LJSPEECH)
    am.set_state_dict(syn.fastspeech2_state(fixed_duration=2))
    am.eval()
    pmu, psd = syn.mel_stats(seed=6)
    voc = HiFiGANInference(ZScore(pmu, psd), g)
    synth = Synthesizer(FastSpeech2Inference(ZScore(*syn.mel_stats(seed=5)), am), voc)
    assert synth.voc is g and synth.hop == 256
    texts = [syn.phoneme_ids(9, seed=3), syn.phoneme_ids(5, seed=4)]
    wav, frames = synth.synthesize_packed(texts)
    frames = [int(f) for f in frames]
    wav = host(wav)
    assert len(frames) == 2 and min(frames) > 0 and wav.shape == (sum(frames) * 256,) and np.isfinite(wav).all()
    mel = host(am.decode_packed(denormalize=True)).reshape(-1, 80)
    mels = [mel[:frames[0]], mel[frames[0]:frames[0] + frames[1]]]
    want = np.concatenate([host(o)[:, 0] for o in g.inference_batch(mels, normalize=True)])
    np.testing.assert_array_equal(wav, want)
    outs = synth.synthesize_batch(texts)
    np.testing.assert_array_equal(np.concatenate([host(o)[:, 0] for o in outs]), want)


@pytest.mark.parametrize("math", hr.MATHS)
def test_v1_two_by_forty_frames_against_fp64(math):
    """One full-width run: HiFi-GAN V1, 2 x 40 frames (20 480 samples), against the same stack in float64 (torch on the
    device).  The bar is the vocoders' north star of the README, the wav relative error 1e-4; the measured figure is printed
    and recorded in DESIGN.md 4.1d."""
    state, _, _ = setup("V1")
    mels = hr.make_mels("V1", (40, 40))
    g = engine("V1", math)
    outs = g.inference_batch(mels)
    dev = outs[0].device
    chain = hr.torch_chain(hr.CONFIGS["V1"], state, mels, device=dev)
    for b in range(2):
        want = chain[b][1]
        assert np.abs(want).max() < 0.95
        got = host(outs[b])[:, 0]
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"SWEEP-RATIO hifigan V1 {math} 40 frames: wav relative error {rel:.3g} (mean abs {np.abs(got - want).mean():.3g})")
        assert rel < NORTH_STAR
