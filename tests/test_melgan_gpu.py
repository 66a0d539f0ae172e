"""MelGAN / multi-band MelGAN generator on the engine (csrc/melgan.hip) against the fp64 restatement of tests/melgan_ref.py.

Every small configuration of melgan_ref runs a ragged batch in both maths; the output and every stage tap must stay within
the derived whole-model bound, and -- the sharp checks -- within the same derivation restarted at every stage and at every
launch from the engine's own taps (melgan_ref.local_ratio / conv_ratios).  ``SWEEP-RATIO`` lines carry the figures.  Every
batch holds an utterance of exactly min_frames (the reflection pad of the input convolution is its length - 1) and one of
min_frames + 1; TINY's and S33's lengths put utterance ends at -1, 0, +1 and +2 of a 256-position tile at the output rate
and at the rate of stage 0 (melgan_ref.FRAMES)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import fp32_bounds as fb  # noqa: E402
import melgan_ref as mr  # noqa: E402
import pqmf_ref as pr  # noqa: E402

from parakeet_amd import _capi  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-4   # README: the wav relative error bar of every vocoder test
_MODELS, _REFS = {}, {}


def setup(name):
    """(state, restatement model, mels) of a configuration; built once."""
    if name not in _MODELS:
        cfg = mr.CONFIGS[name]
        state = syn.melgan_state(cfg, seed=mr.SEEDS[name])
        _MODELS[name] = (state, mr.Model(cfg, state), mr.make_mels(name) if name in mr.FRAMES else None)
    return _MODELS[name]


def reference(name, b):
    """forward() with the bounds of both maths for utterance b of the configuration's batch; computed once, never changed."""
    if (name, b) not in _REFS:
        _, model, mels = setup(name)
        _REFS[(name, b)] = mr.forward(model, mels[b], maths=mr.MATHS)
    return _REFS[(name, b)]


def engine(name, math="f16x3", state=None):
    from parakeet_amd.melgan import MelGANGenerator
    g = MelGANGenerator(**mr.ctor_kwargs(mr.CONFIGS[name]))
    g.set_state_dict(setup(name)[0] if state is None else state)
    g.remove_weight_norm()
    g.eval()
    g.set_math(math)
    return g


def host(t):
    return t.as_subclass(torch.Tensor).cpu().numpy()


def test_frame_counts_cover_the_edges():
    """The arithmetic behind the module docstring: what the chosen frame counts put against the 256-position tile."""
    for name in mr.SMALL:
        mf = mr.min_frames(mr.CONFIGS[name])
        assert mr.FRAMES[name][:2] == (mf, mf + 1), name
    ends = lambda rate, name: {(f * rate + 128) % 256 - 128 for f in mr.FRAMES[name]}          # noqa: E731
    assert {-1, 0, 1, 2} <= ends(9, "S33") and {-1, 0, 1, 2} <= ends(3, "S33")
    assert {0, 2} <= ends(6, "TINY") | ends(2, "TINY")


@pytest.mark.parametrize("math", mr.MATHS)
@pytest.mark.parametrize("name", list(mr.SMALL))
def test_sweep_within_derived_bounds(name, math):
    _, model, mels = setup(name)
    g = engine(name, math)
    outs = g.inference_batch(mels)
    cout = mr.CONFIGS[name]["out_channels"]
    worst = {"whole": 0.0, "stage": 0.0, "conv": 0.0}
    for b, mel in enumerate(mels):
        out = host(outs[b]).T                                     # (out_channels, T' hop)
        assert out.shape == (cout, len(mel) * model.hop)
        stages = g.debug_stages(b)
        taps = g.debug_convs(b, with_output=True)
        np.testing.assert_array_equal(taps[-1], out)               # the output convolution's tap is the call's result
        taps = taps[:-1]
        ref = reference(name, b)
        whole = mr.global_ratio(ref, stages, out, math)
        per_stage = max(mr.local_ratio(model, mel, stages, out, math))
        per_conv = mr.conv_ratios(model, mel, taps, out, math)
        print(f"SWEEP-RATIO melgan {name} {math} frames={len(mel)}: whole-model={whole:.3g} per-stage={per_stage:.3g} "
              f"per-launch={max(per_conv):.3g} (launch {int(np.argmax(per_conv))}) "
              f"err/peak={np.abs(out - ref['out']).max() / np.abs(ref['out']).max():.3g}")
        worst = {"whole": max(worst["whole"], whole), "stage": max(worst["stage"], per_stage),
                 "conv": max(worst["conv"], max(per_conv))}
        np.testing.assert_array_equal(taps[-1], stages[-1])        # the last stack's x' is the last stage tap
    print(f"SWEEP-RATIO melgan {name} {math} worst: {worst}")
    assert worst["whole"] <= 1.0 and worst["stage"] <= 1.0 and worst["conv"] <= 1.0, worst


@pytest.mark.parametrize("name", ["TINY", "K5"])
def test_weight_norm_state_against_the_restatement(name):
    cfg = mr.CONFIGS[name]
    state = syn.melgan_state(cfg, seed=mr.SEEDS[name] + 50, weight_norm=True)
    assert "melgan.3.weight_g" in state and "melgan.3.weight" not in state
    model = mr.Model(cfg, state)
    mf = mr.min_frames(cfg)
    mels = mr.make_mels(name, (mf, 9))
    g = engine(name, "f16x3", state)
    outs = g.inference_batch(mels)
    for b, mel in enumerate(mels):
        out = host(outs[b]).T
        per_conv = mr.conv_ratios(model, mel, g.debug_convs(b), out, "f16x3")
        print(f"SWEEP-RATIO melgan {name} weight-norm state frames={len(mel)}: per-launch={max(per_conv):.3g}")
        assert max(per_conv) <= 1.0


@pytest.mark.parametrize("math", mr.MATHS)
@pytest.mark.parametrize("name", ["TINY", "MB-TINY", "S33"])
def test_same_bits_alone_in_any_batch_and_order(name, math):
    _, _, mels = setup(name)
    g = engine(name, math)
    if name == "MB-TINY":
        from parakeet_amd.melgan import PQMF
        g.set_pqmf(PQMF())                                        # through the bank as well
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
    mels = mr.make_mels("TINY", (11, 11))
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
    i32p = C.POINTER(C.c_int32)
    out = np.empty(22 * model.hop, np.float32)
    _capi.check(ctx.lib.pk_mgan_infer(g._h, _capi.fptr(flat), frames.ctypes.data_as(i32p), 2, _capi.fptr(out), _capi.PK_HOST_IO))
    np.testing.assert_array_equal(out, np.concatenate(want))
    with pytest.raises(ValueError):
        g.infer_packed(ctx.to_device(flat), [11, 11], noise=np.zeros(4))
    # a too-short utterance: PK_EINVAL naming min_frames, from the C side and as ValueError from Python
    lib = ctx.lib
    assert lib.pk_mgan_min_frames(g._h) == 4 == g.min_frames
    short = np.array([11, 3], np.int32)
    assert lib.pk_mgan_infer(g._h, _capi.fptr(flat), short.ctypes.data_as(i32p), 2, _capi.fptr(out), _capi.PK_HOST_IO) == -1
    assert b"min_frames = 4" in lib.pk_last_error()
    with pytest.raises(ValueError, match="min_frames"):
        g.inference(mels[0][:3])
    # the C side's own refusals and states
    h = C.c_void_p()
    for field, value in (("out_channels", 17), ("bias", 0), ("kernel_size", 4), ("stacks", 5), ("stack_kernel_size", 9),
                         ("channels", 24), ("in_channels", 0), ("n_upsample", 7)):
        cfg = g._cfg()
        setattr(cfg, field, value)
        assert lib.pk_mgan_create(ctx.handle, C.byref(cfg), C.byref(h)) == -3 and not h, field
    cfg = g._cfg()
    cfg.upsample_scales[0] = 17
    assert lib.pk_mgan_create(ctx.handle, C.byref(cfg), C.byref(h)) == -3
    assert lib.pk_mgan_set_math(g._h, _capi.PK_PWG_MATH_BF16X3) == -3 and lib.pk_mgan_set_math(g._h, 7) == -1
    g.inference(mels[0])
    buf = np.empty(4, np.float32)
    assert lib.pk_mgan_debug_read(g._h, 0, 0, _capi.fptr(buf), buf.size) == -2           # wrong size
    assert lib.pk_mgan_debug_read(g._h, 9, 0, _capi.fptr(buf), buf.size) == -1
    assert lib.pk_mgan_debug_conv(g._h, 99, 0, _capi.fptr(buf), buf.size) == -1
    assert lib.pk_mgan_infer(g._h, _capi.fptr(flat), frames.ctypes.data_as(i32p), 0, _capi.fptr(out), 1) == -1
    from parakeet_amd.melgan import PQMF
    q = PQMF()
    q._engine()
    assert lib.pk_mgan_set_pqmf(g._h, q._h) == -1                                          # 4 bands, 1 output channel


def test_normalize_equals_normalising_on_the_host():
    from parakeet_amd.melgan import MelGANInference
    from parakeet_amd.normalizer import ZScore
    _, _, mels = setup("TINY")
    rng = np.random.default_rng(4)
    mu = rng.normal(size=20).astype(np.float32)
    sigma = rng.uniform(0.5, 2.0, size=20).astype(np.float32)
    g = engine("TINY")
    voc = MelGANInference(ZScore(mu, sigma), g)
    raw = [(m * sigma + mu).astype(np.float32) for m in mels]
    on_host = [((r - mu) / sigma).astype(np.float32) for r in raw]
    want = g.inference_batch(on_host)
    got = g.inference_batch(raw, normalize=True)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(host(a), host(b))
    np.testing.assert_array_equal(host(voc(raw[3])), host(want[3]))
    np.testing.assert_array_equal(host(voc.inference_batch(raw)[2]), host(want[2]))


@pytest.mark.parametrize("math", mr.MATHS)
def test_bank_attached_equals_synthesis_of_the_subband_tap(math):
    """pk_mgan_infer with a bank attached writes synthesis(sub-bands): bit for bit the bank applied to the generator's own
    sub-band tap, which in turn is the call's result without a bank -- and within the bank's derived bound of the fp64
    synthesis of those sub-bands."""
    from parakeet_amd.melgan import PQMF, MelGANInference
    _, model, mels = setup("MB-TINY")
    g = engine("MB-TINY", math)
    sub = [host(o).T for o in g.inference_batch(mels)]            # (4, T' hop) each, no bank
    q = PQMF()
    voc = MelGANInference(None, g, q)
    assert g.upsample_factor == model.hop * 4 == 24
    full = [host(o)[:, 0] for o in g.inference_batch(mels)]
    _, syn_f = (f.astype(np.float64) for f in q.filters())
    for b, mel in enumerate(mels):
        assert full[b].shape == (len(mel) * 24,)
        tap = g.debug_convs(b, with_output=True)[-1]
        np.testing.assert_array_equal(tap, sub[b])
        np.testing.assert_array_equal(full[b], host(q.synthesis(tap)))
        want, bound = pr.synthesis(tap, syn_f)
        r = fb.ratio(full[b], want, bound)
        print(f"SWEEP-RATIO mb-melgan MB-TINY {math} frames={len(mel)}: synthesis of the sub-band tap={r:.3g}")
        assert r <= 1.0
    voc.pqmf = None
    voc.bind()
    np.testing.assert_array_equal(host(g.inference(mels[1])).T, sub[1])   # detached again


def test_synthesizer_fastspeech2_to_multiband_melgan():
    from parakeet_amd.fastspeech2 import FastSpeech2, FastSpeech2Inference
    from parakeet_amd.melgan import PQMF, MelGANGenerator, MelGANInference
    from parakeet_amd.normalizer import ZScore
    from parakeet_amd.synthesize import Synthesizer
    cfg = dict(syn.MB_MELGAN, channels=128)
    g = MelGANGenerator(**cfg)
    g.set_state_dict(syn.melgan_state(cfg, seed=21, weight_norm=True))
    g.eval()
    am = FastSpeech2(80, 80, **syn.FS2_LJSPEECH)
    am.set_state_dict(syn.fastspeech2_state(fixed_duration=2))
    am.eval()
    pmu, psd = syn.mel_stats(seed=6)
    voc = MelGANInference(ZScore(pmu, psd), g, PQMF())
    synth = Synthesizer(FastSpeech2Inference(ZScore(*syn.mel_stats(seed=5)), am), voc)
    assert synth.voc is g and synth.hop == 256
    texts = [syn.phoneme_ids(9, seed=3), syn.phoneme_ids(5, seed=4)]
    wav, frames = synth.synthesize_packed(texts)
    frames = [int(f) for f in frames]
    wav = host(wav)
    assert len(frames) == 2 and min(frames) >= g.min_frames and wav.shape == (sum(frames) * 256,) and np.isfinite(wav).all()
    mel = host(am.decode_packed(denormalize=True)).reshape(-1, 80)
    mels = [mel[:frames[0]], mel[frames[0]:frames[0] + frames[1]]]
    want = np.concatenate([host(o)[:, 0] for o in g.inference_batch(mels, normalize=True)])
    np.testing.assert_array_equal(wav, want)
    outs = synth.synthesize_batch(texts)
    np.testing.assert_array_equal(np.concatenate([host(o)[:, 0] for o in outs]), want)


@pytest.mark.parametrize("math", mr.MATHS)
@pytest.mark.parametrize("name", ["FULL", "MB-FULL"])
def test_full_width_two_by_forty_frames_against_fp64(name, math):
    """One full-width run of each family, 2 x 40 frames, against the same stack in float64 (torch on the device): MelGAN at
    512 channels; multi-band MelGAN at 384 channels and scales (8, 4, 2) with its PQMF (the oracle's bank is the fp64
    restatement on the engine's float32 filters).  The bar is the vocoders' north star of the README, the wav relative error
    1e-4; the measured figure is printed and recorded in DESIGN.md 4.1e."""
    from parakeet_amd.melgan import PQMF
    state, _, _ = setup(name)
    mels = mr.make_mels(name, (40, 40))
    g = engine(name, math)
    q = None
    if name == "MB-FULL":
        q = PQMF()
        g.set_pqmf(q)
        syn_f = q.filters()[1].astype(np.float64)
    outs = g.inference_batch(mels)
    dev = outs[0].device
    chain = mr.torch_chain(mr.CONFIGS[name], state, mels, device=dev)
    for b in range(2):
        want = chain[b][1]
        assert np.abs(want).max() < 0.95
        if q is not None:
            want = pr.synthesis(want, syn_f, with_bound=False)[0]
            assert np.abs(want).max() < 0.95
        else:
            want = want[0]
        got = host(outs[b])[:, 0]
        assert got.shape == (40 * 256,) == want.shape
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"SWEEP-RATIO melgan {name} {math} 40 frames: wav relative error {rel:.3g} (mean abs {np.abs(got - want).mean():.3g})")
        assert rel < NORTH_STAR
