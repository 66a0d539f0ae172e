"""GPU: the conditioning filter of the Parallel WaveGAN layer kernel on the fp32 matrix pipe (pwg.hip, PK_PWG_AUX_MFMA: the accumulator
init of k_pwg_layer_b3 at hop 256 as twelve v_mfma_f32_32x32x2_f32 -- the five staged P rows and the bias are the A operand, the
lane's upsampler weights the B operand).  The sum is formed in another order than the vector filter's, so nothing here is compared
with an earlier build: every case is held against the fp64 oracle (oracle/pwg_ref) at the bars tests/test_pwg_gpu.py holds this
path to (_run_case: waveform, final residual stream and skip sum 1e-4 of the reference's maximum), and the paths that must agree
with each other do so bit for bit.

Synthetic weights, default math.  A handle's first call is the guarded one (AMAX instantiations, k_pwg_last_h3), its second the
noise-fed first block + ordinary blocks + fused tail: both are checked."""
import math

import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn
from test_pwg_gpu import _cancelling_state, _rel_err

pytestmark = pytest.mark.gpu

HOP = 256
BAR = 1e-4                                              # test_pwg_gpu._run_case: wav, x_last (tap 1) and skips (tap 2)
CFG_8 = dict(syn.PWG_LJSPEECH, layers=8, stacks=1)      # dilations 1 .. 128
EDGE_FRAMES = (1, 2, 3, 4, 5, 6)                        # one frame: first and last at once; 2 - 4: second / second-last next to the ends


def _inputs(frames, seed, hop=HOP):
    rng = np.random.default_rng(seed)
    mels = [rng.normal(size=(L, 80)).astype(np.float32) for L in frames]
    noises = [rng.normal(size=(L * hop,)).astype(np.float32) for L in frames]
    return mels, noises


def _generator(cfg, state, **options):
    from parakeet_amd.parallel_wavegan import PWGGenerator
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(state)
    gen.eval()
    for k, v in options.items():
        gen.set_option(k, v)
    return gen


def _wavs(gen, mels, noises):
    return [o.cpu().numpy() for o in gen.inference_batch(mels, noises)]


def _oracle(cfg, state, mels, noises):
    """[(wav, x_last, skips)] per utterance, float64."""
    from oracle import pwg_ref
    ocfg = {k: cfg[k] for k in ("layers", "stacks", "kernel_size", "aux_context_window", "upsample_scales")}
    out = []
    for mel, noise in zip(mels, noises):
        c = torch.from_numpy(mel).transpose(0, 1).unsqueeze(0)
        c = torch.nn.functional.pad(c, (cfg["aux_context_window"],) * 2, mode="replicate")
        ref, parts = pwg_ref.generator_forward(state, torch.from_numpy(noise).reshape(1, 1, -1), c, ocfg, torch.float64,
                                               return_parts=True)
        out.append((ref[0, 0].numpy(), parts["x_last"][0].numpy(), parts["skips"][0].numpy()))
    return out


def _check_against_oracle(cfg, state, mels, noises, label):
    refs = _oracle(cfg, state, mels, noises)
    gen = _generator(cfg, state)
    first = _wavs(gen, mels, noises)        # guarded: AMAX instantiations
    second = _wavs(gen, mels, noises)       # noise-fed first block, ordinary blocks, fused tail
    over, fell_back = gen.scale_overshoot()
    assert not fell_back, over              # (the cases here stay on the planes path: it is the path under test)
    worst = 0.0
    for b, (wav, x_last, skips) in enumerate(refs):
        e1, e2 = _rel_err(first[b][:, 0], wav), _rel_err(second[b][:, 0], wav)
        ex = _rel_err(gen.debug_tap(1, b), x_last)
        es = _rel_err(gen.debug_tap(2, b) * math.sqrt(1.0 / cfg["layers"]), skips)
        print(f"{label}: utt {b} ({mels[b].shape[0]} frames)  wav {e1:.3g} (guarded) {e2:.3g} (fused)  x_last {ex:.3g}  skips {es:.3g}")
        worst = max(worst, e1, e2, ex, es)
        assert e1 < BAR and e2 < BAR, f"utt {b}: wav rel err {e1} / {e2}"
        assert ex < BAR, f"utt {b}: x_last rel err {ex}"
        assert es < BAR, f"utt {b}: skips rel err {es}"
    return worst


def test_every_edge_class_and_tap_pairing():
    """Utterances of 1 .. 6 frames in one batch: every edge class of the composite upsampler, so every pairing of a tap with a
    staged P row (rows before the first / behind the last frame included)."""
    state = syn.pwg_state(CFG_8, seed=31)
    mels, noises = _inputs(EDGE_FRAMES, 32)
    _check_against_oracle(CFG_8, state, mels, noises, "edges")


def test_conditioning_alone_feeds_the_gate():
    """Every block's dilated conv is zero: the pre-activation is bias + filter alone, the new code is all there is between the mel
    and the gate."""
    state = {k: np.array(v, copy=True) for k, v in syn.pwg_state(CFG_8, seed=33).items()}
    for i in range(CFG_8["layers"]):
        state[f"conv_layers.{i}.conv.weight"][...] = 0.0
    mels, noises = _inputs(EDGE_FRAMES, 34)
    _check_against_oracle(CFG_8, state, mels, noises, "conditioning only")


def test_neighbouring_rows_orders_of_magnitude_apart():
    """Mel frames scaled by 2^8, 2^-8, 2^8, ...: the five P rows of one tile differ by orders of magnitude."""
    state = syn.pwg_state(CFG_8, seed=35)
    mels, noises = _inputs(EDGE_FRAMES, 36)
    for m in mels:
        m *= np.where(np.arange(m.shape[0]) % 2 == 0, 2.0 ** 8, 2.0 ** -8).astype(np.float32)[:, None]
    _check_against_oracle(CFG_8, state, mels, noises, "scales")


def test_an_utterance_is_independent_of_its_batch():
    state = syn.pwg_state(CFG_8, seed=37)
    mels, noises = _inputs((1, 3, 7, 2), 38)
    for opts in (dict(), dict(scale_guard=0)):      # guarded first call; unguarded: noise-fed first block and fused tail
        batch = _wavs(_generator(CFG_8, state, **opts), mels, noises)
        alone = _wavs(_generator(CFG_8, state, **opts), [mels[2]], [noises[2]])
        np.testing.assert_array_equal(alone[0], batch[2])


def test_scale_guard_fallback_equals_planes_0():
    """Cancelling weights (test_pwg_gpu._cancelling_state) over 30 layers: the guarded call falls back to the fp32-x path.  That is
    the path of "planes" = 0: the two handles run the same kernels, the filter included, and agree bit for bit."""
    cfg = dict(syn.PWG_LJSPEECH, layers=30, stacks=3)
    state = _cancelling_state(cfg, 77, 64.0, 2.0 ** -10)
    mels, noises = _inputs((6, 3), 78)
    gen = _generator(cfg, state)
    got = _wavs(gen, mels, noises)
    _, fell_back = gen.scale_overshoot()
    assert fell_back
    want = _wavs(_generator(cfg, state, planes=0), mels, noises)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_hop_300_keeps_the_vector_filter_and_its_bar():
    """upsample_scales [4, 5, 3, 5]: a wave tile can straddle two frames, these instantiations keep the vector filter."""
    cfg = dict(CFG_8, upsample_scales=[4, 5, 3, 5])
    state = syn.pwg_state(cfg, seed=39)
    mels, noises = _inputs((3, 2), 40, hop=300)
    _check_against_oracle(cfg, state, mels, noises, "hop 300")
