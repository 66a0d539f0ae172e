"""GPU: the split PWG kernels keep the skip sum in accumulator order (pwg.hip, PK_PWG_SKIP_VEC: per 32-sample block
[channel quad 16][sample 32][4 channels], one 16-byte vector per lane and register quad).  Where a value is stored is all that
changed, so these tests aim at indexing: the decoded skip tap against the fp32-x path and the fp64 oracle (a wrong channel
permutation or block offset is an error of order 1), a dilation that carries a tile's taps across blocks and utterance gaps, one
utterance alone against the same utterance inside a batch (bit for bit), and the scale guard's second attempt, which runs the
other kernel family's instantiations over the buffer the first attempt filled.

Synthetic weights, hop 256, default math.  Every bar is the bar of the test in test_pwg_gpu.py named next to it."""
import functools
import math

import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HOP = 256
OKEYS = ("layers", "stacks", "kernel_size", "aux_context_window", "upsample_scales")
CFG_6 = dict(syn.PWG_LJSPEECH, layers=6, stacks=2)      # dilations 1, 2, 4 twice
CFG_8 = dict(syn.PWG_LJSPEECH, layers=8, stacks=1)      # dilations 1 .. 128: taps cross 32-sample blocks and utterance gaps
FRAMES3 = (1, 3, 7)
FRAMES4 = (1, 3, 7, 2)


def _rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _inputs(frames, seed):
    rng = np.random.default_rng(seed)
    mels = [rng.normal(size=(L, 80)).astype(np.float32) for L in frames]
    noises = [rng.normal(size=(L * HOP,)).astype(np.float32) for L in frames]
    return mels, noises


def _generator(cfg, state, pwg_math="f16x3", options=None):
    from parakeet_amd.parallel_wavegan import PWGGenerator
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(state)
    gen.eval()
    gen.set_math(pwg_math)
    for k, v in (options or {}).items():
        gen.set_option(k, v)
    return gen


@functools.lru_cache(maxsize=None)
def _oracle(which, frames, seed_state, seed_in):
    """fp64 oracle of (waveform, skips) per utterance, computed once per configuration."""
    from oracle import pwg_ref
    cfg = {"6": CFG_6, "8": CFG_8}[which]
    state = syn.pwg_state(cfg, seed=seed_state)
    mels, noises = _inputs(frames, seed_in)
    ocfg = {k: cfg[k] for k in OKEYS}
    out = []
    for mel, noise in zip(mels, noises):
        c = torch.from_numpy(mel).transpose(0, 1).unsqueeze(0)
        c = torch.nn.functional.pad(c, (cfg["aux_context_window"],) * 2, mode="replicate")
        ref, parts = pwg_ref.generator_forward(state, torch.from_numpy(noise).reshape(1, 1, -1), c, ocfg, torch.float64,
                                               return_parts=True)
        out.append((ref[0, 0].numpy(), parts["skips"][0].numpy()))
    return out


def test_skip_tap_matches_the_fp32_x_path_and_the_oracle():
    """Bar: test_pwg_fp32_x_path_meets_the_same_bars (option "planes" = 0; its skip tap bar is 1e-4 relative).  The same bar holds
    against the oracle's skips, so a decode that is wrong on both paths alike cannot pass either."""
    state = syn.pwg_state(CFG_6, seed=11)
    mels, noises = _inputs(FRAMES3, 12)
    planes = _generator(CFG_6, state)
    fp32x = _generator(CFG_6, state, options={"planes": 0})
    planes.inference_batch(mels, noises)
    fp32x.inference_batch(mels, noises)
    refs = _oracle("6", FRAMES3, 11, 12)
    for b, L in enumerate(FRAMES3):
        got = planes.debug_tap(2, b)
        want = fp32x.debug_tap(2, b)
        assert got.shape == want.shape == (64, L * HOP)
        err = _rel_err(got, want)
        err_o = _rel_err(got * math.sqrt(1.0 / CFG_6["layers"]), refs[b][1])
        print(f"utt {b}: skip tap planes vs fp32-x {err:.3e}, vs oracle {err_o:.3e}")
        assert err < 1e-4, f"utt {b}: skip tap, planes path vs fp32-x path {err}"
        assert err_o < 1e-4, f"utt {b}: skip tap vs oracle {err_o}"


def test_waveform_with_dilations_up_to_128():
    """Bar: test_pwg_small_stack_ragged (waveform 1e-4 relative against the fp64 oracle)."""
    state = syn.pwg_state(CFG_8, seed=13)
    mels, noises = _inputs(FRAMES4, 14)
    outs = _generator(CFG_8, state).inference_batch(mels, noises)
    refs = _oracle("8", FRAMES4, 13, 14)
    for b in range(len(FRAMES4)):
        got = outs[b].cpu().numpy()[:, 0]
        assert got.shape == refs[b][0].shape
        err = _rel_err(got, refs[b][0])
        print(f"utt {b}: wav {err:.3e}")
        assert err < 1e-4, f"utt {b}: wav rel err {err}"


def test_single_utterance_equals_the_same_utterance_in_a_batch():
    """Indexing must not depend on where a tile sits in the timeline: the 7-frame utterance alone and as the third of four,
    waveform and skip tap bit for bit."""
    state = syn.pwg_state(CFG_8, seed=13)
    mels, noises = _inputs(FRAMES4, 14)
    b = 2
    batch = _generator(CFG_8, state)
    wav_batch = batch.inference_batch(mels, noises)[b].cpu().numpy()
    tap_batch = batch.debug_tap(2, b)
    alone = _generator(CFG_8, state)
    wav_alone = alone.inference_batch([mels[b]], [noises[b]])[0].cpu().numpy()
    tap_alone = alone.debug_tap(2, 0)
    np.testing.assert_array_equal(wav_alone, wav_batch)
    np.testing.assert_array_equal(tap_alone, tap_batch)


def _cancelling_state(cfg, seed, gain, eps):
    """The generator of test_pwg_scale_guard_on_cancelling_weights (test_pwg_gpu.py, _cancelling_state with paired conditioning
    rows): identical gate-channel pairs and conv1x1_out columns that cancel pairwise, so the residual stream stays far below the
    a-priori bound the planes path scales it by."""
    st = {k: np.array(v, dtype=np.float32, copy=True) for k, v in syn.pwg_state(cfg, seed=seed).items()}
    rng = np.random.default_rng(seed + 1000)
    for i in range(cfg["layers"]):
        p = f"conv_layers.{i}."
        for name in ("conv.weight", "conv.bias", "conv1x1_aux.weight"):
            w = st[p + name]
            for half in (0, 64):
                w[half + 1:half + 64:2] = w[half:half + 64:2]
        wo = st[p + "conv1x1_out.weight"]
        base = (rng.uniform(-1, 1, size=(64, 32)) * gain / 8).astype(np.float32)
        e = (eps * rng.uniform(0.5, 1.0, size=(1, 32))).astype(np.float32)
        wo[:, 0::2, 0] = base
        wo[:, 1::2, 0] = -(1 - e) * base
        st[p + "conv1x1_out.bias"] *= np.float32(eps)
    return st


def test_scale_guard_fallback_runs_over_the_buffer_of_the_planes_attempt():
    """Weights and eps of the expect_fallback case of test_pwg_scale_guard_on_cancelling_weights, cut to 6 layers: the guarded first
    call runs the planes kernels, finds the overshoot and repeats the stack on the fp32-x kernels over the same skip buffer.
    Bar: that test's (the split path as close to the fp64 oracle as the exact-fp32 path)."""
    from oracle import pwg_ref
    cfg = dict(syn.PWG_LJSPEECH, layers=6, stacks=3)
    state = _cancelling_state(cfg, 77, 64.0, 2.0 ** -10)
    rng = np.random.default_rng(78)
    frames = [6, 3]
    mels = [rng.normal(size=(L, 80)).astype(np.float32) for L in frames]
    noises = [rng.normal(size=(L * HOP,)).astype(np.float32) for L in frames]
    ocfg = {k: cfg[k] for k in OKEYS}
    refs = [pwg_ref.generator_inference(state, torch.from_numpy(m), torch.from_numpy(n), ocfg, dtype=torch.float64)[:, 0].numpy()
            for m, n in zip(mels, noises)]
    errs = {}
    for mode in ("f32", "f16x3"):
        gen = _generator(cfg, state, pwg_math=mode)
        outs = gen.inference_batch(mels, noises)
        errs[mode] = max(_rel_err(o.cpu().numpy()[:, 0], r) for o, r in zip(outs, refs))
        if mode == "f16x3":
            over, fell_back = gen.scale_overshoot()
            print("overshoot", over, "fell back", fell_back)
            assert fell_back, over       # otherwise this test runs one path only
            again = gen.inference_batch(mels, noises)
            for a, o in zip(again, outs):
                np.testing.assert_array_equal(a.cpu().numpy(), o.cpu().numpy())
    print("errs", errs)
    assert errs["f32"] < 1e-4, errs
    assert errs["f16x3"] < 2.0 * errs["f32"] + 2e-7, errs
