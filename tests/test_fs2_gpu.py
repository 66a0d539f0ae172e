"""GPU parity: FastSpeech2 inference (HIP, through the C ABI) vs the CPU oracle.

Each utterance of a ragged batch is compared with an independent single-utterance
oracle call -- the only form of inference the reference defines
(fastspeech2.py:519-522).  Tolerance: north_star's mel L1 < 1e-4 and exactly equal
integer durations; max-abs is asserted too.
"""
import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MEL_L1_TOL = 1e-4      # BASELINE.json north_star
MEL_MAX_TOL = 2e-3     # max-abs bound on the same comparison (fp32 summation-order noise)


def _cfg(**over):
    return dict(syn.FS2_LJSPEECH, **over)


def _model_kwargs(cfg):
    return {k: v for k, v in cfg.items()}


def _oracle_cfg(cfg):
    keys = ("adim aheads elayers eunits dlayers dunits positionwise_conv_kernel_size "
            "duration_predictor_layers duration_predictor_chans duration_predictor_kernel_size "
            "pitch_predictor_layers pitch_predictor_chans pitch_predictor_kernel_size "
            "energy_predictor_layers energy_predictor_chans energy_predictor_kernel_size "
            "pitch_embed_kernel_size energy_embed_kernel_size postnet_layers postnet_chans postnet_filts").split()
    return {k: cfg[k] for k in keys}


def _check(cfg, tok_lens, seed, alpha=1.0, fixed_duration=None, taps=True, idim=80, odim=80, options=None):
    from oracle import fastspeech2_ref as ref
    from parakeet_amd.fastspeech2 import FastSpeech2

    state = syn.fastspeech2_state(idim, odim, cfg, seed=seed, fixed_duration=fixed_duration)
    texts = [syn.phoneme_ids(T, idim, seed=seed + 10 + i) for i, T in enumerate(tok_lens)]
    model = FastSpeech2(idim, odim, **_model_kwargs(cfg))
    model.set_state_dict(state)
    model.eval()
    model.set_debug(True)
    for k, v in (options or {}).items():
        model.set_option(k, v)
    outs = model.inference_batch(texts, alpha=alpha)
    for b, ids in enumerate(texts):
        want, parts = ref.inference(state, ids, _oracle_cfg(cfg), alpha=alpha, dtype=torch.float64,
                                    return_parts=True)
        want = want.numpy()
        d_ref = parts["d"].numpy()
        if alpha != 1.0:
            d_ref = np.sign(d_ref * alpha) * np.floor(np.abs(np.float32(d_ref) * np.float32(alpha)) + 0.5)
        if taps:
            hs = model.debug_tap(0, b)
            assert np.abs(hs - parts["hs"].numpy()).max() < 1e-3, "encoder output"
            assert np.abs(model.debug_tap(1, b) - parts["p"].numpy()).max() < 1e-3, "pitch"
            assert np.abs(model.debug_tap(2, b) - parts["e"].numpy()).max() < 1e-3, "energy"
        np.testing.assert_array_equal(model.debug_tap(3, b), d_ref)  # integer durations: exact
        got = outs[b].numpy()
        assert got.shape == want.shape, (got.shape, want.shape)
        if taps and got.shape[0]:
            assert np.abs(model.debug_tap(4, b) - parts["hs_up"].numpy()).max() < 1e-3, "length regulator"
            assert np.abs(model.debug_tap(5, b) - parts["zs"].numpy()).max() < 2e-3, "decoder output"
            assert np.abs(model.debug_tap(6, b) - parts["before"].numpy()).max() < 2e-3, "before_outs"
        if got.size:
            l1 = np.abs(got - want).mean()
            mx = np.abs(got - want).max()
            assert l1 < MEL_L1_TOL, f"utt {b}: mel L1 {l1}"
            assert mx < MEL_MAX_TOL, f"utt {b}: mel max-abs {mx}"


def test_fs2_ljspeech_ragged_batch():
    _check(_cfg(), [37, 5, 64, 1, 23], seed=100)


def test_fs2_ljspeech_fixed_duration_shape():
    # throughput configuration: every token -> 5 frames through the normal inference path
    _check(_cfg(), [16, 9], seed=101, fixed_duration=5)


def test_fs2_alpha_speed_control():
    _check(_cfg(), [21, 12], seed=102, alpha=1.3, taps=False)


def test_fs2_four_heads_small():
    # aheads=4 (d_k = 96), fewer layers, other kernel sizes
    cfg = _cfg(aheads=4, elayers=2, dlayers=2, eunits=512, dunits=512, positionwise_conv_kernel_size=1,
               pitch_predictor_layers=2, pitch_predictor_kernel_size=3, postnet_layers=3, postnet_chans=128)
    _check(cfg, [19, 40, 7], seed=103)


def test_fs2_long_utterance_multi_tile():
    # > 128 tokens and several hundred frames: several GEMM row tiles and attention key tiles
    _check(_cfg(), [150, 33], seed=104, taps=False)


def _rescaled_fs2_state(state, cfg, kf, kv, kq):
    """An equivalent model with rescaled internal streams (powers of two, exactly compensated): FFN hidden
    activations 2^kf (w_1 weight and bias up, w_2 weight down; ReLU commutes with a positive factor), attention
    values 2^kv (linear_v up, linear_out weight down), queries 2^kq with keys 2^-kq."""
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in state.items()}
    for stack, n in (("encoder", cfg["elayers"]), ("decoder", cfg["dlayers"])):
        for i in range(n):
            p = f"{stack}.encoders.{i}."
            out[p + "feed_forward.w_1.weight"] *= np.float32(2.0 ** kf)
            out[p + "feed_forward.w_1.bias"] *= np.float32(2.0 ** kf)
            out[p + "feed_forward.w_2.weight"] *= np.float32(2.0 ** -kf)
            out[p + "self_attn.linear_v.weight"] *= np.float32(2.0 ** kv)
            out[p + "self_attn.linear_v.bias"] *= np.float32(2.0 ** kv)
            out[p + "self_attn.linear_out.weight"] *= np.float32(2.0 ** -kv)
            out[p + "self_attn.linear_q.weight"] *= np.float32(2.0 ** kq)
            out[p + "self_attn.linear_q.bias"] *= np.float32(2.0 ** kq)
            out[p + "self_attn.linear_k.weight"] *= np.float32(2.0 ** -kq)
            out[p + "self_attn.linear_k.bias"] *= np.float32(2.0 ** -kq)
    return out


@pytest.mark.parametrize("kf,kv,kq", [(-10, 6, 8), (8, -12, -9), (-20, -20, 14)])
def test_fs2_split_math_is_scale_invariant(kf, kv, kq):
    """VERDICT r1 weak #2 for the FastSpeech2 kernels (split-fp16 GEMM and attention): rescaled-but-equivalent
    weights must give the original's output at the exact-fp32 path's error; durations stay bit-equal."""
    from oracle import fastspeech2_ref as ref
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = _cfg()
    state = syn.fastspeech2_state(80, 80, cfg, seed=140)
    ids = syn.phoneme_ids(45, 80, seed=141)
    want, parts = ref.inference(state, ids, _oracle_cfg(cfg), dtype=torch.float64, return_parts=True)
    want = want.numpy()
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(_rescaled_fs2_state(state, cfg, kf, kv, kq))
    model.eval()
    model.set_debug(True)
    l1 = {}
    for mode in ("f32", "f16x3"):
        model.set_math(mode)
        got = model.inference(ids).numpy()
        np.testing.assert_array_equal(model.debug_tap(3, 0), parts["d"].numpy())
        assert got.shape == want.shape
        l1[mode] = float(np.abs(got - want).mean())
    assert l1["f32"] < 2e-5, l1
    assert l1["f16x3"] < 2.0 * l1["f32"] + 5e-7, l1


def _planes_options(variant):
    """Run norm1 + q|k|v and norm2 + the feed-forward convs on the planes kernels (csrc/ffn_planes.hip) whatever the timeline
    length; variant: the "ffnp_variant" option of pk_fs2_set_option (first digit 8 / 4: 256 / 128 columns per wave in the first
    conv, second digit: waves per workgroup of the second), 0 = the launcher's own choice."""
    return {"ffn_planes": 1, "ffn_planes_min_blocks": 0, "ffnp_variant": variant}


@pytest.mark.parametrize("variant", [0, 88, 44])
def test_fs2_ffn_planes_kernels(variant):
    """The ragged batch of test_fs2_ljspeech_ragged_batch (gaps, 1-token utterances, tiles that straddle utterances, idle
    waves) under each first-conv / second-conv kernel variant: the same bars, internal taps included, and the profile shows
    that the planes kernels are what ran."""
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _check(_cfg(), [37, 5, 64, 1, 23], seed=100, options=_planes_options(variant))
        names = {k for k, (n, _) in ctx.prof_dump().items() if n > 0}
    finally:
        ctx.prof_enable(False)
    assert {"fs2_layernorm_planes", "fs2_gemm_qkv_planes", "fs2_gemm_attn_out_planes", "fs2_conv_ffn1_planes",
            "fs2_conv_ffn2_planes", "fs2_rows_to_planes", "fs2_conv_predictor_planes", "fs2_conv_postnet_planes"} <= names, names
    # (round 4: the predictors' convs and the postnet's middle layers run the planes kernel too; what stays on the tile GEMM
    # is the postnet's first and last layer)
    assert "fs2_conv_predictor_h3" not in names and "fs2_conv_predictor" not in names, names
    assert not any(n.startswith(("fs2_conv_ffn", "fs2_gemm_qkv", "fs2_gemm_attn_out")) and "planes" not in n for n in names), names


def test_fs2_tile_gemm_path_still_meets_the_bars():
    """Option "ffn_planes" = 0: every dense layer on the tile GEMM (rounds 1 - 2's path, and the path of shapes the planes kernels
    are not instantiated for): same bars, internal taps included, and none of the planes kernels runs."""
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _check(_cfg(), [37, 5, 64, 1, 23], seed=100, options={"ffn_planes": 0})
        names = {k for k, (n, _) in ctx.prof_dump().items() if n > 0}
    finally:
        ctx.prof_enable(False)
    assert not any("planes" in n for n in names), names


def test_fs2_batch_composition_invariance():
    """An utterance's mel does not depend on the batch it is in, bit for bit -- alone, in a ragged batch, in the reversed
    batch -- nor on which of the first-conv kernels runs (the "ffnp_variant" option: they differ in tiling only).  The planes
    kernels keep one scale per ROW for this (a per-block scale would couple neighbouring utterances), and one weight scale per 32
    output channels whatever the tile width."""
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = _cfg()
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(syn.fastspeech2_state(80, 80, cfg, seed=150))
    model.eval()
    texts = [syn.phoneme_ids(T, 80, seed=151 + i) for i, T in enumerate([37, 5, 64, 1, 23])]
    ref = [o.as_subclass(torch.Tensor).clone() for o in model.inference_batch(texts)]
    rev = model.inference_batch(texts[::-1])
    for b in range(len(texts)):
        assert torch.equal(ref[b], rev[len(texts) - 1 - b].as_subclass(torch.Tensor)), b
    solo = model.inference_batch([texts[2]])[0].as_subclass(torch.Tensor)
    assert torch.equal(ref[2], solo)
    for variant in (88, 84, 48, 44):
        model.set_option("ffnp_variant", variant)
        out = model.inference_batch(texts)
        for b in range(len(texts)):
            assert torch.equal(ref[b], out[b].as_subclass(torch.Tensor)), (variant, b)
    # ... nor on the one-tile-per-wave kernels of short timelines ("ffn_one_tile_max": the default runs them here, 0 never does,
    # the forced variants above never do either)
    model.set_option("ffnp_variant", 0)
    for one_max in (0, 1 << 20):
        model.set_option("ffn_one_tile_max", one_max)
        out = model.inference_batch(texts)
        for b in range(len(texts)):
            assert torch.equal(ref[b], out[b].as_subclass(torch.Tensor)), (one_max, b)


def test_fs2_ffn_planes_long_utterance():
    _check(_cfg(), [150, 33], seed=104, taps=False, options=_planes_options(0))


@pytest.mark.parametrize("kf", [-20, 8])
def test_fs2_ffn_planes_scale_invariant(kf):
    """The hidden activations are stored with the scale of a magnitude BOUND: a model whose hidden stream is rescaled by 2^kf
    (exactly compensated) must give the original's output at the exact-fp32 path's error."""
    from oracle import fastspeech2_ref as ref
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = _cfg()
    state = syn.fastspeech2_state(80, 80, cfg, seed=140)
    ids = syn.phoneme_ids(45, 80, seed=141)
    want, parts = ref.inference(state, ids, _oracle_cfg(cfg), dtype=torch.float64, return_parts=True)
    want = want.numpy()
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(_rescaled_fs2_state(state, cfg, kf, 0, 0))
    model.eval()
    model.set_debug(True)
    for k, v in _planes_options(0).items():
        model.set_option(k, v)
    l1 = {}
    for mode in ("f32", "f16x3"):
        model.set_math(mode)
        got = model.inference(ids).numpy()
        np.testing.assert_array_equal(model.debug_tap(3, 0), parts["d"].numpy())
        l1[mode] = float(np.abs(got - want).mean())
    assert l1["f32"] < 2e-5, l1
    assert l1["f16x3"] < 2.0 * l1["f32"] + 5e-7, l1


def test_fs2_inference_wrapper_denormalizes():
    from oracle import fastspeech2_ref as ref
    from parakeet_amd.fastspeech2 import FastSpeech2, FastSpeech2Inference
    from parakeet_amd.normalizer import ZScore
    cfg = _cfg()
    state = syn.fastspeech2_state(80, 80, cfg, seed=105)
    mu, sigma = syn.mel_stats()
    ids = syn.phoneme_ids(30, 80, seed=3)
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(state)
    model.eval()
    inf = FastSpeech2Inference(ZScore(mu, sigma), model)
    got = inf(ids).numpy()
    want = ref.fastspeech2_inference(state, mu, sigma, ids, _oracle_cfg(cfg), dtype=torch.float64).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).mean() < MEL_L1_TOL
    # wrapping does not change the model's own inference(): it stays in the normalised domain like the
    # reference's (fastspeech2.py:468-558); two wrappers with different statistics around one model coexist
    plain = model.inference(ids).numpy()
    want_plain = ref.inference(state, ids, _oracle_cfg(cfg), dtype=torch.float64).numpy()
    assert np.abs(plain - want_plain).mean() < MEL_L1_TOL
    inf2 = FastSpeech2Inference(ZScore(mu + 1.0, sigma * 2.0), model)
    want2 = ref.fastspeech2_inference(state, mu + 1.0, sigma * 2.0, ids, _oracle_cfg(cfg), dtype=torch.float64).numpy()
    assert np.abs(inf2(ids).numpy() - want2).mean() < MEL_L1_TOL
    assert np.abs(inf(ids).numpy() - want).mean() < MEL_L1_TOL


def test_fs2_error_mapping():
    from parakeet_amd.fastspeech2 import FastSpeech2
    with pytest.raises(ValueError):
        FastSpeech2(80, 80, encoder_type="conformer")
    with pytest.raises(NotImplementedError):
        FastSpeech2(80, 80, **_cfg(reduction_factor=32))            # 1 .. 16
    m = FastSpeech2(80, 80, **_cfg())
    with pytest.raises(RuntimeError):
        m.inference(np.array([1, 2, 3]))            # parameters never set
    m.set_state_dict(syn.fastspeech2_state(80, 80, _cfg()))
    with pytest.raises(ValueError):
        m.inference(np.array([1, 2, 999]))          # id out of range
    with pytest.raises(AssertionError):
        m.inference(np.array([1, 2, 3]), alpha=0.0)  # assert alpha > 0 (length_regulator.py:86)


def _cancelling_values_state(cfg, seed, gain):
    """A model whose attention contexts are far below the bound the engine scales them by (|ctx| <= max|v|): two tokens with
    embeddings +gain u and -gain u alternate, every linear_k is zero (uniform attention), so the values of an utterance alternate
    in sign at full magnitude and their mean -- the context -- is what the positional encoding leaves: a factor ~gain smaller."""
    st = {k: np.array(v, dtype=np.float32, copy=True)
          for k, v in syn.fastspeech2_state(80, 80, cfg, seed=seed, fixed_duration=5).items()}
    rng = np.random.default_rng(seed + 1)
    u = rng.standard_normal(cfg["adim"]).astype(np.float32)
    u /= np.linalg.norm(u) / np.sqrt(cfg["adim"])
    st["encoder.embed.0.weight"][1] = gain * u
    st["encoder.embed.0.weight"][2] = -gain * u
    for stack, n in (("encoder", cfg["elayers"]), ("decoder", cfg["dlayers"])):
        for i in range(n):
            st[f"{stack}.encoders.{i}.self_attn.linear_k.weight"][:] = 0
            st[f"{stack}.encoders.{i}.self_attn.linear_k.bias"][:] = 0
            st[f"{stack}.encoders.{i}.self_attn.linear_v.bias"][:] = 0     # (constant terms of v would not cancel)
            st[f"{stack}.encoders.{i}.norm1.bias"][:] = 0
    return st


def _context_overshoot(state, cfg, ids):
    """max|v| / max|context| of encoder layer 0 under uniform attention, in fp64 (what the engine's bound is loose by)."""
    A = cfg["adim"]
    emb = torch.tensor(state["encoder.embed.0.weight"], dtype=torch.float64)[torch.as_tensor(ids)]
    pos = torch.arange(len(ids), dtype=torch.float64)[:, None]
    div = torch.exp(torch.arange(0, A, 2, dtype=torch.float64) * -(np.log(10000.0) / A))
    pe = torch.zeros(len(ids), A, dtype=torch.float64)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    x = emb + float(state["encoder.embed.1.alpha"][0]) * pe
    p = "encoder.encoders.0."
    xn = torch.nn.functional.layer_norm(x, (A,), torch.tensor(state[p + "norm1.weight"], dtype=torch.float64),
                                        torch.tensor(state[p + "norm1.bias"], dtype=torch.float64), 1e-12)
    v = xn @ torch.tensor(state[p + "self_attn.linear_v.weight"], dtype=torch.float64) + torch.tensor(state[p + "self_attn.linear_v.bias"], dtype=torch.float64)
    ctx = v.mean(0)
    return float(v.abs().max() / ctx.abs().max())


@pytest.mark.parametrize("gain", [16.0, 1024.0])
def test_fs2_cancelling_values_under_uniform_attention(gain):
    """VERDICT r3 #2, second half: the row scales of the split-fp16 path come from magnitude BOUNDS (|ctx| <= max|v| for the
    attention context, c1 max|x| + c0 for a layer's output), and a value far below its bound loses bits.  Hostile case for the
    context bound: values that cancel under uniform attention (overshoot ~ gain).  The bounds are per row and per layer -- not
    cumulative -- and the exact-fp32 evaluation of a cancelling sum has an absolute error relative to the SAME magnitude, so the
    split path must stay at the exact path's error: 2 x + 5e-7 against the fp64 oracle, durations bit-equal."""
    from oracle import fastspeech2_ref as ref
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = _cfg()
    state = _cancelling_values_state(cfg, 170, gain)
    ids = np.array([1, 2] * 32, dtype=np.int64)
    assert _context_overshoot(state, cfg, ids) > 0.25 * gain      # (the construction does what it says: the bound is loose by ~gain)
    want, parts = ref.inference(state, ids, _oracle_cfg(cfg), dtype=torch.float64, return_parts=True)
    want = want.numpy()
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(state)
    model.eval()
    model.set_debug(True)
    l1 = {}
    for mode in ("f32", "f16x3"):
        model.set_math(mode)
        got = model.inference(ids).numpy()
        np.testing.assert_array_equal(model.debug_tap(3, 0), parts["d"].numpy())
        assert got.shape == want.shape
        l1[mode] = float(np.abs(got - want).mean())
    assert l1["f32"] < 2e-5, l1
    assert l1["f16x3"] < 2.0 * l1["f32"] + 5e-7, l1
