"""GPU: the fused tail of the Parallel WaveGAN stack (pwg.hip, k_pwg_layer_b3's LAST instantiation; handle option "fused_tail").
On an unguarded, unsampled call of the planes path at hop 256 the last residual block computes the waveform itself: conv1x1_out, the
x_out planes, the store of the finished skip sum and the k_pwg_last_h3 launch are gone.  The tail follows k_pwg_last_h3 step for step,
so every comparison here is BIT FOR BIT against a handle with "fused_tail" = 0 -- the path that test_pwg_gpu.py,
test_pwg_skip_layout_gpu.py and test_benchshape_gpu.py hold against the fp64 oracle and the goldens; equality carries their bars over.

Synthetic weights, default math.  "scale_guard" = 0 makes the first call of a handle an unguarded one (a guarded call is never fused)."""
import numpy as np
import pytest

from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HOP = 256
CFG_8 = dict(syn.PWG_LJSPEECH, layers=8, stacks=1)      # dilations 1 .. 128: taps cross 32-sample blocks and utterance gaps
CFG_FULL = dict(syn.PWG_LJSPEECH)                       # 30 layers, 3 stacks: dilations to 512
FRAMES4 = (1, 3, 7, 2)


def _inputs(frames, seed, hop=HOP):
    rng = np.random.default_rng(seed)
    mels = [rng.normal(size=(L, 80)).astype(np.float32) for L in frames]
    noises = [rng.normal(size=(L * hop,)).astype(np.float32) for L in frames]
    return mels, noises


def _generator(cfg, state, pwg_math=None, **options):
    from parakeet_amd.parallel_wavegan import PWGGenerator
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(state)
    gen.eval()
    if pwg_math:
        gen.set_math(pwg_math)
    for k, v in options.items():
        gen.set_option(k, v)
    return gen


def _wavs(gen, mels, noises):
    return [o.cpu().numpy() for o in gen.inference_batch(mels, noises)]


def _profiled(gen, mels, noises):
    """(waveforms, {profile key: launches}) of one call."""
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        outs = _wavs(gen, mels, noises)
        counts = {k: n for k, (n, _) in ctx.prof_dump().items() if n > 0}   # (names of earlier tests stay registered with 0 launches)
    finally:
        ctx.prof_enable(False)
    return outs, counts


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("which", ["layers8", "full"])
def test_small_ragged_stack_is_bit_equal(which):
    """Frames (1, 3, 7, 2): edge classes of every kind, tiles whose taps reach into the gaps and across utterances' blocks.  The first
    call is fused (checked by its launches); the 7-frame utterance alone equals itself inside the batch."""
    cfg = CFG_8 if which == "layers8" else CFG_FULL
    state = syn.pwg_state(cfg, seed=21)
    mels, noises = _inputs(FRAMES4, 22)
    want = _wavs(_generator(cfg, state, scale_guard=0, fused_tail=0), mels, noises)
    fused = _generator(cfg, state, scale_guard=0)
    got, counts = _profiled(fused, mels, noises)
    assert "pwg_last_h3" not in counts and counts.get("pwg_layer_h3") == cfg["layers"], counts
    _assert_same(got, want)
    alone = _wavs(_generator(cfg, state, scale_guard=0), [mels[2]], [noises[2]])
    np.testing.assert_array_equal(alone[0], got[2])


def test_default_options_first_call_guarded_second_fused():
    cfg = CFG_8
    state = syn.pwg_state(cfg, seed=23)
    mels, noises = _inputs(FRAMES4, 24)
    ref = _generator(cfg, state, fused_tail=0)
    want = _wavs(ref, mels, noises)
    over_ref, fb_ref = ref.scale_overshoot()
    gen = _generator(cfg, state)
    first, c1 = _profiled(gen, mels, noises)
    over1, fb1 = gen.scale_overshoot()
    assert c1.get("pwg_last_h3") == 1 and c1.get("pwg_layer_h3") == cfg["layers"], c1      # guarded: the present code
    second, c2 = _profiled(gen, mels, noises)
    assert "pwg_last_h3" not in c2 and "pwg_last" not in c2 and c2.get("pwg_layer_h3") == cfg["layers"], c2
    _assert_same(first, want)
    _assert_same(second, want)
    assert over1.shape == (cfg["layers"] + 1,) and not fb1 and not fb_ref
    np.testing.assert_array_equal(over1, over_ref)
    over2, _ = gen.scale_overshoot()          # the fused call measured nothing: the report is still the guarded call's
    np.testing.assert_array_equal(over2, over_ref)


def test_debug_taps_after_a_fused_call_replay_the_ordinary_block():
    """Taps 1 (the final x_out) and 2 (the skip sum) after a fused call: the handle replays the ordinary last block once.  Two
    utterances, both orders of the taps, a tap read twice; the next inference must not see the replay's skip write."""
    cfg = CFG_8
    state = syn.pwg_state(cfg, seed=25)
    mels, noises = _inputs(FRAMES4, 26)
    ref = _generator(cfg, state, scale_guard=0, fused_tail=0)
    want = _wavs(ref, mels, noises)
    taps = {(w, b): ref.debug_tap(w, b) for w in (1, 2) for b in (1, 2)}
    gen = _generator(cfg, state, scale_guard=0)
    for order in ((1, 2), (2, 1)):
        got = _wavs(gen, mels, noises)
        _assert_same(got, want)
        for b in (1, 2):
            for w in order:
                np.testing.assert_array_equal(gen.debug_tap(w, b), taps[(w, b)])
        np.testing.assert_array_equal(gen.debug_tap(order[0], 2), taps[(order[0], 2)])     # read again: no second replay
    _assert_same(_wavs(gen, mels, noises), want)
    np.testing.assert_array_equal(gen.debug_tap(2, 1), taps[(2, 1)])


def test_loop_carried_state_over_one_and_two_tiles_per_wave():
    """Frames (200, 131) on the full configuration: 2 648 wave tiles on the 2 048 wave slots of 256 workgroups, so waves take one or two
    tiles and the last sweep is partial -- everything a wave carries from tile to tile (operand ring, offsets, scales, the prefetched
    rows) passes through the fused epilogue once."""
    cfg = CFG_FULL
    state = syn.pwg_state(cfg, seed=27)
    mels, noises = _inputs((200, 131), 28)
    want = _wavs(_generator(cfg, state, scale_guard=0, fused_tail=0), mels, noises)
    got, counts = _profiled(_generator(cfg, state, scale_guard=0), mels, noises)
    assert "pwg_last_h3" not in counts, counts
    _assert_same(got, want)


@pytest.mark.parametrize("case", ["planes0", "f32", "hop300"])
def test_fallbacks_launch_the_last_kernels_as_before(case):
    cfg = dict(CFG_8, upsample_scales=[4, 5, 3, 5]) if case == "hop300" else CFG_8
    hop = 300 if case == "hop300" else HOP
    state = syn.pwg_state(cfg, seed=29)
    mels, noises = _inputs((3, 2), 30, hop)
    opts = dict(scale_guard=0)
    if case == "planes0":
        opts["planes"] = 0
    pwg_math = "f32" if case == "f32" else None
    want = _wavs(_generator(cfg, state, pwg_math, fused_tail=0, **opts), mels, noises)
    got, counts = _profiled(_generator(cfg, state, pwg_math, **opts), mels, noises)
    last = "pwg_last" if case == "f32" else "pwg_last_h3"
    assert counts.get(last) == 1, counts
    _assert_same(got, want)
