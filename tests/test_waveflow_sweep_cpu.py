"""CPU twin of tests/test_waveflow_sweep_gpu.py: the case table holds together, the bars leave room for an fp32 evaluation, the cases
can tell a subtly wrong engine from a right one, and the upsampler's a-priori bound is sound.  No GPU, no engine code: the oracle in
float64 and float32 and deliberately wrong restatements of it."""
import numpy as np
import pytest
import torch

import fp32_bounds as fb
import waveflow_cases as wc
from oracle import waveflow_ref as ref
from oracle.nn_ref import Weights, fold_weight_norm

NAMES = [c.name for c in wc.CASES]


# ---------------------------------------------------------------- 1. the table
def test_table_covers_every_family_the_engine_admits():
    groups = {c.group for c in wc.CASES}
    assert groups == {"fused_width", "n_group", "unfused_width", "unfused_n_mels", "upsample"}
    cfgs = [wc.cfg_of(c) for c in wc.CASES]
    assert {c["channels"] for c in cfgs} == {64, 128, 192, 256}
    assert {c["n_group"] for c in cfgs} == {8, 16, 32, 64, 128}                      # every key of Flow.dilations_dict
    assert {c["n_mels"] for c in cfgs} >= {16, 48, 64, 80, 112, 128, 176, 256}
    assert {wc.mp_of(c["n_mels"]) for c in cfgs} == {32, 64, 96, 128, 192, 256}           # every padding class of the condition block
    assert max(c["n_mels"] for c in cfgs) == wc.MAX_N_MELS
    stacks = {tuple(c["upsample_factors"]) for c in cfgs}
    assert stacks >= {(2,), (64,), (2, 2, 2, 2), (8, 4, 2), (2, 64), (64, 2), (4, 4), (16, 16)}
    assert {len(s) for s in stacks} == {1, 2, 3, 4}
    assert any(c.fused and c.group == "upsample" for c in wc.CASES)
    assert any(wc.cfg_of(c)["n_mels"] == 256 and c.group == "upsample" for c in wc.CASES)
    assert any(wc.cfg_of(c)["n_flows"] == 4 and c.group == "fused_width" for c in wc.CASES)
    for c in wc.CASES:
        cfg = wc.cfg_of(c)
        # the table's own consistency only (a typo in ``fused``): that the engine takes the fused kernel exactly for these is what
        # the GPU sweep's kernel-family assertion checks, case by case
        assert c.fused == (cfg["channels"] in (64, 128) and 64 < cfg["n_mels"] < 96), c.name
        assert ("f16" in c.maths) <= c.fused, c.name                                   # the fp16-operand mode lives on the fused kernel
        assert set(c.dirs) <= {"infer", "forward"} and "infer" in c.dirs
        assert not c.waves or cfg["channels"] == 64
    fused_fw = {c.name for c in wc.CASES if c.group == "fused_width"}
    assert any(wc.BY_NAME[n].waves == (8, 12, 6) for n in fused_fw)
    for ch in (192, 256):
        assert any(wc.cfg_of(c)["channels"] == ch and set(c.maths) == {"f32", "f16x3"} and set(c.dirs) == {"infer", "forward"}
                   for c in wc.CASES)
    for g in groups:                                                                   # every group also runs forward
        assert any(c.group == g and "forward" in c.dirs for c in wc.CASES), g


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_and_has_the_widths_it_claims(name):
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    state, mels, zs, audios = wc.inputs(name)
    W = Weights(fold_weight_norm(state), torch.float64)
    got_w = []
    for b, T in enumerate(case.frames):
        clen, pruned = wc.lengths(cfg, T)
        with torch.no_grad():
            up = ref.upsample(W.sub("encoder."), torch.from_numpy(mels[b])[None].double(), cfg["upsample_factors"], trim=True)
            full = ref.upsample(W.sub("encoder."), torch.from_numpy(mels[b])[None].double(), cfg["upsample_factors"], trim=False)
        assert up.shape == (1, cfg["n_mels"], clen) == (1, cfg["n_mels"], len(zs[b]))   # the length arithmetic is the oracle's
        assert full.shape[-1] == T * wc.hop(cfg)
        assert pruned >= cfg["n_group"], f"utterance {b} has no position"
        got_w.append(pruned // cfg["n_group"])
        n = len(audios[b])                                                             # forward: same width, ragged tail
        assert cfg["n_group"] <= n <= T * wc.hop(cfg) and (T * wc.hop(cfg) - n) % cfg["n_group"] != 0
        assert n // cfg["n_group"] == got_w[-1]
    assert tuple(got_w) == case.widths == wc.widths(case)
    if case.group == "fused_width":
        assert all(wc.lengths(cfg, T)[0] - wc.lengths(cfg, T)[1] == 12 for T in case.frames)
    if case.group in ("fused_width", "n_group", "upsample") and name != "ng8_f16x16":
        assert min(got_w) < 32 and (32 in got_w or 64 in got_w or 128 in got_w or case.group == "upsample") and max(got_w) > 32
    if name == "ng8_f16x16":
        assert got_w == [30, 62, 94]


def test_width_edges_of_the_fused_group():
    a, b = wc.BY_NAME["fw_c64_a"], wc.BY_NAME["fw_c64_b_4flows"]
    assert set(wc.widths(a)) | set(wc.widths(b)) == {1, 2, 31, 32, 33, 63, 64, 127, 128, 129}


# ---------------------------------------------------------------- 2. the bars leave room
@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_is_inside_the_bars(name):
    case = wc.BY_NAME[name]
    worst = max(wc.rel_err(g, w) for g, w in zip(wc.infer_ref(name, "f32"), wc.infer_ref(name, "f64")))
    print(f"{name}: infer, fp32 oracle against fp64: {worst:.3g} of the peak (bar {wc.INFER_BAR['f32']:g}, room x{wc.INFER_BAR['f32'] / worst:.0f})")
    assert worst < wc.INFER_BAR["f32"]
    if "forward" in case.dirs:
        ez = el = 0.0
        for (z32, l32), (z64, l64) in zip(wc.forward_ref(name, "f32"), wc.forward_ref(name, "f64")):
            ez, el = max(ez, wc.rel_err(z32, z64)), max(el, abs(l32 - l64) / z64.size)
        print(f"{name}: forward, fp32 oracle against fp64: z {ez:.3g} (bar {wc.Z_BAR:g}), logdet {el:.3g} nats/sample (bar {wc.LD_BAR:g})")
        assert ez < wc.Z_BAR and el < wc.LD_BAR


# ---------------------------------------------------------------- 3. the cases can tell right from wrong
@pytest.mark.parametrize("name", ["fw_c64_a", "fw_c64_b_4flows"])
def test_z_offsets_counted_in_pruned_show_from_the_second_utterance_on(name):
    """The engine reads utterance b's latent at the sum of the earlier cond_len; one that counted the earlier ``pruned`` (as the
    waveform's offsets do) reads 12 samples early per earlier utterance."""
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    state, mels, zs, _ = wc.inputs(name)
    packed = np.concatenate(zs)
    want = wc.infer_ref(name)
    off = 0
    for b, T in enumerate(case.frames):
        clen, pruned = wc.lengths(cfg, T)
        wrong = wc.oracle_infer(state, mels[b], packed[off:off + clen].copy(), cfg)
        err = wc.rel_err(wrong, want[b])
        print(f"{name} utterance {b}: wrong z offset {off} -> {err:.3g} of the peak")
        assert (err == 0.0) if b == 0 else (err > 100 * wc.INFER_BAR["f16"])
        off += pruned


@pytest.mark.parametrize("name", ["up_2", "up_64_m256", "up_2x2x2x2", "up_8x4x2_m112", "fw_c64_a"])
def test_upsampler_without_its_second_tap_is_caught(name):
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    state, mels, zs, _ = wc.inputs(name)
    caught_wave = 0
    for b, T in enumerate(case.frames):
        for direction in ("infer", "forward"):
            want, bound = wc.cond_ref(name, direction)[b]
            trim = direction == "infer"
            same = wc.upsample_direct(state, mels[b], cfg["upsample_factors"], trim)[:, :want.shape[1]]
            assert np.abs(same - want).max() <= 1e-12 * np.abs(want).max()              # the restatement is the oracle's upsampler
            wrong = wc.upsample_direct(state, mels[b], cfg["upsample_factors"], trim, drop_second_tap=True)[:, :want.shape[1]]
            r = fb.ratio(wrong.astype(np.float32), want, bound)
            assert r > 1e3, (b, direction, r)
        wrong = wc.upsample_direct(state, mels[b], cfg["upsample_factors"], True, drop_second_tap=True)
        err = wc.rel_err(wc.infer_from_cond(state, wrong, zs[b], cfg), wc.infer_ref(name)[b])
        caught_wave += err > 10 * wc.INFER_BAR["f32"]
    assert caught_wave == len(case.frames)


@pytest.mark.parametrize("name", ["m16", "m48", "m112", "c192_m48"])
def test_nonzero_padding_of_the_condition_block_is_caught(name):
    """The GEMM path multiplies mp = n_mels rounded up to 32 condition channels; the pad must contribute nothing.  A wrong engine
    whose pad channels wrap around (channel n_mels + k holds channel k's value and weight) adds the first mp - n_mels channels'
    contribution twice: the oracle with those condition_proj weights doubled."""
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    state, mels, zs, _ = wc.inputs(name)
    pad = wc.mp_of(cfg["n_mels"]) - cfg["n_mels"]
    assert 0 < pad <= cfg["n_mels"]
    wrong_state = dict(fold_weight_norm(state))
    for k in list(wrong_state):
        if k.endswith("condition_proj.weight"):
            w = np.array(wrong_state[k])
            w[:, :pad] *= 2
            wrong_state[k] = w
    for b in range(len(case.frames)):
        err = wc.rel_err(wc.oracle_infer(wrong_state, mels[b], zs[b], cfg), wc.infer_ref(name)[b])
        print(f"{name} utterance {b}: wrapped padding -> {err:.3g} of the peak")
        assert err > 100 * wc.INFER_BAR["f32"]


# ---------------------------------------------------------------- 4. the upsample bound is sound
@pytest.mark.parametrize("name", wc.COND_CASES)
def test_upsample_bound_holds_for_the_fp32_oracle(name):
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    state, mels, _, _ = wc.inputs(name)
    W32 = Weights(fold_weight_norm(state), torch.float32).sub("encoder.")
    worst = 0.0
    for b in range(len(case.frames)):
        for direction in ("infer", "forward"):
            want, bound = wc.cond_ref(name, direction)[b]
            with torch.no_grad():
                got = ref.upsample(W32, torch.from_numpy(mels[b])[None], cfg["upsample_factors"], trim=direction == "infer")[0].numpy()
            assert got.dtype == np.float32
            worst = max(worst, fb.ratio(got[:, :want.shape[1]], want, bound))
            assert (bound > 0).all() and (bound < 1e-4 * np.abs(want).max()).all()     # and it is an fp32-sized bound, not a loose one
    print(f"{name}: fp32 upsampler against fp64, largest error / bound = {worst:.3f}")
    assert worst <= 1.0
