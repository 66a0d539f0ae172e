"""The FFT-stack kernels (csrc/fft.hip, csrc/ffn_planes.hip) over head sizes, length edges and maths, through ``FastSpeech2``
and its debug taps, against the float64 oracle under the bar of tests/fft_stack_cases.py (4 x the float32 oracle's own error,
from the references alone).  ``SWEEP-RATIO fft_stack <case> <tap> <error / bar>`` before every assertion.

Per case: the ragged batch of tile-edge lengths in table order and reversed; encoder tap (0) and decoder tap (5) of every
utterance under the bar; durations (tap 3) equal to the oracle's; both batch orders give each utterance the same bits; and the
profile shows the kernels the case is meant to run.
"""
import functools

import numpy as np
import pytest

import fft_stack_cases as fc

pytestmark = pytest.mark.gpu

TILE_GEMM = ("fs2_gemm_qkv", "fs2_gemm_attn_out", "fs2_conv_ffn1", "fs2_conv_ffn2")
PLANES = ("fs2_layernorm_planes", "fs2_gemm_qkv_planes", "fs2_gemm_attn_out_planes", "fs2_conv_ffn1_planes", "fs2_conv_ffn2_planes")


@functools.lru_cache(maxsize=1)
def _model(name, gain):
    """The engine model of a case (kept for the case's second math; its options are never touched)."""
    from parakeet_amd.fastspeech2 import FastSpeech2
    model = FastSpeech2(fc.IDIM, fc.ODIM, **fc.config(name))
    model.set_state_dict(fc.state(name, gain))
    model.eval()
    model.set_debug(True)
    return model


def _fresh_model(name, gain, math, options):
    from parakeet_amd.fastspeech2 import FastSpeech2
    model = FastSpeech2(fc.IDIM, fc.ODIM, **fc.config(name))
    model.set_state_dict(fc.state(name, gain))
    model.eval()
    model.set_debug(True)
    model.set_math(math)
    for k, v in options.items():
        model.set_option(k, v)
    return model


def _run(model, texts):
    """encode + decode of one batch with the profile on -> (taps 0, 5, 3 per utterance, names of the kernels that ran)."""
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        frames = model.encode_batch(texts)
        model.decode_packed()
        names = {k for k, (n, _) in ctx.prof_dump().items() if n > 0}
    finally:
        ctx.prof_enable(False)
    assert [int(f) for f in frames] == [len(t) for t in texts]
    taps = [(model.debug_tap(0, b), model.debug_tap(5, b), model.debug_tap(3, b)) for b in range(len(texts))]
    return taps, names


def _sweep(model, name, gain, tag):
    """Both batch orders against the references; returns the kernel names and the taps of the run in table order."""
    ref, texts = fc.reference(name, gain), fc.texts(name)
    fwd, names = _run(model, texts)
    rev, _ = _run(model, texts[::-1])
    rev = rev[::-1]
    for tap, i in (("hs", 0), ("zs", 1)):
        err = fc.tap_error([t[i] for t in fwd], ref[tap])
        print(f"SWEEP-RATIO fft_stack {tag} {tap} {err / ref['bar'][tap]:.4f}   (error {err:.3e}, bar {ref['bar'][tap]:.3e})")
    for tap, i in (("hs", 0), ("zs", 1)):
        err = fc.tap_error([t[i] for t in fwd], ref[tap])
        assert err <= ref["bar"][tap], f"{tag} {tap}: error {err:.3e} above the bar {ref['bar'][tap]:.3e}"
    for b, T in enumerate(fc.LENGTHS):
        np.testing.assert_array_equal(fwd[b][2], ref["d"][b])
        for i in range(3):
            assert np.array_equal(fwd[b][i], rev[b][i]), f"{tag}: utterance of {T} rows differs between the batch orders (tap {(0, 5, 3)[i]})"
    return names, fwd


def _ran(names, prefix):
    """A kernel of the profile name ``prefix`` ran (the tile GEMM appends its own variant to the name it is given)."""
    return any(n == prefix or (n.startswith(prefix + "_") and "planes" not in n) for n in names)


@pytest.mark.parametrize("math", fc.MATHS)
@pytest.mark.parametrize("gain", fc.GAINS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_fft_stack_sweep(name, gain, math):
    """(The oracle's position table takes its frequencies rounded once, oracle/nn_ref.py::sinusoid_table, as the engine's are: a
    last-bit difference there is multiplied by the row's position and was larger than this bar at gain 1.)"""
    model = _model(name, gain)
    model.set_math(math)
    names, _ = _sweep(model, name, gain, fc.case_id(name, gain, math))
    # paths taken: exact fp32 -> k_attention and the tile GEMM; split-fp16 -> the LDS attention kernels, and the planes kernels
    # for the one shape they are built for (adim 384, units 1536, k 3, pre-norm), the tile GEMM for every other
    assert "fs2_layernorm" in names, names
    if math == "f32":
        assert "fs2_attention" in names and "fs2_attention_h3" not in names, names
    else:
        assert "fs2_attention_h3" in names and "fs2_attention" not in names, names
    if math == "f16x3" and name == fc.PLANES_MODEL:
        assert set(PLANES) <= names, names
        assert not any(_ran(names, p) for p in TILE_GEMM), names
    else:
        assert not any("planes" in n for n in names), names
        assert all(_ran(names, p) for p in TILE_GEMM), names
    if math == "f16x3":     # post-norm: the operand scales of attention come from a pass over q|k|v, pre-norm: from bounds
        assert ("fs2_qkv_amax" in names) == (not fc.MODEL[name].get("prenorm", True)), names


@pytest.mark.parametrize("gain", fc.GAINS)
def test_fft_stack_planes_shape_on_the_tile_gemm(gain):
    """Option "ffn_planes" = 0 for the planes-capable model: the same bars on the other path, and no planes kernel runs."""
    name = fc.PLANES_MODEL
    model = _fresh_model(name, gain, "f16x3", {"ffn_planes": 0})
    names, _ = _sweep(model, name, gain, fc.case_id(name, gain, "f16x3") + "-ffn_planes=0")
    assert not any("planes" in n for n in names), names
    assert all(_ran(names, p) for p in TILE_GEMM), names


@pytest.mark.parametrize("gain", fc.GAINS)
@pytest.mark.parametrize("name", ("a384h2", "a192h1"))
def test_fft_stack_attention_waves(name, gain):
    """dk 192 in split-fp16 runs the pipelined attention kernel with 4 or 8 query tiles per workgroup ("attn_waves"; 0 = the
    launcher's choice).  Each meets the bar; 4 and 8 are the same bits: a wave's arithmetic does not depend on the workgroup's
    size, only the split of the K / V loads among its threads does.

    (The profile gives both kernels the name fs2_attention_h3 and does not expose the launch geometry, so nothing here observes
    WHICH one ran.  From pk_fft_run_attention: with at most 3 x 2 x 13 workgroups of 128 queries, far fewer than the CUs, 0 picks
    4 tiles; 8 forces k_attention_h3_lds<192, true, 512>.  If the option were ignored, 4 == 8 would hold trivially.)"""
    taps = {}
    for waves in (0, 4, 8):
        model = _fresh_model(name, gain, "f16x3", {"attn_waves": waves})
        names, taps[waves] = _sweep(model, name, gain, fc.case_id(name, gain, "f16x3") + f"-attn_waves={waves}")
        assert "fs2_attention_h3" in names, names
    for b, T in enumerate(fc.LENGTHS):
        for i in range(2):
            assert np.array_equal(taps[4][b][i], taps[8][b][i]), f"utterance of {T} rows: 4 and 8 query tiles differ (tap {(0, 5)[i]})"
