"""GPU sweep of ConditionalWaveFlow over every family of configuration pk_wf_create admits (tests/waveflow_cases.py): infer and
forward against the float64 oracle at the project's existing bars, the upsampled condition on its own against an a-priori fp32
bound, which kernel family ran, run-to-run determinism, and the configurations the engine refuses.

Every test prints what it measured next to the float32 oracle's own error at the same case, so the headroom can be read from a log
(DESIGN.md 4.3d lists a hardware run of the whole table)."""
import numpy as np
import pytest

import fp32_bounds as fb
import waveflow_cases as wc
from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FUSED, UNFUSED = (("wf_layer", "wf_row"), "wf_gemm_conv_gate"), ("wf_gemm_conv_gate", ("wf_layer", "wf_row"))
INFER = [(c.name, m) for c in wc.CASES for m in c.maths]
FORWARD = [(c.name, m) for c in wc.CASES if "forward" in c.dirs for m in c.maths]
COND = [(n, d) for n in wc.COND_CASES for d in wc.BY_NAME[n].dirs]


def _model(case, math=None):
    from parakeet_amd.waveflow import ConditionalWaveFlow
    model = ConditionalWaveFlow(**wc.cfg_of(case))
    model.set_state_dict(wc.inputs(case.name)[0])
    model.eval()
    if math:
        model.set_math(math)
    return model


class _Kernels:
    """The ``expect_kernel`` device of tests/test_waveflow_gpu.py: which kernel families had launches inside the block."""

    def __init__(self, expect):
        self.present, self.absent = expect

    def __enter__(self):
        from parakeet_amd.runtime import Context
        self.ctx = Context.get()
        self.ctx.prof_enable(True)
        self.ctx.prof_reset()

    def __exit__(self, *exc):
        names = {k for k, (n, _) in self.ctx.prof_dump().items() if n > 0}
        self.ctx.prof_enable(False)
        if exc[0] is None:
            assert any(n.startswith(self.present) for n in names) and not any(n.startswith(self.absent) for n in names), names


@pytest.mark.parametrize("name,math", INFER)
def test_sweep_infer(name, math):
    case = wc.BY_NAME[name]
    cfg = wc.cfg_of(case)
    _, mels, zs, _ = wc.inputs(name)
    model = _model(case, math)
    for T in case.frames:
        assert model.lengths(T) == wc.lengths(cfg, T)
    with _Kernels(FUSED if wc.fused(case, math) else UNFUSED):
        outs = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
    want, o32 = wc.infer_ref(name), wc.infer_ref(name, "f32")
    errs = []
    for b, T in enumerate(case.frames):
        assert outs[b].shape == want[b].shape == (wc.lengths(cfg, T)[1],) and outs[b].dtype == np.float32
        errs.append(wc.rel_err(outs[b], want[b]) if np.isfinite(outs[b]).all() else float("inf"))
        print(f"{name} {math} infer utt {b} (width {case.widths[b]}): engine {errs[-1]:.3g}, fp32 oracle {wc.rel_err(o32[b], want[b]):.3g} "
              f"of the peak (bar {wc.INFER_BAR[math]:g})")
    assert max(errs) < wc.INFER_BAR[math], errs
    again = model.infer_batch(mels, zs)
    for a, b in zip(outs, again):
        np.testing.assert_array_equal(a, b.numpy())
    if wc.fused(case, math):
        for waves in case.waves:                       # scheduling only: the same bits (test_waveflow_12_wave_workgroups_bit_identical)
            model.set_option("layer_waves", waves)
            for a, b in zip(outs, model.infer_batch(mels, zs)):
                np.testing.assert_array_equal(a, b.numpy(), err_msg=f"layer_waves {waves}")


@pytest.mark.parametrize("name,math", FORWARD)
def test_sweep_forward(name, math):
    case = wc.BY_NAME[name]
    _, mels, _, audios = wc.inputs(name)
    model = _model(case, math)
    with _Kernels((("wf_layer",), "wf_gemm_conv_gate") if wc.fused(case, math) else UNFUSED):
        outs = [(z.numpy().copy(), float(ld)) for z, ld in model.forward_batch(audios, mels)]
    want, o32 = wc.forward_ref(name), wc.forward_ref(name, "f32")
    z_bar, ld_bar = (wc.Z_BAR_F16, wc.LD_BAR_F16) if math == "f16" else (wc.Z_BAR, wc.LD_BAR)
    ezs, els = [], []
    for b, ((z, ld), (zw, lw)) in enumerate(zip(outs, want)):
        assert z.shape == zw.shape and z.dtype == np.float32
        ezs.append(wc.rel_err(z, zw) if np.isfinite(z).all() else float("inf"))
        els.append(abs(ld - lw) / zw.size)
        print(f"{name} {math} forward utt {b} (width {case.widths[b]}): z {ezs[-1]:.3g} (fp32 oracle {wc.rel_err(o32[b][0], zw):.3g}, bar "
              f"{z_bar:g}), logdet {els[-1]:.3g} nats/sample (fp32 oracle {abs(o32[b][1] - lw) / zw.size:.3g}, bar {ld_bar:g})")
    assert max(ezs) < z_bar and max(els) < ld_bar, (ezs, els)
    for (z0, l0), (z1, l1) in zip(outs, model.forward_batch(audios, mels)):
        assert np.array_equal(z0, z1.numpy()) and l0 == float(l1)
    if wc.fused(case, math):
        for waves in case.waves:
            model.set_option("layer_waves", waves)
            for (z0, l0), (z1, l1) in zip(outs, model.forward_batch(audios, mels)):
                assert np.array_equal(z0, z1.numpy()) and l0 == float(l1), f"layer_waves {waves}"


@pytest.mark.parametrize("name,direction", COND)
def test_sweep_condition_tap(name, direction):
    """The upsampler on its own: ``debug_tap("cond", b)`` against ``oracle.waveflow_ref.upsample`` in float64 within the a-priori
    bound of waveflow_cases.upsample_with_bound -- in the layout of the case's own kernel family (blocks of 32 positions on the
    fused kernel, [pos][mp] on the GEMM path) and, for a fused case, in the other one too (math "f32")."""
    case = wc.BY_NAME[name]
    _, mels, zs, audios = wc.inputs(name)
    want = wc.cond_ref(name, direction)
    for math in (("f16x3", "f32") if case.fused else ("f16x3",)):
        model = _model(case, math)
        with pytest.raises(RuntimeError):
            model.debug_tap("cond", 0)                 # PK_ESTATE: no call has run
        if direction == "infer":
            model.set_option("keep_cond", 1)           # the fused infer path turns the condition into planes in place
            model.infer_batch(mels, zs)
        else:
            model.forward_batch(audios, mels)
        worst = 0.0
        for b in range(len(case.frames)):
            got = model.debug_tap("cond", b)
            assert got.shape == want[b][0].shape and got.dtype == np.float32
            worst = max(worst, fb.ratio(got, want[b][0], want[b][1]))
        print(f"{name} {direction} ({'blocked' if wc.fused(case, math) else 'rows'} layout): upsample ratio {worst:.3f}")
        assert worst <= 1.0
        with pytest.raises(ValueError):
            model.debug_tap("cond", len(case.frames))


def test_condition_tap_after_a_fused_infer_needs_keep_cond():
    case = wc.BY_NAME["up_2x2x2x2"]
    _, mels, zs, _ = wc.inputs(case.name)
    model = _model(case)
    model.infer_batch(mels, zs)
    with pytest.raises(RuntimeError, match="keep_cond"):
        model.debug_tap("cond", 0)
    want = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
    model.set_option("keep_cond", 1)                   # a copy, nothing else: the same waveform
    for a, b in zip(want, model.infer_batch(mels, zs)):
        np.testing.assert_array_equal(a, b.numpy())
    assert model.debug_tap("cond", 1).shape == (80, wc.lengths(wc.cfg_of(case), case.frames[1])[1])


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if not c.fused])
def test_fp16_operand_mode_is_refused_off_the_fused_kernel(name):
    model = _model(wc.BY_NAME[name])
    with pytest.raises(NotImplementedError):
        model.set_math("f16")


def test_configurations_outside_the_table_are_refused():
    """k_wf_upsample runs 256 // n_mels time steps per block: none beyond 256 bins (a division by zero on the host before this
    check; no recipe has more than 80).  No mel bins and no or negative channels passed the "multiple of" checks and are refused
    too.  The ends of the admitted ranges construct."""
    from parakeet_amd.waveflow import ConditionalWaveFlow
    base = dict(syn.WAVEFLOW_LJSPEECH, channels=64, n_flows=2)
    for n_mels in (272, 512, 0, -16, 24):
        with pytest.raises(NotImplementedError, match="n_mels"):
            ConditionalWaveFlow(**dict(base, n_mels=n_mels))
    for channels in (0, -64, 320, 96):
        with pytest.raises(NotImplementedError, match="channels"):
            ConditionalWaveFlow(**dict(base, channels=channels))
    for over in (dict(n_mels=wc.MAX_N_MELS), dict(n_mels=16), dict(channels=256)):
        ConditionalWaveFlow(**dict(base, **over))


@pytest.mark.parametrize("name,fused", [("up_2x2x2x2", True), ("m48", False), ("c192_m48", False)])
def test_auto_cast_runs_every_model(name, fused):
    """``with amp.auto_cast():`` (examples/waveflow/synthesize.py:40): fp16 operands where the model has that mode -- the result of
    set_math("f16") bit for bit -- and the model's own math where it has not: the call outside the context bit for bit."""
    from parakeet_amd import amp
    case = wc.BY_NAME[name]
    assert case.fused == fused
    _, mels, zs, audios = wc.inputs(name)
    model = _model(case)
    plain = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
    plain_fw = [(z.numpy().copy(), float(ld)) for z, ld in model.forward_batch(audios, mels)]
    with amp.auto_cast():
        cast = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
        cast_fw = [(z.numpy().copy(), float(ld)) for z, ld in model.forward_batch(audios, mels)]
    after = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
    for a, b in zip(plain, after):
        np.testing.assert_array_equal(a, b)            # the context leaves the model's math as it was
    if fused:
        model.set_math("f16")
        want = [o.numpy().copy() for o in model.infer_batch(mels, zs)]
        want_fw = [(z.numpy().copy(), float(ld)) for z, ld in model.forward_batch(audios, mels)]
        assert any(not np.array_equal(a, b) for a, b in zip(plain, want))
    else:
        want, want_fw = plain, plain_fw
    for a, b in zip(cast, want):
        np.testing.assert_array_equal(a, b)
    for (z0, l0), (z1, l1) in zip(cast_fw, want_fw):
        assert np.array_equal(z0, z1) and l0 == l1
