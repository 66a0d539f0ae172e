"""The few-rows GEMM of the autoregressive decoders (k_rowgemm<LN>, csrc/rowgemm.hip) through pk_op_rowgemm: plain path,
LayerNorm prologue, ReLU / dropout / residual, LSTM-cell epilogue, stop-token head and status codes, against fp64
references under the derived bounds of tests/fp32_bounds.py.  ``SWEEP-RATIO`` lines as in tests/test_ops_sweep_gpu.py.
"""
import numpy as np
import pytest
import torch

import fp32_bounds as fb
import sweep_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)


def _report(test, case, **ratios):
    for name, r in ratios.items():
        print(f"SWEEP-RATIO {test} {case} {name} {r:.4g}")
    return max(ratios.values())


def _dev(a, dtype=torch.float32):
    from parakeet_amd.runtime import Context
    return Context.get().to_device(a, dtype)


def _full(shape, value=float(SENTINEL), dtype=torch.float32):
    from parakeet_amd.runtime import Context
    return torch.full(shape, value, dtype=dtype, device=Context.get().device)


def _padded(a, extra):
    """(M, K) -> device (M, K + extra) with SENTINEL-free padding that must never be read into a result: huge values"""
    out = np.full((a.shape[0], a.shape[1] + extra), 1e30, np.float32)
    out[:, :a.shape[1]] = a
    return _dev(out)


def _plain(x, w, bias, **kw):
    from parakeet_amd import engine_ops as eo
    M, K = x.shape
    N = w.shape[1]
    y = _full((M + 1, N + 3))
    eo.rowgemm(x=_padded(x, 4), ldx=K + 4, W=w, bias=bias, y=y, ldy=N + 3, M=M, K=K, N=N, **kw)
    y = y.cpu().numpy()
    assert np.all(y[M:] == SENTINEL) and np.all(y[:, N:] == SENTINEL)
    return y[:M, :N]


@pytest.mark.parametrize("c", sc.ROW_CASES, ids=sc.row_id)
def test_rowgemm_plain_sweep(c):
    x, w, bias = sc.rowgemm_inputs(c.M, c.K, c.N, bias=c.bias)
    want, bound = sc.matmul_reference(x, w, bias)
    got = _plain(x, w, bias)
    assert _report("rowgemm", sc.row_id(c), y=fb.ratio(got, want, bound)) <= 1.0
    if not c.bias:                                # exact fp32 FMA arithmetic: powers of two pass through bit for bit
        for s in (np.float32(2.0 ** 20), np.float32(2.0 ** -20)):
            assert np.array_equal(_plain(x * s, w, None), got * s)


@pytest.mark.parametrize("K", sc.ROW_LN_K)
@pytest.mark.parametrize("M,N", ((1, 17), (31, 80), (32, 16)))
def test_rowgemm_layernorm_prologue(K, M, N):
    _, w, bias = sc.rowgemm_inputs(M, K, N, "lnw")
    x, g, beta = sc.layernorm_rows(M, K)
    want, bound, _, _ = sc.rowgemm_ln_reference(x, g, beta, w, bias)
    got = _plain(x, w, bias, ln_g=g, ln_b=beta, ln_eps=1e-5)
    assert _report("rowgemm_ln", f"M{M}-K{K}-N{N}", y=fb.ratio(got, want, bound)) <= 1.0


@pytest.mark.parametrize("base,J,j", ((0, 1, 0), (5, 3, 2), (2 ** 33, 2, 1)))
def test_rowgemm_relu_dropout_residual(base, J, j):
    from oracle import philox_ref
    M, K, N = 31, 64, 80
    x, w, bias = sc.rowgemm_inputs(M, K, N, "drop")
    res = sc.f32(sc.rng_for("dropres").normal(0.3, 1, (M, N + 2)))
    seeds = np.arange(M, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(7)
    p, scale = 0.25, np.float32(1.0 / 0.75)
    got = _plain(x, w, bias, act=1, dropout=1, drop_base=base, drop_J=J, drop_j=j, drop_seeds=seeds,
                 drop_thr=philox_ref.dropout_threshold(p), drop_scale=float(scale), res=res, ldr=N + 2)
    pre, b = sc.matmul_reference(x, w, bias)
    idx = np.uint64((base * J + j) * N) + np.arange(N, dtype=np.uint64)
    keep = np.stack([philox_ref.dropout_keep(idx, p, int(s)) for s in seeds])
    # the kernel's own mask, read off its output: a dropped element is exactly the residual
    live = np.maximum(pre, 0) > 4 * b             # where ReLU's output is certainly non-zero the mask is visible
    assert np.array_equal((got != res[:, :N])[live], keep[live])
    want = np.where(keep, np.maximum(pre, 0) * np.float64(scale), 0.0) + res[:, :N]
    bound = fb.epilogue_step(want, fb.epilogue_step(np.maximum(pre, 0) * scale, b * scale))
    assert _report("rowgemm_dropout", f"base{base}-J{J}-j{j}", y=fb.ratio(got, want, bound)) <= 1.0
    assert 0.6 < keep.mean() < 0.9


@pytest.mark.parametrize("H", sc.ROW_LSTM_H)
def test_rowgemm_lstm_epilogue_two_steps(H):
    from parakeet_amd import engine_ops as eo
    M, K = 31, 64
    r = sc.rng_for("lstm", H)
    _, w, bias = sc.rowgemm_inputs(M, K, 4 * H, "lstmw")
    xs = [sc.f32(r.normal(0.3, 1, (M, K))) for _ in range(2)]
    c0 = sc.f32(r.normal(0.2, 1, (M, H)))
    c = _dev(c0)
    y = _full((M, 4 * H))
    cw, b_c = c0.astype(np.float64), 0.0
    for step, x in enumerate(xs):
        h1, h2 = _full((M + 1, H + 1)), _full((M + 1, H + 5))
        eo.rowgemm(x=x, ldx=K, W=w, bias=bias, y=y, ldy=4 * H, M=M, K=K, N=4 * H, lstm_c=c, lstm_H=H, lstm_h1=h1,
                   lstm_ld1=H + 1, lstm_h2=h2, lstm_ld2=H + 5)
        cw, hw, b_c, b_h = sc.lstm_reference(x, w, bias, cw, b_c)
        g1, g2 = h1.cpu().numpy(), h2.cpu().numpy()
        assert np.all(g1[M:] == SENTINEL) and np.all(g1[:, H:] == SENTINEL) and np.all(g2[M:] == SENTINEL) and \
            np.all(g2[:, H:] == SENTINEL)
        assert np.array_equal(g1[:M, :H], g2[:M, :H])
        assert _report("rowgemm_lstm", f"H{H}-step{step}", c=fb.ratio(c.cpu().numpy(), cw, b_c),
                       h=fb.ratio(g1[:M, :H], hw, b_h)) <= 1.0
        if step == 1:                              # a stale c (step 2 computed from c0) must be outside the bound
            stale, _, _, _ = sc.lstm_reference(x, w, bias, c0.astype(np.float64), 0.0)
            assert fb.ratio(stale, cw, b_c) > 1.0
    assert np.all(y.cpu().numpy() == SENTINEL)    # y is not written by the LSTM epilogue


@pytest.mark.parametrize("ln", (False, True))
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_rowgemm_stop_head(kind, ln):
    from parakeet_amd import engine_ops as eo
    if kind >= 1 and ln:
        with pytest.raises(ValueError):           # Tacotron2's rule has no LayerNorm
            eo.rowgemm(x=np.zeros((1, 64), np.float32), ldx=64, W=np.zeros((64, 16), np.float32), y=_full((1, 16)), ldy=16,
                       M=1, K=64, N=16, ln_g=np.ones(64, np.float32), ln_b=np.zeros(64, np.float32),
                       stop_w=np.ones(64, np.float32), stop_kind=kind, stop_probs=_full((4,)),
                       stop_len=_full((1,), 0, torch.int32), stop_ndone=_full((1,), 0, torch.int32))
        return
    M, K, N = 6, 256, 16
    x, sw, g, beta = sc.stop_inputs(ln)           # rows 0, 2, 4 fire, rows 1, 3, 5 do not -- by construction
    _, w, bias = sc.rowgemm_inputs(M, K, N, "stop")
    sbias = 0.25
    logit, b_logit, _ = sc.stop_reference(x, sw, g, beta, sbias)
    fire = logit > 0
    assert np.all(np.abs(logit) > 100 * b_logit) and list(fire) == [True, False] * 3, "a stop decision is ambiguous"
    step = 3
    minlen = np.array([0, 0, 5, 0, 0, 0], np.int32)                   # row 2 fires but is below its minimum length
    maxlen = np.array([9, 3, 9, 9, 9, 9], np.int32)                   # row 1 does not fire but has reached its maximum
    slen0 = np.array([0, 0, 0, 0, 2, 0], np.int32)                    # row 4 had stopped before
    for max_steps in (10, step + 1):              # step + 1 == max_steps: kind 1 ends every running row
        probs = _full(((step + 1) * M,))
        slen, ndone = _dev(slen0, torch.int32), _dev(np.array([1], np.int32), torch.int32)
        if kind == 2:                             # records the logit and touches neither array
            slen, ndone = _full((M,), 1234, torch.int32), _full((1,), 1234, torch.int32)
        y = _full((M, N))
        eo.rowgemm(x=x, ldx=K, W=w, bias=bias, y=y, ldy=N, M=M, K=K, N=N, ln_g=g, ln_b=beta, stop_w=sw, stop_bias=sbias,
                   stop_thr=0.5, stop_kind=kind, stop_max_steps=max_steps, stop_step=step, stop_probs=probs,
                   stop_minlen=minlen, stop_maxlen=maxlen, stop_len=slen, stop_ndone=ndone)
        pr = probs.cpu().numpy().reshape(step + 1, M)
        row = step - 1 if kind == 0 else step
        if kind == 0:
            want, bound = 1 / (1 + np.exp(-logit)), fb.sigmoid_bound(None, b_logit)
        else:
            want, bound = logit, b_logit
        assert _report("rowgemm_stop", f"kind{kind}-{'ln' if ln else 'noln'}-max{max_steps}",
                       p=fb.ratio(pr[row], want, bound)) <= 1.0
        assert np.all(np.delete(pr, row, 0) == SENTINEL)
        if kind == 0:
            ends = (slen0 == 0) & (fire | (step >= maxlen)) & (step >= minlen)
            exp_len = np.where(ends, step, slen0)
        elif kind == 1:
            ends = (slen0 == 0) & (fire | (step + 1 >= max_steps))
            exp_len = np.where(ends, step + 1, slen0)
            assert ends.sum() == (5 if max_steps == step + 1 else 2)
        if kind == 2:
            assert np.all(slen.cpu().numpy() == 1234) and int(ndone.cpu()) == 1234
        else:
            assert np.array_equal(slen.cpu().numpy(), exp_len) and int(ndone.cpu()) == 1 + int(ends.sum())
        # the GEMM of the same launch is unaffected
        wanty, boundy = (sc.rowgemm_ln_reference(x, g, beta, w, bias)[:2] if ln else sc.matmul_reference(x, w, bias))
        assert fb.ratio(y.cpu().numpy(), wanty, boundy) <= 1.0


def test_rowgemm_status_codes():
    from parakeet_amd import engine_ops as eo
    z = lambda *s: np.zeros(s, np.float32)
    ok = dict(x=z(2, 64), ldx=64, W=z(64, 16), y=_full((2, 16)), ldy=16, M=2, K=64, N=16)
    def run(**kw):
        eo.rowgemm(**dict(ok, **kw))
    run()
    with pytest.raises(ValueError):
        run(M=0)
    with pytest.raises(NotImplementedError):      # K % 4
        run(K=62, W=z(62, 16))
    with pytest.raises(NotImplementedError):      # ldx % 4
        run(x=z(2, 66), ldx=66)
    with pytest.raises(NotImplementedError):      # LayerNorm over K > 512
        run(x=z(2, 516), ldx=516, K=516, W=z(516, 16), ln_g=z(516), ln_b=z(516))
    with pytest.raises(NotImplementedError):      # LayerNorm without its bias
        run(ln_g=z(64))
    with pytest.raises(NotImplementedError):      # tanh is not an activation of this kernel
        run(act=2)
    lst = dict(lstm_c=_full((2, 4)), lstm_H=4, lstm_h1=_full((2, 4)), lstm_ld1=4, lstm_h2=_full((2, 4)), lstm_ld2=4)
    run(**lst)
    with pytest.raises(ValueError):               # N != 4 H
        run(**dict(lst, lstm_H=8))
    with pytest.raises(ValueError):               # an activation with the LSTM epilogue
        run(**dict(lst, act=1))
    with pytest.raises(ValueError):               # one h destination missing
        run(**dict(lst, lstm_h2=None))
    stop = dict(stop_w=z(64), stop_probs=_full((8,)), stop_len=_full((2,), 0, torch.int32),
                stop_ndone=_full((1,), 0, torch.int32), stop_minlen=np.zeros(2, np.int32), stop_maxlen=np.zeros(2, np.int32),
                stop_step=1)
    run(**stop)
    for bad in (dict(stop_probs=None), dict(stop_len=None), dict(stop_minlen=None), dict(stop_kind=3), dict(stop_kind=-1)):
        with pytest.raises(ValueError):
            run(**dict(stop, **bad))
    with pytest.raises(ValueError):               # more rows than one stop workgroup pass holds
        run(**dict(stop, x=z(33, 64), M=33, y=_full((33, 16))))
    run(**dict(stop, stop_kind=2, stop_len=None, stop_ndone=None, stop_minlen=None, stop_maxlen=None))
