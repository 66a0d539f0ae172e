"""Sweep of the public primitives of parakeet_amd.modules (ops.hip, and through them the exact-fp32 GEMM k_gemm at
arbitrary shapes) against fp64 restatements, under the derived bounds of tests/fp32_bounds.py.

Cases, inputs and references live in tests/sweep_cases.py, shared with tests/test_fp32_bounds_cpu.py, which shows on the
host that every bound used here rejects a wrong result.  Every test prints ``SWEEP-RATIO <test> <case> <quantity>
<error / bound>`` before it asserts, so a log shows the headroom.  Everything goes through the Python classes; the raw C
ABI is used only for what they cannot reach (no batch norm, the matmul bias, weights = NULL, status codes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import sweep_cases as sc

pytestmark = pytest.mark.gpu

UP, DOWN = np.float32(2.0 ** 20), np.float32(2.0 ** -20)


def _report(test, case, **ratios):
    for name, r in ratios.items():
        print(f"SWEEP-RATIO {test} {case} {name} {r:.4g}")
    return max(ratios.values())


def _ctx():
    from parakeet_amd.runtime import Context
    return Context.get()


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("c", sc.ATT_CASES + [sc.ATT_LDS_EDGE], ids=sc.att_id)
def test_attention_sweep(c):
    from parakeet_amd.modules import scaled_dot_product_attention
    q, k, v, mask = sc.attention_inputs(c)
    ref = sc.attention_reference(q, k, v, mask)
    out, w = scaled_dot_product_attention(q, k, v, mask)
    out, w = _np(out), _np(w)
    worst = _report("attention", sc.att_id(c), weights=fb.ratio(w, ref["w"], ref["b_w"]),
                    out=fb.ratio(out, ref["out"], ref["b_out"]))
    assert worst <= 1.0
    # masked keys of a live row have reference weight 0 and bound 0: the ratio above already demands exact zeros
    if ref["dead"].any():
        # fp32 semantics of the reference: s - 1e9 loses s (|s| < ulp(1e9) / 2 = 32), all logits equal -> exactly 1 / Tk
        assert np.array_equal(w[ref["dead"]], np.full_like(w[ref["dead"]], np.float32(1.0) / np.float32(c.Tk)))
    # the fp32 path scales exactly with a power of two on v: same weights, out times the power, bit for bit
    for s in (UP, DOWN):
        o2, w2 = scaled_dot_product_attention(q, k, v * s, mask)
        assert np.array_equal(_np(w2), w)
        assert np.array_equal(_np(o2), out * s)


def test_attention_c_abi_null_weights_and_lds_limit():
    from parakeet_amd import _capi
    from parakeet_amd.runtime import dptr
    ctx = _ctx()
    c = sc.AttCase(200, 80, 65, 4, "none")
    q, k, v, _ = sc.attention_inputs(c)
    B, Tq = sc.ATT_ROWS[c.rows]
    dq, dk, dv_ = ctx.to_device(q), ctx.to_device(k), ctx.to_device(v)
    o1, o2, w = ctx.empty((B, Tq, c.dv)), ctx.empty((B, Tq, c.dv)), ctx.empty((B, Tq, c.Tk))
    f = ctx.lib.pk_op_scaled_dot_product_attention
    assert f(ctx.handle, dptr(dq), dptr(dk), dptr(dv_), None, 0, B, Tq, c.Tk, c.d, c.dv, dptr(o1), dptr(w)) == _capi.PK_OK
    assert f(ctx.handle, dptr(dq), dptr(dk), dptr(dv_), None, 0, B, Tq, c.Tk, c.d, c.dv, dptr(o2), None) == _capi.PK_OK
    assert np.array_equal(_np(o1), _np(o2))
    # d + Tk = 4097: four waves of (d + Tk) floats no longer fit the 64 KB of LDS -> PK_EUNSUPPORTED, nothing launched
    Tk, d = 4001, 96
    big_q, big_k, big_v = ctx.to_device(np.zeros((1, 1, d), np.float32)), ctx.to_device(np.zeros((1, Tk, d), np.float32)), \
        ctx.to_device(np.zeros((1, Tk, 8), np.float32))
    o, w = ctx.empty((1, 1, 8)), ctx.empty((1, 1, Tk))
    assert f(ctx.handle, dptr(big_q), dptr(big_k), dptr(big_v), None, 0, 1, 1, Tk, d, 8, dptr(o), dptr(w)) == -3
    from parakeet_amd.modules import scaled_dot_product_attention
    with pytest.raises(NotImplementedError):
        scaled_dot_product_attention(_np(big_q), _np(big_k), _np(big_v))
    assert f(ctx.handle, dptr(big_q), dptr(big_k), dptr(big_v), dptr(w), 3, 1, 1, Tk - 1, d, 8, dptr(o), dptr(w)) == -1


# ------------------------------------------------------------------------------------------------ Conv1dBatchNorm
def _conv_raw(x_nlc, st, c, pad=None, tout=None):
    """pk_op_conv1d_batchnorm_nlc without batch norm (the Python class always passes one)."""
    from parakeet_amd import _capi
    from parakeet_amd.runtime import dptr
    ctx = _ctx()
    pad = c.pad if pad is None else pad
    x = ctx.to_device(x_nlc)
    B, T, _ = x.shape
    y = ctx.empty((B, T + 2 * pad - c.k + 1 if tout is None else tout, c.Cout))
    bias = st.get("conv.bias")
    _capi.check(ctx.lib.pk_op_conv1d_batchnorm_nlc(
        ctx.handle, dptr(x), B, T, c.Cin, c.Cout, c.k, pad, _capi.fptr(st["conv.weight"]),
        None if bias is None else _capi.fptr(bias), None, None, None, None, C.c_float(1e-5), dptr(y)))
    return _np(y)


@pytest.mark.parametrize("c", sc.CONV_CASES, ids=sc.conv_id)
def test_conv1d_batchnorm_sweep(c):
    from parakeet_amd.modules import Conv1dBatchNorm
    x, st = sc.conv_inputs(c)
    want, bound, _, _, sh = sc.conv_reference(x, st, c.k, c.pad)
    if c.bn:
        m = Conv1dBatchNorm(c.Cin, c.Cout, c.k, padding=c.pad, data_format=c.layout)
        m.set_state_dict(st)
        m.eval()
        got = _np(m(np.ascontiguousarray(x.transpose(0, 2, 1)) if c.layout == "NCL" else x))
        got = got.transpose(0, 2, 1) if c.layout == "NCL" else got
    else:
        got = _conv_raw(x, st, c)
    assert got.shape == want.shape
    assert _report("conv1d_bn", sc.conv_id(c), y=fb.ratio(got, want, bound)) <= 1.0
    lead = min(c.pad - c.k + 1, want.shape[1])
    if lead > 0:
        # output rows whose taps see nothing but padding hold the folded bias of their channel: one value per channel
        edge = np.concatenate([got[:, :lead], got[:, want.shape[1] - lead:]], axis=1)
        assert np.array_equal(edge, np.broadcast_to(edge[0, 0], edge.shape))
        assert fb.ratio(edge[0, 0], sh, 2.0 * fb.U * np.abs(sh)) <= 1.0
    # exact scaling of the fp32 path: no bias, no batch norm, activations times 2^20 and 2^-20
    plain = {"conv.weight": st["conv.weight"]}
    y0 = _conv_raw(x, plain, c)
    for s in (UP, DOWN):
        assert np.array_equal(_conv_raw(x * s, plain, c), y0 * s)


def test_conv1d_batchnorm_status_codes():
    from parakeet_amd.modules import Conv1dBatchNorm

    def run(cin, cout, k, pad, T):
        r = np.random.default_rng(0)
        m = Conv1dBatchNorm(cin, cout, k, padding=pad, data_format="NLC")
        m.set_state_dict({"conv.weight": r.normal(size=(cout, cin, k)), "bn.weight": np.ones(cout), "bn.bias": np.zeros(cout),
                          "bn._mean": np.zeros(cout), "bn._variance": np.ones(cout)})
        return m(r.normal(size=(2, T, cin)).astype(np.float32))

    with pytest.raises(NotImplementedError):      # PK_EUNSUPPORTED: in_channels not a multiple of 16
        run(20, 8, 3, 1, 9)
    with pytest.raises(ValueError):               # PK_EINVAL: more than 12 taps
        run(16, 8, 13, 6, 40)
    # PK_ESHAPE: kernel longer than the padded input (through the C ABI: the Python class has no output to hand over)
    c = sc.ConvCase(16, 8, 5, 1, 2, 2, False, False, "NLC")
    with pytest.raises(AssertionError):
        _conv_raw(np.zeros((2, 2, 16), np.float32), {"conv.weight": np.zeros((8, 16, 5), np.float32)}, c, pad=1, tout=1)
    assert tuple(run(16, 8, 5, 2, 1).shape) == (2, 1, 8)      # T smaller than k is fine once the padding covers it


# ------------------------------------------------------------------------------------------------ Linear / MultiheadAttention
@pytest.mark.parametrize("cin,cout,rows", [(16, 1, 1), (80, 127, 127), (256, 128, 128), (16, 129, 129), (80, 300, 1000)])
def test_linear_sweep(cin, cout, rows):
    from parakeet_amd.modules import Linear
    r = sc.rng_for("linear", cin, cout, rows)
    w = sc.f32(r.normal(0.3, 1.0, (cin, cout)) / np.sqrt(cin))
    b = sc.f32(r.normal(0.2, 1.0, cout))
    x = sc.f32(r.normal(0.5, 1.0, (rows, cin)))
    lin = Linear(cin, cout)
    for bias in (b, None):
        lin.set(w, bias)
        want, bound = sc.matmul_reference(x, w, bias)
        got = _np(lin(x))
        assert _report("linear", f"{cin}x{cout}-rows{rows}-{'bias' if bias is not None else 'nobias'}",
                       y=fb.ratio(got, want, bound)) <= 1.0
    for s in (UP, DOWN):                          # lin holds no bias now
        assert np.array_equal(_np(lin(x * s)), got * s)
    assert np.array_equal(_np(lin(x.reshape(1, rows, cin))).reshape(rows, cout), got)     # leading dimensions are views


@pytest.mark.parametrize("D,H,kd,vd,B,Tq,Tk", [(64, 4, None, None, 3, 9, 13), (80, 1, None, None, 1, 5, 200),
                                               (64, 2, 48, 80, 2, 7, 65), (48, 3, 16, 32, 2, 1, 130)])
def test_multihead_attention_is_the_composition_of_the_swept_primitives(D, H, kd, vd, B, Tq, Tk):
    """affine_q/k/v -> split heads -> attention -> merge -> affine_o: the head split and merge are layout moves, so the
    module must equal, bit for bit, Linear and scaled_dot_product_attention (both swept above against fp64) called by hand;
    the attention weights are checked against fp64 from the engine's own projections."""
    from parakeet_amd.modules import Linear, MultiheadAttention, scaled_dot_product_attention
    r = sc.rng_for("mha", D, H, kd, vd, B, Tq, Tk)
    depth = D // H
    dims = {"q": (D, H * (kd or depth)), "k": (D, H * (kd or depth)), "v": (D, H * (vd or depth)), "o": (H * (vd or depth), D)}
    st = {}
    for nm, (i, o) in dims.items():
        st[f"affine_{nm}.weight"] = sc.f32(r.normal(0.1, 1.0, (i, o)) / np.sqrt(i))
        st[f"affine_{nm}.bias"] = sc.f32(r.normal(0.0, 0.1, o))
    q, k, v = (sc.f32(r.normal(0.3, 1.0, (B, T, D))) for T in (Tq, Tk, Tk))
    mask = np.ones((B, 1, Tk), np.float32)
    mask[B - 1, :, Tk // 2:] = 0
    mha = MultiheadAttention(D, H, k_dim=kd, v_dim=vd)
    mha.set_state_dict(st)
    mha.eval()
    out, w = mha(q, k, v, mask)
    lin = {}
    for nm, (i, o) in dims.items():
        lin[nm] = Linear(i, o)
        lin[nm].set(st[f"affine_{nm}.weight"], st[f"affine_{nm}.bias"])

    def split(t, T):
        return _np(t).reshape(B, T, H, -1).transpose(0, 2, 1, 3)

    qq, kk, vv = split(lin["q"](q), Tq), split(lin["k"](k), Tk), split(lin["v"](v), Tk)
    ctxv, ww = scaled_dot_product_attention(qq, kk, vv, mask[:, None])
    assert tuple(w.shape) == (B, H, Tq, Tk)
    assert np.array_equal(_np(w), _np(ww))
    merged = _np(ctxv).transpose(0, 2, 1, 3).reshape(B, Tq, -1)
    assert np.array_equal(_np(out), _np(lin["o"](np.ascontiguousarray(merged))))
    ref = sc.attention_reference(qq.reshape(B * H, Tq, -1), kk.reshape(B * H, Tk, -1), vv.reshape(B * H, Tk, -1),
                                 np.repeat(mask, H, axis=0))
    assert _report("mha", f"D{D}-H{H}-kd{kd}-vd{vd}-Tk{Tk}",
                   weights=fb.ratio(_np(w).reshape(B * H, Tq, Tk), ref["w"], ref["b_w"]),
                   context=fb.ratio(_np(ctxv).reshape(B * H, Tq, -1), ref["out"], ref["b_out"])) <= 1.0


# ------------------------------------------------------------------------------------------------ matmul
def _matmul_raw(x, w, bias):
    from parakeet_amd import _capi
    from parakeet_amd.runtime import dptr
    ctx = _ctx()
    dx = ctx.to_device(x)
    M, K = x.shape
    N = w.shape[1]
    y = ctx.empty((M, N))
    _capi.check(ctx.lib.pk_op_matmul(ctx.handle, dptr(dx), M, K, N, _capi.fptr(w), None if bias is None else _capi.fptr(bias),
                                     dptr(y)))
    return _np(y)


@pytest.mark.parametrize("c", sc.MM_CASES, ids=sc.mm_id)
def test_matmul_sweep(c):
    x, w, b = sc.matmul_inputs(c)
    want, bound = sc.matmul_reference(x, w, b)
    got = _matmul_raw(x, w, b)
    assert _report("matmul", sc.mm_id(c), y=fb.ratio(got, want, bound)) <= 1.0
    if b is None:
        for s in (UP, DOWN):
            assert np.array_equal(_matmul_raw(x * s, w, None), got * s)


# ------------------------------------------------------------------------------------------------ Conv1dCell
def _cell(c, st):
    from parakeet_amd.modules import Conv1dCell
    cell = Conv1dCell(c.Cin, c.Cout, c.k, dilation=c.dil, bias_attr=None if c.bias else False)
    cell.set_state_dict(st)
    cell.eval()
    cell.start_sequence()
    return cell


@pytest.mark.parametrize("c", sc.CELL_CASES, ids=sc.cell_id)
def test_conv1d_cell_sweep(c):
    x, st = sc.cell_inputs(c)
    want, bound, _, _, _ = sc.cell_reference(x, st, c.k, c.dil)
    cell = _cell(c, st)
    assert x.shape[2] == 2 * cell.receptive_field
    got = np.stack([_np(cell.add_input(x[:, :, t])) for t in range(x.shape[2])], axis=-1)
    assert _report("conv1d_cell", sc.cell_id(c), y=fb.ratio(got, want, bound)) <= 1.0
    plain = _cell(c._replace(bias=False), {"weight": st["weight"]})
    y0 = np.stack([_np(plain.add_input(x[:, :, t])) for t in range(x.shape[2])], axis=-1)
    for s in (UP, DOWN):
        plain.start_sequence()
        ys = np.stack([_np(plain.add_input(x[:, :, t] * s)) for t in range(x.shape[2])], axis=-1)
        assert np.array_equal(ys, y0 * s)


def test_two_interleaved_cells_keep_their_own_buffers():
    ca, cb = sc.CELL_CASES[2], sc.CELL_CASES[1]
    (xa, sa), (xb, sb) = sc.cell_inputs(ca, tag=1), sc.cell_inputs(cb, tag=2)
    T = min(xa.shape[2], xb.shape[2])
    alone_a, alone_b = _cell(ca, sa), _cell(cb, sb)
    ya = [_np(alone_a.add_input(xa[:, :, t])) for t in range(T)]
    yb = [_np(alone_b.add_input(xb[:, :, t])) for t in range(T)]
    a, b = _cell(ca, sa), _cell(cb, sb)
    for t in range(T):
        assert np.array_equal(_np(a.add_input(xa[:, :, t])), ya[t])
        assert np.array_equal(_np(b.add_input(xb[:, :, t])), yb[t])


# ------------------------------------------------------------------------------------------------ expand / sinusoid
@pytest.mark.parametrize("Cc", sc.EXPAND_C)
def test_expand_sweep(Cc):
    from parakeet_amd.modules import expand
    r = sc.rng_for("expand", Cc)
    B, T = 3, 6
    x = sc.f32(r.normal(size=(B, T, Cc)))
    d = r.integers(0, 51, size=(B, T))
    d[0, 2], d[1] = 50, 0                         # durations up to 50; one utterance of all-zero durations in the batch
    got = _np(expand(x, d))
    want = sc.expand_reference(x, d)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not got[1].any()                       # the empty utterance is padding only
    empty = expand(x, np.zeros((B, T), np.int64))                                  # t_dec == 0
    assert tuple(empty.shape) == (B, 0, Cc)


@pytest.mark.parametrize("size,npos,start,omega", sc.SIN_CASES)
def test_sinusoid_sweep(size, npos, start, omega):
    from parakeet_amd.modules import sinusoid_position_encoding
    got = _np(sinusoid_position_encoding(npos, size, omega=omega, start_pos=start))
    want, bound = sc.sinusoid_reference(npos, size, omega, start)
    assert got.shape == want.shape
    assert _report("sinusoid", f"size{size}-n{npos}-start{start}-omega{omega}", table=fb.ratio(got, want, bound)) <= 1.0
