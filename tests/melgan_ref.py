"""fp64 restatement of the MelGAN / multi-band MelGAN generator with a derived error bound for the engine's evaluation (a
plain module, not a conftest; shared by tests/test_melgan_cpu.py and tests/test_melgan_gpu.py).  Modelled on
tests/hifigan_ref.py, whose transposed convolution, weight folding and bound steps it reuses.

Semantics (parakeet_amd/melgan.py; THE PARAMETER NAMES AND THE LAYOUT ARE AS RECALLED AND COULD NOT BE CHECKED AGAINST A
RELEASED CHECKPOINT).  With ``ch_i = channels >> i``, ``a`` = LeakyReLU(negative_slope), S = stacks, R = reflection padding:
  x = Conv1D(in_channels -> channels, kernel_size)(R((kernel_size - 1) / 2)(mel))                     melgan.1
  per stage i (scale s_i), q_i = 2 + i (2 + S):
    x = Conv1DTranspose(ch_i -> ch_(i+1), 2 s_i, stride s_i, padding s_i // 2 + s_i % 2, output_padding s_i % 2)(a(x))
                                                                                                      melgan.{q_i + 1}
    per stack j, d = stack_kernel_size ** j:
      t = Conv1D(k = stack_kernel_size, dilation d)(R((k - 1) / 2 d)(a(x)))                           melgan.{q_i+2+j}.stack.2
      x = Conv1D(1x1)(a(t)) + Conv1D(1x1)(x)                            ...stack.4   and   melgan.{q_i+2+j}.skip_layer
  y = Conv1D(ch_last -> out_channels, kernel_size)(R(...)(a(x)))                                      melgan.{2 + n (2 + S) + 2}
  y = tanh(y) with use_final_nonlinear_activation
R(p) needs p < length at every padded convolution: ``min_frames``.

The bound is hifigan_ref's, layer by layer, with two additions:
  reflection   a reflected operand is a COPY of an in-range value: it carries that value's bound, and the maximum the
               producer measured over the utterance still bounds it.  The bound arrays are therefore reflected with the
               operand (``rconv`` is applied to |a|, to b_a and to the ones alike).
  the stack    t: one convolution.  skip: a 1x1 convolution of the un-activated x (the engine stages it with slope 1, an
               exact identity: no rounding of an operand).  x' = Conv1x1(a(t)) + skip: the two bounds added, + one rounding
               for the addition -- the step of hifigan_ref's ``y = t + y`` with the skip's bound in place of y's.
"""
import numpy as np

import fp32_bounds as fb
from hifigan_ref import _f32_up, conv_transpose, folded
from pwg_disc_ref import conv, leaky

MATHS = ("f32", "f16x3")

CONFIGS = {
    "TINY": dict(in_channels=20, out_channels=1, channels=32, kernel_size=7, upsample_scales=(2, 3), stacks=2,
                 stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
    "MB-TINY": dict(in_channels=20, out_channels=4, channels=32, kernel_size=7, upsample_scales=(2, 3), stacks=2,
                    stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
    # an odd scale and an odd number of 32-channel groups (160 channels: five) after it, as hifigan_ref's ODD
    "ODD": dict(in_channels=24, out_channels=1, channels=320, kernel_size=3, upsample_scales=(13,), stacks=2,
                stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
    # scales (3, 3): the only small way to lengths of 256 m - 1 and 256 m + 1 at the output rate (a length is a multiple
    # of the hop) -- the frame counts below
    "S33": dict(in_channels=8, out_channels=1, channels=32, kernel_size=3, upsample_scales=(3, 3), stacks=1,
                stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
    # stack kernel 5 (pads 2 and 10), 8 input channels of a 16-wide k block, two output channels, no tanh
    "K5": dict(in_channels=16, out_channels=2, channels=16, kernel_size=5, upsample_scales=(4,), stacks=2,
               stack_kernel_size=5, negative_slope=0.1, use_final_nonlinear_activation=False),
    "FULL": dict(in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2), stacks=3,
                 stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
    "MB-FULL": dict(in_channels=80, out_channels=4, channels=384, kernel_size=7, upsample_scales=(8, 4, 2), stacks=4,
                    stack_kernel_size=3, negative_slope=0.2, use_final_nonlinear_activation=True),
}
SMALL = ("TINY", "MB-TINY", "ODD", "S33", "K5")
# the first two of every list: min_frames and min_frames + 1.
# TINY (rates 1, 2, 6): 43 frames end 2 past a 256 tile at the output rate, 128 / 129 at 0 / + 2 of it at rate 2 ... .
# S33 (rates 1, 3, 9): output rate 9 f = 513 (+1), 1026 (+2), 1791 (-1), 2304 (0) for f = 57, 114, 199, 256; the rate of
# stage 0, 3 f = 255 (-1), 258 (+2), 513 (+1), 768 (0) for f = 85, 86, 171, 256.
FRAMES = {"TINY": (4, 5, 11, 22, 43, 128, 129), "MB-TINY": (4, 5, 11, 43), "ODD": (2, 3, 20), "K5": (3, 4, 9, 65),
          "S33": (2, 3, 57, 85, 86, 114, 171, 199, 256)}
SEEDS = {"TINY": 201, "MB-TINY": 202, "ODD": 203, "S33": 204, "K5": 205, "FULL": 206, "MB-FULL": 207}


def ctor_kwargs(cfg):
    """Constructor arguments of parakeet_amd.melgan.MelGANGenerator for a configuration of this module."""
    kw = dict(cfg)
    kw["nonlinear_activation_params"] = {"negative_slope": kw.pop("negative_slope")}
    return kw


def make_mels(name, frames=None):
    """Seeded mel inputs (T'_b, C_in) float32 of a configuration, N(0, 1)."""
    rng = np.random.default_rng(SEEDS[name] + 1000)
    cin = CONFIGS[name]["in_channels"]
    return [rng.standard_normal((f, cin)).astype(np.float32) for f in (FRAMES[name] if frames is None else frames)]


def min_frames(cfg):
    """The smallest frame count at which every reflection pad is smaller than the length it pads."""
    k, sk, S = cfg["kernel_size"], cfg["stack_kernel_size"], cfg["stacks"]
    need, mul = (k - 1) // 2 + 1, 1
    for s in cfg["upsample_scales"]:
        mul *= s
        pad = (sk - 1) // 2 * sk ** (S - 1)
        need = max(need, -(-(pad + 1) // mul))
    return max(need, -(-((k - 1) // 2 + 1) // mul))


def names_of(cfg):
    """-> (input, [per stage (transposed, [(stack.2, stack.4, skip_layer) per stack])], output) parameter bases."""
    S, n = cfg["stacks"], len(cfg["upsample_scales"])
    stages = []
    for i in range(n):
        q = 2 + i * (2 + S)
        stages.append((f"melgan.{q + 1}", [(f"melgan.{q + 2 + j}.stack.2", f"melgan.{q + 2 + j}.stack.4",
                                            f"melgan.{q + 2 + j}.skip_layer") for j in range(S)]))
    return "melgan.1", stages, f"melgan.{2 + n * (2 + S) + 2}"


class Model:
    def __init__(self, cfg, state):
        self.cfg = dict(cfg)
        self.scales = list(cfg["upsample_scales"])
        self.stacks, self.sk = int(cfg["stacks"]), int(cfg["stack_kernel_size"])
        self.slope = float(np.float32(cfg.get("negative_slope", 0.2)))
        assert abs(self.slope) <= 1.0
        self.tanh = bool(cfg.get("use_final_nonlinear_activation", True))
        self.hop = int(np.prod(self.scales))
        self.first, self.stage_names, self.last = names_of(cfg)
        self.names = [self.first, self.last]
        for up, stacks in self.stage_names:
            self.names.append(up)
            for trio in stacks:
                self.names.extend(trio)
        self.w = {n: folded(state, n).astype(np.float64) for n in self.names}
        self.b = {n: np.asarray(state[n + ".bias"], np.float64).reshape(-1) for n in self.names}


def rconv(x, w, d=1):
    """x (Cin, T), w (Cout, Cin, k), dilation d, REFLECTION padding (k - 1) / 2 * d (< T) -> (Cout, T)."""
    p = (w.shape[2] - 1) // 2 * d
    if p == 0:
        return conv(x, w, d)
    assert p < x.shape[1], "reflection needs its pad smaller than the length"
    return conv(np.pad(x, ((0, 0), (p, p)), mode="reflect"), w, d)[:, p:-p]


def _linear(model, name, h, b, slope, maths, d=1, s=None, reflect=False, mut=None):
    """One convolution ``name`` on the input h (pre-activation, bound b per math): -> (pre, {math: bound}); hifigan_ref's
    step with the boundary rule as a parameter.  ``mut`` = "zero": the mutant that zero-pads a reflecting convolution."""
    w, bias = model.w[name], model.b[name][:, None]
    aw = np.abs(w)
    if s is None:
        f = rconv if (reflect and mut != "zero") else conv
        op = lambda z, ww: f(z, ww, d)                                                       # noqa: E731
        K = w.shape[1] * w.shape[2]
        sum_w = aw.reshape(w.shape[0], -1).sum(1)[:, None]
        ones = np.ones((1,) + w.shape[1:])
    else:
        op = lambda z, ww: conv_transpose(z, ww, s)                                          # noqa: E731
        K = 2 * w.shape[0]
        sum_w = np.max([(aw[:, :, k0] + aw[:, :, k0 + s]).sum(0) for k0 in range(s)], axis=0)[:, None]
        ones = np.ones((w.shape[0], 1, w.shape[2]))
    a = h if slope is None else leaky(h, slope)
    pre = op(a, w) + bias
    if not maths:
        return pre, {}
    p_abs = op(np.abs(a), aw)
    out = {}
    for m in maths:
        ba = b[m] if slope is None else fb.epilogue_step(a, b[m], 1)
        through = op(ba, aw)
        absprod = p_abs + through
        if m == "f16x3":
            sum_a = op(np.abs(a) + ba, ones)
            amax = float((np.abs(h) + b[m]).max()) * max(1.0, abs(slope if slope is not None else 1.0))
            own = fb.split_dot_bound(absprod, K, sum_a, sum_w, fb.act_scale(_f32_up(amax)), fb.weight_scale(aw.max()), bias)
        else:
            own = fb.dot_bound(absprod, K, bias)
        out[m] = fb.epilogue_step(pre, through + own, 1)
    return pre, out


def _stack(model, trio, j, x, b, maths, mut=None, rec=None):
    """One residual stack from x with bound b -> (x', bound); ``rec`` receives t, the skip and x' (the engine's launches)."""
    d = model.sk ** j
    if mut == "dil" and j == model.stacks - 1:
        d += 1
    t, bt = _linear(model, trio[0], x, b, model.slope, maths, d=d, reflect=True, mut=mut)
    sk, bs = _linear(model, trio[2], x if mut != "askip" else leaky(x, model.slope), b, None, maths)
    u, bu = _linear(model, trio[1], t, bt, model.slope, maths)
    y = u + sk
    by = {m: fb.epilogue_step(y, bu[m] + bs[m], 1) for m in maths}
    if rec is not None:
        rec.extend([t, sk, y])
    return y, by


def _stage(model, i, x, b, maths, mut=None, rec=None):
    up, stacks = model.stage_names[i]
    x, b = _linear(model, up, x, b, model.slope, maths, s=model.scales[i])
    if rec is not None:
        rec.append(x)
    for j, trio in enumerate(stacks):
        x, b = _stack(model, trio, j, x, b, maths, mut if i == 0 else None, rec)
    return x, b


def _final(model, x, b, maths, mut=None):
    pre, b = _linear(model, model.last, x, b, None if mut == "noact" else model.slope, maths, reflect=True)
    if model.tanh:
        return np.tanh(pre), {m: fb.tanh_bound(pre, b[m]) for m in maths}
    return pre, b


def forward(model, mel=None, maths=MATHS, mut=None, first=0, x0=None, last=None):
    """mel (T', C_in) -> dict: ``stages`` (every stage's output, (ch_{i+1}, L_i) each), ``out`` (out_channels, T' hop),
    ``taps`` (what every launch before the output convolution writes), and per math ``b_stages`` / ``b_out``.  ``first`` > 0
    with ``x0``: start at stage ``first`` from that input with a zero bound (``first`` = number of stages: only the output
    convolution).  ``last``: stop after that stage.  ``mut``: a mutant's name (``zero``: the reflecting convolutions of
    stage 0's stacks zero-pad; ``askip``: the skip convolution sees a(x); ``dil``; ``noact``; ``inzero``: the input
    convolution zero-pads)."""
    n = len(model.scales)
    taps = []
    if first == 0:
        h = np.asarray(mel, np.float64).T
        b = {m: np.zeros_like(h) for m in maths}
        x, b = _linear(model, model.first, h, b, None, maths, reflect=True, mut="zero" if mut == "inzero" else None)
        taps.append(x)
    else:
        x = np.asarray(x0, np.float64)
        b = {m: np.zeros_like(x) for m in maths}
    stages, b_stages = [], {m: [] for m in maths}
    for i in range(first, n):
        x, b = _stage(model, i, x, b, maths, mut, taps)
        stages.append(x)
        for m in maths:
            b_stages[m].append(b[m])
        if last is not None and i == last:
            return {"stages": stages, "b_stages": b_stages, "out": None, "b_out": {}}
    out, b = _final(model, x, b, maths, mut)
    return {"stages": stages, "b_stages": b_stages, "out": out, "b_out": b, "taps": taps}


def global_ratio(ref, stages, out, math):
    rs = [fb.ratio(g, w, b) for g, w, b in zip(stages, ref["stages"], ref["b_stages"][math])]
    return max(rs + [fb.ratio(out, ref["out"], ref["b_out"][math])])


def local_ratio(model, mel, stages, out, math):
    """The derivation restarted at every stage from the evaluation's OWN output of the stage before."""
    n = len(model.scales)
    res = []
    for i in range(n):
        if i == 0:
            r = forward(model, mel, maths=(math,), last=0)
        else:
            r = forward(model, maths=(math,), first=i, x0=stages[i - 1], last=i)
        res.append(fb.ratio(stages[i], r["stages"][0], r["b_stages"][math][0]))
    r = forward(model, maths=(math,), first=n, x0=stages[n - 1])
    res.append(fb.ratio(out, r["out"], r["b_out"][math]))
    return res


def conv_ratios(model, mel, taps, out, math):
    """The derivation restarted at EVERY LAUNCH: ``taps`` is what each launch of the engine wrote (float32, in its order:
    input convolution; per stage the transposed convolution, then per stack t, the skip, x'), each compared with the exact
    result of its own step applied to the taps it read, under the bound of that one step.  -> [ratio per launch ..., ratio
    of the output]."""
    mm = (math,)
    f64 = lambda a: np.asarray(a, np.float64)                   # noqa: E731
    zero = lambda a: {math: np.zeros_like(a)}                    # noqa: E731
    res, k = [], 0
    h = f64(mel).T
    pre, b = _linear(model, model.first, h, zero(h), None, mm, reflect=True)
    res.append(fb.ratio(taps[0], pre, b[math]))
    x, k = f64(taps[0]), 1
    for i, s in enumerate(model.scales):
        up, stacks = model.stage_names[i]
        pre, b = _linear(model, up, x, zero(x), model.slope, mm, s=s)
        res.append(fb.ratio(taps[k], pre, b[math]))
        x, k = f64(taps[k]), k + 1
        for j, trio in enumerate(stacks):
            pre, b = _linear(model, trio[0], x, zero(x), model.slope, mm, d=model.sk ** j, reflect=True)
            res.append(fb.ratio(taps[k], pre, b[math]))
            t, k = f64(taps[k]), k + 1
            pre, b = _linear(model, trio[2], x, zero(x), None, mm)
            res.append(fb.ratio(taps[k], pre, b[math]))
            sk, k = f64(taps[k]), k + 1
            pre, b = _linear(model, trio[1], t, zero(t), model.slope, mm)
            y = pre + sk
            res.append(fb.ratio(taps[k], y, fb.epilogue_step(y, b[math], 1)))
            x, k = f64(taps[k]), k + 1
    assert k == len(taps)
    want, b = _final(model, x, zero(x), mm)
    res.append(fb.ratio(out, want, b[math]))
    return res


def mutant(model, mel, name):
    """(stages, out, taps) of a subtly wrong evaluation (forward's ``mut``)."""
    r = forward(model, mel, maths=(), mut=name)
    return r["stages"], r["out"], r["taps"]


def torch_chain(cfg, state, mels, device="cpu", dtype=None):
    """The same stack as torch.nn.functional calls (pad(mode="reflect"), conv1d, conv_transpose1d, leaky_relu; float64 by
    default) on ``device``: list of (T'_b, C_in) -> list of (stages, out) as numpy.  An independent statement of the
    semantics for the restatement to be checked against, and the float64 reference of the full-width runs."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    m = Model(cfg, state)
    W = {n: torch.as_tensor(m.w[n], dtype=dtype, device=device) for n in m.names}
    B = {n: torch.as_tensor(m.b[n], dtype=dtype, device=device) for n in m.names}
    k, sk = cfg["kernel_size"], m.sk
    res = []
    for mel in mels:
        x = torch.as_tensor(np.asarray(mel), dtype=dtype, device=device).T[None]
        x = F.conv1d(F.pad(x, ((k - 1) // 2,) * 2, mode="reflect"), W[m.first], B[m.first])
        stages = []
        for i, s in enumerate(m.scales):
            up, stacks = m.stage_names[i]
            x = F.conv_transpose1d(F.leaky_relu(x, m.slope), W[up], B[up], stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
            for j, (c2, c4, skip) in enumerate(stacks):
                d = sk ** j
                t = F.conv1d(F.pad(F.leaky_relu(x, m.slope), ((sk - 1) // 2 * d,) * 2, mode="reflect"), W[c2], B[c2], dilation=d)
                x = F.conv1d(F.leaky_relu(t, m.slope), W[c4], B[c4]) + F.conv1d(x, W[skip], B[skip])
            stages.append(x[0].cpu().numpy())
        y = F.conv1d(F.pad(F.leaky_relu(x, m.slope), ((k - 1) // 2,) * 2, mode="reflect"), W[m.last], B[m.last])
        if m.tanh:
            y = torch.tanh(y)
        res.append((stages, y[0].cpu().numpy()))
    return res
