"""fp64 restatement of the HiFi-GAN generator (Kong et al. 2020) with a derived error bound for the engine's evaluation (a
plain module, not a conftest; shared by tests/test_hifigan_cpu.py and tests/test_hifigan_gpu.py).

Semantics (parakeet_amd/hifigan.py; the parameter names and the slope 0.01 before ``output_conv`` are as recalled and could
not be checked against a real checkpoint).  With ``ch_i = channels >> i`` and ``a_s`` = LeakyReLU(s):
  x = Conv1D(in_channels -> channels, kernel_size)(mel)
  per stage i: x = Conv1DTranspose(ch_i -> ch_{i+1}, 2 s_i, stride s_i, padding s_i // 2 + s_i % 2, output_padding
               s_i % 2)(a_slope(x)); per residual block j, y = x, per dilation d: t = Conv1D(k_j, dilation d)(a_slope(y)),
               with use_additional_convs t = Conv1D(k_j)(a_slope(t)), y = t + y;  x = (sum_j y_j) / nb
  wav = tanh(Conv1D(ch_last -> 1, kernel_size)(a_0.01(x)))
Every convolution zero-pads its own input at the two ends of the utterance.  Weights: the float32 ``weight``, or ``weight_g *
weight_v / ||weight_v||`` (norm over all axes but 0, ``weight_g`` of any shape with that many elements) folded in float64 and
rounded once to float32, which is what the engine uses; slopes are their float32 values.

The transposed convolution is evaluated per output: with p = s // 2 + s % 2, k0 = (n + p) mod s, m0 = (n + p - k0) / s,
  y[:, n] = b + W[:, :, k0]^T x[:, m0] + W[:, :, k0 + s]^T x[:, m0 - 1]   (terms with m outside [0, L) dropped).

The bound, layer by layer (nothing in it comes from an observed error).  With b the bound of a convolution's input h (0 for
the mel, or for a stage input the evaluation is restarted from) and a = a_s(h) the operand:
  operand         b_a = b + u (|a| + b): LeakyReLU is 1-Lipschitz for |s| <= 1, one rounding for the product with the slope
  pre-activation  |W| . b_a                    the input's error through the linear map
                  + the product's own error on the operands actually used, |a| + b_a:
                      "f32":   fp32_bounds.dot_bound(|W| . (|a| + b_a), K, bias), K = k C_in (2 C_in for the transposed one)
                      "f16x3": fp32_bounds.split_dot_bound(...) with the weight scale of the tensor and the activation scale
                               of the LARGEST |h| + b of the whole utterance times max(1, |s|) -- the kernel takes the
                               maximum of its own values of h over the utterance, which is at most that, and the bound
                               grows with the maximum
                  + one rounding for the bias addition (epilogue_step)
  y = t + y       the two bounds added, + one rounding
  block mean      y / nb: two roundings (the rounded 1 / nb and the product); the sum with the running mean: one
  wav             fp32_bounds.tanh_bound
The bound is carried through |W|, which amplifies by a row's 1-norm where the signal grows by its 2-norm: sqrt(k C) per
convolution for the dense rows used here.  Over a whole model it therefore exceeds the waveform itself (DESIGN.md 4.1d has
the figures) and is of use only as a sanity bar.  The SAME derivation restarted at every stage from the engine's own
output of the stage before (``local_ratio``: the engine computed stage i from exactly those float32 values, so the bound of
one stage applies) is still 10 - 20 % of the signal, ten convolutions deep.  The bound that tells a wrong kernel from a right
one is the derivation restarted at EVERY CONVOLUTION from the taps of pk_hfg_debug_conv (``conv_ratios``).
"""
import numpy as np

import fp32_bounds as fb
from pwg_disc_ref import conv, leaky

MATHS = ("f32", "f16x3")
OUTPUT_SLOPE = float(np.float32(0.01))   # LeakyReLU's default: the activation before output_conv takes no arguments

_V = dict(in_channels=80, kernel_size=7, resblock_kernel_sizes=(3, 7, 11), resblock_dilations=((1, 3, 5),) * 3,
          use_additional_convs=True, negative_slope=0.1)
CONFIGS = {
    "TINY": dict(in_channels=20, channels=32, kernel_size=7, upsample_scales=(2, 3), resblock_kernel_sizes=(3, 5),
                 resblock_dilations=((1, 3), (1, 2)), use_additional_convs=True, negative_slope=0.1),
    "V2": dict(_V, channels=128, upsample_scales=(8, 8, 2, 2)),
    "CS": dict(_V, channels=128, upsample_scales=(5, 5, 4, 3)),
    "V3": dict(_V, channels=256, upsample_scales=(8, 8, 4), resblock_kernel_sizes=(3, 5, 7),
               resblock_dilations=((1, 2), (2, 6), (3, 12)), use_additional_convs=False),
    "V1": dict(_V, channels=512, upsample_scales=(8, 8, 2, 2)),
    # an odd number of 32-channel output groups (160 channels: five, one per workgroup) under a large odd scale: 5 x 13 = 65
    # scale maxima per tile of the transposed convolution, the most the kernel's slot layout meets among the small shapes
    "ODD": dict(in_channels=24, channels=320, kernel_size=3, upsample_scales=(13,), resblock_kernel_sizes=(3, 5),
                resblock_dilations=((1,), (2,)), use_additional_convs=False, negative_slope=0.1),
}
FRAMES = {"TINY": (1, 2, 10, 11, 21, 22, 43), "V2": (1, 2, 5, 33), "CS": (1, 2, 5, 33), "V3": (1, 2, 5, 33), "V1": (1, 4),
          "ODD": (1, 20)}
SEEDS = {"TINY": 101, "V2": 102, "CS": 103, "V3": 104, "V1": 105, "ODD": 106}


def ctor_kwargs(cfg):
    """Constructor arguments of parakeet_amd.hifigan.HiFiGANGenerator for a configuration of this module."""
    kw = dict(cfg)
    kw["nonlinear_activation_params"] = {"negative_slope": kw.pop("negative_slope")}
    kw["upsample_kernel_sizes"] = tuple(2 * s for s in cfg["upsample_scales"])
    return kw


def make_mels(name, frames=None):
    """Seeded mel inputs (T'_b, C_in) float32 of a configuration, N(0, 1)."""
    rng = np.random.default_rng(SEEDS[name] + 1000)
    cin = CONFIGS[name]["in_channels"]
    return [rng.standard_normal((f, cin)).astype(np.float32) for f in (FRAMES[name] if frames is None else frames)]


def folded(state, base):
    """float32 weight of convolution ``base`` as the engine folds it (norm over all axes but 0, for both layouts)."""
    if base + ".weight" in state:
        return np.asarray(state[base + ".weight"], np.float32)
    g = np.asarray(state[base + ".weight_g"], np.float64).reshape(-1)
    v = np.asarray(state[base + ".weight_v"], np.float64)
    norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1))
    return (v * (g / norm)[:, None, None]).astype(np.float32)


class Model:
    def __init__(self, cfg, state):
        self.cfg = dict(cfg)
        self.scales = list(cfg["upsample_scales"])
        self.rks = list(cfg["resblock_kernel_sizes"])
        self.dils = [list(d) for d in cfg["resblock_dilations"]]
        self.additional = bool(cfg.get("use_additional_convs", True))
        self.slope = float(np.float32(cfg.get("negative_slope", 0.1)))
        assert abs(self.slope) <= 1.0
        self.nb = len(self.rks)
        self.hop = int(np.prod(self.scales))
        self.names = ["input_conv", "output_conv.1"]
        for i in range(len(self.scales)):
            self.names.append(f"upsamples.{i}.1")
            for j in range(self.nb):
                for n in range(len(self.dils[j])):
                    self.names.append(f"blocks.{i * self.nb + j}.convs1.{n}.1")
                    if self.additional:
                        self.names.append(f"blocks.{i * self.nb + j}.convs2.{n}.1")
        self.w = {n: folded(state, n).astype(np.float64) for n in self.names}
        self.b = {n: np.asarray(state[n + ".bias"], np.float64).reshape(-1) for n in self.names}


def conv_transpose(x, w, s, swap=False):
    """x (Cin, L), w (Cin, Cout, 2 s), stride s, padding s // 2 + s % 2, output_padding s % 2 -> (Cout, L s), by the
    per-output identity of the docstring.  ``swap``: the mutant that exchanges the two taps."""
    L, p = x.shape[1], s // 2 + s % 2
    xp = np.concatenate([np.zeros((x.shape[0], 1)), x, np.zeros((x.shape[0], 1))], axis=1)   # xp[:, m + 1] = x[:, m]
    y = np.zeros((w.shape[1], L * s))
    for k0 in range(s):
        a0, a1 = w[:, :, k0].T, w[:, :, k0 + s].T
        if swap:
            a0, a1 = a1, a0
        m0 = np.arange(0, L + 1)
        n = m0 * s + k0 - p
        ok = (n >= 0) & (n < L * s)
        m0, n = m0[ok], n[ok]
        y[:, n] = a0 @ xp[:, m0 + 1] + a1 @ xp[:, m0]
    return y


def _f32_up(v):
    """the smallest float32 >= v"""
    f = np.float32(v)
    return f if float(f) >= float(v) else np.nextafter(f, np.float32(np.inf))


def _linear(model, name, h, b, slope, maths, d=1, s=None, swap=False):
    """One convolution ``name`` on the input h (pre-activation, bound b per math): -> (pre, {math: bound})."""
    w, bias = model.w[name], model.b[name][:, None]
    aw = np.abs(w)
    if s is None:
        op = lambda z, ww: conv(z, ww, d)                                                    # noqa: E731
        K = w.shape[1] * w.shape[2]
        sum_w = aw.reshape(w.shape[0], -1).sum(1)[:, None]
        ones = np.ones((1,) + w.shape[1:])
    else:
        op = lambda z, ww: conv_transpose(z, ww, s, swap)                                    # noqa: E731
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


def _stage(model, i, x, b, maths, mut=None, rec=None):
    """Stage i from its input x (ch_i, L) with bound b -> (output (ch_{i+1}, L s_i), {math: bound}).  ``rec``: a list that
    receives what every launch of the engine writes, in its order (pk_hfg_debug_conv)."""
    s, nb = model.scales[i], model.nb
    rec = [] if rec is None else rec
    x, b = _linear(model, f"upsamples.{i}.1", x, b, model.slope, maths, s=s, swap=(mut == "tapswap" and i == 0))
    rec.append(x)
    total, b_total = None, None
    div = nb + (1 if mut == "nb_plus" else -1 if mut == "nb_minus" else 0) if i == 0 else nb
    for j in range(nb):
        y, by = x, b
        for n, d in enumerate(model.dils[j]):
            if mut == "dil" and i == 0 and j == 0 and n == len(model.dils[j]) - 1:
                d += 1
            blk = f"blocks.{i * nb + j}"
            t, bt = _linear(model, f"{blk}.convs1.{n}.1", y, by, model.slope, maths, d=d)
            if model.additional:
                rec.append(t)
                t, bt = _linear(model, f"{blk}.convs2.{n}.1", t, bt, model.slope, maths, d=1)
            yn = t + y
            by = {m: fb.epilogue_step(yn, bt[m] + by[m], 1) for m in maths}
            y = yn
            if n < len(model.dils[j]) - 1:
                rec.append(y)
        part = y / div
        bp = {m: fb.epilogue_step(part, by[m] / nb, 2) for m in maths}
        if total is None:
            total, b_total = part, bp
        else:
            total = total + part
            b_total = {m: fb.epilogue_step(total, b_total[m] + bp[m], 1) for m in maths}
        rec.append(total)
    return total, b_total


def forward(model, mel=None, maths=MATHS, mut=None, first=0, x0=None, last=None):
    """mel (T', C_in) -> dict: ``stages`` (every stage's output after its block mean, (ch_{i+1}, L_i) each), ``wav`` (T' hop,),
    and per math ``b_stages`` / ``b_wav`` (and ``pre`` / ``b_pre``: output_conv's pre-activation), the bounds of the docstring.
    ``first`` > 0 with ``x0`` (ch_first, L): start at stage ``first`` from that input with a zero bound (``first`` = number of
    stages: only the output convolution).  ``last``: stop after that stage (no wav).  ``mut``: a mutant's name."""
    S = len(model.scales)
    taps = []
    if first == 0:
        h = np.asarray(mel, np.float64).T
        b = {m: np.zeros_like(h) for m in maths}
        x, b = _linear(model, "input_conv", h, b, None, maths)
        taps.append(x)
    else:
        x = np.asarray(x0, np.float64)
        b = {m: np.zeros_like(x) for m in maths}
    stages, b_stages = [], {m: [] for m in maths}
    for i in range(first, S):
        x, b = _stage(model, i, x, b, maths, mut, taps)
        stages.append(x)
        for m in maths:
            b_stages[m].append(b[m])
        if last is not None and i == last:
            return {"stages": stages, "b_stages": b_stages, "wav": None, "b_wav": {}}
    pre, b = _linear(model, "output_conv.1", x, b, 0.1 if mut == "outslope" else OUTPUT_SLOPE, maths)
    return {"stages": stages, "b_stages": b_stages, "wav": np.tanh(pre[0]), "pre": pre[0], "taps": taps,
            "b_pre": {m: b[m][0] for m in maths},
            "b_wav": {m: fb.tanh_bound(pre[0], b[m][0]) for m in maths}}


def abias_mutant(model, mel, pad=24):
    """The mutant whose positions outside the utterance hold a(bias) and what follows from it instead of 0: the stack on
    the mel extended by ``pad`` zero frames on both sides, cropped.  -> (stages, wav, taps)"""
    mel = np.asarray(mel, np.float64)
    z = np.zeros((pad, mel.shape[1]))
    r = forward(model, np.concatenate([z, mel, z]), maths=())
    T, Tp = len(mel), len(mel) + 2 * pad

    def crop(a):
        rate = a.shape[-1] // Tp
        return a[..., pad * rate:(pad + T) * rate]
    return [crop(a) for a in r["stages"]], crop(r["wav"]), [crop(a) for a in r["taps"]]


def mutant(model, mel, name):
    """(stages, wav, taps) of a subtly wrong evaluation: ``outslope`` (0.1 before output_conv), ``nb_plus`` / ``nb_minus`` (the
    block sum of stage 0 divided by nb +- 1), ``tapswap`` (the two taps of the first transposed convolution exchanged),
    ``abias``, ``dil`` (the last dilation of the first block of stage 0 off by one)."""
    if name == "abias":
        return abias_mutant(model, mel)
    r = forward(model, mel, maths=(), mut=name)
    return r["stages"], r["wav"], r["taps"]


def global_ratio(ref, stages, wav, math):
    """max |got - exact| / bound over every stage tap and the waveform, against ``ref = forward(model, mel)``."""
    rs = [fb.ratio(g, w, b) for g, w, b in zip(stages, ref["stages"], ref["b_stages"][math])]
    return max(rs + [fb.ratio(wav, ref["wav"], ref["b_wav"][math])])


def local_ratio(model, mel, stages, wav, math):
    """The derivation restarted at every stage from the evaluation's OWN output of the stage before (float32 values, exact
    inputs of what it computed next): -> [ratio of stage 0 from the mel, stage 1 from stage 0, ..., wav from the last]."""
    S = len(model.scales)
    out = []
    for i in range(S):
        if i == 0:
            r = forward(model, mel, maths=(math,), last=0)
        else:
            r = forward(model, maths=(math,), first=i, x0=stages[i - 1], last=i)
        out.append(fb.ratio(stages[i], r["stages"][0], r["b_stages"][math][0]))
    r = forward(model, maths=(math,), first=S, x0=stages[S - 1])
    out.append(fb.ratio(wav, r["wav"], r["b_wav"][math]))
    return out


def conv_ratios(model, mel, taps, wav, math):
    """The derivation restarted at EVERY CONVOLUTION: ``taps`` is what each launch of the engine wrote (float32, in its
    order: pk_hfg_debug_conv), and each one is compared with the exact result of its own step -- one convolution and its
    epilogue -- applied to the taps it read, under the bound of that one step.  -> [ratio per launch ..., ratio of wav].
    One step's bound is a few 1e-5 of |W| . |a|: nothing a kernel can do wrong hides under it."""
    mm = (math,)
    f64 = lambda a: np.asarray(a, np.float64)                   # noqa: E731
    zero = lambda a: {math: np.zeros_like(a)}                    # noqa: E731
    out, k, nb = [], 0, model.nb
    h = f64(mel).T
    pre, b = _linear(model, "input_conv", h, zero(h), None, mm)
    out.append(fb.ratio(taps[0], pre, b[math]))
    x, k = f64(taps[0]), 1
    for i, s in enumerate(model.scales):
        pre, b = _linear(model, f"upsamples.{i}.1", x, zero(x), model.slope, mm, s=s)
        out.append(fb.ratio(taps[k], pre, b[math]))
        X, k = f64(taps[k]), k + 1
        run = None
        for j in range(nb):
            y = X
            for n, d in enumerate(model.dils[j]):
                blk = f"blocks.{i * nb + j}"
                pre, b = _linear(model, f"{blk}.convs1.{n}.1", y, zero(y), model.slope, mm, d=d)
                if model.additional:
                    out.append(fb.ratio(taps[k], pre, b[math]))
                    t, k = f64(taps[k]), k + 1
                    pre, b = _linear(model, f"{blk}.convs2.{n}.1", t, zero(t), model.slope, mm, d=1)
                yn = pre + y
                by = fb.epilogue_step(yn, b[math], 1)
                if n < len(model.dils[j]) - 1:
                    out.append(fb.ratio(taps[k], yn, by))
                    y, k = f64(taps[k]), k + 1
                else:
                    part = yn / nb
                    bp = fb.epilogue_step(part, by / nb, 2)
                    if run is not None:
                        part = run + part
                        bp = fb.epilogue_step(part, bp, 1)
                    out.append(fb.ratio(taps[k], part, bp))
                    run, k = f64(taps[k]), k + 1
        x = run
    assert k == len(taps)
    pre, b = _linear(model, "output_conv.1", x, zero(x), OUTPUT_SLOPE, mm)
    out.append(fb.ratio(wav, np.tanh(pre[0]), fb.tanh_bound(pre[0], b[math][0])))
    return out


def output_conv_split(model, x, drop_lo=False):
    """output_conv on the stage output x evaluated as the engine's split product, through fb.split_emulation -> pre (L,).
    ``drop_lo``: the mutant that uses the hi parts alone (both operands rounded to their fp16 hi part first, which leaves
    the emulation's lo terms exactly zero)."""
    w = model.w["output_conv.1"]
    k, c = w.shape[2], (w.shape[2] - 1) // 2
    a = leaky(np.asarray(x, np.float64), OUTPUT_SLOPE).astype(np.float32)
    ap = np.pad(a, ((0, 0), (c, c)))
    L = a.shape[1]
    A = np.stack([ap[:, t:t + L] for t in range(k)], axis=0).transpose(2, 1, 0).reshape(L, -1)     # (L, C k): [ci][t]
    Wm = w[0].reshape(-1, 1).astype(np.float32)
    sa = np.full((1, 1), float(fb.act_scale(_f32_up(np.abs(x).max()))))
    sw = np.full((1, 1), float(fb.weight_scale(np.abs(w).max())))
    if drop_lo:
        A = ((A.astype(np.float64) * sa).astype(np.float16).astype(np.float64) / sa).astype(np.float32)
        Wm = ((Wm.astype(np.float64) * sw).astype(np.float16).astype(np.float64) / sw).astype(np.float32)
    acc = fb.split_emulation(A, Wm, sa, sw)[:, 0]
    return (acc + np.float32(model.b["output_conv.1"][0])).astype(np.float32)


def torch_chain(cfg, state, mels, device="cpu", dtype=None):
    """The same stack as torch.nn.functional calls (conv1d / conv_transpose1d, float64 by default) on ``device``: list of
    (T'_b, C_in) -> list of (stages, wav) as numpy.  An independent statement of the semantics for the restatement to be
    checked against, and the float64 reference of the one full-size run."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    m = Model(cfg, state)
    W = {n: torch.as_tensor(m.w[n], dtype=dtype, device=device) for n in m.names}
    B = {n: torch.as_tensor(m.b[n], dtype=dtype, device=device) for n in m.names}
    k = cfg["kernel_size"]
    res = []
    for mel in mels:
        x = torch.as_tensor(np.asarray(mel), dtype=dtype, device=device).T[None]
        x = F.conv1d(x, W["input_conv"], B["input_conv"], padding=(k - 1) // 2)
        stages = []
        for i, s in enumerate(m.scales):
            n_ = f"upsamples.{i}.1"
            x = F.conv_transpose1d(F.leaky_relu(x, m.slope), W[n_], B[n_], stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
            tot = None
            for j, kj in enumerate(m.rks):
                y = x
                for n, d in enumerate(m.dils[j]):
                    blk = f"blocks.{i * m.nb + j}"
                    t = F.conv1d(F.leaky_relu(y, m.slope), W[f"{blk}.convs1.{n}.1"], B[f"{blk}.convs1.{n}.1"],
                                 padding=(kj - 1) // 2 * d, dilation=d)
                    if m.additional:
                        t = F.conv1d(F.leaky_relu(t, m.slope), W[f"{blk}.convs2.{n}.1"], B[f"{blk}.convs2.{n}.1"],
                                     padding=(kj - 1) // 2)
                    y = t + y
                tot = y if tot is None else tot + y
            x = tot / m.nb
            stages.append(x[0].cpu().numpy())
        wav = torch.tanh(F.conv1d(F.leaky_relu(x, OUTPUT_SLOPE), W["output_conv.1"], B["output_conv.1"], padding=(k - 1) // 2))
        res.append((stages, wav[0, 0].cpu().numpy()))
    return res
