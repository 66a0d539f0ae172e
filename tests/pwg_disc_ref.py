"""fp64 restatement of the reference's PWGDiscriminator with a derived error bound for the engine's evaluation (a plain
module, not a conftest; shared by tests/test_pwg_disc_cpu.py and tests/test_pwg_disc_gpu.py).

Semantics (parakeet/models/parallel_wavegan/parallel_wavegan.py:554-614): ``layers - 1`` blocks of ``Conv1D(k, dilation d_i,
padding (k - 1) / 2 * d_i)`` + ``LeakyReLU(slope)``, ``d_0 = 1`` and ``d_i = i`` for ``dilation_factor == 1`` else
``dilation_factor ** i``, then ``Conv1D(conv_channels -> 1, k, dilation 1)`` without an activation.  Every conv zero-pads its
own input at the two ends of the utterance.  The evaluator's MSE terms (parallel_wavegan_updater.py:192-223) are means of
``(p - 1)^2`` and ``p^2`` over the logits.  Weights: the float32 ``weight``, or ``weight_g * weight_v / ||weight_v||`` folded
in float64 and rounded once to float32, which is what the engine is handed at finalize; the slope is its float32 value.

The bound, layer by layer (nothing in it comes from an observed error).  With b_l the bound of block l's input (b = 0 for the
waveform itself) and x the exact activation:
  pre-activation  |W| . b_l                    the input's error through the linear map
                  + the product's own error on the operands actually used, |x| + b_l:
                      "f32":   fp32_bounds.dot_bound(|W| . (|x| + b), K = k * C_in, bias)            (every layer)
                      "f16x3": fp32_bounds.split_dot_bound(...) for the C -> C blocks, with the weight scale of the tensor
                               and the activation scale of the LARGEST |x| + b of the whole utterance -- the kernel measures
                               the maximum of one window, which is at most that, and the bound grows with the maximum; block
                               0 and the output conv are fp32 FMAs in both maths
                  + one rounding for the bias addition (epilogue_step; dot_bound already counts one, this is spare)
  LeakyReLU       1-Lipschitz for |slope| <= 1: the bound passes; + one rounding for the multiply by the slope
  logits          the output conv as a pre-activation
  loss sums       e = p - 1: b_e = b_p + u (|e| + b_p);  e^2: 2 |e| b_e + b_e^2 + u (|e| + b_e)^2;  p^2 alike;
                  sum of the term bounds + gamma * sum (term + its bound), gamma = (tile + 8) u: a tile's terms are added in
                  fp32 in some order, the tiles in fp64 (as stft_loss_ref.sums_with_bound).
"""
import numpy as np

import fp32_bounds as fb

MATHS = ("f32", "f16x3")


def dilations(layers, dilation_factor):
    """Dilation of the ``layers - 1`` hidden blocks (:571-577)."""
    return [1 if i == 0 else (i if dilation_factor == 1 else dilation_factor ** i) for i in range(layers - 1)]


def halo(cfg):
    """Receptive field per side: (k - 1) / 2 * (sum of the hidden dilations + 1)."""
    return (cfg["kernel_size"] - 1) // 2 * (sum(dilations(cfg["layers"], cfg["dilation_factor"])) + 1)


def folded(state, i):
    """float32 weight of conv ``conv_layers.{2i}`` as the engine folds it."""
    base = f"conv_layers.{2 * i}"
    if base + ".weight" in state:
        return np.asarray(state[base + ".weight"], np.float32)
    g = np.asarray(state[base + ".weight_g"], np.float64).reshape(-1)
    v = np.asarray(state[base + ".weight_v"], np.float64)
    norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1))
    return (v * (g / norm)[:, None, None]).astype(np.float32)


class Model:
    def __init__(self, cfg, state):
        self.cfg = dict(cfg)
        L = cfg["layers"]
        self.k = cfg["kernel_size"]
        self.slope = float(np.float32(cfg.get("negative_slope", 0.2)))
        assert abs(self.slope) <= 1.0
        self.dil = dilations(L, cfg["dilation_factor"]) + [1]
        self.w = [folded(state, i).astype(np.float64) for i in range(L)]
        self.b = [np.asarray(state[f"conv_layers.{2 * i}.bias"], np.float64).reshape(-1) if cfg.get("bias", True)
                  else np.zeros(self.w[i].shape[0]) for i in range(L)]
        self.halo = (self.k - 1) // 2 * sum(self.dil)


def conv(x, w, d):
    """x (Cin, T), w (Cout, Cin, k), dilation d, zero padding (k - 1) / 2 * d -> (Cout, T)."""
    k, T = w.shape[2], x.shape[1]
    c = (k - 1) // 2
    y = np.zeros((w.shape[0], T))
    taps = np.ascontiguousarray(np.moveaxis(w, 2, 0))   # (k, Cout, Cin): a strided w[:, :, t] would miss the BLAS path
    for t in range(k):
        s = (t - c) * d           # y[:, p] += w[:, :, t] @ x[:, p + s]
        lo, hi = max(0, -s), min(T, T - s)
        if hi > lo:
            y[:, lo:hi] += taps[t] @ x[:, lo + s:hi + s]
    return y


def leaky(v, slope):
    return np.where(v > 0, v, v * slope)


def forward(model, x, maths=MATHS, keep=True, dil=None, last_activation=False):
    """x (T,) -> dict: ``acts`` (the activation after every hidden block, (C, T) each; empty unless ``keep``), ``logits``
    (T,), and per math in ``maths`` ``b_acts`` / ``b_logits``: the bounds of the docstring.  ``dil`` and ``last_activation``
    are the mutants' handles."""
    dil = model.dil if dil is None else dil
    L = len(model.w)
    h = np.asarray(x, np.float64).reshape(1, -1)
    b = {m: np.zeros_like(h) for m in maths}
    acts, b_acts = [], {m: [] for m in maths}
    for i in range(L):
        w, bias = model.w[i], model.b[i][:, None]
        aw = np.abs(w)
        K = w.shape[1] * w.shape[2]
        pre = conv(h, w, dil[i]) + bias
        p_abs = conv(np.abs(h), aw, dil[i])
        for m in maths:
            through = conv(b[m], aw, dil[i])
            absprod = p_abs + through
            if m == "f16x3" and 0 < i < L - 1:
                ones = np.ones((1,) + w.shape[1:])
                sum_a = conv(np.abs(h) + b[m], ones, dil[i])                 # (1, T): sum of |operands| of a position
                sum_w = aw.reshape(w.shape[0], -1).sum(1)[:, None]            # (C, 1)
                sa = fb.act_scale(np.float32((np.abs(h) + b[m]).max()))
                own = fb.split_dot_bound(absprod, K, sum_a, sum_w, sa, fb.weight_scale(aw.max()), bias)
            else:
                own = fb.dot_bound(absprod, K, bias)
            b[m] = fb.epilogue_step(pre, through + own, 1)
        if i < L - 1 or last_activation:
            h = leaky(pre, model.slope)
            for m in maths:
                b[m] = fb.epilogue_step(h, b[m], 1)
        else:
            h = pre
        if i < L - 1 and keep:
            acts.append(h)
            for m in maths:
                b_acts[m].append(b[m])
    return {"acts": acts, "logits": h[0], "b_acts": b_acts, "b_logits": {m: b[m][0] for m in maths}}


def forward_long(model, x, maths=MATHS, chunk=4096, window=256):
    """``forward(keep=False)`` of a long utterance piece by piece (arrays that stay in the caches): logits and their bounds.

    A piece is ``chunk`` samples plus E = window + halo on each side (less at the utterance's ends, where the true zero
    padding applies).  Inside the chunk every value has its whole receptive field, so the logits are those of ``forward``
    (up to the summation order of the matrix products).  The "f16x3" bound takes the activation scale from the largest
    |x| + b of the PIECE instead of the utterance: every kernel window (at most ``window`` samples) that holds a position of
    the chunk lies inside the piece with exact values, and whatever else the piece holds can only raise the maximum, so this
    is still an upper bound of what the kernel measured -- and a smaller one than the utterance's."""
    x = np.asarray(x, np.float64)
    T, E = len(x), window + model.halo
    logits, bounds = [], {m: [] for m in maths}
    for c0 in range(0, T, chunk):
        lo, hi = max(0, c0 - E), min(T, c0 + chunk + E)
        r = forward(model, x[lo:hi], maths=maths, keep=False)
        a, b = c0 - lo, min(c0 + chunk, T) - lo
        logits.append(r["logits"][a:b])
        for m in maths:
            bounds[m].append(r["b_logits"][m][a:b])
    return {"logits": np.concatenate(logits), "b_logits": {m: np.concatenate(bounds[m]) for m in maths}}


def full_size_input(n=163840):
    """The seeded utterance of the full-size case (tests/golden/pwg_disc.npz holds the restatement's sums of it)."""
    return (0.5 * np.random.default_rng(9).standard_normal(n)).astype(np.float32)


def terms(p):
    return (p - 1.0) ** 2, p ** 2


def sums(p):
    """logits -> [sum (p - 1)^2, sum p^2]"""
    return np.array([t.sum() for t in terms(np.asarray(p, np.float64))])


def sums_with_bound(p, b_p, tile=256):
    """logits with their bound -> (sums (2,), bound (2,)); ``tile``: the most terms added in fp32 before fp64 takes over."""
    U = fb.U
    p, b_p = np.asarray(p, np.float64), np.asarray(b_p, np.float64)
    e = np.abs(p - 1.0)
    b_e = b_p + U * (e + b_p)
    t = terms(p)
    bt = (2.0 * e * b_e + b_e ** 2 + U * (e + b_e) ** 2, 2.0 * np.abs(p) * b_p + b_p ** 2 + U * (np.abs(p) + b_p) ** 2)
    gamma = (tile + 8) * U
    return (np.array([v.sum() for v in t]),
            np.array([bv.sum() + gamma * (v.sum() + bv.sum()) for v, bv in zip(t, bt)]))


def mse_losses(p_fake, p_real):
    """The evaluator's three MSE numbers from the logits of the generated and of the real batch (means over all entries)."""
    p_fake, p_real = np.asarray(p_fake, np.float64), np.asarray(p_real, np.float64)
    return {"adversarial_loss": ((p_fake - 1.0) ** 2).mean(), "real_loss": ((p_real - 1.0) ** 2).mean(),
            "fake_loss": (p_fake ** 2).mean()}


def evaluate(p_fake, p_real, sc_loss, mag_loss, lambda_adv):
    """The seven ``eval/*`` numbers as PWGEvaluator.evaluate_core forms them (:192-223)."""
    m = mse_losses(p_fake, p_real)
    gen = lambda_adv * m["adversarial_loss"] + sc_loss + mag_loss
    return {"eval/adversarial_loss": m["adversarial_loss"], "eval/spectral_convergence_loss": float(sc_loss),
            "eval/log_stft_magnitude_loss": float(mag_loss), "eval/generator_loss": gen, "eval/real_loss": m["real_loss"],
            "eval/fake_loss": m["fake_loss"], "eval/discriminator_loss": m["real_loss"] + m["fake_loss"]}


# ------------------------------------------------------------------------------------------------------------ mutants
def mutants(model, x, tile=None):
    """{name: (logits, sums)} of subtly wrong evaluations of one utterance:
       nozero  hidden positions outside the utterance are not zeroed: the stack runs on the zero-extended signal
               (identical to the truth for a model without biases, where LeakyReLU(0) = 0: returned only with biases);
       dil     d_i = i + 1;
       lastact the output conv is followed by the activation;
       twice   the loss terms of the first tile (``tile`` samples, default the whole receptive field) are added twice."""
    x = np.asarray(x, np.float64)
    T, H = len(x), model.halo
    out = {}
    if model.cfg.get("bias", True):
        p = forward(model, np.concatenate([np.zeros(H), x, np.zeros(H)]), maths=(), keep=False)["logits"][H:H + T]
        out["nozero"] = (p, sums(p))
    p = forward(model, x, maths=(), keep=False, dil=[i + 1 for i in range(len(model.w) - 1)] + [1])["logits"]
    out["dil"] = (p, sums(p))
    p = forward(model, x, maths=(), keep=False, last_activation=True)["logits"]
    out["lastact"] = (p, sums(p))
    p = forward(model, x, maths=(), keep=False)["logits"]
    out["twice"] = (p, sums(p) + sums(p[:max(1, tile or H)]))
    return out


def golden_configs():
    """The two configurations of tests/golden/pwg_disc.npz: name -> (constructor kwargs, seed, input shape)."""
    return {
        "a": (dict(in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, bias=True,
                   negative_slope=0.2), 501, (2, 1, 300)),
        "b": (dict(in_channels=1, out_channels=1, kernel_size=5, layers=5, conv_channels=16, dilation_factor=2, bias=False,
                   negative_slope=0.2), 502, (1, 1, 97)),
    }


def golden_inputs(name):
    """(state dict in weight-norm form, x (N, 1, T) float32) of a golden configuration, regenerated from its seed.  The
    weights are synthetic.pwg_disc_state's ``peaked`` ones: with dense rows the bound above, which is carried through |W|,
    exceeds the logits themselves and no mutant could fall outside it."""
    from parakeet_amd import synthetic as syn
    cfg, seed, shape = golden_configs()[name]
    state = syn.pwg_disc_state(dict(cfg), seed=seed, weight_norm=True, peaked=True)
    x = np.random.default_rng(seed + 1000).normal(size=shape).astype(np.float32) * 0.5
    return state, x
