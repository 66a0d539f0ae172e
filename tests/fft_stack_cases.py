"""Cases, inputs and float64 references of the FFT-stack sweep (tests/test_fft_stack_cpu.py, tests/test_fft_stack_gpu.py).

The feed-forward-transformer stack (csrc/fft.hip, csrc/ffn_planes.hip: LayerNorm, three attention kernel families, the q|k|v and
out projections, the feed-forward convs) is driven through ``FastSpeech2`` and its debug taps and compared with
``oracle/fastspeech2_ref.py`` in float64.

Models.  MODELS below: every head size ``pk_fs2_create`` admits (64, 96, 128, 192) at two widths, LayerNorm rows of 1 and of
PK_FFT_LN_MAXPER elements per lane, a two-layer stack, a post-norm stack and one stack of the shape the planes kernels are built
for (adim 384, units 1536, k 3).  One layer per stack, units 2 adim, predictor channels 64 and no postnet unless the entry says
otherwise; the rest is the LJSpeech recipe.  (adim <= 64 PK_FFT_LN_MAXPER and dk >= 64 leave at most 8 heads, so no model reaches
PK_FFT_MAX_HEADS.)

State.  ``synthetic.fastspeech2_state(80, 80, cfg, seed, fixed_duration=1)``: one frame per token, so the decoder's timeline has
the token lengths too.  Every layer's ``linear_q`` weight and bias is multiplied by the query gain (1, 8, 32): with Xavier
weights attention is nearly uniform (median row peak 0.02 at 257 keys), and the running maximum, the rescale of O and the masking
of clamped keys hardly move the output; gain 8 gives peaks around 0.5, gain 32 nearly one-hot rows and logits a few hundred wide.

Lengths.  LENGTHS as one ragged batch, in that order and reversed: the edges of the 32-key tile, the 32-query wave tile, the
128- and 256-query workgroups, odd and even numbers of key tiles (the two fragment buffers of the pipelined kernel), a one-row
utterance between long ones, and grids whose trailing workgroups return at once for the short utterances.

Bar.  Per case and tap (0 = encoder output ``hs``, 5 = decoder output ``zs``):
    e32 = max |float32 oracle - float64 oracle| over the batch,      bar = 4 * max(e32, ulp32(peak |float64 tap|))
from the references alone.  The factor 4: LayerNorm, the GEMMs and the online softmax each sum in another order than the oracle
(three stages, each up to the oracle's own rounding), and the split-fp16 path may be twice the exact path's error
(tests/test_fs2_gpu.py::test_fs2_split_math_is_scale_invariant).

Seeds.  The ``seed`` of each entry was searched on the CPU (``python tests/fft_stack_cases.py --search NAME``) so that the
reference alone meets the input conditions tests/test_fft_stack_cpu.py asserts: at gains 8 and 32, some query row of layer 0 puts
at least 0.1 on the keys of the last, partial key tile of every utterance of 33, 65, 97, 129 and 257 rows.  That condition is
searched for and asserted in the encoder (whose layer 0 sees nothing but the embeddings); the decoder runs the same kernels at
the same lengths on what the encoder made of them, and its figures are printed.
"""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from parakeet_amd import synthetic as syn   # noqa: E402

LENGTHS = (1, 31, 32, 33, 64, 65, 97, 127, 128, 129, 255, 256, 257)
PARTIAL_TAIL = (33, 65, 97, 129, 257)     # lengths whose last key tile is partial and not the only one
GAINS = (1, 8, 32)
MATHS = ("f32", "f16x3")
IDIM = ODIM = 80
KEY_TILE = 32

MODELS = (
    dict(name="a64h1", adim=64, aheads=1, seed=4),        # dk 64; LayerNorm with one element per lane
    dict(name="a128h2", adim=128, aheads=2, seed=0),      # dk 64
    dict(name="a192h2", adim=192, aheads=2, seed=17),      # dk 96
    dict(name="a128h1", adim=128, aheads=1, seed=59),      # dk 128
    dict(name="a256h2", adim=256, aheads=2, seed=4),      # dk 128
    dict(name="a192h1", adim=192, aheads=1, seed=73),      # dk 192
    dict(name="a384h2", adim=384, aheads=2, seed=0),      # dk 192, the recipe's own
    dict(name="a512h8", adim=512, aheads=8, seed=0),      # dk 64; LayerNorm at 64 * PK_FFT_LN_MAXPER
    dict(name="a384h2x2", adim=384, aheads=2, layers=2, seed=0),        # layer 1 takes its operand scales from layer 0's output
    dict(name="a384h2post", adim=384, aheads=2, prenorm=False, seed=2),  # post-norm: scales from the k_qkv_amax pass
    dict(name="a384h2planes", adim=384, aheads=2, units=1536, seed=2),   # the one shape the planes kernels are built for
)
MODEL = {m["name"]: m for m in MODELS}
NAMES = tuple(m["name"] for m in MODELS)
PLANES_MODEL = "a384h2planes"


def config(name):
    """Constructor arguments of ``FastSpeech2`` for a model of the table."""
    m = MODEL[name]
    A, n = m["adim"], m.get("layers", 1)
    units = m.get("units", 2 * A)
    pre = m.get("prenorm", True)
    return dict(syn.FS2_LJSPEECH, adim=A, aheads=m["aheads"], elayers=n, dlayers=n, eunits=units, dunits=units,
                duration_predictor_chans=64, pitch_predictor_chans=64, energy_predictor_chans=64, postnet_layers=0,
                encoder_normalize_before=pre, decoder_normalize_before=pre)


_ORACLE_KEYS = ("adim aheads elayers eunits dlayers dunits positionwise_conv_kernel_size "
                "duration_predictor_layers duration_predictor_chans duration_predictor_kernel_size "
                "pitch_predictor_layers pitch_predictor_chans pitch_predictor_kernel_size "
                "energy_predictor_layers energy_predictor_chans energy_predictor_kernel_size "
                "pitch_embed_kernel_size energy_embed_kernel_size postnet_layers postnet_chans postnet_filts "
                "encoder_normalize_before decoder_normalize_before").split()


def oracle_config(name):
    cfg = config(name)
    return {k: cfg[k] for k in _ORACLE_KEYS}


def state(name, gain, seed=None):
    """The model's float32 state with every layer's query projection multiplied by ``gain`` (a new dict per call)."""
    m, cfg = MODEL[name], config(name)
    st = syn.fastspeech2_state(IDIM, ODIM, cfg, seed=m["seed"] if seed is None else seed, fixed_duration=1)
    g = np.float32(gain)
    for stack, n in (("encoder", cfg["elayers"]), ("decoder", cfg["dlayers"])):
        for i in range(n):
            for leaf in ("weight", "bias"):
                key = f"{stack}.encoders.{i}.self_attn.linear_q.{leaf}"
                st[key] = (st[key] * g).astype(np.float32)
    return st


def texts(name, seed=None):
    """The ragged batch in table order: one id array per length of LENGTHS."""
    s = MODEL[name]["seed"] if seed is None else seed
    return [syn.phoneme_ids(T, IDIM, seed=1000 * s + 10 + i) for i, T in enumerate(LENGTHS)]


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def case_id(name, gain, math=None):
    return f"{name}-g{gain}" + (f"-{math}" if math else "")


def _attention_stats(attn, T):
    """(row peak, row argmax, weight on the last partial key tile) of one (heads, T, T) array of attention weights."""
    a = attn.numpy()
    tail0 = KEY_TILE * ((T - 1) // KEY_TILE)
    return dict(peak=a.max(-1), argmax=a.argmax(-1), tail=a[:, :, tail0:].sum(-1))


def _oracle(st, ids, name, dtype, attention=False):
    from oracle import fastspeech2_ref as ref
    _, parts = ref.inference(st, ids, oracle_config(name), dtype=dtype, return_parts=True, return_attention=attention)
    return parts


@functools.lru_cache(maxsize=None)
def reference(name, gain, seed=None):
    """The float64 references of a case, computed once and never modified: per utterance ``hs`` / ``zs`` / ``d`` (numpy), the
    attention statistics of layer 0 of either stack, and ``e32`` / ``peak`` / ``bar`` per tap ("hs", "zs")."""
    st, tx = state(name, gain, seed), texts(name, seed)
    out = dict(hs=[], zs=[], d=[], enc=[], dec=[])
    e32 = dict(hs=0.0, zs=0.0)
    peak = dict(hs=0.0, zs=0.0)
    for ids in tx:
        p64 = _oracle(st, ids, name, torch.float64, attention=True)
        p32 = _oracle(st, ids, name, torch.float32)
        for tap in ("hs", "zs"):
            w = p64[tap].numpy()
            w.setflags(write=False)
            out[tap].append(w)
            e32[tap] = max(e32[tap], float(np.abs(p32[tap].numpy().astype(np.float64) - w).max()))
            peak[tap] = max(peak[tap], float(np.abs(w).max()))
        out["d"].append(p64["d"].numpy())
        out["enc"].append(_attention_stats(p64["attn_enc"][0], len(ids)))
        out["dec"].append(_attention_stats(p64["attn_dec"][0], len(ids)))
    out["e32"], out["peak"] = e32, peak
    out["bar"] = {tap: 4.0 * max(e32[tap], ulp32(peak[tap])) for tap in e32}
    return out


def attention_layer0(name, gain, b, stack="encoder"):
    """The float64 attention weights (heads, T, T) of layer 0 of ``stack`` for utterance ``b`` of the case's batch."""
    p64 = _oracle(state(name, gain), texts(name)[b], name, torch.float64, attention=True)
    return p64["attn_enc" if stack == "encoder" else "attn_dec"][0].numpy()


# ---- a second float64 statement of the encoder stack, with planted defects -----------------------------------------------------
# Plain numpy, the whole ragged batch at once (two of the defects read a neighbouring utterance), attention as the kernels do it:
# key tiles of 32 with a running maximum.  defect=None must reproduce the oracle's ``hs``; each switch is a way the kernels could
# be subtly wrong, and the bar of the case has to reject it.
DEFECTS = {
    "last_key_ignored": "the last key of an utterance is left out",
    "clamped_keys_counted": "the keys behind the end of the final tile count as copies of key len - 1 (clamped loads, no mask)",
    "no_rescale": "O is not rescaled when the running maximum rises in a later key tile",
    "next_utterance_key": "the first row of the batch's next utterance is read as one more key",
    "k_single_fp16": "the K operand is rounded to one fp16 term (no lo part)",
    "unbiased_variance": "LayerNorm divides the squared deviations by C - 1",
    "conv_reads_neighbour": "the +-1 taps of the feed-forward convs at an utterance's edges read the neighbouring utterance",
}


def _f64(st, key):
    return np.asarray(st[key], dtype=np.float64)


def _layer_norm(x, g, b, unbiased):
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d * d).sum(-1, keepdims=True) / (x.shape[-1] - 1 if unbiased else x.shape[-1])
    return d / np.sqrt(var + 1e-5) * g + b


def _round_fp16_block(k):
    """One fp16 term under a power-of-two block scale that puts max|k| into (0.5, 1] (pk_split.h keeps a second term)."""
    s = 2.0 ** math.ceil(math.log2(max(np.abs(k).max(), 1e-30)))
    return (k / s).astype(np.float16).astype(np.float64) * s


def _attend(q, k, v, defect, k_next, v_next):
    """softmax(q k^T) v of one (utterance, head) over key tiles of KEY_TILE with a running maximum (q is already scaled)."""
    T = k.shape[0]
    if defect == "last_key_ignored" and T > 1:
        k, v = k[:-1], v[:-1]
    if defect == "next_utterance_key" and k_next is not None:
        k, v = np.concatenate([k, k_next[None]]), np.concatenate([v, v_next[None]])
    if defect == "clamped_keys_counted" and k.shape[0] % KEY_TILE:
        n = KEY_TILE - k.shape[0] % KEY_TILE
        k, v = np.concatenate([k, np.repeat(k[-1:], n, 0)]), np.concatenate([v, np.repeat(v[-1:], n, 0)])
    if defect == "k_single_fp16":
        k = _round_fp16_block(k)
    m = np.full(q.shape[0], -np.inf)
    l = np.zeros(q.shape[0])
    O = np.zeros((q.shape[0], v.shape[1]))
    for k0 in range(0, k.shape[0], KEY_TILE):
        s = q @ k[k0:k0 + KEY_TILE].T
        m_new = np.maximum(m, s.max(-1))
        alpha = np.exp(m - m_new)
        p = np.exp(s - m_new[:, None])
        l = l * alpha + p.sum(-1)
        O = (O if defect == "no_rescale" else O * alpha[:, None]) + p @ v[k0:k0 + KEY_TILE]
        m = m_new
    return O / l[:, None]


def _conv(xs, w, b, neighbours):
    """Conv1D(k = 3, 'same') over every utterance of the list; w [Cout, Cin, 3].  neighbours: the edge taps read the last / first
    row of the previous / next utterance of the batch instead of zero."""
    out = []
    for i, x in enumerate(xs):
        zero = np.zeros((1, x.shape[1]))
        lo = xs[i - 1][-1:] if neighbours and i > 0 else zero
        hi = xs[i + 1][:1] if neighbours and i + 1 < len(xs) else zero
        xp = np.concatenate([lo, x, hi])
        T = x.shape[0]
        out.append(sum(xp[t:t + T] @ w[:, :, t].T for t in range(3)) + b)
    return out


def restated_hs(name, gain, defect=None, reverse=False):
    """The encoder tap ``hs`` of every utterance of the batch (table order, or reversed) from the second statement."""
    assert defect is None or defect in DEFECTS, defect
    cfg, st = config(name), state(name, gain)
    tx = texts(name)[::-1] if reverse else texts(name)
    A, H, pre = cfg["adim"], cfg["aheads"], cfg["encoder_normalize_before"]
    dk = A // H
    unb = defect == "unbiased_variance"
    table = _f64(st, "encoder.embed.0.weight").copy()
    table[0] = 0.0
    from oracle.nn_ref import sinusoid_table   # (the float32 table the reference builds: a constant of the model)
    pe = sinusoid_table(max(LENGTHS), A, torch.float64).numpy()
    xs = [table[ids] + float(st["encoder.embed.1.alpha"][0]) * pe[:len(ids)] for ids in tx]
    for i in range(cfg["elayers"]):
        p = f"encoder.encoders.{i}."
        n1 = lambda x: _layer_norm(x, _f64(st, p + "norm1.weight"), _f64(st, p + "norm1.bias"), unb)   # noqa: E731
        n2 = lambda x: _layer_norm(x, _f64(st, p + "norm2.weight"), _f64(st, p + "norm2.bias"), unb)   # noqa: E731
        hs = [n1(x) for x in xs] if pre else xs
        q, k, v = ([h @ _f64(st, p + f"self_attn.linear_{c}.weight") + _f64(st, p + f"self_attn.linear_{c}.bias") for h in hs]
                   for c in "qkv")
        att = []
        for b in range(len(xs)):
            ctx = np.empty_like(q[b])
            nxt = b + 1 if b + 1 < len(xs) else None
            for hd in range(H):
                c = slice(hd * dk, (hd + 1) * dk)
                ctx[:, c] = _attend(q[b][:, c] / math.sqrt(dk), k[b][:, c], v[b][:, c], defect,
                                    None if nxt is None else k[nxt][0, c], None if nxt is None else v[nxt][0, c])
            att.append(ctx @ _f64(st, p + "self_attn.linear_out.weight") + _f64(st, p + "self_attn.linear_out.bias"))
        xs = [x + a for x, a in zip(xs, att)]
        if not pre:
            xs = [n1(x) for x in xs]
        hs = [n2(x) for x in xs] if pre else xs
        nb = defect == "conv_reads_neighbour"
        f = [np.maximum(y, 0.0) for y in _conv(hs, _f64(st, p + "feed_forward.w_1.weight"), _f64(st, p + "feed_forward.w_1.bias"), nb)]
        f = _conv(f, _f64(st, p + "feed_forward.w_2.weight"), _f64(st, p + "feed_forward.w_2.bias"), nb)
        xs = [x + y for x, y in zip(xs, f)]
        if not pre:
            xs = [n2(x) for x in xs]
    if pre:
        xs = [_layer_norm(x, _f64(st, "encoder.after_norm.weight"), _f64(st, "encoder.after_norm.bias"), unb) for x in xs]
    return xs


def tap_error(got, want):
    """max |got - want| over the utterances of a batch (lists of (T, adim) arrays)."""
    return max(float(np.abs(np.asarray(g, dtype=np.float64) - w).max()) for g, w in zip(got, want))


# ---- input conditions (asserted by tests/test_fft_stack_cpu.py; searched by --search) ------------------------------------------
PEAK_MEDIAN_MIN = {8: 0.4, 32: 0.9}
TAIL_WEIGHT_MIN = 0.1


def input_conditions(ref):
    """(median row peak, lengths > 32 without a row whose largest weight lies outside key tile 0, lengths of PARTIAL_TAIL without
    a row that puts TAIL_WEIGHT_MIN on the last partial tile) per stack ("enc", "dec"), from a ``reference``."""
    res = {}
    for stack in ("enc", "dec"):
        peaks = np.concatenate([s["peak"].reshape(-1) for s in ref[stack]])
        no_far = [T for T, s in zip(LENGTHS, ref[stack]) if T > KEY_TILE and not (s["argmax"] >= KEY_TILE).any()]
        no_tail = [T for T, s in zip(LENGTHS, ref[stack]) if T in PARTIAL_TAIL and not (s["tail"] >= TAIL_WEIGHT_MIN).any()]
        res[stack] = (float(np.median(peaks)), no_far, no_tail)
    return res


def _encoder_layer0_stats(st, cfg, ids):
    """The attention statistics of encoder layer 0 for one utterance from a few lines of numpy (the seed search's inner loop;
    the test asserts on the oracle's weights, not on these)."""
    A, H = cfg["adim"], cfg["aheads"]
    from oracle.nn_ref import sinusoid_table
    table = _f64(st, "encoder.embed.0.weight")
    x = table[ids] + float(st["encoder.embed.1.alpha"][0]) * sinusoid_table(len(ids), A, torch.float64).numpy()
    p = "encoder.encoders.0."
    if cfg["encoder_normalize_before"]:
        x = _layer_norm(x, _f64(st, p + "norm1.weight"), _f64(st, p + "norm1.bias"), False)
    q, k = (x @ _f64(st, p + f"self_attn.linear_{c}.weight") + _f64(st, p + f"self_attn.linear_{c}.bias") for c in "qk")
    T, dk = len(ids), A // H
    s = np.einsum("thd,shd->hts", q.reshape(T, H, dk), k.reshape(T, H, dk)) / math.sqrt(dk)
    w = np.exp(s - s.max(-1, keepdims=True))
    return _attention_stats(torch.from_numpy(w / w.sum(-1, keepdims=True)), T)


def _search(name, tries=300):
    """The first seed whose encoder meets the per-utterance input conditions at gains 8 and 32."""
    cfg = config(name)
    for seed in range(tries):
        ok = True
        for gain in (8, 32):
            st, tx = state(name, gain, seed), texts(name, seed)
            ref = dict(enc=[_encoder_layer0_stats(st, cfg, ids) for ids in tx])
            ref["dec"] = ref["enc"]
            med, no_far, no_tail = input_conditions(ref)["enc"]
            ok = not no_far and not no_tail     # (the median is a property of the gain, not of the seed)
            if not ok:
                break
        if ok:
            return seed
    return None


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--search":
        torch.set_num_threads(8)
        for nm in sys.argv[2:]:
            print("FOUND", nm, _search(nm), flush=True)
