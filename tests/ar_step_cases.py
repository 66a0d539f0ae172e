"""Cases, inputs and float64 references of the autoregressive step sweep (tests/test_ar_step_cpu.py, tests/test_ar_step_gpu.py).

The per-step kernels and the per-step dispatch of TransformerTTS (csrc/tts.hip) and Tacotron2 (csrc/taco2.hip) are driven through
``TransformerTTS.inference_batch`` / ``Tacotron2.infer_batch`` and compared with ``oracle/transformer_tts_ref.py`` /
``oracle/tacotron2_ref.py`` in float64, one oracle run per utterance.

Dispatch boundaries (read from ``attn_step()``, the step loop of ``pk_tts_infer`` and ``taco_run()``; restated by
``attn_step_choice`` / ``src_q_fused`` / ``fused_prenet`` / ``lstm_threads`` below, and asserted per case by the CPU test):

    TransformerTTS attention of one step, nmax keys (self: the step number; source: the longest text + <eos>)
      query projected in the kernel (dk 64, maxT <= 256, adim <= 512)   nmax <= 128 -> k_tts_attn_step64<8, true>, else <16, true>
      dk 64, nmax <= 640, nb = ceil(nmax / 16)                          nb <= 8 | 16 | 24 | 32 | 40 -> k_tts_attn_step64<nb>
      dk 96 / 128 / 192, or more than 640 keys                          k_tts_attn_step: nv = dk / 4 float4 columns (16, 24, 32, 48),
                                                                        G = 256 / nv value groups, 256-key score passes, 256-stride softmax
      source attention, maxT > 256 or dk != 64                          query from a row GEMM (tts_row_src_q), kernel name tts_attn_src
      stop head, B <= 32                                                rides on the feat_out row GEMM (tts_row_feat_out_stop)
      stop head, B > 32                                                 tts_row_feat_out (two row blocks) + tts_stop with the LayerNorm
    Tacotron2 step
      prenet, (d_prenet / 4) divides 512 and d_prenet <= 512            k_ar_prenet_embed (taco_prenet); else two row GEMMs with dropout in
                                                                        the epilogue (taco_row_prenet); teacher forcing: w1 == NULL rows
      projection, stop token and B <= 32                                taco_row_proj_stop; else taco_row_proj + taco_stop
      k_taco_lstm_seq                                                   min(1024, 64 ceil(4 Hh / 64)) threads for 4 Hh gates
      k_taco_lsa_ctx                                                    256-stride softmax over T, ceil((E + G) / 256) context blocks,
                                                                        16-row clamped context walk
The profile gives every instantiation of a step kernel one name; which template ran is not observable, hence this table.

Models.  One encoder layer, two decoder layers, no postnet, units 2 adim, dprenet_units 32 for TransformerTTS (TTS_MODELS);
``_T2_SMALL`` of tests/ar_cases.py for Tacotron2 (T2_MODELS).  The stop head is held off with stop_bias -8 unless the case is about
stopping.  Dropout stays on, one seed per utterance (DROP_SEED + b).

Input conditions.  With Xavier weights attention is nearly uniform, and a kernel that dropped its last keys would move nothing.  The
decoder's ``self_attn.linear_q`` / ``src_attn.linear_q`` (weight and bias) are multiplied by ``gain``; Tacotron2's
``attention_layer.value.weight`` likewise.  Seeds of the weights and of the texts were searched on the CPU (``python
tests/ar_step_cases.py --search CALL``) so that the float64 reference alone meets the conditions tests/test_ar_step_cpu.py asserts
-- with 1.5 x room, and for the long decodes so that the float32 oracle does not drift past the fixed bars (query gain 8 did over
70 steps: group 1 uses 4, the 649-step decode 5); SEEDS records them.  The calls of group 2 share one architecture and take one
seed of the weights per K: the position table makes the weight on the last key a property of the weights, not of the text.

Bar.  Per call and quantity:  e32 = max |float32 oracle - float64 oracle| over the call's utterances (same inputs, seeds, steps),
    bar = 4 * max(e32, ulp32(peak |float64 value|))
the convention and the factor of tests/fft_stack_cases.py.  Quantities named ``x:mean`` compare the mean |.| per frame, maximised
over frames (the per-step check).  FIXED_BAR holds what the existing tests ask of the same quantity; no derived bar may be looser.
"""
import functools
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from parakeet_amd import synthetic as syn   # noqa: E402
from ar_cases import _T2_SMALL              # noqa: E402

TTS_IDIM, ODIM = 40, 80
DROP_SEED = 7
TAIL_WEIGHT_MIN = 0.1
STOP_PROB_MARGIN, STOP_LOGIT_MARGIN, TOP2_MARGIN = 0.02, 0.05, 1e-3

FIXED_BAR = {"att": 1e-4, "probs": 1e-4, "hs": 1e-4, "zs": 2e-4, "before": 2e-4, "before:mean": 1e-4,
             "enc": 1e-4, "alignments": 1e-4, "stop_logits": 1e-3,
             "mel_output": 2e-3, "mel_outputs_postnet": 2e-3, "mel_output:mean": 1e-4, "mel_outputs_postnet:mean": 1e-4}
TTS_QUANTITIES = ("hs", "zs", "before", "before:mean", "probs", "att")
T2_QUANTITIES = ("enc", "mel_output", "mel_output:mean", "mel_outputs_postnet", "mel_outputs_postnet:mean", "alignments", "stop_logits")


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------
def src_q_fused(dk, maxT, adim):
    return dk == 64 and maxT <= 256 and adim <= 512 and adim % 8 == 0


def attn_step_choice(dk, nmax, fused_q=False):
    """The kernel ``attn_step()`` launches for ``nmax`` keys (q | k | v rows of adim floats: every ld is a multiple of 4)."""
    if fused_q:
        return "step64<8,q>" if nmax <= 128 else "step64<16,q>"
    if dk == 64 and nmax <= 640:
        return "step64<%d>" % next(n for n in (8, 16, 24, 32, 40) if (nmax + 15) // 16 <= n)
    return "general"


def fused_prenet(d_prenet, d_mels=80):
    return d_prenet % 4 == 0 and d_prenet // 4 <= 512 and 512 % (d_prenet // 4) == 0 and d_prenet <= 512 and d_mels <= 512


def lstm_threads(Hh):
    return min(1024, (4 * Hh + 63) // 64 * 64)


# ---- TransformerTTS ------------------------------------------------------------------------------------------------------------
TTS_MODELS = {
    "dk96": dict(adim=192, aheads=2, seed=1, gain=4),
    "dk128": dict(adim=128, aheads=1, seed=2, gain=4),
    "dk192": dict(adim=192, aheads=1, seed=3, gain=4),
    "dk192h2": dict(adim=384, aheads=2, seed=4, gain=4),        # the second head's column offset
    "src64": dict(adim=128, aheads=2, seed=5, gain=8),
    "self64": dict(adim=64, aheads=1, seed=6, gain=5),
    "b33": dict(adim=64, aheads=1, seed=7, gain=4, stop_gain=2.0, stop_bias=0.6),
}
SRC_KEYS = (128, 129, 256, 257, 384, 385, 512, 513, 640, 641)
B33_KEYS = tuple(2 + b % 5 for b in range(33))                   # 2 .. 6 source keys; ratio 2 -> at most 12 steps

# searched seeds: call -> {"model": seed of the weights (default: the model's own), utterance: seed of its ids}; every other utterance
# takes 1000 + 50 * (index of the call) + b
SEEDS = {
    "heads-dk96": {"model": 36, 0: 36},
    "heads-dk128": {"model": 572, 0: 572},
    "heads-dk192": {"model": 274, 0: 274},
    "heads-dk192h2": {"model": 8, 0: 8},
    "lsa-max": {"model": 14, 10: 14, 11: 0},
    "src-129": {"model": 3, 0: 3},
    "src-385": {"model": 7, 0: 7},
    "src-513": {"model": 69, 0: 69},
    "src-640": {"model": 7, 0: 7},
    "src-641": {"model": 8, 0: 8},
    "self-649": {"model": 105, 0: 105},
    "lsa-min": {"model": 126, 10: 126, 11: 0},
    "lsa-base": {"model": 955, 10: 955, 11: 0},
    "t2-b33": {32: 1235, 0: 5003, 1: 5101, 2: 5200, 3: 5304, 4: 5400, 5: 5500, 6: 5600, 7: 5701, 8: 5800, 9: 5902, 10: 6001, 11: 6100, 12: 6200,
               13: 6300, 14: 6400, 15: 6501, 16: 6601, 17: 6700, 18: 6800, 19: 6904, 20: 7000, 21: 7103, 22: 7200, 23: 7300, 24: 7400,
               25: 7500, 26: 7601, 27: 7700, 28: 7802, 29: 7900, 30: 8000, 31: 8101},
    "src-128": {0: 0},
    "src-256": {0: 0},
    "src-257": {0: 0},
    "src-384": {0: 0},
    "src-512": {0: 0},
    "nostop": {1: 0, 2: 13, 3: 0},
    "tts-b33": {32: 42, 0: 5041, 1: 5143, 2: 5203, 3: 5301, 4: 5401, 5: 5500, 6: 5606, 7: 5701, 8: 5844, 9: 5902, 10: 6007, 11: 6106, 12: 6201,
                13: 6300, 14: 6400, 15: 6500, 16: 6956, 17: 6700, 18: 6800, 19: 6900, 20: 7002, 21: 7141, 22: 7205, 23: 7306, 24: 7405,
                25: 7500, 26: 7617, 27: 7741, 28: 7800, 29: 7903, 30: 8041, 31: 8100},
}

TTS_CALLS = {}
for _m in ("dk96", "dk128", "dk192", "dk192h2"):
    # group 1: 70 steps for the 257-key utterance (self keys walk through 16, 64, 65), int(65 r) = 17, int(2 r) = 0 -> one step
    TTS_CALLS["heads-" + _m] = dict(group=1, model=_m, keys=(257, 65, 2), ratio=70.5 / 257, maths=("f16x3", "f32"))
for _K in SRC_KEYS:
    # group 2: three steps for the K-key utterance, one for the others (int(17 * 3.5 / K) = 0)
    TTS_CALLS["src-%d" % _K] = dict(group=2, model="src64", keys=(_K, 17, 2), ratio=3.5 / _K, maths=("f16x3", "f32"))
# group 3: int(3 r) = 649 steps, int(2 r) = 433; kstride = B = 2, utterance 1's rows are dead for the last third
TTS_CALLS["self-649"] = dict(group=3, model="self64", keys=(3, 2), ratio=216.5, maths=("f16x3",))
# group 4: stop tokens at different steps
TTS_CALLS["tts-b33"] = dict(group=4, model="b33", keys=B33_KEYS, ratio=2.0, maths=("f16x3",))
_TTS_INDEX = {c: i for i, c in enumerate(TTS_CALLS)}


def tts_config(model):
    m = TTS_MODELS[model]
    A = m["adim"]
    return dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=2, postnet_layers=0, adim=A, aheads=m["aheads"], eunits=2 * A,
                dunits=2 * A, dprenet_units=32)


@functools.lru_cache(maxsize=None)
def tts_state(model, seed=None):
    """The float32 state of a model, the decoder's query projections multiplied by the gain (read-only arrays)."""
    m, cfg = TTS_MODELS[model], tts_config(model)
    st = syn.transformer_tts_state(TTS_IDIM, ODIM, cfg, seed=m["seed"] if seed is None else seed,
                                   stop_bias=m.get("stop_bias", -8.0), stop_gain=m.get("stop_gain", 1.0))
    g = np.float32(m["gain"])
    for l in range(cfg["dlayers"]):
        for att in ("self_attn", "src_attn"):
            for leaf in ("weight", "bias"):
                key = f"decoder.decoders.{l}.{att}.linear_q.{leaf}"
                st[key] = (st[key] * g).astype(np.float32)
    return st


def text_seed(call, b, index):
    return SEEDS.get(call, {}).get(b, 1000 + 50 * index[call] + b)


def tts_texts(call, seeds=None):
    """Token ids without <eos>: keys - 1 of them per utterance."""
    c = TTS_CALLS[call]
    return [syn.phoneme_ids(k - 1, TTS_IDIM, seed=(seeds or {}).get(b, text_seed(call, b, _TTS_INDEX))) for b, k in enumerate(c["keys"])]


def drop_seeds(n):
    return [DROP_SEED + b for b in range(n)]


def tts_call_state(call, mseed=None):
    c = TTS_CALLS[call]
    return tts_state(c["model"], SEEDS.get(call, {}).get("model") if mseed is None else mseed)


def tts_oracle(call, b, dtype, attn_hook=None, ids=None, mseed=None):
    """One oracle run -> dict of numpy arrays: hs, zs, before, probs, att (dlayers, H, L, T), self_last (dlayers, H, L)."""
    from oracle import transformer_tts_ref as tt
    c = TTS_CALLS[call]
    ids = tts_texts(call)[b] if ids is None else ids
    _, probs, att, parts = tt.inference(tts_call_state(call, mseed), ids, tts_config(c["model"]), maxlenratio=c["ratio"], seed=DROP_SEED + b,
                                        dtype=dtype, return_parts=True, attn_hook=attn_hook)
    out = dict(hs=parts["hs"], zs=parts["zs"], before=parts["before"], probs=probs, att=att, self_last=parts["self_att"][-1])
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def error(q, got, want):
    """The figure a quantity is held to: max |.|, or for ``x:mean`` the largest per-frame mean |.|."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(d.reshape(d.shape[0], -1).mean(-1).max()) if q.endswith(":mean") else float(d.max())


def _bars(quantities, runs64, runs32):
    e32 = {q: 0.0 for q in quantities}
    peak = dict(e32)
    for r64, r32 in zip(runs64, runs32):
        for q in quantities:
            k = q.split(":")[0]
            if k not in r64:
                continue
            assert r64[k].shape == r32[k].shape, f"the float32 oracle ends {k} elsewhere: {r32[k].shape} vs {r64[k].shape}"
            e32[q] = max(e32[q], error(q, r32[k], r64[k]))
            peak[q] = max(peak[q], float(np.abs(r64[k]).max()))
    return e32, peak, {q: 4.0 * max(e32[q], ulp32(peak[q])) for q in quantities if peak[q] > 0.0}


def _freeze(runs):
    for r in runs:
        for v in r.values():
            v.setflags(write=False)
    return runs


@functools.lru_cache(maxsize=None)
def tts_reference(call):
    """The float64 references of a call, computed once: ``utts`` (one dict per utterance), ``lengths``, ``e32`` / ``peak`` / ``bar``,
    ``seconds`` (the CPU time of the two oracles)."""
    n, t0 = len(TTS_CALLS[call]["keys"]), time.time()
    runs64 = _freeze([tts_oracle(call, b, torch.float64) for b in range(n)])
    runs32 = [tts_oracle(call, b, torch.float32) for b in range(n)]
    e32, peak, bar = _bars(TTS_QUANTITIES, runs64, runs32)
    return dict(utts=runs64, lengths=[r["before"].shape[0] for r in runs64], e32=e32, peak=peak, bar=bar, seconds=time.time() - t0)


def tail16(n):
    """First key of the last 16-key group of n keys."""
    return 16 * ((n - 1) // 16)


def tts_tail_weights(run):
    """(largest source weight, largest self weight) any head puts on the last 16-key group at the run's last step."""
    T, L = run["att"].shape[-1], run["att"].shape[2]
    src = run["att"][:, :, -1, tail16(T):].sum(-1).max()
    own = run["self_last"][:, :, tail16(L):].sum(-1).max()
    return float(src), float(own)


def ratios(ref, got_runs, quantities, only=None):
    """error / bar per quantity, maximised over the utterances of ``only`` (default: all)."""
    res = {}
    for b, got in enumerate(got_runs):
        if got is None or (only is not None and b not in only):
            continue
        for q in quantities:
            k = q.split(":")[0]
            if q in ref["bar"] and k in got and k in ref["utts"][b]:
                if got[k].shape != ref["utts"][b][k].shape:
                    res[q] = float("inf")
                else:
                    res[q] = max(res.get(q, 0.0), error(q, got[k], ref["utts"][b][k]) / ref["bar"][q])
    return res


# ---- planted defects of the attention step (hooks of oracle/transformer_tts_ref.py::mha) ----------------------------------------
def _drop_last_key(q, k, v):
    return (q, k[:, :, :-1], v[:, :, :-1]) if k.shape[2] > 1 else (q, k, v)


def _drop_keys_from_256(q, k, v):
    return q, k[:, :, :256], v[:, :, :256]


def _clamped_keys_counted(q, k, v):
    n = -k.shape[2] % 16
    return q, torch.cat([k] + [k[:, :, -1:]] * n, dim=2), torch.cat([v] + [v[:, :, -1:]] * n, dim=2)


def _drop_columns_from_64(q, k, v):
    q = q.clone()
    q[..., 64:] = 0.0
    return q, k, v


# defect -> (what it is, hook, the call and utterance it is planted in)
TTS_DEFECTS = {
    "last_key_ignored": ("the last key is left out of the softmax", _drop_last_key, "src-129", 0),
    "keys_from_256_ignored": ("keys at and beyond 256 are left out (the 256-stride second trip)", _drop_keys_from_256, "src-257", 0),
    "clamped_keys_counted": ("the last partial 16-key group counts key n - 1 for every slot (clamped loads, no mask)",
                             _clamped_keys_counted, "src-129", 0),
    "columns_from_16_ignored": ("float4 columns >= 16 of a dk > 64 head are left out of the score", _drop_columns_from_64,
                                "heads-dk96", 1),
}


# ---- Tacotron2 -----------------------------------------------------------------------------------------------------------------
T2_MODELS = {
    # group 5: the attention envelope
    "lsa-min": dict(over=dict(d_attention=16, attention_filters=1, attention_kernel_size=1), seed=11, gain=4),
    "lsa-max": dict(over=dict(d_attention=256, attention_filters=64, attention_kernel_size=63), seed=12, gain=16),
    "lsa-base": dict(over=dict(), seed=13, gain=4),
    # group 6: encoder LSTM and context widths
    "enc32": dict(over=dict(d_encoder=32, d_global_condition=16), seed=14, gain=1),
    "enc96": dict(over=dict(d_encoder=96, d_global_condition=16), seed=15, gain=1),
    "enc544": dict(over=dict(d_encoder=544, d_global_condition=16), seed=16, gain=1),
    # group 7: prenet and cell widths
    "pre16": dict(over=dict(d_prenet=16), seed=17, gain=1),
    "pre48": dict(over=dict(d_prenet=48, d_attention_rnn=48, d_decoder_rnn=80), seed=18, gain=1),
    "pre48p25": dict(over=dict(d_prenet=48, d_attention_rnn=48, d_decoder_rnn=80, p_prenet_dropout=0.25), seed=19, gain=1),
    "pre512": dict(over=dict(d_prenet=512), seed=20, gain=1),
    # group 8 / 9
    "b33": dict(over=dict(), seed=21, gain=1, stop_gain=400.0, stop_bias=-26.0),
    "nostop": dict(over=dict(use_stop_token=False), seed=22, gain=4),
}
LSA_T = (1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300)
T2_B33_T = tuple(2 + (3 * b) % 7 for b in range(33))
T2_CALLS = {}
for _m in ("lsa-min", "lsa-max", "lsa-base"):
    T2_CALLS[_m] = dict(group=5, model=_m, T=LSA_T, steps=6, maths=("f16x3", "f32"))
for _m in ("enc32", "enc96", "enc544"):
    T2_CALLS[_m] = dict(group=6, model=_m, T=(1, 17, 40), steps=4, maths=("f16x3",))
for _m in ("pre16", "pre48", "pre48p25", "pre512"):
    T2_CALLS[_m] = dict(group=7, model=_m, T=(5, 9, 3), steps=6, maths=("f16x3",))
T2_CALLS["t2-b33"] = dict(group=8, model="b33", T=T2_B33_T, steps=10, maths=("f16x3",))
T2_CALLS["nostop"] = dict(group=9, model="nostop", T=(1, 64, 65, 130), steps=26, maths=("f16x3",))
_T2_INDEX = {c: 100 + i for i, c in enumerate(T2_CALLS)}
TEACHER_CALL, TEACHER_FRAMES = "pre48", 6


def t2_config(model):
    return dict(syn.TACOTRON2_LJSPEECH, **dict(_T2_SMALL, **T2_MODELS[model]["over"]))


@functools.lru_cache(maxsize=None)
def t2_state(model, seed=None):
    m = T2_MODELS[model]
    st = syn.tacotron2_state(t2_config(model), seed=m["seed"] if seed is None else seed, stop_bias=m.get("stop_bias", -8.0), stop_gain=m.get("stop_gain", 1.0))
    key = "decoder.attention_layer.value.weight"
    st[key] = (st[key] * np.float32(m["gain"])).astype(np.float32)
    return st


def t2_texts(call, seeds=None):
    c = T2_CALLS[call]
    return [np.random.default_rng((seeds or {}).get(b, text_seed(call, b, _T2_INDEX))).integers(1, 37, size=T).astype(np.int64)
            for b, T in enumerate(c["T"])]


def t2_global_condition(call):
    """(B, d_global_condition) float32, or None."""
    G = t2_config(T2_CALLS[call]["model"]).get("d_global_condition")
    if not G:
        return None
    return np.random.default_rng(900 + _T2_INDEX[call]).standard_normal((len(T2_CALLS[call]["T"]), G)).astype(np.float32)


def teacher_mels(call=TEACHER_CALL):
    """The teacher frames of the forward() case: (B, TEACHER_FRAMES, 80) float32."""
    return np.random.default_rng(950).standard_normal((len(T2_CALLS[call]["T"]), TEACHER_FRAMES, ODIM)).astype(np.float32)


def _t2_out(o):
    out = {k: o[k].numpy().astype(np.float64) for k in ("mel_output", "mel_outputs_postnet", "alignments", "stop_logits") if k in o}
    out["enc"] = o["encoder_outputs"].numpy().astype(np.float64)
    return out


def t2_call_state(call, mseed=None):
    return t2_state(T2_CALLS[call]["model"], SEEDS.get(call, {}).get("model") if mseed is None else mseed)


def t2_oracle(call, b, dtype, hooks=None, drop="stream", ids=None, mseed=None):
    from oracle import tacotron2_ref as t2
    c = T2_CALLS[call]
    cfg = t2_config(c["model"])
    gc = t2_global_condition(call)
    if drop != "stream":
        drop = drop(DROP_SEED + b, cfg["d_prenet"], float(cfg["p_prenet_dropout"]))
    return _t2_out(t2.infer(t2_call_state(call, mseed), t2_texts(call)[b] if ids is None else ids, cfg, max_decoder_steps=c["steps"],
                            seed=DROP_SEED + b, drop=drop, dtype=dtype, return_parts=True,
                            global_condition=None if gc is None else gc[b], hooks=hooks))


@functools.lru_cache(maxsize=None)
def t2_reference(call):
    n, t0 = len(T2_CALLS[call]["T"]), time.time()
    runs64 = _freeze([t2_oracle(call, b, torch.float64) for b in range(n)])
    runs32 = [t2_oracle(call, b, torch.float32) for b in range(n)]
    e32, peak, bar = _bars(T2_QUANTITIES, runs64, runs32)
    return dict(utts=runs64, lengths=[r["mel_output"].shape[0] for r in runs64], e32=e32, peak=peak, bar=bar, seconds=time.time() - t0)


@functools.lru_cache(maxsize=None)
def t2_teacher_reference(call=TEACHER_CALL):
    """The teacher-forced forward() of the call's texts on ``teacher_mels`` (dropout stream seed 0 + b, as forward() numbers them)."""
    import taco2_forward_ref as fw
    c = T2_CALLS[call]
    cfg, st, mels = t2_config(c["model"]), t2_call_state(call), teacher_mels(call)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        runs[dtype] = [_t2_out(fw.forward(st, ids, mels[b], cfg, seed=b, dtype=dtype, return_parts=True))
                       for b, ids in enumerate(t2_texts(call))]
    e32, peak, bar = _bars(T2_QUANTITIES, runs[torch.float64], runs[torch.float32])
    return dict(utts=_freeze(runs[torch.float64]), e32=e32, peak=peak, bar=bar)


# planted defects of the Tacotron2 step
def _lsa_hook(kind):
    def hook(what, x, pad=None):
        if what == "window":
            xp = torch.nn.functional.pad(x, (pad, pad))
            if kind == "window_reads_neighbour" and pad > 0:
                # behind the utterance's end the window reads the rows that follow in a packed buffer instead of zeros; the
                # utterance's own first rows stand in for the neighbour's (one oracle run holds one utterance)
                T = x.shape[-1]
                xp[..., pad + T:] = x[..., torch.arange(pad) % T]
            return xp
        if kind == "last_key_ignored" and x.shape[1] > 1:
            x = x.clone()
            x[:, -1] = -float("inf")
        if kind == "keys_from_256_ignored":
            x = x.clone()
            x[:, 256:] = -float("inf")
        return x
    return hook


def _gates_from_1024(xg, hg):
    g = xg + hg
    g[:, 1024:] = xg[:, 1024:]
    return g


def _second_layer_takes_first_word(seed, units, p):
    from oracle import tacotron2_ref as t2
    drop = t2.stream_dropout(seed, units, p)
    return lambda step, layer, n: drop(step, 0, n)


# defect -> (what it is, keyword arguments of t2_oracle, the call and the utterances it is planted in)
T2_DEFECTS = {
    "last_key_ignored": ("the last position is left out of the softmax", dict(hooks=dict(lsa=_lsa_hook("last_key_ignored"))),
                         "lsa-base", (LSA_T.index(257),)),
    "keys_from_256_ignored": ("positions at and beyond 256 are left out (the 256-stride second trip)",
                              dict(hooks=dict(lsa=_lsa_hook("keys_from_256_ignored"))), "lsa-base", (LSA_T.index(257), LSA_T.index(300))),
    "window_reads_neighbour": ("the location window is not zero padded at the utterance's end",
                               dict(hooks=dict(lsa=_lsa_hook("window_reads_neighbour"))), "lsa-max", (LSA_T.index(17), LSA_T.index(33))),
    "no_cumulation": ("the cumulative alignment is not updated", dict(hooks=dict(no_cumulation=True)), "lsa-base",
                      (LSA_T.index(17), LSA_T.index(33))),
    "gates_from_1024": ("gate columns >= 1024 of the encoder LSTM are left at their input term", dict(hooks=dict(gates=_gates_from_1024)),
                        "enc544", (1, 2)),
    "second_dropout_word": ("the dropout word index of the second prenet layer is taken as the first's",
                            dict(drop=_second_layer_takes_first_word), "pre48", (0, 1, 2)),
}


# ---- seed search ---------------------------------------------------------------------------------------------------------------
def _search_tts(call, tries=600):
    """A seed of the weights and of utterance 0's text (the longest) that meets the tail conditions.  (The position table
    makes the weight a query puts on a position a property of the weights more than of the text.)  AR_STEP_SEARCH_FROM: the first
    seed to try (several searches of one call side by side); progress goes to stderr."""
    c = TTS_CALLS[call]
    for seed in range(int(os.environ.get("AR_STEP_SEARCH_FROM", "0")), tries):
        ids = syn.phoneme_ids(c["keys"][0] - 1, TTS_IDIM, seed=seed)
        r64 = tts_oracle(call, 0, torch.float64, ids=ids, mseed=seed)
        src, own = tts_tail_weights(r64)
        if src >= 1.5 * TAIL_WEIGHT_MIN and own >= 1.5 * TAIL_WEIGHT_MIN:
            # and the float32 oracle does not drift: every derived bar stays under the fixed one, with room
            _, _, bar = _bars(TTS_QUANTITIES, [r64], [tts_oracle(call, 0, torch.float32, ids=ids, mseed=seed)])
            print("#", call, seed, f"{src:.2f} {own:.2f}", max(bar[q] / FIXED_BAR[q] for q in bar), file=sys.stderr, flush=True)
            if all(1.5 * bar[q] <= FIXED_BAR[q] for q in bar):
                return {"model": seed, 0: seed}
        tts_state.cache_clear()
    return None


def t2_tail_weights(run):
    """(largest weight any step puts on the last position, largest any step puts on positions >= 256)."""
    a = run["alignments"]
    return float(a[:, -1].max()), float(a[:, 256:].sum(-1).max()) if a.shape[1] > 256 else None


def _search_lsa(call, tries=3000):
    """A seed of the weights and of the 257-token text that puts weight on position 256, then a text of 300 tokens that puts
    weight beyond it."""
    T = T2_CALLS[call]["T"]
    b257, b300 = T.index(257), T.index(300)
    for seed in range(tries):
        ids = np.random.default_rng(seed).integers(1, 37, size=257).astype(np.int64)
        _, far = t2_tail_weights(t2_oracle(call, b257, torch.float64, ids=ids, mseed=seed))
        t2_state.cache_clear()
        if far >= 1.5 * TAIL_WEIGHT_MIN:
            break
    else:
        return None
    found = {"model": seed, b257: seed}
    for s in range(tries):
        ids = np.random.default_rng(s).integers(1, 37, size=300).astype(np.int64)
        if t2_tail_weights(t2_oracle(call, b300, torch.float64, ids=ids, mseed=seed))[1] >= 1.5 * TAIL_WEIGHT_MIN:
            found[b300] = s
            break
    return found


def _search_nostop(call="nostop", tries=600):
    """Texts whose alignment maxima are not marginal; one of them puts weight on its last position."""
    found, T = {}, T2_CALLS[call]["T"]
    for b in range(1, len(T)):
        for s in range(tries):
            ids = np.random.default_rng(s).integers(1, 37, size=T[b]).astype(np.int64)
            r = t2_oracle(call, b, torch.float64, ids=ids)
            top = np.sort(r["alignments"], axis=-1)
            if (top[:, -1] - top[:, -2]).min() >= 1.5 * TOP2_MARGIN and (b != 2 or t2_tail_weights(r)[0] >= 1.5 * TAIL_WEIGHT_MIN):
                found[b] = s
                break
    return found


def stop_margin_tts(run, threshold=0.5):
    return float(np.abs(run["probs"] - threshold).min())


def _search_stop(call, tts, tries=400, tries32=8000):
    """Per utterance a text seed with the stop margin at every live step; utterance 32 ends through the stop token at a step no other
    ends at; at least two utterances end at their cap."""
    oracle = tts_oracle if tts else t2_oracle
    c = (TTS_CALLS if tts else T2_CALLS)[call]
    n = len(c["keys"] if tts else c["T"])

    def run(b, seed):
        if tts:
            ids = syn.phoneme_ids(c["keys"][b] - 1, TTS_IDIM, seed=seed)
            r = oracle(call, b, torch.float64, ids=ids)
            L, cap = r["before"].shape[0], int(c["keys"][b] * c["ratio"])
            return L, cap, stop_margin_tts(r) >= 1.5 * STOP_PROB_MARGIN
        ids = np.random.default_rng(seed).integers(1, 37, size=c["T"][b]).astype(np.int64)
        r = oracle(call, b, torch.float64, ids=ids)
        return r["mel_output"].shape[0], c["steps"], float(np.abs(r["stop_logits"]).min()) >= 1.5 * STOP_LOGIT_MARGIN

    found, L32 = {}, None
    for seed in range(tries32):
        L, cap, ok = run(n - 1, seed)
        if ok and 3 <= L < cap - 1:
            found[n - 1], L32 = seed, L
            break
    at_cap = 0
    for b in range(n - 1):
        for seed in range(tries):
            L, cap, ok = run(b, 5000 + 100 * b + seed)
            want_cap = b in (3, 9)
            if ok and L != L32 and ((L == cap) == want_cap or not want_cap and seed > 40):
                found[b] = 5000 + 100 * b + seed
                at_cap += L == cap
                break
    print("# lengths end at cap:", at_cap, "utterance 32 stops at", L32, file=sys.stderr)
    return found


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--search":
        torch.set_num_threads(2)
        for nm in sys.argv[2:]:
            if nm in ("tts-b33", "t2-b33"):
                print(f'    "{nm}": {_search_stop(nm, nm == "tts-b33")},', flush=True)
            elif nm in TTS_CALLS:
                print(f'    "{nm}": {_search_tts(nm)},', flush=True)
            elif nm == "nostop":
                print(f'    "{nm}": {_search_nostop()},', flush=True)
            else:
                print(f'    "{nm}": {_search_lsa(nm)},', flush=True)
