"""Cases, inputs and float64 references of the speaker-encoder sweep (tests/test_spk_lstm_cpu.py, tests/test_spk_lstm_gpu.py).

The GE2E speaker encoder (csrc/spk.hip: ``k_spk_pad_in``, the layer GEMMs, ``k_spk_lstm_rec``, ``k_spk_head``) is driven through
``LSTMSpeakerEncoder`` and compared with ``tests/ge2e_ref.py`` in float64.

Probe.  There is no debug read for the encoder.  The recurrence groups (A - D) use ``output_size = 2 H``, ``linear.weight =
[I | -I]`` and a zero bias: the embedding is normalize([relu(h), relu(-h)]), h(T) of the last layer element by element up to its
norm, so a wrong hidden unit shows up as that unit and is not averaged through a random projection.  The head group (E) uses the
Xavier head of ``synthetic.ge2e_state``.

Groups (CASES below; all seeded, inputs exp(N(-2, 2)) as a power mel has them, zero initial states unless said).
  A  every hidden size 32 ... 512, two layers, T 12, P 33 (a full tile and a one-row tail): every wave occupancy of both UBW
     instantiations of the recurrence (H = 32: seven idle waves; H = 288 ... 480: some waves with two unit blocks, some with one),
     and ``hseq`` of a second unit block read by the second layer's GEMM.
  B  initial states: H 32, 96, 256, 288, 512 x 2 and 3 layers x T 1, 2, 3, 8.  ``h0`` rows of magnitude 10^U(-4, 1) each (the row
     exponent of the split path), ``c0`` N(0, 2).  T is short on purpose: an LSTM forgets its initial state, and after 40 steps a
     wrong state offset moves the result by less than the bar (``layer0_states`` below is asserted on this group only).
  C  tile and length edges: H 64 and 320, three layers, every P of 1, 31, 32, 33, 64, 65, 97 and every T of 1, 2, 160 at least
     once per H.
  D  input widths: n_mels 1, 32 (no padding), 33, 257 at H 288 and the limit 4096 at H 32; P 5, T 3, two layers.  Above 512
     channels layer 0 is projected by k_spk_proj_wide (fp64 accumulators) instead of the tile GEMM: 512 and 513 at H 288 are the
     two sides of that threshold.
  E  the head: O 32, 288, 4096 x H 32, 512, one layer, T 6, 73 partials per partial and as utterances of 1, 2 and 70 partials;
     "E-zero": O 288, bias -100 on all but four outputs and inputs picked (from the float64 reference) so that one partial of a
     four-partial utterance has an all-zero ReLU output among live ones (the 1e-12 clamp, and the mean over a zero row).
  G  the size refusal: H 512, n_mels 1, one partial of REFUSED_T = 2^30 / 4H + 1 frames (a 2 MB input) must be refused before
     anything is launched; "G-small" is the small call on the same model that must be right afterwards.  (No case just under
     the limit: half a million sequential steps over a 4 GB buffer.)
Group F (bit-exact properties) needs no reference and lives in the GPU test.

Bar.  Per case and compared quantity ("seq": the per-partial embeddings, "utt": the utterance embeddings):
    e32 = max over two float32 evaluations of |float32 - float64|,      bar = 4 * max(e32, ulp32(peak |float64 value|))
from the references alone.  The two float32 evaluations are ge2e_ref in float32 as it stands, and with the recurrent product
summed in 16-wide k chunks, last chunk first, so that the figure does not rest on one summation order.  The factor 4: the input
GEMM, the recurrent product and the device's tanhf / expf each round differently from the oracle, and the split-fp16 path may
carry twice the exact path's error (the rule tests/test_pwg_gpu.py and tests/test_fs2_gpu.py hold the split path to).

Planted defects.  ``restated`` is a second float64 statement of the model in plain numpy with switches (DEFECTS).  With no
switch it reproduces ge2e_ref; every defect ``applicable`` to a case has to move the float64 result by at least DEFECT_MARGIN x
that case's bar (tests/test_spk_lstm_cpu.py) -- a condition on the inputs, checked without a GPU.

Not a bar defect: a tile-wide ``h0`` exponent in place of the per-row one.  Small rows contribute little in absolute terms, so
the probe stays below 0.1 x bar; the bitwise batch-invariance test of group F guards it instead.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from parakeet_amd import synthetic as syn   # noqa: E402
import ge2e_ref                              # noqa: E402

MATHS = ("f32", "f16x3")
TILE = 32                 # SPK_M: partials per workgroup
DEFECT_MARGIN = 8.0
UTTERANCES = (1, 2, 70)   # group E: partials per utterance


def _case(name, group, H, layers, T, P, n_mels=40, head="identity", O=None, states=False, seed=0, utterances=None):
    return dict(name=name, group=group, H=H, layers=layers, T=T, P=P, n_mels=n_mels, head=head,
                O=2 * H if head == "identity" else O, states=states, seed=seed, utterances=utterances)


def _build():
    cases = []
    for i, H in enumerate(range(32, 513, 32)):
        cases.append(_case(f"A-h{H}", "A", H, 2, 12, 33, seed=100 + i))
    i = 0
    for H in (32, 96, 256, 288, 512):
        for L in (2, 3):
            for T in (1, 2, 3, 8):
                cases.append(_case(f"B-h{H}-l{L}-t{T}", "B", H, L, T, 33, states=True, seed=200 + i))
                i += 1
    edges = {64: ((1, 160), (31, 1), (32, 2), (33, 160), (64, 1), (65, 2), (97, 160)),
             320: ((1, 2), (31, 160), (32, 1), (33, 2), (64, 160), (65, 1), (97, 2))}
    i = 0
    for H, pts in edges.items():
        for P, T in pts:
            cases.append(_case(f"C-h{H}-p{P}-t{T}", "C", H, 3, T, P, seed=300 + i))
            i += 1
    # (512 and 513: the two sides of SPK_GEMM_MAX_IN, the tile GEMM and k_spk_proj_wide; 4 H = 1152 is 4.5 of its column blocks)
    for i, (H, C) in enumerate(((288, 1), (288, 32), (288, 33), (288, 257), (32, 4096), (288, 512), (288, 513))):
        cases.append(_case(f"D-h{H}-m{C}", "D", H, 2, 3, 5, n_mels=C, seed=400 + i))
    i = 0
    for H in (32, 512):
        for O in (32, 288, 4096):
            cases.append(_case(f"E-h{H}-o{O}", "E", H, 1, 6, sum(UTTERANCES), head="xavier", O=O, seed=500 + i,
                               utterances=UTTERANCES))
            i += 1
    cases.append(_case("E-zero", "E", 32, 1, 6, 7, head="zero", O=288, seed=520, utterances=(3, 4)))
    cases.append(_case("G-small", "G", 512, 1, 3, 2, n_mels=1, seed=600))
    return tuple(cases)


CASES = _build()
CASE = {c["name"]: c for c in CASES}
NAMES = tuple(c["name"] for c in CASES)
GROUPS = ("A", "B", "C", "D", "E", "G")
REFUSED_T = (1 << 30) // (4 * 512) + 1     # group G: one row more than 2^30 / 4H at H = 512, in one partial

ZERO_LIVE = (0, 255, 256, 287)   # E-zero: the outputs that keep a zero bias (both trips of the head's stride loop); the
                                 # others get ZERO_BIAS
ZERO_BIAS = -100.0
ZERO_MARGIN = 1e-3       # the picked pre-activations keep this distance from zero (far above any float32 error)
ZERO_ROW = 4             # E-zero: the partial with the all-zero ReLU output (second partial of the second utterance)
ZERO_POOL = 256


def config(name):
    c = CASE[name]
    return dict(n_mels=c["n_mels"], num_layers=c["layers"], hidden_size=c["H"], output_size=c["O"])


def state(name):
    """The float32 state dict of a case (a new dict per call)."""
    c = CASE[name]
    st = syn.ge2e_state(config(name), seed=c["seed"])
    H = c["H"]
    if c["head"] == "identity":
        eye = np.eye(H, dtype=np.float32)
        st["linear.weight"] = np.concatenate([eye, -eye], 1)
        st["linear.bias"] = np.zeros(2 * H, dtype=np.float32)
    elif c["head"] == "zero":
        b = np.full(c["O"], ZERO_BIAS, dtype=np.float32)
        b[list(ZERO_LIVE)] = 0.0
        st["linear.bias"] = b
    return st


def partials(P, T, n_mels, seed):
    """Power-mel-like inputs: magnitudes spread over decades, as the front end produces."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(-2.0, 2.0, size=(P, T, n_mels))).astype(np.float32)


def initial_states(L, P, H, seed, special_rows=False):
    """h0 with one magnitude per row, 10^U(-4, 1), c0 N(0, 2).  special_rows: row 1 all zero, row 2 of magnitude 1e-30."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-4.0, 1.0, size=(L, P, 1))
    h0 = (rng.uniform(-1.0, 1.0, size=(L, P, H)) * mag).astype(np.float32)
    c0 = (rng.standard_normal((L, P, H)) * 2.0).astype(np.float32)
    if special_rows:
        h0[:, 1] = 0.0
        h0[:, 2] = (rng.uniform(-1.0, 1.0, size=(L, H)) * 1e-30).astype(np.float32)
    return h0, c0


def _zero_case_inputs(c, st):
    """E-zero: seven partials out of a seeded pool, chosen from the float64 pre-activations of the live outputs: row ZERO_ROW
    has all of them below -ZERO_MARGIN, every other row has one above ZERO_MARGIN."""
    pool = partials(ZERO_POOL, c["T"], c["n_mels"], 1000 + c["seed"])
    h = ge2e_ref.lstm_last_hidden(st, pool, c["layers"]).numpy()
    pre = (h @ np.asarray(st["linear.weight"], np.float64))[:, list(ZERO_LIVE)]
    dead = np.nonzero((pre < -ZERO_MARGIN).all(1))[0]
    live = np.nonzero((pre > ZERO_MARGIN).any(1))[0]
    assert len(dead) >= 1 and len(live) >= c["P"] - 1, (len(dead), len(live))
    rows = list(live[:c["P"] - 1])
    rows.insert(ZERO_ROW, dead[0])
    return np.ascontiguousarray(pool[rows])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x (P, T, n_mels) float32, (h0, c0) or None); shared, never modified."""
    c = CASE[name]
    if c["head"] == "zero":
        x = _zero_case_inputs(c, state(name))
    else:
        x = partials(c["P"], c["T"], c["n_mels"], 1000 + c["seed"])
    states = initial_states(c["layers"], c["P"], c["H"], 2000 + c["seed"]) if c["states"] else None
    return x, states


def bounds(name):
    """cu_partials of the case's utterances, or None."""
    u = CASE[name]["utterances"]
    return None if u is None else np.concatenate([[0], np.cumsum(u)]).astype(np.int64)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _chunked_last_first(h, whh):
    """h @ whh.T summed in 16-wide k chunks, the last chunk first (float32: another summation order)."""
    H = whh.shape[1]
    acc = None
    for k0 in range(H - 16, -1, -16):
        part = h[:, k0:k0 + 16] @ whh[:, k0:k0 + 16].T
        acc = part if acc is None else acc + part
    return acc


def _quantities(e, cu):
    """{"seq": (P, O)} and, with utterance bounds, {"utt": (U, O)}: mean of an utterance's rows, normalised again."""
    out = {"seq": e}
    if cu is not None:
        out["utt"] = torch.stack([ge2e_ref.normalize(e[a:b].mean(0), 0) for a, b in zip(cu[:-1], cu[1:])])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 references of a case, computed once and never modified: ``seq`` (and ``utt``) as numpy, h(T) of the last
    layer (``h``), and ``e32`` / ``peak`` / ``bar`` per quantity."""
    c, st = CASE[name], state(name)
    x, states = inputs(name)
    cu = bounds(name)
    L = c["layers"]
    e64, layers = ge2e_ref.embed_sequences(st, x, L, states, return_layers=True)
    q64 = {k: v.numpy() for k, v in _quantities(e64, cu).items()}
    runs = (ge2e_ref.embed_sequences(st, x, L, states, dtype=torch.float32),
            ge2e_ref.embed_sequences(st, x, L, states, dtype=torch.float32, rec_matmul=_chunked_last_first))
    out = dict(q64, h=layers[-1][:, -1].numpy(), e32={}, peak={}, bar={})
    for k, w in q64.items():
        w.setflags(write=False)
        e32 = max(float(np.abs(_quantities(r, cu)[k].numpy().astype(np.float64) - w).max()) for r in runs)
        peak = float(np.abs(w).max())
        out["e32"][k], out["peak"][k] = e32, peak
        out["bar"][k] = 4.0 * max(e32, ulp32(peak))
    return out


def error(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


# ---- a second float64 statement of the model, with planted defects -------------------------------------------------------------
# Plain numpy.  defect=None must reproduce ge2e_ref; each switch is a way the kernels could be subtly wrong (an index, a guard, a
# dropped term), and the bar of every case it applies to has to reject it.
DEFECTS = {
    "last_k_chunk": "the last 16 columns of W_hh are dropped (the last k chunk of the split path)",
    "last_8_columns": "the last 8 columns of W_hh are dropped (the hi = 1 half of the last chunk)",
    "h_single_fp16": "h(t-1) is rounded to one fp16 term at its scale (2^14; the row's own for h0): no lo part",
    "layer0_states": "every layer takes the initial states of layer 0",
    "c0_last_block_zero": "c0 of the last 32 units is read as zero",
    "second_block_stale": "H > 256: units >= 256 of h are never written to the next step's operand",
    "last_step_missing": "the next layer sees zeros at t = T - 1",
    "tail_row_neighbour": "row P - 1 of a partial tile reads row P - 2's xg",
    "o_tail_dropped": "head: outputs >= 256 are zero (no second trip of the stride loop)",
    "mean_before_normalise": "head: the utterance mean is taken over un-normalised partial embeddings",
    "pad_column_live": "the guard of the padded input column n_mels is missing: it holds the next row's first value, and the "
                       "packed weight row n_mels holds what follows in W_ih (the next gate's first weight)",
}


def applicable(name, defect):
    """Whether ``defect`` can change the result of the case at all (from the case's shape alone, never from a measurement)."""
    c = CASE[name]
    recurrent = c["T"] >= 2 or c["states"]          # with zero states the first step multiplies W_hh by zero
    if defect in ("last_k_chunk", "last_8_columns"):
        return recurrent
    if defect == "h_single_fp16":
        # one rounded operand moves a gate by about 2^-12 |h| / sqrt(3): it takes the recurrence a few steps to carry that
        # above 8 bars (26 x the bar after 40 steps).  Asserted where the recurrence runs at least 8 steps.
        return c["T"] >= 8
    if defect in ("layer0_states", "c0_last_block_zero"):
        return c["states"]
    if defect == "second_block_stale":
        return c["H"] > 256 and c["T"] >= 2
    if defect == "last_step_missing":
        return c["layers"] >= 2
    if defect == "tail_row_neighbour":
        return c["P"] >= 2 and c["P"] % TILE != 0
    if defect == "o_tail_dropped":
        return c["O"] > 256
    if defect == "mean_before_normalise":
        return c["utterances"] is not None and max(c["utterances"]) >= 2
    if defect == "pad_column_live":
        return c["n_mels"] % 32 != 0
    raise KeyError(defect)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _f64(st, key):
    return np.asarray(st[key], dtype=np.float64)


def _one_fp16(h, unit):
    """One fp16 term under a power-of-two scale: 2^14 (operands bounded by one), or per row the scale that brings the row's
    maximum to [2^13, 2^14) as pk_split.h does for h0."""
    if unit:
        s = np.full((h.shape[0], 1), 2.0 ** 14)
    else:
        m = np.maximum(np.abs(h).max(1, keepdims=True), 2.0 ** -40)
        s = 2.0 ** (13 - np.floor(np.log2(m)))
    return (h * s).astype(np.float16).astype(np.float64) / s


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)


def restated(name, defect=None):
    """{"seq": ..., "utt": ...} of a case from the second statement."""
    assert defect is None or defect in DEFECTS, defect
    c, st = CASE[name], state(name)
    x, states = inputs(name)
    P, T, C = x.shape
    H, L, G = c["H"], c["layers"], 4 * c["H"]
    h_in = x.astype(np.float64)
    for l in range(L):
        wih, whh = _f64(st, f"lstm.weight_ih_l{l}"), _f64(st, f"lstm.weight_hh_l{l}").copy()
        b = _f64(st, f"lstm.bias_ih_l{l}") + _f64(st, f"lstm.bias_hh_l{l}")
        if defect == "last_k_chunk":
            whh[:, -16:] = 0.0
        if defect == "last_8_columns":
            whh[:, -8:] = 0.0
        if states is None:
            h, cell = np.zeros((P, H)), np.zeros((P, H))
        else:
            sl = 0 if defect == "layer0_states" else l
            h, cell = states[0][sl].astype(np.float64), states[1][sl].astype(np.float64)
        if defect == "c0_last_block_zero":
            cell[:, -32:] = 0.0
        xg = h_in @ wih.T + b                                  # (P, T, G)
        if defect == "pad_column_live" and l == 0 and C % 32:
            nxt = np.append(h_in.reshape(-1), 0.0)[(np.arange(P * T) + 1) * C].reshape(P, T, 1)
            wpad = np.append(wih.reshape(-1), 0.0)[(np.arange(G) + 1) * C]
            xg = xg + nxt * wpad
        if defect == "tail_row_neighbour" and P >= 2 and P % TILE:
            xg[P - 1] = xg[P - 2]
        op = h
        outs = []
        for t in range(T):
            a = _one_fp16(op, unit=t > 0 or states is None) if defect == "h_single_fp16" else op
            g = xg[:, t] + a @ whh.T
            gi, gf, gg, go = (g[:, q * H:(q + 1) * H] for q in range(4))
            cell = _sigmoid(gf) * cell + _sigmoid(gi) * np.tanh(gg)
            h = _sigmoid(go) * np.tanh(cell)
            outs.append(h)
            if defect == "second_block_stale" and H > 256:
                op = np.concatenate([h[:, :256], op[:, 256:]], 1)
            else:
                op = h
        h_in = np.stack(outs, 1)
        if defect == "last_step_missing" and l + 1 < L:
            h_in[:, -1] = 0.0
    e = np.maximum(h @ _f64(st, "linear.weight") + _f64(st, "linear.bias"), 0.0)
    if defect == "o_tail_dropped":
        e[:, 256:] = 0.0
    out = {"seq": _normalize(e)}
    cu = bounds(name)
    if cu is not None:
        src = e if defect == "mean_before_normalise" else out["seq"]
        out["utt"] = np.stack([_normalize(src[a:b].mean(0)) for a, b in zip(cu[:-1], cu[1:])])
    return out


def defect_shift(name, defect):
    """max over the case's quantities of |defective float64 result - reference| / bar."""
    ref, got = reference(name), restated(name, defect)
    return max(error(got[k], ref[k]) / ref["bar"][k] for k in got)


if __name__ == "__main__":
    # the table of the CPU test, for reading: e32, bar and every applicable defect's shift per case
    torch.set_num_threads(8)
    for nm in (sys.argv[1:] or NAMES):
        r = reference(nm)
        shifts = {d: defect_shift(nm, d) for d in DEFECTS if applicable(nm, d)}
        print(nm, {k: f"e32 {r['e32'][k]:.2e} bar {r['bar'][k]:.2e}" for k in r["bar"]},
              {d: f"{v:.3g}" for d, v in shifts.items()}, flush=True)
