"""The cases of tests/golden/fs2_forward.npz: one table for the generator (tools/make_golden_fs2_forward.py), the
restatement test (test_fs2_forward_cpu.py) and the engine test (test_fs2_forward_gpu.py).  Weights and targets are
regenerated from seeds; the file stores the reference's outputs (and the targets, so a reader needs no generator)."""
import numpy as np

from parakeet_amd import synthetic as syn

SEED = 2031
SMALL = dict(elayers=2, dlayers=2)

# name -> (configuration overrides, how the reference was called, token counts, speaker conditioning)
#   "_forward": FastSpeech2._forward(xs, ilens, olens, ds, ps, es, is_inference=False) with B = 1
#   "forward":  FastSpeech2.forward(...) per utterance (B = 1), or for a batch of equal lengths
#   "inference": FastSpeech2.inference(..., use_teacher_forcing=True), which the reference's `if durations:` (:516) lets
#                run for T = 1 only
CASES = {
    "t1": (dict(), "_forward", [1], None),
    "t7": (dict(), "forward", [7], None),
    "t40": (dict(), "_forward", [40], None),
    "zero_dur": (dict(), "forward", [7], None),                       # durations of 0 inside the utterance
    "spk_add": (dict(spk_embed_dim=256, spk_embed_integration_type="add"), "forward", [7], "spk_id"),
    "spk_concat": (dict(spk_embed_dim=256, spk_embed_integration_type="concat"), "_forward", [9], "spembs"),
    "r2": (dict(reduction_factor=2), "forward", [7], None),
    "postnorm": (dict(encoder_normalize_before=False, decoder_normalize_before=False), "_forward", [7], None),
    "linear": (dict(positionwise_layer_type="linear"), "forward", [7], None),
    "batch3": (dict(), "forward", [7, 7, 7], None),                   # equal token counts AND equal frame counts
    "tf_t1": (dict(), "inference", [1], None),
}
NUM_SPEAKERS = 6


def case_cfg(name):
    return dict(syn.FS2_LJSPEECH, **SMALL, **CASES[name][0])


def case_state(name):
    cfg = case_cfg(name)
    return syn.fastspeech2_state(80, 80, cfg, seed=SEED, num_speakers=NUM_SPEAKERS if "spk_embed_dim" in cfg else None)


def model_kwargs(name):
    cfg = case_cfg(name)
    if "spk_embed_dim" in cfg:
        cfg["num_speakers"] = NUM_SPEAKERS
    return cfg


def case_inputs(name):
    """Per utterance: dict(ids, ds, ps, es[, spk_id | spembs], olen) -- olen is the speech length handed to forward()."""
    over, _, toks, spk = CASES[name]
    r = over.get("reduction_factor", 1)
    idx = list(CASES).index(name)
    rng = np.random.default_rng(SEED + 100 + idx)
    utts = []
    for b, T in enumerate(toks):
        ids = syn.phoneme_ids(T, 80, seed=SEED + 1000 + 10 * idx + b)
        if name == "zero_dur":
            ds = np.array([2, 0, 3, 0, 0, 1, 4], dtype=np.int64)
        elif name == "batch3":
            ds = np.array([[1, 2, 3, 0, 2, 1, 3], [3, 3, 0, 1, 1, 2, 2], [2, 2, 2, 2, 2, 1, 1]][b], dtype=np.int64)
        else:
            ds = rng.integers(0, 5, size=T).astype(np.int64)
            ds[0] = max(int(ds[0]), 1)
        u = dict(ids=ids, ds=ds, ps=rng.normal(size=T).astype(np.float32), es=rng.normal(size=T).astype(np.float32),
                 olen=int(ds.sum()) * r + (1 if r > 1 else 0))        # r > 1: a remainder that forward() trims (:369-373)
        if spk == "spk_id":
            u["spk_id"] = 3
        elif spk == "spembs":
            u["spembs"] = rng.normal(size=256).astype(np.float32)
        utts.append(u)
    return utts
