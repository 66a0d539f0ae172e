"""FastSpeech2 with given durations, pitch and energy, CPU side: the fp32 restatement (tests/fs2_forward_ref.py) against
the golden vectors the reference's own source produced (tools/make_golden_fs2_forward.py -> golden/fs2_forward.npz), the
new exports of the C boundary, and the host reference of ``audio.average_by_duration``."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fs2_forward_cases as cases  # noqa: E402
import fs2_forward_ref as fref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fs2_forward.npz")
TOL = 2e-5      # the oracle <-> golden bar of tests/test_golden_cpu.py (max-abs, fp32 restatement vs fp32 reference source)
NEW_EXPORTS = ("pk_fs2_set_targets", "pk_fs2_read_predictions", "pk_fs2_read_before", "pk_op_average_by_duration")


def test_golden_file_holds_every_case():
    g = np.load(GOLD)
    assert str(g["cases"]).split(",") == list(cases.CASES)
    assert int(g["seed"]) == cases.SEED
    assert os.path.getsize(GOLD) < 1 << 20
    for name in cases.CASES:        # the stored targets are the ones the case table regenerates
        for b, u in enumerate(cases.case_inputs(name)):
            for k in ("ids", "ds", "ps", "es"):
                assert np.array_equal(g[f"{name}_{k}{b}"], u[k]), (name, k)


def test_restatement_matches_reference_source():
    g = np.load(GOLD)
    for name, (_, how, _, _) in cases.CASES.items():
        cfg, state = cases.case_cfg(name), cases.case_state(name)
        r = cfg.get("reduction_factor", 1)
        for b, u in enumerate(cases.case_inputs(name)):
            out = fref.forward(state, u["ids"], u["ds"], u["ps"], u["es"], cfg, spk_id=u.get("spk_id"),
                               spembs=u.get("spembs"))
            after = out["after"].numpy()
            assert after.shape == g[f"{name}_after{b}"].shape == (r * int(u["ds"].sum()), 80), name     # lengths: exact
            assert np.abs(after - g[f"{name}_after{b}"]).max() < TOL, name
            if how == "inference":
                continue
            for k in ("before", "d_outs", "p_outs", "e_outs"):
                got = out[k].numpy()
                assert got.shape == g[f"{name}_{k}{b}"].shape, (name, k)
                assert np.abs(got - g[f"{name}_{k}{b}"]).max() < TOL, (name, k)
        if how == "forward":        # forward() trims speech lengths to a multiple of r (:369-373)
            want = [u["olen"] - u["olen"] % r for u in cases.case_inputs(name)]
            assert list(g[f"{name}_olens_out"]) == want and int(g[f"{name}_ys_len"]) == max(want)


def test_given_targets_are_live_in_the_restatement():
    name = "t7"
    cfg, state, u = cases.case_cfg(name), cases.case_state(name), cases.case_inputs(name)[0]
    a = fref.forward(state, u["ids"], u["ds"], u["ps"], u["es"], cfg)
    b = fref.forward(state, u["ids"], u["ds"], u["ps"] + 1.0, u["es"], cfg)
    assert np.abs(a["after"].numpy() - b["after"].numpy()).max() > 1e-3
    assert np.array_equal(a["d_outs"].numpy(), b["d_outs"].numpy()) and np.array_equal(a["p_outs"].numpy(), b["p_outs"].numpy())


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pk_synth.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))


def test_new_exports_in_header_binding_and_library():
    import __graft_entry__ as ge
    ge.build()
    from parakeet_amd import _capi
    lib = _capi.lib()
    bound = _capi._declare(lib)
    declared = _declared_symbols()
    for s in NEW_EXPORTS:
        assert s in declared, f"include/pk_synth.h does not declare {s}"
        assert s in bound, f"_capi does not bind {s}"
        assert hasattr(lib, s), f"libpk_synth.so does not export {s}"
    # argument counts of the bindings are the header's
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pk_synth.h")).read(), flags=re.S)
    for s in NEW_EXPORTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % s, text).group(1)
        assert len(bound[s][1]) == len(args.split(",")), s


def _average_loop(x, d):
    """What the reference's loop computes (get_feats.py:205-214): per token the mean of its slice of frames, 0 if empty."""
    out, start = [], 0
    for n in d:
        part = x[start:start + int(n)]
        out.append(part.mean(axis=0) if len(part) else np.zeros(x.shape[1:], x.dtype))
        start += int(n)
    return np.array(out)


def test_average_by_duration_host_reference():
    from parakeet_amd.audio import average_by_duration_numpy
    rng = np.random.default_rng(5)
    for shape, d in (((12,), [3, 0, 4, 0, 0, 5]), ((12, 3), [0, 0, 12]), ((9,), [0, 2, 0, 7, 0]), ((7,), [1] * 7),
                     ((10,), [4, 4, 4]), ((10,), [2, 3])):          # spans past the last frame are cut like a slice
        x = rng.normal(size=shape).astype(np.float64)
        got = average_by_duration_numpy(x, np.array(d))
        want = _average_loop(x, d)
        assert got.shape == want.shape == (len(d),) + tuple(shape[1:])
        assert np.abs(got - want).max() < 1e-12, (shape, d)
        for t, n in enumerate(d):
            if n == 0:
                assert not np.any(got[t])
    x32 = rng.normal(size=(20,)).astype(np.float32)
    assert average_by_duration_numpy(x32, [5, 0, 15]).dtype == np.float32
