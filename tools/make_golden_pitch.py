#!/usr/bin/env python
"""tests/golden/pitch_post.npz: the REFERENCE's own steps after the f0 estimator, on fixed f0 tracks.

Runs ``Pitch._convert_to_continuous_f0``, ``Pitch._average_by_duration`` and ``Pitch.get_pitch`` of
parakeet/data/get_feats.py (:99-164).  Patches, applied at run time in this tool only:
  * ``pyworld`` and ``librosa`` are stub modules: ``pyworld.dio`` returns the f0 track that was handed in as the "wav" (the
    estimator itself is third-party C++ and not part of what is pinned here), ``pyworld.stonemask`` is the identity;
  * ``np.float = float``: the reference uses the alias numpy has removed.
The file holds data only: per case the f0 track, the durations, and what the three methods returned.
Needs the reference checkout and scipy.  Run from the repository root:  python tools/make_golden_pitch.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def cases():
    rng = np.random.default_rng(20)
    v = lambda n: rng.uniform(90.0, 380.0, n)   # noqa: E731
    z = np.zeros
    out = {
        "voiced": (v(12), [3, 0, 4, 5]),
        "lead_trail": (np.concatenate([z(3), v(7), z(4)]), [2, 2, 0, 0, 6, 4]),
        "one_voiced": (np.concatenate([z(5), v(1), z(6)]), [12]),
        "one_voiced_first": (np.concatenate([v(1), z(4)]), [1, 4]),
        "unvoiced": (z(9), [4, 5]),
        "gap1": (np.concatenate([v(4), z(1), v(3), z(1), v(2)]), [1] * 11),
        "gap_many": (np.concatenate([v(2), z(17), v(1), z(9), v(3)]), [10, 0, 7, 15]),
        "two_frames": (np.array([0.0, 140.0]), [0, 2]),
        "two_voiced_ends": (np.concatenate([v(1), z(38), v(1)]), [13, 13, 14]),
        "mixed": (np.where(rng.uniform(size=40) < 0.5, 0.0, v(40)), [5, 0, 0, 9, 1, 20, 5]),
        "short_durations": (np.concatenate([z(2), v(6), z(2)]), [2, 3]),
    }
    return {k: (np.asarray(f, np.float64), np.asarray(d, np.int64)) for k, (f, d) in out.items()}


def main():
    np.float = float
    pw = types.ModuleType("pyworld")
    pw.dio = lambda x, fs=None, f0_floor=None, f0_ceil=None, frame_period=None: (np.array(x, np.float64), None)
    pw.stonemask = lambda x, f0, t, fs: f0
    sys.modules["pyworld"] = pw
    sys.modules["librosa"] = types.ModuleType("librosa")
    spec = importlib.util.spec_from_file_location("ref_get_feats", os.path.join(ref_import.REF, "parakeet", "data", "get_feats.py"))
    gf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gf)
    p = gf.Pitch(sr=24000, hop_length=300, f0min=80, f0max=7600)
    out = {"names": np.array(sorted(cases()))}
    for name, (f0, d) in cases().items():
        out[f"{name}_f0"] = f0
        out[f"{name}_d"] = d
        out[f"{name}_cont"] = np.asarray(p._convert_to_continuous_f0(f0.copy()), np.float64)
        out[f"{name}_log"] = np.asarray(p.get_pitch(f0.copy(), use_continuous_f0=True, use_log_f0=True), np.float64)
        out[f"{name}_rawlog"] = np.asarray(p.get_pitch(f0.copy(), use_continuous_f0=False, use_log_f0=True), np.float64)
        out[f"{name}_avg"] = np.asarray(p._average_by_duration(f0.copy(), d), np.float64)
        out[f"{name}_pitch"] = np.asarray(p.get_pitch(f0.copy(), duration=d), np.float64)
    path = os.path.join(ref_import.golden_dir(), "pitch_post.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
