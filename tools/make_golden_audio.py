#!/usr/bin/env python
"""tests/golden/spec_normalizer.npz: the REFERENCE's own spectrogram-magnitude normalizers, parakeet/audio/spec_normalizer.py
(LogMagnitude, UnitMagnitude; numpy only), run on a fixed magnitude field spanning 1e-7 .. 1e2: transform and inverse of both.
tests/test_audio_cpu.py compares parakeet_amd.audio's normalizers with these vectors.  Needs the reference checkout."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("ref_spec_normalizer",
                                                  os.path.join(ref_import.REF, "parakeet", "audio", "spec_normalizer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(3)
    x = np.abs(rng.normal(size=(80, 50))) * 10.0 ** rng.uniform(-7, 2, size=(80, 50))
    out = {"x": x}
    for name, norm in (("log", ref.LogMagnitude()), ("unit", ref.UnitMagnitude())):
        out[name + "_transform"] = norm.transform(x)
        out[name + "_inverse"] = norm.inverse(out[name + "_transform"])
    path = os.path.join(ref_import.golden_dir(), "spec_normalizer.npz")
    np.savez(path, **out)
    print(path)


if __name__ == "__main__":
    main()
