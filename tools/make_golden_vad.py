#!/usr/bin/env python
"""tests/golden/vad_post.npz: the REFERENCE's own ``trim_long_silences`` (examples/ge2e/audio_processor.py:53-107) on fixed
voice flags.

Patches, applied at run time in this tool only:
  * ``webrtcvad`` is a stub module whose ``Vad.is_speech`` returns the supplied flags in order (the detector itself is
    third-party C and not part of what is pinned here); ``librosa`` is an empty stub module;
  * ``scipy.ndimage.morphology`` is aliased to ``scipy.ndimage`` where scipy has dropped the old name;
  * ``np.bool = bool`` where numpy lacks it: the reference uses the alias numpy 1.24 removed (numpy 2 has it again).
Tiny cases: sampling rate 1000 and a 4 ms window, so a window is 4 samples (1 ms, one sample, for the cases of a few hundred
windows); the samples lie on a grid of 1 / 4096 (all different within a case's reach, and the file stays small).  The file
holds data only: per case the wav, the
flags, the parameters (window in ms, W, S, sampling rate) and what the function returned -- a gather of the wav's own
samples, so a comparison is bit for bit.
Needs the reference checkout and scipy.  Run from the repository root:  python tools/make_golden_vad.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

SR = 1000
FEED = []          # the flags the stub detector hands out, in order


def cases():
    """name -> (n_w, tail samples, flags, W, S, window in ms)"""
    rng = np.random.default_rng(53)
    out = {}
    for W in range(1, 10):                                   # every width against a random pattern with runs, S = 6
        n = 40 + 3 * W
        f = np.repeat(rng.uniform(size=n // 3 + 1) < 0.5, 3)[:n]
        out[f"width{W}"] = (n, W % 4, f, W, 6)
    for S in range(0, 9):                                    # every dilation, W = 8 and W = 3
        n = 50 + S
        f = np.repeat(rng.uniform(size=n // 4 + 1) < 0.4, 4)[:n]
        out[f"silence{S}"] = (n, (S + 1) % 4, f, 8 if S % 2 == 0 else 3, S)
    for n in (1, 2, 3, 7, 8, 9):                             # fewer windows than the average and the dilation span
        out[f"short{n}"] = (n, 1, rng.uniform(size=n) < 0.6, 8, 6)
    out["ones1"] = (1, 0, np.ones(1, bool), 8, 6)
    out["zeros1"] = (1, 3, np.zeros(1, bool), 8, 6)
    out["all_zero"] = (37, 2, np.zeros(37, bool), 8, 6)
    out["all_one"] = (41, 0, np.ones(41, bool), 8, 6)
    out["isolated"] = (60, 1, np.arange(60) % 7 == 0, 2, 1)    # single flags: 2 c > W fails at W = 2 ... and holds at W = 1
    out["isolated_w1"] = (60, 1, np.arange(60) % 7 == 0, 1, 2)
    for n in (255, 256, 257, 300, 513):                      # a few hundred windows, random and in long runs
        out[f"random{n}"] = (n, n % 4, rng.uniform(size=n) < 0.5, 5, 3)
        out[f"runs{n}"] = (n, (n + 1) % 4, np.repeat(rng.uniform(size=n // 9 + 1) < 0.45, 9)[:n], 8, 6)
    return {k: v + ((1 if v[0] > 200 else 4),) for k, v in out.items()}


def main():
    if not hasattr(np, "bool"):
        np.bool = bool
    vad = types.ModuleType("webrtcvad")

    class Vad:
        def __init__(self, mode=None):
            pass

        def is_speech(self, buf, sample_rate=None):
            return bool(FEED.pop(0))
    vad.Vad = Vad
    sys.modules["webrtcvad"] = vad
    sys.modules["librosa"] = types.ModuleType("librosa")
    try:
        import scipy.ndimage.morphology  # noqa: F401
    except ImportError:
        import scipy.ndimage
        sys.modules["scipy.ndimage.morphology"] = scipy.ndimage
    spec = importlib.util.spec_from_file_location("ref_ge2e_audio", os.path.join(ref_import.REF, "examples", "ge2e",
                                                                                 "audio_processor.py"))
    ap = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ap)
    names, wavs, flgs, params, outs = [], [], [], [], []
    for name, (n_w, tail, flags, W, S, ms) in sorted(cases().items()):
        w = ms * SR // 1000
        tail = tail % w
        wav = (((np.arange(n_w * w + tail) * 37 + 11) % 4093 - 2046) / 4096.0).astype(np.float32)
        FEED[:] = list(flags)
        got = ap.trim_long_silences(wav.copy(), ms, W, S, SR)
        assert not FEED and got.dtype == np.float32
        names.append(name)
        wavs.append(wav)
        flgs.append(np.asarray(flags, bool))
        params.append([ms, W, S, SR])
        outs.append(got)
    # one array per kind (a zip member per case would cost more than its data): tests/trim_ref.py vad_golden() splits them
    out = dict(names=np.array(names), params=np.array(params, np.int64), wav=np.concatenate(wavs), flags=np.concatenate(flgs),
               out=np.concatenate(outs), wav_len=np.array([a.size for a in wavs], np.int64),
               out_len=np.array([a.size for a in outs], np.int64))
    path = os.path.join(ref_import.golden_dir(), "vad_post.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
