"""Bring a directory of wavs to one programme loudness: for every *.wav in --in-dir (PCM or float, mono or averaged to mono,
any rate that is a multiple of 10 Hz from 8 000 to 192 000) print the file, its gated loudness in LUFS (ITU-R BS.1770-4), its
sample peak, the gain applied in dB and the peak after it; write the scaled file under the same name to --out-dir; then print
the corpus means of the loudness before and of the gain.  A file whose loudness is -inf (shorter than 400 ms, or nothing above
-70 LUFS) is written unchanged with gain 0 dB.  With --max-peak the gain of a file is capped so that no sample exceeds it.
Files of one rate are measured and scaled in batches of --batch on the engine.

The measure is this project's own restatement of the Recommendation for mono (K-weighting in float64, 400 ms
blocks on a 100 ms sample grid, gates at -70 LUFS and -10 LU); it is not pyloudnorm or libebur128, and nobody has compared its
numbers with another meter's on speech.

    python examples/normalize_loudness.py --in-dir wavs --out-dir wavs_m23 [--target -23] [--max-peak 0.99] [--batch 32]
                                          [--subtype PCM_16]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parakeet_amd import audio  # noqa: E402
from parakeet_amd.metrics import loudness_batch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in-dir", required=True, help="directory of *.wav")
    ap.add_argument("--out-dir", required=True, help="where the scaled files go (created)")
    ap.add_argument("--target", type=float, default=-23.0, help="target loudness in LUFS (default -23; podcasts use -16)")
    ap.add_argument("--max-peak", type=float, default=None, help="cap a file's gain so that no sample exceeds this")
    ap.add_argument("--batch", type=int, default=32, help="files per engine call")
    ap.add_argument("--subtype", default="PCM_16", choices=("PCM_16", "FLOAT"), help="sample format of the written files")
    a = ap.parse_args(argv)
    if a.batch < 1:
        raise SystemExit("--batch must be positive")
    names = sorted(f for f in os.listdir(a.in_dir) if f.endswith(".wav"))
    if not names:
        raise SystemExit(f"no *.wav in {a.in_dir}")
    os.makedirs(a.out_dir, exist_ok=True)
    by_rate = {}
    for f in names:
        wav, sr = audio.load_wav(os.path.join(a.in_dir, f))
        by_rate.setdefault(sr, []).append((f, wav))
    lufs_all, gain_all = [], []
    for sr, items in sorted(by_rate.items()):
        for i in range(0, len(items), a.batch):
            part = items[i:i + a.batch]
            wavs = [w for _, w in part]
            try:
                det = loudness_batch(wavs, sr, return_details=True)
            except NotImplementedError as e:
                for f, _ in part:
                    print(f"{f}\tskipped: {e}", file=sys.stderr)
                continue
            out, gains = audio.normalize_loudness_batch(wavs, sr, a.target, a.max_peak, return_gains=True)
            for (f, _), d, y, g in zip(part, det, out, gains):
                y = y.numpy()
                audio.write_wav(os.path.join(a.out_dir, f), y, sr, subtype=a.subtype)
                gdb = 20.0 * math.log10(float(g))
                peak_after = float(np.abs(y).max()) if y.size else 0.0
                print(f"{f}\t{sr}\t{d['lufs']:.3f}\t{d['peak']:.6f}\t{gdb:+.3f}\t{peak_after:.6f}")
                if math.isfinite(d["lufs"]):
                    lufs_all.append(d["lufs"])
                    gain_all.append(gdb)
    if lufs_all:
        print(f"loudness\t{np.mean(lufs_all):.3f}\ngain_db\t{np.mean(gain_all):+.3f}\tover {len(lufs_all)} files, target {a.target:.3f} LUFS")
    else:
        print(f"loudness\tnan\ngain_db\tnan\tover 0 files, target {a.target:.3f} LUFS")


if __name__ == "__main__":
    main()
