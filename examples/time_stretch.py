"""Change the speed and / or the pitch of a directory of wavs: every *.wav in --in-dir (PCM or float, mono or averaged to
mono, any rate) is stretched by --rate (> 1 faster and shorter, < 1 slower and longer; the pitch stays) and / or shifted by
--n-steps (semitones by default, up for positive; the length stays), and written under the same name and at the same rate to
--out-dir.  With both, the stretch comes first.  The whole directory runs as ONE ragged batch per effect on the engine.  One
line per file: name, rate of the file, samples in, samples out.

The effects are ``librosa.effects.time_stretch`` / ``pitch_shift`` over this project's restatement of librosa's phase vocoder
(DESIGN.md 4.5i): no phase locking, so the usual phasiness and an amplitude loss on stretched steady tones remain; the pitch
shift resamples with this project's own filter at a rational ratio within 0.03 cent of the one asked for.  Nobody has compared
either effect with librosa's output or listened to it on speech.

    python examples/time_stretch.py --in-dir wavs --out-dir wavs_slow --rate 0.8 [--n-steps -2] [--bins-per-octave 12]
                                    [--n-fft 2048] [--hop-length 512] [--transform dense|fft] [--subtype PCM_16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parakeet_amd import audio  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in-dir", required=True, help="directory of *.wav")
    ap.add_argument("--out-dir", required=True, help="where the results go (created)")
    ap.add_argument("--rate", type=float, default=None, help="time-stretch rate: 2 is twice as fast, 0.5 half as fast")
    ap.add_argument("--n-steps", type=float, default=None, help="pitch shift in steps of an octave / --bins-per-octave")
    ap.add_argument("--bins-per-octave", type=int, default=12)
    ap.add_argument("--n-fft", type=int, default=2048, help="a multiple of 16 (a power of two from 32 to 4096 with --transform fft)")
    ap.add_argument("--hop-length", type=int, default=None, help="a multiple of 4 (default: n_fft / 4)")
    ap.add_argument("--transform", default="dense", choices=("dense", "fft"))
    ap.add_argument("--subtype", default="PCM_16", choices=("PCM_16", "FLOAT"), help="sample format of the written files")
    a = ap.parse_args(argv)
    if a.rate is None and a.n_steps is None:
        raise SystemExit("give --rate, --n-steps or both")
    names = sorted(f for f in os.listdir(a.in_dir) if f.endswith(".wav"))
    if not names:
        raise SystemExit(f"no *.wav in {a.in_dir}")
    os.makedirs(a.out_dir, exist_ok=True)
    loaded = [audio.load_wav(os.path.join(a.in_dir, f)) for f in names]
    wavs, srs = [w for w, _ in loaded], [sr for _, sr in loaded]
    kw = dict(n_fft=a.n_fft, hop_length=a.hop_length, transform=a.transform)
    out = wavs
    if a.rate is not None:
        out = audio.time_stretch_batch(out, a.rate, **kw)
    if a.n_steps is not None:
        # the files' rates may differ: the ratio of the shift does not depend on the sampling rate
        out = audio.pitch_shift_batch(out, srs[0], a.n_steps, a.bins_per_octave, **kw)
    for f, sr, x, y in zip(names, srs, wavs, out):
        y = y.numpy() if hasattr(y, "numpy") else y
        audio.write_wav(os.path.join(a.out_dir, f), y, sr, subtype=a.subtype)
        print(f"{f}\t{sr}\t{len(x)}\t{len(y)}")


if __name__ == "__main__":
    main()
