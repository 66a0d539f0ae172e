"""Score vocoder output against the recordings with the multi-resolution STFT loss of the Parallel WaveGAN recipes: for every
<utt_id>.wav in --gen-dir with a <utt_id>.wav in --ref-dir (PCM or float, any rate) print the utterance id, the samples
scored, the spectral convergence loss and the log STFT magnitude loss (each the mean over the resolutions), then the corpus
means of the two -- what the reference's evaluator reports as eval/spectral_convergence_loss and
eval/log_stft_magnitude_loss when it scores one utterance per batch.  A pair of unequal length is trimmed to the shorter one,
and the line says so.  A pair is scored at the recording's rate: generated audio at another rate is resampled to it on the
engine (parakeet_amd.audio.load_wav), and the line says so.

With --discriminator-checkpoint (a snapshot_iter_*.pdz, which carries discriminator_params beside generator_params; needs
--config for the discriminator's shape) every line gains four columns from the recipe's discriminator: the mean logit of the
generated audio, eval/adversarial_loss and eval/fake_loss of it and eval/real_loss of the recording; their corpus means follow
the two STFT lines.  Without it the output is what it always was.

With --stoi every line gains two columns, the short-time objective intelligibility of the generated wav against the recording
(STOI, Taal et al. 2011) and its extended form (ESTOI, Jensen & Taal 2016), on the pair as trimmed above and resampled to 10 kHz
on the engine; the corpus means follow (over the pairs long enough to have a segment; shorter ones print nan).  The measure is
this project's restatement of the papers, not pystoi's or MATLAB's code.

With --loudness every line gains three columns, the gated programme loudness (ITU-R BS.1770-4, LUFS) of the generated wav and
of the recording and their difference in LU, on the pair as trimmed above at the recording's rate; the corpus means follow (over
the pairs where both are finite; a signal shorter than 400 ms or below -70 LUFS prints -inf).  The measure is this project's
restatement of the Recommendation for mono, not pyloudnorm or libebur128; a pair at a rate that is no multiple
of 10 Hz in 8 000 ... 192 000 prints nan.

    python examples/score_vocoder.py --gen-dir generated --ref-dir recordings [--config conf/default.yaml]
                                     [--discriminator-checkpoint snapshot_iter_400000.pdz] [--stoi] [--loudness]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parakeet_amd.audio import load_wav  # noqa: E402
from parakeet_amd.stft_loss import MultiResolutionSTFTLoss  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gen-dir", required=True, help="generated waveforms")
    ap.add_argument("--ref-dir", required=True, help="recordings")
    ap.add_argument("--config", default=None, help="Parallel WaveGAN yaml; its stft_loss_params are used (default: the "
                                                   "reference's 1024/120/600, 2048/240/1200, 512/50/240, hann)")
    ap.add_argument("--batch", type=int, default=16, help="pairs per call")
    ap.add_argument("--discriminator-checkpoint", default=None,
                    help="snapshot with discriminator_params: adds the discriminator's columns (needs --config)")
    ap.add_argument("--stoi", action="store_true", help="add STOI and ESTOI of generated against recording (at 10 kHz)")
    ap.add_argument("--loudness", action="store_true", help="add BS.1770 loudness (LUFS) of generated and recording, and the difference")
    a = ap.parse_args(argv)
    params, disc = {}, None
    if a.config:
        import yaml
        with open(a.config) as f:
            cfg = yaml.safe_load(f)
        params = dict(cfg.get("stft_loss_params") or {})
    if a.discriminator_checkpoint:
        if not a.config:
            raise SystemExit("--discriminator-checkpoint needs --config (the discriminator_params of the recipe)")
        from parakeet_amd.checkpoint import load_pwg_discriminator
        disc = load_pwg_discriminator(cfg, a.discriminator_checkpoint)
    crit = MultiResolutionSTFTLoss(**params)
    need = max(crit.fft_sizes) // 2 + 1
    ids = sorted(f[:-4] for f in os.listdir(a.gen_dir) if f.endswith(".wav") and os.path.exists(os.path.join(a.ref_dir, f)))
    if not ids:
        raise SystemExit("no <utt_id>.wav present in both directories")
    rows, drows, srows, lrows = [], [], [], []
    for i in range(0, len(ids), a.batch):
        xs, ys, kept, notes, rates = [], [], [], [], []
        for u in ids[i:i + a.batch]:
            (x, sx), (y, sy) = load_wav(os.path.join(a.gen_dir, u + ".wav")), load_wav(os.path.join(a.ref_dir, u + ".wav"))
            rnote = ""
            if sx != sy:
                rnote = f"\tresampled from {sx} Hz to {sy} Hz"
                x = load_wav(os.path.join(a.gen_dir, u + ".wav"), sr=sy)[0]
            n = min(len(x), len(y))
            if n < need:
                print(f"{u}\tskipped: {n} samples, the largest transform needs {need}", file=sys.stderr)
                continue
            notes.append(("" if len(x) == len(y) else f"\ttrimmed from {len(x)} / {len(y)}") + rnote)
            xs.append(x[:n])
            ys.append(y[:n])
            kept.append(u)
            rates.append(int(sy))
        if not kept:
            continue
        per = crit.per_utterance(xs, ys).mean(axis=1)            # (B, 2): mean over the resolutions
        extra = [""] * len(kept)
        if disc is not None:
            (sf, nf), (sr, nr), ml = disc.scores(xs), disc.scores(ys), disc.mean_logit(xs)
            d = np.stack([ml, sf[:, 0] / nf, sf[:, 1] / nf, sr[:, 0] / nr], 1)   # mean logit, adversarial, fake, real
            extra = ["".join(f"\t{v:.6f}" for v in row) for row in d]
            drows.extend(d)
        if a.stoi:
            from parakeet_amd.metrics import stoi_batch
            by_rate = {}
            for k, r in enumerate(rates):                            # one engine call per rate that occurs
                by_rate.setdefault(r, []).append(k)
            st = np.full((len(kept), 2), np.nan)
            for r, ks in by_rate.items():
                for c, ext in enumerate((False, True)):
                    st[ks, c] = stoi_batch([ys[k] for k in ks], [xs[k] for k in ks], r, extended=ext)
            extra = [e + f"\t{v[0]:.6f}\t{v[1]:.6f}" for e, v in zip(extra, st)]
            srows.extend(st)
        if a.loudness:
            from parakeet_amd.metrics import loudness_batch
            by_rate = {}
            for k, r in enumerate(rates):                            # one engine call per rate that occurs
                by_rate.setdefault(r, []).append(k)
            lu = np.full((len(kept), 2), np.nan)
            for r, ks in by_rate.items():
                try:
                    lu[ks, 0], lu[ks, 1] = loudness_batch([xs[k] for k in ks], r), loudness_batch([ys[k] for k in ks], r)
                except NotImplementedError:                          # a rate off the 100 ms sample grid: nan
                    pass
            with np.errstate(invalid="ignore"):
                lu = np.concatenate([lu, lu[:, :1] - lu[:, 1:]], axis=1)
            extra = [e + f"\t{v[0]:.3f}\t{v[1]:.3f}\t{v[2]:.3f}" for e, v in zip(extra, lu)]
            lrows.extend(lu)
        for u, x, (sc, mag), e, note in zip(kept, xs, per, extra, notes):
            print(f"{u}\t{len(x)}\t{sc:.6f}\t{mag:.6f}{e}{note}")
            rows.append((sc, mag))
    if rows:
        sc, mag = np.mean(rows, axis=0)
        print(f"spectral_convergence_loss\t{sc:.6f}\nlog_stft_magnitude_loss\t{mag:.6f}\tover {len(rows)} utterances")
    if drows:
        ml, adv, fake, real = np.mean(drows, axis=0)
        print(f"mean_logit\t{ml:.6f}\nadversarial_loss\t{adv:.6f}\nfake_loss\t{fake:.6f}\nreal_loss\t{real:.6f}")
    if srows:
        ok = [r for r in srows if not np.isnan(r[0])]
        if ok:
            st, est = np.mean(ok, axis=0)
            print(f"stoi\t{st:.6f}\nestoi\t{est:.6f}\tover {len(ok)} utterances")
        else:
            print("stoi\tnan\nestoi\tnan\tover 0 utterances")
    if lrows:
        ok = [r for r in lrows if np.isfinite(r).all()]
        if ok:
            g, r, d = np.mean(ok, axis=0)
            print(f"loudness_generated\t{g:.3f}\nloudness_recording\t{r:.3f}\nloudness_difference\t{d:.3f}\tover {len(ok)} utterances")
        else:
            print("loudness_generated\tnan\nloudness_recording\tnan\nloudness_difference\tnan\tover 0 utterances")


if __name__ == "__main__":
    main()
