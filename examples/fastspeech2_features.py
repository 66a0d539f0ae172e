#!/usr/bin/env python
"""FastSpeech2's three frame-level features of a directory of recordings on the MI355X engine -- the steps of
``process_sentence`` in the reference's examples/fastspeech2/preprocess.py (:40-119), and with statistics files those of its
normalize.py:

    wav (any rate) -> load_wav(sr=fs) -> [--cut-sil] -> log-mel -> durations fixed up to the mel length
                   -> Pitch.get_pitch(duration=) -> Energy.get_energy(duration=)

``--durations`` is MFA's ``durations.txt`` as ``get_phn_dur`` reads it, one line per utterance: ``utt|speaker|ph d ph d ...``
(d in frames of ``n_shift`` samples).  ``--config`` is the recipe's yaml: ``fs, n_fft, n_shift, win_length, window, n_mels,
fmin, fmax, f0min, f0max``.  Written under ``--output-dir``: ``data_speech/<utt>_speech.npy`` (L, n_mels),
``data_pitch/<utt>_pitch.npy`` and ``data_energy/<utt>_energy.npy`` (T, 1), and ``metadata.jsonl`` with the keys
examples/fastspeech2_gta.py reads (``utt_id, phones, durations, pitch, energy, feats``; ``text`` with ``--phones-dict``,
``spk_id`` with ``--speaker-dict``).  With ``--speech-stats / --pitch-stats / --energy-stats`` (the (2, dim) mean / scale
files of compute_statistics.py) the features are written normalised, as normalize.py leaves them.  ``--write-stats DIR``
saves ``speech_stats.npy``, ``pitch_stats.npy`` and ``energy_stats.npy`` of the raw (not normalised) features just extracted,
from the device tensors (parakeet_amd.normalizer.FeatureStats).

The pitch is this project's estimator (parakeet_amd.audio.Pitch), NOT pyworld's DIO + StoneMask, which the
reference calls; the wav loader's resampler is the project's own too (4.5d).  ``--pitch-tracker viterbi`` decides the lags by
Viterbi tracking over every frame's candidates instead of frame by frame (4.5e; checked on synthetic signals only).  All
utterances run as one ragged batch through each extractor.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_durations(path):
    """{utt: [phones, durations, speaker]} of a ``utt|speaker|ph d ph d ...`` file."""
    sentences = {}
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split("|")
            if len(parts) < 3:
                continue
            pd = parts[-1].split()
            assert len(pd) % 2 == 0, f"{parts[0]}: phones and durations do not pair up"
            sentences[parts[0]] = [pd[::2], [int(v) for v in pd[1::2]], parts[1]]
    return sentences


def fix_durations(durations, n_frames):
    """compare_duration_and_mel_length (preprocess_utils.py:163-187): the difference to the mel length goes to the last
    token, or to the first if the last would not stay positive; None if neither can take it."""
    d = list(durations)
    diff = n_frames - sum(d)
    if diff == 0:
        return d
    if diff > 0 or d[-1] + diff > 0:
        d[-1] += diff
    elif d[0] + diff > 0:
        d[0] += diff
    else:
        return None
    return d


def _id_map(path):
    if path is None:
        return None
    with open(path, "rt", encoding="utf-8") as f:
        return {k: int(v) for k, v in (line.split() for line in f if line.strip())}


def _zscore(x, stats):
    return ((x - stats[0]) / stats[1]).astype(np.float32)


def extract(args):
    """Returns the metadata records after writing the files."""
    from parakeet_amd import checkpoint
    from parakeet_amd.audio import Energy, LogMelFBank, Pitch, average_by_duration, load_wav
    cfg = checkpoint._config(args.config)
    fs, hop = int(cfg["fs"]), int(cfg["n_shift"])
    mel_extractor = LogMelFBank(sr=fs, n_fft=cfg["n_fft"], hop_length=hop, win_length=cfg.get("win_length"),
                                window=cfg.get("window", "hann"), n_mels=cfg["n_mels"], fmin=cfg.get("fmin"), fmax=cfg.get("fmax"))
    pitch_extractor = Pitch(sr=fs, hop_length=hop, f0min=cfg["f0min"], f0max=cfg["f0max"], tracker=args.pitch_tracker)
    energy_extractor = Energy(sr=fs, n_fft=cfg["n_fft"], hop_length=hop, win_length=cfg.get("win_length"),
                              window=cfg.get("window", "hann"))
    sentences = read_durations(args.durations)
    phone_ids, speaker_ids = _id_map(args.phones_dict), _id_map(args.speaker_dict)
    stats = [None if p is None else np.load(p) for p in (args.speech_stats, args.pitch_stats, args.energy_stats)]
    utts, wavs = [], []
    for name in sorted(os.listdir(args.input_dir)):
        utt = os.path.splitext(name)[0]
        if not name.lower().endswith(".wav") or utt not in sentences:
            continue
        wav, _ = load_wav(os.path.join(args.input_dir, name), sr=fs)
        if wav.ndim != 1 or np.abs(wav).max() > 1.0:
            continue
        phones, durations, _ = sentences[utt]
        if args.cut_sil:
            cum = np.concatenate([[0], np.cumsum(durations)])
            start, end = 0, int(cum[-1])
            if phones[0] == "sil" and len(durations) > 1:
                start, phones, durations = int(cum[1]), phones[1:], durations[1:]
            if phones[-1] == "sil" and len(durations) > 1:
                end, phones, durations = int(cum[-2]), phones[:-1], durations[:-1]
            wav = wav[start * hop:end * hop]
            sentences[utt][:2] = [phones, durations]
        if wav.size:
            utts.append(utt)
            wavs.append(wav)
    if not utts:
        raise SystemExit(f"no .wav file of {args.input_dir} has a line in {args.durations}")
    mels = mel_extractor.get_log_mel_fbank_batch(wavs)
    keep = []
    for i, utt in enumerate(utts):
        d = fix_durations(sentences[utt][1], mels[i].shape[0])
        if d is None:
            print(f"{utt}: the durations cannot be brought to {mels[i].shape[0]} frames, skipped")
            continue
        sentences[utt][1] = d
        keep.append(i)
    durs = [np.asarray(sentences[utts[i]][1], dtype=np.int64) for i in keep]
    pitch = pitch_extractor.get_pitch_batch([wavs[i] for i in keep], durs)
    energy = [average_by_duration(e, d).reshape(-1, 1)
              for e, d in zip(energy_extractor.get_energy_batch([wavs[i] for i in keep]), durs)]
    for sub in ("data_speech", "data_pitch", "data_energy"):
        os.makedirs(os.path.join(args.output_dir, sub), exist_ok=True)
    if args.write_stats is not None:
        from parakeet_amd.normalizer import FeatureStats
        os.makedirs(args.write_stats, exist_ok=True)
        for kind, xs in (("speech", [mels[i] for i in keep]), ("pitch", pitch), ("energy", energy)):
            if xs:
                FeatureStats(xs[0].shape[1]).fit(xs).save(os.path.join(args.write_stats, f"{kind}_stats.npy"))
    records = []
    for i, d, f0, en in zip(keep, durs, pitch, energy):
        utt = utts[i]
        phones, _, speaker = sentences[utt]
        feats = [mels[i].cpu().numpy(), f0.cpu().numpy(), en.cpu().numpy()]
        assert feats[0].shape[0] == int(d.sum()) and feats[1].shape == feats[2].shape == (len(phones), 1)
        feats = [x.astype(np.float32) if s is None else _zscore(x, s) for x, s in zip(feats, stats)]
        paths = [os.path.join(sub, f"{utt}_{kind}.npy") for sub, kind in
                 (("data_speech", "speech"), ("data_pitch", "pitch"), ("data_energy", "energy"))]
        for p, x in zip(paths, feats):
            np.save(os.path.join(args.output_dir, p), x, allow_pickle=False)
        rec = {"utt_id": utt, "phones": list(phones), "text_lengths": len(phones), "speech_lengths": int(d.sum()),
               "durations": [int(v) for v in d], "speech": paths[0], "feats": paths[0], "pitch": paths[1], "energy": paths[2],
               "speaker": speaker}
        if phone_ids is not None:
            rec["text"] = [phone_ids[p] for p in phones]
        if speaker_ids is not None:
            rec["spk_id"] = speaker_ids[speaker]
        records.append(rec)
    with open(os.path.join(args.output_dir, "metadata.jsonl"), "wt", encoding="utf-8") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    print(f"{len(records)} utterances, {sum(r['speech_lengths'] for r in records)} frames -> {args.output_dir}")
    return records


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="the recipe's yaml")
    ap.add_argument("--input-dir", required=True, help="directory of wav files")
    ap.add_argument("--durations", required=True, help="MFA durations.txt: utt|speaker|ph d ph d ...")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--cut-sil", action="store_true", help="drop a leading / trailing 'sil' token and its samples")
    ap.add_argument("--phones-dict", default=None, help="'phone id' lines: adds 'text' to the metadata")
    ap.add_argument("--speaker-dict", default=None, help="'speaker id' lines: adds 'spk_id' to the metadata")
    ap.add_argument("--pitch-tracker", choices=("frame", "viterbi"), default="frame",
                    help="how a frame's lag is decided: on its own, or by Viterbi tracking over the frames' candidates")
    ap.add_argument("--speech-stats", default=None)
    ap.add_argument("--pitch-stats", default=None)
    ap.add_argument("--energy-stats", default=None)
    ap.add_argument("--write-stats", default=None, metavar="DIR",
                    help="save speech_stats.npy, pitch_stats.npy and energy_stats.npy of the raw features here")
    return ap.parse_args(argv)


if __name__ == "__main__":
    extract(parse_args())
