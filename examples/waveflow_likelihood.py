"""Score recordings under a WaveFlow vocoder: for every <utt_id>.npy mel in --mel-dir with a waveform <utt_id>.npy in --wav-dir
(float samples at the model's rate; the mel must cover the audio: len(wav) <= frames x hop) print the utterance id, the samples
scored and the mean log-likelihood in nats per sample (minus WaveFlowLoss of that utterance).

    python examples/waveflow_likelihood.py --config config.yaml --checkpoint step-2000000 --mel-dir mels --wav-dir wavs
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parakeet_amd.utils import layer_tools  # noqa: E402
from parakeet_amd.waveflow import ConditionalWaveFlow  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="yaml with model / data sections (examples/waveflow/config.py)")
    ap.add_argument("--checkpoint", required=True, help="checkpoint path without the .pdparams suffix")
    ap.add_argument("--mel-dir", required=True)
    ap.add_argument("--wav-dir", required=True)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=8, help="utterances per call")
    a = ap.parse_args()
    model = ConditionalWaveFlow.from_pretrained(a.config, a.checkpoint)
    layer_tools.recursively_remove_weight_norm(model)
    model.eval()
    ids = sorted(f[:-4] for f in os.listdir(a.mel_dir) if f.endswith(".npy") and os.path.exists(os.path.join(a.wav_dir, f)))
    for i in range(0, len(ids), a.batch):
        chunk = ids[i:i + a.batch]
        mels = [np.load(os.path.join(a.mel_dir, u + ".npy")).astype(np.float32) for u in chunk]
        wavs = [np.load(os.path.join(a.wav_dir, u + ".npy")).astype(np.float32).reshape(-1) for u in chunk]
        for u, w, ll in zip(chunk, wavs, model.log_likelihood(wavs, mels, sigma=a.sigma)):
            print(f"{u}\t{len(w) // model.n_group * model.n_group}\t{ll:.6f}")


if __name__ == "__main__":
    main()
