#!/usr/bin/env python
"""Voice cloning on the MI355X engine -- examples/tacotron2_aishell3/voice_cloning.ipynb of the reference as a script:
reference wav -> GE2E embedding (256) -> Tacotron2(d_global_condition=256, the notebook's aishell3 kwargs) -> WaveFlow
(128 channels) -> WAV at 22.05 kHz.

The notebook's text front end (chinese_g2p.convert_sentence: pypinyin / jieba) is not available, so ``--text`` holds
one ``utt_id | PHONE_IDS | TONE_IDS`` line per sentence (space-separated ids of aishell3's voc_phones / voc_tones).
The speaker embedding uses the notebook's preprocessor (partial overlap 0.5); ``--vad energy`` trims the reference wav's long
silences first (the engine's energy detector, NOT webrtcvad; off by default).  All sentences are decoded as one
ragged batch conditioned on the same voice.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parakeet_amd import checkpoint  # noqa: E402
from parakeet_amd.audio import write_wav  # noqa: E402
from parakeet_amd.ge2e_audio import ge2e_preprocessor  # noqa: E402
from parakeet_amd.tacotron2 import Tacotron2  # noqa: E402
from parakeet_amd.waveflow import ConditionalWaveFlow  # noqa: E402

AISHELL3_TACOTRON2 = dict(  # the notebook's synthesizer
    vocab_size=68, n_tones=10, d_mels=80, d_encoder=512, encoder_conv_layers=3, encoder_kernel_size=5, d_prenet=256,
    d_attention_rnn=1024, d_decoder_rnn=1024, attention_filters=32, attention_kernel_size=31, d_attention=128,
    d_postnet=512, postnet_kernel_size=5, postnet_conv_layers=5, reduction_factor=1, p_encoder_dropout=0.5,
    p_prenet_dropout=0.5, p_attention_dropout=0.1, p_decoder_dropout=0.1, p_postnet_dropout=0.5, d_global_condition=256,
    use_stop_token=False)
WAVEFLOW = dict(upsample_factors=[16, 16], n_flows=8, n_layers=8, n_group=16, channels=128, n_mels=80, kernel_size=[3, 3])


def read_text(path):
    items = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            utt, ph, tn = (p.strip() for p in line.split("|"))
            items.append((utt, np.array(ph.split(), np.int64), np.array(tn.split(), np.int64)))
    return items


def main():
    ap = argparse.ArgumentParser(description="GE2E voice cloning with Tacotron2-aishell3 and WaveFlow.")
    ap.add_argument("--ref_audio", required=True, help="reference speaker, 16-bit PCM WAV")
    ap.add_argument("--ge2e_checkpoint", required=True, help="GE2E step-N (with or without .pdparams)")
    ap.add_argument("--tacotron2_checkpoint", required=True, help="Tacotron2-aishell3 step-N.pdparams")
    ap.add_argument("--waveflow_checkpoint", required=True, help="WaveFlow step-N.pdparams")
    ap.add_argument("--text", required=True, help="lines 'utt_id | phone ids | tone ids'")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--max_decoder_steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0, help="decoder-prenet dropout stream")
    ap.add_argument("--vad", choices=["none", "energy"], default="none",
                    help="trim the reference wav's long silences: 'energy' is the engine's energy detector, not webrtcvad")
    args = ap.parse_args()

    p = ge2e_preprocessor(overlap=0.5, vad=None if args.vad == "none" else args.vad)
    encoder = checkpoint.load_ge2e(args.ge2e_checkpoint)
    embed = encoder.embed_utterance(p.extract_mel_partials(p.preprocess_wav(args.ref_audio)))

    synthesizer = Tacotron2(**AISHELL3_TACOTRON2)
    path = args.tacotron2_checkpoint
    synthesizer.set_state_dict(checkpoint.load_params(path if path.endswith(".pdparams") else path + ".pdparams"))
    synthesizer.eval()
    vocoder = ConditionalWaveFlow(**WAVEFLOW)
    path = args.waveflow_checkpoint
    vocoder.set_state_dict(checkpoint.load_params(path if path.endswith(".pdparams") else path + ".pdparams"))
    vocoder.eval()

    items = read_text(args.text)
    cond = embed.reshape(1, -1).repeat(len(items), 1)
    outs = synthesizer.infer_batch([ph for _, ph, _ in items], args.max_decoder_steps, tones=[tn for _, _, tn in items],
                                   seeds=[args.seed] * len(items), global_condition=cond)
    wavs = vocoder.infer_batch([o["mel_outputs_postnet"].T.contiguous() for o in outs])
    os.makedirs(args.output_dir, exist_ok=True)
    for (utt, _, _), wav in zip(items, wavs):
        write_wav(os.path.join(args.output_dir, utt + ".wav"), wav.cpu().numpy(), 22050)
        print(utt, wav.shape[0], "samples")


if __name__ == "__main__":
    main()
