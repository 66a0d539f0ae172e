"""fp64 torch restatement of the GE2E speaker encoder and its front end (the oracle of the speaker-encoder tests).

Model: parakeet/models/lstm_speaker_encoder.py:40-53 -- a unidirectional multi-layer LSTM (gate order i, f, g, o),
h[-1] of the last layer, relu(h . W + b) with a Paddle Linear weight [in, out], F.normalize (x / max(||x||, 1e-12));
with reduce the mean over the partials normalised again.
Front end: examples/ge2e/audio_processor.py:223-246 -- librosa's power mel (hann, center, reflect, Slaney filters),
computed on the zero-padded wav once and sliced into partials.
"""
import numpy as np
import torch

from oracle import audio_ref


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def lstm_last_hidden(state, x, num_layers, initial_states=None, dtype=torch.float64, return_layers=False, rec_matmul=None):
    """x (B, T, C) -> h(T) of the last layer (B, H), evaluated in ``dtype`` (float64: the oracle; float32: its own
    rounding, for error bars).  return_layers: also the list of every layer's h sequence (B, T, H).  rec_matmul(h, whh):
    another evaluation of the recurrent product h @ whh.T (another summation order, for the same purpose)."""
    h_in = _t(x, dtype)
    B, T, _ = h_in.shape
    layers = []
    for layer in range(num_layers):
        wih, whh = _t(state[f"lstm.weight_ih_l{layer}"], dtype), _t(state[f"lstm.weight_hh_l{layer}"], dtype)
        b = _t(state[f"lstm.bias_ih_l{layer}"], dtype) + _t(state[f"lstm.bias_hh_l{layer}"], dtype)
        H = whh.shape[1]
        if initial_states is None:
            h = torch.zeros(B, H, dtype=dtype)
            c = torch.zeros(B, H, dtype=dtype)
        else:
            h, c = _t(initial_states[0][layer], dtype), _t(initial_states[1][layer], dtype)
        xg = h_in @ wih.T + b
        outs = []
        for t in range(T):
            g = xg[:, t] + (h @ whh.T if rec_matmul is None else rec_matmul(h, whh))
            i, f, gg, o = g.split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        h_in = torch.stack(outs, 1)
        layers.append(h_in)
    return (h, layers) if return_layers else h


def normalize(x, axis):
    return x / torch.clamp(torch.linalg.norm(x, dim=axis, keepdim=True), min=1e-12)


def embed_sequences(state, x, num_layers, initial_states=None, reduce=False, dtype=torch.float64, return_layers=False,
                    rec_matmul=None):
    h, layers = lstm_last_hidden(state, x, num_layers, initial_states, dtype, True, rec_matmul)
    e = normalize(torch.relu(h @ _t(state["linear.weight"], dtype) + _t(state["linear.bias"], dtype)), 1)
    if reduce:
        e = normalize(e.mean(0), 0)
    return (e, layers) if return_layers else e


def power_mel(wav, sr=16000, n_fft=400, hop=160, n_mels=40):
    """librosa.feature.melspectrogram(wav, sr, n_fft, hop, n_mels).T in fp64: (frames, n_mels)."""
    re, im = audio_ref.stft(_t(wav)[None], n_fft=n_fft, hop_length=hop, dtype=torch.float64)
    pw = (re ** 2 + im ** 2)[0]                                            # (n_bin, frames)
    basis = _t(audio_ref.mel_filterbank(sr, n_fft, n_mels, 0.0, sr / 2.0))
    return (basis @ pw).T


def mel_partials(wav, partial_starts, n_frames=160, **kw):
    mel = power_mel(wav, **kw)
    return torch.stack([mel[s:s + n_frames] for s in partial_starts])


def synthetic_clip(seconds, seed, sr=16000):
    """Seeded harmonics + noise with a slow amplitude envelope: power mels of speech-like magnitude."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    f0 = rng.uniform(90, 260)
    wav = np.zeros(n)
    for k in range(1, 12):
        wav += rng.uniform(0.2, 1.0) / k * np.sin(2 * np.pi * f0 * k * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t))
                                                  + rng.uniform(0, 2 * np.pi))
    env = 0.5 + 0.5 * np.abs(np.sin(2 * np.pi * rng.uniform(1.5, 4.0) * t))
    wav = 0.05 * wav * env + 0.005 * rng.standard_normal(n)
    return wav.astype(np.float32)
