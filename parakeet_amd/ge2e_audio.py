"""The GE2E front end: examples/ge2e/audio_processor.py of the reference.

``normalize_volume`` (:33-50), ``compute_partial_slices`` (:110-170) and ``SpeakerVerificationPreprocessor`` (:173-246)
with the same constructor.  ``melspectrogram`` is librosa.feature.melspectrogram's power mel (hann, center=True, reflect
padding, Slaney filters 0 .. sr / 2) computed by the engine's STFT / mel kernels (csrc/mel.hip); the mel and the
partial batches stay on the device.

Differences from the reference, both forced by what this package depends on:
  * silence trimming (``trim_long_silences``, :53-107) needs ``webrtcvad``; without it the reference skips the step with a
    warning (:23-27, :217-220), and so does this module by default (``vad=None``, one warning per process).  ``vad="energy"``
    runs the step on the engine (``audio.trim_long_silences``) after ``normalize_volume``, as the reference
    does at :217-220: everything after the voice detector is the reference's, but the detector is this project's energy
    detector, NOT webrtcvad -- its two thresholds are design choices nobody has compared with webrtcvad on speech, and an
    energy detector flags loud noise as voice.  ``vad=callable`` (``wav -> one flag per window``, e.g. a wrapper around
    webrtcvad where it is installed) supplies the flags instead, and then the whole step is the reference's;
  * other sampling rates are resampled with ``scipy.signal.resample_poly`` on the host (``resampler="scipy"``, the default)
    or with the engine's polyphase kernel (``resampler="engine"``, ``audio.Resample``); neither is librosa's resampler.
"""
import warnings
from fractions import Fraction

import numpy as np
import torch

from .audio import _Engine, _resampler, load_wav, mel_filterbank, trim_long_silences

_VAD_WARNED = False


def _warn_no_vad():
    global _VAD_WARNED
    if not _VAD_WARNED:
        warnings.warn("Silence trimming (webrtcvad) is not available: partials are taken from the untrimmed wav, "
                      "as the reference does without webrtcvad.")
        _VAD_WARNED = True


def normalize_volume(wav, target_dBFS, increase_only=False, decrease_only=False):
    if increase_only and decrease_only:
        raise ValueError("Both increase only and decrease only are set")
    dBFS_change = target_dBFS - 10 * np.log10(np.mean(wav ** 2))
    if dBFS_change < 0 and increase_only:
        return wav
    if dBFS_change > 0 and decrease_only:
        return wav
    gain = 10 ** (dBFS_change / 20)
    return wav * gain


def compute_partial_slices(n_samples, partial_utterance_n_frames, hop_length, min_pad_coverage=0.75, overlap=0.5):
    """(wav_slices, mel_slices): partials of ``partial_utterance_n_frames`` frames every
    round(frames * (1 - overlap)) frames; the last one is dropped when the wav covers less than ``min_pad_coverage``
    of it, unless it is the only one."""
    assert 0 <= overlap < 1
    assert 0 < min_pad_coverage <= 1
    n_frames = int(np.ceil((n_samples + 1) / hop_length))
    frame_step = max(1, int(np.round(partial_utterance_n_frames * (1 - overlap))))
    wav_slices, mel_slices = [], []
    steps = max(1, n_frames - partial_utterance_n_frames + frame_step + 1)
    for i in range(0, steps, frame_step):
        mel_slices.append(slice(i, i + partial_utterance_n_frames))
        wav_slices.append(slice(i * hop_length, (i + partial_utterance_n_frames) * hop_length))
    last = wav_slices[-1]
    coverage = (n_samples - last.start) / (last.stop - last.start)
    if coverage < min_pad_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


def read_wav(path):
    """(wav float32 in [-1, 1), sampling rate) of a 16-bit PCM WAV file, channels averaged: librosa.load(path, sr=None)
    for the files the recipes use (audio_processor.py:204), without librosa."""
    import wave
    with wave.open(str(path), "rb") as w:
        sr, ch, width = w.getframerate(), w.getnchannels(), w.getsampwidth()
        raw = w.readframes(w.getnframes())
    if width != 2:
        raise NotImplementedError(f"{path}: only 16-bit PCM WAV is read")
    return np.frombuffer(raw, dtype="<i2").astype(np.float32).reshape(-1, ch).mean(axis=1) / 32768.0, sr


def resample(wav, source_sr, target_sr):
    """Polyphase resampling (scipy.signal.resample_poly): NOT librosa.resample, results differ slightly."""
    import scipy.signal
    fr = Fraction(int(target_sr), int(source_sr))
    return scipy.signal.resample_poly(np.asarray(wav, dtype=np.float64), fr.numerator, fr.denominator).astype(np.float32)


class SpeakerVerificationPreprocessor:
    def __init__(self, sampling_rate, audio_norm_target_dBFS, vad_window_length, vad_moving_average_width,
                 vad_max_silence_length, mel_window_length, mel_window_step, n_mels, partial_n_frames,
                 min_pad_coverage=0.75, partial_overlap_ratio=0.5, device=None, resampler="scipy", vad=None):
        if resampler not in ("scipy", "engine"):
            raise ValueError(f"resampler must be 'scipy' or 'engine', got {resampler!r}")
        if not (vad is None or vad == "energy" or callable(vad)):
            raise ValueError(f"vad must be None, 'energy' or a callable wav -> voice flags, got {vad!r}")
        self.resampler = resampler
        self.vad = vad
        self.sampling_rate = sampling_rate
        self.audio_norm_target_dBFS = audio_norm_target_dBFS
        self.vad_window_length = vad_window_length
        self.vad_moving_average_width = vad_moving_average_width
        self.vad_max_silence_length = vad_max_silence_length
        self.n_fft = int(mel_window_length * sampling_rate / 1000)
        self.hop_length = int(mel_window_step * sampling_rate / 1000)
        self.n_mels = n_mels
        self.partial_n_frames = partial_n_frames
        self.min_pad_coverage = min_pad_coverage
        self.partial_overlap_ratio = partial_overlap_ratio
        self._device = device
        self._eng = None

    def _engine(self):
        if self._eng is None:
            basis = mel_filterbank(self.sampling_rate, self.n_fft, self.n_mels, 0.0, self.sampling_rate / 2.0)
            self._eng = _Engine(self.n_fft, self.hop_length, self.n_fft, "hann", True, True, basis, 0, self._device)
        return self._eng

    def preprocess_wav(self, fpath_or_wav, source_sr=None):
        if isinstance(fpath_or_wav, (str, bytes)) or hasattr(fpath_or_wav, "__fspath__"):
            wav, source_sr = load_wav(fpath_or_wav)
        else:
            wav = np.asarray(fpath_or_wav, dtype=np.float32)
        if source_sr is not None and source_sr != self.sampling_rate:
            if self.resampler == "engine":
                wav = _resampler(source_sr, self.sampling_rate, device=self._device)(wav).cpu().numpy()
            else:
                wav = resample(wav, source_sr, self.sampling_rate)
        wav = normalize_volume(wav, self.audio_norm_target_dBFS, increase_only=True)
        if self.vad is None:
            _warn_no_vad()
            return wav
        return self.trim_long_silences(wav)

    def trim_long_silences(self, wav):
        """The reference's step (:53-107) with this preprocessor's VAD parameters, on the engine -> float32 numpy.  The voice
        flags come from the energy detector (``vad="energy"``, NOT webrtcvad) or from the callable, which gets the wav cut to
        whole windows, as the reference hands it to its detector."""
        wav = np.asarray(wav, dtype=np.float32)
        flags = None
        if callable(self.vad):
            w = (self.vad_window_length * self.sampling_rate) // 1000
            flags = self.vad(wav[:len(wav) - len(wav) % w])
        return trim_long_silences(wav, self.vad_window_length, self.vad_moving_average_width, self.vad_max_silence_length,
                                  self.sampling_rate, voice_flags=flags, device=self._device).cpu().numpy()

    def melspectrogram(self, wav):
        """(frames, n_mels) float32 power mel on the device."""
        return self._engine().run([np.asarray(wav, dtype=np.float32)], 2)[0]

    def _padded(self, wav):
        wav_slices, mel_slices = compute_partial_slices(len(wav), self.partial_n_frames, self.hop_length,
                                                        self.min_pad_coverage, self.partial_overlap_ratio)
        need = wav_slices[-1].stop
        wav = np.asarray(wav, dtype=np.float32)
        if need >= len(wav):
            wav = np.pad(wav, (0, need - len(wav)), "constant")
        return wav, [s.start for s in mel_slices]

    def extract_mel_partials(self, wav):
        """(B, partial_n_frames, n_mels) on the device: the mel of the whole padded wav, sliced."""
        return self.extract_mel_partials_batch([wav])[0]

    def extract_mel_partials_batch(self, wavs):
        """A list of wavs -> a list of (B_u, partial_n_frames, n_mels) device tensors, the mels in one engine call."""
        padded = [self._padded(w) for w in wavs]
        mels = self._engine().run([p[0] for p in padded], 2)
        F = self.partial_n_frames
        out = []
        for mel, (_, starts) in zip(mels, padded):
            idx = (torch.tensor(starts, dtype=torch.long)[:, None] + torch.arange(F)[None, :]).to(mel.device)
            out.append(mel[idx.reshape(-1)].reshape(len(starts), F, self.n_mels))
        return out


def ge2e_preprocessor(overlap=0.5, device=None, resampler="scipy", vad=None):
    """The released configuration (examples/ge2e/config.py): 16 kHz, -30 dBFS, 25 ms / 10 ms windows, 40 mels,
    160-frame partials, min_pad_coverage 0.75.  examples/ge2e/inference.py passes ``partial_overlap_ratio =
    min_pad_coverage`` (:81): use overlap=0.75 to reproduce its corpus embeddings; the class default is 0.5."""
    return SpeakerVerificationPreprocessor(16000, -30, 30, 8, 6, 25, 10, 40, 160, min_pad_coverage=0.75,
                                           partial_overlap_ratio=overlap, device=device, resampler=resampler, vad=vad)
