"""Golden vectors of ConditionalWaveFlow.forward and WaveFlowLoss from the reference's own source (see tools/make_golden.py):
tests/golden/waveflow_forward_c64.npz -- mel, two recordings (1000 and 523 samples, run one utterance at a time: the reference's
forward has no ragged batch), their z, log-determinants and the loss at sigma 1.0 and 0.7."""
import os

import numpy as np

import ref_import

ref_import.setup()
import paddle  # noqa: E402  (stand-in or real, see ref_import)

from parakeet_amd import synthetic as syn  # noqa: E402

LENGTHS = (1000, 523)


def golden_waveflow_forward(out_dir):
    from make_golden_fs2_forward import save_npz_reproducible
    wfm = ref_import.load("parakeet.models.waveflow")
    cfg = dict(syn.WAVEFLOW_LJSPEECH, channels=64)
    state = syn.waveflow_state(cfg, seed=314, weight_norm=True)
    model = wfm.ConditionalWaveFlow(**cfg)
    model.set_state_dict(state)
    model.eval()
    for layer in model.sublayers():   # utils/layer_tools.recursively_remove_weight_norm (layer_tools.py:40-46)
        try:
            paddle.nn.utils.remove_weight_norm(layer)
        except ValueError:
            pass
    rng = np.random.default_rng(21)
    mel = np.maximum(rng.normal(-4, 2, size=(2, 80, 4)), np.log(1e-5)).astype(np.float32)
    arrays = dict(seed=np.array(314), mel=mel, sigmas=np.array([1.0, 0.7]))
    for b, n in enumerate(LENGTHS):
        audio = (0.3 * rng.normal(size=(1, n))).astype(np.float32)
        with paddle.no_grad():
            z, ldj = model(paddle.to_tensor(audio), paddle.to_tensor(mel[b:b + 1]))
            losses = [float(np.asarray(wfm.WaveFlowLoss(sigma=s)(z, ldj).numpy()).reshape(-1)[0]) for s in (1.0, 0.7)]
        arrays[f"audio{b}"] = audio[0]
        arrays[f"z{b}"] = z.numpy().astype(np.float32)[0]
        arrays[f"logdet{b}"] = np.asarray(ldj.numpy(), dtype=np.float64).reshape(-1)[:1]
        arrays[f"loss{b}"] = np.array(losses, dtype=np.float64)
        print("waveflow forward:", n, "->", arrays[f"z{b}"].shape, float(arrays[f"logdet{b}"][0]), losses)
    save_npz_reproducible(os.path.join(out_dir, "waveflow_forward_c64.npz"), arrays)


if __name__ == "__main__":
    os.makedirs(ref_import.golden_dir(), exist_ok=True)
    golden_waveflow_forward(ref_import.golden_dir())
