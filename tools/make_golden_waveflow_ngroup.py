"""Golden vectors of ConditionalWaveFlow at n_group 32, 64 and 128 -- the models whose residual layers have height dilations
(Flow.dilations_dict, waveflow.py:420-426) -- from the reference's own source (see tools/make_golden.py):
tests/golden/waveflow_ngroup.npz.  Per n_group a 64-channel model of 2 flows (weights: syn.waveflow_state, seed 314), a
(1, 80, 3) mel, ``infer``'s waveform for a fixed z and ``forward``'s z and log-determinant for a 0.3 N(0, 1) recording of
3 * 256 - 37 samples."""
import os

import numpy as np

import ref_import

ref_import.setup()
import paddle  # noqa: E402  (stand-in or real, see ref_import)

from parakeet_amd import synthetic as syn  # noqa: E402

N_GROUPS = (32, 64, 128)
FRAMES = 3


def golden_waveflow_ngroup(out_dir):
    from make_golden_fs2_forward import save_npz_reproducible
    wfm = ref_import.load("parakeet.models.waveflow")
    arrays = dict(seed=np.array(314), n_groups=np.array(N_GROUPS))
    for g in N_GROUPS:
        cfg = dict(syn.WAVEFLOW_LJSPEECH, channels=64, n_flows=2, n_group=g)
        state = syn.waveflow_state(cfg, seed=314, weight_norm=True)
        model = wfm.ConditionalWaveFlow(**cfg)
        model.set_state_dict(state)
        model.eval()
        for layer in model.sublayers():   # utils/layer_tools.recursively_remove_weight_norm (layer_tools.py:40-46)
            try:
                paddle.nn.utils.remove_weight_norm(layer)
            except ValueError:
                pass
        rng = np.random.default_rng(1000 + g)
        mel = np.maximum(rng.normal(-4, 2, size=(1, 80, FRAMES)), np.log(1e-5)).astype(np.float32)
        t = FRAMES
        for f in cfg["upsample_factors"]:
            t = f * t - f
        z = rng.normal(size=(1, t)).astype(np.float32)
        audio = (0.3 * rng.normal(size=(1, FRAMES * 256 - 37))).astype(np.float32)
        with ref_import.fixed_randn(z), paddle.no_grad():
            wav = model.infer(paddle.to_tensor(mel)).numpy().astype(np.float32)
        with paddle.no_grad():
            fz, ldj = model(paddle.to_tensor(audio), paddle.to_tensor(mel))
        arrays[f"mel_{g}"] = mel
        arrays[f"z_{g}"] = z
        arrays[f"wav_{g}"] = wav
        arrays[f"audio_{g}"] = audio
        arrays[f"fz_{g}"] = fz.numpy().astype(np.float32)
        arrays[f"logdet_{g}"] = np.asarray(ldj.numpy(), dtype=np.float64).reshape(-1)[:1]
        print(f"waveflow n_group {g}: infer {wav.shape}, forward {arrays[f'fz_{g}'].shape}, logdet {float(arrays[f'logdet_{g}'][0]):.6f}")
    save_npz_reproducible(os.path.join(out_dir, "waveflow_ngroup.npz"), arrays)


if __name__ == "__main__":
    os.makedirs(ref_import.golden_dir(), exist_ok=True)
    golden_waveflow_ngroup(ref_import.golden_dir())
