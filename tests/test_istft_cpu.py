"""The fp64 restatement of istft / Griffin-Lim (tests/istft_ref.py) and its derived bound, checked on the host: against
torch.istft in float64, as a round trip, against a float32 evaluation and three wrong ones, and for convergence."""
import numpy as np
import pytest
import torch

import fp32_bounds as fb
import istft_ref as ir
import sweep_cases as sc


def _torch_istft(D, c, center=True):
    win = torch.from_numpy(ir.window64(c))
    y = torch.istft(torch.from_numpy(np.ascontiguousarray(np.asarray(D, np.complex128).T)), c.n_fft, hop_length=c.hop,
                    win_length=c.n_fft, window=win, center=center, normalized=False, onesided=True)
    return y.numpy()


@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_restatement_agrees_with_torch_istft(c):
    """center=True: sample for sample.  center=False: torch refuses the configuration (its NOLA check sees the zero of the
    periodic hann window at sample 0), so torch inverts the same spectra with center=True -- which is the same overlap-add
    minus n_fft/2 samples at both ends -- and the samples whose envelope exceeds 1e-3 of its maximum are compared."""
    for w in sc.mel_batch(c):
        D = ir.stft(w, c)
        if D.shape[0] == 0:
            continue
        got = ir.istft(D, c, with_bound=True)
        if c.center:
            want = _torch_istft(D, c)
            assert want.shape == got["wav"].shape == (ir.num_samples(c, D.shape[0]),)
            assert np.abs(got["wav"] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
        else:
            with pytest.raises(RuntimeError):
                _torch_istft(D, c, center=False)
            if D.shape[0] < 2:
                continue            # nothing is left of one frame after the trim
            want = _torch_istft(D, c)
            h = c.n_fft // 2
            mine, env = got["wav"][h:-h], got["env"][h:-h]
            assert want.shape == mine.shape
            sel = env > 1e-3 * got["env"].max()
            assert sel.sum() > 0.5 * sel.size
            assert np.abs(mine - want)[sel].max() <= 1e-12 * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("c", [c for c in sc.MEL_CFGS if c.center], ids=sc.mel_id)
def test_restatement_round_trip(c):
    for w in sc.mel_batch(c):
        D = ir.stft(w, c)
        y = ir.istft(D, c)
        assert y.shape == (c.hop * (D.shape[0] - 1),)
        assert np.abs(y - w[:y.size]).max() <= 1e-12


@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_bound_accepts_float32_and_rejects_mutants(c):
    B = ir.synthesis_basis(c)
    specs = ir.sweep_spectra(c)
    worst = 0.0
    for D in specs:
        ref = ir.istft(D, c, with_bound=True, basis=B)
        worst = max(worst, fb.ratio(ir.istft_f32(D, c), ref["wav"], ref["bound"]))
    print(f"SWEEP-RATIO istft_f32_numpy {sc.mel_id(c)} {worst:.4g}")
    assert worst <= 1.0
    D = max(specs, key=lambda d: d.shape[0])               # the long utterance
    ref = ir.istft(D, c, with_bound=True, basis=B)
    mutants = {"frame_dropped": ir.istft_f32(D, c, drop_frame=D.shape[0] // 2),
               "envelope_one_frame_short": ir.istft_f32(D, c, env_short=True),
               "interior_bins_without_factor_2": ir.istft_f32(D, c, interior=1.0)}
    for name, y in mutants.items():
        r = fb.ratio(y, ref["wav"], ref["bound"])
        print(f"SWEEP-MUTANT istft {sc.mel_id(c)} {name} {r:.4g}")
        assert r > 1.0, name


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_restatement_converges(c):
    S, a0 = ir.gl_problem(c)
    g = ir.griffin_lim(S, c, 32, 0.99, a0, keep=(0, 4, 32))
    s0, s4, s32 = (ir.spectral_convergence(g["waves"][i], S, c) for i in (0, 4, 32))
    print(f"GL-SC restatement {sc.mel_id(c)} {s0:.4f} {s4:.4f} {s32:.4f}")
    assert s32 < s4 < s0
    assert np.allclose(np.abs(g["angles"]), 1.0, atol=1e-12)
