"""The polyphase resampler (csrc/resample.hip) against the fp64 direct sum of its definition (tests/resample_ref.py).

Comparator: ``ratio(got, want, dot_bound(sum |x| |g|, K = T))`` of tests/fp32_bounds.py -- one rounding of the stored tap and an
fp32 FMA chain of T terms; a test asserts ratio <= 1 and prints it.  Where the arithmetic is exact (an impulse, equal
rates, the same utterance in another batch) the comparison is bit for bit.

First hardware run (MI355X), largest ratio per test: see DESIGN.md 4.5d.
"""
import importlib.util
import os
import pickle
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402
import resample_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HANDLES = {}


def _rs(L, M, res_type="kaiser_best"):
    """A Resample with up = L, down = M (L, M coprime: the rates M -> L)."""
    from parakeet_amd.audio import Resample
    if (L, M, res_type) not in _HANDLES:
        rs = Resample(M, L, res_type=res_type)
        assert (rs.up, rs.down) == (L, M)
        _HANDLES[(L, M, res_type)] = rs
    return _HANDLES[(L, M, res_type)]


def _bits(a):
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)      # + 0: -0.0 and 0.0 are one value


def _ratio(got, x, L, M, res_type, T, n_lo=0, n_hi=None):
    want, a = rr.resample_ref(x, L, M, res_type, n_lo, n_hi, with_abs=True)
    return fb.ratio(got, want, fb.dot_bound(a, K=T))


def _n_for(out_len, L, M):
    """Input lengths whose output length is out_len, or (when L > M leaves it out) the two next to it."""
    lo, hi = max(1, out_len * M // L), max(1, -(-out_len * M // L))
    return sorted({lo, hi})


# ---------------------------------------------------------------------------------------------------------- impulse
@pytest.mark.parametrize("L,M", [(147, 320), (441, 320), (2, 1), (1, 3)])
def test_impulse_returns_the_table_bit_for_bit(L, M):
    """x = 1.0 at m0, 0 elsewhere: y[n] is the fp32 table entry of phase (n M) mod L whose tap lands on m0 (products with 1.0 and
    sums of zeros are exact) -- phase and base indexing, with nothing to hide behind."""
    rs = _rs(L, M)
    T, H = rs.taps, rs.taps // 2
    N = 2 * T + 37
    xs, want = [], []
    for m0 in (0, 1, N // 2, N - 1):
        x = np.zeros(N, np.float32)
        x[m0] = 1.0
        xs.append(x)
        n = np.arange(rs.output_length(N), dtype=np.int64)
        k = m0 - (n * M // L - (H - 1))                    # tap k multiplies x[base - (H - 1) + k]
        ok = (k >= 0) & (k < T)
        want.append(np.where(ok, rs.table[(n * M) % L, np.clip(k, 0, T - 1)], np.float32(0.0)))
    got = [o.cpu().numpy() for o in rs.run_batch(xs)]
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.count_nonzero(w) > 0
        assert np.array_equal(_bits(g), _bits(w))


# ---------------------------------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("L,M", [(147, 320), (160, 441), (441, 320), (320, 441), (2, 1), (1, 2), (3, 1), (1, 12)])
def test_tile_edges_and_short_utterances(L, M, res_type):
    rs = _rs(L, M, res_type)
    tile = rs.tile_samples
    assert tile > 0 and tile % L == 0
    lens = [1, 2, 50, 127, 128, 129]
    for out_len in (tile - 1, tile, tile + 1, 3 * tile + 1):
        lens += _n_for(out_len, L, M)
    lens = list(dict.fromkeys(lens))
    outs = {rs.output_length(n) for n in lens}
    if L <= M:                                             # every output length is some input's
        assert {tile - 1, tile, tile + 1, 3 * tile + 1} <= outs
    else:                                                  # only every (L / M)-th: the tile itself and both neighbours of the others
        assert tile in outs and min(outs - {tile}, key=lambda v: abs(v - tile)) != tile and max(outs) >= 3 * tile + 1
    rng = np.random.default_rng(L * 4099 + M)
    xs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    got = rs.run_batch(xs)
    worst = 0.0
    for x, g in zip(xs, got):
        assert g.shape == (rr.out_len(x.size, L, M),)
        worst = max(worst, _ratio(g.cpu().numpy(), x, L, M, res_type, rs.taps))
    print(f"resample {L}/{M} {res_type}: tile {tile}, T {rs.taps}, {len(lens)} utterances, ratio {worst:.3f}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("L,M", [(147, 320), (441, 320)])
def test_ragged_batch_is_bit_equal_to_each_utterance_alone(L, M):
    """Six utterances of 1 ... 3 tiles + 1 outputs in shuffled order, every one between two guard utterances of 1e30 in the
    packed buffer: bit-equal to itself alone and at another position of another batch, and within the bound of the reference
    (a read across an utterance's end would show as 1e30)."""
    rs = _rs(L, M)
    tile = rs.tile_samples
    rng = np.random.default_rng(7)
    lens = [1, _n_for(tile, L, M)[0], _n_for(3 * tile + 1, L, M)[-1], 77, _n_for(tile + 1, L, M)[-1], _n_for(2 * tile - 5, L, M)[0]]
    assert rs.output_length(lens[2]) >= 3 * tile + 1
    order = rng.permutation(len(lens))
    xs = [rng.standard_normal(lens[i]).astype(np.float32) for i in order]
    guard = np.full(rs.taps + 3, 1e30, np.float32)
    batch = [guard]
    for x in xs:
        batch += [x, guard]
    out = [o.cpu().numpy() for o in rs.run_batch(batch)][1::2]
    other = [o.cpu().numpy() for o in rs.run_batch(xs[::-1])][::-1]
    worst = 0.0
    for x, a, b in zip(xs, out, other):
        alone = rs(x).cpu().numpy()
        assert np.array_equal(_bits(a), _bits(alone)) and np.array_equal(_bits(b), _bits(alone))
        worst = max(worst, _ratio(a, x, L, M, "kaiser_best", rs.taps))
    print(f"resample {L}/{M} ragged batch: ratio {worst:.3f}")
    assert worst <= 1.0


def test_equal_rates_return_the_input():
    import torch
    from parakeet_amd.audio import Resample, resample
    x = np.random.default_rng(2).standard_normal(1000).astype(np.float32)
    x[3] = -0.0
    rs = Resample(22050, 22050)
    assert (rs.up, rs.down) == (1, 1) and rs.output_length(1000) == 1000
    y = rs(x)
    assert isinstance(y, torch.Tensor) and np.array_equal(y.cpu().numpy().view(np.uint32), x.view(np.uint32))
    ys = rs.run_batch([x, x[:10]])
    assert [tuple(v.shape) for v in ys] == [(1000,), (10,)]
    assert np.array_equal(resample(x, 16000, 16000).view(np.uint32), x.view(np.uint32))


def test_c_abi_refusals():
    """PK_EINVAL for a NULL pointer, B <= 0 and an empty utterance; PK_EUNSUPPORTED, naming the limit, outside the envelope."""
    import ctypes as C
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    lib = ctx.lib
    tab = np.zeros(4 << 20, np.float32)
    h = C.c_void_p()
    for (up, down, taps), word in (((4097, 1, 2), "4096"), ((1, 4097, 2), "4096"), ((2, 1, 8193), "8192"), ((4096, 1, 1025), str(4 << 20))):
        cfg = _capi.ResampleCfg(up, down, taps)
        assert lib.pk_resample_create(ctx.handle, C.byref(cfg), _capi.fptr(tab), C.byref(h)) == -3
        assert word in lib.pk_last_error().decode() and not h.value
    cfg = _capi.ResampleCfg(2, 1, 4)
    assert lib.pk_resample_create(ctx.handle, C.byref(cfg), None, C.byref(h)) == -1
    assert lib.pk_resample_create(ctx.handle, None, _capi.fptr(tab), C.byref(h)) == -1
    rs = _rs(2, 1)
    x, out = ctx.to_device(np.ones(8, np.float32)), ctx.empty((16,))
    lens = (C.c_int32 * 2)(8, 0)
    n = C.c_int64()
    assert lib.pk_resample_out_len(rs.h, 8, C.byref(n)) == 0 and n.value == 16
    assert lib.pk_resample_out_len(rs.h, -1, C.byref(n)) == -1
    assert lib.pk_resample_run(rs.h, dptr(x), lens, 0, dptr(out), 0) == -1
    assert lib.pk_resample_run(rs.h, dptr(x), lens, 2, dptr(out), 0) == -1 and b"empty" in lib.pk_last_error()
    assert lib.pk_resample_run(rs.h, None, lens, 1, dptr(out), 0) == -1
    assert lib.pk_resample_run(rs.h, dptr(x), None, 1, dptr(out), 0) == -1
    assert lib.pk_resample_run(rs.h, dptr(x), lens, 1, None, 0) == -1
    # host pointers (PK_HOST_IO) give what device pointers give
    xh, oh = np.random.default_rng(1).standard_normal(300).astype(np.float32), np.empty(600, np.float32)
    one = (C.c_int32 * 1)(300)
    _capi.check(lib.pk_resample_run(rs.h, _capi.fptr(xh), one, 1, _capi.fptr(oh), _capi.PK_HOST_IO))
    assert np.array_equal(_bits(oh), _bits(rs(xh).cpu().numpy()))


# -------------------------------------------------------------------------------------------------- 64-bit indexing
def test_output_index_times_down_beyond_2_to_31():
    """44100 -> 16000 (L 160, M 441) with 13.7 M samples: n M passes 2^31 at n = 4 869 576 of 4 970 522 outputs.  Two windows
    of 1024 outputs against the reference: one straddling that output, and the last 1024."""
    L, M, N = 160, 441, 13_700_000
    rs = _rs(L, M)
    x = np.random.default_rng(11).standard_normal(N, dtype=np.float32)
    y = rs(x)
    n_out = rr.out_len(N, L, M)
    assert y.shape == (n_out,) and (n_out - 1) * M > 2 ** 31
    n_star = -(-2 ** 31 // M)
    for lo, hi in ((n_star - 512, n_star + 512), (n_out - 1024, n_out)):
        r = _ratio(y[lo:hi].cpu().numpy(), x, L, M, "kaiser_best", rs.taps, lo, hi)
        print(f"resample 160/441, outputs {lo} ... {hi - 1} of {n_out}: ratio {r:.3f}")
        assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------- surface
def _signal(n, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def test_numpy_resample_and_load_wav(tmp_path):
    from parakeet_amd.audio import AudioProcessor, load_wav, resample, write_wav
    x = _signal(6000, 3)
    y = resample(x, 48000, 22050)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (rr.out_len(6000, 147, 320),)
    T = _rs(147, 320).taps
    r = _ratio(y, x, 147, 320, "kaiser_best", T)
    yf = resample(x, 48000, 22050, res_type="kaiser_fast")
    rf = _ratio(yf, x, 147, 320, "kaiser_fast", _rs(147, 320, "kaiser_fast").taps)
    two = resample(np.stack([x, x[::-1]]), 48000, 22050)
    assert two.shape == (2, y.size) and np.array_equal(two[0], y)
    print(f"resample() 48000 -> 22050: ratio {r:.3f} (kaiser_best), {rf:.3f} (kaiser_fast)")
    assert r <= 1.0 and rf <= 1.0
    write_wav(tmp_path / "f48.wav", x, 48000, subtype="FLOAT")
    got, sr = load_wav(tmp_path / "f48.wav", sr=22050)
    assert sr == 22050 and np.array_equal(got, y)
    raw, sr = load_wav(tmp_path / "f48.wav")
    assert sr == 48000 and np.array_equal(raw, x)
    # a 16-bit 48 kHz stereo file through AudioProcessor.read_wav: the decoded samples, resampled
    st = np.stack([x, _signal(6000, 4)], 1)
    write_wav(tmp_path / "p48.wav", st, 48000)
    dec = (np.rint(st * 32767.0).astype(np.float32).mean(axis=1) / 32768.0).astype(np.float32)
    ap = AudioProcessor(22050, 1024, 1024, 256, normalize=False)
    wav = ap.read_wav(tmp_path / "p48.wav")
    assert np.array_equal(wav, load_wav(tmp_path / "p48.wav", sr=22050)[0]) and np.array_equal(wav, resample(dec, 48000, 22050))
    r16 = _ratio(wav, dec, 147, 320, "kaiser_best", T)
    print(f"AudioProcessor.read_wav of a 48 kHz file: ratio {r16:.3f}")
    assert r16 <= 1.0


def test_log_mel_of_a_signal_at_another_rate():
    import torch
    from parakeet_amd.audio import LogMelFBank, resample
    x = _signal(9000, 5)
    ex = LogMelFBank(sr=22050, n_fft=1024, hop_length=256, n_mels=80, fmin=0, fmax=8000)
    a = ex.get_log_mel_fbank(x, sr=48000)
    b = ex.get_log_mel_fbank(resample(x, 48000, 22050))
    assert a.shape == (1 + rr.out_len(9000, 147, 320) // 256, 80) and torch.equal(a, b)
    assert torch.equal(ex.get_log_mel_fbank(x, sr=22050), ex.get_log_mel_fbank(x))       # its own rate: nothing happens


def test_write_wav_at_another_rate(tmp_path):
    """write_wav(source_samplerate=) resamples, then encodes: the decoded file is within the encoding's step of the reference.
    PCM_16 stores rint(32767 v) and decodes / 32768: |decoded - v| <= (|v| + 0.5) / 32768, at most one 16-bit step for
    |v| <= 0.5 (asserted), plus the resampler's own bound."""
    from parakeet_amd.audio import load_wav, wav_bytes, write_wav
    x = _signal(5000, 6)
    for sr_out, (L, M) in ((44100, (441, 220)), (16000, (8, 11))):
        write_wav(tmp_path / "o.wav", x, sr_out, source_samplerate=22000)
        got, sr = load_wav(tmp_path / "o.wav")
        want, a = rr.resample_ref(x, L, M, "kaiser_best", with_abs=True)
        assert sr == sr_out and got.shape == want.shape and np.abs(want).max() <= 0.5
        bound = fb.dot_bound(a, K=_rs(L, M).taps) + (np.abs(want) + 0.5) / 32768.0
        r = fb.ratio(got, want, bound)
        print(f"write_wav 22000 -> {sr_out}: ratio {r:.3f}")
        assert r <= 1.0
        assert (tmp_path / "o.wav").read_bytes() == wav_bytes(x, sr_out, source_samplerate=22000)
    write_wav(tmp_path / "s.wav", x, 22000, source_samplerate=22000)
    assert (tmp_path / "s.wav").read_bytes() == wav_bytes(x, 22000)


# The largest difference between the 16 kHz signals of the two resamplers on the input below (N(0, 1) at 48 kHz, 48 000
# samples), measured once on an MI355X against the float64 scipy path.  The two apply different filters
# (scipy: a Kaiser(5.0) FIR of 20 max(up, down) + 1 taps with its cutoff AT the new Nyquist frequency; the engine: 0.9476 of it,
# 64 zero crossings), so the figure is a filter difference; the engine's fp32 rounding is orders below it.  A resampler
# that is a whole sample off differs by the signal itself (rms 0.58 here, several times that at the maximum).
GE2E_ENGINE_VS_SCIPY = 0.3071


def test_ge2e_preprocessor_with_the_engine_resampler():
    from parakeet_amd.ge2e_audio import ge2e_preprocessor
    x = np.random.default_rng(16).standard_normal(48000).astype(np.float32)
    a = ge2e_preprocessor(resampler="scipy").preprocess_wav(x, source_sr=48000)
    b = ge2e_preprocessor(resampler="engine").preprocess_wav(x, source_sr=48000)
    c = ge2e_preprocessor().preprocess_wav(x, source_sr=48000)
    assert np.array_equal(a, c)                              # the default is scipy
    assert a.shape == b.shape == (16000,)
    d = float(np.abs(a.astype(np.float64) - b).max())
    print(f"GE2E preprocessor, 48 kHz -> 16 kHz: max |engine - scipy| = {d:.6f}, rms of the signal {np.sqrt(np.mean(a * a)):.4f}")
    assert d <= 2.0 * GE2E_ENGINE_VS_SCIPY
    with pytest.raises(ValueError):
        ge2e_preprocessor(resampler="librosa")


# ---------------------------------------------------------------------------------------------------------- example
def test_example_synthesize_from_wav(tmp_path):
    """examples/synthesize_from_wav.py on files at 48 kHz, 44.1 kHz and the model's 24 kHz with a small seeded generator:
    gen_<name> of frames * hop samples each, equal bit for bit to PWGInference applied to the mels of the explicitly resampled
    signals."""
    import yaml
    from parakeet_amd import synthetic as syn
    from parakeet_amd.audio import LogMelFBank, load_wav, resample, wav_bytes, write_wav
    from parakeet_amd.normalizer import ZScore
    from parakeet_amd.parallel_wavegan import PWGGenerator, PWGInference
    gen_cfg = dict(syn.PWG_LJSPEECH, layers=4, stacks=2, upsample_scales=[4, 5, 3, 5])
    cfg = dict(fs=24000, n_fft=2048, n_shift=300, win_length=1200, window="hann", n_mels=80, fmin=80, fmax=7600,
               generator_params=gen_cfg)
    (tmp_path / "pwg.yaml").write_text(yaml.safe_dump(cfg))
    state = syn.pwg_state(gen_cfg, seed=12, weight_norm=True)
    with open(tmp_path / "pwg.pdz", "wb") as f:
        pickle.dump({"generator_params": dict(state)}, f, protocol=4)
    mu, sd = syn.mel_stats(seed=6)
    np.save(tmp_path / "stats.npy", np.stack([mu, sd]))
    (tmp_path / "in").mkdir()
    sigs = {"a48.wav": (48000, _signal(9000, 21)), "b44.wav": (44100, _signal(7000, 22)), "c24.wav": (24000, _signal(5000, 23))}
    for name, (sr, x) in sigs.items():
        write_wav(tmp_path / "in" / name, x, sr, subtype="FLOAT")
    (tmp_path / "in" / "notes.txt").write_text("not audio")
    spec = importlib.util.spec_from_file_location("synthesize_from_wav", os.path.join(ROOT, "examples", "synthesize_from_wav.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.evaluate(types.SimpleNamespace(config=str(tmp_path / "pwg.yaml"), checkpoint=str(tmp_path / "pwg.pdz"),
                                             stat=str(tmp_path / "stats.npy"), input_dir=str(tmp_path / "in"),
                                             output_dir=str(tmp_path / "out"), output_sr=None, seed=5))
    assert sorted(os.listdir(tmp_path / "out")) == ["gen_a48.wav", "gen_b44.wav", "gen_c24.wav"]
    # the same thing step by step
    voc = PWGGenerator(**gen_cfg)
    voc.set_state_dict(state)
    voc.remove_weight_norm()
    voc.eval()
    inf = PWGInference(ZScore(mu, sd), voc)
    ex = LogMelFBank(sr=24000, n_fft=2048, hop_length=300, win_length=1200, window="hann", n_mels=80, fmin=80, fmax=7600)
    names = sorted(sigs)
    at24 = [resample(sigs[n][1], sigs[n][0], 24000) for n in names]
    assert np.array_equal(at24[2], sigs["c24.wav"][1])
    mels = [ex.get_log_mel_fbank(w) for w in at24]
    gen = inf.bind()
    gen.set_seed(5)
    want = [o.cpu().numpy()[:, 0] for o in gen.inference_batch(mels, normalize=True)]
    for n, w24, mel, w in zip(names, at24, mels, want):
        assert mel.shape[0] == 1 + w24.size // 300 and res[n].shape == (mel.shape[0] * 300,)
        assert np.array_equal(res[n].view(np.uint32), w.view(np.uint32))
        data, sr = load_wav(tmp_path / "out" / ("gen_" + n))
        assert sr == 24000 and data.size == mel.shape[0] * 300
        assert (tmp_path / "out" / ("gen_" + n)).read_bytes() == wav_bytes(w, 24000)
