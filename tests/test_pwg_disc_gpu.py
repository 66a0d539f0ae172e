"""The Parallel WaveGAN discriminator on the engine (csrc/pwg_disc.hip, parakeet_amd.parallel_wavegan.PWGDiscriminator) against
the fp64 restatement of tests/pwg_disc_ref.py under its derived bound and against the reference's own numbers
(tests/golden/pwg_disc.npz), in both maths and for both golden configurations: logits, the activation after every block, the
loss sums, batch invariance bit for bit, the output modes, host pointers, block scaling, the refusals, the evaluator's seven
numbers on a real generator, and one full-size utterance.  ``SWEEP-RATIO`` lines give error / bound.

Lengths: with ``tile, halo = pk_pwgd_tile_samples``: 1, 2, halo, halo + 1, 2 halo + 1 and k tile + {-halo - 1, -halo, -1, 0, 1,
halo, halo + 1} for k = 1, 2 -- every way an utterance's end can fall against a tile's edge and its receptive field.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import pwg_disc_ref as ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(n, m) for n in ("a", "b") for m in ref.MATHS]
I32P = C.POINTER(C.c_int32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "pwg_disc.npz")))


@functools.lru_cache(maxsize=None)
def _model(name):
    cfg = ref.golden_configs()[name][0]
    state = {k[len(name) + 1:]: v for k, v in _gold().items() if k.startswith(name + "/")}
    return cfg, state, ref.Model(cfg, state)


def _new_disc(name, math, state=None):
    from parakeet_amd.parallel_wavegan import PWGDiscriminator
    cfg, st, _ = _model(name)
    kw = {k: v for k, v in cfg.items() if k != "negative_slope"}
    d = PWGDiscriminator(nonlinear_activation_params={"negative_slope": cfg["negative_slope"]}, **kw)
    d.set_state_dict(st if state is None else state)
    d.set_math(math)
    return d.eval()


@functools.lru_cache(maxsize=None)
def _disc(name, math):
    return _new_disc(name, math)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The ragged batch of the module docstring and its restatement: (signals, [ref.forward of each], tile, halo)."""
    tile, halo = _disc(name, "f32").tile_samples()
    assert halo == _model(name)[2].halo and tile >= 32
    lens = [1, 2, halo, halo + 1, 2 * halo + 1]
    for k in (1, 2):
        lens += [k * tile + o for o in (-halo - 1, -halo, -1, 0, 1, halo, halo + 1)]
    lens = sorted({n for n in lens if n >= 1})
    rng = np.random.default_rng(4242)
    xs = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    return xs, [ref.forward(_model(name)[2], x) for x in xs], tile, halo


def _raw_run(d, xs, logits=True, sums=True, host=False):
    """pk_pwgd_run itself -> (packed logits or None, (B, 2) sums or None) as numpy"""
    from parakeet_amd import _capi
    ctx = d._engine()
    lens = np.array([len(x) for x in xs], np.int32)
    flat = np.ascontiguousarray(np.concatenate(xs), np.float32)
    if host:
        out = np.full(flat.size, np.nan, np.float32) if logits else None
        acc = np.full((len(xs), 2), np.nan) if sums else None
        _capi.check(ctx.lib.pk_pwgd_run(d._h, _capi.fptr(flat), lens.ctypes.data_as(I32P), len(xs),
                                        None if out is None else _capi.fptr(out),
                                        None if acc is None else acc.ctypes.data_as(C.c_void_p), _capi.PK_HOST_IO))
        return out, acc
    x = torch.from_numpy(flat).cuda()
    out = torch.full((flat.size,), float("nan"), device="cuda") if logits else None
    acc = torch.full((len(xs), 2), float("nan"), dtype=torch.float64, device="cuda") if sums else None
    _capi.check(ctx.lib.pk_pwgd_run(d._h, C.c_void_p(x.data_ptr()), lens.ctypes.data_as(I32P), len(xs),
                                    None if out is None else C.c_void_p(out.data_ptr()),
                                    None if acc is None else C.c_void_p(acc.data_ptr()), 0))
    torch.cuda.synchronize()
    return (None if out is None else _np(out)), (None if acc is None else _np(acc))


@pytest.mark.parametrize("name,math", CASES)
def test_logits_layers_and_sums_are_within_the_derived_bound(name, math):
    xs, refs, tile, _ = _batch(name)
    d = _disc(name, math)
    logits = [_np(p) for p in d.forward_batch(xs)]
    sums, counts = d.scores(xs)
    layers = d.debug_layers(xs)
    assert sums.shape == (len(xs), 2) and sums.dtype == np.float64 and list(counts) == [len(x) for x in xs]
    worst = [0.0] * (len(refs[0]["acts"]) + 2)
    for b, r in enumerate(refs):
        assert logits[b].shape == r["logits"].shape
        q = [fb.ratio(layers[b][i], r["acts"][i], r["b_acts"][math][i]) for i in range(len(r["acts"]))]
        q.append(fb.ratio(logits[b], r["logits"], r["b_logits"][math]))
        s, bs = ref.sums_with_bound(r["logits"], r["b_logits"][math], tile)
        q.append(fb.ratio(sums[b], s, bs))
        worst = [max(a, v) for a, v in zip(worst, q)]
        assert max(q) <= 1.0, f"utterance {b} ({len(xs[b])} samples): layers ..., logits, sums = {q}"
    print(f"SWEEP-RATIO pwg_disc {name} {math} layers " + " ".join(f"{v:.4f}" for v in worst[:-2]) +
          f" logits {worst[-2]:.4f} sums {worst[-1]:.4f}")


@pytest.mark.parametrize("name,math", CASES)
def test_an_utterance_has_the_same_bits_alone_and_in_any_batch(name, math):
    xs, _, _, _ = _batch(name)
    d = _disc(name, math)
    logits, sums = _raw_run(d, xs)
    off = np.cumsum([0] + [len(x) for x in xs])
    again, sums2 = _raw_run(d, xs[::-1])
    assert np.array_equal(sums2[::-1], sums)
    assert np.array_equal(again, np.concatenate([logits[off[b]:off[b + 1]] for b in range(len(xs) - 1, -1, -1)]))
    o = 0
    for b, x in enumerate(xs):
        p, s = _raw_run(d, [x])
        assert np.array_equal(p, logits[o:o + len(x)]) and np.array_equal(s[0], sums[b]), f"utterance {b}"
        o += len(x)
    assert np.isfinite(logits).all() and np.isfinite(sums).all()


@pytest.mark.parametrize("name,math", CASES)
def test_output_modes_and_host_pointers_give_the_same_bits(name, math):
    xs, _, _, _ = _batch(name)
    d = _disc(name, math)
    logits, sums = _raw_run(d, xs)
    none, only = _raw_run(d, xs, logits=False)
    assert none is None and np.array_equal(only, sums)
    p, none = _raw_run(d, xs, sums=False)
    assert none is None and np.array_equal(p, logits)
    hp, hs = _raw_run(d, xs, host=True)
    assert np.array_equal(hp, logits) and np.array_equal(hs, sums)
    _, hs = _raw_run(d, xs, logits=False, host=True)
    assert np.array_equal(hs, sums)


@pytest.mark.parametrize("name,math", CASES)
def test_engine_matches_the_golden(name, math):
    """The reference's own logits and MSE numbers.  Engine and golden are each within the bound b of the exact value (the
    golden's distance is asserted by tests/test_pwg_disc_cpu.py), so they are within 2 b of each other."""
    g, (_, _, model) = _gold(), _model(name)
    d = _disc(name, math)
    nums, bnum = {}, {}
    for tag in ("x", "y"):
        x, want = g[f"{name}_{tag}"], g[f"{name}_p{tag}"]
        got = _np(d(torch.from_numpy(x)))
        assert got.shape == want.shape == x.shape
        rs = [ref.forward(model, x[n, 0], maths=(math,), keep=False) for n in range(x.shape[0])]
        q = max(fb.ratio(got[n, 0], want[n, 0], 2.0 * r["b_logits"][math]) for n, r in enumerate(rs))
        s, n = d.scores([x[i, 0] for i in range(x.shape[0])])
        nums[tag] = s.sum(0) / n.sum()
        bnum[tag] = sum(ref.sums_with_bound(r["logits"], r["b_logits"][math])[1] for r in rs) / n.sum()
        print(f"SWEEP-RATIO pwg_disc {name} {math} golden logits {tag} {q:.4f}")
        assert q <= 1.0
    got = np.array([nums["x"][0], nums["y"][0], nums["x"][1]])
    bound = 2.0 * np.array([bnum["x"][0], bnum["y"][0], bnum["x"][1]]) + 2.0 * fb.U * np.abs(g[f"{name}_mse"])   # + its float32
    q = fb.ratio(got, g[f"{name}_mse"], bound)
    print(f"SWEEP-RATIO pwg_disc {name} {math} golden mse {q:.4f} adversarial={got[0]:.6f} real={got[1]:.6f} fake={got[2]:.6f}")
    assert q <= 1.0


@pytest.mark.parametrize("name,math", CASES)
@pytest.mark.parametrize("e", [20, -20])
def test_block_scaling_input_times_2_to_the_e(name, math, e):
    """x * 2^e with block 0's weights * 2^-e is the same function, exactly representable: the result stays within the bound
    of the unscaled evaluation (the scales are measured, nothing assumes the size of the input)."""
    xs, refs, _, _ = _batch(name)
    _, st, _ = _model(name)
    st = dict(st)
    st["conv_layers.0.weight_g"] = (st["conv_layers.0.weight_g"].astype(np.float64) * 2.0 ** -e).astype(np.float32)
    d = _new_disc(name, math, st)
    pick = [0, len(xs) // 2, len(xs) - 1]
    got = d.forward_batch([(xs[b].astype(np.float64) * 2.0 ** e).astype(np.float32) for b in pick])
    q = max(fb.ratio(_np(p), refs[b]["logits"], refs[b]["b_logits"][math]) for p, b in zip(got, pick))
    print(f"SWEEP-RATIO pwg_disc {name} {math} scaled 2^{e} logits {q:.4f}")
    assert q <= 1.0


def test_the_envelope_is_refused_with_status_codes():
    from parakeet_amd import _capi
    from parakeet_amd.parallel_wavegan import PWGDiscriminator
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    lib = ctx.lib

    def create(**kw):
        f = dict(in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1,
                 negative_slope=0.2, bias=1)
        f.update(kw)
        cfg = _capi.PwgdCfg(*[f[n] for n, _ in _capi.PwgdCfg._fields_])
        h = C.c_void_p()
        st = lib.pk_pwgd_create(ctx.handle, C.byref(cfg), C.byref(h))
        if h:
            lib.pk_pwgd_destroy(h)
        return st, lib.pk_last_error().decode()

    assert create()[0] == 0
    for kw, word in ((dict(in_channels=2), "in_channels"), (dict(out_channels=2), "out_channels"),
                     (dict(kernel_size=4), "kernel_size"), (dict(kernel_size=11), "kernel_size"),
                     (dict(layers=2), "layers"), (dict(layers=17), "layers"), (dict(conv_channels=24), "conv_channels"),
                     (dict(conv_channels=144), "conv_channels"), (dict(dilation_factor=0), "dilation_factor"),
                     (dict(dilation_factor=2), "112"),               # 1 + 2 + ... + 256 + 1 samples per side
                     (dict(layers=16, kernel_size=5), "112"),        # 2 * 107
                     (dict(conv_channels=128, kernel_size=5), "48")):
        st, msg = create(**kw)
        assert st == -3 and word in msg, (kw, st, msg)
    # the largest stacks that fit: 107 samples per side at 64 channels, the recipe's 38 at 128
    assert create(layers=16)[0] == 0 and create(conv_channels=128)[0] == 0
    with pytest.raises(NotImplementedError, match="112"):
        PWGDiscriminator(dilation_factor=2).tile_samples()

    d = _disc("b", "f32")
    d._engine()
    x = torch.zeros(8, device="cuda")
    out = torch.zeros(8, device="cuda")
    lens = np.array([8], np.int32)
    run = lambda wav, ln, B: lib.pk_pwgd_run(d._h, wav, ln, B, C.c_void_p(out.data_ptr()), None, 0)   # noqa: E731
    ptr = C.c_void_p(x.data_ptr())
    assert run(ptr, lens.ctypes.data_as(I32P), 1) == 0
    assert run(None, lens.ctypes.data_as(I32P), 1) == -1
    assert run(ptr, None, 1) == -1
    assert run(ptr, lens.ctypes.data_as(I32P), 0) == -1
    assert run(ptr, np.array([0], np.int32).ctypes.data_as(I32P), 1) == -1 and "empty" in lib.pk_last_error().decode()
    assert lib.pk_pwgd_set_math(d._h, _capi.PK_PWG_MATH_BF16X3) == -3 and lib.pk_pwgd_set_math(d._h, 7) == -1
    buf = np.zeros(16 * 8, np.float32)
    assert lib.pk_pwgd_debug_read(d._h, 0, 0, _capi.fptr(buf), buf.size) == -6          # no run under set_debug
    fresh = _new_disc("b", "f32", {})
    with pytest.raises(RuntimeError, match="never set"):
        fresh.scores([np.zeros(8, np.float32)])
    torch.cuda.synchronize()


def test_pwg_evaluate_on_a_real_generator_matches_the_restatement():
    """The seven numbers of PWGEvaluator.evaluate_core from a real (small) generator, the golden discriminator and the
    default STFT criterion, against the restatement fed the engine's own generated audio."""
    import stft_loss_cases as lc
    import stft_loss_ref as lr
    from parakeet_amd import synthetic as syn
    from parakeet_amd.losses import pwg_evaluate, pwg_evaluate_per_utterance
    from parakeet_amd.parallel_wavegan import PWGGenerator
    from parakeet_amd.stft_loss import MultiResolutionSTFTLoss
    cfg = syn.pwg_size_config("A")
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(syn.pwg_state(cfg, seed=101, weight_norm=True))
    gen.eval()
    frames, hop, ctxw, N = 5, 256, cfg["aux_context_window"], 2             # 1280 samples: above n_fft / 2 of every resolution
    rng = np.random.default_rng(77)
    mel = rng.standard_normal((N, cfg["aux_channels"], frames + 2 * ctxw)).astype(np.float32)
    noise = rng.standard_normal((N, 1, frames * hop)).astype(np.float32)
    wav = (0.3 * rng.standard_normal((N, 1, frames * hop))).astype(np.float32)
    d, crit, lam = _disc("a", "f16x3"), MultiResolutionSTFTLoss(), 4.0
    got = pwg_evaluate(gen, d, crit, wav, mel, noise, lam)
    fake = _np(gen(noise, mel))[:, 0]
    model = _model("a")[2]
    rf = [ref.forward(model, fake[n], maths=("f16x3",), keep=False) for n in range(N)]
    rr = [ref.forward(model, wav[n, 0], maths=("f16x3",), keep=False) for n in range(N)]
    sb = lambda rs: [sum(v) for v in zip(*[ref.sums_with_bound(r["logits"], r["b_logits"]["f16x3"]) for r in rs])]   # noqa: E731
    (sf, bf), (sr, br) = sb(rf), sb(rr)
    n = N * frames * hop
    parts = []
    for r in lc.RECIPE:
        per = [lr.sums_with_bound(x, y, r) for x, y in zip(fake, wav[:, 0])]
        parts.append(lr.loss_bounds(sum(p[0] for p in per), sum(p[1] for p in per), sum(p[2].X.size for p in per)))
    sc, mag = np.mean([p[0] for p in parts]), np.mean([p[1] for p in parts])
    f32 = lambda v: 2.0 * fb.U * abs(v)                                     # noqa: E731  the criterion returns float32 scalars
    b_sc, b_mag = np.mean([p[2] for p in parts]) + f32(sc), np.mean([p[3] for p in parts]) + f32(mag)
    want = ref.evaluate(np.concatenate([r["logits"] for r in rf]), np.concatenate([r["logits"] for r in rr]), sc, mag, lam)
    bound = {"eval/adversarial_loss": bf[0] / n, "eval/fake_loss": bf[1] / n, "eval/real_loss": br[0] / n,
             "eval/spectral_convergence_loss": b_sc, "eval/log_stft_magnitude_loss": b_mag}
    bound["eval/generator_loss"] = lam * bound["eval/adversarial_loss"] + b_sc + b_mag
    bound["eval/discriminator_loss"] = bound["eval/real_loss"] + bound["eval/fake_loss"]
    assert list(got) == list(want)
    for k in want:
        q = abs(got[k] - want[k]) / bound[k]
        print(f"SWEEP-RATIO pwg_disc evaluate {k} {q:.4f} value={got[k]:.6f}")
        assert q <= 1.0, k
    per = pwg_evaluate_per_utterance(d, crit, [fake[0], fake[1][:1100]], [wav[0, 0], wav[1, 0][:1100]], lam)
    assert all(v.shape == (2,) for v in per.values())
    alone = pwg_evaluate_per_utterance(d, crit, [fake[1][:1100]], [wav[1, 0][:1100]], lam)
    assert all(per[k][1] == alone[k][0] for k in per)


@pytest.mark.parametrize("math", ref.MATHS)
def test_one_full_size_utterance_sums_only(math):
    """163 840 samples (911 tiles) against the restatement's sums and their bound, which tools/make_golden_pwg_disc.py
    stored with the golden (pwg_disc_ref.forward_long over the seeded input; ten seconds of numpy, so not repeated here)."""
    g = _gold()
    d = _disc("a", math)
    got, n = d.scores([ref.full_size_input()])
    q = fb.ratio(got[0], g["a_full_sums"], g[f"a_full_bound_{math}"])
    print(f"SWEEP-RATIO pwg_disc a {math} full size sums {q:.4f}")
    assert n[0] == 163840 and q <= 1.0
