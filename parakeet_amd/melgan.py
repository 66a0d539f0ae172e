"""MelGAN (Kumar et al. 2019) and multi-band MelGAN (Yang et al. 2020) generators with the pseudo-QMF bank, behind a
look-alike of the usual Python API.

``MelGANGenerator``, ``PQMF`` and ``MelGANInference`` mirror ``HiFiGANGenerator`` / ``HiFiGANInference`` of this package; all
arithmetic runs in libpk_synth.so (csrc/melgan.hip on the convolution kernel of csrc/pk_hfg_conv.h, csrc/pqmf.hip).  The
model is restated with the module layout of the ``MelGANGenerator`` that the reference's successor project ships, as
recalled: NEITHER THE PARAMETER NAMES NOR THIS LAYOUT COULD BE CHECKED AGAINST A RELEASED CHECKPOINT.  A checkpoint with other
names fails at finalize with the name it misses.

With ``ch_i = channels >> i``, ``a`` = LeakyReLU(negative_slope), S = stacks, R = ReflectionPad1d:
  x = Conv1D(in_channels -> channels, kernel_size)(R((kernel_size - 1) / 2)(mel))                     melgan.1
  per stage i (scale s_i), q_i = 2 + i (2 + S):
    x = Conv1DTranspose(ch_i -> ch_(i+1), 2 s_i, stride s_i, padding s_i // 2 + s_i % 2,
                        output_padding s_i % 2)(a(x))                                                 melgan.{q_i + 1}
    per stack j, d = stack_kernel_size ** j:
      t = Conv1D(k = stack_kernel_size, dilation d)(R((k - 1) / 2 d)(a(x)))                           melgan.{q_i+2+j}.stack.2
      x = Conv1D(1x1)(a(t)) + Conv1D(1x1)(x)                            ...stack.4   and   melgan.{q_i+2+j}.skip_layer
  y = Conv1D(ch_last -> out_channels, kernel_size)(R(...)(a(x)))                                      melgan.{2 + n (2 + S) + 2}
  y = tanh(y) with use_final_nonlinear_activation
Multi-band MelGAN is this generator with ``out_channels`` sub-bands at 1 / out_channels of the sample rate and a ``PQMF``
synthesis bank that merges them (``MelGANInference(normalizer, generator, pqmf)``).

Envelope (anything else raises NotImplementedError from the constructor, without a device): in_channels 1 ... 512,
out_channels 1 ... 16, kernel_size odd 3 ... 11, 1 ... 6 stages with scales 2 ... 16, every ch_i a multiple of 8 in
8 ... 512, stacks 1 ... 6, stack_kernel_size odd 3 ... 7 with (k - 1) / 2 * k ** (S - 1) <= 64, bias=True, LeakyReLU with
only ``negative_slope``, pad="ReflectionPad1d", use_causal_conv=False.  PQMF: subbands 2 ... 16, taps even 4 ... 254,
cutoff_ratio in (0, 0.5), beta 0 ... 700.

Reflection needs its pad smaller than the length it pads: ``min_frames`` (4 for the defaults) is the shortest utterance;
a shorter one raises ValueError, the reflection is never clamped.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap


def _unsupported(msg, who="MelGANGenerator"):
    raise NotImplementedError(who + ": " + msg)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class PQMF:
    """The pseudo-QMF bank (csrc/pk_pqmf.h): ``analysis`` (T,) -> (subbands, T // subbands), ``synthesis`` back."""

    def __init__(self, subbands=4, taps=62, cutoff_ratio=0.142, beta=9.0, device=None):
        if not (2 <= int(subbands) <= 16):
            _unsupported(f"subbands must be 2 ... 16 (got {subbands})", "PQMF")
        if taps % 2 or not (4 <= int(taps) <= 254):
            _unsupported(f"taps must be even, 4 ... 254 (got {taps})", "PQMF")
        if not (0.0 < float(cutoff_ratio) < 0.5):
            _unsupported(f"cutoff_ratio must lie in (0, 0.5) (got {cutoff_ratio})", "PQMF")
        if not (0.0 <= float(beta) <= 700.0):
            _unsupported(f"beta must be 0 ... 700, where I0(beta) still is a float64 (got {beta})", "PQMF")
        self.subbands, self.taps = int(subbands), int(taps)
        self.cutoff_ratio, self.beta = float(cutoff_ratio), float(beta)
        self._device = device
        self._ctx = self._h = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_pqmf_destroy(h)
            except Exception:
                pass

    def _engine(self):
        ctx = Context.get(self._device)
        if self._h is None:
            cfg = _capi.PqmfCfg(self.subbands, self.taps, self.cutoff_ratio, self.beta)
            h = C.c_void_p()
            _capi.check(ctx.lib.pk_pqmf_create(ctx.handle, C.byref(cfg), C.byref(h)))
            self._ctx, self._h = ctx, h
        return ctx

    def filters(self):
        """The engine's float32 (analysis, synthesis) filters, (subbands, taps + 1) numpy each."""
        ctx = self._engine()
        a = np.empty((self.subbands, self.taps + 1), np.float32)
        s = np.empty_like(a)
        _capi.check(ctx.lib.pk_pqmf_filters(self._h, _capi.fptr(a), _capi.fptr(s), a.size))
        return a, s

    def analysis_packed(self, wav, lens):
        """wav: packed (sum(lens),) -> per utterance a (subbands, lens[b] // subbands) block, packed in one device tensor."""
        ctx = self._engine()
        lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        wav = ctx.to_device(wav).reshape(-1)
        assert wav.shape[0] == int(lens.sum()), "wav samples must equal sum(lens)"
        out = ctx.empty((int((lens // self.subbands).sum()) * self.subbands,))
        _capi.check(ctx.lib.pk_pqmf_analysis(self._h, dptr(wav), _i32p(lens), len(lens), dptr(out), 0))
        return out

    def synthesis_packed(self, bands, band_lens):
        """bands: per utterance a (subbands, band_lens[b]) block, packed -> packed (sum(band_lens) * subbands,) wav."""
        ctx = self._engine()
        band_lens = np.ascontiguousarray(np.asarray(band_lens, dtype=np.int32))
        bands = ctx.to_device(bands).reshape(-1)
        assert bands.shape[0] == int(band_lens.sum()) * self.subbands, "bands must hold subbands * sum(band_lens) values"
        out = ctx.empty((int(band_lens.sum()) * self.subbands,))
        _capi.check(ctx.lib.pk_pqmf_synthesis(self._h, dptr(bands), _i32p(band_lens), len(band_lens), dptr(out), 0))
        return out

    def analysis(self, x):
        """(T,) or (N, 1, T) -> (subbands, T // subbands) or (N, subbands, T // subbands)."""
        ctx = self._engine()
        x = ctx.to_device(x)
        if x.dim() == 1:
            return wrap(self.analysis_packed(x, [x.shape[0]]).reshape(self.subbands, -1))
        assert x.dim() == 3 and x.shape[1] == 1, f"expected (N, 1, T), got {tuple(x.shape)}"
        N, _, T = x.shape
        return wrap(self.analysis_packed(x.contiguous().reshape(-1), [T] * N).reshape(N, self.subbands, -1))

    def synthesis(self, x):
        """(subbands, M) or (N, subbands, M) -> (M * subbands,) or (N, 1, M * subbands)."""
        ctx = self._engine()
        x = ctx.to_device(x)
        if x.dim() == 2:
            assert x.shape[0] == self.subbands
            return wrap(self.synthesis_packed(x.contiguous(), [x.shape[1]]))
        assert x.dim() == 3 and x.shape[1] == self.subbands, f"expected (N, {self.subbands}, M), got {tuple(x.shape)}"
        N, _, M = x.shape
        return wrap(self.synthesis_packed(x.contiguous(), [M] * N).reshape(N, 1, -1))


class MelGANGenerator:
    def __init__(self, in_channels=80, out_channels=1, kernel_size=7, channels=512, bias=True, upsample_scales=(8, 8, 2, 2),
                 stack_kernel_size=3, stacks=3, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, pad="ReflectionPad1d", pad_params={},
                 use_final_nonlinear_activation=True, use_weight_norm=True, use_causal_conv=False, device=None):
        scales = [int(s) for s in upsample_scales]
        if use_causal_conv:
            _unsupported("use_causal_conv=True is not implemented")
        if pad != "ReflectionPad1d" or pad_params:
            _unsupported(f"pad {pad!r} with {pad_params!r} is not implemented; the kernel reflects")
        if nonlinear_activation != "LeakyReLU":
            _unsupported(f"nonlinear_activation {nonlinear_activation!r} is not implemented; the kernel applies LeakyReLU")
        params = dict(nonlinear_activation_params or {})
        unknown = set(params) - {"negative_slope"}
        if unknown:
            _unsupported(f"LeakyReLU parameters {sorted(unknown)} are not implemented")
        if not bias:
            _unsupported("bias=False is not implemented")
        if not (1 <= in_channels <= 512):
            _unsupported(f"in_channels must be 1 ... 512 (got {in_channels})")
        if not (1 <= out_channels <= 16):
            _unsupported(f"out_channels must be 1 ... 16 (got {out_channels})")
        if kernel_size % 2 == 0 or not (3 <= kernel_size <= 11):
            _unsupported(f"kernel_size must be odd, 3 ... 11 (got {kernel_size})")
        if not (1 <= len(scales) <= 6):
            _unsupported(f"1 ... 6 upsample stages (got {len(scales)})")
        for s in scales:
            if not (2 <= s <= 16):
                _unsupported(f"upsample_scales must be 2 ... 16 (got {s})")
        if not (8 <= channels <= 512):
            _unsupported(f"channels must be 8 ... 512 (got {channels})")
        for i in range(len(scales) + 1):
            if (channels >> i) < 8 or (channels >> i) % 8:
                _unsupported(f"channels >> {i} = {channels >> i} must be a multiple of 8 in 8 ... 512")
        if not (1 <= stacks <= 6):
            _unsupported(f"stacks must be 1 ... 6 (got {stacks})")
        if stack_kernel_size % 2 == 0 or not (3 <= stack_kernel_size <= 7):
            _unsupported(f"stack_kernel_size must be odd, 3 ... 7 (got {stack_kernel_size})")
        if (stack_kernel_size - 1) // 2 * stack_kernel_size ** (stacks - 1) > 64:
            _unsupported("(stack_kernel_size - 1) / 2 * stack_kernel_size ** (stacks - 1) must be at most 64 "
                         f"(kernel {stack_kernel_size}, {stacks} stacks)")
        self.in_channels, self.out_channels, self.channels = int(in_channels), int(out_channels), int(channels)
        self.kernel_size, self.upsample_scales = int(kernel_size), scales
        self.stacks, self.stack_kernel_size = int(stacks), int(stack_kernel_size)
        self.use_final_nonlinear_activation = bool(use_final_nonlinear_activation)
        self.negative_slope = float(params.get("negative_slope", 0.01))   # nn.LeakyReLU's default
        if not np.isfinite(self.negative_slope):
            raise ValueError("MelGANGenerator: negative_slope is not finite")
        self.use_weight_norm = use_weight_norm
        self.hop = int(np.prod(scales))
        self.aux_channels = self.in_channels
        # the smallest frame count with every reflection pad below the length it pads (csrc/melgan.hip computes the same)
        need, mul = (self.kernel_size - 1) // 2 + 1, 1
        for s in scales:
            mul *= s
            need = max(need, -(-((self.stack_kernel_size - 1) // 2 * self.stack_kernel_size ** (self.stacks - 1) + 1) // mul))
        self.min_frames = max(need, -(-((self.kernel_size - 1) // 2 + 1) // mul))
        self.training = True
        self._device = device
        self._state = {}
        self._math = "f16x3"
        self._normalizer = None
        self._pqmf = None
        self._ctx = self._h = None
        self._finalized = self._norm_set = self._pqmf_set = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_mgan_destroy(h)
            except Exception:
                pass

    @property
    def upsample_factor(self):
        """Samples per frame of what ``infer_packed`` returns: prod(scales), times the sub-bands once a bank is attached."""
        return self.hop * (self._pqmf.subbands if self._pqmf is not None else 1)

    # -- nn.Layer look-alikes ------------------------------------------------
    def set_state_dict(self, state_dict):
        self._state.update({k: to_numpy_f32(v) for k, v in state_dict.items() if not k.startswith("pqmf.")})
        self._finalized = False

    def state_dict(self):
        return dict(self._state)

    def eval(self):
        self.training = False
        return self

    def remove_weight_norm(self):
        """Numerically neutral here: weight_g / weight_v pairs are folded at finalize."""
        return None

    def set_math(self, mode):
        """'f16x3' (default: 3-term split-fp16 MFMA on block-scaled operands) or 'f32' (fp32 MFMA)."""
        if mode not in ("f32", "f16x3"):
            raise NotImplementedError(f"MelGANGenerator.set_math({mode!r}): 'f32' and 'f16x3' are implemented")
        self._math = mode
        if self._h:
            self._apply_math()

    def set_normalizer(self, normalizer):
        """Register ZScore statistics; applied only by calls passing ``normalize=True`` (what MelGANInference does)."""
        self._norm_owner = None
        self._normalizer = normalizer
        self._norm_set = False

    def set_pqmf(self, pqmf):
        """Attach a synthesis bank (None: detach): calls then return the full-band waveform."""
        if pqmf is not None and pqmf.subbands != self.out_channels:
            raise ValueError(f"MelGANGenerator.set_pqmf: the bank has {pqmf.subbands} subbands, the generator "
                             f"{self.out_channels} output channels")
        self._pqmf = pqmf
        self._pqmf_set = False

    def _apply_math(self):
        m = {"f32": _capi.PK_PWG_MATH_F32, "f16x3": _capi.PK_PWG_MATH_F16X3}[self._math]
        _capi.check(self._ctx.lib.pk_mgan_set_math(self._h, m))

    def _cfg(self):
        cfg = _capi.MganCfg()
        cfg.in_channels, cfg.out_channels, cfg.channels = self.in_channels, self.out_channels, self.channels
        cfg.kernel_size, cfg.n_upsample = self.kernel_size, len(self.upsample_scales)
        for i, s in enumerate(self.upsample_scales):
            cfg.upsample_scales[i] = s
        cfg.stacks, cfg.stack_kernel_size, cfg.bias = self.stacks, self.stack_kernel_size, 1
        cfg.use_final_nonlinear_activation = int(self.use_final_nonlinear_activation)
        cfg.negative_slope = self.negative_slope
        return cfg

    def _engine(self):
        """The finalized handle on the current stream's context (created at the first call that computes)."""
        ctx = Context.get(self._device)
        if self._h is None:
            cfg = self._cfg()
            h = C.c_void_p()
            _capi.check(ctx.lib.pk_mgan_create(ctx.handle, C.byref(cfg), C.byref(h)))
            self._ctx, self._h = ctx, h
            assert int(ctx.lib.pk_mgan_min_frames(h)) == self.min_frames
            self._apply_math()
        if not self._finalized:
            set_params(ctx.lib.pk_mgan_set_param, self._h, self._state)
            _capi.check(ctx.lib.pk_mgan_finalize(self._h))
            self._finalized = True
        if not self._norm_set:
            if self._normalizer is None:
                _capi.check(ctx.lib.pk_mgan_set_normalizer(self._h, None, None, 0))
            else:
                mu = to_numpy_f32(self._normalizer.mu).reshape(-1)
                sigma = to_numpy_f32(self._normalizer.sigma).reshape(-1)
                _capi.check(ctx.lib.pk_mgan_set_normalizer(self._h, _capi.fptr(mu), _capi.fptr(sigma), mu.size))
            self._norm_set = True
        if not self._pqmf_set:
            if self._pqmf is None:
                _capi.check(ctx.lib.pk_mgan_set_pqmf(self._h, None))
            else:
                self._pqmf._engine()
                _capi.check(ctx.lib.pk_mgan_set_pqmf(self._h, self._pqmf._h))
            self._pqmf_set = True
        return ctx

    # -- synthesis -------------------------------------------------------------
    def _infer(self, ctx, mel, frames, normalize):
        frames = np.ascontiguousarray(np.asarray(frames, dtype=np.int32))
        if frames.size == 0:
            raise ValueError("no utterances given")
        if normalize and self._normalizer is None:
            raise ValueError("normalize=True without set_normalizer")
        assert mel.shape[0] == int(frames.sum()), "mel rows must equal sum(frames)"
        self._last_frames = [int(f) for f in frames]
        out = ctx.empty((int(frames.sum()) * self.hop * self.out_channels,))
        _capi.check(ctx.lib.pk_mgan_infer(self._h, dptr(mel), _i32p(frames), len(frames), dptr(out),
                                          _capi.PK_APPLY_NORMALIZER if normalize else 0))
        return out

    def _banded(self):
        """True when a call's result is (out_channels, T) blocks rather than a waveform."""
        return self.out_channels > 1 and self._pqmf is None

    def inference_batch(self, mels, normalize=False):
        """mels: list of (T'_b, in_channels) arrays.  Returns a list of (T'_b * upsample_factor, 1) device tensors -- without a
        bank and with out_channels > 1, of (T'_b * hop, out_channels) sub-band tensors; one engine call."""
        ctx = self._engine()
        frames = [int(m.shape[0]) for m in mels]
        mel = torch.cat([ctx.to_device(m).reshape(-1, self.in_channels) for m in mels], dim=0)
        out = self._infer(ctx, mel, frames, normalize)
        outs, o = [], 0
        for f in frames:
            n = f * self.hop * self.out_channels
            blk = out[o:o + n]
            outs.append(wrap(blk.reshape(self.out_channels, -1).T if self._banded() else blk.reshape(n, 1)))
            o += n
        return outs

    def infer_packed(self, mel, frames, noise=None, generator=None, normalize=False):
        """mel: packed (sum(frames), in_channels) DEVICE tensor (e.g. FastSpeech2.decode_packed()); returns the packed
        (sum(frames) * upsample_factor,) device waveform (without a bank and with out_channels > 1: the packed
        (out_channels, frames[b] * hop) blocks).  ``noise`` / ``generator`` exist so that the call site is the one of
        PWGGenerator: MelGAN takes no noise, anything but None raises."""
        if noise is not None or generator is not None:
            raise ValueError("MelGANGenerator takes no noise input")
        ctx = self._engine()
        mel = ctx.to_device(mel).reshape(-1, self.in_channels)
        return self._infer(ctx, mel, frames, normalize)

    def forward(self, c):
        """(N, in_channels, T') -> (N, out_channels, T' * hop); with a bank attached (N, 1, T' * hop * subbands)."""
        ctx = self._engine()
        c = ctx.to_device(c)
        if c.dim() != 3 or c.shape[1] != self.in_channels:
            raise AssertionError(f"expected (N, {self.in_channels}, T'), got {tuple(c.shape)}")
        N, _, T = c.shape
        mel = c.transpose(1, 2).contiguous().reshape(-1, self.in_channels)
        out = self._infer(ctx, mel, [T] * N, False)
        return wrap(out.reshape(N, self.out_channels if self._banded() else 1, -1))

    __call__ = forward

    def inference(self, c, normalize=False):
        """(T', in_channels) -> (T' * upsample_factor, 1) (sub-bands without a bank: (T' * hop, out_channels))."""
        return self.inference_batch([c], normalize=normalize)[0]

    def debug_stages(self, b=0):
        """Test tap: the output of every stage (after its last stack) of utterance b of the last call, a list of
        (channels >> (i + 1), T'_b * scales up to stage i) float32 numpy (``pk_mgan_debug_read``; runs the stack again)."""
        ctx = self._engine()
        res, n = [], self._last_frames[b]
        for i, s in enumerate(self.upsample_scales):
            n *= s
            out = np.empty((self.channels >> (i + 1), n), dtype=np.float32)
            _capi.check(ctx.lib.pk_mgan_debug_read(self._h, i, b, _capi.fptr(out), out.size))
            res.append(out)
        return res

    def debug_convs(self, b=0, with_output=False):
        """Test tap: what every launch before the output convolution wrote for utterance b of the last call, in launch order
        (``pk_mgan_debug_conv``): the input convolution; per stage the transposed convolution, then per stack t, the skip
        convolution and x'.  ``with_output``: the output convolution's (out_channels, T'_b * hop) last -- the sub-bands."""
        ctx = self._engine()
        shapes, n = [(self.channels, self._last_frames[b])], self._last_frames[b]
        for i, s in enumerate(self.upsample_scales):
            n *= s
            shapes += [(self.channels >> (i + 1), n)] * (1 + 3 * self.stacks)
        if with_output:
            shapes.append((self.out_channels, n))
        res = []
        for k, shape in enumerate(shapes):
            out = np.empty(shape, dtype=np.float32)
            _capi.check(ctx.lib.pk_mgan_debug_conv(self._h, k, b, _capi.fptr(out), out.size))
            res.append(out)
        return res


class MelGANInference:
    """normalizer(logmel) -> generator.inference (-> pqmf.synthesis), as HiFiGANInference."""

    def __init__(self, normalizer, generator, pqmf=None):
        self.normalizer = normalizer
        self.generator = generator
        self.pqmf = pqmf
        self.bind()

    @property
    def melgan_generator(self):
        return self.generator

    @property
    def pwg_generator(self):
        """The accessor code written for PWGInference picks the vocoder through."""
        return self.generator

    def bind(self):
        g = self.generator
        if getattr(g, "_norm_owner", None) is not self:
            g.set_normalizer(self.normalizer)
            g._norm_owner = self
        if g._pqmf is not self.pqmf:
            g.set_pqmf(self.pqmf)
        return g

    def infer_packed(self, mel, frames, noise=None, generator=None, normalize=True):
        return self.bind().infer_packed(mel, frames, noise=noise, generator=generator, normalize=normalize)

    def inference(self, logmel):
        return self.bind().inference(logmel, normalize=True)

    def inference_batch(self, logmels):
        return self.bind().inference_batch(logmels, normalize=True)

    def forward(self, logmel):
        return self.inference(logmel)

    __call__ = forward

    def set_math(self, mode):
        self.generator.set_math(mode)

    def remove_weight_norm(self):
        return self.generator.remove_weight_norm()

    def debug_stages(self, b=0):
        return self.generator.debug_stages(b)

    def debug_convs(self, b=0, with_output=False):
        return self.generator.debug_convs(b, with_output)

    def eval(self):
        return self
