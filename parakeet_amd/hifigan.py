"""HiFi-GAN generator (Kong et al. 2020) behind a look-alike of the usual Python API.

``HiFiGANGenerator`` and ``HiFiGANInference`` mirror ``PWGGenerator`` / ``PWGInference`` of this package; all arithmetic runs
in libpk_synth.so (csrc/hifigan.hip).  The model is restated from the paper with the module layout of the
``HiFiGANGenerator`` that the reference's successor project ships, as recalled: NEITHER THE PARAMETER NAMES (``input_conv``,
``upsamples.{i}.1``, ``blocks.{i * nb + j}.convs1.{n}.1``, ``convs2.{n}.1``, ``output_conv.1``) NOR THE SLOPE 0.01 OF THE
ACTIVATION BEFORE ``output_conv`` COULD BE CHECKED AGAINST A REAL CHECKPOINT.  A checkpoint with other names fails at
finalize with the name it misses; one with another output slope would need ``HFG_OUTPUT_SLOPE`` of csrc/pk_hifigan.h changed.

With ``ch_i = channels >> i`` and ``a_s`` = LeakyReLU(s):
  x = Conv1D(in_channels -> channels, kernel_size)(mel)                                    input_conv (no activation before it)
  per stage i: x = Conv1DTranspose(ch_i -> ch_{i+1}, 2 s_i, stride s_i, padding s_i // 2 + s_i % 2,
                                   output_padding s_i % 2)(a_slope(x))                     length L -> exactly L * s_i
               per residual block j, y = x, for every dilation d: t = Conv1D(k_j, dilation d)(a_slope(y));
                   with use_additional_convs t = Conv1D(k_j)(a_slope(t)); y = t + y
               x = (sum_j y_j) / nb
  wav = tanh(Conv1D(ch_last -> 1, kernel_size)(a_0.01(x)))
Every convolution zero-pads its own input at the two ends of the utterance.

Envelope (anything else raises NotImplementedError from the constructor, without a device): in_channels 1 ... 512,
out_channels 1, kernel_size odd 3 ... 11, 1 ... 6 stages with scales 2 ... 16 and ``upsample_kernel_sizes[i] == 2 *
upsample_scales[i]``, hop 4 ... 1024, every ch_i a multiple of 8 in 8 ... 512, 1 ... 4 residual blocks with odd kernels
3 ... 11 and 1 ... 4 dilations each with (k - 1) / 2 * d <= 64, bias=True, LeakyReLU with only ``negative_slope``,
global_channels -1.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap

OUTPUT_SLOPE = 0.01   # nn.LeakyReLU() before output_conv is built without arguments (csrc/pk_hifigan.h HFG_OUTPUT_SLOPE)


def _unsupported(msg):
    raise NotImplementedError("HiFiGANGenerator: " + msg)


class HiFiGANGenerator:
    def __init__(self, in_channels=80, out_channels=1, channels=512, global_channels=-1, kernel_size=7,
                 upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)), use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_weight_norm=True, device=None):
        scales = [int(s) for s in upsample_scales]
        uks = [int(k) for k in upsample_kernel_sizes]
        rks = [int(k) for k in resblock_kernel_sizes]
        dils = [[int(d) for d in ds] for ds in resblock_dilations]
        if global_channels not in (-1, None):
            _unsupported(f"global_channels={global_channels} (speaker conditioning) is not implemented")
        if nonlinear_activation != "LeakyReLU":
            _unsupported(f"nonlinear_activation {nonlinear_activation!r} is not implemented; the kernel applies LeakyReLU")
        params = dict(nonlinear_activation_params or {})
        unknown = set(params) - {"negative_slope"}
        if unknown:
            _unsupported(f"LeakyReLU parameters {sorted(unknown)} are not implemented")
        if not bias:
            _unsupported("bias=False is not implemented")
        if not (1 <= in_channels <= 512) or out_channels != 1:
            _unsupported(f"in_channels must be 1 ... 512 and out_channels 1 (got {in_channels}, {out_channels})")
        if kernel_size % 2 == 0 or not (3 <= kernel_size <= 11):
            _unsupported(f"kernel_size must be odd, 3 ... 11 (got {kernel_size})")
        if not (1 <= len(scales) <= 6) or len(uks) != len(scales):
            _unsupported("1 ... 6 upsample stages, one kernel size per scale")
        for s, k in zip(scales, uks):
            if not (2 <= s <= 16):
                _unsupported(f"upsample_scales must be 2 ... 16 (got {s})")
            if k != 2 * s:
                _unsupported(f"upsample_kernel_sizes must be twice the scales (got {k} for {s}): only then is a stage's "
                             "length exactly scale times its input's")
        hop = int(np.prod(scales))
        if not (4 <= hop <= 1024):
            _unsupported(f"the hop (product of the scales) must be 4 ... 1024 (got {hop})")
        if not (8 <= channels <= 512) or channels % (1 << len(scales)):
            _unsupported(f"channels must be 8 ... 512 and halve exactly at every stage (got {channels})")
        for i in range(len(scales) + 1):
            if (channels >> i) < 8 or (channels >> i) % 8:
                _unsupported(f"channels >> {i} = {channels >> i} must be a multiple of 8 in 8 ... 512")
        if not (1 <= len(rks) <= 4) or len(dils) != len(rks):
            _unsupported("1 ... 4 residual blocks per stage, one dilation list per kernel size")
        for k, ds in zip(rks, dils):
            if k % 2 == 0 or not (3 <= k <= 11):
                _unsupported(f"resblock_kernel_sizes must be odd, 3 ... 11 (got {k})")
            if not (1 <= len(ds) <= 4):
                _unsupported(f"1 ... 4 dilations per residual block (got {len(ds)})")
            for d in ds:
                if d < 1 or (k - 1) // 2 * d > 64:
                    _unsupported(f"(kernel - 1) / 2 * dilation must be 1 ... 64 (kernel {k}, dilation {d})")
        self.in_channels, self.out_channels, self.channels = int(in_channels), int(out_channels), int(channels)
        self.kernel_size = int(kernel_size)
        self.upsample_scales, self.upsample_kernel_sizes = scales, uks
        self.resblock_kernel_sizes, self.resblock_dilations = rks, dils
        self.use_additional_convs = bool(use_additional_convs)
        self.negative_slope = float(params.get("negative_slope", 0.01))   # nn.LeakyReLU's default
        if not np.isfinite(self.negative_slope):
            raise ValueError("HiFiGANGenerator: negative_slope is not finite")
        self.use_weight_norm = use_weight_norm
        self.upsample_factor = hop
        self.aux_channels = self.in_channels
        self.training = True
        self._device = device
        self._state = {}
        self._math = "f16x3"
        self._normalizer = None
        self._ctx = self._h = None
        self._finalized = False
        self._norm_set = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_hfg_destroy(h)
            except Exception:
                pass

    # -- nn.Layer look-alikes ------------------------------------------------
    def set_state_dict(self, state_dict):
        self._state.update({k: to_numpy_f32(v) for k, v in state_dict.items()})
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
            raise NotImplementedError(f"HiFiGANGenerator.set_math({mode!r}): 'f32' and 'f16x3' are implemented")
        self._math = mode
        if self._h:
            self._apply_math()

    def set_normalizer(self, normalizer):
        """Register ZScore statistics; applied only by calls passing ``normalize=True`` (what HiFiGANInference does)."""
        self._norm_owner = None
        self._normalizer = normalizer
        self._norm_set = False

    def _apply_math(self):
        m = {"f32": _capi.PK_PWG_MATH_F32, "f16x3": _capi.PK_PWG_MATH_F16X3}[self._math]
        _capi.check(self._ctx.lib.pk_hfg_set_math(self._h, m))

    def _cfg(self):
        cfg = _capi.HfgCfg()
        cfg.in_channels, cfg.out_channels, cfg.channels = self.in_channels, self.out_channels, self.channels
        cfg.kernel_size, cfg.n_upsample = self.kernel_size, len(self.upsample_scales)
        for i, (s, k) in enumerate(zip(self.upsample_scales, self.upsample_kernel_sizes)):
            cfg.upsample_scales[i], cfg.upsample_kernel_sizes[i] = s, k
        cfg.n_blocks = len(self.resblock_kernel_sizes)
        for j, (k, ds) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilations)):
            cfg.resblock_kernel_sizes[j], cfg.n_dilations[j] = k, len(ds)
            for n, d in enumerate(ds):
                cfg.resblock_dilations[j][n] = d
        cfg.use_additional_convs, cfg.bias = int(self.use_additional_convs), 1
        cfg.negative_slope = self.negative_slope
        return cfg

    def _engine(self):
        """The finalized handle on the current stream's context (created at the first call that computes)."""
        ctx = Context.get(self._device)
        if self._h is None:
            cfg = self._cfg()
            h = C.c_void_p()
            _capi.check(ctx.lib.pk_hfg_create(ctx.handle, C.byref(cfg), C.byref(h)))
            self._ctx, self._h = ctx, h
            self._apply_math()
        if not self._finalized:
            set_params(ctx.lib.pk_hfg_set_param, self._h, self._state)
            _capi.check(ctx.lib.pk_hfg_finalize(self._h))
            self._finalized = True
        if not self._norm_set:
            if self._normalizer is None:
                _capi.check(ctx.lib.pk_hfg_set_normalizer(self._h, None, None, 0))
            else:
                mu = to_numpy_f32(self._normalizer.mu).reshape(-1)
                sigma = to_numpy_f32(self._normalizer.sigma).reshape(-1)
                _capi.check(ctx.lib.pk_hfg_set_normalizer(self._h, _capi.fptr(mu), _capi.fptr(sigma), mu.size))
            self._norm_set = True
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
        wav = ctx.empty((int(frames.sum()) * self.upsample_factor,))
        _capi.check(ctx.lib.pk_hfg_infer(self._h, dptr(mel), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(frames),
                                         dptr(wav), _capi.PK_APPLY_NORMALIZER if normalize else 0))
        return wav

    def inference_batch(self, mels, normalize=False):
        """mels: list of (T'_b, in_channels) arrays.  Returns a list of (T'_b * hop, 1) device tensors; one engine call."""
        ctx = self._engine()
        frames = [int(m.shape[0]) for m in mels]
        mel = torch.cat([ctx.to_device(m).reshape(-1, self.in_channels) for m in mels], dim=0)
        wav = self._infer(ctx, mel, frames, normalize)
        outs, o = [], 0
        for f in frames:
            n = f * self.upsample_factor
            outs.append(wrap(wav[o:o + n].reshape(n, self.out_channels)))
            o += n
        return outs

    def infer_packed(self, mel, frames, noise=None, generator=None, normalize=False):
        """mel: packed (sum(frames), in_channels) DEVICE tensor (e.g. FastSpeech2.decode_packed()); returns the packed
        (sum(frames) * hop,) device waveform.  ``noise`` / ``generator`` exist so that the call site is the one of
        PWGGenerator: HiFi-GAN takes no noise, anything but None raises."""
        if noise is not None or generator is not None:
            raise ValueError("HiFiGANGenerator takes no noise input")
        ctx = self._engine()
        mel = ctx.to_device(mel).reshape(-1, self.in_channels)
        return self._infer(ctx, mel, frames, normalize)

    def forward(self, c):
        """(N, in_channels, T') -> (N, 1, T' * hop)."""
        ctx = self._engine()
        c = ctx.to_device(c)
        if c.dim() != 3 or c.shape[1] != self.in_channels:
            raise AssertionError(f"expected (N, {self.in_channels}, T'), got {tuple(c.shape)}")
        N, _, T = c.shape
        mel = c.transpose(1, 2).contiguous().reshape(-1, self.in_channels)
        wav = self._infer(ctx, mel, [T] * N, False)
        return wrap(wav.reshape(N, self.out_channels, -1))

    __call__ = forward

    def inference(self, c, normalize=False):
        """(T', in_channels) -> (T' * hop, 1)."""
        return self.inference_batch([c], normalize=normalize)[0]

    def debug_stages(self, b=0):
        """Test tap: the output of every stage (after its block mean) of utterance b of the last call, a list of
        (channels >> (i + 1), T'_b * scales up to stage i) float32 numpy (``pk_hfg_debug_read``; runs the stack again)."""
        ctx = self._engine()
        res, n = [], self._last_frames[b]
        for i, s in enumerate(self.upsample_scales):
            n *= s
            out = np.empty((self.channels >> (i + 1), n), dtype=np.float32)
            _capi.check(ctx.lib.pk_hfg_debug_read(self._h, i, b, _capi.fptr(out), out.size))
            res.append(out)
        return res

    def debug_convs(self, b=0):
        """Test tap: what every launch before the output convolution wrote for utterance b of the last call, in launch order
        (``pk_hfg_debug_conv``): input_conv; per stage the transposed convolution, then per residual block and dilation
        convs1's t (with use_additional_convs) and t + y -- the block's last one holds the running block mean instead."""
        ctx = self._engine()
        shapes, n = [(self.channels, self._last_frames[b])], self._last_frames[b]
        for i, s in enumerate(self.upsample_scales):
            n *= s
            per_pair = 2 if self.use_additional_convs else 1
            shapes += [(self.channels >> (i + 1), n)] * (1 + per_pair * sum(len(d) for d in self.resblock_dilations))
        res = []
        for k, shape in enumerate(shapes):
            out = np.empty(shape, dtype=np.float32)
            _capi.check(ctx.lib.pk_hfg_debug_conv(self._h, k, b, _capi.fptr(out), out.size))
            res.append(out)
        return res


class HiFiGANInference:
    """normalizer(logmel) -> generator.inference, as PWGInference."""

    def __init__(self, normalizer, hifigan_generator):
        self.normalizer = normalizer
        self.generator = hifigan_generator
        self.bind()

    @property
    def hifigan_generator(self):
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
        return g

    def forward(self, logmel):
        return self.bind().inference(logmel, normalize=True)

    __call__ = forward

    def eval(self):
        return self
