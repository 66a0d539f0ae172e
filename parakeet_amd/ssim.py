"""``parakeet/modules/ssim.py`` on the HIP engine: ``gaussian`` (:21-26), ``create_window`` (:29-34), ``ssim`` (:77-80) and
class ``SSIM`` (:64-74), plus ``ssim_per_pair`` for ragged lists of mel spectrograms.  The map is computed by
``pk_mel_loss_run`` (csrc/mel_loss.hip), which builds the reference's window itself; the device leaves each image's sum of
the map, the means are formed on the host in float64.  Inference only: no gradients."""
from math import exp

import numpy as np
import torch

from .losses import mel_loss_sums
from .runtime import Context, wrap


def gaussian(window_size, sigma):
    """(window_size,) float32: exp in Python doubles, rounded to float32, divided by its float32 sum."""
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                         dtype=torch.float32)
    return gauss / gauss.sum()


def create_window(window_size, channel):
    """(channel, 1, window_size, window_size): the outer product of ``gaussian(window_size, 1.5)`` for every channel."""
    w1 = gaussian(window_size, 1.5).unsqueeze(1)
    w2 = torch.matmul(w1, w1.t()).unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous()


def _image_sums(img1, img2, window_size):
    ctx = Context.get()
    a, b = ctx.to_device(img1), ctx.to_device(img2)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"img1 {tuple(a.shape)} and img2 {tuple(b.shape)} must be one (B, C, H, W) shape")
    B, Cn, H, W = a.shape
    if H == 0 or W == 0 or B * Cn == 0:
        raise ValueError(f"empty images {tuple(a.shape)}")
    # groups = channel: every (item, channel) plane is an image of its own
    sums = mel_loss_sums(a.reshape(B * Cn * H, W), b.reshape(B * Cn * H, W), [H] * (B * Cn), window_size=window_size)
    return sums[:, 1].reshape(B, Cn), H * W


def ssim(img1, img2, window_size=11, size_average=True):
    """ssim.py:77-80: (B, C, H, W) pairs -> the mean of the SSIM map (0-d), or with ``size_average=False`` its mean per batch
    item (B,); float32 device tensors."""
    per, n = _image_sums(img1, img2, window_size)
    dev = Context.get().device
    if size_average:
        return wrap(torch.tensor(per.sum() / (per.size * n), dtype=torch.float32, device=dev))
    return wrap(torch.tensor(per.sum(1) / (per.shape[1] * n), dtype=torch.float32, device=dev))


class SSIM:
    """ssim.py:64-74."""

    def __init__(self, window_size=11, size_average=True):
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.window = create_window(window_size, self.channel)

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)

    __call__ = forward


def ssim_per_pair(preds, targets, window_size=11):
    """Ragged lists of (L_b, W) mels -> (B,) float64 numpy: the SSIM of every pair, each scored as ``ssim`` scores a batch of
    one.  One pass over the batch; a pair's number is the same bits in any batch."""
    ctx = Context.get()
    ps, ts = [ctx.to_device(p) for p in preds], [ctx.to_device(t) for t in targets]
    if len(ps) != len(ts) or len(ps) == 0:
        raise ValueError(f"{len(ps)} predictions against {len(ts)} targets")
    for b, (p, t) in enumerate(zip(ps, ts)):
        if p.dim() != 2 or p.shape != t.shape or p.shape[1] != ps[0].shape[1] or p.numel() == 0:
            raise ValueError(f"pair {b}: prediction {tuple(p.shape)}, target {tuple(t.shape)}")
    lens = [int(p.shape[0]) for p in ps]
    sums = mel_loss_sums(torch.cat(ps) if len(ps) > 1 else ps[0], torch.cat(ts) if len(ts) > 1 else ts[0], lens,
                         window_size=window_size)
    return sums[:, 1] / (np.asarray(lens, np.float64) * ps[0].shape[1])
