"""float64 restatement of parakeet/modules/ssim.py:21-61, parakeet/modules/losses.py:60-100 (``weighted_mean``,
``masked_l1_loss``) and of the evaluator's Huber duration loss (speedyspeech_updater.py:129-136;
``paddle.fluid.layers.huber_loss``: r = label - input, 0.5 r^2 for |r| <= delta, delta (|r| - 0.5 delta) beyond).
TEST INFRASTRUCTURE ONLY.  Every function runs in the dtype asked for: float64 is the reference of the tests, float32 the
reference's own arithmetic."""
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def gaussian(window_size, sigma=1.5):
    """ssim.py:21-26: Python-double exp, rounded to float32, divided by its float32 sum."""
    g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


def window2d(window_size, dtype=torch.float64):
    """ssim.py:29-34 with channel = 1: the float32 outer product, then cast."""
    w = gaussian(window_size).unsqueeze(1)
    return torch.matmul(w, w.t()).to(dtype)


def ssim_map(img1, img2, window_size=11, dtype=torch.float64):
    """ssim.py:37-56 of two (H, W) images -> the (H, W) map as numpy in ``dtype``."""
    a = torch.as_tensor(np.asarray(img1)).to(dtype)[None, None]
    b = torch.as_tensor(np.asarray(img2)).to(dtype)[None, None]
    w = window2d(window_size, dtype)[None, None]
    p = window_size // 2
    mu1, mu2 = F.conv2d(a, w, padding=p), F.conv2d(b, w, padding=p)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = F.conv2d(a * a, w, padding=p) - mu1_sq
    s2 = F.conv2d(b * b, w, padding=p) - mu2_sq
    s12 = F.conv2d(a * b, w, padding=p) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m[0, 0].numpy()


def ssim(img1, img2, window_size=11, size_average=True, dtype=torch.float64):
    """ssim.py:77-80 for (B, C, H, W): channels are independent images (groups = channel)."""
    a, b = np.asarray(img1), np.asarray(img2)
    maps = np.stack([np.stack([ssim_map(a[i, c], b[i, c], window_size, dtype) for c in range(a.shape[1])])
                     for i in range(a.shape[0])])
    return maps.mean() if size_average else maps.mean(axis=(1, 2, 3))


def pair_sums(pred, target, rows=None, window_size=11, dtype=torch.float64):
    """One masked pair as pk_mel_loss_run sees it: (sum |pred - target| over the (L, W) entries, the (rows, W) SSIM map of
    both images zero-extended to ``rows``)."""
    pred, target = np.asarray(pred), np.asarray(target)
    rows = pred.shape[0] if rows is None else rows
    ext = lambda x: np.concatenate([x, np.zeros((rows - x.shape[0], x.shape[1]), x.dtype)])   # noqa: E731
    l1 = np.abs(pred.astype(np.float64) - target.astype(np.float64)).sum()
    return l1, ssim_map(ext(pred), ext(target), window_size, dtype)


def weighted_mean(x, weight):
    """losses.py:60-77."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    return (x * weight).sum() / (weight.sum() * (x.size / weight.size))


def masked_l1_loss(prediction, target, mask):
    """losses.py:80-100."""
    return weighted_mean(np.abs(np.asarray(prediction, np.float64) - np.asarray(target, np.float64)), mask)


def huber(pred, label, delta=1.0):
    r = np.asarray(label, np.float64) - np.asarray(pred, np.float64)
    a = np.abs(r)
    return np.where(a <= delta, 0.5 * r * r, delta * (a - 0.5 * delta))


def sequence_mask(lens, maxlen):
    return (np.arange(maxlen)[None, :] < np.asarray(lens)[:, None]).astype(np.float64)


def evaluate(decoded, pred_durations, durations, feats, num_frames, num_phones, window_size=11):
    """SpeedySpeechEvaluator.evaluate_core :119-142 in float64 -> dict of the four numbers."""
    decoded, feats = np.asarray(decoded, np.float64), np.asarray(feats, np.float64)
    B, L, _ = decoded.shape
    spec_mask = sequence_mask(num_frames, L)[:, :, None]
    text_mask = sequence_mask(num_phones, np.asarray(durations).shape[1])
    l1 = masked_l1_loss(decoded, feats, spec_mask)
    label = np.log(np.maximum(np.asarray(durations, np.float64), 1.0))
    dur = weighted_mean(huber(pred_durations, label), text_mask)
    ss = 1.0 - ssim((decoded * spec_mask)[:, None], (feats * spec_mask)[:, None], window_size)
    return {"l1_loss": float(l1), "ssim_loss": float(ss), "duration_loss": float(dur), "loss": float(l1 + ss + dur)}
