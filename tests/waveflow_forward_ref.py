"""ConditionalWaveFlow.forward and WaveFlowLoss restated in plain torch (fp32 or fp64), composed from oracle/waveflow_ref.py.

Follows parakeet/models/waveflow.py:
  ConditionalWaveFlow.forward   :759-782   (the encoder WITHOUT trim_conv_artifact, :780)
  WaveFlow._trim                :617-625, WaveFlow.forward :627-672 (fold :653-656, shuffle after every flow :664-665,
                                log_det_jacobian = sum of all logs :671)
  Flow.forward                  :465-494   (_predict_parameters :452-457 on rows 0..H-2 with condition rows 1..H-1, _transform :459-463)
  ResidualBlock.forward         :199-246   (causal (3, 3) conv: padding rh - 1 rows on top, "same" in width :229-236)
  ResidualNet.forward           :345-366   (sum of the skips)
  WaveFlowLoss                  :855-891
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import waveflow_ref as wr
from oracle.nn_ref import Weights, fold_weight_norm


def flow_forward(W, x, cond, n_layers, dil_h):
    """Flow.forward :465-494.  x (B,1,H,Wd), cond (B,Cm,H,Wd) -> z (B,1,H,Wd), logs (B,1,H-1,Wd)."""
    h = F.conv2d(x[:, :, :-1, :], W["input_proj.weight"], W["input_proj.bias"])      # :453, 491
    c = cond[:, :, 1:, :]                                                            # :492
    skips = 0
    for l in range(n_layers):
        wl = W.sub(f"resnet.{l}.")
        cw = wl["conv.weight"]
        kh, kw = cw.shape[2], cw.shape[3]
        dh, dw = dil_h[l], 2 ** l
        rh, rw = 1 + (kh - 1) * dh, 1 + (kw - 1) * dw
        y = F.conv2d(F.pad(h, (rw // 2, (rw - 1) // 2, rh - 1, 0)), cw, wl["conv.bias"], dilation=(dh, dw))   # :229-236
        y = y + F.conv2d(c, wl["condition_proj.weight"], wl["condition_proj.bias"])  # :238
        content, gate = torch.chunk(y, 2, dim=1)
        y = torch.tanh(content) * torch.sigmoid(gate)                                # :240-241
        y = F.conv2d(y, wl["out_proj.weight"], wl["out_proj.bias"])
        res, skip = torch.chunk(y, 2, dim=1)                                         # :243-245
        h = h + res
        skips = skips + skip                                                         # ResidualNet.forward :361-365
    params = F.conv2d(skips, W["output_proj.weight"], W["output_proj.bias"])         # :455
    logs, b = torch.chunk(params, 2, dim=1)
    z = torch.cat([x[:, :, :1, :], x[:, :, 1:, :] * torch.exp(logs) + b], dim=2)     # _transform :459-463
    return z, logs


def waveflow_forward(W, x, cond, cfg):
    """WaveFlow.forward :627-672.  x (B,T), cond (B,Cm,Tc >= T) -> z (B,T'), logdet per utterance (B,)."""
    ng = cfg["n_group"]
    assert cond.shape[-1] >= x.shape[-1]             # _trim :618
    pruned = x.shape[-1] // ng * ng
    x = x[:, :pruned]
    cond = cond[:, :, :pruned]
    B = x.shape[0]
    x = x.reshape(B, pruned // ng, ng).transpose(1, 2).unsqueeze(1)
    cond = cond.reshape(B, cond.shape[1], pruned // ng, ng).transpose(2, 3)
    perms = wr.create_perms(ng, cfg["n_flows"])
    logdet = torch.zeros(B, dtype=x.dtype)
    for i in range(cfg["n_flows"]):
        x, logs = flow_forward(W.sub(f"{i}."), x, cond, cfg["n_layers"], wr.DILATIONS_H[ng])
        logdet = logdet + logs.reshape(B, -1).sum(1)
        p = torch.tensor(perms[i])
        x = torch.index_select(x, 2, p)              # :664
        cond = torch.index_select(cond, 2, p)        # :665
    return x.squeeze(1).transpose(1, 2).reshape(B, -1), logdet


def condition(state, mel, cfg, dtype=torch.float64):
    """The untrimmed upsampled mel (:780): (B, Cm, T_mel * hop)."""
    W = Weights(fold_weight_norm(state), dtype)
    return wr.upsample(W.sub("encoder."), torch.as_tensor(mel).to(dtype), cfg["upsample_factors"], trim=False)


def forward(state, audio, mel, cfg, dtype=torch.float64):
    """ConditionalWaveFlow.forward :759-782.  audio (B,T), mel (B,Cm,T_mel) -> z (B,T'), logdet (B,) per utterance (the reference
    returns their sum)."""
    cfg = dict(wr.DEFAULT_CFG, **(cfg or {}))
    W = Weights(fold_weight_norm(state), dtype)
    with torch.no_grad():
        cond = wr.upsample(W.sub("encoder."), torch.as_tensor(mel).to(dtype), cfg["upsample_factors"], trim=False)
        return waveflow_forward(W.sub("decoder."), torch.as_tensor(audio).to(dtype), cond, cfg)


def inverse(state, z, mel, cfg, dtype=torch.float64):
    """WaveFlow.inverse :674-711 under the UNTRIMMED condition: the audio whose forward() is z (n_flows a multiple of 4)."""
    cfg = dict(wr.DEFAULT_CFG, **(cfg or {}))
    W = Weights(fold_weight_norm(state), dtype)
    with torch.no_grad():
        cond = wr.upsample(W.sub("encoder."), torch.as_tensor(mel).to(dtype), cfg["upsample_factors"], trim=False)
        return wr.waveflow_inverse(W.sub("decoder."), torch.as_tensor(z).to(dtype), cond, cfg)


def loss(z, logdet, sigma=1.0):
    """WaveFlowLoss.forward :870-891 (z and logdet as numpy / torch, any shape; float out)."""
    z = np.asarray(z, dtype=np.float64)
    const = 0.5 * np.log(2 * np.pi) + np.log(sigma)                                  # :868
    return float(((z * z).sum() / (2 * sigma * sigma) - float(np.asarray(logdet, dtype=np.float64).sum())) / z.size + const)
