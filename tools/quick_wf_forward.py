"""WaveFlow forward() against infer() at BASELINE config 5's shape (8 x 640 frames), same process, same device:
    python tools/quick_wf_forward.py [channels] [math|-]
Prints ms per batch of both directions (median of 7 after 2 warm-up calls), the layer kernel's launches and time per launch."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from parakeet_amd import synthetic as syn
from parakeet_amd.runtime import Context
from parakeet_amd.waveflow import ConditionalWaveFlow

B, L = 8, 640
C = int(sys.argv[1]) if len(sys.argv) > 1 else 64
MATH = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
cfg = dict(syn.WAVEFLOW_LJSPEECH, channels=C)
m = ConditionalWaveFlow(**cfg)
m.set_state_dict(syn.waveflow_state(cfg, weight_norm=True))
m.eval()
if MATH:
    m.set_math(MATH)
rng = np.random.default_rng(0)
mels = [torch.tensor(np.maximum(rng.normal(-4, 2, size=(80, L)), np.log(1e-5)).astype(np.float32)).cuda() for _ in range(B)]
zs = [torch.randn(m.lengths(L)[0], device="cuda") for _ in range(B)]
auds = [0.3 * torch.randn(L * 256, device="cuda") for _ in range(B)]
ctx = Context.get()


def timed(fn, n=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def layer_stats(fn):
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    d = {k: v for k, v in ctx.prof_dump().items() if v[0] > 0}
    ctx.prof_enable(False)
    return d


fwd = lambda: m.forward_batch(auds, mels)
inf = lambda: m.infer_batch(mels, zs)
out = fwd()
assert all(bool(torch.isfinite(z).all()) for z, _ in out)
tf, ti = timed(fwd), timed(inf)
nf, ni = sum(z.numel() for z, _ in out), sum(o.numel() for o in inf())
print(f"WaveFlow C={C} math={MATH or 'f16x3'} B={B} L={L}")
print(f"  forward: {tf[0]*1e3:8.1f} ms/batch (min {tf[1]*1e3:.1f}, max {tf[2]*1e3:.1f}), {nf/tf[0]/1e6:.2f} Msamples/s")
print(f"  infer:   {ti[0]*1e3:8.1f} ms/batch (min {ti[1]*1e3:.1f}, max {ti[2]*1e3:.1f}), {ni/ti[0]/1e6:.2f} Msamples/s")
for name, fn in (("forward", fwd), ("infer", inf)):
    for k, (n_, ms) in sorted(layer_stats(fn).items()):
        print(f"  {name:8s} {k:22s} n={n_:5d} total={ms:9.3f} ms avg={ms/n_*1e3:9.1f} us")
