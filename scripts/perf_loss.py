"""Dev tool: time the MRSTFT loss forward + backward alone (64 clips x 2 channels x 262144 samples).
usage: python scripts/perf_loss.py [--scale mel [--n-bins 64]] [--unpaired] [--clips 64]
  --scale mel   the mel-scaled loss (rfx_stft_scaled_loss / _grad on memoised spectra)
  --unpaired    the linear loss through two analyses + rfx_stft_loss_reduce / rfx_stft_loss_grad + synthesis (RFX_LOSS_PAIRED=0):
                the path that moves the same spectra as the scaled one, its comparison point"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--scale", choices=("linear", "mel"), default="linear")
ap.add_argument("--n-bins", type=int, default=64)       # 64 / 80 fit the 512-point resolution at 48 kHz; 96 leaves empty filters
ap.add_argument("--unpaired", action="store_true")
ap.add_argument("--clips", type=int, default=64)
args = ap.parse_args()
if args.unpaired:
    os.environ["RFX_LOSS_PAIRED"] = "0"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from remfx_amd import losses, ops

dev = "cuda:0"
ops.set_gemm_precision("bf16")
kw = dict(scale="mel", n_bins=args.n_bins, sample_rate=48000) if args.scale == "mel" else {}
crit = losses.MultiResolutionSTFTLoss(**kw).to(dev)
x = torch.randn(args.clips, 2, 262144, device=dev, requires_grad=True)
y = torch.randn(args.clips, 2, 262144, device=dev)


def step():
    x.grad = None
    l = crit(x, y)
    l.backward()
    return l


for _ in range(3):
    step()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10):
    l = step()
e1.record()
torch.cuda.synchronize()
what = f"mel x{args.n_bins}" if args.scale == "mel" else ("linear, unpaired" if args.unpaired else "linear")
print(f"MRSTFT loss fwd + bwd ({what}): {e0.elapsed_time(e1) / 10:.3f} ms  (loss {float(l):.5f})")
