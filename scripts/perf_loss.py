"""Dev tool: time the MRSTFT loss forward + backward alone (64 clips x 2 channels x 262144 samples).
usage: python scripts/perf_loss.py [--scale mel [--n-bins 64]] [--unpaired] [--clips 64]
       python scripts/perf_loss.py --time-loss KIND [--prefilter] [--clips 64]
  --scale mel   the mel-scaled loss (rfx_stft_scaled_loss / _grad on memoised spectra)
  --unpaired    the linear loss through two analyses + rfx_stft_loss_reduce / rfx_stft_loss_grad + synthesis (RFX_LOSS_PAIRED=0):
                the path that moves the same spectra as the scaled one, its comparison point
  --time-loss KIND   one of the time-domain losses (sisdr, sdsdr, snr, esr, dc, logcosh) on clips x 262144 samples, forward (sums + rows)
                and backward timed apart, next to L1Loss (rfx_l1_sum / rfx_l1_grad) on the same tensors: the same bytes -- read
                2 x clips x 1 MiB, write clips x 1 MiB in the backward -- so the natural yardstick, and the share of the HBM roofline
  --prefilter   with --time-loss: the pre-emphasis prefilter (-0.85, 1, 0)"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--scale", choices=("linear", "mel"), default="linear")
ap.add_argument("--n-bins", type=int, default=64)       # 64 / 80 fit the 512-point resolution at 48 kHz; 96 leaves empty filters
ap.add_argument("--unpaired", action="store_true")
ap.add_argument("--clips", type=int, default=64)
ap.add_argument("--time-loss", choices=("sisdr", "sdsdr", "snr", "esr", "dc", "logcosh"))
ap.add_argument("--prefilter", action="store_true")
args = ap.parse_args()
if args.unpaired:
    os.environ["RFX_LOSS_PAIRED"] = "0"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from remfx_amd import losses, ops

dev = "cuda:0"
HBM_BYTES_PER_S = 8.0e12                                   # MI355X HBM3E peak


def time_domain():
    """Forward and backward of one time-domain loss and of L1Loss on the same (clips, 262144) tensors, alternating, 20 rounds."""
    L = 262144
    kw = dict(prefilter=(-0.85, 1.0, 0.0)) if args.prefilter else {}
    cands = {args.time_loss + (" + prefilter" if args.prefilter else ""): losses.TIME_LOSSES[args.time_loss](**kw), "l1": losses.L1Loss()}
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(args.clips, L, generator=g) * 0.3 + 0.05).to(dev).requires_grad_(True)
    y = (x.detach() + 0.1 * torch.randn(args.clips, L, generator=g).to(dev))
    acc = {k: [0.0, 0.0] for k in cands}
    rounds = 20
    for it in range(3 + rounds):
        for name, crit in cands.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            x.grad = None
            ev[0].record()
            l = crit(x, y)
            ev[1].record()
            l.backward()
            ev[2].record()
            torch.cuda.synchronize()
            if it >= 3:
                acc[name][0] += ev[0].elapsed_time(ev[1])
                acc[name][1] += ev[1].elapsed_time(ev[2])
    nbytes = args.clips * L * 4
    for name, (f, b) in acc.items():
        f, b = f / rounds * 1e-3, b / rounds * 1e-3
        print(f"{name:>18}: forward {f * 1e6:8.1f} us ({2 * nbytes / f / HBM_BYTES_PER_S:5.1%} of HBM peak)   "
              f"backward {b * 1e6:8.1f} us ({3 * nbytes / b / HBM_BYTES_PER_S:5.1%})   [{args.clips} x {L}, device events, "
              f"launch overhead of the autograd call included]")


if args.time_loss:
    time_domain()
    sys.exit(0)
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
