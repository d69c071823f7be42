"""rfx_fir_same at the workload's size -- 64 rows x 262144 samples, two signals, 101 A-weighting taps, forward (flip = 0) and adjoint
(flip = 1) -- against the call it replaces, F.conv1d(x, w, padding=50) on (64, 1, 262144) once per signal through torch-ROCm, and
against two floors: memory (each signal read once and written once, 2 x (read + write) = 268 MB per launch of two signals, over the
8 TB/s HBM roof) and arithmetic (R L K fused multiply-adds per signal at the 157.3 TFLOPS fp32 vector peak, which is the PACKED rate:
two FMAs per lane and instruction, v_pk_fma_f32 -- what hipcc emits for this kernel).

Method.  Kernel and conv1d are timed alternately in one process after a warm-up of each.  A window is as many back-to-back calls as
fill --window-s seconds (0.25 by default: ~2300 kernel calls, ~75 conv1d pairs), between two device events and ending in a
synchronise; --reps windows per path; min / median / max per call.  Calls rotate over --sets independent buffer sets (input, target
and both outputs; 3 sets = 805 MB, more than L2 + Infinity Cache), so no call finds its operands in a cache.  rfx_fir_same writes
preallocated outputs; F.conv1d has no `out=` and takes its outputs from torch's caching allocator (no device allocation after the
warm-up) -- that cost is part of the call it replaces.

    python scripts/perf_fir.py [--rows 64] [--length 262144] [--taps 101] [--window-s 0.25] [--reps 10] [--sets 3] [--no-conv1d]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from remfx_amd import losses, ops  # noqa: E402

HBM = 8.0e12
FMA_RATE = 157.3e12 / 2            # fp32 vector peak in fused multiply-adds per second (packed: 2 per lane and instruction)


def window(fn, calls):
    """us per call over `calls` back-to-back calls fn(i)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--length", type=int, default=262144)
    ap.add_argument("--taps", type=int, default=101)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--no-conv1d", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    R, L, K, S = a.rows, a.length, a.taps, a.sets
    g = torch.Generator().manual_seed(0)
    xs = [(torch.randn(R, L, generator=g) * 0.3).to(dev) for _ in range(S)]
    ts = [(torch.randn(R, L, generator=g) * 0.3).to(dev) for _ in range(S)]
    yxs, yts = [torch.empty_like(x) for x in xs], [torch.empty_like(t) for t in ts]
    h = torch.from_numpy(losses.a_weighting_taps(48000, K).astype(np.float32)).to(dev)
    nbytes = 2 * 2 * R * L * 4
    print(f"{R} x {L}, K = {K}, two signals, {S} buffer sets of {nbytes / 1e6:.1f} MB: HBM floor {nbytes / HBM * 1e6:.1f} us, "
          f"packed fp32 FMA floor {2 * R * L * K / FMA_RATE * 1e6:.1f} us", flush=True)
    def fir(flip, i):
        j = i % S
        ops.launch("rfx_fir_same", xs[j], yxs[j], ts[j], yts[j], R, L, L, L, L, L, h, K, flip)

    w = {0: h.view(1, 1, K), 1: h.flip(0).contiguous().view(1, 1, K)}

    def conv(flip, i):
        j = i % S
        F.conv1d(xs[j].view(R, 1, L), w[flip], padding=K // 2)
        F.conv1d(ts[j].view(R, 1, L), w[flip], padding=K // 2)

    paths = [("rfx_fir_same", fir)] + ([] if a.no_conv1d else [("F.conv1d x 2", conv)])
    for flip in (0, 1):
        calls = {}
        for name, fn in paths:                                        # warm-up (code objects, algorithm choice) and window size
            window(lambda i: fn(flip, i), 2 * S)
            per = window(lambda i: fn(flip, i), 4 * S)
            calls[name] = max(4 * S, int(a.window_s * 1e6 / per))
        times = {name: [] for name, _ in paths}
        for _ in range(a.reps):
            for name, fn in paths:
                times[name].append(window(lambda i: fn(flip, i), calls[name]))
        for name, _ in paths:
            us = sorted(times[name])
            med = us[len(us) // 2]
            print(f"flip = {flip} {name:14s} {calls[name]:5d} calls per window: min {us[0]:8.1f}  median {med:8.1f}  max {us[-1]:8.1f} us "
                  f"per call = {nbytes / (med * 1e-6) / 1e12:.2f} TB/s, {nbytes / (med * 1e-6) / HBM:.2f} of the HBM roof, "
                  f"{2 * R * L * K / FMA_RATE / (med * 1e-6):.2f} of the fp32 vector peak", flush=True)
        if not a.no_conv1d:
            fir(flip, 0)
            ref = F.conv1d(xs[0].view(R, 1, L), w[flip], padding=K // 2).view(R, L)
            print(f"flip = {flip} max |rfx_fir_same - F.conv1d| = {float((yxs[0] - ref).abs().max()):.3e} "
                  f"(max |y| {float(ref.abs().max()):.3f})", flush=True)


if __name__ == "__main__":
    main()
