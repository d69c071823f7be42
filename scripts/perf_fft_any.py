"""Dev tool: analysis (complex_fm) and synthesis (the STFT's adjoint) of the generic framed FFT (csrc/fft_any.hip) at every size it
serves, on 64 x 262144 samples at hop = n_fft / 4, with the 1024- and 4096-point kernels of csrc/fft.hip from the same run for scale.
One process, one GPU; HIP events around single launches after warm-up, median of 20.  Bytes = signal + spectrum (each moved once);
the fraction is of 8.0 TB/s."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from remfx_amd import ops, stft

dev = torch.device("cuda:0")
R, L = 64, 262144
SIZES = (16, 32, 64, 128, 256, 1024, 4096, 8192, 16384, 32768)
HBM = 8.0e12


def median_us(fn, warm=5, n=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    x = torch.randn(R, L, device=dev)
    print(f"{'n_fft':>6} {'frames':>7} {'GB':>7} {'analysis us':>12} {'of HBM':>7} {'synthesis us':>13} {'of HBM':>7} {'scratch GB':>11}")
    for n in SIZES:
        hop, frames, bins = n // 4, 1 + L // (n // 4), n // 2 + 1
        w = stft.hann(n, dev)
        X = torch.empty((R, frames, bins, 2), device=dev)
        d = stft._desc(R, L, n, hop, n, bins, 0, frames, 5)
        ana = lambda: ops.launch("rfx_fft_analysis", C.byref(d), x, w, None, X)
        t_a = median_us(ana)
        ws, gx = stft.syn_ws(d, dev), torch.empty_like(x)
        syn = lambda: ops.launch("rfx_fft_synthesis", C.byref(d), X, w, None, ws, gx)
        t_s = median_us(syn)
        nbytes = x.numel() * 4 + X.numel() * 4
        print(f"{n:>6} {frames:>7} {nbytes / 1e9:>7.3f} {t_a:>12.1f} {nbytes / (t_a * 1e-6) / HBM:>7.3f} {t_s:>13.1f} "
              f"{nbytes / (t_s * 1e-6) / HBM:>7.3f} {ws.numel() * 4 / 1e9:>11.3f}", flush=True)
        del X, ws, gx


if __name__ == "__main__":
    main()
