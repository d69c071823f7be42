"""Times rfx_wiener (csrc/wiener.hip) at Open-Unmix's own shape -- n_fft 4096, hop 1024, two channels, four targets +
residual, one EM iteration, windows of 300 frames, 4 clips of 262144 samples -- next to what a port without the kernel would run:
the fp32 restatement of tests/wiener_ref.py (upstream's operation order) as torch ops on the device, one Python loop over samples and
windows as upstream has it (its sums over the frames as torch.sum: upstream adds them in pieces of 200 frames, not one by one).

Prints both times (device events, warm-up first, median of the repeats), the largest difference between the two results in units of
the window's scale, and the kernel's share of the HBM roofline on the algorithmic bytes: S and X read once, Y written once.

    python scripts/perf_wiener.py [--clips 4] [--niter 1] [--repeats 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes / s, MI355X datasheet
EPS = 1e-10


def torch_wiener(X, S, B, C, W, niter, residual):
    """tests/wiener_ref.wiener32 over torch ops: X (B*C, bins, frames) complex64, S (J0, B*C, bins, frames) -> (B, J, C, bins, frames)"""
    bins, frames = X.shape[-2:]
    X, S = X.view(B, C, bins, frames), S.view(-1, B, C, bins, frames)
    J = S.shape[0] + residual
    Y = torch.empty((B, J, C, bins, frames), dtype=torch.complex64, device=X.device)
    eye = torch.eye(C, device=X.device) * EPS ** 0.5
    for b in range(B):
        for t0 in range(0, frames, W):
            x, s = X[b, :, :, t0:t0 + W], S[:, b, :, :, t0:t0 + W]
            ang = torch.atan2(x.imag, x.real)
            y = torch.complex(s * torch.cos(ang), s * torch.sin(ang))
            if residual:
                y = torch.cat([y, (x - y.sum(0))[None]], 0)
            if niter > 0:
                m = torch.clamp(x.abs().max() / 10, min=1.0)
                x, y = x / m, y / m
                for _ in range(niter):
                    v = (y.real ** 2 + y.imag ** 2).sum(1) / C                                  # (J, bins, n)
                    R = (y[:, :, None] * y[:, None, :].conj()).sum(-1) / (EPS + v.sum(-1))[:, None, None]
                    R = R.permute(0, 3, 1, 2)                                                   # (J, bins, C, C)
                    Cxx = eye + (v[..., None, None] * R[:, :, None]).sum(0)                     # (bins, n, C, C)
                    if C == 1:
                        inv = 1.0 / Cxx
                    else:
                        det = Cxx[..., 0, 0] * Cxx[..., 1, 1] - Cxx[..., 0, 1] * Cxx[..., 1, 0]
                        inv = torch.stack([torch.stack([Cxx[..., 1, 1], -Cxx[..., 0, 1]], -1),
                                           torch.stack([-Cxx[..., 1, 0], Cxx[..., 0, 0]], -1)], -2) / det[..., None, None]
                    xv = x.permute(1, 2, 0)                                                     # (bins, n, C)
                    out = []
                    for j in range(J):
                        G = torch.zeros_like(inv)
                        for i1 in range(C):
                            for i2 in range(C):
                                for i3 in range(C):
                                    G[..., i1, i2] += R[j][:, None, i1, i3] * inv[..., i3, i2]
                        G = G * v[j][..., None, None]
                        out.append(sum(G[..., i] * xv[..., i, None] for i in range(C)).permute(2, 0, 1))
                    y = torch.stack(out)
                y = y * m
            Y[b, ..., t0:t0 + W] = y
    return Y


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--niter", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_wiener.py measures on the GPU; none found")
    from remfx_amd import ops
    B, C, J0, residual, W, n_fft, hop = a.clips, 2, 4, 1, 300, 4096, 1024
    bins, frames, J = n_fft // 2 + 1, 1 + a.samples // hop, J0 + residual
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((B * C, bins, frames, 2), device="cuda", generator=g)
    S = torch.view_as_complex(X).abs()[None] * torch.rand((J0, B * C, bins, frames), device="cuda", generator=g)
    Y = torch.empty((B, J, C, bins, frames, 2), device="cuda")
    ws = torch.empty((ops.query("rfx_wiener_ws_floats", B, C, bins, frames, W),), device="cuda")

    def kernel():
        ops.launch("rfx_wiener", X, S, Y, B, C, J0, residual, bins, frames, W, a.niter, 0, ws)

    Xc = torch.view_as_complex(X)
    k_ms = timed(kernel, 3, a.repeats)
    t_ms = timed(lambda: torch_wiener(Xc, S, B, C, W, a.niter, residual), 1, max(3, a.repeats // 4))
    ref = torch_wiener(Xc, S, B, C, W, a.niter, residual)
    diff = float((torch.view_as_complex(Y) - ref).abs().max() / Xc.abs().max())
    nbytes = S.numel() * 4 + X.numel() * 4 + Y.numel() * 4
    out = {"shape": {"clips": B, "channels": C, "targets": J0, "residual": bool(residual), "bins": bins, "frames": frames, "window": W,
                     "niter": a.niter},
           "kernel_ms": {"median": k_ms[0], "min": k_ms[1], "max": k_ms[2]},
           "torch_restatement_ms": {"median": t_ms[0], "min": t_ms[1], "max": t_ms[2]},
           "speedup_median": t_ms[0] / k_ms[0],
           "algorithmic_bytes": nbytes, "kernel_bytes_per_s": nbytes / (k_ms[0] * 1e-3),
           "hbm_roofline_fraction": nbytes / (k_ms[0] * 1e-3) / HBM_PEAK,
           "largest_difference_over_scale": diff}
    print(f"rfx_wiener            {k_ms[0]:9.3f} ms (min {k_ms[1]:.3f}, max {k_ms[2]:.3f}), two launches")
    print(f"torch-op restatement  {t_ms[0]:9.3f} ms (min {t_ms[1]:.3f}, max {t_ms[2]:.3f})   x{t_ms[0] / k_ms[0]:.1f}")
    print(f"algorithmic bytes {nbytes / 1e6:.1f} MB -> {nbytes / (k_ms[0] * 1e-3) / 1e12:.3f} TB/s = {out['hbm_roofline_fraction']:.3f} of the "
          f"{HBM_PEAK / 1e12:.1f} TB/s HBM peak; largest difference between the two results {diff:.2e} of max |X|")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
