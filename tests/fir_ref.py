"""fp64 reference of the 'same'-padded FIR (rfx_fir_same) and an independent restatement of the A-weighting IIR the `aw` taps are fitted
to, for tests/test_fir_cpu.py and tests/test_gpu_fir.py.  Test infrastructure only.

  fir_same(x, h)              F.conv1d(x, h, padding=K // 2) on (R, 1, L) in float64: y[n] = sum_k h[k] x[n + k - K/2], zeros outside
  fir_same(x, h, flip=True)   the same call with the kernel flipped, h[K-1-k]: with odd K and this padding its exact adjoint
  fir_loop                    the definition as an explicit double loop (tests/test_fir_cpu.py checks fir_same against it)
  fir_bound(x, h)             (K + 2) 2^-24 sum_k |h_k| |x_(n+k-K/2)| + 2^-126 per sample, evaluated in float64: what ANY fp32 evaluation
                              of the sum can be off by -- K products and K - 1 adds, each one rounding (unit roundoff u = 2^-24), give
                              gamma_K = K u / (1 - K u) <= (K + 2) u for K <= 1025 in any order, fused or not, and the last term
                              covers a subnormal result

auraloss is not available: the A-weighting construction (IEC/CD 1672 prototype, bilinear transform) is restated, PARITY UNPINNED.
"""
import numpy as np
import torch
import torch.nn.functional as F


def fir_same(x, h, flip=False):
    """x (..., L), h (K,), K odd -> float64 tensor of x's shape."""
    x = torch.as_tensor(x, dtype=torch.float64)
    h = torch.as_tensor(h, dtype=torch.float64)
    K = h.numel()
    assert K % 2 == 1
    w = (h.flip(0) if flip else h).view(1, 1, K)
    return F.conv1d(x.reshape(-1, 1, x.shape[-1]), w, padding=K // 2).reshape(x.shape)


def fir_loop(row, h, flip=False):
    """One row as lists of Python floats: the definition, sample by sample and tap by tap."""
    L, K = len(row), len(h)
    out = []
    for n in range(L):
        acc = 0.0
        for k in range(K):
            m = n + k - K // 2
            if 0 <= m < L:
                acc += (h[K - 1 - k] if flip else h[k]) * row[m]
        out.append(acc)
    return out


def fir_bound(x, h, flip=False):
    h = torch.as_tensor(h, dtype=torch.float64)
    return (h.numel() + 2) * 2.0 ** -24 * fir_same(torch.as_tensor(x, dtype=torch.float64).abs(), h.abs(), flip) + 2.0 ** -126


def a_weighting_iir(fs):
    """(b, a) of the digital A-weighting filter: the analog prototype with a double pole at f1 and at f4, single poles at f2 and f3, four
    zeros at 0 and unit gain at 1 kHz, through the bilinear transform."""
    import scipy.signal
    f1, f2, f3, f4 = 20.598997, 107.65265, 737.86223, 12194.217
    gain = (2 * np.pi * f4) ** 2 * 10 ** (1.9997 / 20)
    poles = [-2 * np.pi * f1] * 2 + [-2 * np.pi * f4] * 2 + [-2 * np.pi * f2, -2 * np.pi * f3]
    return scipy.signal.bilinear(gain * np.poly([0.0] * 4), np.poly(poles), fs=fs)


def magnitude_db(b, a, freqs, fs):
    import scipy.signal
    _, h = scipy.signal.freqz(b, a, worN=np.asarray(freqs, dtype=np.float64), fs=fs)
    return 20 * np.log10(np.abs(h))
