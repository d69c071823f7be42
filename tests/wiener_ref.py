"""Restatements of Open-Unmix's Wiener filter with expectation-maximisation (open-unmix-pytorch `filtering.wiener` +
`expectation_maximization`) for tests/test_gpu_wiener_kernel.py and tests/test_gpu_umx_separator.py:

    wiener64   the algorithm as include/remfx_hip.h states it, numpy complex128
    wiener32   the same in fp32 in upstream's operation order: atan2 / cos / sin initialisation, the gain G_j = v_j R_j Cxx^-1 formed
               before it is applied, sums over the frames added one frame after the other

Layouts are the kernel's: X (B*C, bins, frames) complex, S (J0, B*C, bins, frames) real -> Y (B, J, C, bins, frames) complex.
`window_scales` gives max |X| per (sample, window) -- the unit the kernel's error is judged in."""
import numpy as np

EPS = 1e-10


def make_case(seed, B, C, J0, bins, frames, amp=1.0):
    """X (B*C, bins, frames) complex64 normal of scale amp, S (J0, B*C, bins, frames) float32 = |X| U(0, 1); one cell of X (last row, frame 0)
    and one of S (first row, frame 1) are zero (both in every case: atan2(0, 0) and a source without energy in a cell)"""
    g = np.random.default_rng(seed)
    X = ((g.standard_normal((B * C, bins, frames)) + 1j * g.standard_normal((B * C, bins, frames))) * amp).astype(np.complex64)
    X[-1, -1, 0] = 0
    S = (np.abs(X)[None] * g.random((J0, B * C, bins, frames))).astype(np.float32)
    S[0, 0, 0, 1] = 0
    return X, S


def _windows(frames, W):
    return [(t0, min(W, frames - t0)) for t0 in range(0, frames, W)]


def window_scales(X, B, C, W):
    """-> (B, frames): max |X| over the channels, bins and frames of the window the frame lies in"""
    X = np.asarray(X).reshape(B, C, *X.shape[-2:])
    out = np.zeros((B, X.shape[-1]))
    for b in range(B):
        for t0, n in _windows(X.shape[-1], W):
            out[b, t0:t0 + n] = np.abs(X[b, :, :, t0:t0 + n].astype(np.complex128)).max()
    return out


def initial(x, s, softmask, residual, trig=False):
    """x (C, bins, n) complex, s (J0, C, bins, n) real -> y (J, C, bins, n): step A"""
    f = s.dtype.type
    if softmask:
        y = x[None] * (s / (f(EPS) + s.sum(0, keepdims=True)))
    elif trig:
        ang = np.arctan2(x.imag, x.real)
        y = np.empty(s.shape, x.dtype)
        y.real, y.imag = s * np.cos(ang)[None], s * np.sin(ang)[None]
    else:
        mag = np.abs(x)
        ph = np.where(mag > 0, x / np.where(mag > 0, mag, 1), 1)
        y = s * ph[None]
    y = y.astype(x.dtype)
    if residual:
        acc = y[0].copy()
        for j in range(1, y.shape[0]):
            acc = acc + y[j]
        y = np.concatenate([y, (x - acc)[None]], 0)
    return y


def _inverse(M):
    """(..., C, C) -> its inverse in closed form: reciprocal (C = 1), adjugate / determinant (C = 2)"""
    one = M.real.dtype.type(1)
    if M.shape[-1] == 1:
        return one / M
    a, b, c, d = M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1]
    det = a * d - b * c
    inv = np.empty_like(M)
    inv[..., 0, 0], inv[..., 0, 1], inv[..., 1, 0], inv[..., 1, 1] = d, -b, -c, a
    return inv / det[..., None, None]


def em_step(x, y, sequential=False):
    """one iteration of step C.  x (C, bins, n), y (J, C, bins, n) -> the new y"""
    f = y.real.dtype.type
    J, C, bins, n = y.shape
    v = (y.real * y.real + y.imag * y.imag).sum(1) / f(C)                                   # (J, bins, n)
    outer = y[:, :, None] * np.conj(y[:, None, :])                                          # (J, C, C, bins, n)
    if sequential:
        Ryy, wgt = np.zeros(outer.shape[:-1], y.dtype), np.full((J, bins), f(EPS))
        for t in range(n):
            Ryy, wgt = Ryy + outer[..., t], wgt + v[..., t]
    else:
        Ryy, wgt = outer.sum(-1), f(EPS) + v.sum(-1)
    R = np.moveaxis(Ryy / wgt[:, None, None], (1, 2), (-2, -1))                             # (J, bins, C, C)
    Cxx = np.zeros((bins, n, C, C), y.dtype) + (f(np.sqrt(EPS)) * np.eye(C, dtype=f))
    for j in range(J):
        Cxx = Cxx + v[j][..., None, None] * R[j][:, None]
    inv = _inverse(Cxx)                                                                     # (bins, n, C, C)
    xv = np.moveaxis(x, 0, -1)                                                              # (bins, n, C)
    out = np.empty_like(y)
    for j in range(J):
        G = np.zeros_like(inv)
        for i1 in range(C):
            for i2 in range(C):
                for i3 in range(C):
                    G[..., i1, i2] = G[..., i1, i2] + R[j][:, None, i1, i3] * inv[..., i3, i2]
        G = G * v[j][..., None, None]
        yj = np.zeros((bins, n, C), y.dtype)
        for i in range(C):
            yj = yj + G[..., i] * xv[..., i, None]
        out[j] = np.moveaxis(yj, -1, 0)
    return out


def _wiener(X, S, B, C, W, niter, softmask, residual, ctype, trig, sequential):
    ftype = np.float64 if ctype is np.complex128 else np.float32
    bins, frames = X.shape[-2:]
    X = np.asarray(X).astype(ctype).reshape(B, C, bins, frames)
    S = np.asarray(S).astype(ftype).reshape(-1, B, C, bins, frames)
    J = S.shape[0] + bool(residual)
    if niter > 0 and J == 1:
        raise ValueError("expectation-maximisation needs more than one source")
    Y = np.zeros((B, J, C, bins, frames), ctype)
    for b in range(B):
        for t0, n in _windows(frames, W):
            x, s = X[b, :, :, t0:t0 + n], S[:, b, :, :, t0:t0 + n]
            y = initial(x, s, softmask, residual, trig)
            if niter > 0:
                m = max(ftype(1), np.abs(x).max() / ftype(10))
                x, y = x / m, y / m
                for _ in range(niter):
                    y = em_step(x, y, sequential)
                y = y * m
            assert y.dtype == ctype, y.dtype
            Y[b, ..., t0:t0 + n] = y
    return Y


def wiener64(X, S, B, C, W, niter=0, softmask=False, residual=False):
    return _wiener(X, S, B, C, W, niter, softmask, residual, np.complex128, False, False)


def wiener32(X, S, B, C, W, niter=0, softmask=False, residual=False):
    return _wiener(X, S, B, C, W, niter, softmask, residual, np.complex64, True, True)
