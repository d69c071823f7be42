"""fp64 closed forms of the framed FFT (remfx_amd/csrc/fft.hip, csrc/fft_any.hip) and of the STFT-loss cell arithmetic that sits on its
spectra, written from the contract of include/remfx_hip.h (the rfx_stft_desc block) and not from the kernels: frames of the padded
signal, a DFT, the layouts; the inverse transform, the window, the overlap-add and the adjoint of the padding.  forms_*() say which
kernel instantiation and which of its launch-time branches a descriptor reaches (mirrors of launch_fft, syn_own_geometry, batch_fast,
pair_loss_geometry and any_launch at the default RFX_FFT_OWN / RFX_FFT_OWN_FW / RFX_FFT_SYN_NB / RFX_FFT_ANA_NB, which the library
reads once per process), restate_*() are float32 evaluations of the same closed forms (the fp32-windowed frame through fft32, a
fixed-order float32 transform -- see its docstring for why not torch.fft --, fp32 overlap-add in ascending frame order; never a kernel)
that give the floors, and the *_CASES tables are what the CPU and the GPU test walk.

Bounds, eps32 = 2^-23; none is measured on a kernel.  Per element |got - ref| <= K eps32 magnitude, K = 8 floor + 8.
An FFT output's rounding error scales with its frame's norm, not with the output, so `magnitude` is a frame quantity:
  spectrum cell   |scale| ||w . mul . x_f||_2 of its frame (the l2 norm of the windowed samples), times 2 where herm doubles.
  synthesis       |scale mul[p]| sum_f |w[p - f hop]| rms(frame f's fp64 inverse transform), summed over the padded positions p that map
                  to the sample (mirror images included); under accum + half an ulp of |out0 + value|.
  mag/pow/magpow  the fp64 image of |X| +- sqrt(2) (cell bound) through the function, + one ulp of the result.  No cell is excluded.
  row sums        the sum of the cells' interval bounds + gamma_n sum |terms| for the fp32 partial sums + K eps32 times the first-order
                  magnitude of each term's own float32 evaluation (K = 8 FLOOR_TERMS + 8, a measured floor like the others: the issue's
                  two terms alone are unsound where the interval bounds are 0); the fp64 tail counts as nothing.
  loss gradient   the synthesis rule with rms(frame) replaced by sqrt(sum_k m_k^2), m_k = |ksc| (|X| + ymag) |X| / |X|c + |w_lm| |X| / |X|c^2
                  the first-order magnitude of the two terms of cell k (|X|c = the clamped magnitude): it bounds the rms of the
                  frame's inverse transform and carries the cells' own rounding through the (linear) transform."""
import functools
import math
import types

import numpy as np
import torch

from tests import fft_any_ref
from tests.ref_common import EPS32, f32  # noqa: F401

HALF = 2.0 ** -24
COMPLEX, CAC, MAG, POW, MAGPOW, FM = range(6)
MODE_NAMES = ("complex", "cac", "mag", "pow", "magpow", "complex_fm")
SPECTRUM_MODES = (COMPLEX, CAC, FM)
FFT_SIZES = (512, 1024, 2048, 4096)
EPS, ALPHA = 1e-8, 0.3
ANA_NB_MAX, SYN_NB_MAX, PAIR_NB_MAX = 4, 2, 4           # RFX_FFT_ANA_NB / RFX_FFT_SYN_NB defaults; the pair kernel's constant

# floors in units of eps32 x magnitude, measured on restate_* over the case tables (test_floors prints and recomputes them) and rounded
# up to the next quarter; K = 8 floor + 8.  One class per entry point and kernel file: the four sizes of fft.hip together, one class per
# n_fft decade of fft_any.hip.
# Measured: ana 7.4275 | 3.5864, 4.3059, 4.8818, 5.9398; syn 6.4670 | 2.9416, 4.3305, 5.2878, 6.4421
FLOOR = {"ana_fft": 7.5, "syn_fft": 6.5, "ana_any_1": 3.75, "syn_any_1": 3.0, "ana_any_2": 4.5, "syn_any_2": 4.5,
         "ana_any_3": 5.0, "syn_any_3": 5.5, "ana_any_4": 6.0, "syn_any_4": 6.5}


def k_of(name):
    return 8.0 * FLOOR[name] + 8.0


def klass(kind, n_fft):
    """the floor class of an entry point at n_fft: 'ana' / 'syn' + the kernel file (fft_any: the decade of n_fft)"""
    if n_fft in FFT_SIZES:
        return kind + "_fft"
    return f"{kind}_any_{len(str(n_fft)) - 1}"


# ---- descriptor --------------------------------------------------------------------------------------------------------------------
FIELDS = ("R", "T", "n_fft", "hop", "win", "bins", "frame0", "frames_out", "mode", "extra_pad_l", "extra_pad_r", "in_mode", "in_offset",
          "herm", "scale", "eps", "alpha", "accum")


def desc(R, T, n_fft, hop, win, bins=None, frame0=0, frames_out=None, mode=COMPLEX, pads=(0, 0), in_mode=0, in_offset=0, herm=0,
         scale=1.0, eps=0.0, alpha=1.0, accum=0):
    """the fields of rfx_stft_desc; frames_out defaults to every frame of torch.stft(center=True) from frame0 on"""
    if frames_out is None:
        frames_out = 1 + (T + pads[0] + pads[1]) // hop - frame0
    return types.SimpleNamespace(R=R, T=T, n_fft=n_fft, hop=hop, win=win, bins=n_fft // 2 + 1 if bins is None else bins, frame0=frame0,
                                 frames_out=frames_out, mode=mode, extra_pad_l=pads[0], extra_pad_r=pads[1], in_mode=in_mode,
                                 in_offset=in_offset, herm=herm, scale=f32(scale), eps=f32(eps), alpha=f32(alpha), accum=accum)


def with_(d, **kw):
    out = types.SimpleNamespace(**vars(d))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def padded_len(d):
    """padded positions the stored frames touch: [0, padded_len)"""
    return (d.frame0 + d.frames_out - 1) * d.hop + d.n_fft


def map_sample(d, p):
    """padded position (int64 tensor) -> sample index of the row, -1 where the position holds a zero.  in_mode 0: the extra reflect pads
    are applied first, then the centre pad of n_fft / 2; a position whose double reflection leaves the row counts as zero."""
    if d.in_mode == 0:
        Tp = d.T + d.extra_pad_l + d.extra_pad_r
        s = (p - d.n_fft // 2).abs()
        s = torch.where(s >= Tp, 2 * (Tp - 1) - s, s)
        s = (s - d.extra_pad_l).abs()
        s = torch.where(s >= d.T, 2 * (d.T - 1) - s, s)
    else:
        s = p - d.in_offset
    return torch.where((s >= 0) & (s < d.T), s, torch.full_like(s, -1))


def full_window(d, window):
    """the win-sample window centred at (n_fft - win) // 2 of an n_fft frame"""
    w = torch.zeros(d.n_fft, dtype=window.dtype)
    woff = (d.n_fft - d.win) // 2
    w[woff:woff + d.win] = window
    return w


def hann(win):
    return torch.hann_window(win, dtype=torch.float64).float()


def inv_envelope(d, window, frames, dtype=torch.float32):
    """1 / sum_f w^2[p - f hop] over the padded positions of `frames` frames (torch.istft's envelope), as float32 (what the kernel reads)"""
    w = full_window(d, window.double())
    env = torch.zeros((frames - 1) * d.hop + d.n_fft, dtype=torch.float64)
    for f in range(frames):
        env[f * d.hop:f * d.hop + d.n_fft] += w * w
    return torch.where(env > 1e-11, 1.0 / env, torch.zeros_like(env)).to(dtype)


# ---- analysis ----------------------------------------------------------------------------------------------------------------------
def _frame_positions(d):
    return (d.frame0 + torch.arange(d.frames_out))[:, None] * d.hop + torch.arange(d.n_fft)[None, :]          # (F, N)


def windowed_frames(d, x, window, mul=None, rows=None):
    """(rows, F, N): scale w[t] mul[p] xpad[p] at p = f hop + t of the stored frames, in x's dtype arithmetic (fp64 for the reference)"""
    p = _frame_positions(d)
    s = map_sample(d, p)
    xr = x if rows is None else x[rows]
    fr = xr[:, s.clamp_min(0)] * (s >= 0).to(x.dtype)
    fr = fr * full_window(d, window.to(x.dtype))[None, None, :]
    fr = fr * torch.tensor(d.scale, dtype=x.dtype)
    if mul is not None:
        fr = fr * mul.to(x.dtype)[p][None]
    return fr


def _dft(fr, bins):
    """X[k] = sum_t fr[t] e^{-2 pi i k t / N}, k < bins: a direct DFT matrix product for a few bins, torch.fft.rfft otherwise"""
    N = fr.shape[-1]
    if bins > 16 or fr.dtype != torch.float64:
        return torch.fft.rfft(fr, dim=-1)[..., :bins]
    kt = (torch.arange(bins)[None, :] * torch.arange(N)[:, None]) % N
    ang = kt.double() * (-2.0 * math.pi / N)
    return torch.complex(fr @ torch.cos(ang), fr @ torch.sin(ang))


def _herm_weights(d):
    k = torch.arange(d.bins)
    return torch.where((k == 0) | (k == d.n_fft // 2), 1.0, 2.0).double()


def spectrum(d, x, window, mul=None, chunk=8):
    """-> X complex (R, F, bins) and the cells' magnitude (R, F, bins) = the l2 norm of the frame's windowed samples (x 2 where herm
    doubles).  herm: middle bins doubled, the imaginary parts of DC and Nyquist dropped."""
    xs, ms = [], []
    mul64 = None if mul is None else mul.double()
    for r0 in range(0, d.R, chunk):
        fr = windowed_frames(d, x.double(), window.double(), mul64, slice(r0, min(r0 + chunk, d.R)))
        xs.append(_dft(fr, d.bins))
        ms.append(fr.pow(2).sum(-1).sqrt())
    X, nrm = torch.cat(xs), torch.cat(ms)
    mag = nrm[..., None].expand(-1, -1, d.bins)
    if d.herm:
        hw = _herm_weights(d)
        real_only = (hw == 1.0)
        X = torch.complex(X.real * hw, torch.where(real_only, torch.zeros_like(X.imag), X.imag * hw))
        mag = mag * hw
    return X, mag.contiguous()


def mode_value(d, m):
    """the mag / pow / magpow value of a cell of modulus m (fp64), with the descriptor's float32 eps and alpha"""
    if d.mode == MAG:
        return torch.sqrt(torch.clamp(m * m, min=d.eps))
    if d.mode == POW:
        return m * m
    return (m + d.eps) ** d.alpha


def to_layout(d, X):
    """complex (R, F, bins) -> the tensor the output mode stores"""
    if d.mode == COMPLEX:
        return torch.view_as_real(X.permute(0, 2, 1).contiguous())
    if d.mode == CAC:
        Xt = X.permute(0, 2, 1)
        return torch.stack((Xt.real, Xt.imag), 1).contiguous()
    if d.mode == FM:
        return torch.view_as_real(X.contiguous())
    return mode_value(d, X.abs()).permute(0, 2, 1).contiguous()


def real_to_layout(d, b):
    """a real per-cell quantity (R, F, bins) -> the layout of the mode (the same for the real and the imaginary part)"""
    if d.mode == COMPLEX:
        return b.permute(0, 2, 1)[..., None].expand(-1, -1, -1, 2).contiguous()
    if d.mode == CAC:
        return b.permute(0, 2, 1)[:, None].expand(-1, 2, -1, -1).contiguous()
    if d.mode == FM:
        return b[..., None].expand(-1, -1, -1, 2).contiguous()
    return b.permute(0, 2, 1).contiguous()


def from_layout(d, t):
    """a stored spectrum (COMPLEX, CAC or FM) -> complex (R, F, bins)"""
    t = t.reshape(layout_shape(d))
    if d.mode == COMPLEX:
        return torch.complex(t[..., 0], t[..., 1]).permute(0, 2, 1)
    if d.mode == CAC:
        return torch.complex(t[:, 0], t[:, 1]).permute(0, 2, 1)
    return torch.complex(t[..., 0], t[..., 1])


def layout_shape(d):
    return {COMPLEX: (d.R, d.bins, d.frames_out, 2), CAC: (d.R, 2, d.bins, d.frames_out), FM: (d.R, d.frames_out, d.bins, 2)}.get(
        d.mode, (d.R, d.bins, d.frames_out))


def cell_index(d, j):
    """flat element j of an analysis output -> 'row r frame f bin k (re / im)' for the failure message"""
    shape = layout_shape(d)
    idx = np.unravel_index(j, shape)
    if d.mode == COMPLEX:
        r, k, f, c = idx
    elif d.mode == CAC:
        r, c, k, f = idx
    elif d.mode == FM:
        r, f, k, c = idx
    else:
        (r, k, f), c = idx, 0
    return f"row {int(r)} frame {int(f) + d.frame0} bin {int(k)} {'im' if c else 're'}"


def analysis(d, x, window, mul=None):
    """rfx_fft_analysis in fp64 -> (output in the mode's layout, per-element bound)"""
    X, mag = spectrum(d, x, window, mul)
    return to_layout(d, X), analysis_bound(d, X, mag)


def analysis_bound(d, X, mag):
    b = k_of(klass("ana", d.n_fft)) * EPS32 * mag
    if d.mode in SPECTRUM_MODES:
        return real_to_layout(d, b)
    return real_to_layout(d, interval_bound(lambda m: mode_value(d, m), X.abs(), math.sqrt(2.0) * b))


def interval_bound(fn, m, bm):
    """the image of [max(m - bm, 0), m + bm] through a non-decreasing fn, as a distance from fn(m), + one ulp of fn(m)"""
    v = fn(m)
    return torch.maximum(fn(m + bm) - v, v - fn((m - bm).clamp_min(0.0))) + EPS32 * v.abs()


def fft32(re, im):
    """forward DFT over the last axis in float32: an iterative radix-2 decimation-in-time transform whose every product and sum is one
    IEEE float32 operation on arrays (twiddles rounded from fp64), so the floors are the same figures on every host.  torch.fft in
    float32 is not: its library picks a code path by the host's instruction set, and the floors measured through it moved by up to
    30 % between the AVX-512, AVX2 and SSE4.2 paths of one machine."""
    f = np.float32
    re, im = np.ascontiguousarray(re, f), np.ascontiguousarray(im, f)
    lead, N = re.shape[:-1], re.shape[-1]
    bits = N.bit_length() - 1
    idx = np.arange(N)
    rev = np.zeros(N, np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    re, im = re.reshape(-1, N)[:, rev], im.reshape(-1, N)[:, rev]
    M, size = re.shape[0], 2
    while size <= N:
        half = size // 2
        ang = -2.0 * math.pi * np.arange(half) / size
        wr, wi = np.cos(ang).astype(f), np.sin(ang).astype(f)
        re, im = re.reshape(M, N // size, 2, half), im.reshape(M, N // size, 2, half)
        ar, ai, br, bi = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
        tr, ti = br * wr - bi * wi, br * wi + bi * wr
        re, im = np.stack((ar + tr, ar - tr), 2).reshape(M, N), np.stack((ai + ti, ai - ti), 2).reshape(M, N)
        size *= 2
    return re.reshape(lead + (N,)), im.reshape(lead + (N,))


def restate_analysis(d, x, window, mul=None):
    """float32 restatement: the fp32-windowed frame (x w, scale, mul: one rounding each) through fft32 -> complex64 (R, F, bins)"""
    fr = windowed_frames(d, x.float(), window.float(), None if mul is None else mul.float())
    re, im = fft32(fr.numpy(), np.zeros_like(fr.numpy()))
    X = torch.complex(torch.from_numpy(re[..., :d.bins].copy()), torch.from_numpy(im[..., :d.bins].copy()))
    if d.herm:
        hw = _herm_weights(d).float()
        X = torch.complex(X.real * hw, torch.where(hw == 1.0, torch.zeros_like(X.imag), X.imag * hw))
    return X


def floor_of(got, ref, mag):
    """the largest |got - ref| / (eps32 magnitude) over the elements with a magnitude"""
    e = (got.double() - ref.double()).abs()
    ok = mag > 0
    assert bool((e[~ok] == 0).all())
    return float((e[ok] / (EPS32 * mag[ok])).max()) if bool(ok.any()) else 0.0


# ---- synthesis ---------------------------------------------------------------------------------------------------------------------
def _half_spectrum(d, S):
    """stored bins -> the n_fft / 2 + 1 bins the inverse real transform takes: a missing Nyquist bin is zero, the imaginary parts of DC
    and Nyquist are ignored, herm = 0 halves the middle bins (the adjoint of the one-sided rfft)"""
    NH = d.n_fft // 2 + 1
    H = torch.zeros(S.shape[:-1] + (NH,), dtype=S.dtype)
    H[..., :d.bins] = S
    k = torch.arange(NH)
    edge = (k == 0) | (k == NH - 1)
    im = torch.where(edge, torch.zeros_like(H.imag), H.imag)
    H = torch.complex(H.real, im)
    if not d.herm:
        H = H * torch.where(edge, 1.0, 0.5).to(H.real.dtype)
    return H


def inverse_frames(d, S):
    """(R, F, N): y[t] = Re X[0] + (-1)^t Re X[N/2] + 2 sum_mid Re(X[k] e^{2 pi i k t / N}) of the half spectrum (irfft x N)"""
    return torch.fft.irfft(_half_spectrum(d, S), n=d.n_fft, dim=-1) * d.n_fft


def _overlap_add(d, y):
    """(R, F, N) -> (R, padded_len): sum of the frames at p = f hop + t, ascending f"""
    pad = torch.zeros(y.shape[0], padded_len(d), dtype=y.dtype)
    for j in range(d.frames_out):
        p0 = (d.frame0 + j) * d.hop
        pad[:, p0:p0 + d.n_fft] += y[:, j]
    return pad


def _fold(d, pad):
    """adjoint of map_sample: out[s] = sum of pad[p] over the padded positions p that map to s (ascending p)"""
    s = map_sample(d, torch.arange(pad.shape[1]))
    p = torch.nonzero(s >= 0)[:, 0]
    order = torch.argsort(s[p], stable=True)                       # by sample, ascending p within a sample
    p, sp = p[order], s[p][order]
    first = torch.cat((torch.ones(1, dtype=torch.bool), sp[1:] != sp[:-1]))
    start = torch.cummax(torch.where(first, torch.arange(sp.numel()), torch.zeros_like(sp)), 0)[0]
    rank = torch.arange(sp.numel()) - start
    out = torch.zeros(pad.shape[0], d.T, dtype=pad.dtype)
    for r in range(int(rank.max()) + 1 if rank.numel() else 0):      # one add per sample and round: the same order on every host
        m = rank == r
        out[:, sp[m]] += pad[:, p[m]]
    return out


def synthesis(d, spec, window, mul=None, out0=None):
    """rfx_fft_synthesis in fp64: spec complex (R, F, bins) -> (out (R, T), bound).  Samples no stored frame covers are exactly 0 (or
    out0 unchanged under accum: their bound is 0)."""
    y = inverse_frames(d, spec.to(torch.complex128))
    return _synthesis_tail(d, y, y.pow(2).mean(-1).sqrt(), window, mul, out0)


def _synthesis_tail(d, y, frame_rms, window, mul, out0):
    w = full_window(d, window.double())
    m = torch.tensor(d.scale, dtype=torch.float64) * (torch.ones(padded_len(d), dtype=torch.float64) if mul is None else mul.double()[:padded_len(d)])
    out = _fold(d, _overlap_add(d, y * w) * m)
    mag = _fold(d, _overlap_add(d, frame_rms[..., None] * w.abs()) * m.abs())
    bound = k_of(klass("syn", d.n_fft)) * EPS32 * mag
    if d.accum:
        out = out + out0.double()
        bound = torch.where(mag > 0, bound + HALF * out.abs(), bound)
    return out, bound


def restate_synthesis(d, spec, window, mul=None):
    """float32 restatement: the Hermitian extension of the half spectrum through fft32 (the inverse is the forward transform of the
    conjugate), the fp32 window, fp32 overlap-add in ascending frame order, scale, mul, the fold"""
    H = _half_spectrum(d, spec.to(torch.complex64))
    full = torch.cat((H, H[..., 1:-1].flip(-1).conj()), -1)
    re, _ = fft32(full.real.numpy(), (-full.imag).numpy())
    y = torch.from_numpy(re) * full_window(d, window.float())
    pad = _overlap_add(d, y) * torch.tensor(d.scale, dtype=torch.float32)
    if mul is not None:
        pad = pad * mul.float()[:pad.shape[1]]
    return _fold(d, pad)


# ---- STFT-loss cells ---------------------------------------------------------------------------------------------------------------
def clamped_mag(X, eps):
    return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=f32(eps)))


def loss_sums(X, Y, eps):
    """complex (R, ...) spectra -> (R, 3): sum (|Y| - |X|)^2, sum |Y|^2, sum |log|X| - log|Y|| on clamped powers"""
    return loss_sums_m(clamped_mag(X.to(torch.complex128), eps), clamped_mag(Y.to(torch.complex128), eps))


def loss_sums_m(xm, ym):
    R = xm.shape[0]
    xm, ym = xm.reshape(R, -1), ym.reshape(R, -1)
    return torch.stack((((ym - xm) ** 2).sum(1), (ym * ym).sum(1), (xm.log() - ym.log()).abs().sum(1)), 1)


def loss_sums_bound(X, Y, bx, by, eps, group=8):
    """bound of the three row sums when the spectra's cells carry the per-component bounds bx, by (0: the stored fp32 values are the
    inputs): the cells' interval bounds + gamma_n sum |terms| for fp32 partial sums of `group` cells + the float32 evaluation of the
    terms themselves, K eps32 times their first-order magnitude (loss_term_magnitudes) with K = 8 FLOOR_TERMS + 8: without it the
    bound is unsound where the interval bounds are 0"""
    R = X.shape[0]
    e = f32(eps)
    mx, my = X.abs().reshape(R, -1), Y.abs().reshape(R, -1)
    bx, by = math.sqrt(2.0) * bx.reshape(R, -1), math.sqrt(2.0) * by.reshape(R, -1)
    cm = lambda m: torch.sqrt(torch.clamp(m * m, min=e))                                    # noqa: E731
    xlo, xhi, ylo, yhi = cm((mx - bx).clamp_min(0)), cm(mx + bx), cm((my - by).clamp_min(0)), cm(my + by)
    xm, ym = cm(mx), cm(my)
    dmax = torch.maximum((yhi - xlo).abs(), (ylo - xhi).abs())
    t0 = (ym - xm) ** 2
    b0 = torch.maximum(dmax ** 2 - t0, t0 - torch.where((ylo <= xhi) & (xlo <= yhi), torch.zeros_like(t0), torch.minimum((ylo - xhi).abs(), (xlo - yhi).abs()) ** 2))
    b1 = yhi ** 2 - ylo ** 2
    t2 = (xm.log() - ym.log()).abs()
    b2 = (xhi.log() - xlo.log()) + (yhi.log() - ylo.log())
    terms = torch.stack((t0, ym * ym, t2), 0)
    cells = torch.stack((b0, b1, b2), 0)
    own = k_terms() * EPS32 * torch.stack(loss_term_magnitudes(xm, ym), 0)
    gamma = group * HALF
    return (cells.sum(2) + own.sum(2) + gamma * terms.sum(2)).t().contiguous()


FLOOR_TERMS = 1.0                 # measured 0.9621 on restate_loss_terms over CELL_N x CELL_R (test_floors), next quarter


def k_terms():
    return 8.0 * FLOOR_TERMS + 8.0


def loss_term_magnitudes(xm, ym):
    """first-order magnitude of the float32 evaluation of the three terms when |X|, |Y| carry a relative rounding: d = |Y| - |X| moves by
    eps (|X| + |Y|), so d^2 by 2 |d| (|X| + |Y|) eps (+ its own rounding); |Y|^2 by its own; a log of a power by eps (the power's
    rounding, derivative 1) + eps |log|: (log px - log py) / 2 by eps (1 + |ln |X|| + |ln |Y||)"""
    d = (ym - xm).abs()
    return 2.0 * d * (xm + ym) + d * d, ym * ym, 1.0 + xm.log().abs() + ym.log().abs()


def restate_loss_terms(X, Y, eps):
    """the three terms per cell in float32, one rounding per operation (numpy; the log is the fp64 log rounded once, so that the figure
    does not depend on a host's float32 log) -> (3, R, n) float32"""
    f = np.float32
    out = []
    p = []
    for Z in (X, Y):
        re, im = Z.real.numpy().astype(f), Z.imag.numpy().astype(f)
        p.append(np.maximum(im * im + re * re, f(eps)))
    px, py = p
    d = np.sqrt(py) - np.sqrt(px)
    lg = lambda v: np.log(v.astype(np.float64)).astype(f)                                     # noqa: E731
    out = (d * d, py, np.abs(lg(px) - lg(py)) * f(0.5))
    return torch.from_numpy(np.stack(out, 0))


def measure_terms_floor():
    worst = 0.0
    for R in CELL_R:
        for n in CELL_N:
            X, Y, _, _ = cell_inputs(R, n, 100 * R + n)
            xm, ym = clamped_mag(X.to(torch.complex128), CELL_EPS), clamped_mag(Y.to(torch.complex128), CELL_EPS)
            ref = torch.stack(((ym - xm) ** 2, ym * ym, (xm.log() - ym.log()).abs()), 0)
            worst = max(worst, floor_of(restate_loss_terms(X, Y, CELL_EPS), ref, torch.stack(loss_term_magnitudes(xm, ym), 0)))
    return worst


def lossgrad_cells(xspec, ymag, sums, w_sc, w_lm, eps, gup=None):
    """d [w_sc sqrt(A) / sqrt(B) + w_lm sum |log|X| - log|Y||] / dX per cell, as a function of the fp32 values the forward stored:
    xspec complex (R, ...), ymag (R, ...) clamped target magnitudes, sums (R, 3).  ksc = w_sc gup / (sqrt(A) sqrt(B)), 0 unless A > 0 and
    B > 0; the weights are the float32 products w gup the ABI forms; no gradient at or below eps; the sign of the log term from
    |X| - ymag.  -> (gradient complex128, first-order magnitude per cell)"""
    R = xspec.shape[0]
    X = xspec.to(torch.complex128)
    ym = ymag.double()
    wsc, wlm = np.float32(w_sc), np.float32(w_lm)
    if gup is not None:
        wsc, wlm = wsc * np.float32(gup), wlm * np.float32(gup)
    A, B = sums[:, 0].double(), sums[:, 1].double()
    ok = (A > 0) & (B > 0)
    ksc = torch.where(ok, float(wsc) / (A.clamp_min(1e-300).sqrt() * B.clamp_min(1e-300).sqrt()), torch.zeros_like(A))
    ksc = ksc.reshape((R,) + (1,) * (X.dim() - 1))
    px = X.real ** 2 + X.imag ** 2
    e = f32(eps)
    xm = torch.sqrt(torch.clamp(px, min=e))
    sc = (ksc * (xm - ym) + float(wlm) * torch.sign(xm - ym) / xm) / xm
    live = px > e
    sc = torch.where(live, sc, torch.zeros_like(sc))
    mag = torch.where(live, (ksc.abs() * (xm + ym) + abs(float(wlm)) / xm) * X.abs() / xm, torch.zeros_like(xm))
    return sc * X, mag


def synthesis_lossgrad(d, xspec, ymag, sums, w_sc, w_lm, eps, gup, window, out0=None):
    """rfx_fft_synthesis_lossgrad: lossgrad_cells through synthesis (in_mode 0, herm 0, frame-major); the frames' magnitude is
    sqrt(sum_k m_k^2) of the cells' first-order magnitudes"""
    G, m = lossgrad_cells(xspec, ymag, sums, w_sc, w_lm, eps, gup)
    y = inverse_frames(d, G)
    return _synthesis_tail(d, y, m.pow(2).sum(-1).sqrt(), window, None, out0)


def stft_loss_grad(xc, yc, sums, w_sc, w_lm, eps, gup=None):
    """the two-spectrum form (rfx_stft_loss_grad): the target's clamped magnitude comes from its spectrum"""
    return lossgrad_cells(xc, clamped_mag(yc.to(torch.complex128), eps), sums, w_sc, w_lm, eps, gup)


def pair_loss(d, x, y, window, eps):
    """rfx_stft_pair_loss: analysis of both signals (frame-major, every bin, scale 1), the three row sums, the prediction's spectrum and
    the target's clamped magnitudes -> dict(sums, xspec, ymag, and their bounds)"""
    dd = with_(d, mode=FM, scale=1.0)
    X, magx = spectrum(dd, x, window)
    Y, magy = spectrum(dd, y, window)
    bx, by = k_of("ana_fft") * EPS32 * magx, k_of("ana_fft") * EPS32 * magy
    e = f32(eps)
    ym = clamped_mag(Y, e)
    # a thread adds its items of one batch in fp32 (9 cells of each of the two frames of a pair: 18 terms), everything beyond in fp64
    return dict(sums=loss_sums(X, Y, e), sums_bound=loss_sums_bound(X, Y, bx, by, e, group=18), xspec=torch.view_as_real(X.contiguous()), xspec_bound=real_to_layout(dd, bx),
                ymag=ym, ymag_bound=interval_bound(lambda m: torch.sqrt(torch.clamp(m * m, min=e)), Y.abs(), math.sqrt(2.0) * by), X=X, Y=Y)


def ulp32(v):
    """the spacing of float32 at |v| (tensor, fp64)"""
    a = v.double().abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def band_cells(xspec, ymag, eps):
    """cells inside the sign band (||X| - ymag| <= 4 ulp) or the eps band (|px - eps| <= 4 ulp(eps)): where the fp32 and the fp64
    evaluation may legitimately take different branches"""
    X = xspec.to(torch.complex128)
    px = X.real ** 2 + X.imag ** 2
    e = f32(eps)
    xm = torch.sqrt(torch.clamp(px, min=e))
    return ((xm - ymag.double()).abs() <= 4 * ulp32(xm)) | ((px - e).abs() <= 4 * float(ulp32(torch.tensor(e))))


# ---- the cell kernels of losses.hip: rfx_stft_loss_reduce, rfx_stft_loss_grad, rfx_stft_loss_grad_m ---------------------------------
CELL_EPS = 2.0 ** -26             # a power of two near auraloss' 1e-8, so that |X|^2 == eps, one step below and one ulp above are float32 cells
CELL_N = (1, 255, 256, 2049, 40001)          # 2049 = 8 x 256 x grid + 1 at grid = 1: the unroll-by-eight tail and the clamped index at n - 1
CELL_R = (1, 3)
REDUCE_SLOTS = 64
# designated cells, columns 8 .. 14 of every row from n = 255 on: every one is exact in float32 and in fp64 alike
DESIGNATED = ("x_zero", "below_eps", "at_eps", "above_eps", "sign_zero", "ymag_one_ulp_above", "ymag_one_ulp_below")
DESIGNATED_COL = 8
FLOOR_CELL = 2.75                 # measured 2.5819 on restate_lossgrad_cells over CELL_N x CELL_R (test_floors), next quarter


def k_cell():
    return 8.0 * FLOOR_CELL + 8.0


def cell_inputs(R, n, seed):
    """-> X, Y complex64 (R, n), ymag float32 (R, n) = the clamped |Y| rounded once, sums float32 (R, 3).  |X| spreads over 0.01 .. 10,
    |Y| is |X| times a factor away from 1; the last row of R = 3 has A = 0"""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(R, n, generator=g, dtype=torch.float64)                        # noqa: E731
    X = torch.polar(10.0 ** (r() * 3.0 - 2.0), 2.0 * math.pi * r()).to(torch.complex64)
    f = 1.0 + (0.05 + 0.5 * r()) * torch.where(r() < 0.5, -1.0, 1.0)
    Y = torch.polar(X.abs().double() * f, 2.0 * math.pi * r()).to(torch.complex64)
    ymag = clamped_mag(Y.to(torch.complex128), CELL_EPS).float()
    if n >= 255:
        c, h = DESIGNATED_COL, np.float32(2.0 ** -13)
        X[:, c], Y[:, c + 0] = 0, 0.5
        X[:, c + 1] = float(np.nextafter(h, np.float32(0)))
        X[:, c + 2] = float(h)
        X[:, c + 3] = complex(float(h), f32(2.0 ** -24.5))
        Y[:, c + 1:c + 4] = 0.5
        ymag[:, c:c + 4] = 0.5
        X[:, c + 4:c + 7] = 0.375 + 0.5j                                                  # |X| = 0.625 exactly, in float32 too
        m = np.float32(0.625)
        for j, v in enumerate((m, np.nextafter(m, np.float32(1)), np.nextafter(m, np.float32(0)))):
            Y[:, c + 4 + j], ymag[:, c + 4 + j] = float(v), float(v)
    sums = torch.stack((0.5 + torch.rand(R, generator=g), 2.0 + torch.rand(R, generator=g), torch.rand(R, generator=g)), 1).float()
    if R == 3:
        sums[2, 0] = 0.0
    return X, Y, ymag, sums


def designated_mask(n):
    m = torch.zeros(n, dtype=torch.bool)
    if n >= 255:
        m[DESIGNATED_COL:DESIGNATED_COL + len(DESIGNATED)] = True
    return m


def restate_lossgrad_cells(xspec, ymag, sums, w_sc, w_lm, eps, gup=None):
    """the cell formula in float32, one rounding per operation (numpy: sqrt and division correctly rounded)"""
    f = np.float32
    re, im, ym = xspec.real.numpy().astype(f), xspec.imag.numpy().astype(f), ymag.numpy().astype(f)
    wsc, wlm = f(w_sc), f(w_lm)
    if gup is not None:
        wsc, wlm = wsc * f(gup), wlm * f(gup)
    A, B = sums[:, 0].numpy().astype(f), sums[:, 1].numpy().astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        ksc = np.where((A > 0) & (B > 0), wsc / (np.sqrt(A) * np.sqrt(B)), f(0)).astype(f)[:, None]
    px = im * im + re * re
    xm = np.sqrt(np.maximum(px, f(eps)))
    dm = ksc * (xm - ym) + wlm * np.sign(xm - ym).astype(f) / xm
    live = px > f(eps)
    return torch.complex(torch.from_numpy(np.where(live, dm * re / xm, f(0))), torch.from_numpy(np.where(live, dm * im / xm, f(0))))


def measure_cell_floor():
    worst = 0.0
    for R in CELL_R:
        for n in CELL_N:
            X, _, ymag, sums = cell_inputs(R, n, 100 * R + n)
            for gup in (None, 1.7):
                G, mag = lossgrad_cells(X, ymag, sums, LG_W_SC, LG_W_LM, CELL_EPS, gup)
                g32 = restate_lossgrad_cells(X, ymag, sums, LG_W_SC, LG_W_LM, CELL_EPS, gup)
                worst = max(worst, floor_of(g32.real, G.real, mag), floor_of(g32.imag, G.imag, mag))
    return worst


def forms_cells(n, kernel, gup=False):
    """losses.hip: grid_red / grid_x and the loops' tails"""
    if kernel == "reduce":
        g = min(max(-(-n // 16384), 1), REDUCE_SLOTS)
        out = {"stft_loss_reduce_kernel:" + ("one_slot" if g == 1 else "slots")}
        if n % (8 * 256 * g):
            out.add("stft_loss_reduce_kernel:clamped_tail")
        if n > 8 * 256 * g:
            out.add("stft_loss_reduce_kernel:second_iteration")
        if n < 256:
            out.add("stft_loss_reduce_kernel:idle_lanes")
        return out
    g = min(max(-(-n // 2048), 1), 512)
    out = {f"stft_loss_grad_kernel:{kernel}", "stft_loss_grad_kernel:" + ("gup" if gup else "no_gup")}
    if n > g * 256:
        out.add("stft_loss_grad_kernel:second_iteration")
    return out


# ---- forms: fft.hip ----------------------------------------------------------------------------------------------------------------
def _fb(n_fft):
    return 4096 // (n_fft // 2)


def _nb(d, syn):
    """frame batches a workgroup walks (launch_fft): only the frame-major layout, while the grid stays at 4096 workgroups"""
    batches, rows8 = -(-d.frames_out // _fb(d.n_fft)), -(-d.R // 8)
    nb = 1
    if d.mode == FM:
        while nb < (SYN_NB_MAX if syn else ANA_NB_MAX) and rows8 * 8 * (-(-batches // (2 * nb))) >= 4096:
            nb *= 2
    return nb


def batch_fast(d, row, fb0, x_misaligned):
    """batch_fast of fft_analysis_kernel: every frame of the batch inside the signal, even hop, an 8-byte-aligned first pair"""
    FB, N = _fb(d.n_fft), d.n_fft
    shift = d.n_fft // 2 + d.extra_pad_l if d.in_mode == 0 else d.in_offset
    pb0, f_end = fb0 * d.hop, d.frame0 + d.frames_out
    return (fb0 + FB <= f_end and pb0 - shift >= 0 and pb0 + (FB - 1) * d.hop + N - 1 - shift < d.T and d.hop % 2 == 0
            and (row * d.T + pb0 - shift) % 2 == 0 and not x_misaligned)


def forms_analysis(d, x_misaligned=False, mul=False):
    """fft.hip: instantiation and output mode, the load paths its batches take, nb, and the descriptor branches"""
    if d.n_fft not in FFT_SIZES:
        return forms_any(d, False, mul)
    FB, nb, f_end = _fb(d.n_fft), _nb(d, False), d.frame0 + d.frames_out
    out = {f"fft_analysis_kernel<{d.n_fft}>:{MODE_NAMES[d.mode]}", f"fft_analysis_kernel:nb{nb}"}
    per_row = []
    for row in range(d.R):
        paths = set()
        for f_first in range(d.frame0, f_end, FB * nb):
            fast = batch_fast(d, row, f_first, x_misaligned)
            for g in range(nb):
                fb0 = f_first + g * FB
                if fb0 >= f_end:
                    break
                paths.add("fast" if fast else "mapped")
                left = fb0 * d.hop < (d.n_fft // 2 + d.extra_pad_l if d.in_mode == 0 else d.in_offset)
                if not fast and d.hop % 2 == 0 and not x_misaligned:
                    paths.add("edge_left" if left else ("ragged" if fb0 + FB > f_end else "edge_right_or_odd_row"))
                if fast and g > 0:
                    out.add("fft_analysis_kernel:fast_batch_prefetched_over_epilogue")
                nxt = g + 1 < nb and fb0 + FB < f_end
                was = fast
                fast = nxt and batch_fast(d, row, fb0 + FB, x_misaligned)
                if nxt and was and not fast:
                    out.add("fft_analysis_kernel:fast_then_mapped_in_one_walk")
                if nxt and not was and fast:
                    out.add("fft_analysis_kernel:mapped_then_fast_in_one_walk")
        per_row.append(frozenset(p for p in paths if p in ("fast", "mapped")))
        out.update("fft_analysis_kernel:" + ("load_" + p if p in ("fast", "mapped") else p + "_batch") for p in paths)
    if len(set(per_row)) > 1:
        out.add("fft_analysis_kernel:rows_take_different_paths")
    if x_misaligned:
        out.add("fft_analysis_kernel:x_misaligned")
    if d.hop % 2:
        out.add("fft_analysis_kernel:odd_hop")
    if mul:
        out.update("fft_analysis_kernel:mul_" + p for p in set().union(*per_row))
    out |= _desc_forms("fft_analysis_kernel", d)
    return out


def _desc_forms(k, d):
    out = set()
    if d.herm:
        out.add(k + ":herm")
    if d.in_mode:
        out.add(k + ":in_mode1")
    if d.extra_pad_l or d.extra_pad_r:
        out.add(k + ":extra_pads")
    if d.R % 8:
        out.add(k + ":partial_row_group")
    if d.R > 8:
        out.add(k + ":second_row_group")
    if d.bins < d.n_fft // 2 + 1:
        out.add(k + (":no_nyquist" if d.bins == d.n_fft // 2 else ":few_bins"))
    if d.frame0:
        out.add(k + ":frame0")
    if d.frames_out % _fb(d.n_fft) if d.n_fft in FFT_SIZES else 0:
        out.add(k + ":ragged_last_batch")
    if d.win < d.n_fft:
        out.add(k + ":win_short")
    if (d.n_fft - d.win) % 2:
        out.add(k + ":odd_window_offset")
    return out


def syn_own_geometry(d):
    """syn_own_geometry at RFX_FFT_OWN = 1, RFX_FFT_OWN_FW unset -> (walk_frames, halo, nwalks, ws_floats); nwalks 0: the atomic form"""
    woff, nc = (d.n_fft - d.win) // 2, d.n_fft // 2
    fb = 4096 // nc
    own = d.hop <= d.win and (d.in_mode == 1 or (not d.extra_pad_l and not d.extra_pad_r and d.frame0 == 0 and d.T > 2 * d.n_fft + 2))
    if not own:
        return 0, 0, 0, 0
    halo = (d.win - 1) // d.hop
    fw_min = halo + 1
    if d.in_mode == 0:
        fw_min = max(fw_min, (d.n_fft + 1 - woff + d.hop - 1) // d.hop + 1, 2 + (woff + d.hop) // d.hop)
    fw_min = max(fw_min, 2 * halo)
    fw = (d.frames_out * d.R + 2047) // 2048
    fw = min(fw, max(16 * halo, 4 * fb))
    fw = max(fw, fw_min)
    fw = -(-fw // fb) * fb
    nwalks = max(1, d.frames_out // fw)
    grid = -(-d.R // 8) * nwalks * 8
    return fw, halo, nwalks, d.R * 2 * (d.n_fft + 1) + grid * 2 * d.n_fft


def syn_ws_floats(d):
    """rfx_fft_synthesis_ws"""
    if d.n_fft not in FFT_SIZES:
        return d.R * d.frames_out * d.n_fft
    return max(syn_own_geometry(d)[3], 1)


def syn_full(d):
    """does some stored frame cover every sample (launch_fft's `full`: else the launcher zero-fills unless accum)"""
    woff, nc = (d.n_fft - d.win) // 2, d.n_fft // 2
    c_lo, c_hi = d.frame0 * d.hop + woff, (d.frame0 + d.frames_out - 1) * d.hop + woff + d.win
    if d.in_mode == 1:
        return c_lo <= d.in_offset and c_hi >= d.in_offset + d.T
    return c_lo <= 2 * nc + 1 and c_hi >= d.T - 1


def forms_synthesis(d, lossgrad=False, mul=False):
    if d.n_fft not in FFT_SIZES:
        return forms_any(d, True, mul)
    fw, halo, nwalks, _ = syn_own_geometry(d)
    lg = "LG" if lossgrad else "plain"
    k = "fft_synthesis_kernel"
    out = {f"{k}<{d.n_fft},{lg},{'own' if nwalks else 'atomic'}>", f"{k}:{MODE_NAMES[d.mode]}", f"{k}:{'hop_magic' if d.hop <= 4096 else 'hop_division'}"}
    if nwalks:
        out.add(f"{k}:own_walks{min(nwalks, 3)}{'' if nwalks < 3 else '_or_more'}")
        if d.frames_out - (nwalks - 1) * fw != fw:
            out.add(f"{k}:own_last_walk_{'short' if d.frames_out < nwalks * fw else 'takes_remainder'}")
        out.add(f"{k}:own_{'full' if syn_full(d) else ('uncovered_kept' if d.accum else 'uncovered_memset')}")
        out.add(f"{k}:own_{'accum' if d.accum else 'write'}")
        out.add("fft_fold_zones_kernel" if d.in_mode == 0 else f"{k}:own_in_mode1")
        walk_batches = -(-(min(fw, d.frames_out) + halo) // _fb(d.n_fft))
        if walk_batches > 2:
            out.add(f"{k}:own_carry_beyond_two_batches")
    else:
        nb = _nb(d, True)
        out.add(f"{k}:atomic_nb{nb}")
        out.add(f"{k}:atomic_{'accum' if d.accum else 'memset'}")
        if d.hop > d.win:
            out.add(f"{k}:atomic_because_hop_gt_win")
        elif d.extra_pad_l or d.extra_pad_r:
            out.add(f"{k}:atomic_because_extra_pads")
        elif d.frame0:
            out.add(f"{k}:atomic_because_frame0")
        else:
            out.add(f"{k}:atomic_because_short_row")
    if mul:
        out.add(k + ":mul")
    out |= _desc_forms(k, d)
    return out


def pair_geometry(d):
    """pair_loss_geometry -> (nb, groups per row); rfx_stft_pair_loss_ws = 3 R groups doubles"""
    fb = 2 * (4096 // d.n_fft)
    batches, rows8 = -(-d.frames_out // fb), -(-d.R // 8)
    nb = 1
    while nb < PAIR_NB_MAX and rows8 * 8 * (-(-batches // (2 * nb))) >= 4096:
        nb *= 2
    return nb, -(-batches // nb)


def forms_pair(d, store):
    k = "fft_pair_loss_kernel"
    nb, groups = pair_geometry(d)
    fb = 2 * (4096 // d.n_fft)
    out = {f"{k}<{d.n_fft}>", f"{k}:nb{nb}", f"{k}:{'spectra_stored' if store else 'sums_only'}"}
    if d.frames_out % fb:
        out.add(k + ":ragged_last_batch")
        if d.frames_out % fb <= fb // 2:
            out.add(k + ":last_pair_frame_missing")
    if d.frames_out < fb:
        out.add(k + ":fewer_frames_than_a_batch")
    if groups > 1:
        out.add(k + ":several_groups")
    inside = [f for f in range(0, d.frames_out, fb) if f * d.hop >= d.n_fft // 2 and (f + fb - 1) * d.hop + d.n_fft - 1 - d.n_fft // 2 < d.T and f + fb <= d.frames_out]
    out.add(k + (":interior_batches" if inside and d.hop % 2 == 0 else ":edge_batches_only"))
    if d.hop % 2:
        out.add(k + ":odd_hop")
    if d.R % 8:
        out.add(k + ":partial_row_group")
    if d.R > 8:
        out.add(k + ":second_row_group")
    return out


# ---- forms: fft_any.hip ------------------------------------------------------------------------------------------------------------
def forms_any(d, syn, mul=False):
    fb = 1 if d.n_fft >= 2048 else 2048 // d.n_fft
    k = "fft_any_frames_kernel" if syn else "fft_any_analysis_kernel"
    out = {f"{k}<{d.n_fft}>", f"{k}:{MODE_NAMES[d.mode]}"}
    if d.frames_out % fb:
        out.add(k + ":ragged_last_batch")
    if d.frames_out > fb:
        out.add(k + ":several_batches")
    if d.herm:
        out.add(k + ":herm")
    if d.bins < d.n_fft // 2 + 1:
        out.add(k + (":no_nyquist" if d.bins == d.n_fft // 2 else ":few_bins"))
    if d.frame0:
        out.add(k + ":frame0")
    if mul:
        out.add(("fft_any_gather_kernel" if syn else k) + ":mul")
    if syn:
        g = "fft_any_gather_kernel"
        out.add(g + (":offset" if d.in_mode else (":mirrored_extra_pads" if d.extra_pad_l or d.extra_pad_r else ":mirrored")))
        out.add(g + (":accum" if d.accum else ":write"))
    else:
        out.add(k + (":in_mode1" if d.in_mode else (":extra_pads" if d.extra_pad_l or d.extra_pad_r else ":reflect")))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def signal(R, T, seed):
    """Gaussian rows of rms 0.3; the first and the last sample of every row are 1.5 (leaving an edge sample out must show)"""
    x = 0.3 * torch.randn(R, T, generator=torch.Generator().manual_seed(seed))
    x[:, 0] = 1.5
    x[:, -1] = -1.5
    return x


def spec_data(d, seed):
    """a complex Gaussian spectrum (R, F, bins) as float32 pairs, imaginary parts of DC / Nyquist included (they must be ignored)"""
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(d.R, d.frames_out, d.bins, generator=g), torch.randn(d.R, d.frames_out, d.bins, generator=g))


def store_layout(d, S):
    """complex (R, F, bins) -> the float32 tensor a synthesis reads in mode COMPLEX / CAC / FM"""
    return to_layout(d, S.to(torch.complex64)).float().contiguous()


# ---- case tables -------------------------------------------------------------------------------------------------------------------
GEOMS = ((512, 128, 512), (512, 50, 240), (512, 75, 301), (1024, 256, 1024), (1024, 120, 600), (2048, 512, 2048), (2048, 240, 1200),
         (4096, 1024, 4096), (4096, 1000, 4095))
ANY_GEOMS = tuple(fft_any_ref.GEOMS)             # all eight instantiations of fft_any.hip
ALL_MODES = (COMPLEX, CAC, MAG, POW, MAGPOW, FM)


def _case(name, d, **kw):
    c = dict(name=name, d=d, mul=False, x_off=0, modes=(d.mode,), seed=sum(map(ord, name)))
    c.update(kw)
    return c


def _ragged_len(n, hop):
    return hop * (3 * _fb(n) + 5) + n + 3


def _istft_desc(n, hop, win, R, frames, mode, frame0=0, frames_in=None, crop=0, cut=0, bins=None, normalized=False, accum=0):
    """torch.istft(center=True) of `frames` frames, of which [frame0, frame0 + frames_in) are stored; `cut` samples fewer than
    (frames - 1) hop; -> in_mode 1 descriptor (the same for the synthesis and for its backward, the analysis)"""
    length = (frames - 1) * hop - cut - crop
    return desc(R, length, n, hop, win, bins=bins, frame0=frame0, frames_out=frames - frame0 if frames_in is None else frames_in, mode=mode,
                in_mode=1, in_offset=n // 2 + crop, herm=1, scale=(math.sqrt(n) if normalized else 1.0) / n, accum=accum)


def _hdemucs_spec_desc(n, R, length, mode):
    """HDemucs._spec: hop n / 4, extra reflect pads of 3 hop / 2 (+ the fill to a whole number of hops), frames [2, 2 + le), no Nyquist
    bin, normalized"""
    hl = n // 4
    le, pad = -(-length // hl), hl // 2 * 3
    return desc(R, length, n, hl, n, bins=n // 2, frame0=2, frames_out=le, mode=mode, pads=(pad, pad + le * hl - length), scale=1.0 / math.sqrt(n))


def _hdemucs_ispec_desc(n, R, length, mode, accum=0):
    """HDemucs._ispec: frames [2, 2 + le) of le + 4, no Nyquist bin, crop of 3 hop / 2, normalized"""
    hl = n // 4
    le, pad = -(-length // hl), hl // 2 * 3
    return desc(R, length, n, hl, n, bins=n // 2, frame0=2, frames_out=le, mode=mode, in_mode=1, in_offset=n // 2 + pad, herm=1,
                scale=math.sqrt(n) / n, accum=accum)


def _analysis_cases():
    out = []
    for (n, hop, win) in GEOMS:
        L = _ragged_len(n, hop)
        tag = f"{n}_{hop}_{win}"
        out.append(_case(f"ana_{tag}_R3", desc(3, L, n, hop, win, eps=EPS, alpha=ALPHA), modes=ALL_MODES))
        out.append(_case(f"ana_{tag}_R9_fm", desc(9, L, n, hop, win, mode=FM)))
        out.append(_case(f"ana_{tag}_even", desc(3, L + 1, n, hop, win, mode=COMPLEX), modes=(COMPLEX, FM)))
    for (n, hop, win) in ((512, 128, 512), (1024, 120, 600), (4096, 1024, 4096)):
        L, tag = _ragged_len(n, hop), f"{n}_{hop}_{win}"
        out.append(_case(f"ana_{tag}_misaligned", desc(3, L + 1, n, hop, win, mode=FM), x_off=1, modes=(FM, CAC)))
        out.append(_case(f"ana_{tag}_no_nyquist", desc(3, L, n, hop, win, bins=n // 2, mode=COMPLEX), modes=(COMPLEX, FM)))
        out.append(_case(f"ana_{tag}_bins8", desc(3, L, n, hop, win, bins=8, mode=CAC, eps=EPS), modes=(CAC, FM, MAG)))
        out.append(_case(f"ana_{tag}_frame0", desc(3, L, n, hop, win, frame0=2, frames_out=2 * _fb(n) + 1, mode=COMPLEX), modes=(COMPLEX, FM)))
        out.append(_case(f"ana_{tag}_shortest_row", desc(2, n // 2 + 1, n, hop, win, mode=FM), modes=(FM, COMPLEX)))
    for n in (4096, 1024):
        out.append(_case(f"ana_hdemucs_spec_{n}", _hdemucs_spec_desc(n, 4, 5 * n + 777, CAC), modes=(CAC, FM)))
    # the iSTFT backward: in_mode 1, herm, the envelope as mul; an even and an odd row length (alternate rows mapped), an odd hop
    for (n, hop, win), cut in (((512, 128, 512), 0), ((512, 128, 512), 3), ((1024, 120, 600), 1), ((512, 75, 301), 0), ((4096, 1024, 4096), 0), ((2048, 240, 1200), 5)):
        frames = 3 * _fb(n) + 6
        out.append(_case(f"ana_istft_bwd_{n}_{hop}_{win}_cut{cut}", _istft_desc(n, hop, win, 3, frames, COMPLEX, cut=cut), mul=True, modes=(COMPLEX, FM)))
    out.append(_case("ana_hdemucs_ispec_bwd_4096", _hdemucs_ispec_desc(4096, 4, 5 * 4096 + 777, FM), mul=True, modes=(FM, CAC)))
    # nb = 2 / 4: frame-major only, rows8 8 ceil(batches / (2 nb)) >= 4096.  R = 64, 8 bins: 127 / 253 batches are the thresholds
    for (n, hop, frames) in ((512, 16, 127 * 16 - 11), (512, 16, 253 * 16 + 2), (4096, 64, 127 * 2), (4096, 64, 253 * 2 + 3)):
        out.append(_case(f"ana_{n}_{hop}_nb_frames{frames}", desc(64, (frames - 1) * hop + 5, n, hop, n, bins=8, mode=FM)))
    for (n, hop, win) in ANY_GEOMS:
        lens = fft_any_ref.lengths(n, hop)
        for L in lens:
            out.append(_case(f"ana_any_{n}_{hop}_{win}_L{L}", desc(3, L, n, hop, win, eps=EPS, alpha=ALPHA), modes=ALL_MODES))
        out.append(_case(f"ana_any_{n}_no_nyquist_frame0", desc(2, lens[0], n, hop, win, bins=n // 2, frame0=1, frames_out=2, mode=FM), modes=(FM, COMPLEX)))
        out.append(_case(f"ana_any_{n}_pads_bins8", desc(2, lens[0], n, hop, win, bins=8, mode=CAC, pads=(3, hop + 1)), modes=(CAC,)))
        out.append(_case(f"ana_any_istft_bwd_{n}", _istft_desc(n, hop, win, 2, 7, FM, cut=1), mul=True))
    return tuple(out)


def own_frame_counts(n, hop, win, in_mode, R=3):
    """frame counts that give one walk, two walks and three walks with a remainder (and, in_mode 0, a row longer than 2 n_fft + 2)"""
    probe = desc(R, 10 * n, n, hop, win, frames_out=1, in_mode=in_mode)
    fw = syn_own_geometry(probe)[0]
    fmin = (2 * n + 3) // hop + 1 if in_mode == 0 else 1
    return tuple(sorted({max(fw, fmin), max(2 * fw, fmin), max(3 * fw + fw // 2 + 1, fmin)}))


def _synthesis_cases():
    out = []
    lay = (COMPLEX, CAC, FM)
    i = 0
    for (n, hop, win) in GEOMS:
        tag = f"{n}_{hop}_{win}"
        for frames in own_frame_counts(n, hop, win, 0):
            # the adjoint of the STFT: in_mode 0, herm 0, every frame; T not a multiple of hop
            out.append(_case(f"syn_adj_{tag}_F{frames}", desc(3, (frames - 1) * hop + 3, n, hop, win, mode=lay[i % 3], accum=i % 2)))
            i += 1
        for frames in own_frame_counts(n, hop, win, 1):
            out.append(_case(f"syn_istft_{tag}_F{frames}", _istft_desc(n, hop, win, 3, frames, lay[i % 3], accum=i % 2, cut=i % 4), mul=True))
            i += 1
    for (n, hop, win) in ((512, 128, 512), (1024, 120, 600), (4096, 1024, 4096)):
        tag = f"{n}_{hop}_{win}"
        out.append(_case(f"syn_adj_{tag}_smallest_own_row", desc(9, 2 * n + 3, n, hop, win, mode=FM)))
        out.append(_case(f"syn_adj_{tag}_largest_atomic_row", desc(9, 2 * n + 2, n, hop, win, mode=FM)))
        out.append(_case(f"syn_adj_{tag}_shortest_row_accum", desc(2, n // 2 + 1, n, hop, win, mode=COMPLEX, accum=1)))
        F = own_frame_counts(n, hop, win, 0)[1]
        out.append(_case(f"syn_adj_{tag}_short_frames_out", desc(3, (F + 3) * hop + 3, n, hop, win, frames_out=F, mode=COMPLEX)))
        out.append(_case(f"syn_adj_{tag}_short_frames_out_accum", desc(3, (F + 3) * hop + 3, n, hop, win, frames_out=F, mode=CAC, accum=1)))
        out.append(_case(f"syn_adj_{tag}_frame0", desc(3, (F + 3) * hop + 3, n, hop, win, frame0=2, mode=COMPLEX)))
        out.append(_case(f"syn_adj_{tag}_no_nyquist_mul", desc(3, (F - 1) * hop + 3, n, hop, win, bins=n // 2, mode=FM), mul=True))
        out.append(_case(f"syn_istft_{tag}_frame0_short", _istft_desc(n, hop, win, 3, F + 4, CAC, frame0=2, frames_in=F - 1), mul=True))
        out.append(_case(f"syn_istft_{tag}_frame0_short_accum", _istft_desc(n, hop, win, 3, F + 4, FM, frame0=2, frames_in=F - 1, accum=1), mul=True))
        out.append(_case(f"syn_adj_{tag}_R64_many_walks", desc(64, 40 * _fb(n) * hop + 3, n, hop, win, bins=8, mode=FM)))
    for n in (4096, 1024):
        out.append(_case(f"syn_hdemucs_ispec_{n}", _hdemucs_ispec_desc(n, 4, 5 * n + 777, FM), mul=True))
        out.append(_case(f"syn_hdemucs_ispec_{n}_cac", _hdemucs_ispec_desc(n, 4, 5 * n + 777, CAC), mul=True))
        out.append(_case(f"syn_hdemucs_spec_adjoint_{n}", _hdemucs_spec_desc(n, 4, 5 * n + 777, CAC)))
    out.append(_case("syn_adj_hop_gt_win", desc(3, 9 * 300 + 3, 512, 300, 240, mode=COMPLEX)))
    out.append(_case("syn_adj_hop_gt_win_accum", desc(3, 9 * 300 + 3, 512, 300, 240, mode=FM, accum=1)))
    out.append(_case("syn_adj_hop_division", desc(3, 5 * 4100 + 3, 4096, 4100, 4096, mode=FM)))
    # no envelope here: without overlap 1 / envelope is 1 / w^2, which has no bound at the ends of a hann window
    out.append(_case("syn_istft_hop_division", _istft_desc(4096, 4100, 4096, 3, 5, COMPLEX)))
    for (n, hop, win) in ANY_GEOMS:
        L = 3 * n + 7
        for j, mode in enumerate(lay):
            out.append(_case(f"syn_any_adj_{n}_{MODE_NAMES[mode]}", desc(3, L, n, hop, win, mode=mode, accum=j % 2)))
        out.append(_case(f"syn_any_adj_{n}_pads", desc(2, L, n, hop, win, bins=n // 2, mode=FM, pads=(3, hop + 1))))
        out.append(_case(f"syn_any_adj_{n}_pads_accum", desc(2, L, n, hop, win, frame0=1, frames_out=2, mode=CAC, pads=(hop + 1, 2), accum=1)))
        out.append(_case(f"syn_any_istft_{n}", _istft_desc(n, hop, win, 2, 7, COMPLEX, cut=1), mul=True))
        out.append(_case(f"syn_any_istft_{n}_frame0_accum", _istft_desc(n, hop, win, 2, 9, FM, frame0=2, frames_in=5, accum=1, bins=n // 2), mul=True))
    return tuple(out)


def _lossgrad_cases():
    """rfx_fft_synthesis_lossgrad on synthetic xspec / ymag / sums: all four sizes (n_fft = 4096 has no forward that could feed it: the pair
    loss stops at 2048), ownership with one and several walks, the atomic form, gup null and set, a row whose A or B is 0"""
    out = []
    for i, (n, hop, win) in enumerate(((512, 128, 512), (512, 75, 301), (1024, 120, 600), (2048, 512, 2048), (4096, 1024, 4096), (4096, 1000, 4095))):
        fr = own_frame_counts(n, hop, win, 0)
        for frames in (fr[0], fr[-1]):
            out.append(_case(f"lg_{n}_{hop}_{win}_F{frames}", desc(3, (frames - 1) * hop + 3, n, hop, win, mode=FM, accum=(i + frames) % 2), gup=(None, 1.7)[(i + frames // 2) % 2]))
        out.append(_case(f"lg_{n}_{hop}_{win}_atomic", desc(3, 2 * n + 2, n, hop, win, mode=FM, accum=i % 2), gup=(1.7, None)[i % 2]))
    return tuple(out)


PAIR_CASES = tuple(
    [_case(f"pair_{n}_{hop}_{win}_R{R}_L{L}", desc(R, L, n, hop, win, mode=FM)) for (n, hop, win, R, L) in (
        (512, 75, 301, 1, 1500), (1024, 256, 1024, 9, 4099), (2048, 512, 2048, 2, 2049 + 512), (512, 128, 400, 17, 700),
        (512, 128, 512, 3, 128 * (3 * 32 + 5) + 512 + 3), (1024, 120, 600, 17, 120 * (3 * 8 + 4) + 1024), (2048, 240, 1200, 3, 240 * (3 * 4 + 3) + 2048 + 3))])

# nb = 2 / 4 of the pair kernel: rows8 8 ceil(batches / (2 nb)) >= 4096 at 16 frames per batch: 127 / 253 batches at R = 64
PAIR_NB_CASES = tuple(_case(f"pair_512_16_512_R64_frames{fr}", desc(64, (fr - 1) * 16 + 5, 512, 16, 512, mode=FM)) for fr in (127 * 16 - 11, 253 * 16 - 8))
PAIR_SAMPLE_ROWS = (0, 7, 8, -1)


def pair_sample_frames(d):
    """the frames on either side of every batch boundary (so of every group boundary too), and the first and the last frame"""
    fb = 2 * (4096 // d.n_fft)
    f = {0, d.frames_out - 1}
    for b in range(fb, d.frames_out, fb):
        f.update((b - 1, b))
    return torch.tensor(sorted(f))


def pair_loss_sampled(d, x, y, window, eps, chunk=4):
    """pair_loss where the stored spectra are too large to judge whole (0.5 GB): every row's sums and their bounds, and the cells of a
    SAMPLE -- all frames of rows 0, 7, 8 and R - 1 (both sides of a row-group boundary), and in every row the frames on either side of
    every batch and group boundary, where a walk's prefetch, carry or last-pair rule would go wrong -> dict"""
    dd = with_(d, mode=FM, scale=1.0)
    e, K = f32(eps), k_of("ana_fft") * EPS32
    rows = [r % d.R for r in PAIR_SAMPLE_ROWS]
    fr = pair_sample_frames(d)
    out = dict(sums=[], sums_bound=[], rows=rows, frames=fr, row_x=[], row_bx=[], row_ym=[], row_bym=[], fr_x=[], fr_bx=[], fr_ym=[], fr_bym=[])
    cm = lambda m: torch.sqrt(torch.clamp(m * m, min=e))                                    # noqa: E731
    for r0 in range(0, d.R, chunk):
        dc = with_(dd, R=min(chunk, d.R - r0))
        X, magx = spectrum(dc, x[r0:r0 + dc.R], window)
        Y, magy = spectrum(dc, y[r0:r0 + dc.R], window)
        bx, by = K * magx, K * magy
        out["sums"].append(loss_sums(X, Y, e))
        out["sums_bound"].append(loss_sums_bound(X, Y, bx, by, e, group=18))
        ym, bym = clamped_mag(Y, e), interval_bound(cm, Y.abs(), math.sqrt(2.0) * by)
        out["fr_x"].append(torch.view_as_real(X[:, fr].contiguous())), out["fr_bx"].append(bx[:, fr]), out["fr_ym"].append(ym[:, fr]), out["fr_bym"].append(bym[:, fr])
        for r in rows:
            if r0 <= r < r0 + dc.R:
                out["row_x"].append(torch.view_as_real(X[r - r0].contiguous())), out["row_bx"].append(bx[r - r0]), out["row_ym"].append(ym[r - r0]), out["row_bym"].append(bym[r - r0])
    for k in ("sums", "sums_bound", "fr_x", "fr_bx", "fr_ym", "fr_bym"):
        out[k] = torch.cat(out[k])
    for k in ("row_x", "row_bx", "row_ym", "row_bym"):
        out[k] = torch.stack(out[k])
    return out


ANALYSIS_CASES = _analysis_cases()
SYNTHESIS_CASES = _synthesis_cases()
LOSSGRAD_CASES = _lossgrad_cases()
LG_W_SC, LG_W_LM = 0.8, 1.3
LG_EPS = 2.0 ** -26            # = CELL_EPS: a float32 whose square root is one too
LG_DESIGNATED_BINS = (3, 4, 5, 6)
LG_LONE_FRAMES, LG_LONE_BIN = (1, 4, 7), 7        # row 0: |X|^2 one ulp above eps, ymag one ulp above |X|, one ulp below


@functools.lru_cache(maxsize=None)
def _case_by_name(name):
    for c in ANALYSIS_CASES + SYNTHESIS_CASES + LOSSGRAD_CASES + PAIR_CASES + PAIR_NB_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def analysis_inputs(c):
    """-> x (R, T) float32, window float32, mul float32 or None"""
    d = c["d"]
    x, w = signal(d.R, d.T, c["seed"]), hann(d.win)
    mul = inv_envelope(d, w, d.frame0 + d.frames_out + (2 if d.frame0 else 0)) if c["mul"] else None
    return x, w, mul


def synthesis_inputs(c):
    """-> spectrum complex64 (R, F, bins), window, mul or None, out0 (R, T) or None"""
    d = c["d"]
    w = hann(d.win)
    if not c["mul"]:
        mul = None
    elif d.in_mode == 1:
        mul = inv_envelope(d, w, d.frame0 + d.frames_out + (2 if d.frame0 else 0))
    else:
        mul = 0.5 + torch.rand(padded_len(d), generator=torch.Generator().manual_seed(c["seed"] + 7))
    out0 = signal(d.R, d.T, c["seed"] + 3) if d.accum else None
    return spec_data(d, c["seed"] + 1), w, mul, out0


def lossgrad_inputs(c):
    """-> xspec complex64 (R, F, bins), ymag (R, F, bins), sums (R, 3) float32, window.  |X| spreads over 0.5 .. 2 (so that 1 / |X| does
    not dominate a frame's magnitude) with a random phase, ymag is |X| times a factor away from 1 (no cell in the sign band); the last
    row's A is 0 (ksc = 0 there: only the log term).  Designated cells, all exact in float32 and in fp64 alike: bins 3 .. 6 of every
    frame hold X = 0, |X|^2 == eps, |X|^2 one step below eps (no gradient: the clamp is strict) and X = (0.375, 0.5) against
    ymag = 0.625 (the sign is exactly 0 and so is the difference: no gradient).  The band cells sit ALONE in a frame of row 0 whose
    other cells are X = 0 (LG_LONE_FRAMES, bin LG_LONE_BIN): |X|^2 one ulp above eps (the full gradient, 1 / |X| ~ 8192: alone, so that
    it weighs on no other frame's cells), and ymag one ulp above / below |X| = 0.625, where a hardware square root one ulp off would
    give the sign 0: both outcomes of those two frames are closed forms (lossgrad_sign_deltas)"""
    d = c["d"]
    g = torch.Generator().manual_seed(c["seed"] + 11)
    ph = 2.0 * math.pi * torch.rand(d.R, d.frames_out, d.bins, generator=g, dtype=torch.float64)
    X = (torch.polar(10.0 ** (torch.rand(d.R, d.frames_out, d.bins, generator=g, dtype=torch.float64) * 0.6 - 0.3), ph)).to(torch.complex64)
    f = 1.0 + (0.05 + 0.5 * torch.rand(d.R, d.frames_out, d.bins, generator=g)) * torch.where(torch.rand(d.R, d.frames_out, d.bins, generator=g) < 0.5, -1.0, 1.0)
    ymag = (X.abs() * f).float()
    h, m = np.float32(2.0 ** -13), np.float32(0.625)
    X[..., 3], X[..., 4], X[..., 5], X[..., 6] = 0, float(h), float(np.nextafter(h, np.float32(0))), 0.375 + 0.5j
    ymag[..., 3:6], ymag[..., 6] = 0.5, 0.625
    for fr in LG_LONE_FRAMES:
        X[0, fr], ymag[0, fr] = 0, 0.5
    b = LG_LONE_BIN
    X[0, LG_LONE_FRAMES[0], b] = complex(float(h), f32(2.0 ** -24.5))
    X[0, LG_LONE_FRAMES[1], b], ymag[0, LG_LONE_FRAMES[1], b] = 0.375 + 0.5j, float(np.nextafter(m, np.float32(1)))
    X[0, LG_LONE_FRAMES[2], b], ymag[0, LG_LONE_FRAMES[2], b] = 0.375 + 0.5j, float(np.nextafter(m, np.float32(0)))
    sums = torch.stack((0.5 + torch.rand(d.R, generator=g), 2.0 + torch.rand(d.R, generator=g), torch.rand(d.R, generator=g)), 1).float()
    sums[d.R - 1, 0] = 0.0
    return X, ymag, sums, hann(d.win)


def lossgrad_sign_deltas(d, X, ymag, sums, w_sc, w_lm, eps, gup, window):
    """what the output loses when the sign of the log term at one of the two one-ulp cells comes out 0: (R, T) per cell.  The four
    admissible outcomes of a case are the reference minus any subset of these."""
    G, _ = lossgrad_cells(X, ymag, sums, w_sc, w_lm, eps, gup)
    G0, _ = lossgrad_cells(X, ymag, sums, w_sc, 0.0, eps, gup)
    out = []
    for fr in LG_LONE_FRAMES[1:]:
        D = torch.zeros_like(G)
        D[0, fr, LG_LONE_BIN] = G[0, fr, LG_LONE_BIN] - G0[0, fr, LG_LONE_BIN]
        y = inverse_frames(d, D)
        out.append(_synthesis_tail(with_(d, accum=0), y, y.pow(2).mean(-1).sqrt(), window, None, None)[0])
    return out


def pair_inputs(c):
    """-> x, y (R, T), window; row 0 of y equals row 0 of x where R > 1 (its two numerator sums are exactly 0)"""
    d = c["d"]
    g = torch.Generator().manual_seed(c["seed"])
    x = 0.3 * torch.randn(d.R, d.T, generator=g)
    y = x + 0.1 * torch.randn(d.R, d.T, generator=g)
    if d.R > 1:
        y[0] = x[0]
    return x, y, hann(d.win)


FLOOR_ROWS = 3               # rows of a case the floors are measured on (the rows are independent draws; the R = 64 cases hold 10^8 cells)


def measure_floors(stats=None):
    """restate_* against the fp64 reference over the analysis and synthesis tables -> {class: largest error / (eps32 magnitude)}.
    stats (a dict) receives per case: `power` = the largest bound over the frame's rms |X| (analysis: Parseval makes that the frame's
    l2 norm) or over the row's rms output (synthesis); `weak` = the share of cells whose own value is within their bound"""
    fl = {}
    stats = {} if stats is None else stats
    for c in ANALYSIS_CASES:
        d = with_(c["d"], R=min(c["d"].R, FLOOR_ROWS), mode=FM)
        x, w, mul = analysis_inputs(c)
        X, mag = spectrum(d, x[:d.R], w, mul)
        X32 = restate_analysis(d, x[:d.R], w, mul)
        k = klass("ana", d.n_fft)
        fl[k] = max(fl.get(k, 0.0), floor_of(X32.real, X.real, mag), floor_of(X32.imag, X.imag, mag))
        b = k_of(k) * EPS32 * mag
        frame_rms = windowed_frames(d, x[:d.R].double(), w.double(), None if mul is None else mul.double()).pow(2).sum(-1).sqrt()
        stats[c["name"]] = dict(power=float((b / frame_rms[..., None].clamp_min(1e-300)).max()), weak=float((X.abs() <= b).double().mean()))
    for c in SYNTHESIS_CASES:
        d = with_(c["d"], R=min(c["d"].R, FLOOR_ROWS), accum=0)
        S, w, mul, _ = synthesis_inputs(c)
        out, bound = synthesis(d, S[:d.R], w, mul)
        k = klass("syn", d.n_fft)
        fl[k] = max(fl.get(k, 0.0), floor_of(restate_synthesis(d, S[:d.R], w, mul), out, bound / (k_of(k) * EPS32)))
        covered = bound > 0
        stats[c["name"]] = dict(power=float((bound / out.pow(2).mean(1, keepdim=True).sqrt()).max()),
                                weak=float((out.abs() <= bound)[covered].double().mean()), covered=float(covered.double().mean()))
    return fl


# ---- every form --------------------------------------------------------------------------------------------------------------------
# forms the case tables do not reach, by name with the reason (test_fft_ref_cpu.py asserts that this list and the walk together are
# exactly all_forms())
UNREACHED = {
    "fft_synthesis_kernel:atomic_nb2": "the atomic form walks two batches per workgroup only from 4096 workgroups on (R x frames >= 2^16 on a geometry "
                                       "the ownership form does not take: extra pads, hop > win or rows below 2 n_fft + 3): 0.5 GB of spectrum at the "
                                       "smallest, and nothing in the package launches it",
}


def all_forms():
    out = set(UNREACHED)
    a, s, p = "fft_analysis_kernel", "fft_synthesis_kernel", "fft_pair_loss_kernel"
    for n in FFT_SIZES:
        out.update(f"{a}<{n}>:{m}" for m in MODE_NAMES)
        out.update(f"{s}<{n},{lg},{own}>" for lg in ("plain", "LG") for own in ("own", "atomic"))
    out.update(f"{p}<{n}>" for n in FFT_SIZES[:3])
    out.update(f"{a}:{x}" for x in (
        "nb1", "nb2", "nb4", "load_fast", "load_mapped", "edge_left_batch", "ragged_batch", "edge_right_or_odd_row_batch", "fast_batch_prefetched_over_epilogue",
        "fast_then_mapped_in_one_walk", "mapped_then_fast_in_one_walk", "rows_take_different_paths", "x_misaligned", "odd_hop", "mul_fast", "mul_mapped"))
    desc_forms = ("herm", "in_mode1", "extra_pads", "partial_row_group", "second_row_group", "no_nyquist", "few_bins", "frame0", "ragged_last_batch", "win_short",
                  "odd_window_offset")
    out.update(f"{a}:{x}" for x in desc_forms)
    out.update(f"{s}:{x}" for x in desc_forms)
    out.update(f"{s}:{MODE_NAMES[m]}" for m in SPECTRUM_MODES)
    out.update(f"{s}:{x}" for x in (
        "hop_magic", "hop_division", "own_walks1", "own_walks2", "own_walks3_or_more", "own_last_walk_short", "own_last_walk_takes_remainder", "own_full",
        "own_uncovered_kept", "own_uncovered_memset", "own_accum", "own_write", "own_in_mode1", "own_carry_beyond_two_batches", "atomic_nb1", "atomic_accum",
        "atomic_memset", "atomic_because_hop_gt_win", "atomic_because_extra_pads", "atomic_because_frame0", "atomic_because_short_row", "mul"))
    out.add("fft_fold_zones_kernel")
    out.update(f"{p}:{x}" for x in ("nb1", "nb2", "nb4", "spectra_stored", "sums_only", "ragged_last_batch", "last_pair_frame_missing", "fewer_frames_than_a_batch", "several_groups",
                                    "interior_batches", "edge_batches_only", "odd_hop", "partial_row_group", "second_row_group"))
    for (n, _, _) in ANY_GEOMS:
        out.update((f"fft_any_analysis_kernel<{n}>", f"fft_any_frames_kernel<{n}>"))
    ka, kf, kg = "fft_any_analysis_kernel", "fft_any_frames_kernel", "fft_any_gather_kernel"
    out.update(f"{ka}:{m}" for m in MODE_NAMES)
    out.update(f"{kf}:{MODE_NAMES[m]}" for m in SPECTRUM_MODES)
    for k in (ka, kf):
        out.update(f"{k}:{x}" for x in ("ragged_last_batch", "several_batches", "herm", "no_nyquist", "frame0"))
    out.update(f"{ka}:{x}" for x in ("few_bins", "mul", "in_mode1", "extra_pads", "reflect"))
    out.update(f"{kg}:{x}" for x in ("mul", "offset", "mirrored_extra_pads", "mirrored", "accum", "write"))
    out.update("stft_loss_reduce_kernel:" + x for x in ("one_slot", "slots", "clamped_tail", "second_iteration", "idle_lanes"))
    out.update("stft_loss_grad_kernel:" + x for x in ("yc", "ymag", "gup", "no_gup", "second_iteration"))
    return out


def walk_all_cases():
    out = set()
    for c in ANALYSIS_CASES:
        for m in c["modes"]:
            out |= forms_analysis(with_(c["d"], mode=m), bool(c["x_off"]), c["mul"])
    for c in SYNTHESIS_CASES:
        out |= forms_synthesis(c["d"], False, c["mul"])
    for c in LOSSGRAD_CASES:
        out |= forms_synthesis(c["d"], True)
    for c in PAIR_CASES + PAIR_NB_CASES:
        for store in (False, True):
            out |= forms_pair(c["d"], store)
    for n in CELL_N:
        out |= forms_cells(n, "reduce")
        for kernel in ("yc", "ymag"):
            for gup in (False, True):
                out |= forms_cells(n, kernel, gup)
    return out
