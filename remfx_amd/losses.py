"""Losses and metrics of the removal path on HIP kernels.

Mirrors the auraloss objects the reference instantiates (remfx/models.py:7-8,
35-44, 171-176, 289-291, 312-314, 351-353, 374-376):
  MultiResolutionSTFTLoss(fft 1024/2048/512, hop 120/240/50, win 600/1200/240):
      mean over resolutions of [ ||Y|-|X||_F / ||Y||_F  +  mean |log|X| - log|Y|| ]
  SISDRLoss(zero_mean=True, eps=1e-8)
  nn.L1Loss
The class takes auraloss's keywords under auraloss's names.  With scale=None and weights (1, 1, 0) -- what the reference
builds -- `n_bins` / `sample_rate` are inert, as upstream, and the path above runs.  Otherwise:
  scale="mel"            |X|, |Y| go through a librosa-default mel filter bank (`mel_filterbank`) of `n_bins` filters at
                         `sample_rate` before the terms: rfx_stft_scaled_loss walks the BANDED bank inside the reduction pass
  w_sc, w_log_mag, w_lin_mag   per resolution w_sc sc + w_log_mag mean|log Mx - log My| + w_lin_mag mean|Mx - My|
                         (rfx_mrstft_combine_w; gradient rfx_stft_scaled_loss_grad + rfx_fft_synthesis)
  scale="chroma", w_phs != 0, perceptual_weighting, scale_invariance, output != "loss", reduction != "mean", mag_distance != "L1",
  a window other than hann      raise NotImplementedError at construction: nothing is accepted and dropped.
One deliberate difference: a mel filter without a non-zero weight (more filters than the low bins can carry) makes auraloss return
NaN (log 0 - log 0); here the constructor raises ValueError naming the resolution and the count.
`STFTLoss` is the single-resolution class auraloss exports, over the same function.
Resolutions: every power of two from 16 to 32768 (stft._desc), e.g. micro-tcn's (32, 128, 512, 2048, 8192, 32768).  512 / 1024 / 2048
take the paired one-launch forward and the fused gradient; every other size goes through two analyses + rfx_stft_loss_reduce /
rfx_stft_loss_grad + rfx_fft_synthesis (there is no paired or fused form for them).  scale="mel" stages a frame's magnitudes and the
bank in 64 KiB of LDS, which n_fft = 8192 and above do not fit: scale="mel" with any n_fft > 4096 raises NotImplementedError at
construction, naming the resolution.  The linear scale has no such limit, with default and non-default term weights.
`RandomResolutionSTFTLoss` is not ported.

Time-domain losses (auraloss.time; auraloss is not available to pin them: PARITY UNPINNED, restated in tests/time_loss_ref.py), on
(..., L) inputs taken as R rows of L samples, reduction "mean" / "sum" / "none" over the rows, differentiable in the prediction:
  SISDRLoss, SDSDRLoss, SNRLoss (zero_mean=True, eps=1e-8), ESRLoss, DCLoss (eps=1e-8), LogCoshLoss (a=1.0, eps=1e-8)
The five ratio losses are functions of the row sums {Sx, St, Sxt, Sxx, Stt}, so their gradient is a x + b t + c with three fp64
numbers per row: rfx_time_sums, rfx_time_loss_rows, and ONE rfx_time_loss_grad launch in the backward.
`prefilter=(h_prev, h_cur, h_next)` is a keyword this port adds (auraloss applies its FIRFilter as a separate module): both signals are
first replaced by h_prev s[n-1] + h_cur s[n] + h_next s[n+1], zeros outside the row -- conv1d with those weights and padding=1;
pre-emphasis is (-0.85, 1, 0), and the three conv weights of an auraloss FIRFilter of the first-order kinds can be passed as they are
(the A-weighting kind is not a `prefilter`: it is the FIRFilter module below).  Unknown `reduction`, a `prefilter` that is not three
finite numbers, L < 1: ValueError.
SISDRLoss without a gradient to compute and with default keywords is the metric it always was: rfx_sisdr_sums + rfx_sisdr_finish.

Perceptual prefilter and stereo term (auraloss.perceptual.FIRFilter, auraloss.freq.SumAndDifferenceSTFTLoss; PARITY UNPINNED; DESIGN.md
4.3c):
  FIRFilter(filter_type="hp" | "fd" | "aw", coef, fs, ntaps)   forward(input, target) -> both filtered: rfx_fir_same, a 'same'-padded
                         K-tap FIR per row (K odd, <= 1025), both signals in one launch; the backward is the same kernel with the
                         taps flipped.  `a_weighting_taps(fs, ntaps)` is auraloss's A-weighting design.  MultiResolutionSTFTLoss(
                         perceptual_weighting=True) keeps raising: apply the module in front of the loss.
  SumAndDifferenceSTFTLoss(..., w_sum, w_diff, **mrstft keywords)   (B, 2, T): rfx_sum_diff, then one inner MultiResolutionSTFTLoss
                         on the sum and on the difference pair; (w_sum * sum + w_diff * diff) / 2.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import stft
from .ops import _req, launch, query, scratch, zeros

FFT_SIZES = (1024, 2048, 512)
HOP_SIZES = (120, 240, 50)
WIN_LENGTHS = (600, 1200, 240)
MEL_MAX_N_FFT = 4096                                              # rfx_stft_scaled_loss with a bank: 64 KiB of LDS per frame


FUSED_GRAD = os.environ.get("RFX_LOSS_FUSED_GRAD", "1") != "0"    # A/B: 0 = rfx_stft_loss_grad_m + rfx_fft_synthesis as two launches
PAIRED = os.environ.get("RFX_LOSS_PAIRED", "1") != "0"            # A/B: 0 = two analyses + rfx_stft_loss_reduce / _grad at every n_fft

_MEMO = None


class stft_memo:
    """Scope in which the spectra the MRSTFT loss / metric take are computed once per (signal, resolution).

    RemFX.common_step evaluates MRSTFT three times on one batch -- loss(output, target), metric(output, target) and
    metric(input, target) (models.py:220-255) -- i.e. the same STFT of the target three times and of the output twice.
    Inside ``with stft_memo():`` a repeated request for the spectrum of the same storage at the same version returns
    the tensor computed the first time.  The memo dies with the scope, so nothing is carried from one step to the next.
    """

    def __enter__(self):
        global _MEMO
        self._prev, _MEMO = _MEMO, {}
        return self

    def __exit__(self, *exc):
        global _MEMO
        _MEMO = self._prev
        return False


# The loss kernels are elementwise over (prediction, target) spectra plus row sums: layout-free.  Frame-major spectra
# ([R][frames][bins][2]) let the FFT kernels store / load whole lines instead of pieces of a [bin][frame] transpose.
_SPEC_MODE = stft.MODES["complex_fm"]


def _spectrum(sig, n_fft, hop, win, w):
    if _MEMO is None:
        return stft.stft_raw(sig, n_fft, hop, win, w, _SPEC_MODE)
    key = (sig.data_ptr(), sig._version, tuple(sig.shape), tuple(sig.stride()), n_fft, hop, win)
    hit = _MEMO.get(key)
    if hit is None:
        hit = (sig, stft.stft_raw(sig, n_fft, hop, win, w, _SPEC_MODE))     # holding sig keeps its storage from being reused
        _MEMO[key] = hit
        _MEMO[("spec", hit[1].data_ptr())] = True
    return hit[1]


def _sig_key(sig):
    return (sig.data_ptr(), sig._version, tuple(sig.shape), tuple(sig.stride()))


def _pair_sums(x2, y2, n_fft, hop, win, w, eps, store):
    """One resolution in one launch (rfx_stft_pair_loss): row sums [R, 3]; with store=True also the prediction's spectrum
    (frame-major complex) and the clamped target magnitudes, which the backward reads.  Memoised like _spectrum."""
    key = ("pair", _sig_key(x2), _sig_key(y2), n_fft, hop, win, eps)
    hit = _MEMO.get(key) if _MEMO is not None else None
    if hit is not None and (hit[1] is not None or not store):
        return hit[0], hit[1], hit[2]
    R, L = x2.shape
    if n_fft // 2 >= L:
        raise ValueError("reflect padding needs n_fft/2 < signal length")
    frames, bins = 1 + L // hop, n_fft // 2 + 1
    sums = torch.empty((R, 3), device=x2.device, dtype=torch.float32)       # written, not accumulated: no zero fill
    X = torch.empty((R, frames, bins, 2), device=x2.device, dtype=torch.float32) if store else None
    ym = torch.empty((R, frames, bins), device=x2.device, dtype=torch.float32) if store else None
    d = stft._desc(R, L, n_fft, hop, win, bins, 0, frames, _SPEC_MODE)
    ws = torch.empty(query("rfx_stft_pair_loss_ws", C.byref(d)), device=x2.device, dtype=torch.float64)   # one slot per workgroup
    launch("rfx_stft_pair_loss", C.byref(d), x2, y2, w, eps, ws, sums, X, ym)
    if _MEMO is not None:
        _MEMO[key] = (sums, X, ym, x2, y2)      # holding the signals keeps their storage from being reused under the key
    return sums, X, ym


DEFAULT_WEIGHTS = (1.0, 1.0, 0.0)        # auraloss: w_sc, w_log_mag, w_lin_mag


def _hz_to_mel(f):
    """Slaney's mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz (200 / 3 Hz per mel), then log with step ln(6.4) / 27."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sample_rate, n_fft, n_mels):
    """librosa.filters.mel(sr=sample_rate, n_fft=n_fft, n_mels=n_mels) with its defaults, restated (librosa is not a dependency):
    Slaney mel scale, fmin = 0, fmax = sr / 2, triangles between n_mels + 2 edge frequencies equally spaced in mel, each scaled by
    2 / (f[i + 2] - f[i]) (Slaney area normalisation).  fp64 arithmetic; returns fp32 (n_mels, n_fft / 2 + 1) -- what
    auraloss.freq.STFTLoss(scale="mel") multiplies the magnitudes by."""
    bins = n_fft // 2 + 1
    freqs = np.linspace(0.0, sample_rate / 2.0, bins)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sample_rate / 2.0), n_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return torch.from_numpy(w.astype(np.float32))


def pack_banded(dense):
    """(rows, cols) matrix -> (idx int32 [rows, 3], w fp32 [n_w]): per row the first non-zero column, the length up to the last one
    and the offset of its weights in w -- the form rfx_stft_scaled_loss (fb) and rfx_stft_scaled_loss_grad (fb^T) take.  Exact:
    interior zeros of a row are kept, so any matrix round-trips; a triangular bank costs ~2 * cols weights instead of rows * cols."""
    d = np.asarray(dense, dtype=np.float32)
    idx, w = np.zeros((d.shape[0], 3), dtype=np.int32), []
    for r in range(d.shape[0]):
        nz = np.nonzero(d[r])[0]
        first, ln = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        idx[r] = (first, ln, sum(len(c) for c in w))
        w.append(d[r, first:first + ln])
    w = np.concatenate(w) if w else np.zeros(0, dtype=np.float32)
    if w.size == 0:
        w = np.zeros(1, dtype=np.float32)
    return torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(w))


class _Bank:
    """One resolution's banded filter bank on the device: the band of fb (forward) and of fb^T (backward)."""

    def __init__(self, idx, w, tidx, tw, n_out, bins):
        self.idx, self.w, self.tidx, self.tw, self.n_out, self.bins = idx, w, tidx, tw, n_out, bins


def _scaled_sums(X, Y, bank, eps, weights, store):
    """Row sums [R, 4] fp64 of one resolution through rfx_stft_scaled_loss (+ Mx, My with store=True).  Memoised next to the spectra:
    metric-style repeats of the same (spectra, filter bank, weights) evaluation inside stft_memo() reuse them."""
    R, frames, bins = X.shape[:3]
    n_out = bank.n_out if bank is not None else bins
    key = ("ssums", X.data_ptr(), Y.data_ptr(), eps, bank.w.data_ptr() if bank is not None else 0, weights)
    hit = _MEMO.get(key) if _MEMO is not None else None
    if hit is not None and (hit[1] is not None or not store):
        return hit
    sums = torch.empty((R, 4), device=X.device, dtype=torch.float64)         # written, not accumulated: no zero fill
    mx = torch.empty((R, frames, n_out), device=X.device, dtype=torch.float32) if store else None
    my = torch.empty((R, frames, n_out), device=X.device, dtype=torch.float32) if store else None
    ws = torch.empty(query("rfx_stft_scaled_loss_ws", R, frames), device=X.device, dtype=torch.float64)   # one slot per workgroup
    if bank is not None and (bank.bins != bins or bank.w.device != X.device):
        raise ValueError(f"filter bank for {bank.bins} bins on {bank.w.device}, spectrum has {bins} on {X.device}")
    launch("rfx_stft_scaled_loss", X, Y, R, frames, bins, bank.idx if bank is not None else None,
           bank.w if bank is not None else None, n_out, bank.w.numel() if bank is not None else 0, eps, ws, sums, mx, my)
    hit = (sums, mx, my)
    if _MEMO is not None and ("spec", X.data_ptr()) in _MEMO and ("spec", Y.data_ptr()) in _MEMO:
        _MEMO[key] = hit                                                     # both spectra are held by the memo: pointers stay valid
    return hit


def _scaled_forward(ctx, x, y, fft_sizes, hops, wins, eps, per_example_sc, weights, banks):
    """auraloss STFTLoss.forward with a frequency scale and / or non-default term weights, per resolution: two memoised spectra,
    rfx_stft_scaled_loss, then one rfx_mrstft_combine_w over all resolutions."""
    _req(x, "input"); _req(y, "target")
    L = x.shape[-1]
    x2, y2 = x.reshape(-1, L).contiguous(), y.reshape(-1, L).contiguous()
    R = x2.shape[0]
    saved = []
    for (n_fft, hop, win), bank in zip(zip(fft_sizes, hops, wins), banks):
        w = stft.hann(win, x.device)
        X = _spectrum(x2, n_fft, hop, win, w)
        Y = _spectrum(y2, n_fft, hop, win, w)
        sums, mx, my = _scaled_sums(X, Y, bank, eps, weights, ctx.needs_input_grad[0])
        n_out = bank.n_out if bank is not None else X.shape[2]
        saved.append((X, mx, my, sums, X.shape[1] * n_out, n_fft, hop, win, bank))
    nres, total = len(saved), None
    for c0 in range(0, nres, 8):                   # rfx_mrstft_combine_w takes up to 8 resolutions per launch
        part = saved[c0:c0 + 8]
        m = len(part)
        t = torch.empty((), device=x.device, dtype=torch.float32)
        sp = (C.c_void_p * m)(*[e[3].data_ptr() for e in part])
        nn_ = (C.c_int64 * m)(*[int(e[4]) for e in part])
        launch("rfx_mrstft_combine_w", sp, nn_, m, R, 1 if per_example_sc else 0, weights[0], weights[1], weights[2], t)
        total = t if nres <= 8 else (t * (m / nres) if total is None else total + t * (m / nres))
    ctx.scaled = True
    ctx.saved = saved
    ctx.meta = (x.shape, R, L, eps, per_example_sc, nres, weights)
    return total


def _scaled_backward(ctx, g):
    shape, R, L, eps, per_example_sc, nres, (w_sc, w_lm, w_lin) = ctx.meta
    gx = torch.empty((R, L), device=g.device, dtype=torch.float32)        # the first resolution writes it, the others add (accum)
    gup = g.detach().reshape(1).float().contiguous()                      # upstream scalar gradient stays on the device
    for ires, (X, mx, my, sums, n, n_fft, hop, win, bank) in enumerate(ctx.saved):
        frames, bins = X.shape[1], X.shape[2]
        G = torch.empty_like(X)
        launch("rfx_stft_scaled_loss_grad",
               X, mx, my, R, frames, bins, bank.tidx if bank is not None else None,
               bank.tw if bank is not None else None, n // frames, eps, sums, 1 if per_example_sc else 0,
               w_sc / (nres * R) if per_example_sc else w_sc / nres, w_lm / (nres * R * n), w_lin / (nres * R * n), gup, G)
        d = stft._desc(R, L, n_fft, hop, win, bins, 0, frames, _SPEC_MODE, in_mode=0, herm=0, scale=1.0, accum=1 if ires else 0)
        launch("rfx_fft_synthesis", C.byref(d), G, stft.hann(win, g.device), None, stft.syn_ws(d, g.device), gx)
    ctx.saved = None
    return gx.view(shape)


class _MRSTFTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, fft_sizes, hops, wins, eps, per_example_sc, *scaled):
        # scaled = (weights, banks): the three term weights and one banded filter bank (or None) per resolution; absent, or the
        # default (1, 1, 0) without a bank: the path below, untouched
        ctx.n_extra, ctx.scaled = len(scaled), False
        if scaled and (tuple(scaled[0]) != DEFAULT_WEIGHTS or any(b is not None for b in scaled[1])):
            return _scaled_forward(ctx, x, y, fft_sizes, hops, wins, eps, per_example_sc, tuple(scaled[0]), scaled[1])
        _req(x, "input"); _req(y, "target")
        L = x.shape[-1]
        x2, y2 = x.reshape(-1, L).contiguous(), y.reshape(-1, L).contiguous()
        R = x2.shape[0]
        saved, total = [], None
        for n_fft, hop, win in zip(fft_sizes, hops, wins):
            w = stft.hann(win, x.device)
            if PAIRED and n_fft in (512, 1024, 2048):
                # both spectra of a frame from one complex FFT, sums in its epilogue: no spectrum is written unless the backward
                # needs it, and then only the prediction's + the target's magnitudes
                sums, X, Y = _pair_sums(x2, y2, n_fft, hop, win, w, eps, ctx.needs_input_grad[0])
                n = (1 + L // hop) * (n_fft // 2 + 1)
                paired = True
            else:
                X = _spectrum(x2, n_fft, hop, win, w)
                Y = _spectrum(y2, n_fft, hop, win, w)
                n = X.shape[1] * X.shape[2]
                paired = False
                skey = ("sums", X.data_ptr(), Y.data_ptr(), eps)
                sums = _MEMO.get(skey) if _MEMO is not None else None   # metric(output, target) repeats the loss's row sums
                if sums is None:
                    sums = torch.empty((R, 3), device=x.device, dtype=torch.float32)
                    ws = scratch("rfx_stft_loss_reduce_ws", R, n, device=x.device, dtype=torch.float64)      # per-workgroup partials
                    launch("rfx_stft_loss_reduce", X, Y, R, n, eps, ws, sums)
                    if _MEMO is not None and ("spec", X.data_ptr()) in _MEMO and ("spec", Y.data_ptr()) in _MEMO:
                        _MEMO[skey] = sums                               # both spectra are held by the memo: pointers stay valid
            saved.append((paired, X, Y, sums, n, n_fft, hop, win))
        # sc + lm of every resolution and their mean: one launch on the row sums (was ~24 one-element torch launches per evaluation)
        nres = len(saved)
        total = None
        for c0 in range(0, nres, 8):               # rfx_mrstft_combine takes up to 8 resolutions per launch (auraloss's default has 3)
            part, m = saved[c0:c0 + 8], len(saved[c0:c0 + 8])
            t = torch.empty((), device=x.device, dtype=torch.float32)
            sp = (C.c_void_p * m)(*[e[3].data_ptr() for e in part])
            nn_ = (C.c_int64 * m)(*[int(e[4]) for e in part])
            launch("rfx_mrstft_combine", sp, nn_, m, R, 1 if per_example_sc else 0, t)
            total = t if nres <= 8 else (t * (m / nres) if total is None else total + t * (m / nres))
        ctx.saved = saved
        ctx.meta = (x.shape, R, L, eps, per_example_sc, nres)
        return total

    @staticmethod
    def backward(ctx, g):
        if ctx.scaled:
            return (_scaled_backward(ctx, g),) + (None,) * (6 + ctx.n_extra)
        shape, R, L, eps, per_example_sc, nres = ctx.meta
        gx = torch.empty((R, L), device=g.device, dtype=torch.float32)    # the first resolution writes it, the others add (accum)
        gval = 1.0               # the scalar upstream gradient stays on the device: the kernels multiply their weights by *gup
        gup = g.detach().reshape(1).float().contiguous()
        for ires, (paired, X, Y, sums, n, n_fft, hop, win) in enumerate(ctx.saved):
            if not per_example_sc:      # whole-batch Frobenius norm: same A, B for every row
                sums = sums.clone()
                sums[:, 0] = sums[:, 0].sum()
                sums[:, 1] = sums[:, 1].sum()
                w_sc = gval / nres
            else:
                w_sc = gval / (nres * R)
            w_lm = gval / (nres * R * n)
            w = stft.hann(win, g.device)
            d = stft._desc(R, L, n_fft, hop, win, X.shape[2], 0, X.shape[1], _SPEC_MODE, in_mode=0, herm=0, scale=1.0,
                           accum=1 if ires else 0)
            if paired and FUSED_GRAD:   # Y = the clamped target magnitudes; the gradient spectrum is formed inside the synthesis
                launch("rfx_fft_synthesis_lossgrad", C.byref(d), X, Y, sums, w_sc, w_lm, eps, gup, w, stft.syn_ws(d, g.device), gx)
                continue
            G = torch.empty_like(X)
            launch("rfx_stft_loss_grad_m" if paired else "rfx_stft_loss_grad", X, Y, R, n, eps, sums, w_sc, w_lm, gup, G)
            launch("rfx_fft_synthesis", C.byref(d), G, w, None, stft.syn_ws(d, g.device), gx)
        ctx.saved = None
        return (gx.view(shape),) + (None,) * (6 + ctx.n_extra)


def _check_honoured(scale, w_phs, perceptual_weighting, scale_invariance, output, reduction, mag_distance, window):
    """auraloss keywords this port does not implement raise here instead of being accepted and dropped."""
    bad = []
    if scale not in (None, "mel"):
        bad.append(f"scale={scale!r} (None and 'mel' are implemented)")
    if w_phs != 0:
        bad.append(f"w_phs={w_phs!r} (the phase term)")
    if perceptual_weighting:
        bad.append("perceptual_weighting=True (apply FIRFilter(\"aw\", fs=...) to both signals in front of the loss instead)")
    if scale_invariance:
        bad.append("scale_invariance=True")
    if output != "loss":
        bad.append(f"output={output!r}")
    if reduction != "mean":
        bad.append(f"reduction={reduction!r}")
    if mag_distance != "L1":
        bad.append(f"mag_distance={mag_distance!r}")
    if window != "hann_window":
        bad.append(f"window={window!r}")
    if bad:
        raise NotImplementedError("MultiResolutionSTFTLoss / STFTLoss on HIP kernels does not implement: " + "; ".join(bad))


class MultiResolutionSTFTLoss(nn.Module):
    """auraloss.freq.MultiResolutionSTFTLoss with auraloss's keyword names and defaults (module docstring: what is implemented and
    what raises).  `per_example_sc` picks the spectral-convergence form of auraloss >= 0.4 (True) or the older whole-batch norm.
    With scale="mel" the dense banks are `self.filterbanks` (one fp32 (n_bins, n_fft / 2 + 1) per resolution); they and their banded
    forms are non-persistent buffers, so `.to(device)` moves them and checkpoints keep their keys."""

    def __init__(self, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, window="hann_window", w_sc=1.0,
                 w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0, sample_rate=None, scale=None, n_bins=None, perceptual_weighting=False,
                 scale_invariance=False, eps=1e-8, output="loss", reduction="mean", mag_distance="L1", device=None,
                 per_example_sc=True):
        super().__init__()
        self.fft_sizes, self.hop_sizes, self.win_lengths = tuple(fft_sizes), tuple(hop_sizes), tuple(win_lengths)
        if not len(self.fft_sizes) == len(self.hop_sizes) == len(self.win_lengths):
            raise ValueError("fft_sizes, hop_sizes and win_lengths need one entry per resolution")
        self.eps, self.per_example_sc = eps, per_example_sc
        _check_honoured(scale, w_phs, perceptual_weighting, scale_invariance, output, reduction, mag_distance, window)
        self.scale, self.n_bins, self.sample_rate = scale, n_bins, sample_rate
        self.weights = (float(w_sc), float(w_log_mag), float(w_lin_mag))
        self._nbank = 0
        if scale == "mel":
            if n_bins is None or sample_rate is None:
                raise ValueError('scale="mel" needs n_bins (the number of mel filters) and sample_rate')
            for k, n_fft in enumerate(self.fft_sizes):
                if n_fft > MEL_MAX_N_FFT:
                    raise NotImplementedError(f'scale="mel" at resolution {k} (n_fft={n_fft}): the mel reduction kernel holds a frame\'s '
                                              f"magnitudes and the bank in LDS and covers n_fft <= {MEL_MAX_N_FFT}; use the linear "
                                              "scale (scale=None) for larger resolutions")
                fb = mel_filterbank(sample_rate, n_fft, n_bins)
                empty = int((fb.abs().sum(1) == 0).sum())
                if empty:
                    raise ValueError(f"mel filter bank of resolution {k} (n_fft={n_fft}, sample_rate={sample_rate}): {empty} of "
                                     f"{n_bins} filters have no non-zero weight (narrower than a bin); auraloss would return NaN. "
                                     "Use fewer n_bins or a larger n_fft")
                idx, w = pack_banded(fb.numpy())
                tidx, tw = pack_banded(fb.numpy().T)
                for name, t in (("fb", fb), ("fb_idx", idx), ("fb_w", w), ("fbt_idx", tidx), ("fbt_w", tw)):
                    self.register_buffer(f"{name}_{k}", t, persistent=False)
            self._nbank = len(self.fft_sizes)

    @property
    def filterbanks(self):
        return [getattr(self, f"fb_{k}") for k in range(self._nbank)]

    def _banks(self):
        if not self._nbank:
            return (None,) * len(self.fft_sizes)
        return tuple(_Bank(getattr(self, f"fb_idx_{k}"), getattr(self, f"fb_w_{k}"), getattr(self, f"fbt_idx_{k}"),
                           getattr(self, f"fbt_w_{k}"), self.n_bins, n_fft // 2 + 1) for k, n_fft in enumerate(self.fft_sizes))

    def forward(self, input, target):
        if self.scale is None and self.weights == DEFAULT_WEIGHTS:
            return _MRSTFTFn.apply(input, target, self.fft_sizes, self.hop_sizes, self.win_lengths, self.eps,
                                   self.per_example_sc)
        return _MRSTFTFn.apply(input, target, self.fft_sizes, self.hop_sizes, self.win_lengths, self.eps,
                               self.per_example_sc, self.weights, self._banks())


class STFTLoss(MultiResolutionSTFTLoss):
    """auraloss.freq.STFTLoss: one resolution (auraloss's defaults 1024 / 256 / 1024) of the same function."""

    def __init__(self, fft_size=1024, hop_size=256, win_length=1024, **kwargs):
        super().__init__(fft_sizes=(fft_size,), hop_sizes=(hop_size,), win_lengths=(win_length,), **kwargs)


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _req(a, "input"); _req(b, "target")
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws = scratch("rfx_l1_sum_ws", a.numel(), device=a.device, dtype=torch.float64)      # per-workgroup partials
        launch("rfx_l1_sum", a, b, a.numel(), ws, 1.0 / a.numel(), out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)
        gup = g.detach().reshape(1).float().contiguous()          # upstream scalar gradient, multiplied in on the device (no host sync)
        launch("rfx_l1_grad", a, b, a.numel(), 1.0 / a.numel(), gup, ga)
        return ga, None


class L1Loss(nn.Module):
    def forward(self, input, target):
        return _L1Fn.apply(input, target)


TIME_KINDS = {"sisdr": 0, "sdsdr": 1, "snr": 2, "esr": 3, "dc": 4, "logcosh": 5}          # RFX_TIME_* of include/remfx_hip.h
REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}                                                 # RFX_REDUCE_*


def _check_reduction(reduction):
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction={reduction!r}: one of 'mean', 'sum', 'none'")
    return reduction


def _check_prefilter(prefilter):
    """None, or the three conv weights (h_prev, h_cur, h_next) of a first-order FIR prefilter as finite numbers."""
    if prefilter is None:
        return None
    try:
        taps = tuple(float(v) for v in prefilter)
    except (TypeError, ValueError):
        raise ValueError(f"prefilter={prefilter!r}: three finite numbers (h_prev, h_cur, h_next), e.g. (-0.85, 1, 0)") from None
    if len(taps) != 3 or not all(np.isfinite(v) for v in taps):
        raise ValueError(f"prefilter={prefilter!r}: three finite numbers (h_prev, h_cur, h_next), e.g. (-0.85, 1, 0)")
    return taps


def _rows(input, target):
    """(..., L) -> R rows of L samples with unit sample stride; cropped views keep their row stride (no copy)."""
    _req(input, "input"); _req(target, "target")
    if input.shape != target.shape:
        raise ValueError(f"input {tuple(input.shape)} and target {tuple(target.shape)} differ in shape")
    if input.dim() < 1 or input.shape[-1] < 1 or input.numel() == 0:
        raise ValueError(f"time-domain losses need (..., L) with L >= 1 and at least one row (got {tuple(input.shape)})")
    L = input.shape[-1]
    x, t = input.reshape(-1, L), target.reshape(-1, L)
    if x.stride(-1) != 1:
        x = x.contiguous()
    if t.stride(-1) != 1:
        t = t.contiguous()
    return x, t, x.shape[0], L


class _TimeLossFn(torch.autograd.Function):
    """The six time-domain losses: row sums (rfx_time_sums / rfx_logcosh_rows), the per-row kernel (rfx_time_loss_rows: losses,
    gradient coefficients, reduced scalar), and in the backward ONE streaming launch (rfx_time_loss_grad / rfx_logcosh_grad) that
    reads the upstream gradient on the device.  No gradient with respect to the target."""

    @staticmethod
    def forward(ctx, input, target, kind, zero_mean, eps, reduction, taps, a):
        x, t, R, L = _rows(input, target)
        dev = x.device
        k, red = TIME_KINDS[kind], REDUCTIONS[reduction]
        h = taps if taps is not None else (0.0, 1.0, 0.0)
        need = ctx.needs_input_grad[0]
        if kind == "logcosh":
            s = torch.empty((R,), device=dev, dtype=torch.float64)
            ws = torch.empty(query("rfx_logcosh_ws", R, L), device=dev, dtype=torch.float64)      # one slot per workgroup
            launch("rfx_logcosh_rows", x, t, R, L, x.stride(0), t.stride(0), float(a), float(eps), ws, s)
            coef = None
        else:
            s = torch.empty((R, 5), device=dev, dtype=torch.float64)                            # written, not accumulated: no zero fill
            ws = torch.empty(query("rfx_time_sums_ws", R, L), device=dev, dtype=torch.float64)
            launch("rfx_time_sums", x, t, R, L, x.stride(0), t.stride(0), 1 if taps is not None else 0, h[0], h[1], h[2], ws, s)
            coef = torch.empty((R, 3), device=dev, dtype=torch.float64) if need else None
        rows = torch.empty((R,), device=dev, dtype=torch.float32)
        out = torch.empty((), device=dev, dtype=torch.float32) if reduction != "none" else None
        launch("rfx_time_loss_rows", s, R, L, k, 1 if zero_mean else 0, float(eps), red, rows, coef, out)
        if need:
            ctx.save_for_backward(x, t, coef)
            ctx.meta = (input.shape, R, L, kind, red, taps, h, float(a), float(eps))
        return out if out is not None else rows.view(input.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        x, t, coef = ctx.saved_tensors
        shape, R, L, kind, red, taps, h, a, eps = ctx.meta
        gx = torch.empty((R, L), device=x.device, dtype=torch.float32)
        gup = g.detach().reshape(-1).float().contiguous()                 # 1 value (mean / sum) or R (none); stays on the device
        if kind == "logcosh":
            launch("rfx_logcosh_grad", x, t, R, L, x.stride(0), t.stride(0), a, eps, gup, red, gx)
        else:
            launch("rfx_time_loss_grad", x, t, R, L, x.stride(0), t.stride(0), coef, 1 if taps is not None else 0, h[0], h[1], h[2],
                   gup, red, gx)
        return (gx.view(shape),) + (None,) * 7


class _TimeLoss(nn.Module):
    """Base of the time-domain losses: no parameters, no buffers; `forward(input, target)` on (..., L) fp32 GPU tensors."""
    kind = None

    def __init__(self, zero_mean=True, eps=1e-8, reduction="mean", prefilter=None, a=1.0):
        super().__init__()
        self.zero_mean, self.eps, self.reduction = bool(zero_mean), float(eps), _check_reduction(reduction)
        self.prefilter, self.a = _check_prefilter(prefilter), float(a)

    def forward(self, input, target):
        return _TimeLossFn.apply(input, target, self.kind, self.zero_mean, self.eps, self.reduction, self.prefilter, self.a)


class SISDRLoss(_TimeLoss):
    """-SI-SDR (auraloss.time.SISDRLoss; the metric of models.py:227-255 and a training loss): per row, after removing the row means
    when `zero_mean`, alpha = <x, t> / (|t|^2 + eps) and -10 log10(|alpha t|^2 / (|x - alpha t|^2 + eps) + eps).  `prefilter` is this
    port's keyword (module docstring).  Without a gradient to compute and with reduction="mean", prefilter=None -- the metric path of
    the training step -- it is the two launches rfx_sisdr_sums + rfx_sisdr_finish; the differentiable path returns the same bits."""
    kind = "sisdr"

    def __init__(self, zero_mean=True, eps=1e-8, reduction="mean", prefilter=None):
        super().__init__(zero_mean, eps, reduction, prefilter)

    def forward(self, input, target):
        if self.reduction != "mean" or self.prefilter is not None or (torch.is_grad_enabled() and input.requires_grad):
            return super().forward(input, target)
        with torch.no_grad():
            return self._metric(input, target)

    def _metric(self, input, target):
        _req(input, "input"); _req(target, "target")
        L = input.shape[-1]
        x, t = input.reshape(-1, L), target.reshape(-1, L)
        if x.stride(-1) != 1:
            x = x.contiguous()
        if t.stride(-1) != 1:
            t = t.contiguous()
        R = x.shape[0]
        s = torch.empty((R, 5), device=x.device, dtype=torch.float64)
        ws = scratch("rfx_sisdr_sums_ws", R, L, device=x.device, dtype=torch.float64)       # per-workgroup partials per row
        launch("rfx_sisdr_sums", x, t, R, L, x.stride(0), t.stride(0), ws, s)
        out = torch.empty((), device=x.device, dtype=torch.float32)      # the scalar tail in one launch (fp64 inside)
        launch("rfx_sisdr_finish", s, R, L, 1 if self.zero_mean else 0, float(self.eps), out)
        return out


class SDSDRLoss(_TimeLoss):
    """-SD-SDR (auraloss.time.SDSDRLoss): SI-SDR's scaled target alpha t over the UNSCALED residual x - t."""
    kind = "sdsdr"

    def __init__(self, zero_mean=True, eps=1e-8, reduction="mean", prefilter=None):
        super().__init__(zero_mean, eps, reduction, prefilter)


class SNRLoss(_TimeLoss):
    """-SNR (auraloss.time.SNRLoss): -10 log10(|t|^2 / (|x - t|^2 + eps) + eps) per row, row means removed when `zero_mean`."""
    kind = "snr"

    def __init__(self, zero_mean=True, eps=1e-8, reduction="mean", prefilter=None):
        super().__init__(zero_mean, eps, reduction, prefilter)


class ESRLoss(_TimeLoss):
    """Error-to-signal ratio (auraloss.time.ESRLoss): |t - x|^2 / (|t|^2 + eps) per row.  With prefilter=(-0.85, 1, 0) the
    pre-emphasised ESR of audio-effect modelling."""
    kind = "esr"

    def __init__(self, eps=1e-8, reduction="mean", prefilter=None):
        super().__init__(False, eps, reduction, prefilter)


class DCLoss(_TimeLoss):
    """DC loss (auraloss.time.DCLoss): (mean t - mean x)^2 / (mean t^2 + eps) per row."""
    kind = "dc"

    def __init__(self, eps=1e-8, reduction="mean", prefilter=None):
        super().__init__(False, eps, reduction, prefilter)


class LogCoshLoss(_TimeLoss):
    """Log-cosh loss (auraloss.time.LogCoshLoss): mean_n log(cosh(a (x - t)) + eps) / a per row; elementwise, no prefilter."""
    kind = "logcosh"

    def __init__(self, a=1.0, eps=1e-8, reduction="mean"):
        a = float(a)
        if not (np.isfinite(a) and a > 0.0):
            raise ValueError(f"a={a!r}: a finite positive number")
        super().__init__(False, eps, reduction, None, a)


TIME_LOSSES = {"sisdr": SISDRLoss, "sdsdr": SDSDRLoss, "snr": SNRLoss, "esr": ESRLoss, "dc": DCLoss, "logcosh": LogCoshLoss}


def time_loss(time_loss_kwargs):
    """(module, weight) from the wrappers' `time_loss_kwargs`: a mapping with `name` (one of TIME_LOSSES), `weight` (default 1.0) and
    the class's own keywords -- e.g. `+model.network.time_loss_kwargs.name=sisdr +model.network.time_loss_kwargs.weight=0.1`."""
    kw = dict(time_loss_kwargs)
    name = kw.pop("name", None)
    if name not in TIME_LOSSES:
        raise ValueError(f"time_loss_kwargs.name={name!r}: one of {', '.join(TIME_LOSSES)}")
    weight = float(kw.pop("weight", 1.0))
    if "prefilter" in kw and kw["prefilter"] is not None:
        kw["prefilter"] = tuple(kw["prefilter"])                           # an OmegaConf list from the command line
    return TIME_LOSSES[name](**kw), weight


# ---- perceptual FIR prefilter and the sum / difference stereo loss ---------------------------------------------------
FIR_MAX_TAPS = 1025                                                      # FIR_KMAX of csrc/fir.hip


def a_weighting_taps(fs, ntaps=101):
    """The `ntaps` float64 FIR taps auraloss.perceptual.FIRFilter("aw") builds at sample rate `fs`: the IEC/CD 1672 analog A-weighting
    prototype (poles at f1..f4 = 20.598997, 107.65265, 737.86223, 12194.217 Hz, numerator (2 pi f4)^2 10^(A1000 / 20) s^4 with
    A1000 = 1.9997), scipy.signal.bilinear to a digital IIR, its response at freqz(worN=512), and a least-squares linear-phase fit
    firls(ntaps, w, |h|, fs=fs).  auraloss is not available to pin it: PARITY UNPINNED (the construction is restated from its source).
    The taps are exactly symmetric.  With 101 taps the fit follows the curve to ~0.2 dB from 500 Hz up; BELOW that it cannot: at 100 Hz
    it sits at -16.6 dB against the curve's -19.1 dB.  That is a property of auraloss's design (101 taps span 2 ms), not a defect here."""
    import scipy.signal
    if int(ntaps) != ntaps or ntaps < 1 or ntaps % 2 == 0:
        raise ValueError(f"ntaps={ntaps!r}: an odd positive integer")
    f1, f2, f3, f4, a1000 = 20.598997, 107.65265, 737.86223, 12194.217, 1.9997
    nums = [(2 * np.pi * f4) ** 2 * (10 ** (a1000 / 20)), 0, 0, 0, 0]
    dens = np.polymul([1, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    dens = np.polymul(np.polymul(dens, [1, 2 * np.pi * f3]), [1, 2 * np.pi * f2])
    b, a = scipy.signal.bilinear(nums, dens, fs=fs)
    w_iir, h_iir = scipy.signal.freqz(b, a, worN=512, fs=fs)
    return np.asarray(scipy.signal.firls(int(ntaps), w_iir, np.abs(h_iir), fs=fs), dtype=np.float64)


def _check_taps(taps):
    """An odd number (1 .. FIR_MAX_TAPS) of numbers that are finite in fp32, as a float64 array."""
    try:
        h = np.asarray([float(v) for v in taps], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"taps={taps!r}: an odd-length sequence of finite numbers") from None
    if h.size < 1 or h.size % 2 == 0 or h.size > FIR_MAX_TAPS:
        raise ValueError(f"{h.size} taps: rfx_fir_same takes an odd number of taps, 1 to {FIR_MAX_TAPS}")
    with np.errstate(over="ignore"):
        if not np.isfinite(h.astype(np.float32)).all():
            raise ValueError("taps: every tap must be finite in fp32")
    return h


def _fir_rows(t, name):
    """(..., L) -> R rows of L samples with unit sample stride; a cropped view keeps its row stride (no copy)."""
    _req(t, name)
    if t.dim() < 1 or t.shape[-1] < 1 or t.numel() == 0:
        raise ValueError(f"{name}: the FIR filter needs (..., L) with L >= 1 and at least one row (got {tuple(t.shape)})")
    L = t.shape[-1]
    r = t.reshape(-1, L)
    if r.stride(-1) != 1 or (r.shape[0] > 1 and r.stride(0) < L):
        r = r.contiguous()
    return r


def _fir_launch(sigs, h, flip):
    rows = [_fir_rows(s, "signal") for s in sigs]
    R, L = rows[0].shape
    outs = [torch.empty((R, L), device=r.device, dtype=torch.float32) for r in rows]
    x2, y2 = (rows[1], outs[1]) if len(rows) == 2 else (None, None)
    launch("rfx_fir_same", rows[0], outs[0], x2, y2, R, L, rows[0].stride(0), L, x2.stride(0) if x2 is not None else 0, L, h, h.numel(),
           1 if flip else 0)
    return [o.view(s.shape) for o, s in zip(outs, sigs)]


def fir_same(sigs, h, flip=False):
    """rfx_fir_same on one or two (..., L) fp32 device tensors: y[n] = sum_k h[k] x[n + k - K/2] per row, zeros outside the row --
    F.conv1d(x, h, padding=K // 2) on (R, 1, L); flip=True uses h[K-1-k], the adjoint.  `h`: K fp32 taps on the device, K odd,
    1 <= K <= 1025.  Two signals of one shape share a launch.  Returns new contiguous tensors of the inputs' shapes."""
    sigs = list(sigs)
    if any(s.device != h.device for s in sigs):
        raise ValueError(f"taps on {h.device}, signal on {sigs[0].device}: move the filter with .to(device)")
    if not (h.dtype == torch.float32 and h.dim() == 1 and h.is_contiguous()):
        raise ValueError("taps: a contiguous 1-D fp32 tensor")
    if h.numel() < 1 or h.numel() % 2 == 0 or h.numel() > FIR_MAX_TAPS:
        raise ValueError(f"{h.numel()} taps: rfx_fir_same takes an odd number of taps, 1 to {FIR_MAX_TAPS}")
    if len(sigs) == 2 and sigs[0].shape != sigs[1].shape:
        return _fir_launch(sigs[:1], h, flip) + _fir_launch(sigs[1:], h, flip)
    return _fir_launch(sigs, h, flip)


class _FIRFn(torch.autograd.Function):
    """(input, target) -> (fir(input), fir(target)) in one launch; the backward is the same kernel with flip = 1 on the output
    gradients of the arguments that need one (one launch again when both do)."""

    @staticmethod
    def forward(ctx, input, target, h):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h)
        return tuple(fir_same((input, target), h))

    @staticmethod
    def backward(ctx, g_input, g_target):
        (h,) = ctx.saved_tensors
        want = [g if need else None for g, need in zip((g_input, g_target), ctx.needs_input_grad[:2])]
        done = iter(fir_same([g for g in want if g is not None], h, flip=True)) if any(g is not None for g in want) else None
        return tuple(next(done) if g is not None else None for g in want) + (None,)


class FIRFilter(nn.Module):
    """auraloss.perceptual.FIRFilter with auraloss's keywords: `forward(input, target)` returns both signals filtered, on (..., L)
    fp32 device tensors, differentiable in both.  The conv weights, as upstream (cross-correlation, padding = K // 2):
      "hp"  first-order pre-emphasis   (1, -coef, 0)
      "fd"  folded differentiator      (1, 0, -coef)
      "aw"  A-weighting                a_weighting_taps(fs, ntaps)
    An even `ntaps` or an unknown kind is a ValueError.  `taps=` is this port's keyword: any odd-length (<= 1025) finite sequence, for
    filters auraloss does not name (`filter_type`, `coef`, `ntaps` are then unused).  The taps are a NON-persistent buffer (`.to(device)`
    moves them, checkpoints keep their keys).  One rfx_fir_same launch per call and one per backward.  PARITY UNPINNED (auraloss
    absent); the fp64 reference is tests/fir_ref.py."""

    def __init__(self, filter_type="hp", coef=0.85, fs=44100, ntaps=101, taps=None):
        super().__init__()
        self.filter_type, self.coef, self.fs, self.ntaps = filter_type, coef, fs, ntaps
        if ntaps % 2 == 0:
            raise ValueError(f"ntaps={ntaps!r} must be odd")
        if taps is not None:
            h = _check_taps(taps)
        elif filter_type == "hp":
            h = _check_taps((1.0, -coef, 0.0))
        elif filter_type == "fd":
            h = _check_taps((1.0, 0.0, -coef))
        elif filter_type == "aw":
            h = _check_taps(a_weighting_taps(fs, ntaps))
        else:
            raise ValueError(f"filter_type={filter_type!r}: one of 'hp', 'fd', 'aw'")
        self.register_buffer("taps", torch.from_numpy(h.astype(np.float32)), persistent=False)

    def forward(self, input, target):
        return _FIRFn.apply(input, target, self.taps)


class _SumDiffFn(torch.autograd.Function):
    """(B, 2, T) input and target -> (s_in, d_in, s_tg, d_tg), each (B, 1, T), in one rfx_sum_diff launch; the gradient goes to the
    input only (rfx_sum_diff_adj), as with the MR-STFT loss the four feed."""

    @staticmethod
    def forward(ctx, input, target):
        _req(input, "input"); _req(target, "target")
        x = input if input.stride(-1) == 1 else input.contiguous()
        t = target if target.stride(-1) == 1 else target.contiguous()
        B, _, T = x.shape
        s_in, d_in, s_tg, d_tg = (torch.empty((B, 1, T), device=x.device, dtype=torch.float32) for _ in range(4))
        launch("rfx_sum_diff", x, s_in, d_in, t, s_tg, d_tg, B, T, x.stride(0), x.stride(1), t.stride(0), t.stride(1))
        ctx.mark_non_differentiable(s_tg, d_tg)
        return s_in, d_in, s_tg, d_tg

    @staticmethod
    def backward(ctx, gs, gd, _gs_tg, _gd_tg):
        B, _, T = gs.shape
        gx = torch.empty((B, 2, T), device=gs.device, dtype=torch.float32)
        launch("rfx_sum_diff_adj", gs.contiguous(), gd.contiguous(), gx, B, T)
        return gx, None


class SumAndDifferenceSTFTLoss(nn.Module):
    """auraloss.freq.SumAndDifferenceSTFTLoss: on (B, 2, T) input and target (anything else: ValueError),
        loss = (w_sum * mrstft(L_in + R_in, L_tg + R_tg) + w_diff * mrstft(L_in - R_in, L_tg - R_tg)) / 2
    through ONE inner MultiResolutionSTFTLoss (`self.mrstft`), which takes the remaining keywords: scale="mel" and the term weights
    work through it.  The `/ 2` follows recent auraloss releases (older ones return the unhalved sum); auraloss is absent: PARITY
    UNPINNED.  The gradient goes to the input only."""

    def __init__(self, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, w_sum=1.0, w_diff=1.0, **mrstft_kwargs):
        super().__init__()
        self.w_sum, self.w_diff = float(w_sum), float(w_diff)
        self.mrstft = MultiResolutionSTFTLoss(fft_sizes, hop_sizes, win_lengths, **mrstft_kwargs)

    def forward(self, input, target):
        if input.dim() != 3 or input.shape[1] != 2 or input.shape != target.shape:
            raise ValueError(f"SumAndDifferenceSTFTLoss needs (B, 2, T) input and target (got {tuple(input.shape)}, "
                             f"{tuple(target.shape)})")
        s_in, d_in, s_tg, d_tg = _SumDiffFn.apply(input, target)
        return (self.w_sum * self.mrstft(s_in, s_tg) + self.w_diff * self.mrstft(d_in, d_tg)) / 2


def perceptual_filter(perceptual_kwargs, sample_rate):
    """FIRFilter from the wrappers' `perceptual_kwargs` = {filter_type, coef, ntaps}; `fs` is the wrapper's sample rate -- e.g.
    `+model.network.perceptual_kwargs.filter_type=aw` on the command line."""
    return FIRFilter(fs=sample_rate, **dict(perceptual_kwargs))


def sum_diff_loss(sum_diff_kwargs, channels, **mrstft_kwargs):
    """(module, weight) from the wrappers' `sum_diff_kwargs` = {w_sum, w_diff, weight=1.0}; `channels` = the network's output
    channels."""
    kw = dict(sum_diff_kwargs)
    weight = float(kw.pop("weight", 1.0))
    if channels != 2:
        raise ValueError(f"sum_diff_kwargs needs a two-channel network (this one has {channels} output channel(s))")
    return SumAndDifferenceSTFTLoss(**kw, **mrstft_kwargs), weight
