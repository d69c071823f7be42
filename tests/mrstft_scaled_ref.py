"""Pure-torch restatement of auraloss.freq.STFTLoss / MultiResolutionSTFTLoss with a frequency scale and the three magnitude term
weights, plus librosa.filters.mel as a literal loop, for tests/test_mrstft_scaled_cpu.py and tests/test_gpu_mrstft_scaled.py.
Test infrastructure only.

auraloss and librosa are not available to pin it (as for oracle/ref_losses.py): this restates the published algorithms, PARITY
UNPINNED.

  STFTLoss.forward:  |X| = sqrt(clamp(re^2 + im^2, min=eps)) of torch.stft(hann window, center, reflect);
                     scale="mel":  |X| <- fb @ |X|,  fb = librosa.filters.mel(sr=sample_rate, n_fft=fft_size, n_mels=n_bins);
                     sc  = mean_r ||My - Mx||_F / ||My||_F          (auraloss >= 0.4; older: one norm over the batch tensor)
                     lm  = mean |log Mx - log My|,   lin = mean |Mx - My|
                     loss = w_sc sc + w_log_mag lm + w_lin_mag lin  (a term whose weight is 0 is not evaluated)
  MultiResolutionSTFTLoss.forward: the mean over the resolutions.
  librosa.filters.mel defaults: htk=False (Slaney scale: 200 / 3 Hz per mel below 1 kHz, log step ln(6.4) / 27 above), fmin=0,
                     fmax=sr / 2, norm="slaney" (2 / (f[i + 2] - f[i])), dtype float32 (the weight array is fp32 from the start).

Runs in the dtype of its inputs (fp32 or fp64); gradients come from torch autograd.
"""
import math

import numpy as np
import torch

F_SP = 200.0 / 3
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = MIN_LOG_HZ / F_SP
LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    if f >= MIN_LOG_HZ:
        return MIN_LOG_MEL + math.log(f / MIN_LOG_HZ) / LOGSTEP
    return f / F_SP


def mel_to_hz(m):
    if m >= MIN_LOG_MEL:
        return MIN_LOG_HZ * math.exp(LOGSTEP * (m - MIN_LOG_MEL))
    return F_SP * m


def librosa_mel(sr, n_fft, n_mels):
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels), loop by loop."""
    bins = 1 + n_fft // 2
    weights = np.zeros((n_mels, bins), dtype=np.float32)
    fftfreqs = [k * sr / n_fft for k in range(bins)]                       # np.fft.rfftfreq(n_fft, 1 / sr)
    lo, hi = hz_to_mel(0.0), hz_to_mel(sr / 2.0)
    mel_f = [mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    for i in range(n_mels):
        for k in range(bins):
            lower = -(mel_f[i] - fftfreqs[k]) / (mel_f[i + 1] - mel_f[i])
            upper = (mel_f[i + 2] - fftfreqs[k]) / (mel_f[i + 2] - mel_f[i + 1])
            weights[i, k] = max(0.0, min(lower, upper))
    for i in range(n_mels):
        enorm = 2.0 / (mel_f[i + 2] - mel_f[i])
        for k in range(bins):
            weights[i, k] = np.float32(np.float64(weights[i, k]) * enorm)
    return weights


def unpack_banded(idx, w, cols):
    """The dense matrix of losses.pack_banded's (idx, w)."""
    idx, w = np.asarray(idx), np.asarray(w)
    d = np.zeros((idx.shape[0], cols), dtype=np.float32)
    for r, (first, ln, off) in enumerate(idx):
        d[r, first:first + ln] = w[off:off + ln]
    return d


def stft_mag(x, n_fft, hop, win, eps=1e-8):
    X = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=x.dtype), return_complex=True)
    return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=eps))      # (R, bins, frames)


def stft_loss(inp, tgt, n_fft, hop, win, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, scale=None, n_bins=None, sample_rate=None,
              per_example_sc=True, eps=1e-8):
    L = inp.shape[-1]
    xm = stft_mag(inp.reshape(-1, L), n_fft, hop, win, eps)
    ym = stft_mag(tgt.reshape(-1, L), n_fft, hop, win, eps)
    if scale == "mel":
        fb = torch.from_numpy(librosa_mel(sample_rate, n_fft, n_bins)).to(xm.dtype).unsqueeze(0)
        xm, ym = torch.matmul(fb, xm), torch.matmul(fb, ym)
    elif scale is not None:
        raise ValueError(scale)
    loss = 0.0
    if w_sc:
        if per_example_sc:
            sc = (torch.linalg.norm(ym - xm, dim=(-2, -1)) / torch.linalg.norm(ym, dim=(-2, -1))).mean()
        else:
            sc = torch.linalg.norm((ym - xm).reshape(-1)) / torch.linalg.norm(ym.reshape(-1))
        loss = loss + w_sc * sc
    if w_log_mag:
        loss = loss + w_log_mag * (torch.log(xm) - torch.log(ym)).abs().mean()
    if w_lin_mag:
        loss = loss + w_lin_mag * (xm - ym).abs().mean()
    return loss


def mrstft_loss(inp, tgt, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), **kw):
    tot = 0.0
    for f, h, w in zip(fft_sizes, hop_sizes, win_lengths):
        tot = tot + stft_loss(inp, tgt, f, h, w, **kw)
    return tot / len(fft_sizes)
