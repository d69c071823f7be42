"""Pure-torch restatement of the time-domain losses of remfx_amd.losses (auraloss.time SISDRLoss, SDSDRLoss, SNRLoss, ESRLoss, DCLoss,
LogCoshLoss, with this port's optional three-tap prefilter): literal mean / sum / conv1d, gradients by autograd, in the dtype of its
inputs.  Test infrastructure only.  auraloss is not available to pin it (as for oracle/ref_losses.py and tests/mrstft_scaled_ref.py):
this restates the published definitions, PARITY UNPINNED.

Also `closed_form_coefficients`: the per-row (a, b, c) with d loss_r / d x~[n] = a x~[n] + b t~[n] + c from the five row sums, in numpy
fp64 -- what rfx_time_loss_rows computes on the device -- and `sums_form_value`, the table of the ratio losses on those sums."""
import numpy as np
import torch
import torch.nn.functional as F

KINDS = ("sisdr", "sdsdr", "snr", "esr", "dc")


def prefilter(s, taps):
    """s~[n] = h_prev s[n-1] + h_cur s[n] + h_next s[n+1] per row, zeros outside: conv1d with those weights and padding=1."""
    if taps is None:
        return s
    w = torch.tensor(taps, dtype=s.dtype).view(1, 1, 3)
    L = s.shape[-1]
    return F.conv1d(s.reshape(-1, 1, L), w, padding=1).reshape(s.shape)


def row_sums(x, t, taps=None):
    """[R, 5] numpy fp64 { Sx, St, Sxt, Sxx, Stt } of the (filtered) rows."""
    xf, tf = prefilter(x.double(), taps), prefilter(t.double(), taps)
    L = x.shape[-1]
    xf, tf = xf.reshape(-1, L), tf.reshape(-1, L)
    return torch.stack([xf.sum(-1), tf.sum(-1), (xf * tf).sum(-1), (xf * xf).sum(-1), (tf * tf).sum(-1)], -1).numpy()


def _reduce(rows, reduction):
    if reduction == "mean":
        return rows.mean()
    if reduction == "sum":
        return rows.sum()
    assert reduction == "none"
    return rows


def time_loss(kind, x, t, zero_mean=True, eps=1e-8, reduction="mean", taps=None, a=1.0):
    """The literal definitions on (..., L) signals."""
    if kind == "logcosh":
        assert taps is None
        return _reduce((torch.log(torch.cosh(a * (x - t)) + eps) / a).mean(-1), reduction)
    x, t = prefilter(x, taps), prefilter(t, taps)
    if kind == "esr":
        rows = ((t - x) ** 2).sum(-1) / ((t ** 2).sum(-1) + eps)
    elif kind == "dc":
        rows = (t.mean(-1) - x.mean(-1)) ** 2 / ((t ** 2).mean(-1) + eps)
    else:
        if zero_mean:
            x = x - x.mean(-1, keepdim=True)
            t = t - t.mean(-1, keepdim=True)
        if kind == "snr":
            rows = -10.0 * torch.log10((t ** 2).sum(-1) / (((x - t) ** 2).sum(-1) + eps) + eps)
        else:
            alpha = (x * t).sum(-1) / ((t ** 2).sum(-1) + eps)
            st = t * alpha.unsqueeze(-1)
            res = x - st if kind == "sisdr" else x - t
            assert kind in ("sisdr", "sdsdr")
            rows = -10.0 * torch.log10((st ** 2).sum(-1) / ((res ** 2).sum(-1) + eps) + eps)
    return _reduce(rows, reduction)


def _centred(sums, L, zero_mean):
    sx, st, sxt, sxx, stt = [np.asarray(sums, dtype=np.float64)[..., k] for k in range(5)]
    if zero_mean:
        sxt, sxx, stt = sxt - sx * st / L, sxx - sx * sx / L, stt - st * st / L
    return sx, st, sxt, sxx, stt


def sums_form_value(kind, sums, L, zero_mean=True, eps=1e-8):
    """Per-row losses from the five row sums (the table of the loss definitions), numpy fp64."""
    sx, st, sxt, sxx, stt = _centred(sums, L, zero_mean and kind in ("sisdr", "sdsdr", "snr"))
    if kind == "esr":
        return (stt - 2 * sxt + sxx) / (stt + eps)
    if kind == "dc":
        return ((st - sx) / L) ** 2 / (stt / L + eps)
    if kind == "snr":
        return -10 * np.log10(stt / (sxx - 2 * sxt + stt + eps) + eps)
    al = sxt / (stt + eps)
    res = sxx - 2 * al * sxt + al * al * stt if kind == "sisdr" else sxx - 2 * sxt + stt
    return -10 * np.log10(al * al * stt / (res + eps) + eps)


def closed_form_coefficients(kind, sums, L, zero_mean=True, eps=1e-8):
    """[R, 3] numpy fp64 (a, b, c): with f on the (centred) sums, fa = df / dSxx', fb = df / dSxt',
    a = 2 fa, b = fb, c = -(2 fa Sx + fb St) / L when centred (the chain through Sxx' = Sxx - Sx^2 / L, Sxt' = Sxt - Sx St / L), else 0.
    ESR and DC are never centred; DC depends on x through Sx only."""
    zm = bool(zero_mean) and kind in ("sisdr", "sdsdr", "snr")
    sx, st, sxt, sxx, stt = _centred(sums, L, zm)
    k10 = -10.0 / np.log(10.0)
    zero = np.zeros_like(sx)
    if kind == "esr":
        return np.stack([2 / (stt + eps), -2 / (stt + eps), zero], -1)
    if kind == "dc":
        return np.stack([zero, zero, -2 * (st - sx) / L / L / (stt / L + eps)], -1)
    if kind == "snr":
        den = sxx - 2 * sxt + stt + eps
        q = stt / den + eps
        fa = k10 / q * (-stt / den ** 2)
        fb = -2 * fa
    else:
        ia = 1 / (stt + eps)
        al = sxt * ia
        tt, dtt = al * al * stt, 2 * al * stt * ia
        if kind == "sisdr":
            res, dres = sxx - 2 * al * sxt + tt, -2 * al - 2 * sxt * ia + dtt
        else:
            res, dres = sxx - 2 * sxt + stt, -2.0
        den = res + eps
        q = tt / den + eps
        fa = k10 / q * (-tt / den ** 2)
        fb = k10 / q * (dtt * den - tt * dres) / den ** 2
    c = -(2 * fa * sx + fb * st) / L if zm else zero
    return np.stack([2 * fa, fb, c], -1)


def adjoint_gradient(coef, x, t, taps=None):
    """d (sum_r loss_r) / dx from the coefficients: u = a x~ + b t~ + c inside the row, then the ADJOINT of the zero-padded filter,
    gx[n] = h_prev u[n+1] + h_cur u[n] + h_next u[n-1] (u = 0 outside).  x, t: [R, L] fp64."""
    xf, tf = prefilter(x, taps), prefilter(t, taps)
    co = torch.as_tensor(coef, dtype=x.dtype)
    u = co[:, 0:1] * xf + co[:, 1:2] * tf + co[:, 2:3]
    if taps is None:
        return u
    up = F.pad(u, (1, 1))
    return taps[0] * up[:, 2:] + taps[1] * up[:, 1:-1] + taps[2] * up[:, :-2]
