"""GPU: the time-domain training losses (rfx_time_sums, rfx_time_loss_rows, rfx_time_loss_grad, rfx_logcosh_rows, rfx_logcosh_grad behind
SISDRLoss / SDSDRLoss / SNRLoss / ESRLoss / DCLoss / LogCoshLoss) against the pure-torch restatement (tests/time_loss_ref.py; auraloss
is absent: parity unpinned), forward and gradient, plus what the kernels and the unchanged default path promise.

Tolerance of the parity cases (DESIGN 4.3a's convention): `a` = the error of the restatement's own fp32 run against its fp64 run on the
same inputs (relative for the value -- the largest over the rows with reduction="none" -- and RMS relative to the gradient's RMS for
the gradient); the device must be within max(4 a, 2^-22).  The floor: the device sums in fp64 and rounds once, so it can beat the fp32
restatement, and 4 a alone could then fall below one fp32 rounding of the result times the upstream multiply.  Every case prints both
figures before it asserts."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import time_loss_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]          # no GEMM inside the losses: one arithmetic mode
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FLOOR = 2.0 ** -22
PRE, ASYM = (-0.85, 1.0, 0.0), (0.3, 1.0, -0.5)
UP_SCALAR, UP_ROWS = 1.7, (1.7, -0.6, 2.3)

# shape name -> (R, L) contiguous, or the cropped view base[..., 5:20000] of a (3, 1, 20011) tensor (row stride != L, start misaligned
# by 20 bytes).  1003: L % 4 != 0;  5: shorter than any vector or halo;  70001 > 128 slots * 256 = 32768: every workgroup wraps
# its grid-stride loop and there is a tail
SHAPES = {"3x1003": (3, 1003), "1x5": (1, 5), "2x70001": (2, 70001), "crop": None}


def _cases():
    out = []
    for kind in ("sisdr", "sdsdr", "snr", "esr", "dc", "logcosh"):
        for red in ("mean", "sum", "none"):
            for zm in ((True, False) if kind in ("sisdr", "sdsdr", "snr") else (False,)):
                out.append((kind, "3x1003", red, zm, None))
    for shape in ("1x5", "2x70001", "crop"):
        out += [("sisdr", shape, "mean", True, None), ("esr", shape, "none", False, PRE), ("logcosh", shape, "sum", False, None)]
    out += [("sisdr", "3x1003", "none", True, ASYM), ("snr", "crop", "mean", False, ASYM), ("sdsdr", "2x70001", "sum", True, ASYM),
            ("dc", "3x1003", "mean", False, PRE), ("dc", "1x5", "none", False, ASYM), ("esr", "3x1003", "mean", False, ASYM)]
    return out


CASES = _cases()


def _id(c):
    kind, shape, red, zm, taps = c
    return f"{kind}-{shape}-{red}-{'zm' if zm else 'raw'}-{'none' if taps is None else ('pre' if taps == PRE else 'asym')}"


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    g = torch.Generator().manual_seed(sum(map(ord, shape)))
    if shape == "crop":
        bx = torch.randn(3, 1, 20011, generator=g) * 0.3 + 0.05
        by = bx + 0.1 * torch.randn(3, 1, 20011, generator=g)
        return bx, by
    R, L = SHAPES[shape]
    x = torch.randn(R, L, generator=g) * 0.3 + 0.05
    return x, x + 0.1 * torch.randn(R, L, generator=g)


def _view(t, shape):
    return t[..., 5:20000] if shape == "crop" else t


def _module(kind, red, zm, taps):
    from remfx_amd import losses
    kw = dict(reduction=red)
    if kind in ("sisdr", "sdsdr", "snr"):
        kw["zero_mean"] = zm
    if kind != "logcosh":
        kw["prefilter"] = taps
    return losses.TIME_LOSSES[kind](**kw)


def _upstream(l, red):
    if red != "none":
        return l * UP_SCALAR
    v = torch.tensor(UP_ROWS, dtype=l.dtype, device=l.device)[:l.numel()].view(l.shape)
    return (l * v).sum()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(value64, grad64, a_value, a_grad): the fp64 restatement (with the upstream factor in the gradient) and the fp32 restatement's
    own error against it.  Computed once per case and shared."""
    kind, shape, red, zm, taps = case
    x, y = _inputs(shape)
    out = []
    for dt in (torch.float64, torch.float32):
        xb = x.clone().to(dt).requires_grad_(True)           # a copy: x.to(float32) is x itself
        l = ref.time_loss(kind, _view(xb, shape), _view(y.to(dt), shape), zero_mean=zm, reduction=red, taps=taps)
        _upstream(l, red).backward()
        out.append((l.detach().double(), _view(xb.grad, shape).double()))
    (l64, g64), (l32, g32) = out
    return l64, g64, float(((l32 - l64).abs() / l64.abs()).max()), _rms(g32 - g64) / _rms(g64)


def _device(case, x=None, y=None):
    kind, shape, red, zm, taps = case
    if x is None:
        x, y = _inputs(shape)
    xb = x.to(DEV).requires_grad_(True)
    l = _module(kind, red, zm, taps)(_view(xb, shape), _view(y.to(DEV), shape))
    _upstream(l, red).backward()
    return l.detach(), _view(xb.grad, shape)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_value_and_gradient_vs_fp64_restatement(case):
    """Measured on an MI355X.  Value: relative error of the device | a, the fp32 restatement's own; gradient: RMS error relative to
    the gradient's RMS, device | a.  Bound max(4 a, 2^-22 = 2.4e-07) each.  Case = kind-shape-reduction-centring-prefilter.
        sisdr-3x1003-mean-zm-none      2.716e-08 | 2.716e-08      3.812e-08 | 1.712e-07
        sisdr-3x1003-mean-raw-none     5.809e-09 | 5.809e-09      3.768e-08 | 1.119e-07
        sisdr-3x1003-sum-zm-none       5.811e-09 | 5.811e-09      3.855e-08 | 1.600e-07
        sisdr-3x1003-sum-raw-none      5.809e-09 | 5.809e-09      3.769e-08 | 1.072e-07
        sisdr-3x1003-none-zm-none      4.865e-08 | 5.406e-08      3.585e-08 | 1.581e-07
        sisdr-3x1003-none-raw-none     2.273e-08 | 2.273e-08      3.500e-08 | 1.211e-07
        sdsdr-3x1003-mean-zm-none      3.614e-08 | 6.751e-08      3.782e-08 | 1.822e-07
        sdsdr-3x1003-mean-raw-none     2.338e-08 | 7.870e-08      3.794e-08 | 8.857e-08
        sdsdr-3x1003-sum-zm-none       1.590e-09 | 6.751e-08      3.806e-08 | 1.459e-07
        sdsdr-3x1003-sum-raw-none      2.338e-08 | 1.127e-07      3.682e-08 | 6.539e-08
        sdsdr-3x1003-none-zm-none      2.200e-08 | 1.031e-07      3.734e-08 | 1.159e-07
        sdsdr-3x1003-none-raw-none     4.133e-08 | 1.373e-07      3.495e-08 | 6.028e-08
        snr-3x1003-mean-zm-none        8.928e-09 | 8.928e-09      3.750e-08 | 1.453e-07
        snr-3x1003-mean-raw-none       4.152e-10 | 4.152e-10      3.806e-08 | 9.032e-08
        snr-3x1003-sum-zm-none         2.259e-08 | 4.045e-08      3.756e-08 | 1.454e-07
        snr-3x1003-sum-raw-none        4.152e-10 | 4.152e-10      3.787e-08 | 7.817e-08
        snr-3x1003-none-zm-none        4.172e-08 | 9.350e-08      3.515e-08 | 1.197e-07
        snr-3x1003-none-raw-none       1.783e-08 | 1.783e-08      3.439e-08 | 5.219e-08
        esr-3x1003-mean-raw-none       3.785e-08 | 1.158e-07      3.695e-08 | 6.971e-08
        esr-3x1003-sum-raw-none        1.410e-08 | 8.980e-08      3.766e-08 | 6.104e-08
        esr-3x1003-none-raw-none       3.915e-08 | 9.666e-08      3.521e-08 | 6.246e-08
        dc-3x1003-mean-raw-none        2.445e-08 | 4.708e-06      6.121e-08 | 2.720e-06
        dc-3x1003-sum-raw-none         5.572e-09 | 4.738e-06      6.266e-08 | 2.759e-06
        dc-3x1003-none-raw-none        2.972e-08 | 1.258e-05      1.724e-08 | 2.481e-06
        logcosh-3x1003-mean-raw-none   2.931e-08 | 1.920e-06      3.783e-08 | 6.572e-08
        logcosh-3x1003-sum-raw-none    2.931e-08 | 1.950e-06      3.764e-08 | 8.513e-08
        logcosh-3x1003-none-raw-none   2.919e-08 | 2.234e-06      3.452e-08 | 6.965e-08
        sisdr-1x5-mean-zm-none         5.478e-09 | 1.205e-07      4.845e-08 | 2.310e-07
        esr-1x5-none-raw-pre           1.286e-08 | 1.286e-08      4.623e-08 | 8.713e-08
        logcosh-1x5-sum-raw-none       2.211e-08 | 1.823e-07      2.258e-08 | 7.608e-08
        sisdr-2x70001-mean-zm-none     4.595e-08 | 5.435e-08      3.774e-08 | 1.592e-07
        esr-2x70001-none-raw-pre       3.521e-08 | 1.527e-07      3.897e-08 | 1.319e-07
        logcosh-2x70001-sum-raw-none   7.881e-09 | 2.065e-06      3.778e-08 | 5.775e-08
        sisdr-crop-mean-zm-none        3.829e-08 | 6.154e-08      3.748e-08 | 1.480e-07
        esr-crop-none-raw-pre          3.562e-08 | 3.746e-08      3.509e-08 | 1.476e-07
        logcosh-crop-sum-raw-none      1.400e-09 | 1.999e-06      3.783e-08 | 8.624e-08
        sisdr-3x1003-none-zm-asym      4.576e-08 | 4.576e-08      3.363e-08 | 2.088e-07
        snr-crop-mean-raw-asym         1.007e-08 | 1.007e-08      3.785e-08 | 2.077e-07
        sdsdr-2x70001-sum-zm-asym      1.005e-08 | 1.005e-08      3.780e-08 | 1.948e-07
        dc-3x1003-mean-raw-pre         3.910e-08 | 5.566e-05      3.256e-08 | 3.823e-05
        dc-1x5-none-raw-asym           1.667e-08 | 8.141e-08      3.752e-08 | 8.376e-08
        esr-3x1003-mean-raw-asym       3.244e-08 | 1.089e-07      3.729e-08 | 1.791e-07
    Where the two value figures are equal the device returned the very float the fp32 restatement did.  The device's figures are one
    fp32 rounding of an fp64 result (<= 6e-8) in every case; a is large for DC (the squared difference of two nearly equal means) and
    for log-cosh's value (log of cosh ~ 1 + y^2 / 2 in fp32), where the device's fp64 evaluation does not share the cancellation."""
    l64, g64, a_l, a_g = _reference(case)
    l, g = _device(case)
    assert l.dtype == torch.float32 and tuple(l.shape) == tuple(l64.shape) and tuple(g.shape) == tuple(g64.shape)
    e_l = float(((l.cpu().double() - l64).abs() / l64.abs()).max())
    e_g = _rms(g.cpu().double() - g64) / _rms(g64)
    print(f"\nTIME_PARITY {_id(case)}: value err {e_l:.3e} a {a_l:.3e} | grad err {e_g:.3e} a {a_g:.3e}")
    assert bool(torch.isfinite(g).all())
    assert e_l <= max(4 * a_l, FLOOR), (_id(case), e_l, a_l)
    assert e_g <= max(4 * a_g, FLOOR), (_id(case), e_g, a_g)


@pytest.mark.parametrize("kind,taps", [("esr", PRE), ("sisdr", ASYM)])
def test_rows_are_isolated_under_a_prefilter(kind, taps):
    """Contiguous (3, 1003) with row 1 a thousand times louder: one sample of it leaking into the halo of row 0 or 2 would change their
    sum of squares a thousandfold.  Rows 0 and 2 meet the parity bound, value and gradient."""
    x, y = _inputs("3x1003")
    x, y = x.clone(), y.clone()
    x[1] *= 1e3
    y[1] *= 1e3
    res = []
    for dt in (torch.float64, torch.float32):
        xb = x.clone().to(dt).requires_grad_(True)
        l = ref.time_loss(kind, xb, y.to(dt), reduction="none", taps=taps)
        _upstream(l, "none").backward()
        res.append((l.detach().double(), xb.grad.double()))
    (l64, g64), (l32, g32) = res
    l, g = _device((kind, "3x1003", "none", True, taps), x, y)
    l, g = l.cpu().double(), g.cpu().double()
    for r in (0, 2):
        a_l, a_g = float((l32[r] - l64[r]).abs() / l64[r].abs()), _rms(g32[r] - g64[r]) / _rms(g64[r])
        e_l, e_g = float((l[r] - l64[r]).abs() / l64[r].abs()), _rms(g[r] - g64[r]) / _rms(g64[r])
        print(f"\nTIME_ISOLATION {kind} row {r}: value err {e_l:.3e} a {a_l:.3e} | grad err {e_g:.3e} a {a_g:.3e}")
        assert e_l <= max(4 * a_l, FLOOR) and e_g <= max(4 * a_g, FLOOR), (kind, r, e_l, a_l, e_g, a_g)


def _device_sums_and_coef(x, y, kind, zm, taps):
    from remfx_amd import _lib, losses
    from remfx_amd.ops import _ptr, _stream
    R, L = x.shape
    L_ = _lib.lib()
    h = taps if taps is not None else (0.0, 1.0, 0.0)
    s = torch.empty((R, 5), device=DEV, dtype=torch.float64)
    ws = torch.empty(int(L_.rfx_time_sums_ws(R, L)), device=DEV, dtype=torch.float64)
    _lib.check(L_.rfx_time_sums(_ptr(x), _ptr(y), R, L, x.stride(0), y.stride(0), 1 if taps is not None else 0, h[0], h[1], h[2],
                                _ptr(ws), _ptr(s), _stream()), "rfx_time_sums")
    rows = torch.empty((R,), device=DEV, dtype=torch.float32)
    coef = torch.empty((R, 3), device=DEV, dtype=torch.float64)
    out = torch.empty((), device=DEV, dtype=torch.float32)
    _lib.check(L_.rfx_time_loss_rows(_ptr(s), R, L, losses.TIME_KINDS[kind], 1 if zm else 0, 1e-8, 0, _ptr(rows), _ptr(coef), _ptr(out),
                                     _stream()), "rfx_time_loss_rows")
    return s.cpu().numpy(), coef.cpu().numpy(), rows.cpu(), out.cpu()


@pytest.mark.parametrize("taps", (None, ASYM), ids=("none", "asym"))
@pytest.mark.parametrize("zm", (True, False), ids=("zm", "raw"))
@pytest.mark.parametrize("kind", ref.KINDS)
def test_device_coefficients_match_the_closed_form(kind, zm, taps):
    """The device's (a, b, c) against closed_form_coefficients on the device's OWN sums, relative 1e-12: a and b against their own
    magnitude; c = -(a Sx + b St) / L is a difference of two terms, so against (|a Sx| + |b St|) / L (DC: its own magnitude)."""
    x, y = _inputs("3x1003")
    sums, coef, rows, out = _device_sums_and_coef(x.to(DEV), y.to(DEV), kind, zm, taps)
    L = x.shape[-1]
    want = ref.closed_form_coefficients(kind, sums, L, zm)
    err = np.abs(coef - want)
    scale_c = np.abs(want[:, 2]) if kind == "dc" else (np.abs(want[:, 0] * sums[:, 0]) + np.abs(want[:, 1] * sums[:, 1])) / L
    print(f"\nTIME_COEF {kind} zm={zm} taps={taps}: max rel err a {np.max(err[:, 0] / np.maximum(np.abs(want[:, 0]), 1e-300)):.2e} "
          f"b {np.max(err[:, 1] / np.maximum(np.abs(want[:, 1]), 1e-300)):.2e} c {np.max(err[:, 2] / np.maximum(scale_c, 1e-300)):.2e}")
    assert (err[:, 0] <= 1e-12 * np.abs(want[:, 0])).all() and (err[:, 1] <= 1e-12 * np.abs(want[:, 1])).all()
    assert (err[:, 2] <= 1e-12 * scale_c).all()
    if kind in ("esr", "dc") or not zm:
        assert (coef[:, 2] == 0).all() or kind == "dc"
    val = ref.sums_form_value(kind, sums, L, zm)
    assert np.abs(rows.numpy() - val).max() <= 2.0 ** -23 * np.abs(val).max()           # one fp32 rounding of the fp64 value
    assert abs(float(out) - val.mean()) <= 2.0 ** -23 * abs(val.mean())


def test_sums_without_taps_are_the_sisdr_sums():
    """rfx_time_sums without taps: the kernel, grid and bits of rfx_sisdr_sums (contiguous and cropped rows)."""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    for shape in ("2x70001", "crop"):
        x, y = _inputs(shape)
        x, y = _view(x.to(DEV), shape), _view(y.to(DEV), shape)
        L = x.shape[-1]
        x, y = x.reshape(-1, L), y.reshape(-1, L)
        R = x.shape[0]
        assert x.stride(0) == (L if shape != "crop" else 20011)
        s = torch.empty((R, 5), device=DEV, dtype=torch.float64)
        nws = int(_lib.lib().rfx_sisdr_sums_ws(R, L))
        assert nws == 5 * R * 128
        ws = torch.empty(nws, device=DEV, dtype=torch.float64)
        _lib.check(_lib.lib().rfx_sisdr_sums(_ptr(x), _ptr(y), R, L, x.stride(0), y.stride(0), _ptr(ws), _ptr(s), _stream()), "sums")
        got = _device_sums_and_coef(x, y, "sisdr", True, None)[0]
        assert np.array_equal(got, s.cpu().numpy())


def test_euler_identity_of_sisdr():
    """SI-SDR does not change when the prediction is scaled, so <grad, x> = 0: a check that needs no restatement."""
    from remfx_amd import losses
    x, y = _inputs("2x70001")
    xb = (x - x.mean(-1, keepdim=True)).to(DEV).requires_grad_(True)
    losses.SISDRLoss(zero_mean=True)(xb, y.to(DEV)).backward()
    g, xd = xb.grad.double(), xb.detach().double()
    dot, bound = abs(float((g * xd).sum())), 1e-5 * float(g.norm()) * float(xd.norm())
    print(f"\nTIME_EULER |<g, x>| {dot:.3e}  bound {bound:.3e}")
    assert dot <= bound


def _legacy_sisdr(x, y, zero_mean=True, eps=1e-8):
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    L = x.shape[-1]
    x2, y2 = x.reshape(-1, L), y.reshape(-1, L)
    R = x2.shape[0]
    s = torch.empty((R, 5), device=DEV, dtype=torch.float64)
    nws = int(_lib.lib().rfx_sisdr_sums_ws(R, L))
    assert nws == 5 * R * 128
    ws = torch.empty(nws, device=DEV, dtype=torch.float64)
    _lib.check(_lib.lib().rfx_sisdr_sums(_ptr(x2), _ptr(y2), R, L, x2.stride(0), y2.stride(0), _ptr(ws), _ptr(s), _stream()), "sums")
    out = torch.empty((), device=DEV, dtype=torch.float32)
    _lib.check(_lib.lib().rfx_sisdr_finish(_ptr(s), R, L, 1 if zero_mean else 0, eps, _ptr(out), _stream()), "finish")
    return out


@pytest.mark.parametrize("shape", ("3x1003", "2x70001", "crop"))
def test_sisdr_metric_path_is_unchanged(shape, monkeypatch):
    """SISDRLoss()(x.detach(), y): exactly the two launches rfx_sisdr_sums + rfx_sisdr_finish (behind the one host-only query that
    sizes the workspace of the first) and their bits; the differentiable path (rfx_time_sums + rfx_time_loss_rows) returns the same bits."""
    from remfx_amd import _lib, losses
    x, y = _inputs(shape)
    x, y = _view(x.to(DEV), shape), _view(y.to(DEV), shape)
    for zm in (True, False):
        want = _legacy_sisdr(x, y, zm)
        assert torch.equal(losses.SISDRLoss(zero_mean=zm)(x.detach(), y), want)
        with torch.no_grad():
            assert torch.equal(losses.SISDRLoss(zero_mean=zm)(x.clone().requires_grad_(True), y), want)
        assert torch.equal(losses.SISDRLoss(zero_mean=zm)(x.clone().requires_grad_(True), y).detach(), want)
    calls = []
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name.startswith("rfx_") and callable(fn):
                def wrapped(*a, _fn=fn, _n=name):
                    calls.append(_n)
                    return _fn(*a)
                return wrapped
            return fn

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    losses.SISDRLoss()(x.detach(), y)
    assert calls == ["rfx_sisdr_sums_ws", "rfx_sisdr_sums", "rfx_sisdr_finish"], calls


def test_same_bits_on_two_streams():
    """Slot stores and fixed-order sums: value and gradient on two different streams are torch.equal."""
    res = []
    for case in (("sisdr", "2x70001", "mean", True, ASYM), ("logcosh", "2x70001", "none", False, None)):
        per = []
        for _ in range(2):
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                l, g = _device(case)
            st.synchronize()
            per.append((l, g.clone()))
        res.append(per)
    for (la, ga), (lb, gb) in res:
        assert torch.equal(la, lb) and torch.equal(ga, gb)


TCN = dict(sample_rate=48000, num_bins=1025, ninputs=1, noutputs=1, nblocks=3, channel_width=8, kernel_size=7, stack_size=10,
           dilation_growth=2, causal=False)


def _tcn_step(time_loss_kwargs):
    from remfx_amd import models
    torch.manual_seed(3)
    kw = dict(TCN, time_loss_kwargs=time_loss_kwargs) if time_loss_kwargs is not None else TCN
    net = models.TCNModel(**kw).to(DEV)
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(2, 1, 16384, generator=g) * 0.2).to(DEV)
    x = y + 0.1 * torch.randn(2, 1, 16384, generator=g).to(DEV)
    loss, out = net((x, y))
    tgt = models.causal_crop(y, out.shape[-1])
    assert out.shape[-1] < y.shape[-1]                     # the cropped (strided, misaligned) target of the TCN wrapper
    loss.backward()
    flat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    return net, loss.detach(), out.detach(), tgt, flat


def test_wrapper_default_is_unchanged_and_time_term_adds():
    """Without `time_loss_kwargs` the wrapper's loss is mrstft + 100 l1, bit for bit; with {"name": "sisdr", "weight": 0.1} it is the
    hand sum with that term, and the term reaches the parameters' gradient."""
    from remfx_amd import losses
    net, loss, out, tgt, flat0 = _tcn_step(None)
    assert net.timeloss is None
    assert torch.equal(loss, net.mrstftloss(out, tgt) + net.l1loss(out, tgt) * 100)
    net, loss, out, tgt, flat1 = _tcn_step({"name": "sisdr", "weight": 0.1})
    assert isinstance(net.timeloss, losses.SISDRLoss)
    assert torch.equal(loss, net.mrstftloss(out, tgt) + net.l1loss(out, tgt) * 100 + losses.SISDRLoss()(out, tgt) * 0.1)
    assert bool(torch.isfinite(flat1).all()) and flat0.shape == flat1.shape
    assert float((flat1 - flat0).abs().max()) > 1e-6 * float(flat0.abs().max())


def test_train_script_with_time_loss(tmp_path):
    """scripts/train.py, two steps, with the time-domain term switched on from the command line (a fresh child process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "+exp=reverb", "model=tcn",
                        "model.network.nblocks=3", "model.network.channel_width=16", "chunk_size=16384",
                        "datamodule.train_batch_size=2", "datamodule.train_dataset.total_chunks=4",
                        "datamodule.val_dataset.total_chunks=2", "datamodule.test_dataset.total_chunks=2", "trainer.max_steps=2",
                        "+model.network.time_loss_kwargs.name=sisdr", "+model.network.time_loss_kwargs.weight=0.1",
                        f"logs_dir={tmp_path}", f"logger.save_dir={tmp_path}"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "train_loss" in r.stdout
    import csv
    import glob
    import math
    files = glob.glob(os.path.join(tmp_path, "lightning_logs", "*", "metrics.csv"))
    assert len(files) == 1
    with open(files[0]) as f:
        vals = [float(row["train_loss"]) for row in csv.DictReader(f) if row.get("train_loss")]
    assert vals and all(math.isfinite(v) for v in vals), vals
