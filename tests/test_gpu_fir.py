"""GPU: the 'same'-padded FIR kernel (rfx_fir_same), the sum / difference split (rfx_sum_diff, rfx_sum_diff_adj), FIRFilter's autograd,
SumAndDifferenceSTFTLoss and the MR-STFT loss behind FIRFilter("aw") against fp64 references (tests/fir_ref.py composed with
tests/mrstft_scaled_ref.py; auraloss is absent: parity unpinned), and the wrappers' `perceptual_kwargs` / `sum_diff_kwargs` under
RFX_STRICT_NATIVE=1.

The FIR bound is derived, not tuned (tests/fir_ref.py: fir_bound): per sample |y - y64| <= (K + 2) 2^-24 sum_k |h_k| |x_(n+k-K/2)| +
2^-126 with the sum in fp64 -- it holds for any fp32 summation order, with or without FMA.  The kernel's tile is 2048 samples, so the
lengths 2047 / 2048 / 2049 / 4097 straddle it, and 49 / 50 / 51 straddle K // 2 of the 101-tap filter (a row shorter than a halo)."""
import functools

import numpy as np
import pytest
import torch

from tests import fir_ref
from tests import mrstft_scaled_ref as mref

pytestmark = pytest.mark.gpu                  # `one_mode`: no GEMM inside, the arithmetic modes agree; the wrapper steps run in each
DEV = "cuda:0"

KS = (1, 3, 101, 255, 1025)
LS = (1, 2, 49, 50, 51, 2047, 2048, 2049, 4097)
SENTINEL = -777.0


@functools.lru_cache(maxsize=None)
def _taps(K, kind):
    """fp32 taps (CPU): random magnitudes with random signs, or auraloss's A-weighting design at 48 kHz."""
    if kind == "aw":
        from remfx_amd import losses
        return torch.from_numpy(losses.a_weighting_taps(48000, K).astype(np.float32))
    g = torch.Generator().manual_seed(1000 + K)
    return (torch.rand(K, generator=g) + 0.1) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1).float()


def _signal(R, L, seed, pad=0):
    """(R, L) fp32 on the CPU; with pad: a cropped view of an (R, L + pad) tensor -- row stride > L, a start that is not 16-byte
    aligned."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(R, L + pad, generator=g)
    return big, (big[:, 3:3 + L] if pad else big)


def _launch(x, h, flip, x2=None, out_pad=0):
    """rfx_fir_same straight through the C ABI: x (and x2) (R, L) device views with any row stride; the outputs are views into
    sentinel-filled (R, L + out_pad) buffers.  Returns the output buffers (whole, to check nothing outside the views was written)."""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    R, L = x.shape
    bufs = [torch.full((R, L + out_pad), SENTINEL, device=DEV) for _ in range(2 if x2 is not None else 1)]
    views = [b[:, 1:1 + L] if out_pad else b for b in bufs]
    rc = _lib.lib().rfx_fir_same(_ptr(x), _ptr(views[0]), _ptr(x2), _ptr(views[1] if x2 is not None else None), R, L, x.stride(0),
                                 views[0].stride(0), x2.stride(0) if x2 is not None else 0,
                                 views[1].stride(0) if x2 is not None else 0, _ptr(h), h.numel(), flip, _stream())
    assert rc == 0, rc
    return bufs, views


@pytest.mark.one_mode
@pytest.mark.parametrize("K", KS)
def test_fir_same_vs_fp64_reference(K):
    """Every L x R x flip x layout x tap set at one K; the cropped layout also writes through a strided output view and checks the
    columns beside it keep their sentinel.  The second signal of the two-signal form is the first one negated and reversed in row
    order, checked against its own reference; in the cropped layout it is a cropped view as well, with its own row stride."""
    worst = 0.0
    kinds = ("random", "aw") if K >= 3 else ("random",)
    for kind in kinds:
        h = _taps(K, kind)
        hd = h.to(DEV)
        for L in LS:
            for R in (1, 3):
                for pad in (0, 13):
                    big, x = _signal(R, L, 7 * L + R, pad)
                    bigd = big.to(DEV)
                    xd = bigd[:, 3:3 + L] if pad else bigd
                    x2 = -x.flip(0)
                    if pad:                                            # the second signal cropped too, at another offset and stride
                        big2d = torch.zeros(R, L + 22, device=DEV)
                        big2d[:, 5:5 + L] = x2.to(DEV)
                        x2d = big2d[:, 5:5 + L]
                    else:
                        x2d = x2.contiguous().to(DEV)
                    for flip in (0, 1):
                        bufs, views = _launch(xd, hd, flip, x2d, out_pad=5 if pad else 0)
                        for src, buf, view in zip((x, x2), bufs, views):
                            want, bound = fir_ref.fir_same(src, h, bool(flip)), fir_ref.fir_bound(src, h, bool(flip))
                            err = (view.cpu().double() - want).abs()
                            assert bool((err <= bound).all()), (kind, K, L, R, pad, flip, float((err / bound).max()))
                            worst = max(worst, float((err / bound).max()))
                            if pad:
                                assert bool((buf[:, 0] == SENTINEL).all()) and bool((buf[:, 1 + L:] == SENTINEL).all())
                        one, v1 = _launch(xd, hd, flip, None, out_pad=5 if pad else 0)     # the one-signal form: the same bits
                        assert torch.equal(v1[0], views[0])
    print(f"\nFIR_PARITY K={K}: worst |y - y64| / bound = {worst:.3f}")


@pytest.mark.one_mode
def test_refused_arguments():
    from remfx_amd import _lib, losses
    from remfx_amd.ops import _ptr, _stream
    x = torch.zeros(2, 64, device=DEV)
    y = torch.empty_like(x)
    for K in (0, 2, 100, 1027):
        h = torch.ones(max(K, 1), device=DEV)
        assert _lib.lib().rfx_fir_same(_ptr(x), _ptr(y), None, None, 2, 64, 64, 64, 0, 0, _ptr(h), K, 0, _stream()) != 0
        if K:
            with pytest.raises(ValueError, match="1025"):
                losses.fir_same([x], h)
    h = torch.ones(3, device=DEV)
    assert _lib.lib().rfx_fir_same(_ptr(x), _ptr(y), None, None, 2, 64, 64, 64, 0, 0, _ptr(h), 3, 2, _stream()) != 0      # flip
    assert _lib.lib().rfx_fir_same(_ptr(x), _ptr(y), None, None, 2, 64, 32, 64, 0, 0, _ptr(h), 3, 0, _stream()) != 0      # rows overlap
    assert _lib.lib().rfx_fir_same(_ptr(x), _ptr(y), _ptr(x), None, 2, 64, 64, 64, 64, 64, _ptr(h), 3, 0, _stream()) != 0  # half a pair
    with pytest.raises(ValueError, match="fp32"):
        losses.FIRFilter().to(DEV)(x.double(), x.double())
    with pytest.raises(ValueError, match="device"):
        losses.FIRFilter()(x, x)                                       # the taps were left on the CPU


@pytest.mark.one_mode
@pytest.mark.parametrize("flip", (0, 1))
def test_rows_are_isolated(flip):
    """R = 3, L = 50 < K // 2 + 1 with K = 101, the middle row all NaN: rows 0 and 2 equal their single-row results bit for bit."""
    hd = _taps(101, "random").to(DEV)
    _, x = _signal(3, 50, 11)
    x[1] = float("nan")
    xd = x.to(DEV)
    _, (y,) = _launch(xd, hd, flip)
    for r in (0, 2):
        _, (single,) = _launch(xd[r:r + 1].clone(), hd, flip)
        assert torch.equal(y[r], single[0]) and bool(torch.isfinite(y[r]).all())
    assert bool(torch.isnan(y[1]).all())


@pytest.mark.one_mode
@pytest.mark.parametrize("K", (3, 101, 1025))
def test_flip_is_the_adjoint(K):
    """<fir(x), g> and <x, fir_flip(g)>, both in fp64 from the device outputs, agree to 2 (K + 2) 2^-24 sum |h| sum_n |x_n| max |g|."""
    h = _taps(K, "random")
    hd = h.to(DEV)
    for L in (50, 2049):
        _, x = _signal(3, L, 21 + K)
        _, g = _signal(3, L, 22 + K)
        _, (y,) = _launch(x.to(DEV), hd, 0)
        _, (z,) = _launch(g.to(DEV), hd, 1)
        lhs = float((y.cpu().double() * g.double()).sum())
        rhs = float((x.double() * z.cpu().double()).sum())
        tol = 2 * (K + 2) * 2.0 ** -24 * float(h.double().abs().sum()) * float(x.double().abs().sum()) * float(g.abs().max())
        print(f"\nFIR_ADJOINT K={K} L={L}: {lhs:.9f} {rhs:.9f} diff {abs(lhs - rhs):.3e} tol {tol:.3e}")
        assert abs(lhs - rhs) <= tol
        if K <= 101:                                                   # the check can tell the adjoint from the filter itself
            _, (wrong,) = _launch(g.to(DEV), hd, 0)
            assert abs(lhs - float((x.double() * wrong.cpu().double()).sum())) > tol


@pytest.mark.one_mode
def test_two_launches_are_bit_equal():
    hd = _taps(101, "aw").to(DEV)
    _, x = _signal(3, 4097, 31)
    xd = x.to(DEV)
    for flip in (0, 1):
        _, (a,) = _launch(xd, hd, flip)
        _, (b,) = _launch(xd, hd, flip)
        assert torch.equal(a, b)


@pytest.mark.one_mode
def test_fir_filter_autograd():
    """FIRFilter("aw") on (2, 1, 2049) signals, the target a cropped view: outputs and both gradients against fp64 autograd of the
    reference, the gradient under the same per-sample bound with the upstream gradient in place of the signal; with only the input
    requiring a gradient the target's is None and the backward filters one signal."""
    from remfx_amd import losses
    filt = losses.FIRFilter("aw", fs=48000).to(DEV)
    assert not filt.state_dict() and filt.taps.device.type == "cuda"
    h = filt.taps.cpu()
    _, x = _signal(2, 2049, 41)
    _, t = _signal(2, 2049, 42, pad=13)
    _, gi = _signal(2, 2049, 43)
    _, gt = _signal(2, 2049, 44)
    x, t, gi, gt = (v.reshape(2, 1, 2049) for v in (x, t, gi, gt))
    xd = x.to(DEV).requires_grad_(True)
    tbig = torch.zeros(2, 1, 2049 + 13, device=DEV)
    tbig[..., 3:3 + 2049] = t.to(DEV)
    tleaf = tbig.requires_grad_(True)
    yi, yt = filt(xd, tleaf[..., 3:3 + 2049])
    assert yi.shape == x.shape and yt.shape == t.shape
    for got, src in ((yi, x), (yt, t)):
        assert bool(((got.detach().cpu().double() - fir_ref.fir_same(src, h)).abs() <= fir_ref.fir_bound(src, h)).all())
    ((yi * gi.to(DEV)).sum() + (yt * gt.to(DEV)).sum()).backward()
    x64, t64 = x.double().requires_grad_(True), t.double().requires_grad_(True)
    ((fir_ref.fir_same(x64, h) * gi.double()).sum() + (fir_ref.fir_same(t64, h) * gt.double()).sum()).backward()
    for got, want, g in ((xd.grad, x64.grad, gi), (tleaf.grad[..., 3:3 + 2049], t64.grad, gt)):
        assert bool(((got.cpu().double() - want).abs() <= fir_ref.fir_bound(g, h, True)).all())
    assert float(tleaf.grad[..., :3].abs().max()) == 0.0 and float(tleaf.grad[..., 3 + 2049:].abs().max()) == 0.0
    # only the input needs a gradient
    calls = []
    xd2, td2 = x.to(DEV).requires_grad_(True), t.to(DEV)
    yi, yt = filt(xd2, td2)
    orig = losses._fir_launch
    try:
        losses._fir_launch = lambda sigs, hh, flip: (calls.append((len(sigs), flip)), orig(sigs, hh, flip))[1]
        ((yi * gi.to(DEV)).sum() + (yt * gt.to(DEV)).sum()).backward()
    finally:
        losses._fir_launch = orig
    assert calls == [(1, True)] and td2.grad is None and torch.equal(xd2.grad, xd.grad)


@pytest.mark.one_mode
@pytest.mark.parametrize("T", (1, 255, 2048, 4097))
def test_sum_diff_and_adjoint_bit_equal(T):
    """IEEE add has one answer: s, d and the adjoint equal the fp32 torch expressions bit for bit -- contiguous and cropped inputs; 2048 takes
    the 16-byte path, the other lengths the dword path."""
    from remfx_amd import losses
    g = torch.Generator().manual_seed(50 + T)
    for pad in (0, 5):
        big = torch.randn(3, 2, T + pad, generator=g).to(DEV)
        x = big[..., 2:2 + T] if pad else big
        t = torch.randn(3, 2, T, generator=g).to(DEV)
        xl = x.detach().clone().requires_grad_(True) if not pad else x.requires_grad_(False)
        s_in, d_in, s_tg, d_tg = losses._SumDiffFn.apply(xl, t)
        for got, want in ((s_in, x[:, 0] + x[:, 1]), (d_in, x[:, 0] - x[:, 1]), (s_tg, t[:, 0] + t[:, 1]), (d_tg, t[:, 0] - t[:, 1])):
            assert got.shape == (3, 1, T) and torch.equal(got[:, 0], want)
        if not pad:
            gs, gd = torch.randn(3, 1, T, generator=g).to(DEV), torch.randn(3, 1, T, generator=g).to(DEV)
            ((s_in * gs).sum() + (d_in * gd).sum()).backward()
            assert torch.equal(xl.grad[:, 0], (gs + gd)[:, 0]) and torch.equal(xl.grad[:, 1], (gs - gd)[:, 0])
            assert not s_tg.requires_grad and not d_tg.requires_grad


# ---- the composites: value and input gradient against the fp64 restatements ------------------------------------------------------------
# The scalar `a` (one fp32 CPU evaluation against fp64) can come out far below fp32 resolution by cancellation -- it then says nothing
# about what an fp32 evaluation may be off by.  The device returns the loss as ONE fp32 number, whose rounding alone is up to 2^-24
# relative, so `a` is taken as at least that: the value bound is max(4 a, 2^-22), the form tests/test_gpu_time_loss.py uses.
VALUE_FLOOR = 2.0 ** -22


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def _pair(C):
    g = torch.Generator().manual_seed(60 + C)
    x = torch.randn(2, C, 6000, generator=g) * 0.3
    if C == 2:
        x[:, 1] = 0.7 * x[:, 0] + 0.3 * x[:, 1]                    # a correlated pair: sum and difference differ in level
    return x, x + 0.1 * torch.randn(2, C, 6000, generator=g)


def _ref_sumdiff(x, y, w_sum, w_diff):
    s = mref.mrstft_loss(x[:, 0:1] + x[:, 1:2], y[:, 0:1] + y[:, 1:2])
    d = mref.mrstft_loss(x[:, 0:1] - x[:, 1:2], y[:, 0:1] - y[:, 1:2])
    return (w_sum * s + w_diff * d) / 2


def _ref_aw(x, y, h):
    K = h.numel()
    f = lambda v: torch.nn.functional.conv1d(v.reshape(-1, 1, v.shape[-1]), h.to(v.dtype).view(1, 1, K), padding=K // 2).reshape(v.shape)
    return mref.mrstft_loss(f(x), f(y))


def _value_and_grad(fn, x, y, dt):
    xr = x.clone().to(dt).requires_grad_(True)                 # a copy: .to() of an fp32 tensor is the tensor itself
    l = fn(xr, y.to(dt))
    l.backward()
    return float(l.detach()), xr.grad.double()


@pytest.mark.one_mode
def test_sum_and_difference_loss_vs_fp64_restatement():
    """(2, 2, 6000), the three default resolutions, w_sum = 1, w_diff = 2.  Tolerance as tests/test_gpu_mrstft_scaled.py: a = the fp32
    restatement's own error against its fp64 run; the device must be within 4 a (relative for the scalar, and there never below
    VALUE_FLOOR; RMS relative to the gradient's RMS for the gradient).  The split adds nothing to it: s and d are the very floats torch
    computes.  (2, 1, 6000) is a ValueError."""
    from remfx_amd import losses
    x, y = _pair(2)
    fn = lambda a, b: _ref_sumdiff(a, b, 1.0, 2.0)
    l64, g64 = _value_and_grad(fn, x, y, torch.float64)
    l32, g32 = _value_and_grad(fn, x, y, torch.float32)
    a_l, a_g = abs(l32 - l64) / abs(l64), _rms(g32 - g64) / _rms(g64)
    mod = losses.SumAndDifferenceSTFTLoss(w_sum=1.0, w_diff=2.0).to(DEV)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    l = mod(xd, yd)
    (l * 1.7).backward()
    e_l, e_g = abs(float(l) - l64) / abs(l64), _rms(xd.grad.cpu().double() / 1.7 - g64) / _rms(g64)
    print(f"\nSUMDIFF_PARITY: loss {float(l):.8f} ref64 {l64:.10f}  err {e_l:.3e} a {a_l:.3e} | grad err {e_g:.3e} a {a_g:.3e}")
    assert yd.grad is None                                              # the gradient goes to the input only
    plain = losses.MultiResolutionSTFTLoss()(xd.detach(), yd.detach())
    assert abs(float(plain) - l64) > 1e-3 * abs(l64)                    # ... and it is not the per-channel loss
    assert e_l <= max(4 * a_l, VALUE_FLOOR), (e_l, a_l)
    assert e_g <= 4 * a_g, (e_g, a_g)
    m, s = _pair(1)
    with pytest.raises(ValueError, match=r"\(B, 2, T\)"):
        mod(m.to(DEV), s.to(DEV))


@pytest.mark.one_mode
@pytest.mark.parametrize("C", (1, 2))
def test_mrstft_behind_a_weighting_vs_fp64_restatement(C):
    """MultiResolutionSTFTLoss()(*FIRFilter("aw", fs=48000)(x, y)) on (2, 1, 6000) and (2, 2, 6000) against the fp64 restatement
    composed with the fp64 filter.  Tolerance: max(4 a, VALUE_FLOOR) for the value and 4 a for the gradient as above, a = the
    composite's own fp32-against-fp64 error.  `shift` is printed
    beside it: how far the fp64 loss moves when it is fed the device-filtered signals instead of the fp64-filtered ones (DESIGN.md
    4.3c records it); it did not have to be added to the bound."""
    from remfx_amd import losses
    filt = losses.FIRFilter("aw", fs=48000).to(DEV)
    h = filt.taps.cpu()
    x, y = _pair(C)
    fn = lambda a, b: _ref_aw(a, b, h)
    l64, g64 = _value_and_grad(fn, x, y, torch.float64)
    l32, g32 = _value_and_grad(fn, x, y, torch.float32)
    a_l, a_g = abs(l32 - l64) / abs(l64), _rms(g32 - g64) / _rms(g64)
    xd = x.to(DEV).requires_grad_(True)
    fx, fy = filt(xd, y.to(DEV))
    l = losses.MultiResolutionSTFTLoss()(fx, fy)
    (l * 1.7).backward()
    e_l, e_g = abs(float(l) - l64) / abs(l64), _rms(xd.grad.cpu().double() / 1.7 - g64) / _rms(g64)
    shift = abs(float(mref.mrstft_loss(fx.detach().cpu().double(), fy.detach().cpu().double())) - l64) / abs(l64)
    print(f"\nAW_MRSTFT_PARITY C={C}: loss {float(l):.8f} ref64 {l64:.10f}  err {e_l:.3e} a {a_l:.3e} shift {shift:.3e} | "
          f"grad err {e_g:.3e} a {a_g:.3e}")
    unfiltered = losses.MultiResolutionSTFTLoss()(xd.detach(), y.to(DEV))
    assert abs(float(unfiltered) - l64) > 1e-3 * abs(l64)
    assert e_l <= max(4 * a_l, VALUE_FLOOR), (e_l, a_l, shift)
    assert e_g <= 4 * a_g, (e_g, a_g)


# ---- the wrappers, under RFX_STRICT_NATIVE=1 -------------------------------------------------------------------------------------------
TCN = dict(sample_rate=48000, num_bins=1025, ninputs=1, noutputs=1, nblocks=3, channel_width=8, kernel_size=7, stack_size=10,
           dilation_growth=2, causal=False)
HD = dict(sample_rate=48000, sources=["mixture"], audio_channels=2, nfft=4096, channels=8)


def _step(cls, base, extra, shape):
    from remfx_amd import models
    torch.manual_seed(3)
    net = getattr(models, cls)(**dict(base, **extra)).to(DEV)
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(*shape, generator=g) * 0.2).to(DEV)
    x = y + 0.1 * torch.randn(*shape, generator=g).to(DEV)
    loss, out = net((x, y))
    loss.backward()
    dead = sorted(n for n, p in net.named_parameters() if p.grad is None)
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert all(bool(torch.isfinite(gr).all()) for gr in grads) and bool(torch.isfinite(loss))
    return net, loss.detach(), torch.cat([gr.reshape(-1) for gr in grads]), dead


@pytest.mark.parametrize("cls,base,extra,shape", [("TCNModel", TCN, {"perceptual_kwargs": {"filter_type": "aw"}}, (2, 1, 16384)),
                                                  ("DemucsModel", HD, {"sum_diff_kwargs": {}}, (2, 2, 20000))],
                         ids=["tcn_aw", "hdemucs_sumdiff"])
def test_wrapper_keywords_train_under_strict_native(monkeypatch, cls, base, extra, shape):
    """A small step with the new keyword: finite loss, a finite gradient on every parameter, a loss that differs from the plain
    wrapper's -- and the plain wrapper's loss, computed in the same process before and after the new modules were built and run, is
    torch.equal to itself (same seed, same bits: the default path does not see the new code).  "Every parameter" is every parameter
    the network's forward reaches: Hybrid Demucs carries one GroupNorm its forward never calls (time_encoder.4.norm1, also without a
    gradient in the CPU oracle), so the parameters without a gradient must be exactly that layer's, with and without the keyword."""
    from remfx_amd import losses, nnops
    monkeypatch.setenv("RFX_STRICT_NATIVE", "1")
    nnops.INTERIM.clear()
    plain, l0, g0, dead0 = _step(cls, base, {}, shape)
    assert plain.perceptual is None and plain.sumdiff is None
    net, l1, g1, dead1 = _step(cls, base, extra, shape)
    assert dead1 == dead0 == ([] if cls == "TCNModel" else ["model.time_encoder.4.norm1.bias", "model.time_encoder.4.norm1.weight"])
    assert isinstance(net.perceptual, losses.FIRFilter) or isinstance(net.sumdiff, losses.SumAndDifferenceSTFTLoss)
    assert float(l1) != float(l0) and float((g1 - g0).abs().max()) > 1e-6 * float(g0.abs().max())
    _, l2, _, _ = _step(cls, base, {}, shape)
    assert torch.equal(l0, l2)
    assert not nnops.INTERIM
