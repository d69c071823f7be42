"""rfx_stft_pair_loss and rfx_fft_synthesis_lossgrad called directly at the three auraloss resolutions, at the smallest shapes that
reach each branch of the two kernels, against torch.stft in float64 on the CPU and the closed-form gradient in float64.

Shapes (R rows of T samples):
  * R = 3 and R = 9: row = slot * 8 + xcd with the `row >= R` early return and a partial last group of 8 rows;
  * T = n_fft + 3 hop: one batch, every frame on the edge path (map_sample), frames_out no multiple of the 2 FB frames of a batch;
  * T = 16 n_fft + 7: interior batches on the prefetched path between two edge batches, and a partial last batch (masked sums / stores);
  * R = 8, n_fft 512 / hop 50, T = 880 000: 17 601 frames = 1101 batches, pair_loss_geometry gives nbatch = 2 -- the only shape here at
    which a workgroup hands the prefetched next batch over to its own next iteration.

Bounds are those of test_gpu_stft.py::test_pair_loss_kernel (spectrum and magnitudes: rms < 2e-6 of the largest spectrum value; row
sums: rtol 2e-5) and ::test_loss_gradient_inside_synthesis (gradient: rms < 1e-6 of the largest gradient value).  The reference uses
the same fp32 window values (cast to float64), so what is compared is the kernels' arithmetic.

The gradient reference is the closed form d[w_sc sqrt(A) / sqrt(B) + w_lm sum |log|X| - log|Y||] / dX evaluated in float64 AT the cells
the forward stored (prediction spectrum, clamped target magnitudes, row sums), taken back to the signal by the float64 adjoint of
torch.stft: what rfx_fft_synthesis_lossgrad computes from those inputs.  (The float64 gradient of the whole loss from the signals is no
reference at this bound: the 1 / |X| and sign terms make it ill-conditioned in the spectrum, and an fp32 torch copy of it is itself
2e-6 .. 6e-5 of the largest value away from float64 at these shapes, the kernels 1e-6 .. 5e-5.)  Measured on MI355X, worst case over
the shapes: spectrum 3.2e-8, magnitudes 3.8e-8 of the largest spectrum value, row sums 5.4e-7 relative; gradient 1.2e-8 of the largest
gradient value or less, except 9.4e-7 at n_fft 1024 / R 3 / T 16391 and 5.4e-7 at T 880 000 (a cell whose |X| - |Y| changes sign
between the fp32 and the float64 magnitude).  The parent commit's kernels give the same figures: results are bit for bit unchanged."""
import ctypes as C

import pytest
import torch

from tests.kernel_harness import GUARD                           # NaN-filled elements on each side of every output buffer

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]               # no GEMM inside: one arithmetic mode
DEV = "cuda:0"
EPS = 1e-8

RES = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]     # auraloss: n_fft, hop, win
CASES = [(n, h, w, R, T) for (n, h, w) in RES for R in (3, 9) for T in (n + 3 * h, 16 * n + 7)] + [(512, 50, 240, 8, 880000)]
_REF = {}


def _ids(c):
    return "n%d_R%d_T%d" % (c[0], c[3], c[4])


def _signals(case):
    n_fft, hop, win, R, T = case
    g = torch.Generator().manual_seed(n_fft + 31 * R + T % 977)
    x = torch.randn(R, T, generator=g) * 0.3
    y = x + 0.1 * torch.randn(R, T, generator=g)
    return x, y


def _reference(case):
    """float64 on the CPU, computed once per case and shared: spectrum of x, clamped magnitudes of y, the three row sums."""
    if case in _REF:
        return _REF[case]
    n_fft, hop, win, R, T = case
    x, y = _signals(case)
    w = torch.hann_window(win, dtype=torch.float32).double()
    X = torch.stft(x.double(), n_fft, hop, win, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(1, 2)   # [R, frames, bins]
    Y = torch.stft(y.double(), n_fft, hop, win, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(1, 2)
    xm = torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=EPS))
    ym = torch.sqrt(torch.clamp(Y.real ** 2 + Y.imag ** 2, min=EPS))
    A = ((ym - xm) ** 2).sum(dim=(1, 2))
    B = (ym ** 2).sum(dim=(1, 2))
    Cs = (torch.log(xm) - torch.log(ym)).abs().sum(dim=(1, 2))
    n = X.shape[1] * X.shape[2]
    w_sc, w_lm = 1.0 / R, 1.0 / (R * n)
    ref = dict(X=torch.view_as_real(X).contiguous(), ym=ym, sums=torch.stack([A, B, Cs], 1), w_sc=w_sc, w_lm=w_lm)
    _REF[case] = ref
    return ref


def _closed_form_gradient(case, X, ym, sums, w_sc, w_lm):
    """float64: the loss gradient at the stored cells (stft_loss_grad_kernel's formula), then the adjoint of torch.stft."""
    n_fft, hop, win, R, T = case
    X, ym, sums = X.cpu().double(), ym.cpu().double(), sums.cpu().double()
    px = X[..., 0] ** 2 + X[..., 1] ** 2
    xm = torch.sqrt(torch.clamp(px, min=EPS))
    A, B = sums[:, 0].view(R, 1, 1), sums[:, 1].view(R, 1, 1)
    ksc = torch.where((A > 0) & (B > 0), w_sc / (torch.sqrt(A) * torch.sqrt(B)), torch.zeros_like(A))
    sc = (ksc * (xm - ym) + w_lm * torch.sign(xm - ym) / xm) / xm
    sc = torch.where(px > EPS, sc, torch.zeros_like(sc))        # clamp(min = eps) passes no gradient below eps
    G = (sc.unsqueeze(-1) * X).transpose(1, 2).contiguous()     # [R, bins, frames, 2]
    w = torch.hann_window(win, dtype=torch.float32).double()
    z = torch.zeros(R, T, dtype=torch.float64, requires_grad=True)
    S = torch.view_as_real(torch.stft(z, n_fft, hop, win, window=w, center=True, pad_mode="reflect", return_complex=True))
    return torch.autograd.grad(S, z, grad_outputs=G)[0]


def _guarded(numel, dtype=torch.float32):
    buf = torch.full((numel + 2 * GUARD,), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + numel:]).all())


def _pair(case, x, y, store):
    from remfx_amd import _lib, stft
    from remfx_amd.ops import _ptr, _stream
    n_fft, hop, win, R, T = case
    frames, bins = 1 + T // hop, n_fft // 2 + 1
    w = stft.hann(win, DEV)
    d = stft._desc(R, T, n_fft, hop, win, bins, 0, frames, 5)
    ws = torch.full((int(_lib.lib().rfx_stft_pair_loss_ws(C.byref(d))),), float("nan"), device=DEV, dtype=torch.float64)
    sbuf, sums = _guarded(3 * R)
    xbuf, X = _guarded(R * frames * bins * 2) if store else (None, None)
    ybuf, ym = _guarded(R * frames * bins) if store else (None, None)
    _lib.check(_lib.lib().rfx_stft_pair_loss(C.byref(d), _ptr(x), _ptr(y), _ptr(w), EPS, _ptr(ws), _ptr(sums), _ptr(X), _ptr(ym),
                                             _stream()), "rfx_stft_pair_loss")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, 3 * R) and not bool(torch.isnan(sums).any())
    if store:
        assert _guards_intact(xbuf, X.numel()) and _guards_intact(ybuf, ym.numel())          # nothing beyond the addressed elements ...
        assert not bool(torch.isnan(X).any()) and not bool(torch.isnan(ym).any())             # ... and every one of them written
        X, ym = X.view(R, frames, bins, 2), ym.view(R, frames, bins)
    return sums.view(R, 3), X, ym


def _lossgrad(case, X, ym, sums, w_sc, w_lm):
    from remfx_amd import _lib, stft
    from remfx_amd.ops import _ptr, _stream
    n_fft, hop, win, R, T = case
    w = stft.hann(win, DEV)
    d = stft._desc(R, T, n_fft, hop, win, X.shape[2], 0, X.shape[1], 5, in_mode=0, herm=0, scale=1.0, accum=0)
    gbuf, gx = _guarded(R * T)
    _lib.check(_lib.lib().rfx_fft_synthesis_lossgrad(C.byref(d), _ptr(X), _ptr(ym), _ptr(sums), w_sc, w_lm, EPS, None, _ptr(w),
                                                     _ptr(stft.syn_ws(d, DEV)), _ptr(gx), _stream()), "rfx_fft_synthesis_lossgrad")
    torch.cuda.synchronize()
    assert _guards_intact(gbuf, R * T) and not bool(torch.isnan(gx).any())                   # every sample stored once, none beyond
    return gx.view(R, T)


def _rms(a, b):
    return float(((a.double() - b.double()) ** 2).mean().sqrt())


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_pair_loss_and_gradient_vs_float64(case):
    """Store launch, no-store launch and the fused-gradient synthesis of one shape against the float64 reference."""
    ref = _reference(case)
    x, y = _signals(case)
    x, y = x.to(DEV), y.to(DEV)
    sums, X, ym = _pair(case, x, y, True)
    sums2, _, _ = _pair(case, x, y, False)
    scale = float(ref["X"].abs().max())
    e_x, e_y = _rms(X.cpu(), ref["X"]), _rms(ym.cpu(), ref["ym"])
    e_s = float(((sums.cpu().double() - ref["sums"]).abs() / ref["sums"].abs()).max())
    print("spectrum rms / scale %.3g, magnitude rms / scale %.3g, row sums max rel %.3g" % (e_x / scale, e_y / scale, e_s))
    assert e_x < 2e-6 * scale
    assert e_y < 2e-6 * scale
    assert torch.allclose(sums.cpu().double(), ref["sums"], rtol=2e-5, atol=0)
    assert torch.equal(sums, sums2)                             # the metric launch (nothing stored) adds the same slots in the same order
    gx = _lossgrad(case, X, ym, sums, ref["w_sc"], ref["w_lm"])
    gref = _closed_form_gradient(case, X, ym, sums, ref["w_sc"], ref["w_lm"])
    gscale = float(gref.abs().max())
    e_g = _rms(gx.cpu(), gref)
    print("gradient rms / scale %.3g" % (e_g / gscale))
    assert gscale > 0 and e_g < 1e-6 * gscale


@pytest.mark.parametrize("res", RES, ids=lambda r: "n%d" % r[0])
def test_identical_signals_give_exact_zero(res):
    """x = y: both transforms run the same instruction sequence, so the difference sums and the gradient are exactly 0."""
    n_fft, hop, win = res
    case = (n_fft, hop, win, 9, 16 * n_fft + 7)
    x = _signals(case)[0].to(DEV)
    sums, X, ym = _pair(case, x, x.clone(), True)
    assert float(sums[:, 0].abs().max()) == 0.0 and float(sums[:, 2].abs().max()) == 0.0 and float(sums[:, 1].min()) > 0.0
    n = X.shape[1] * X.shape[2]
    gx = _lossgrad(case, X, ym, sums, 1.0 / 9, 1.0 / (9 * n))
    assert float(gx.abs().max()) == 0.0
