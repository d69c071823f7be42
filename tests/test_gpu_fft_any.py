"""GPU parity of the generic framed FFT (remfx_amd/csrc/fft_any.hip): STFT / iSTFT forward and backward and everything built on them
at the power-of-two n_fft the four-size kernels of csrc/fft.hip do not cover, against torch.stft / torch.istft and torch autograd
in fp64 on the CPU, and tests/mrstft_scaled_ref.py for the loss.  Cases, references and bounds: tests/fft_any_ref.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import fft_any_ref as ref
from tests.conftest import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ISTFT_GEOMS = sorted(set(ref.GEOMS + [(n, n // 4, n) for n in ref.NEW_SIZES]))    # every one meets torch.istft's envelope condition


@pytest.mark.one_mode
@pytest.mark.parametrize("case", ref.CASES)
def test_forward_all_modes(case):
    from remfx_amd import stft
    n_fft, hop, win, L = case
    r64, r32, scale = ref.forward_refs(n_fft, hop, win, L)
    xd = ref.signal(n_fft, hop, L).to(DEV)
    got = {m: stft.stft(xd, n_fft, hop, win, mode=m, eps=ref.EPS, alpha=ref.ALPHA).detach() for m in ref.MODES}
    assert torch.equal(got["complex"].permute(0, 2, 1, 3), got["complex_fm"])
    bad = []
    for m in ref.MODES:
        assert got[m].shape == r64[m].shape, m
        err, own, bound = ref.rms(got[m].cpu(), r64[m]), ref.rms(r32[m], r64[m]), ref.fwd_bound(m, n_fft, scale)
        print(f"n_fft={n_fft} hop={hop} win={win} L={L} {m}: device error {err:.3e}, fp32 torch.stft error {own:.3e}, bound {bound:.3e}")
        if not err < bound:
            bad.append((m, err, bound))
    assert not bad, bad


@pytest.mark.one_mode
@pytest.mark.parametrize("mode", ["complex", "complex_fm"])
@pytest.mark.parametrize("case", ref.CASES)
def test_stft_backward(case, mode):
    from remfx_amd import stft
    n_fft, hop, win, L = case
    x = ref.signal(n_fft, hop, L)
    xr = x.double().requires_grad_(True)
    out = ref.mode_ref(ref.stft_ref(xr, n_fft, hop, win), mode)
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (out * gy).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    (stft.stft(xd, n_fft, hop, win, mode=mode) * gy.float().to(DEV)).sum().backward()
    err, bound = ref.rms(xd.grad.cpu(), xr.grad), 5e-6 * float(xr.grad.abs().max()) * ref.growth(n_fft)
    print(f"n_fft={n_fft} hop={hop} win={win} L={L} {mode}: gradient error {err:.3e}, bound {bound:.3e}")
    assert err < bound


@pytest.mark.one_mode
@pytest.mark.parametrize("geom", ISTFT_GEOMS)
def test_istft_and_backward(geom):
    from remfx_amd import stft
    n_fft, hop, win = geom
    L = 3 * n_fft + 7
    x = ref.signal(n_fft, hop, L)
    spec = stft.stft(x.to(DEV), n_fft, hop, win, mode="complex").detach()                     # (R, bins, frames, 2)
    w64 = torch.hann_window(win, dtype=torch.float64)
    zc = torch.view_as_complex(spec.cpu().double().contiguous()).requires_grad_(True)
    want = torch.istft(zc, n_fft, hop, win, w64)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    (want * go).sum().backward()
    gref = torch.view_as_real(zc.grad)
    sd = spec.clone().requires_grad_(True)
    got = stft.istft(sd, n_fft, hop, win, mode="complex")
    assert got.shape == want.shape
    e1 = ref.rms(got.detach().cpu(), want.detach())
    e2 = ref.rms(got.detach().cpu(), x[:, :got.shape[1]])
    (got * go.float().to(DEV)).sum().backward()
    e3, b3 = ref.rms(sd.grad.cpu(), gref), 5e-6 * float(gref.abs().max()) * ref.growth(n_fft)
    print(f"n_fft={n_fft} hop={hop} win={win}: istft error {e1:.3e} (bound {2e-6 * float(want.abs().max()):.3e}), reconstruction "
          f"{e2:.3e}, gradient {e3:.3e} (bound {b3:.3e})")
    assert e1 < 2e-6 * float(want.abs().max())
    assert e2 < 1e-5
    assert e3 < b3
    fm = spec.permute(0, 2, 1, 3).contiguous()                                                # the other two spectrum layouts
    cac = spec.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(stft.istft(fm, n_fft, hop, win, mode="complex_fm"), got.detach())
    assert torch.equal(stft.istft(cac, n_fft, hop, win, mode="cac"), got.detach())


@pytest.mark.one_mode
def test_descriptor_fields_at_a_new_size():
    """HDemucs' _spec (extra reflect pad, normalized, Nyquist dropped, frames [2 : 2 + le]) and _ispec at n_fft = 256, hop = 64."""
    from remfx_amd import stft
    nfft, hl, T, Rr = 256, 64, 1000, 2
    le, pad = math.ceil(T / hl), hl // 2 * 3
    g = torch.Generator().manual_seed(3)
    x = 0.3 * torch.randn(Rr, T, generator=g)
    w64 = torch.hann_window(nfft, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    xp = F.pad(xr.unsqueeze(1), (pad, pad + le * hl - T), mode="reflect").squeeze(1)
    z = torch.stft(xp, nfft, hl, window=w64, win_length=nfft, normalized=True, center=True, return_complex=True, pad_mode="reflect")
    assert z.shape[-1] == le + 4
    z = z[:, :-1, 2:2 + le]                                                                   # (R, 128, le)
    zr = torch.stack((z.real, z.imag), 1)                                                     # cac (R, 2, 128, le)
    gz = torch.randn(zr.shape, generator=g, dtype=torch.float64)
    (zr * gz).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    cac = stft.stft(xd, nfft, hl, mode="cac", normalized=True, bins=nfft // 2, frame0=2, frames_out=le,
                    extra_pad=(pad, pad + le * hl - T))
    assert cac.shape == (Rr, 2, nfft // 2, le)
    assert ref.rms(cac.detach().cpu(), zr.detach()) < 2e-6 * float(zr.abs().max())
    (cac * gz.float().to(DEV)).sum().backward()
    assert ref.rms(xd.grad.cpu(), xr.grad) < 5e-6 * float(xr.grad.abs().max())
    # inverse
    zin = torch.randn(Rr, nfft // 2, le, 2, generator=g, dtype=torch.float64)
    zc = torch.view_as_complex(zin.clone()).requires_grad_(True)
    full = F.pad(F.pad(zc, (0, 0, 0, 1)), (2, 2))
    lp = hl * math.ceil(T / hl) + 2 * pad
    xo = torch.istft(full, nfft, hl, window=w64, win_length=nfft, normalized=True, length=lp, center=True)[:, pad:pad + T]
    go = torch.randn(xo.shape, generator=g, dtype=torch.float64)
    (xo * go).sum().backward()
    cin = zin.permute(0, 3, 1, 2).float().contiguous().to(DEV).requires_grad_(True)          # (R, 2, 128, le)
    got = stft.istft(cin, nfft, hl, mode="cac", normalized=True, frames=le + 4, frame0=2, crop=pad, length=T)
    assert got.shape == (Rr, T)
    assert ref.rms(got.detach().cpu(), xo.detach()) < 2e-6 * float(xo.abs().max())
    (got * go.float().to(DEV)).sum().backward()
    gref = torch.view_as_real(zc.grad).permute(0, 3, 1, 2)
    assert ref.rms(cin.grad.cpu(), gref) < 5e-6 * float(gref.abs().max())


def _mr_device_grad(variant):
    from remfx_amd import losses
    x, y = ref.loss_signals()
    xd = x.to(DEV).requires_grad_(True)
    l = losses.MultiResolutionSTFTLoss(**ref.MR, **ref.MR_VARIANTS[variant])(xd, y.to(DEV))
    (l * ref.MR_UPSTREAM).backward()                      # upstream gradient != 1: the device-side gup path
    return float(l), xd.grad.detach()


@pytest.mark.one_mode
@pytest.mark.parametrize("variant", sorted(ref.MR_VARIANTS))
def test_mrstft_loss_micro_tcn_resolutions(variant):
    from remfx_amd import losses
    x, _ = ref.loss_signals()
    lref, gref = ref.loss_ref(variant)
    l, grad = _mr_device_grad(variant)
    e, s = ref.rms(grad.cpu(), gref), float(gref.abs().max())
    print(f"{variant}: loss {l:.7f} vs {lref:.7f}, gradient error {e:.3e}, bound {1e-4 * s:.3e}")
    assert abs(l - lref) < 1e-4 * abs(lref)
    assert e < 1e-4 * s
    xd = x.to(DEV).requires_grad_(True)
    l0 = losses.MultiResolutionSTFTLoss(**ref.MR, **ref.MR_VARIANTS[variant])(xd, x.to(DEV).clone())
    l0.backward()
    assert float(l0) == 0.0 and float(xd.grad.abs().max()) == 0.0


@pytest.mark.one_mode
def test_reproducible():
    """Ownership, not atomics: the same launch twice gives the same bits, whatever else was allocated in between."""
    from remfx_amd import stft
    _, g1 = _mr_device_grad("default")
    junk = torch.full((3, 1 << 20), 3.0, device=DEV)
    _, g2 = _mr_device_grad("default")
    assert torch.equal(g1, g2)
    for n_fft in (16, 32768):
        hop, L = n_fft // 4, 3 * n_fft + 7
        spec = stft.stft(ref.signal(n_fft, hop, L).to(DEV), n_fft, hop, mode="complex").detach()
        a = stft.istft(spec, n_fft, hop, mode="complex")
        junk = torch.full((5, 1 << 19), float(n_fft), device=DEV)
        b = stft.istft(spec, n_fft, hop, mode="complex")
        assert torch.equal(a, b), n_fft
    del junk


def test_mel_spectrogram_256():
    from remfx_amd import classifier
    g = torch.Generator().manual_seed(9)
    x = 0.3 * torch.randn(2, 1, 4001, generator=g)
    X = ref.stft_ref(x.reshape(2, 4001), 256, 64, 256)
    p = X.real ** 2 + X.imag ** 2                                                             # (2, 129, frames)
    fb = classifier.melscale_fbanks(129, 0.0, 8000.0, 40, 16000).double()                     # (129, 40)
    want = torch.matmul(p.transpose(1, 2), fb).transpose(1, 2).unsqueeze(1)                   # (2, 1, 40, frames)
    got = classifier.MelSpectrogram(16000, n_fft=256, hop_length=64, n_mels=40).to(DEV)(x.to(DEV))
    assert got.shape == want.shape
    scale = float(X.abs().max())
    err = ref.rms(got.cpu(), want)
    print(f"mel spectrogram: error {err:.3e}, bound {4e-6 * scale * scale:.3e}")
    check(err, 4e-6, scale * scale, what="mel spectrogram n_fft=256")   # the power-mode bound; the mel product is a GEMM (bf16 mode: conftest)
