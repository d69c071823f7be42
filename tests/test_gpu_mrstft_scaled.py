"""GPU parity: the mel-scaled / weighted MR-STFT loss (rfx_stft_scaled_loss, rfx_stft_scaled_loss_grad, rfx_mrstft_combine_w) against
the pure-torch restatement of auraloss (tests/mrstft_scaled_ref.py; auraloss / librosa are absent: parity unpinned), forward and
gradient, plus the properties the default path and the slot sums promise.

Tolerance of the parity cases: `a` = the error of the restatement's own fp32 run against its fp64 run on the same inputs (relative
for the scalar, RMS relative to the gradient's RMS for the gradient); the device must be within 4 a (a different summation order and
the fused sqrt / log).  Every case prints both figures before it asserts."""
import functools

import pytest
import torch

from tests import mrstft_scaled_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GEOM = {1024: (1024, 120, 600), 2048: (2048, 240, 1200), 512: (512, 50, 240)}
# name: (fft sizes, scale, n_bins, (w_sc, w_log_mag, w_lin_mag), per_example_sc, R, L, silence)       L % hop != 0 everywhere
CASES = {
    "mel1024x64": ((1024,), "mel", 64, (1.0, 1.0, 0.0), True, 5, 12007, False),
    "mel2048x128_w_batchsc_r1": ((2048,), "mel", 128, (0.5, 2.0, 1.0), False, 1, 12007, False),
    "mel_multires_batchsc": ((2048, 1024), "mel", 64, (1.0, 1.0, 1.0), False, 5, 9001, False),
    "mel1024x64_silence": ((1024,), "mel", 64, (1.0, 1.0, 0.0), True, 5, 12007, True),
    "linear_lin1": ((1024, 2048, 512), None, None, (1.0, 1.0, 1.0), True, 5, 9001, False),
    "linear_w_batchsc_r1": ((1024, 512), None, None, (0.5, 2.0, 1.0), False, 1, 12007, False),
    "linear_w_r5": ((2048,), None, None, (0.5, 2.0, 1.0), True, 5, 9001, False),
}
MEL_CASES = [k for k, v in CASES.items() if v[1] == "mel"]


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def _inputs(name):
    ffts, scale, n_bins, wts, pe, R, L, silence = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(R, 1, L, generator=g) * 0.3
    y = x + 0.1 * torch.randn(R, 1, L, generator=g)
    if silence:                                    # exact-zero stretches of the prediction, longer than a frame: the eps clamp
        x[:, :, 2000:5000] = 0.0
        x[1, :, 7000:] = 0.0
        x[3] = 0.0
    return x, y


def _kw(name):
    ffts, scale, n_bins, wts, pe, R, L, silence = CASES[name]
    return dict(w_sc=wts[0], w_log_mag=wts[1], w_lin_mag=wts[2], scale=scale, n_bins=n_bins,
                sample_rate=48000 if scale else None, per_example_sc=pe)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(loss64, grad64, a_loss, a_grad): the fp64 restatement and the fp32 restatement's own error against it."""
    ffts = CASES[name][0]
    x, y = _inputs(name)
    out = []
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).requires_grad_(True)
        l = ref.mrstft_loss(xr, y.to(dt), ffts, [GEOM[f][1] for f in ffts], [GEOM[f][2] for f in ffts], **_kw(name))
        l.backward()
        out.append((float(l.detach()), xr.grad.double()))
    (l64, g64), (l32, g32) = out
    return l64, g64, abs(l32 - l64) / abs(l64), _rms(g32 - g64) / _rms(g64)


def _module(name):
    from remfx_amd import losses
    ffts = CASES[name][0]
    return losses.MultiResolutionSTFTLoss(fft_sizes=ffts, hop_sizes=[GEOM[f][1] for f in ffts], win_lengths=[GEOM[f][2] for f in ffts],
                                          **_kw(name)).to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_scaled_loss_and_gradient_vs_fp64_restatement(name):
    """Measured on an MI355X, f32 mode (the loss has no GEMM inside: the modes agree).  Scalar: relative error of the device | a, the
    fp32 restatement's own; gradient: RMS error relative to the gradient's RMS, device | a.  Bound 4 a each.
        mel1024x64                 6.8e-09 | 9.8e-08      4.0e-07 | 4.6e-07
        mel2048x128_w_batchsc_r1   5.3e-08 | 5.3e-08      2.9e-07 | 4.4e-07
        mel_multires_batchsc       3.0e-08 | 6.5e-08      2.8e-07 | 2.6e-07
        mel1024x64_silence         7.0e-08 | 7.0e-08      2.4e-04 | 2.4e-04
        linear_lin1                4.9e-08 | 4.9e-08      1.9e-03 | 1.3e-03
        linear_w_batchsc_r1        1.9e-08 | 1.9e-08      2.5e-04 | 1.7e-04
        linear_w_r5                2.1e-08 | 2.1e-08      8.4e-05 | 1.8e-04
    Where the two scalar figures are equal the device returned the very float the fp32 restatement did (row sums and the scalar
    tail are fp64 on the device; the fp32 result is the last rounding).  The gradient figures of the linear and the silence cases
    are large on BOTH sides: d|log Mx - log My| / dX grows like 1 / |X|, so the few near-zero cells of a noise spectrum (or the
    frames at the edge of a silent stretch) carry most of the gradient's rounding error in any fp32 evaluation."""
    from remfx_amd import losses
    mod = _module(name)
    if CASES[name][1] == "mel":                    # the case's banks have no empty filter
        assert all(bool((fb.abs().sum(1) > 0).all()) for fb in mod.filterbanks) and len(mod.filterbanks) == len(CASES[name][0])
    x, y = _inputs(name)
    l64, g64, a_l, a_g = _reference(name)
    xd = x.to(DEV).requires_grad_(True)
    l = mod(xd, y.to(DEV))
    (l * 1.7).backward()                           # upstream gradient != 1: the device-side gup path
    e_l = abs(float(l) - l64) / abs(l64)
    e_g = _rms(xd.grad.cpu().double() / 1.7 - g64) / _rms(g64)
    print(f"\nSCALED_PARITY {name}: loss {float(l):.8f} ref64 {l64:.10f}  err {e_l:.3e} a {a_l:.3e} | grad err {e_g:.3e} a {a_g:.3e}")
    if CASES[name][7]:                             # clamped cells pass no gradient: a silent row's gradient is exactly zero
        assert float(xd.grad[3].abs().max()) == 0.0 and float(g64[3].abs().max()) == 0.0
    if CASES[name][1] == "mel":                    # ... and it is not the linear loss the keywords used to fall back to
        lin = losses.MultiResolutionSTFTLoss(fft_sizes=mod.fft_sizes, hop_sizes=mod.hop_sizes, win_lengths=mod.win_lengths,
                                             per_example_sc=mod.per_example_sc)(xd.detach(), y.to(DEV))
        assert abs(float(lin) - l64) > 1e-3 * abs(l64)
    assert e_l <= 4 * a_l, (name, e_l, a_l)
    assert e_g <= 4 * a_g, (name, e_g, a_g)


def test_default_keywords_take_the_parent_path_bit_for_bit():
    """scale=None with weights (1, 1, 0): `_MRSTFTFn` with and without the new arguments, value and gradient torch.equal."""
    from remfx_amd import losses
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 1, 24000, generator=g) * 0.3).to(DEV)
    y = x + 0.1 * torch.randn(3, 1, 24000, generator=g).to(DEV)
    res = []
    for extra in ((), (losses.DEFAULT_WEIGHTS, (None, None, None))):
        for pe in (True, False):
            xd = x.clone().requires_grad_(True)
            l = losses._MRSTFTFn.apply(xd, y, losses.FFT_SIZES, losses.HOP_SIZES, losses.WIN_LENGTHS, 1e-8, pe, *extra)
            (l * 1.3).backward()
            res.append((l.detach(), xd.grad))
    for (la, ga), (lb, gb) in zip(res[:2], res[2:]):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    xd = x.clone().requires_grad_(True)
    l = losses.MultiResolutionSTFTLoss(n_bins=1025, sample_rate=48000, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, scale=None)(xd, y)
    (l * 1.3).backward()
    assert torch.equal(l.detach(), res[0][0]) and torch.equal(xd.grad, res[0][1])


def test_identical_signals_give_zero_loss_and_gradient():
    from remfx_amd import losses
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(3, 1, 9001, generator=g) * 0.3).to(DEV)
    for kw in (dict(scale="mel", n_bins=64, sample_rate=48000), dict(scale="mel", n_bins=64, sample_rate=48000, w_lin_mag=1.0,
                                                                      per_example_sc=False), dict(w_lin_mag=1.0)):
        xd = x.clone().requires_grad_(True)
        l = losses.MultiResolutionSTFTLoss(**kw).to(DEV)(xd, x.clone())
        l.backward()
        assert float(l) == 0.0 and float(xd.grad.abs().max()) == 0.0, kw


def test_slot_sums_are_bit_reproducible_across_streams_and_runs():
    from remfx_amd import losses
    mod = _module("mel_multires_batchsc")
    x, y = _inputs("mel_multires_batchsc")
    xd, yd = x.to(DEV), y.to(DEV)
    first = mod(xd, yd)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for s in (s1, s2, s1, s2):
        with torch.cuda.stream(s):
            outs.append(mod(xd, yd))
    torch.cuda.synchronize()
    outs += [mod(xd, yd) for _ in range(3)]
    assert all(torch.equal(o, first) for o in outs)
    # the row sums themselves, into a poisoned buffer's worth of fresh allocations
    from remfx_amd import stft
    w = stft.hann(600, DEV)
    X = stft.stft_raw(xd.reshape(5, -1), 1024, 120, 600, w, 5)
    Y = stft.stft_raw(yd.reshape(5, -1), 1024, 120, 600, w, 5)
    bank = mod._banks()[1]
    a = losses._scaled_sums(X, Y, bank, 1e-8, mod.weights, True)
    b = losses._scaled_sums(X, Y, bank, 1e-8, mod.weights, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and a[0].dtype == torch.float64 and tuple(a[0].shape) == (5, 4)
    assert bool(torch.isfinite(a[0]).all()) and tuple(a[1].shape) == (5, X.shape[1], 64)


def test_memo_shares_spectra_between_mel_loss_and_linear_metric(monkeypatch):
    """Inside stft_memo() the mel loss and the linear metric take their spectra from the same rfx_fft_analysis launches.  4096 has no
    one-launch paired kernel, so the linear metric reads spectra there too: loss(out, tgt) + metric(out, tgt) + metric(inp, tgt) need
    three analyses (out, tgt, inp), not six; at 1024 the linear metric runs rfx_stft_pair_loss (its own FFT) and the mel loss needs
    two.  A repeated mel evaluation adds none, and reuses the row sums."""
    from remfx_amd import losses, stft
    calls = []
    raw = stft.stft_raw

    def counted(sig, n_fft, *a, **k):
        calls.append(n_fft)
        return raw(sig, n_fft, *a, **k)
    monkeypatch.setattr(stft, "stft_raw", counted)
    geo = dict(fft_sizes=(4096, 1024), hop_sizes=(480, 120), win_lengths=(2400, 600))
    mel = losses.MultiResolutionSTFTLoss(scale="mel", n_bins=64, sample_rate=48000, **geo).to(DEV)
    lin = losses.MultiResolutionSTFTLoss(**geo)
    g = torch.Generator().manual_seed(6)
    inp = (torch.randn(2, 1, 16000, generator=g) * 0.3).to(DEV)
    tgt = inp + 0.1 * torch.randn(2, 1, 16000, generator=g).to(DEV)
    out = (inp + 0.05 * torch.randn(2, 1, 16000, generator=g).to(DEV)).requires_grad_(True)
    plain = mel(out.detach(), tgt)
    assert sorted(calls) == [1024, 1024, 4096, 4096]
    del calls[:]
    with losses.stft_memo():
        l = mel(out, tgt)
        m1, m2 = lin(out.detach(), tgt), lin(inp, tgt)
        assert sorted(calls) == [1024, 1024, 4096, 4096, 4096]
        again = mel(out.detach(), tgt)
        assert sorted(calls) == [1024, 1024, 4096, 4096, 4096]
        assert sum(1 for k in losses._MEMO if k[0] == "ssums") == 2
        l.backward()
    assert losses._MEMO is None
    assert torch.equal(l.detach(), plain) and torch.equal(again, plain)
    assert float(out.grad.abs().max()) > 0 and float(m1) != float(m2)


def test_wrapper_keyword_reaches_the_kernel_and_trains(monkeypatch):
    """One small TCNModel(mrstft_kwargs={...}) under RFX_STRICT_NATIVE=1: the loss it trains on is the mel loss, and a few optimiser
    steps lower it."""
    monkeypatch.setenv("RFX_STRICT_NATIVE", "1")
    from remfx_amd import losses, models
    torch.manual_seed(3)
    net = models.TCNModel(sample_rate=48000, num_bins=1025, mrstft_kwargs={"scale": "mel", "n_bins": 64, "w_lin_mag": 1.0},
                          ninputs=1, noutputs=1, nblocks=3, channel_width=8, kernel_size=7, stack_size=10, dilation_growth=2,
                          causal=False).to(DEV)
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(2, 1, 16384, generator=g) * 0.2).to(DEV)
    x = y + 0.1 * torch.randn(2, 1, 16384, generator=g).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    mels = []
    for step in range(6):
        opt.zero_grad()
        loss, out = net((x, y))
        t = models.causal_crop(y, out.shape[-1]) if out.shape[-1] < y.shape[-1] else y
        mel = net.mrstftloss(out.detach(), t)
        if step == 0:
            l1 = losses.L1Loss()(out.detach(), t)
            assert abs(float(loss) - float(mel) - 100 * float(l1)) < 1e-5 * abs(float(loss))     # the wrapper's loss IS mel + 100 L1
            lin = losses.MultiResolutionSTFTLoss()(out.detach(), t.contiguous())
            assert abs(float(lin) - float(mel)) > 1e-3 * abs(float(mel))
        mels.append(float(mel))
        loss.backward()
        opt.step()
    print("\nSCALED_TRAIN mel loss per step:", " ".join(f"{m:.5f}" for m in mels))
    assert mels[-1] < mels[0]
