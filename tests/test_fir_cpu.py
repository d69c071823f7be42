"""CPU: the host side of the perceptual FIR prefilter and the sum / difference stereo loss -- auraloss's A-weighting design
(`a_weighting_taps`), the constructor contracts of FIRFilter / SumAndDifferenceSTFTLoss and of the wrappers' `perceptual_kwargs` /
`sum_diff_kwargs`, and the fp64 reference (tests/fir_ref.py) against the definition written as a loop."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import fir_ref as ref

NET = dict(ninputs=1, noutputs=1, nblocks=2, channel_width=8, kernel_size=7, stack_size=2, dilation_growth=2)
SUM_ABS = {48000: 2.024, 44100: 2.081, 16000: 2.213}           # sum |h| of the 101-tap design (scipy 1.15.3)


@pytest.mark.parametrize("fs", sorted(SUM_ABS))
def test_a_weighting_taps(fs):
    """101 taps: exactly symmetric, finite in fp32, sum |h| as recorded, and within 0.5 dB of the bilinear IIR at 500 Hz, 1, 4 and
    10 kHz below Nyquist (largest observed 0.20 dB, at 500 Hz and 48 kHz; the margin covers scipy-version drift in firls).  100 Hz is
    NOT asserted: a 101-tap FIR sits at -16.6 dB there against the curve's -19.1 dB, a property of auraloss's design."""
    from remfx_amd import losses
    h = losses.a_weighting_taps(fs, 101)
    assert h.dtype == np.float64 and h.shape == (101,)
    assert float(np.abs(h - h[::-1]).max()) == 0.0
    assert np.isfinite(h.astype(np.float32)).all()
    assert abs(float(np.abs(h).sum()) - SUM_ABS[fs]) <= 1e-3, float(np.abs(h).sum())
    freqs = [f for f in (500.0, 1000.0, 4000.0, 10000.0) if f < fs / 2]
    b, a = ref.a_weighting_iir(fs)
    diff = np.abs(ref.magnitude_db(h, [1.0], freqs, fs) - ref.magnitude_db(b, a, freqs, fs))
    print(f"\nAW_TAPS fs={fs}: sum|h| {np.abs(h).sum():.4f}  |FIR - IIR| dB at {freqs}: {np.round(diff, 3)}")
    assert float(diff.max()) <= 0.5, (freqs, diff)
    assert losses.a_weighting_taps(fs).shape == (101,)          # auraloss's default
    with pytest.raises(ValueError, match="ntaps"):
        losses.a_weighting_taps(fs, 100)


def test_fir_filter_constructor_contract():
    from remfx_amd import losses, models
    import remfx.models as alias
    assert alias.FIRFilter is losses.FIRFilter and alias.SumAndDifferenceSTFTLoss is losses.SumAndDifferenceSTFTLoss
    sig = inspect.signature(losses.FIRFilter.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:5]] == [("filter_type", "hp"), ("coef", 0.85), ("fs", 44100), ("ntaps", 101)]
    assert losses.FIRFilter().taps.tolist() == [1.0, np.float32(-0.85), 0.0]
    assert losses.FIRFilter("fd", coef=0.5).taps.tolist() == [1.0, 0.0, -0.5]
    aw = losses.FIRFilter("aw", fs=48000)
    assert aw.taps.dtype == torch.float32 and torch.equal(aw.taps, torch.from_numpy(losses.a_weighting_taps(48000, 101).astype(np.float32)))
    assert losses.FIRFilter(taps=[0.25, 0.5, 1.0, -0.5, 0.125]).taps.tolist() == [0.25, 0.5, 1.0, -0.5, 0.125]
    for m in (losses.FIRFilter(), aw, losses.SumAndDifferenceSTFTLoss(), losses.SumAndDifferenceSTFTLoss(scale="mel", n_bins=64,
                                                                                                          sample_rate=48000)):
        assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not m.state_dict()      # non-persistent buffers only
    with pytest.raises(ValueError, match="odd"):
        losses.FIRFilter("aw", ntaps=100)
    with pytest.raises(ValueError, match="odd"):
        losses.FIRFilter("hp", ntaps=100)                              # as upstream: checked for every kind
    with pytest.raises(ValueError, match="filter_type"):
        losses.FIRFilter("xx")
    with pytest.raises(ValueError, match="1025"):
        losses.FIRFilter(taps=np.ones(1027))
    with pytest.raises(ValueError, match="1025"):
        losses.FIRFilter("aw", ntaps=1027)
    with pytest.raises(ValueError, match="1025"):
        losses.FIRFilter(taps=[1.0, 2.0])
    for bad in ([1.0, float("nan"), 0.0], [float("inf"), 1.0, 0.0], [1e39, 0.0, 0.0], "aw", 3.0):
        with pytest.raises(ValueError, match="taps"):
            losses.FIRFilter(taps=bad)
    assert losses.FIRFilter(taps=np.ones(1025)).taps.numel() == 1025
    # what was refused stays refused, under the same exceptions
    with pytest.raises(NotImplementedError, match="FIRFilter"):
        losses.MultiResolutionSTFTLoss(perceptual_weighting=True)
    with pytest.raises(ValueError, match="prefilter"):
        losses.ESRLoss(prefilter="aw")
    sd = losses.SumAndDifferenceSTFTLoss(w_sum=0.5, w_diff=2.0, w_lin_mag=1.0)
    assert (sd.w_sum, sd.w_diff) == (0.5, 2.0) and sd.mrstft.weights == (1.0, 1.0, 1.0) and sd.mrstft.fft_sizes == losses.FFT_SIZES
    for shape in ((2, 1, 6000), (2, 3, 6000), (2, 6000)):             # the shape check comes before any device work
        with pytest.raises(ValueError, match=r"\(B, 2, T\)"):
            sd(torch.zeros(shape), torch.zeros(shape))
    for cls in (models.TCNModel, models.DemucsModel, models.OpenUnmixModel, models.DCUNetModel, models.DPTNetModel):
        for kw in ("perceptual_kwargs", "sum_diff_kwargs"):
            assert inspect.signature(cls.__init__).parameters[kw].default is None, (cls, kw)


def test_wrapper_keywords():
    from remfx_amd import losses, models
    plain = models.TCNModel(sample_rate=48000, num_bins=1025, **NET)
    assert plain.perceptual is None and plain.sumdiff is None
    assert not {"perceptual", "sumdiff"} & set(dict(plain.named_children()))
    stereo = dict(NET, ninputs=2, noutputs=2)
    plain2 = models.TCNModel(sample_rate=48000, num_bins=1025, **stereo)
    both = models.TCNModel(sample_rate=48000, num_bins=1025, perceptual_kwargs={"filter_type": "aw"},
                           sum_diff_kwargs={"w_sum": 1.0, "w_diff": 2.0, "weight": 0.5}, mrstft_kwargs={"w_lin_mag": 1.0}, **stereo)
    assert sorted(both.state_dict()) == sorted(plain2.state_dict())                  # checkpoints keep their keys
    assert isinstance(both.perceptual, losses.FIRFilter) and both.perceptual.fs == 48000 and both.perceptual.taps.numel() == 101
    assert isinstance(both.sumdiff, losses.SumAndDifferenceSTFTLoss) and both.sum_diff_weight == 0.5
    assert (both.sumdiff.w_sum, both.sumdiff.w_diff) == (1.0, 2.0) and both.sumdiff.mrstft.weights == (1.0, 1.0, 1.0)
    m = models.TCNModel(sample_rate=44100, num_bins=1025, perceptual_kwargs={"filter_type": "hp", "coef": 0.95}, **NET)
    assert m.perceptual.taps.tolist() == [1.0, np.float32(-0.95), 0.0] and m.sumdiff is None
    assert models.TCNModel(sample_rate=48000, num_bins=1025, sum_diff_kwargs={}, **stereo).sum_diff_weight == 1.0
    with pytest.raises(ValueError, match="filter_type"):
        models.TCNModel(sample_rate=48000, num_bins=1025, perceptual_kwargs={"filter_type": "xx"}, **NET)
    with pytest.raises(ValueError, match="two-channel"):
        models.TCNModel(sample_rate=48000, num_bins=1025, sum_diff_kwargs={}, **NET)
    with pytest.raises(ValueError, match="two-channel"):
        models.OpenUnmixModel(n_channels=1, sum_diff_kwargs={"w_diff": 2.0})
    with pytest.raises(TypeError):
        models.TCNModel(sample_rate=48000, num_bins=1025, perceptual_kwargs={"fs": 16000}, **NET)    # fs is the wrapper's sample rate


def test_keywords_through_the_config_composer():
    """`+model.network.perceptual_kwargs.filter_type=aw`, the way scripts/train.py reads it."""
    from remfx_amd import config as rcfg, losses
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = rcfg.compose(os.path.join(root, "cfg"), "config.yaml",
                       ["+exp=reverb", "model=tcn", "model.network.nblocks=2", "model.network.channel_width=8",
                        "+model.network.perceptual_kwargs.filter_type=aw", "+model.network.perceptual_kwargs.ntaps=51"])
    net = rcfg.instantiate(cfg["model"]["network"])
    assert isinstance(net.perceptual, losses.FIRFilter) and net.perceptual.taps.numel() == 51
    assert net.perceptual.fs == cfg["model"]["network"]["sample_rate"]


def test_reference_equals_the_definition_loop():
    """tests/fir_ref.py on a 7-sample row against the explicit double loop: conv1d's cross-correlation with padding K // 2 IS
    y[n] = sum_k h[k] x[n + k - K/2], its flip uses h[K-1-k], and the flip is the adjoint.  K = 9 > L: the row is shorter than a halo."""
    row = [0.5, -1.25, 2.0, 0.75, -0.375, 1.5, -2.5]
    for h in ([2.0], [1.0, -0.85, 0.0], [0.3, -0.7, 1.1, 0.2, -0.9], [0.1, 0.2, -0.3, 0.4, 1.0, -0.6, 0.7, -0.8, 0.9]):
        for flip in (False, True):
            got = ref.fir_same(torch.tensor([row]), h, flip)[0]
            want = torch.tensor(ref.fir_loop(row, h, flip), dtype=torch.float64)
            assert float((got - want).abs().max()) <= 1e-15, (h, flip)
        if len(h) > 1:
            assert float((ref.fir_same(torch.tensor([row]), h) - ref.fir_same(torch.tensor([row]), h, True)).abs().max()) > 0.1
        g = torch.tensor([[1.0, -2.0, 0.5, 3.0, -1.0, 0.25, 2.0]], dtype=torch.float64)
        lhs = float((ref.fir_same(torch.tensor([row]), h) * g).sum())
        rhs = float((torch.tensor([row]).double() * ref.fir_same(g, h, True)).sum())
        assert abs(lhs - rhs) <= 1e-13
    b = ref.fir_bound(torch.tensor([row]), [1.0, -0.85, 0.0])
    assert b.shape == (1, 7) and abs(float(b[0, 1]) - (5 * 2.0 ** -24 * (0.5 + 0.85 * 1.25) + 2.0 ** -126)) < 1e-20
