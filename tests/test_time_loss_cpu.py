"""CPU: the host side of the time-domain training losses (SISDRLoss, SDSDRLoss, SNRLoss, ESRLoss, DCLoss, LogCoshLoss) -- the classes
and the wrappers' `time_loss_kwargs`, the constructor contract, the pure-torch restatement (tests/time_loss_ref.py) against the
existing oracle, and the affine-gradient argument the device kernels rest on: in fp64, a x~ + b t~ + c from the closed-form
coefficients, pushed through the adjoint filter, IS the autograd gradient of every ratio loss."""
import inspect

import numpy as np
import pytest
import torch

from tests import time_loss_ref as ref

TAPS = (None, (-0.85, 1.0, 0.0), (0.3, 1.0, -0.5))
NET = dict(ninputs=1, noutputs=1, nblocks=2, channel_width=8, kernel_size=7, stack_size=2, dilation_growth=2)


def _inputs(seed, R=3, L=1003):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, L, generator=g) * 0.3 + 0.05).double()
    return x, x + 0.1 * torch.randn(R, L, generator=g).double()


def test_classes_and_wrapper_keyword_exist():
    from remfx_amd import losses, models
    import remfx.models as alias
    for name in ("SISDRLoss", "SDSDRLoss", "SNRLoss", "ESRLoss", "DCLoss", "LogCoshLoss"):
        cls = getattr(losses, name)
        m = cls()
        assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
        assert m.reduction == "mean" and m.eps == 1e-8
        assert getattr(alias, name) is cls
    assert sorted(losses.TIME_LOSSES) == ["dc", "esr", "logcosh", "sdsdr", "sisdr", "snr"]
    m = losses.SISDRLoss(False, 1e-6)                                  # the positional keywords it always had
    assert m.zero_mean is False and m.eps == 1e-6 and m.prefilter is None
    assert losses.SNRLoss().zero_mean and losses.SDSDRLoss().zero_mean and losses.LogCoshLoss().a == 1.0
    assert losses.ESRLoss(prefilter=[-0.85, 1, 0]).prefilter == (-0.85, 1.0, 0.0)
    for cls in (models._RemovalWrapper, models.TCNModel, models.DemucsModel, models.OpenUnmixModel, models.DCUNetModel,
                models.DPTNetModel):
        if cls is not models._RemovalWrapper:
            assert inspect.signature(cls.__init__).parameters["time_loss_kwargs"].default is None, cls
        assert hasattr(cls, "_set_time_loss")


def test_constructor_errors():
    from remfx_amd import losses
    for cls in losses.TIME_LOSSES.values():
        with pytest.raises(ValueError, match="reduction"):
            cls(reduction="batchmean")
    for bad in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, float("nan"), 0.0), (float("inf"), 1.0, 0.0), "aw", ("a", "b", "c"), 3.0):
        with pytest.raises(ValueError, match="prefilter"):
            losses.ESRLoss(prefilter=bad)
    with pytest.raises(TypeError):
        losses.ESRLoss(zero_mean=True)                                 # ESR is never centred: not accepted and dropped
    with pytest.raises(TypeError):
        losses.LogCoshLoss(prefilter=(-0.85, 1, 0))
    with pytest.raises(ValueError, match="a="):
        losses.LogCoshLoss(a=0.0)


def test_wrapper_time_loss_kwargs():
    from remfx_amd import losses, models
    plain = models.TCNModel(sample_rate=48000, num_bins=1025, **NET)
    assert plain.timeloss is None and "timeloss" not in dict(plain.named_children())
    m = models.TCNModel(sample_rate=48000, num_bins=1025, time_loss_kwargs={"name": "sisdr", "weight": 0.1}, **NET)
    assert isinstance(m.timeloss, losses.SISDRLoss) and m.time_loss_weight == 0.1
    assert sorted(m.state_dict()) == sorted(plain.state_dict())         # no parameters, no buffers: checkpoints keep their keys
    m = models.TCNModel(sample_rate=48000, num_bins=1025, **NET,
                        time_loss_kwargs={"name": "esr", "prefilter": [-0.85, 1, 0], "eps": 1e-6})
    assert isinstance(m.timeloss, losses.ESRLoss) and m.time_loss_weight == 1.0
    assert m.timeloss.prefilter == (-0.85, 1.0, 0.0) and m.timeloss.eps == 1e-6
    with pytest.raises(ValueError, match="sisdr, sdsdr, snr, esr, dc, logcosh"):
        models.TCNModel(sample_rate=48000, num_bins=1025, time_loss_kwargs={"name": "mse"}, **NET)
    with pytest.raises(ValueError, match="sisdr, sdsdr, snr, esr, dc, logcosh"):
        models.TCNModel(sample_rate=48000, num_bins=1025, time_loss_kwargs={"weight": 2.0}, **NET)
    with pytest.raises(TypeError):
        models.TCNModel(sample_rate=48000, num_bins=1025, time_loss_kwargs={"name": "dc", "zero_mean": True}, **NET)


def test_time_loss_kwargs_through_the_config_composer():
    """`+model.network.time_loss_kwargs.name=sisdr +model.network.time_loss_kwargs.weight=0.1`, the way scripts/train.py reads them."""
    import os
    from remfx_amd import config as rcfg, losses
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = rcfg.compose(os.path.join(root, "cfg"), "config.yaml",
                       ["+exp=reverb", "model=tcn", "model.network.nblocks=2", "model.network.channel_width=8",
                        "+model.network.time_loss_kwargs.name=sisdr", "+model.network.time_loss_kwargs.weight=0.1"])
    net = rcfg.instantiate(cfg["model"]["network"])
    assert isinstance(net.timeloss, losses.SISDRLoss) and net.time_loss_weight == 0.1


def test_restatement_sisdr_equals_oracle():
    from oracle import ref_losses
    x, y = _inputs(3, R=4, L=2000)
    x, y = x.view(2, 2, 2000), y.view(2, 2, 2000)
    assert torch.equal(ref.time_loss("sisdr", x, y), ref_losses.sisdr_loss(x, y))


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("zero_mean", (True, False))
@pytest.mark.parametrize("kind", ref.KINDS)
def test_affine_gradient_and_sums_form(kind, zero_mean, taps):
    """fp64: (1) the table's value on the five row sums equals the literal definition to 1e-12; (2) the closed-form coefficients
    through the adjoint filter equal autograd's gradient to 1e-12 of its largest element."""
    x, y = _inputs(17 + len(kind) + 2 * zero_mean + (0 if taps is None else int(10 * abs(taps[0]))))
    L = x.shape[-1]
    xr = x.clone().requires_grad_(True)
    rows = ref.time_loss(kind, xr, y, zero_mean=zero_mean, reduction="none", taps=taps)
    rows.sum().backward()
    sums = ref.row_sums(x, y, taps)
    val = ref.sums_form_value(kind, sums, L, zero_mean)
    assert np.abs(val - rows.detach().numpy()).max() <= 1e-12 * np.abs(val).max()
    g = ref.adjoint_gradient(ref.closed_form_coefficients(kind, sums, L, zero_mean), x, y, taps)
    assert float((g - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max())
    if taps is not None and taps[0] != taps[2]:                         # the check can tell the adjoint from the filter itself
        sw = ref.adjoint_gradient(ref.closed_form_coefficients(kind, sums, L, zero_mean), x, y, taps[::-1])
        assert float((sw - xr.grad).abs().max()) > 1e-3 * float(xr.grad.abs().max())


def test_logcosh_restatement_gradient():
    """The elementwise gradient the device applies: sinh(a z) / (cosh(a z) + eps) / L."""
    x, y = _inputs(5)
    xr = x.clone().requires_grad_(True)
    ref.time_loss("logcosh", xr, y, reduction="sum", a=2.0).backward()
    z = 2.0 * (x - y)
    want = torch.sinh(z) / (torch.cosh(z) + 1e-8) / x.shape[-1]
    assert float((want - xr.grad).abs().max()) <= 1e-12 * float(want.abs().max())
