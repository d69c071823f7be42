"""GPU parity: HIP DPTNet (remfx_amd/dptnet.py, asteroid DPTNet as cfg/model/dptnet.yaml configures it) vs the CPU oracle
restatement (oracle/ref_dptnet.py, same state_dict; asteroid absent: parity unpinned) -- forward, all gradients, the
DPTNetModel wrapper (reference remfx/models.py:327-344) and the plain multi-head attention kernels."""
import pytest
import torch

from tests.conftest import check, mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(n_src=1, in_chan=64, out_chan=64, chunk_size=100, n_repeats=2, fb_name="free", kernel_size=16, n_filters=64, stride=8,
          sample_rate=48000)


def _rms(a, b):
    return float(((a - b) ** 2).mean().sqrt())


@pytest.mark.one_mode
@pytest.mark.parametrize("B,heads,ch,T", [(3, 4, 16, 100), (2, 4, 16, 658), (2, 2, 24, 37), (2, 2, 16, 65)])
def test_mha_vs_torch(B, heads, ch, T):
    from remfx_amd.dptnet import _MhaFn
    g = torch.Generator().manual_seed(T)
    mk = lambda: (torch.randn(B, heads * ch, T, generator=g) * 0.7).to(DEV).requires_grad_(True)
    q, k, v = mk(), mk(), mk()
    gy = torch.randn(B, heads * ch, T, generator=g).to(DEV)
    qq, kk, vv = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, v))
    w = torch.softmax(torch.einsum("bhct,bhcs->bhts", kk.view(B, heads, ch, T), qq.view(B, heads, ch, T)) / ch ** 0.5, dim=2)
    yr = torch.einsum("bhts,bhct->bhcs", w, vv.view(B, heads, ch, T)).reshape(B, heads * ch, T)
    yr.backward(gy.double().cpu())
    y = _MhaFn.apply(q, k, v, heads)
    y.backward(gy)
    for name, a, b in zip(("out", "dq", "dk", "dv"), (y.detach(), q.grad, k.grad, v.grad), (yr.detach(), qq.grad, kk.grad, vv.grad)):
        rms = float(b.pow(2).mean().sqrt())
        assert float((a.double().cpu() - b).pow(2).mean().sqrt()) <= 2e-5 * rms + 1e-9, name


def test_dptnet_fwd_bwd_vs_oracle():
    from oracle import ref_dptnet
    from remfx_amd.dptnet import DPTNet
    torch.manual_seed(1)
    ref = ref_dptnet.DPTNet(**KW)
    net = DPTNet(**KW)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 9000, generator=g) * 0.3                 # 1124 frames -> 24 chunks of 100
    y = ref(x)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    yd = net(x.to(DEV))
    assert yd.shape == y.shape == (2, 1, 9000)
    check(_rms(yd.detach().cpu(), y.detach()), 1e-4, max(1.0, float(y.detach().abs().max())), what=_rms(yd.detach().cpu(), y.detach()))
    yd.backward(gy.to(DEV))
    refg = dict(ref.named_parameters())
    num = den = 0.0
    for n, p in net.named_parameters():
        r = refg[n].grad
        num += float((p.grad.cpu() - r).pow(2).sum()); den += float(r.pow(2).sum())
    rel = (num / den) ** 0.5
    print(f"DPTNet global relative gradient error vs the fp32 oracle [{mode()}]: {rel:.2e}")
    check(rel, 2e-3, bf16x3=5e-3, bf16=0.3, what=rel)


def test_dptnet_model_wrapper_step():
    """DPTNetModel.forward((x, target)) -> (MRSTFT + 100 L1, output (B, 1, T)); sample(x); one RemFX training step."""
    from remfx_amd import models
    torch.manual_seed(3)
    net = models.DPTNetModel(num_bins=1025, **KW)          # cfg/model/dptnet.yaml: sample_rate reaches the wrapper, not asteroid
    model = models.RemFX(1e-4, 0.95, 0.999, 1e-6, 1e-3, 48000, net).to(DEV)
    g = torch.Generator().manual_seed(4)
    y = (torch.randn(2, 1, 32768, generator=g) * 0.1).to(DEV)
    x = y + (torch.randn(2, 1, 32768, generator=g) * 0.03).to(DEV)
    opt = model.configure_optimizers()["optimizer"]
    before = opt.flat.data.clone()
    opt.zero_grad()
    loss = model.training_step((x, y, None, None), 0)
    assert torch.isfinite(loss) and sorted(model.logged) == ["Input_SISDR", "Input_STFT", "train_SISDR", "train_STFT", "train_loss"]
    loss.backward()
    opt.step(clip_norm=10.0)
    assert float((opt.flat.data - before).abs().max()) > 0
    with torch.no_grad():
        assert net.sample(x).shape == (2, 1, 32768)
