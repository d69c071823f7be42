"""GPU: multi-source Hybrid Demucs -- forward / backward parity against the CPU oracle for S >= 2 sources, the two tail kernels
(rfx_fm_cm_affine_g, rfx_row_affine_add) through ctypes, channel-grouped segmentation (rfx_segment_split_c / _merge_c),
HDemucs.separate and the DemucsModel / RemFX wrappers.  Small geometry throughout: nfft 4096, depth 6, 8 channels, clips of about
20000 samples, 2 clips."""
import pytest
import torch

from tests.conftest import check, mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rms(a, b):
    return float(((a - b) ** 2).mean().sqrt())


def _pair(S, Cin, seed=0):
    from oracle import ref_hdemucs
    from remfx_amd.hdemucs import HDemucs
    names = ["mixture"] if S == 1 else [f"s{i}" for i in range(S)]
    torch.manual_seed(seed)
    ref = ref_hdemucs.HDemucs(sources=names, audio_channels=Cin, nfft=4096, channels=8)
    with torch.no_grad():                                   # make LayerScale / freq-emb paths numerically visible
        for n, p in ref.named_parameters():
            if n.endswith(".scale"):
                p.fill_(0.3)
    net = HDemucs(sources=names, audio_channels=Cin, nfft=4096, channels=8)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.to(DEV)


def _input(g, Cin, length):
    """Two clips whose statistics differ clearly (gain 1 and 0.2, offset 0 and 0.1): a (std, mean) pair that reaches the rows of
    the wrong clip is then an error of the size of the output, not of the difference between two draws of the same noise."""
    x = torch.randn(2, Cin, length, generator=g) * 0.5
    return x * torch.tensor([1.0, 0.2]).view(2, 1, 1) + torch.tensor([0.0, 0.1]).view(2, 1, 1)


def _fwd_err(S, Cin, length, seed=1):
    """Output RMS error against the oracle in units of max(1, |y|max), the scale of the forward bound."""
    ref, net = _pair(S, Cin)
    x = _input(torch.Generator().manual_seed(seed), Cin, length)
    with torch.no_grad():
        y = ref(x)
        yd = net(x.to(DEV)).cpu()
    assert yd.shape == y.shape == (2, S, Cin, length)
    print("output rms per clip", y.pow(2).mean(dim=(1, 2, 3)).sqrt().tolist())
    return _rms(yd, y) / max(1.0, float(y.abs().max()))


def test_four_sources_stereo_fwd_bwd(monkeypatch):
    """S = 4, Cin = 2 against the oracle with the bounds tests/test_gpu_hdemucs.py::test_hdemucs_small_fwd_bwd uses for S = 1 at the
    same size.  Measured on an MI355X (RFX_TOL_LOG; error / bound; the output's RMS is 0.044 and 0.098 for the two clips, its
    maximum below 1, so the output bound is absolute):
      f32     output 3.9e-9 / 1e-4    worst tensor 9.9e-6 / 5e-2 (freq_decoder.5.conv_tr.bias)               global gradient 3.3e-6 / 2e-3
      bf16x3  output 4.4e-8 / 1e-4    worst tensor 5.9e-5 / 5e-2 (time_encoder.2.dconv.layers.1.1.weight)    global gradient 3.7e-6 / 2e-3
      bf16    output 2.4e-5 / 2e-2    worst tensor 3.6e-2 / 2.5e-1 (freq_encoder.1.dconv.layers.1.1.weight)  global gradient 1.0e-3 / 2e-1
              (the bf16 bounds are the conftest defaults)
    bf16: the conftest default cannot see a wrong output, so the S = 4 error is also held to at most twice the error of the
    S = 1, Cin = 1 network on the same seed in the same run (both in units of max(1, |y|max)); the tail is the only new arithmetic,
    the factor 2 allows for four times as many output rows drawing on the same trunk.  Measured: 2.4e-5 against 3.3e-5."""
    from remfx_amd import nnops
    monkeypatch.setenv("RFX_STRICT_NATIVE", "1")            # an op without a HIP kernel raises instead of running through torch-ROCm
    nnops.INTERIM.clear()
    ref, net = _pair(4, 2)
    g = torch.Generator().manual_seed(1)
    x = _input(g, 2, 20000)
    y = ref(x)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    yd = net(x.to(DEV))
    assert yd.shape == y.shape == (2, 4, 2, 20000)
    scale = max(1.0, float(y.detach().abs().max()))
    err = _rms(yd.detach().cpu(), y.detach())
    print("output rms error", err, "scale", scale, "output rms per clip", y.detach().pow(2).mean(dim=(1, 2, 3)).sqrt().tolist())
    check(err, 1e-4, scale, what="output")
    yd.backward(gy.to(DEV))
    refg = dict(ref.named_parameters())
    num = den = 0.0
    worst = ("", 0.0)
    for n, p in net.named_parameters():
        r = refg[n].grad
        if r is None:
            continue
        assert p.grad is not None, n
        d = p.grad.cpu() - r
        num += float((d ** 2).sum()); den += float((r ** 2).sum())
        e = _rms(p.grad.cpu(), r) / max(1e-4, float(r.abs().max()))
        if e > worst[1]:
            worst = (n, e)
        check(e, 5e-2, what=(n, e))
    rel = (num / den) ** 0.5
    print("global relative grad error", rel, "worst tensor", worst)
    check(rel, 2e-3, what=rel)
    assert not nnops.INTERIM
    if mode() == "bf16":
        e1 = _fwd_err(1, 1, 20000)
        print("bf16 forward error: S=4 Cin=2", err / scale, "S=1 Cin=1", e1)
        assert err / scale <= 2.0 * e1, (err / scale, e1)


def test_two_sources_mono_odd_length():
    """S = 2, Cin = 1, 20001 samples (no multiple of the hop): the smallest multi-source case, and the one where the coefficient group
    (S * Cin = 2) differs from Cin.  Measured on an MI355X: f32 8.8e-9, bf16x3 6.4e-8 (bound 1e-4), bf16 3.3e-5 (bound 2e-2)."""
    e = _fwd_err(2, 1, 20001)
    print("forward error", e)
    check(e, 1e-4, what="output")


def test_input_gradient_still_raises():
    _, net = _pair(2, 1)
    x = torch.zeros(1, 1, 20000, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        net(x)


# ---- the two tail kernels through ctypes -------------------------------------------------------------------------------------------
def _call(name, *args):
    from remfx_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)
    torch.cuda.synchronize()


@pytest.mark.one_mode
@pytest.mark.parametrize("group", [1, 2, 3, 6])
@pytest.mark.parametrize("bins,F", [(37, 19), (37, 64), (2048, 19), (2048, 64)])
def test_fm_cm_affine_g(group, bins, F):
    """Both directions against the torch expression in fp64: |err| <= 2^-22 (|a x| + |b|) per element -- one fused or unfused
    multiply-add rounding (at most 2^-24 |a x| + 2^-24 |a x + b| <= 2^-23 (|a x| + |b|)) and nothing else.  N = 6 rows with tile
    remainders on both axes; groups of 2 and 3 rows put a coefficient change inside the batch.  group == 1: the bits of
    rfx_fm_cm_affine."""
    from remfx_amd.ops import _ptr, _stream
    N = 6
    g = torch.Generator().manual_seed(bins * 100 + F + group)
    a = (torch.rand(N // group, generator=g) + 0.5).to(DEV)
    b = torch.randn(N // group, generator=g).to(DEV)
    ar, br = a.double().repeat_interleave(group), b.double().repeat_interleave(group)
    # channel-major -> frame-major, y = x a + b
    x = torch.randn(N, 2, bins, F, generator=g).to(DEV)
    y = torch.full((N, F, bins, 2), float("nan"), device=DEV)
    _call("rfx_fm_cm_affine_g", _ptr(x), _ptr(y), _ptr(a), _ptr(b), N, group, bins, F, 1, _stream())
    ax = x.double() * ar[:, None, None, None]
    want = (ax + br[:, None, None, None]).permute(0, 3, 2, 1)
    bound = 2.0 ** -22 * (ax.abs() + br.abs()[:, None, None, None]).permute(0, 3, 2, 1)
    assert torch.isfinite(y).all()
    assert bool(((y.double() - want).abs() <= bound).all()), float(((y.double() - want).abs() - bound).max())
    # frame-major -> channel-major, the backward: x = y a, no b
    gy = torch.randn(N, F, bins, 2, generator=g).to(DEV)
    gx = torch.full((N, 2, bins, F), float("nan"), device=DEV)
    _call("rfx_fm_cm_affine_g", _ptr(gy), _ptr(gx), _ptr(a), None, N, group, bins, F, 0, _stream())
    want = (gy.double() * ar[:, None, None, None]).permute(0, 3, 2, 1)
    assert bool(((gx.double() - want).abs() <= 2.0 ** -22 * want.abs()).all())
    if group == 1:
        y1, gx1 = torch.empty_like(y), torch.empty_like(gx)
        _call("rfx_fm_cm_affine", _ptr(x), _ptr(y1), _ptr(a), _ptr(b), N, bins, F, 1, _stream())
        _call("rfx_fm_cm_affine", _ptr(gy), _ptr(gx1), _ptr(a), None, N, bins, F, 0, _stream())
        assert torch.equal(y, y1) and torch.equal(gx, gx1)


@pytest.mark.one_mode
def test_fm_cm_affine_g_refuses_bad_geometry():
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    t = torch.zeros(6 * 2 * 4 * 4, device=DEV)
    L = _lib.lib()
    assert L.rfx_fm_cm_affine_g(_ptr(t), _ptr(t), _ptr(t), None, 6, 4, 4, 4, 1, _stream()) != 0       # 6 rows, groups of 4
    assert L.rfx_fm_cm_affine_g(_ptr(t), _ptr(t), _ptr(t), None, 6, 0, 4, 4, 1, _stream()) != 0
    assert L.rfx_row_affine_add(_ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), 6, 4, 4, _stream()) != 0


@pytest.mark.one_mode
@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("L", [1, 1000, 4099])
def test_row_affine_add(group, L):
    """out = x a[r / group] + b[r / group] + y against fp64: the multiply-add as above plus the rounding of the final add,
    |err| <= 2^-22 (|a x| + |b| + |y|).  The gradient: y's is the upstream one itself, x's is rfx_row_affine of it with a."""
    from remfx_amd import nnops
    from remfx_amd.ops import _ptr, _stream
    R = 6
    g = torch.Generator().manual_seed(L + group)
    x, y = torch.randn(R, L, generator=g).to(DEV), torch.randn(R, L, generator=g).to(DEV)
    a = (torch.rand(R // group, generator=g) + 0.5).to(DEV)
    b = torch.randn(R // group, generator=g).to(DEV)
    out = torch.full((R, L), float("nan"), device=DEV)
    _call("rfx_row_affine_add", _ptr(x), _ptr(a), _ptr(b), _ptr(y), _ptr(out), R, group, L, _stream())
    ar, br = a.double().repeat_interleave(group)[:, None], b.double().repeat_interleave(group)[:, None]
    ax = x.double() * ar
    want = ax + br + y.double()
    bound = 2.0 ** -22 * (ax.abs() + br.abs() + y.double().abs())
    assert torch.isfinite(out).all()
    assert bool(((out.double() - want).abs() <= bound).all()), float(((out.double() - want).abs() - bound).max())
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    o = nnops.row_affine_add(xg, a, b, yg, group=group)
    assert torch.equal(o.detach(), out)
    go = torch.randn(R, L, generator=g).to(DEV)
    o.backward(go)
    assert torch.equal(yg.grad, go)
    wantg = go.double() * ar
    assert bool(((xg.grad.double() - wantg).abs() <= 2.0 ** -22 * wantg.abs()).all())


# ---- channel-grouped segmentation --------------------------------------------------------------------------------------------------
SEG, OVERLAP = 20000, 0.25


@pytest.mark.one_mode
@pytest.mark.parametrize("T", [66000, 66001])               # about 3.3 segments: the 16-byte path and the dword path
def test_segment_apply_group_channels(T):
    """C = 2 in, Co = 4 out through a function that mixes the channels of a clip but not its samples: the segmented result equals
    the same expression on the whole signal within the bound of the mono merge test (tests/test_gpu_segment.py:
    (max_cover + 3) 2^-24 max|y|, derived from the merge arithmetic).  Any slip in the [b][segment][channel] order is an error of
    the size of the signal."""
    from remfx_amd import segment
    fn = lambda c: torch.cat([c, 2 * c.flip(1)], 1)
    x = (torch.randn(2, 2, T, generator=torch.Generator().manual_seed(5)) * 0.3).to(DEV)
    seen = []

    def spy(c):
        seen.append(tuple(c.shape))
        return fn(c)
    got = segment.apply(spy, x, SEG, OVERLAP, batch=3, group_channels=True)
    want = fn(x)
    plan = segment.SegmentPlan(T, SEG, segment.overlap_samples(SEG, OVERLAP))
    assert all(s[1:] == (2, SEG) for s in seen) and sum(s[0] for s in seen) == 2 * plan.n_segments
    assert got.shape == want.shape == (2, 4, T)
    err = float((got.double() - want.double()).abs().max())
    bound = (plan.max_cover + 3) * 2.0 ** -24 * float(want.abs().max())
    print(f"grouped apply T={T}: max err {err:.3e}, bound {bound:.3e}")
    assert err < bound, (err, bound)
    # (n, S, Cc, L') results are flattened to Co = S * Cc
    got4 = segment.apply(lambda c: fn(c).view(-1, 2, 2, SEG), x, SEG, OVERLAP, batch=3, group_channels=True)
    assert torch.equal(got4, got)
    # the clips themselves: [b][segment][channel]
    clips = segment.split_c(x, plan)
    assert clips.shape == (2 * plan.n_segments, 2, SEG)
    for b in range(2):
        for i, s in enumerate(plan.starts):
            assert torch.equal(clips[b * plan.n_segments + i], x[b, :, int(s):int(s) + SEG])


@pytest.mark.one_mode
@pytest.mark.parametrize("T", [66000, 66001])
def test_segment_group_channels_mono_is_todays_path(T):
    from remfx_amd import segment
    x = (torch.randn(2, 1, T, generator=torch.Generator().manual_seed(6)) * 0.3).to(DEV)
    fn = lambda c: c * 0.5 + 0.25
    assert torch.equal(segment.apply(fn, x, SEG, OVERLAP, batch=3, group_channels=True), segment.apply(fn, x, SEG, OVERLAP, batch=3))


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_separate():
    """Plumbing only (parity is test_four_sources_stereo_fwd_bwd): one segment is one forward, a longer file is
    split_c -> the network per batch -> merge_c, bit for bit."""
    from remfx_amd import segment
    _, net = _pair(2, 2)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 2, SEG, generator=g) * 0.5).to(DEV)
    with torch.no_grad():
        want = net(x)
    got = net.separate(x, segment=SEG)
    assert got.shape == (2, 2, 2, SEG) and not got.requires_grad and net.training
    assert torch.equal(got, want)
    assert torch.equal(net.separate(x), want)
    T = 50000                                               # 2.5 segments
    x = (torch.randn(2, 2, T, generator=g) * 0.5).to(DEV)
    got = net.separate(x, segment=SEG, overlap=OVERLAP, batch=4)
    plan = segment.SegmentPlan(T, SEG, segment.overlap_samples(SEG, OVERLAP))
    clips = segment.split_c(x, plan)
    net.eval()
    with torch.no_grad():
        res = torch.cat([net(clips[k:k + 4]).reshape(-1, 4, SEG) for k in range(0, clips.shape[0], 4)])
    want = segment.merge_c(res, plan).view(2, 2, 2, T)
    assert got.shape == (2, 2, 2, T)
    assert torch.equal(got, want)
    # one source goes the same way
    _, net1 = _pair(1, 1)
    x1 = (torch.randn(1, 1, T, generator=g) * 0.5).to(DEV)
    assert net1.separate(x1, segment=SEG).shape == (1, 1, 1, T)


def _wrapper():
    from remfx_amd import models
    torch.manual_seed(3)
    net = models.DemucsModel(48000, sources=["dry", "residual"], audio_channels=1, nfft=4096, channels=8)
    g = torch.Generator().manual_seed(4)
    y = (torch.randn(2, 2, 1, 20000, generator=g) * 0.1).to(DEV)
    return net, y.sum(1), y


def test_wrapper_loss_two_sources():
    net, x, y = _wrapper()
    net = net.to(DEV)
    loss, output = net((x, y))
    assert output.shape == (2, 2, 1, 20000)
    with torch.no_grad():
        want = net.mrstftloss(output, y) + net.l1loss(output, y) * 100
        assert net.sample(x).shape == (2, 2, 1, 20000)
    assert torch.isfinite(loss) and torch.equal(loss.detach(), want)


def test_wrapper_training_step_two_sources():
    from remfx_amd import models
    net, x, y = _wrapper()
    model = models.RemFX(1e-4, 0.95, 0.999, 1e-6, 1e-3, 48000, net).to(DEV)
    opt = model.configure_optimizers()["optimizer"]
    before = opt.flat.data.clone()
    opt.zero_grad()
    loss = model.training_step((x, y, None, None), 0)
    assert torch.isfinite(loss) and sorted(model.logged) == ["train_SISDR", "train_STFT", "train_loss"]
    loss.backward()
    for n, p in net.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    opt.step(clip_norm=10.0)
    assert float((opt.flat.data - before).abs().max()) > 0


# ---- the multi-source tail behind the channels-last bf16 trunk ---------------------------------------------------------------------
@pytest.mark.one_mode
def test_two_sources_behind_the_channels_last_trunk():
    """At whole 256-frame tiles and channel counts in 16s the bf16 mode runs the first frequency and time layers on the channels-last
    trunk; with several sources its decoder node hands a channel-major tensor to the generic last transposed convolution and the
    multi-source tail -- another path into the new code than the small geometry above takes.  One clip of 262144 samples, 16
    channels, S = 2.  Statement and bounds of tests/test_gpu_clchain.py::test_trunk_vs_channel_major_full_config: against the same
    network in the exact-fp32 mode (which never takes the trunk) the trunk is no further away than 1.5 x the channel-major bf16
    path + 1e-4, output and whole gradient.  Measured on an MI355X (4 trunk layers): output 1.45e-3 against 1.55e-3 channel-major,
    gradient 3.1e-3 against 2.6e-3."""
    from remfx_amd import hdemucs, ops
    from remfx_amd.hdemucs import HDemucs
    torch.manual_seed(0)
    net = HDemucs(sources=["dry", "residual"], audio_channels=1, nfft=4096, channels=16)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith(".scale"):
                p.fill_(0.3)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, 1, 262144, generator=g) * 0.1).to(DEV)
    gy = torch.randn(1, 2, 1, 262144, generator=g).to(DEV)

    def run(arith, trunk):
        prev, prev_t = ops.gemm_precision(), hdemucs.CL_TRUNK
        ops.set_gemm_precision(arith)
        hdemucs.CL_TRUNK = trunk
        try:
            layers = net._cl_layers(256, torch.device(DEV))
            net.zero_grad(set_to_none=True)
            y = net(x)
            y.backward(gy)
            torch.cuda.synchronize()
            return layers, y.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        finally:
            ops.set_gemm_precision(prev)
            hdemucs.CL_TRUNK = prev_t

    def rel(a, b):
        return float(((a.double() - b.double()) ** 2).sum().sqrt() / (b.double() ** 2).sum().sqrt().clamp_min(1e-30))

    def grel(ga, gb):
        num = sum(float(((ga[n].double() - gb[n].double()) ** 2).sum()) for n in gb)
        return (num / sum(float((gb[n].double() ** 2).sum()) for n in gb)) ** 0.5
    l32, y32, g32 = run("f32", True)
    lcm, y_cm, g_cm = run("bf16", False)
    lcl, y_cl, g_cl = run("bf16", True)
    assert (l32, lcm) == (0, 0) and lcl >= 2, (l32, lcm, lcl)          # the trunk is what the third run took
    assert y_cl.shape == (1, 2, 1, 262144) and sorted(g_cl) == sorted(g32)
    e_cm, e_cl, r_cm, r_cl = rel(y_cm, y32), rel(y_cl, y32), grel(g_cm, g32), grel(g_cl, g32)
    print(f"trunk layers {lcl}; output vs fp32 mode: channel-major bf16 {e_cm:.3e}, trunk {e_cl:.3e}; gradient: {r_cm:.3e}, {r_cl:.3e}")
    assert e_cl < 1.5 * e_cm + 1e-4
    assert r_cl < 1.5 * r_cm + 1e-4


# ---- scripts/separate.py -----------------------------------------------------------------------------------------------------------
@pytest.mark.one_mode
def test_separate_script_writes_one_file_per_source(tmp_path):
    """A caller-supplied checkpoint (Lightning-style keys) in, one float32 WAV per source name out, equal to HDemucs.separate on the
    decoded file.  In process: the script's main() is the unit."""
    from remfx_amd.datasets import load_wav, save_wav
    from remfx_amd.hdemucs import HDemucs
    from scripts import separate
    names = ["dry", "residual"]
    torch.manual_seed(11)
    net = HDemucs(sources=names, audio_channels=2, channels=8)
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {"model.model." + k: v for k, v in net.state_dict().items()}}, ckpt)
    T = 30000
    audio = torch.randn(2, T, generator=torch.Generator().manual_seed(12)) * 0.1
    save_wav(tmp_path / "in.wav", audio, 8000)
    paths = separate.main([f"+checkpoint={ckpt}", f"+audio_input={tmp_path / 'in.wav'}", f"+output_dir={tmp_path / 'stems'}",
                           "+sources=dry,residual", "+channels=8", "+sample_rate=8000", "+segment_seconds=2.5", "+segment_batch=2"])
    assert [p.split("/")[-1] for p in paths] == ["dry.wav", "residual.wav"]
    want = net.to(DEV).separate(audio.unsqueeze(0).to(DEV), segment=20000, overlap=0.25, batch=2)[0].cpu()
    for k, p in enumerate(paths):
        got, sr = load_wav(p)
        assert sr == 8000 and torch.equal(got, want[k])
    with pytest.raises(FileNotFoundError):
        separate.main([f"+checkpoint={tmp_path / 'none.ckpt'}", f"+audio_input={tmp_path / 'in.wav'}", f"+output_dir={tmp_path}"])
