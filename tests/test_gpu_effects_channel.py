"""GPU: the rest of remfx.effects on the device -- parametric EQ, stereo widener, volume automation (against the reference's own
outputs, tests/golden/fx_channel.npz, and a float64 lfilter cascade), phaser and limiter (against the float64 restatements of
tests/fx_channel_ref.py), joint stereo loudness and the RandomAudioEffectsChannel chain."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fx_channel_ref as F

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]
DEV = "cuda:0"
SR = 48000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_channel.npz")


def _golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def _clips(B, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T) / SR
    rows = []
    for b in range(B):
        env = 0.2 + 0.8 * (torch.sin(2 * torch.pi * (0.7 + 0.3 * b) * t) > 0).float()
        rows.append(env * (0.4 * torch.sin(2 * torch.pi * (180.0 + 90.0 * b) * t) + 0.05 * torch.randn(T, generator=g)))
    return torch.stack(rows)


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(((got.double().cpu().numpy() - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-30))


def _ulps(got, ref):
    """max |got - ref| in units of fp32 spacing at |ref|"""
    got, ref = got.cpu().numpy().astype(np.float32), np.asarray(ref, dtype=np.float32)
    return float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))).max())


def test_eq_vs_reference_fixture():
    from remfx_amd import effects as E
    z, meta = _golden()
    for name in ("eq_mono", "eq_stereo"):
        rec = meta[name]
        x = F.fixture_input(rec["input_seed"], rec["channels"], meta["T"])
        _seed(rec["seed"])
        fx = E.RandomParametricEQ(SR)
        y = fx(x.to(DEV))
        ref = z[name + "_y"]
        assert y.shape == ref.shape and y.is_cuda
        assert float((y.cpu().double() - torch.from_numpy(ref).double()).abs().max()) <= 5e-7 * float(np.abs(ref).max()), name
    # the functional form: numpy in, numpy out
    rec = meta["eq_mono"]
    y = E.parametric_eq(F.fixture_input(rec["input_seed"], 1, meta["T"]).numpy(), SR, **rec["params"])
    assert isinstance(y, np.ndarray) and y.dtype == np.float32
    assert np.abs(y - z["eq_mono_y"]).max() <= 5e-7 * np.abs(z["eq_mono_y"]).max()


def test_eq_vs_lfilter_extreme_parameters():
    """20 Hz shelves at Q 0.1 and Q 4, a 16 kHz shelf, bands at the range ends; a clip shorter than the 64 chunks, a tail chunk,
    and the full clip length."""
    from remfx_amd import effects as E
    params = [dict(low_shelf_gain_db=6.0, low_shelf_cutoff_freq=20.0, low_shelf_q_factor=0.1, band_gains_db=[-6.0, 6.0, 3.0],
                   band_cutoff_freqs=[1000.0, 10000.0, 4000.0], band_q_factors=[0.1, 4.0, 1.0], high_shelf_gain_db=-6.0,
                   high_shelf_cutoff_freq=16000.0, high_shelf_q_factor=4.0),
              dict(low_shelf_gain_db=-6.0, low_shelf_cutoff_freq=20.0, low_shelf_q_factor=4.0, band_gains_db=[6.0, -6.0, -1.0],
                   band_cutoff_freqs=[10000.0, 1000.0, 2500.0], band_q_factors=[4.0, 0.1, 2.0], high_shelf_gain_db=6.0,
                   high_shelf_cutoff_freq=8000.0, high_shelf_q_factor=0.1)]
    fx = E.RandomParametricEQ(SR)
    for T in (37, 48000 + 1234, 262144):
        x = _clips(2, T, seed=T % 7)
        y = fx.render(x.to(DEV), params)
        for b, p in enumerate(params):
            ref = F.eq(x[b].numpy(), E._eq_sections(p, SR))
            err = float(np.abs(y[b].cpu().double().numpy() - ref).max())
            assert err <= 5e-7 * np.abs(ref).max(), (T, b, err / np.abs(ref).max())


def test_widener_and_volume_vs_reference_fixture():
    from remfx_amd import effects as E
    z, meta = _golden()
    T = meta["T"]
    rec = meta["widener"]
    _seed(rec["seed"])
    y = E.RandomStereoWidener(SR)(F.fixture_input(rec["input_seed"], 2, T).to(DEV))
    assert _ulps(y, z["widener_y"]) <= 2.0
    for k, rec in enumerate(meta["volume"]):
        x0 = F.fixture_input(rec["input_seed"], 1, T)
        x = x0.to(DEV)
        _seed(rec["seed"])
        fx = E.RandomVolumeAutomation(SR)
        y = fx(x)
        assert y.data_ptr() == x.data_ptr()                   # in place, as upstream
        ref = z["volume_y"][k]
        assert _ulps(y, ref) <= 4.0, k
        # segment boundaries are exact: the unfilled tail is the input bit for bit
        filled = sum(fx.last_params[0]["segment_lengths"])
        assert torch.equal(y[:, filled:].cpu(), x0[:, filled:]) and np.array_equal(ref[:, filled:], x0[:, filled:].numpy())
        if k == 2:
            assert min(fx.last_params[0]["segment_lengths"]) == 0
    # batch: one draw per clip, each channel of a clip with the same gains
    xb = F.fixture_input(5, 6, T).view(3, 2, T).to(DEV)
    xc = xb.clone()
    _seed(9)
    fx(xb)
    _seed(9)
    for b in range(3):
        fx(xc[b])
    assert torch.equal(xb, xc)


def test_phaser_and_limiter_vs_restatement():
    from remfx_amd import effects as E
    T = 262144
    x = _clips(3, T, seed=4)
    x[1] *= 4.0                                               # drives the limiter's second stage hard
    ph = [dict(rate_hz=0.25, depth=0.1, centre_frequency_hz=200.0, feedback=0.6, mix=0.7),
          dict(rate_hz=5.0, depth=0.6, centre_frequency_hz=200.0, feedback=0.1, mix=0.1),
          dict(rate_hz=2.2, depth=0.6, centre_frequency_hz=600.0, feedback=0.35, mix=0.5)]
    y = E.RandomPedalboardPhaser(SR).render(x.to(DEV), ph)
    for b, p in enumerate(ph):
        assert _rel(y[b], F.phaser(x[b].numpy(), SR, **p)) < 1e-5, b
    lim = [dict(threshold_db=-32.0, release_ms=10.0), dict(threshold_db=-6.0, release_ms=300.0),
           dict(threshold_db=-18.0, release_ms=120.0)]
    y = E.RandomPedalboardLimiter(SR).render(x.to(DEV), lim)
    for b, p in enumerate(lim):
        assert _rel(y[b], F.limiter(x[b].numpy(), SR, **p)) < 1e-5, b


def test_phaser_and_limiter_properties():
    from remfx_amd import effects as E
    x = _clips(3, 30011, seed=6).to(DEV) * 3.0
    p = [dict(rate_hz=1.0, depth=0.5, centre_frequency_hz=200.0, feedback=0.5, mix=0.0)] * 3
    assert torch.equal(E.RandomPedalboardPhaser(SR).render(x, p), x)
    fx = E.RandomPedalboardLimiter(SR)
    lim = [dict(threshold_db=-32.0, release_ms=10.0), dict(threshold_db=-6.0, release_ms=300.0),
           dict(threshold_db=-12.0, release_ms=55.0)]
    y = fx.render(x, lim)
    assert float(y.abs().max()) <= 1.0
    comp = E.RandomPedalboardCompressor(SR)
    for b, q in enumerate(lim):
        s1, s2, makeup = fx.stages(q)
        y2 = comp.render(comp.render(x[b:b + 1], [s1]), [s2])
        ref = (y2 * torch.tensor(makeup, dtype=torch.float32)).clamp(-1.0, 1.0)
        assert float((y[b:b + 1] - ref).abs().max()) <= 2.0 ** -23, b


def test_joint_stereo_loudness():
    from remfx_amd import effects as E
    for T in (48000 + 1234, 262144):
        x = _clips(2, T, seed=8)
        x[1] *= 0.3
        x[1, : T // 3] = 0.0                                   # one channel partly silent: the joint gate still sees the other
        norm = E.LoudnessNormalize(SR, target_lufs_db=-24.0)
        lufs, gain = norm.measure_joint(x.unsqueeze(0).to(DEV))
        L = F.integrated_loudness_multichannel(x.numpy(), SR)
        assert abs(float(lufs[0]) - L) < 2e-3, (T, float(lufs[0]), L)
        y = norm(x.to(DEV))
        assert torch.allclose(y, x.to(DEV) * gain[0])
        assert abs(F.integrated_loudness_multichannel(y.cpu().numpy(), SR) + 24.0) < 2e-3


def test_chain():
    from remfx_amd import effects as E
    _, meta = _golden()
    T = 48000
    probs = {k: 0.5 for k in ("parametric_eq_prob", "distortion_prob", "delay_prob", "chorus_prob", "phaser_prob", "compressor_prob",
                               "reverb_prob", "stereo_widener_prob", "limiter_prob", "vol_automation_prob")}
    chain = E.RandomAudioEffectsChannel(SR, target_lufs_db=-28.0, **probs)
    x = torch.stack([F.fixture_input(60 + b, 2, T) for b in range(4)]).to(DEV)
    x0 = x.clone()
    _seed(17)
    yb = chain(x)
    plan = chain.last_plan
    assert torch.equal(x, x0)                                  # the caller's tensor is never written
    counts = [sum(n == name for p in plan for n, _ in p) for name in {n for p in plan for n, _ in p}]
    assert any(0 < c < 4 for c in counts)                     # some stage renders a gathered sub-batch
    _seed(17)
    for b in range(4):
        y1 = chain(x[b])
        assert repr(chain.last_plan[0]) == repr(plan[b])
        assert torch.equal(y1, yb[b]), b
    for b in range(4):
        assert abs(F.integrated_loudness_multichannel(yb[b].cpu().numpy(), SR) + 28.0) < 0.05, b
    # the reference's chain (default probabilities): stages drawn under the recorded seeds
    chain = E.RandomAudioEffectsChannel(SR)
    for rec in meta["chain"][:8]:
        _seed(rec["seed"])
        y = chain(F.fixture_input(7, 2, T).to(DEV))
        assert [n for n, _ in chain.last_plan[0]] == rec["stages"], rec["seed"]
        assert abs(F.integrated_loudness_multichannel(y.cpu().numpy(), SR) + 32.0) < 0.05, rec["seed"]


def test_errors():
    from remfx_amd import effects as E
    for cls in (E.RandomParametricEQ, E.RandomStereoWidener, E.RandomVolumeAutomation, E.RandomPedalboardPhaser,
                E.RandomPedalboardLimiter, E.RandomAudioEffectsChannel):
        with pytest.raises(ValueError):
            cls(SR)(torch.zeros(2, 20000))
    for C in (1, 3):
        with pytest.raises(ValueError):
            E.RandomStereoWidener(SR)(torch.zeros(C, 100, device=DEV))
        with pytest.raises(ValueError):
            E.stereo_widener(torch.zeros(4, C, 100, device=DEV), 0.5)
