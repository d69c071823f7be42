"""GPU: RandomSoxReverb on the device (rfx_fx_sox_reverb, csrc/fx.hip) against the numpy restatement of SoX's reverb
(tests/sox_reverb_ref.py; SoX / torchaudio are absent: parity is against the restated algorithm, unpinned).

Bound of the comparison with the float64 restatement: max(8 a, 2 b), both measured here on the same clips and neither on the
kernel under test:
  (a) the same restatement in float32 (SoX's own arithmetic) against float64, relative RMS, worst clip;
  (b) the merged rfx_fx_reverb kernel against oracle/ref_effects.reverb at the matching corner (room_size 1, damping 0.5 =
      comb feedback 0.98, damp 0.2), worst row: the wave scan of the damping filter and its powf carry cost more than sequential
      float32, and a kernel on the same scheme inherits that.
8 x for fused multiply-adds and summation order; 2 x because a clip runs through two or four banks and one more gain stage than
JUCE's one bank.  Measured on the MI355X: test_vs_restatement (a) 1.24e-7, (b) 2.90e-7, bound 9.9e-7, device
4.0e-8 .. 5.8e-7; test_short_lags_narrow_the_block (a) 9.0e-8, (b) 1.4e-7, bound 7.2e-7, device 6.1e-8 and 1.1e-7."""
import numpy as np
import pytest
import torch

from tests import sox_reverb_ref as S

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]
DEV = "cuda:0"
SR = 48000
NAMES = ("reverberance", "high_freq_damping", "room_scale", "stereo_depth", "wet_dry", "pre_delay")


def _clips(B, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T) / SR
    rows = []
    for b in range(B):
        env = 0.2 + 0.8 * (torch.sin(2 * torch.pi * (0.7 + 0.3 * b) * t) > 0).float()        # on / off bursts
        rows.append(env * (0.4 * torch.sin(2 * torch.pi * (180.0 + 90.0 * b) * t) + 0.05 * torch.randn(T, generator=g)))
    return torch.stack(rows)


def _p(*v):
    return dict(zip(NAMES, v))


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(((got - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-30))


def _sibling_error(rows):
    """(b): rfx_fx_reverb against its float64 oracle at feedback 0.98, damp 0.2, wet only, on mono rows (N, T)."""
    from oracle import ref_effects as R
    from remfx_amd import effects as E
    p = dict(room_size=1.0, damping=0.5, wet_dry=1.0, width=1.0)
    y = E.RandomPedalboardReverb(SR).render(rows.to(DEV), [p] * rows.shape[0]).cpu().numpy()
    return max(_rel(y[i], R.reverb(rows[i].numpy(), SR, 1.0, 0.5, 1.0, 0.0, 1.0)) for i in range(rows.shape[0]))


def _check_vs_restatement(fx, groups, sibling_rows):
    """groups: [(clips (B, Cin, T), params)].  Prints every figure, then asserts every clip under max(8 a, 2 b)."""
    a, dev_err = 0.0, []
    for clips, params in groups:
        y = fx.render(clips.to(DEV), params).cpu().numpy()
        for b, p in enumerate(params):
            args = (clips[b].numpy(), fx.sample_rate) + tuple(p[k] for k in NAMES)
            ref = S.random_sox_reverb(*args, dtype=np.float64)
            a = max(a, _rel(S.random_sox_reverb(*args, dtype=np.float32), ref))
            dev_err.append((_rel(y[b], ref), clips.shape[1], p))
    b_err = _sibling_error(sibling_rows)
    bound = max(8.0 * a, 2.0 * b_err)
    print(f"sox reverb: (a) float32 restatement {a:.3e}, (b) rfx_fx_reverb {b_err:.3e}, bound {bound:.3e}")
    for e, cin, p in dev_err:
        print(f"  device {e:.3e}  Cin {cin}  {p}")
    for e, cin, p in dev_err:
        assert e < bound, (e, bound, cin, p)


def test_vs_restatement():
    """Corners: reverberance 100 with damping 0 (feedback 0.98), room_scale 5 and 100, stereo_depth 20 and 100, pre_delay 0 and
    100 ms, mono and stereo input, a length that is not a multiple of 64."""
    from remfx_amd import effects as E
    T = 20011
    mono = _clips(4, T, seed=1).unsqueeze(1)
    stereo = _clips(4, T, seed=2).view(2, 2, T)
    pm = [_p(100.0, 0.0, 100.0, 100.0, 1.0, 0.0), _p(100.0, 0.0, 5.0, 20.0, 1.0, 100.0), _p(50.0, 50.0, 40.0, 60.0, 0.5, 13.7),
          _p(10.0, 100.0, 100.0, 20.0, 0.3, 0.0)]
    ps = [_p(100.0, 0.0, 100.0, 100.0, 1.0, 100.0), _p(70.0, 30.0, 5.0, 100.0, 0.6, 0.0)]
    rows = torch.cat([mono.view(4, T), stereo.view(4, T)])
    _check_vs_restatement(E.RandomSoxReverb(SR), [(mono, pm), (stereo, ps)], rows)


def test_short_lags_narrow_the_block():
    """At 8 kHz and room_scale 5 the shortest comb is 29 samples: the kernel walks blocks of 29, same bound."""
    from remfx_amd import effects as E
    fx = E.RandomSoxReverb(8000)
    p = _p(100.0, 0.0, 5.0, 100.0, 1.0, 3.0)
    assert E.sox_reverb_plan(p, 8000)["min_lag"] == 29
    clips = _clips(2, 6001, seed=3)
    _check_vs_restatement(fx, [(clips[:1].unsqueeze(1), [p]), (clips.view(1, 2, -1), [dict(p, room_scale=9.0, wet_dry=0.5)])], clips)


def test_impulse_per_clip_geometry():
    """A unit impulse through two parameter sets with different rooms in one batch: bank w is silent until delay + its shortest
    comb and gives gain * wet_dry there; sample 0 holds the dry impulse."""
    from remfx_amd import effects as E
    T = 8000
    x = torch.zeros(2, 1, T)
    x[:, 0, 0] = 1.0
    params = [_p(80.0, 30.0, 5.0, 100.0, 0.8, 2.0), _p(40.0, 70.0, 100.0, 50.0, 0.35, 31.0)]
    y = E.RandomSoxReverb(SR).render(x.to(DEV), params).cpu().numpy()
    ks = []
    for b, p in enumerate(params):
        q = E.sox_reverb_plan(p, SR)
        wd = np.float32(p["wet_dry"])
        for w in range(2):
            k = q["delay"] + min(q["comb_lengths"][w])
            ks.append(k)
            assert y[b, w, 0] == np.float32(1.0) - wd
            assert not y[b, w, 1:k].any(), (b, w)
            want = float(np.float32(q["gain"])) * float(wd)
            assert abs(float(y[b, w, k]) - want) <= 1e-6 * want, (b, w, y[b, w, k], want)
    assert len(set(ks)) == 4


def test_forward_batches_like_single_clips():
    from remfx_amd import effects as E
    x = _clips(3, 20000, seed=4).to(DEV)
    fx = E.RandomSoxReverb(SR)
    torch.manual_seed(11)
    yb = fx(x.unsqueeze(1))
    sets = fx.last_params
    assert yb.shape == (3, 2, 20000) and len(sets) == 3 and list(sets[0]) == list(NAMES)
    torch.manual_seed(11)
    for b in range(3):
        y1 = fx(x[b:b + 1])                                   # (1, T): the reference's call
        assert fx.last_params[0] == sets[b]
        assert y1.shape == (2, 20000) and torch.equal(y1, yb[b])


def test_shapes_errors_and_determinism():
    from remfx_amd import effects as E
    fx = E.RandomSoxReverb(SR)
    T = 9001
    for shape, out in (((1, T), (2, T)), ((2, T), (2, T)), ((3, 1, T), (3, 2, T)), ((3, 2, T), (3, 2, T))):
        x = (0.3 * torch.randn(shape, generator=torch.Generator().manual_seed(5))).to(DEV)
        keep = x.clone()
        y = fx(x)
        assert y.shape == out and y.dtype == torch.float32 and torch.equal(x, keep) and bool(torch.isfinite(y).all())
        assert y.data_ptr() != x.data_ptr()
    with pytest.raises(ValueError):
        fx(torch.zeros(3, T, device=DEV))
    with pytest.raises(ValueError):
        fx(torch.zeros(2, 3, T, device=DEV))
    with pytest.raises(ValueError, match="no CPU path"):
        fx(torch.zeros(1, T))
    with pytest.raises(ValueError, match="lag"):               # a sample rate at which a comb has no sample left
        E.RandomSoxReverb(50).render(torch.zeros(1, 1, 100, device=DEV), [_p(50.0, 50.0, 5.0, 50.0, 0.5, 0.0)])
    x = _clips(4, T, seed=6).view(2, 2, T).to(DEV)
    params = [fx.draw() for _ in range(2)]
    assert torch.equal(fx.render(x, params), fx.render(x, params))
