"""tests/fx_ref.py is right and its bounds have power: the fp64 statements against the independent statements the
project already has (oracle/ref_effects.py, tests/fx_channel_ref.py, tests/sox_reverb_ref.py, the recorded reference outputs of
tests/golden/fx_channel.npz, scipy.signal.lfilter); the host helpers of remfx_amd/effects.py against fx_ref's own constructions; the
case tables through forms_*(); every floor recomputed from restate_*; every bound against a defect of the kind a kernel could have,
applied to the reference alone; the loudness gate margins."""
import json
import os

import numpy as np
import pytest
import scipy.signal

from oracle import ref_effects as R
from tests import fx_channel_ref as FC
from tests import fx_ref as X
from tests import sox_reverb_ref as SX

SR = 48000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_channel.npz")
BIG = 100000                                         # cases beyond it are the grid-stride second trips: floors use the others


def _close(a, b, rel, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= rel * max(float(np.abs(b).max()), 1e-30), (what, err)


# ---- the fp64 statements against the project's independent ones, at the workload's shapes ------------------------------------------------
def test_streams_match_oracle():
    x = X.signal(2, 24000, 1, 0.8)
    g = np.asarray([10.0 ** (-3.0 / 20.0), 10.0 ** (9.0 / 20.0)], np.float32)
    for b, db in enumerate((-3.0, 9.0)):
        _close(X.distortion(x, g)[b], np.tanh(x[b].astype(np.float64) * float(g[b])), 1e-15, "distortion")
        _close(X.distortion(x, g)[b], R.distortion(x[b], db), 1e-7, "distortion vs oracle")          # the gain is a float32 here
    D = np.asarray([int(0.1 * SR), int(0.31 * SR)], np.int32)
    fb, mix = np.asarray([0.5, 0.3], np.float32), np.asarray([0.4, 0.7], np.float32)
    y, _ = X.delay(x, D, fb, mix)
    for b, sec in enumerate((0.1, 0.31)):
        _close(y[b], R.delay(x[b], SR, sec, float(fb[b]), float(mix[b])), 1e-14, "delay")


def test_chorus_matches_oracle():
    x = X.signal(2, 24000, 2, 0.8)
    prm = [np.asarray(v, np.float32) for v in ((1.5, 3.0), (0.4, 0.6), (7.0, 5.0), (0.3, 0.6), (0.5, 0.7))]
    y, _ = X.chorus(x, float(SR), *prm)
    for b in range(2):
        _close(y[b], R.chorus(x[b], SR, *(float(p[b]) for p in prm)), 1e-11, "chorus")


def test_compressor_and_limiter_match_oracle():
    x = X.signal(2, 24000, 3, 0.9, 0.001)
    x[:, 5000:9000] *= np.float32(0.01)
    for b, (tdb, ratio, at, rl) in enumerate(((-20.0, 3.0, 5.0, 100.0), (-30.0, 1.5, 1.0, 250.0))):
        thr = np.asarray([10.0 ** (tdb / 20.0)])
        ca, cr = np.asarray([X.ballistics(at, SR)]), np.asarray([X.ballistics(rl, SR)])
        env, _ = X.comp_env(x[b:b + 1], ca, cr)
        g, _ = X.comp_gain(env, thr, np.asarray([ratio]))
        _close(g * x[b:b + 1], R.compressor(x[b], SR, tdb, ratio, at, rl)[None], 1e-13, "compressor")
    # the limiter: the nine rows, the two stages with fp64 hand-over, make-up and clip
    p = X.limiter_rows([-12.0, 3.0], [50.0, 200.0], SR, dtype=np.float64)
    for b, (tdb, rl) in enumerate(((-12.0, 50.0), (3.0, 200.0))):
        pb = p[:, b:b + 1]
        x3 = x[b:b + 1].astype(np.float64) * 3.0
        e1, _ = X.comp_env(x3, pb[2], pb[3])
        y1 = X.comp_gain(e1, pb[0], pb[1])[0] * x3
        e2, _ = X.comp_env(y1, pb[6], pb[7])
        y, _, _ = X.limiter_out(y1, e2, pb)
        _close(y, FC.limiter(x[b].astype(np.float64) * 3.0, SR, tdb, rl)[None], 1e-12, "limiter")


def test_reverb_matches_oracle():
    """T = 8000 at 48 kHz: every ring (1214 ... 1759 samples) wraps four times; the full 24000 adds run time and no ring state"""
    x = X.signal(2, 8000, 4, 0.8)
    room, dmp, wet, dry, width = (0.3, 0.9), (0.2, 0.8), (0.3, 0.6), (0.7, 0.4), (0.5, 1.0)
    f32 = lambda v: np.asarray(v, np.float64)                                                        # noqa: E731
    y, _ = X.reverb(x, SR, f32(dmp) * 0.4, f32(room) * 0.28 + 0.7, 0.5 * (f32(wet) * 3.0) * (1.0 + f32(width)), f32(dry) * 2.0)
    for b in range(2):
        _close(y[b], R.reverb(x[b], SR, room[b], dmp[b], wet[b], dry[b], width[b]), 1e-7, "reverb")   # 0.015 is a float32 here


def test_sox_reverb_matches_its_restatement_and_the_host_plan():
    from remfx_amd import effects as E
    T = 6000
    for Cin, prm in ((1, dict(reverberance=60.0, high_freq_damping=30.0, room_scale=40.0, stereo_depth=60.0, pre_delay=20.0, wet_dry=0.625)),
                     (2, dict(reverberance=95.0, high_freq_damping=80.0, room_scale=10.0, stereo_depth=100.0, pre_delay=0.0, wet_dry=0.25))):
        x = X.signal(Cin, T, 5 + Cin, 1.4)
        q = E.sox_reverb_plan(prm, SR)
        geom = np.zeros((Cin * 2, 16), np.int32)
        for c in range(Cin):
            for w in range(2):
                geom[c * 2 + w, 0], geom[c * 2 + w, 1:13], geom[c * 2 + w, 13] = q["delay"], q["comb_lengths"][w] + q["allpass_lengths"][w], c
        coef = np.tile(np.asarray([q["feedback"], q["damp"], q["gain"], q["wet_dry"]], np.float32), (Cin * 2, 1))
        ws, _ = X.sox_banks(x[None], geom, coef)
        y, _ = X.sox_mix(x[None], ws, coef, Cin)
        ref = SX.random_sox_reverb(x, SR, prm["reverberance"], prm["high_freq_damping"], prm["room_scale"], prm["stereo_depth"], prm["wet_dry"],
                                   prm["pre_delay"])
        _close(y[0], ref, 1e-12, ("sox", Cin))
        p2 = SX.plan(prm["reverberance"], prm["high_freq_damping"], prm["room_scale"], prm["stereo_depth"], prm["pre_delay"], SR)
        assert q["delay"] == p2["delay"] and q["lds_floats"] == max(sum(b["combs"]) + sum(b["allpasses"]) for b in p2["banks"])


def test_cascades_match_lfilter_and_the_golden_eq():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    rec = meta["eq_mono"]
    x = FC.fixture_input(rec["input_seed"], 1, meta["T"]).numpy()
    p = rec["params"]
    mine = dict(low=(p["low_shelf_gain_db"], p["low_shelf_cutoff_freq"], p["low_shelf_q_factor"]),
                high=(p["high_shelf_gain_db"], p["high_shelf_cutoff_freq"], p["high_shelf_q_factor"]),
                bands=list(zip(p["band_gains_db"], p["band_cutoff_freqs"], p["band_q_factors"])))
    sec = X.eq_sections(mine, SR)
    y, bound = X.eq(x, sec[None])
    ref = x.astype(np.float64)
    for c in sec:
        ref = scipy.signal.lfilter(c[:3], [1.0, c[3], c[4]], ref)
    _close(y, ref, 1e-12, "cascade vs lfilter")
    # the recorded reference output, at the tolerance test_gpu_effects_channel.py holds the device to (the reference's own float32 steps)
    assert np.abs(y - z["eq_mono_y"]).max() <= 5e-7 * np.abs(z["eq_mono_y"]).max()
    # the RBJ biquads against the recorded coefficients
    for (g, f, q), kind, b_ref, a_ref in zip(z["biq_params"], z["biq_kinds"], z["biq_b"], z["biq_a"]):
        c = X.rbj(str(kind), g, f, q, SR)
        np.testing.assert_allclose(c, np.concatenate([b_ref, a_ref[1:]]), rtol=1e-14, atol=0)


def test_widener_and_volume_match_the_golden_outputs():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    T = meta["T"]
    rec = meta["widener"]
    x = FC.fixture_input(rec["input_seed"], 2, T).numpy()
    w = np.float32(rec["draws"][0])
    gm, gs = np.asarray([2 * (1 - w)], np.float32), np.asarray([2 * w], np.float32)
    assert np.array_equal(X.restate_widener(x[None], gm, gs)[0], z["widener_y"]), "the float32 restatement is not the reference's arithmetic"
    _close(X.widener(x[None], gm, gs)[0], z["widener_y"], 1e-6, "widener")
    for k, rec in enumerate(meta["volume"]):
        d = rec["draws"]
        n = int(d[0])
        lengths = (T * np.asarray(d[1 + n:1 + 2 * n])).astype("int")
        gains = [float(np.float32(v)) for v in d[1 + 2 * n:1 + 3 * n]]
        x = FC.fixture_input(rec["input_seed"], 1, T).numpy()
        y, bound = X.volume(x, np.cumsum(lengths)[None].astype(np.int32), np.asarray([[0.0] + gains[:-1]], np.float32), np.asarray([gains], np.float32))
        ref = z["volume_y"][k].astype(np.float64)
        assert (np.abs(y - ref) <= bound).all(), ("volume", k, float((np.abs(y - ref) / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(ref[:, int(lengths.sum()):], x[:, int(lengths.sum()):])


def test_phaser_and_loudness_match_the_channel_restatements():
    x = X.signal(2, 24000, 6, 0.5)
    prm = [np.asarray(v, np.float32) for v in ((1.0, 4.0), (0.3, 0.6), (300.0, 600.0), (0.2, 0.6), (0.5, 0.7))]
    G, _ = X.phaser_coef(24000, float(SR), *prm[:3])
    y, _ = X.phaser(x, G, prm[3], prm[4])
    for b in range(2):
        _close(y[b], FC.phaser(x[b], float(SR), *(float(p[b]) for p in prm)), 1e-10, "phaser")
    # loudness: a second of audio, mono and jointly over two channels
    T = 48000
    chunk, hop, nhop, nblk, inv, _ = X.loud_plan(T, SR)
    x = X.signal(2, T, 7, 0.3)
    x[:, :20000] *= np.float32(0.03)
    c = dict(nhop=nhop, hop=hop, nblk=nblk)
    res = X.loudness(x[:, None, :], X.k_weighting(SR), c)
    for b in range(2):
        assert abs(res["lufs"][b] - R.integrated_loudness(x[b], SR)) < 1e-9
    joint = X.loudness(x[None], X.k_weighting(SR), c)
    assert abs(joint["lufs"][0] - FC.integrated_loudness_multichannel(x, SR)) < 1e-9


def test_host_helpers_match_the_reference_constructions():
    from remfx_amd import effects as E
    (b1, a1), (b2, a2) = E._k_weighting(SR)
    sec = X.k_weighting(SR)
    np.testing.assert_allclose(np.concatenate([b1, a1[1:], b2, a2[1:]]), sec.reshape(-1), rtol=1e-14)
    for chunk in (1, 7, 375, 4096):
        M = E._transition([(b1, a1), (b2, a2)], chunk)
        mine = X.transition(sec, chunk)[1]
        assert np.abs(M - mine).max() <= 1e-9 * max(1.0, np.abs(mine).max()), chunk
    p = dict(low_shelf_gain_db=-4.0, low_shelf_cutoff_freq=30.0, low_shelf_q_factor=2.0, band_gains_db=[1.0, -3.0], band_cutoff_freqs=[2900.0, 5300.0],
             band_q_factors=[2.8, 0.6], high_shelf_gain_db=5.8, high_shelf_cutoff_freq=8100.0, high_shelf_q_factor=0.75)
    secs = E._eq_sections(p, SR)
    mine = X.eq_sections(dict(low=(-4.0, 30.0, 2.0), high=(5.8, 8100.0, 0.75), bands=[(1.0, 2900.0, 2.8), (-3.0, 5300.0, 0.6)]), SR)
    np.testing.assert_allclose(np.stack([np.concatenate([b, a[1:]]) for b, a in secs]), mine, rtol=1e-14)
    assert np.abs(E._transition(secs, 375) - X.transition(mine, 375)[1]).max() <= 1e-9 * np.abs(X.transition(mine, 375)[1]).max()
    for ms in (0.0005, 0.001, 2.0, 200.0):
        assert E._ballistics_cte(ms, SR) == pytest.approx(X.ballistics(ms, SR), rel=1e-15, abs=0)
    lim = E.RandomPedalboardLimiter(SR)
    for tdb, rl in ((-20.0, 50.0), (-3.0, 300.0)):
        s1, s2, mk = lim.stages(dict(threshold_db=tdb, release_ms=rl))
        col = []
        for s in (s1, s2):
            col += [10.0 ** (s["threshold_db"] / 20.0), s["ratio"], E._ballistics_cte(s["attack_ms"], SR), E._ballistics_cte(s["release_ms"], SR)]
        np.testing.assert_allclose(np.asarray(col + [mk], np.float32), X.limiter_rows([tdb], [rl], SR)[:, 0], rtol=0, atol=0)
    for T in (24000, 30011, 262144):
        nhop, (chunk, hop, nhop2, nblk, inv, coef) = E.LoudnessNormalize(SR)._plan(T)
        mine = X.loud_plan(T, SR)
        assert (chunk, hop, nhop2, nblk, inv) == mine[:5] and nhop == nhop2
        assert np.abs(coef - mine[5]).max() <= 1e-9 * np.abs(mine[5]).max()


def test_reverb_rate_range():
    """every ring at least one 64-sample block: 225 sr / 44100 >= 64 from 12544 Hz; the twelve rings in 160 KB of LDS up to 143526 Hz"""
    assert X.reverb_rate_range() == (12544, 143526)
    assert min(sum(X.reverb_lengths(12543), [])) == 63 and 4 * sum(sum(X.reverb_lengths(143527), [])) > 160 * 1024


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
def test_every_form_is_reached_and_every_case_adds_one():
    reached, per = X.walk_all_cases()
    total = X.all_forms()
    assert not reached - total, sorted(reached - total)
    assert total - reached == X.UNREACHABLE, sorted(total - reached - X.UNREACHABLE)
    assert (len(reached), len(total)) == (181, 185)
    for name, c, new in per:
        assert new or c.get("value"), (name, c, "reaches nothing new and is not marked as a value case")


# ---- floors ------------------------------------------------------------------------------------------------------------------------------
def _floor(err, mag):
    return float((err / np.maximum(X.EPS32 * mag, 1e-300)).max())


def _floors():
    out = {}
    put = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))                                  # noqa: E731
    for c in X.DIST_CASES:
        x, g = X.dist_data(c)
        put("tanh", _floor(np.abs(X.restate_distortion(x, g) - X.distortion(x, g)), X.distortion_bound(x, g) / (X.k_of("tanh") * X.EPS32)))
    base, ex = X.powf_data()
    ref = base.astype(np.float64) ** ex.astype(np.float64)
    put("powf", _floor(np.abs(X.restate_powf(base, ex) - ref), ref))
    for c in X.COMP_CASES:
        if c["T"] < BIG:
            x, thr, ratio, ca, cr = X.comp_data(c)
            env, mag = X.comp_env(x, ca, cr)
            put("comp_env", _floor(np.abs(X.restate_comp_env(x, ca, cr) - env), mag))
    for c in X.CHORUS_CASES:
        a = X.chorus_data(c)
        y, mag, extra = X.chorus_parts(a[0], c["sr"], *a[1:])
        put("chorus", _floor(np.maximum(np.abs(X.restate_chorus(a[0], c["sr"], *a[1:]) - y) - extra, 0.0), mag))
    for c in X.REVERB_CASES:
        a = X.reverb_data(c)
        y, bound = X.reverb(a[0], c["sr"], *a[1:])
        put("reverb", _floor(np.abs(X.restate_reverb(a[0], c["sr"], *a[1:]) - y), bound / (X.k_of("reverb") * X.EPS32)))
    for c in X.SOX_CASES:
        x, geom, coef, _ = X.sox_data(c)
        ws, bound = X.sox_banks(x, geom, coef)
        put("sox_bank", _floor(np.abs(X.restate_sox_banks(x, geom, coef) - ws), bound / (X.k_of("sox_bank") * X.EPS32)))
    for c in X.PHASER_CASES:
        x, rate, depth, cen, fb, mix = X.phaser_data(c)
        G, gb = X.phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
        G32 = X.restate_phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
        put("phaser_coef", _floor(np.abs(G32 - G), G))
        n = c.get("prefix", c["T"])
        if not c.get("mix0"):
            y, bound = X.phaser(x[:, :n], G32, fb, mix)
            put("phaser", _floor(np.abs(X.restate_phaser(x[:, :n], G32, fb, mix) - y), bound / (X.k_of("phaser") * X.EPS32)))
    return out


def test_floors_are_below_the_table():
    got = _floors()
    print("\nFX floors (eps32 x magnitude): " + ", ".join(f"{k} {v:.2f}" for k, v in got.items()))
    assert set(got) == set(X.FLOOR)
    for k, v in got.items():
        assert v <= X.FLOOR[k], (k, v)


def test_exact_forms_are_exact_in_the_restatement():
    """mix = 0 gives x bit for bit in the float32 restatements of chorus and phaser (fused or not); below the threshold the gain is 1"""
    c = next(c for c in X.CHORUS_CASES if c.get("mix0"))
    a = X.chorus_data(c)
    assert np.array_equal(X.restate_chorus(a[0], c["sr"], *a[1:]), a[0]) and float(X.chorus(a[0], c["sr"], *a[1:])[1].max()) == 0.0
    c = next(c for c in X.PHASER_CASES if c.get("mix0"))
    x, rate, depth, cen, fb, mix = X.phaser_data(c)
    G32 = X.restate_phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
    assert np.array_equal(X.restate_phaser(x, G32, fb, mix), x) and float(X.phaser(x, G32, fb, mix)[1].max()) == 0.0
    x, g = X.scale_data(X.SCALE_CASES[0])
    assert np.array_equal(X.scale(x, g).astype(np.float32), g[:, None] * x)


# ---- the power of every bound, on the reference alone ------------------------------------------------------------------------------------
def _misses(ref, bad, bound):
    return bool((np.abs(np.asarray(bad, np.float64) - ref) > bound).any())


def _shifted(y):
    """one sample of the last row takes its neighbour's value"""
    out = np.array(y, np.float64)
    k = out.shape[-1] // 2
    out[..., -1, k] = out[..., -1, k + 1]
    return out, k


def _main_outputs():
    """(entry point, reference, bound) of every entry point's result at a small case"""
    out = []
    c = X.DIST_CASES[1]
    x, g = X.dist_data(c)
    out.append(("distortion", X.distortion(x, g), X.distortion_bound(x, g)))
    x, gm, gs = X.wide_data(X.WIDE_CASES[1])
    out.append(("widener", X.restate_widener(x, gm, gs).astype(np.float64).reshape(-1, x.shape[-1]), np.zeros((2 * x.shape[0], x.shape[-1]))))
    x, g = X.scale_data(X.SCALE_CASES[0])
    out.append(("scale", X.scale(x, g).astype(np.float32).astype(np.float64), np.zeros(x.shape)))
    out.append(("delay",) + X.delay(*X.delay_data(X.DELAY_CASES[0])))
    out.append(("volume",) + X.volume(*X.vol_data(X.VOL_CASES[0])))
    x, thr, ratio, ca, cr = X.comp_data(X.COMP_CASES[1])
    env, mag = X.comp_env(x, ca, cr)
    out.append(("compressor env", env, X.comp_env_bound(mag)))
    out.append(("compressor y",) + X.compressor_y(x, env.astype(np.float32), thr, ratio))
    x, p = X.limit_data(X.LIMIT_CASES[0])
    y1, b1 = X.limiter_stage1(x, p)
    out.append(("limiter stage 1", y1, b1))
    e2, m2 = X.comp_env(y1.astype(np.float32), p[6], p[7])
    out.append(("limiter y",) + X.limiter_out(y1.astype(np.float32), e2.astype(np.float32), p)[:2])
    c = X.CHORUS_CASES[1]
    a = X.chorus_data(c)
    out.append(("chorus",) + X.chorus(a[0][:, :600], c["sr"], *a[1:]))
    c = X.REVERB_CASES[0]
    a = X.reverb_data(c)
    out.append(("reverb",) + X.reverb(a[0][:, :700], c["sr"], *a[1:]))
    x, geom, coef, _ = X.sox_data(X.SOX_CASES[0])
    ws, wb = X.sox_banks(x, geom, coef)
    out.append(("sox banks", ws[:3], wb[:3]))                                       # the fourth bank's pre-delay is beyond T: silence
    y, yb = X.sox_mix(x, ws.astype(np.float32), coef, 1)
    out.append(("sox mix", y.reshape(-1, y.shape[-1])[:3], yb.reshape(-1, y.shape[-1])[:3]))
    x, sec, _ = X.eq_data(X.EQ_CASES[1])
    out.append(("eq",) + X.eq(x, sec))
    c = X.PHASER_CASES[1]
    x, rate, depth, cen, fb, mix = X.phaser_data(c)
    G, gb = X.phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
    out.append(("phaser coefficients", G, gb))
    out.append(("phaser",) + X.phaser(x, G.astype(np.float32), fb, mix))
    return out


def test_a_sample_shifted_by_one_position_misses_every_bound():
    for name, ref, bound in _main_outputs():
        bad, k = _shifted(ref)
        assert np.abs(bad[..., -1, k] - ref[..., -1, k]) > bound[..., -1, k], (name, "a neighbour's value passes")
        assert not _misses(ref, ref, bound)


def test_defects_of_each_kind_miss_their_bound():
    # one tap dropped: the delay's first echo
    x, D, fb, mix = X.delay_data(X.DELAY_CASES[0])
    y, bound = X.delay(x, D, fb, mix)
    bad = y.copy()
    bad[3, 7:] -= float(mix[3]) * x[3, :-7].astype(np.float64)
    assert _misses(y, bad, bound), "delay: a dropped tap passes"
    # the delay read at n instead of n - D
    assert _misses(y, X.delay(x, np.maximum(D - 1, 0), fb, mix)[0], bound)
    # a coefficient replaced by its neighbour row's
    x, g = X.scale_data(X.SCALE_CASES[0])
    assert _misses(X.scale(x, g).astype(np.float32).astype(np.float64), X.scale(x, np.roll(g, 1)), np.zeros(x.shape))
    x, sec, _ = X.eq_data(X.EQ_CASES[1])
    y, bound = X.eq(x, sec)
    assert _misses(y, X.eq(x, np.roll(sec, 1, axis=0))[0], bound), "eq: the neighbour row's sections pass"
    x, ends, d0, d1 = X.vol_data(X.VOL_CASES[0])
    y, bound = X.volume(x, ends, d0, d1)
    assert _misses(y, X.volume(x, ends, np.roll(d0, 1, axis=0), d1)[0], bound), "volume: the neighbour row's table passes"
    # volume: the ramp's second half computed by the first half's formula is the same value in exact arithmetic; a step of (steps) not (steps - 1) is not
    assert _misses(y, X.volume(x, ends + 1, d0, d1)[0], bound), "volume: segments one sample longer pass"
    x, thr, ratio, ca, cr = X.comp_data(X.COMP_CASES[1])
    env, mag = X.comp_env(x, ca, cr)
    assert _misses(env, X.comp_env(x, np.roll(ca, 1), cr)[0], X.comp_env_bound(mag)), "envelope: the neighbour row's attack passes"
    # a hop sum attributed to the next hop
    c = X.LOUD_CASES[0]
    x, sec, _, _ = X.loud_data(c)
    res = X.loudness(x, sec, c)
    assert _misses(res["hop"], np.roll(res["hop"], 1, axis=1), res["hop_bound"]), "loudness: a hop sum in the next hop passes"
    moved = X.loudness(np.roll(x, c["hop"], axis=-1), sec, c)
    assert abs(moved["lufs"][1] - res["lufs"][1]) > res["lufs_bound"][1]
    # an off-by-one ring length
    c = X.REVERB_CASES[0]
    a = X.reverb_data(c)
    y, bound = X.reverb(a[0][:, :700], c["sr"], *a[1:])
    cl, al = X.reverb_lengths(c["sr"])
    for j in (0, 7, 8, 11):
        lens = list(cl + al)
        lens[j] += 1
        out, _ = X.freeverb(a[0][:, :700].astype(np.float64) * X.GAIN_015, [lens] * 3, a[1], a[2])
        bad = out * a[3].astype(np.float64)[:, None] + a[0][:, :700].astype(np.float64) * a[4].astype(np.float64)[:, None]
        assert _misses(y, bad, bound), ("reverb: ring", j, "one sample longer passes")
    x, geom, coef, _ = X.sox_data(X.SOX_CASES[0])
    ws, wb = X.sox_banks(x, geom, coef)
    for j in (1, 8, 9, 12):
        g2 = geom.copy()
        g2[:, j] += 1
        assert _misses(ws, X.sox_banks(x, g2, coef)[0], wb), ("sox: ring", j, "one sample longer passes")
    g2 = geom.copy()
    g2[2, 0] += 1
    assert _misses(ws, X.sox_banks(x, g2, coef)[0], wb), "sox: a pre-delay one sample longer passes"
    # chorus: the feedback taken from the wrong lane = a pop one sample older
    c = X.CHORUS_CASES[1]
    a = X.chorus_data(c)
    y, bound = X.chorus(a[0][:, :600], c["sr"], *a[1:])
    assert _misses(y, X.chorus(a[0][:, :600], c["sr"] * (1.0 + 1e-4), *a[1:])[0], bound), "chorus: a delay 1e-4 longer passes"
    # phaser: the coefficient of the neighbouring group of four samples
    c = X.PHASER_CASES[1]
    x, rate, depth, cen, fb, mix = X.phaser_data(c)
    G = X.restate_phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
    y, bound = X.phaser(x, G, fb, mix)
    assert _misses(y, X.phaser(x, np.roll(G, 1, axis=1), fb, mix)[0], bound), "phaser: the neighbouring coefficient passes"


def test_fp64_terms_stay_a_fraction_of_the_fp32_rounding():
    """the bound of the fp64 cascades is the output's fp32 rounding; the fp64 term (largest where a 3 Hz shelf's poles sit next to the
    unit circle) only keeps it honest"""
    for c in X.EQ_CASES:
        x, sec, _ = X.eq_data(c)
        y, big = X.cascade(x, sec)
        assert (X.cascade_fp64_term(sec, c["T"], big) < 0.25 * X.HALF * big).all(), c


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", X.LOUD_CASES + X.NORM_CASES, ids=lambda c: "B%d-C%d-T%d-chunk%d-hop%d" % (c["B"], c["C"], c["T"], c["chunk"], c["hop"]))
def test_loudness_gate_margins(c):
    """in the fp64 reference alone every block's loudness is farther from -70 LUFS and from the relative gate than the hop-sum bound
    can move it: the gates decide the same way on the device"""
    x, sec, _, _ = X.loud_data(c)
    dist, margin = X.loud_margins(X.loudness(x, sec, c))
    assert (dist > margin).all(), (float(dist.min()), float(margin.max()))
    assert float(margin.max()) < 1e-6
