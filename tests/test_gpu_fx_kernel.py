"""Every entry point of remfx_amd/csrc/fx.hip through the C ABI on buffers this test allocates, against tests/fx_ref.py (fp64), per
element and per launch form.  The bounds and where their constants come from are in fx_ref's docstring and DESIGN.md 4.23; none is
measured on a kernel.

Buffers: every input and output sits between NaN guards of 4096 elements, outputs are NaN-filled, workspaces are exactly the size the
_ws_floats / _ws_bytes call (or the header) gives, also between guards; inputs have to come back bit for bit; every case runs twice into
fresh buffers: the same bits.  The exception is the loudness measurement: fx_kweight_kernel adds its lanes' partial hop sums with
floating-point atomics, whose order is not fixed, so the hop sums and what follows from them (LUFS, gain, the normalised rows) are
judged by the same bound in both runs.  Stages that leave their intermediate result in a workspace (the compressor's envelope, the
limiter's stage 1 and stage 2 envelope, the SoX banks, the phaser's coefficients) are judged there, and the stage after them given those
very bits.  A failure names the entry point, the forms, the output and the element."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import fx_ref as X
from tests.kernel_harness import Guarded, api, host, judge, report, stop_after_a_device_error, sync, twice  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

_judge = functools.partial(judge, exact="value", equal_inf=True)       # -0 == +0; an infinity the reference has too is a result

def _ids(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k in ("B", "C", "Cin", "T", "NS", "chunk", "hop", "sr", "off", "long"))


# ---- the 16-byte streams: distortion, widener ------------------------------------------------------------------------------------------
def _run_dist(x, g, off=0, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb, Gb = Guarded.of(x, "x", off), Guarded.of(g, "gain")
    Y = Xb if inplace else Guarded(x.size, what="y", off=off)
    sync(L.rfx_fx_distortion(Xb.ptr(), Y.ptr(), B, T, Gb.ptr(), stream()), "rfx_fx_distortion", (B, T))
    Gb.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, T))}


@pytest.mark.parametrize("c", X.DIST_CASES, ids=_ids)
def test_distortion(c):
    """tanhf(g x) by the K rule: the 16-byte body, the scalar tail, T < 4, rows and payloads off 16-byte alignment, the second trip of
    the grid-stride loop; in place gives the same bits"""
    x, g = X.dist_data(c)
    forms = sorted(X.forms_distortion(c))
    a, _ = twice(lambda: _run_dist(x, g, c.get("off", 0)))
    r = _judge(a["y"], X.distortion(x, g), X.distortion_bound(x, g), ctx=("rfx_fx_distortion", "y", *forms))
    assert np.array_equal(_run_dist(x, g, c.get("off", 0), True)["y"], a["y"]), ("rfx_fx_distortion", "in place differs", forms)
    report("FX", "distortion " + _ids(c), [("y", r)])


def _run_wide(x, gm, gs, off=0, inplace=False):
    L, _, stream = api()
    B, T = x.shape[0], x.shape[-1]
    Xb, A, S = Guarded.of(x, "x", off), Guarded.of(gm, "g_mid"), Guarded.of(gs, "g_side")
    Y = Xb if inplace else Guarded(x.size, what="y", off=off)
    sync(L.rfx_fx_widener(Xb.ptr(), Y.ptr(), B, T, A.ptr(), S.ptr(), stream()), "rfx_fx_widener", (B, T))
    A.unchanged(), S.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, 2, T))}


@pytest.mark.parametrize("c", X.WIDE_CASES, ids=_ids)
def test_widener(c):
    """bit for bit the float32 restatement in the reference's operation order (correctly rounded divisions, no fused product), which
    test_fx_ref_cpu.py ties to the recorded reference output and to the fp64 statement; in place gives the same bits"""
    x, gm, gs = X.wide_data(c)
    forms = sorted(X.forms_widener(c))
    a, _ = twice(lambda: _run_wide(x, gm, gs, c.get("off", 0)))
    ref = X.restate_widener(x, gm, gs)
    _judge(a["y"], ref, np.zeros(ref.shape), ctx=("rfx_fx_widener", "y", *forms))
    assert np.array_equal(_run_wide(x, gm, gs, c.get("off", 0), True)["y"], a["y"]), ("rfx_fx_widener", "in place differs", forms)
    report("FX", "widener " + _ids(c), [("y", 0.0)])


# ---- scale, delay, volume --------------------------------------------------------------------------------------------------------------
def _run_scale(x, g, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb, Gb = Guarded.of(x, "x"), Guarded.of(g, "gain")
    Y = Xb if inplace else Guarded(x.size, what="y")
    sync(L.rfx_fx_scale(Xb.ptr(), Y.ptr(), B, T, Gb.ptr(), stream()), "rfx_fx_scale", (B, T))
    Gb.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, T))}


@pytest.mark.parametrize("c", X.SCALE_CASES, ids=_ids)
def test_scale(c):
    """one rounding of the fp64-exact product, bit for bit; the second trip; in place"""
    x, g = X.scale_data(c)
    a, _ = twice(lambda: _run_scale(x, g))
    _judge(a["y"], X.scale(x, g), np.zeros(x.shape), ctx=("rfx_fx_scale", "y", *sorted(X.forms_scale(c))))
    assert np.array_equal(_run_scale(x, g, True)["y"], a["y"])


def _run_delay(x, D, fb, mix):
    L, _, stream = api()
    B, T = x.shape
    bufs = [Guarded.of(x, "x"), Guarded.of(D, "delay"), Guarded.of(fb, "feedback"), Guarded.of(mix, "mix")]
    Y = Guarded(x.size, what="y")
    sync(L.rfx_fx_delay(bufs[0].ptr(), Y.ptr(), B, T, bufs[1].ptr(), bufs[2].ptr(), bufs[3].ptr(), stream()), "rfx_fx_delay", (B, T))
    for b in bufs:
        b.unchanged()
    return {"y": Y.np((B, T))}


@pytest.mark.parametrize("c", X.DELAY_CASES, ids=_ids)
def test_delay(c):
    """counted: one fma per tap, the weight's k - 1 roundings, the mix.  D = 0 and D < 0 (no tap), D = 1 (n taps), 0 < D < T, D = T and
    D > T (no tap); the second trip with D = 200000"""
    x, D, fb, mix = X.delay_data(c)
    ref, bound = X.delay(x, D, fb, mix)
    a, _ = twice(lambda: _run_delay(x, D, fb, mix))
    report("FX", "delay " + _ids(c), [("y", _judge(a["y"], ref, bound, ctx=("rfx_fx_delay", "y", *sorted(X.forms_delay(c)))))])


def _run_volume(x, ends, d0, d1):
    L, _, stream = api()
    B, T = x.shape
    Xb, E, A, Z = Guarded.of(x, "x"), Guarded.of(ends, "seg_end"), Guarded.of(d0, "db_start"), Guarded.of(d1, "db_end")
    sync(L.rfx_fx_volume(Xb.ptr(), B, T, ends.shape[1], E.ptr(), A.ptr(), Z.ptr(), stream()), "rfx_fx_volume", (B, T))
    E.unchanged(), A.unchanged(), Z.unchanged()
    return {"x": Xb.np((B, T))}


@pytest.mark.parametrize("c", X.VOL_CASES, ids=_ids)
def test_volume(c):
    """the dB ramp counted, powf by the K rule; past the table the input bit for bit (bound 0).  S = 1, 3, 64; a zero-length segment,
    one-sample segments, a table ending before, at and beyond T; the second trip"""
    x, ends, d0, d1 = X.vol_data(c)
    ref, bound = X.volume(x, ends, d0, d1)
    a, _ = twice(lambda: _run_volume(x, ends, d0, d1))
    report("FX", "volume " + _ids(c), [("x", _judge(a["x"], ref, bound, ctx=("rfx_fx_volume", "x", *sorted(X.forms_volume(c)))))])


# ---- compressor, limiter ---------------------------------------------------------------------------------------------------------------
def _run_comp(x, thr, ratio, ca, cr, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    bufs = [Guarded.of(x, "x"), Guarded.of(thr, "thr"), Guarded.of(ratio, "ratio"), Guarded.of(ca, "c_attack"), Guarded.of(cr, "c_release")]
    Y = bufs[0] if inplace else Guarded(x.size, what="y")
    nws = int(L.rfx_fx_compressor_ws(B, T))
    assert nws == B * T                                                  # exactly (B, T)
    W = Guarded(nws, what="env_ws")
    sync(L.rfx_fx_compressor(bufs[0].ptr(), Y.ptr(), W.ptr(), B, T, *(b.ptr() for b in bufs[1:]), stream()), "rfx_fx_compressor", (B, T))
    for b in bufs[1 if inplace else 0:]:
        b.unchanged()
    return {"y": Y.np((B, T)), "env": W.np((B, T))}


@pytest.mark.parametrize("c", X.COMP_CASES, ids=_ids)
def test_compressor(c):
    """the envelope in its (B, T) workspace by the K rule against the majorant of its own recurrence; y counted given that envelope
    (bit for bit x below the threshold).  B = 1, 3, 64, 65, 130: one to three workgroups, a partly filled wave; T < 32, the prefetch
    loop with and without a scalar tail; the output pass's second trip; in place"""
    x, thr, ratio, ca, cr = X.comp_data(c)
    forms = sorted(X.forms_compressor(c))
    env, mag = X.comp_env(x, ca, cr)
    a, _ = twice(lambda: _run_comp(x, thr, ratio, ca, cr))
    r1 = _judge(a["env"], env, X.comp_env_bound(mag), ctx=("rfx_fx_compressor", "env_ws", *forms))
    y, yb = X.compressor_y(x, a["env"], thr, ratio)
    r2 = _judge(a["y"], y, yb, ctx=("rfx_fx_compressor", "y", *forms))
    b = _run_comp(x, thr, ratio, ca, cr, True)
    assert np.array_equal(b["y"], a["y"]) and np.array_equal(b["env"], a["env"]), ("rfx_fx_compressor", "in place differs", forms)
    report("FX", "compressor " + _ids(c), [("env", r1), ("y", r2)])


def _run_limit(x, p, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb, P = Guarded.of(x, "x"), Guarded.of(p, "params")
    Y = Xb if inplace else Guarded(x.size, what="y")
    nws = int(L.rfx_fx_limiter_ws(B, T))
    assert nws == 2 * B * T                                              # exactly 2 B T
    W = Guarded(nws, what="ws")
    sync(L.rfx_fx_limiter(Xb.ptr(), Y.ptr(), W.ptr(), B, T, P.ptr(), stream()), "rfx_fx_limiter", (B, T))
    P.unchanged()
    if not inplace:
        Xb.unchanged()
    w = W.np((2, B, T))
    return {"y": Y.np((B, T)), "env2": w[0], "y1": w[1]}


@pytest.mark.parametrize("c", X.LIMIT_CASES, ids=_ids)
def test_limiter(c):
    """2 B T floats of workspace, which keep stage 2's envelope and stage 1's output: stage 1 against the fp64 compressor with its
    envelope's bound carried through the gain computer's slope; stage 2's envelope by the K rule against the envelope of those very
    stage-1 bits; y counted given both, the clip engaged on the rows whose make-up is not clamped; in place"""
    x, p = X.limit_data(c)
    forms = sorted(X.forms_limiter(c))
    y1, b1 = X.limiter_stage1(x, p)
    a, _ = twice(lambda: _run_limit(x, p))
    r1 = _judge(a["y1"], y1, b1, ctx=("rfx_fx_limiter", "ws stage 1", *forms))
    e2, m2 = X.comp_env(a["y1"], p[6], p[7])
    r2 = _judge(a["env2"], e2, X.comp_env_bound(m2), ctx=("rfx_fx_limiter", "ws envelope 2", *forms))
    y, yb, _ = X.limiter_out(a["y1"], a["env2"], p)
    r3 = _judge(a["y"], y, yb, ctx=("rfx_fx_limiter", "y", *forms))
    assert np.array_equal(_run_limit(x, p, True)["y"], a["y"]), ("rfx_fx_limiter", "in place differs", forms)
    report("FX", "limiter " + _ids(c), [("stage1", r1), ("env2", r2), ("y", r3)])


# ---- chorus, reverb --------------------------------------------------------------------------------------------------------------------
def _run_chorus(x, sr, prm, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb = Guarded.of(x, "x")
    P = [Guarded.of(p, n) for p, n in zip(prm, ("rate", "depth", "centre", "feedback", "mix"))]
    Y = Xb if inplace else Guarded(x.size, what="y")
    sync(L.rfx_fx_chorus(Xb.ptr(), Y.ptr(), B, T, float(sr), *(p.ptr() for p in P), stream()), "rfx_fx_chorus", (B, T, sr))
    for p in P:
        p.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, T))}


@pytest.mark.parametrize("c", X.CHORUS_CASES, ids=_ids)
def test_chorus(c):
    """K rule on the majorant plus the delay's float32 uncertainty times the local slope, no sample excluded.  Blocks of 2 (4 kHz), 46,
    64 (66 kHz) and 64 capped (80 kHz); T = 4200 wraps the 4096-sample ring; a delay of 46 ms at 80 kHz reaches back 3680 samples, past
    half the ring; the 1 ms floor; taps before the clip's start; mix = 0
    gives x bit for bit; in place"""
    a_ = X.chorus_data(c)
    forms = sorted(X.forms_chorus(c))
    ref, bound = X.chorus(a_[0], c["sr"], *a_[1:])
    a, _ = twice(lambda: _run_chorus(a_[0], c["sr"], a_[1:]))
    r = _judge(a["y"], ref, bound, ctx=("rfx_fx_chorus", "y", *forms))
    assert np.array_equal(_run_chorus(a_[0], c["sr"], a_[1:], True)["y"], a["y"]), ("rfx_fx_chorus", "in place differs", forms)
    report("FX", "chorus " + _ids(c), [("y", r)])


def _run_reverb(x, sr, prm, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb = Guarded.of(x, "x")
    P = [Guarded.of(p, n) for p, n in zip(prm, ("damp", "feedback", "wet1", "dry"))]
    Y = Xb if inplace else Guarded(x.size, what="y")
    rc = L.rfx_fx_reverb(Xb.ptr(), Y.ptr(), B, T, int(sr), *(p.ptr() for p in P), stream())
    torch.cuda.synchronize()
    for p in P:
        p.unchanged()
    if not inplace:
        Xb.unchanged()
    return rc, Y


@pytest.mark.parametrize("c", X.REVERB_CASES, ids=_ids)
def test_reverb(c):
    """K rule on the majorant of the twelve rings.  12544 Hz: rings of 64 ... 459 samples, T = 2000 wraps each several times; 48000 Hz;
    a clip shorter than every ring; a whole and a partial last block; in place"""
    a_ = X.reverb_data(c)
    forms = sorted(X.forms_reverb(c))
    ref, bound = X.reverb(a_[0], c["sr"], *a_[1:])

    def run(inplace=False):
        rc, Y = _run_reverb(a_[0], c["sr"], a_[1:], inplace)
        assert rc == 0, ("rfx_fx_reverb", rc, forms)
        return {"y": Y.np(a_[0].shape)}
    a, _ = twice(run)
    r = _judge(a["y"], ref, bound, ctx=("rfx_fx_reverb", "y", *forms))
    assert np.array_equal(run(True)["y"], a["y"]), ("rfx_fx_reverb", "in place differs", forms)
    report("FX", "reverb " + _ids(c), [("y", r)])


def test_reverb_rate_range():
    """12543 Hz (the shortest ring is 63 samples: below a block) and 143527 Hz (the rings exceed 160 KB of LDS) are refused and
    nothing is written; 12544 Hz and 143526 Hz render"""
    lo, hi = X.reverb_rate_range()
    c = dict(B=2, T=70)
    a_ = X.reverb_data(c)
    for sr in (lo - 1, hi + 1, 7999, 192001):
        rc, Y = _run_reverb(a_[0], sr, a_[1:])
        assert rc == -1, ("rfx_fx_reverb accepted", sr)
        Y.untouched()
    for sr in (lo, hi):
        rc, Y = _run_reverb(a_[0], sr, a_[1:])
        assert rc == 0, ("rfx_fx_reverb refused", sr, rc)
        ref, bound = X.reverb(a_[0], sr, *a_[1:])
        _judge(Y.np(a_[0].shape), ref, bound, ctx=("rfx_fx_reverb", "y", "rate", sr))


# ---- SoX reverb ------------------------------------------------------------------------------------------------------------------------
def _run_sox(x, geom, coef, lds, Cin):
    L, _, stream = api()
    B, T = x.shape[0], x.shape[-1]
    Xb, G, Cf = Guarded.of(x, "x"), Guarded.of(geom, "geom"), Guarded.of(coef, "coef")
    n = int(L.rfx_fx_sox_reverb_ws_floats(B, Cin, T))
    assert n == B * Cin * 2 * T
    W, Y = Guarded(n, what="ws"), Guarded(B * 2 * T, what="y")
    sync(L.rfx_fx_sox_reverb(Xb.ptr(), Y.ptr(), W.ptr(), B, Cin, T, G.ptr(), Cf.ptr(), lds, stream()), "rfx_fx_sox_reverb", (B, Cin, T))
    Xb.unchanged(), G.unchanged(), Cf.unchanged()
    return {"y": Y.np((B, 2, T)), "ws": W.np((B * Cin * 2, T))}


@pytest.mark.parametrize("c", X.SOX_CASES, ids=_ids)
def test_sox_reverb(c):
    """the banks in ws by the K rule on their majorant, y counted given those banks.  Geometry passed directly: banks of 64 ... 75
    (blocks of 64), with a 63 and a 7 (narrowed blocks), with a 1 (a one-lane scan); pre-delay 0, inside the clip, T and beyond; mono and
    stereo input; ws exactly rfx_fx_sox_reverb_ws_floats"""
    x, geom, coef, lds = X.sox_data(c)
    forms = sorted(X.forms_sox(c))
    ws, wb = X.sox_banks(x, geom, coef)
    a, _ = twice(lambda: _run_sox(x, geom, coef, lds, c["Cin"]))
    r1 = _judge(a["ws"], ws, wb, ctx=("rfx_fx_sox_reverb", "ws banks", *forms))
    y, yb = X.sox_mix(x, a["ws"], coef, c["Cin"])
    r2 = _judge(a["y"], y, yb, ctx=("rfx_fx_sox_reverb", "y", *forms))
    report("FX", "sox_reverb " + _ids(c), [("banks", r1), ("y", r2)])


@pytest.mark.parametrize("bad", ("length_0", "beyond_lds"))
def test_sox_reverb_nan_plan(bad):
    """the one refusal inside a kernel, as the header describes it: a bank with a length of 0, or whose lengths exceed lds_floats,
    renders NaN -- that bank's row of ws and the one channel of y it feeds; every other row is the reference's"""
    c = X.SOX_CASES[0]
    x, geom, coef, lds = X.sox_data(c)
    geom = geom.copy()
    if bad == "length_0":
        geom[2, 5] = 0
    else:
        geom[2, 5] = lds + 1
    a = _run_sox(x, geom, coef, lds, 1)
    assert np.isnan(a["ws"][2]).all() and np.isnan(a["y"][1, 0]).all(), "the refused bank did not render NaN"
    good = np.ones(4, bool)
    good[2] = False
    g2 = geom.copy()
    g2[2] = geom[3]                                                        # any valid plan: the row is not judged
    ws, wb = X.sox_banks(x, g2, coef)
    _judge(a["ws"][good], ws[good], wb[good], ctx=("rfx_fx_sox_reverb", "ws banks", bad))
    wsd = np.where(good[:, None], a["ws"], 0.0).astype(np.float32)
    y, yb = X.sox_mix(x, wsd, coef, 1)
    yr, ybr = y.reshape(4, -1), yb.reshape(4, -1)
    _judge(a["y"].reshape(4, -1)[good], yr[good], ybr[good], ctx=("rfx_fx_sox_reverb", "y", bad))


# ---- EQ --------------------------------------------------------------------------------------------------------------------------------
def _run_eq(x, coef, NS, chunk, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb, Cf = Guarded.of(x, "x"), Guarded.of(coef, "coef")
    Y = Xb if inplace else Guarded(x.size, what="y")
    sync(L.rfx_fx_eq(Xb.ptr(), Y.ptr(), B, T, NS, chunk, Cf.ptr(), stream()), "rfx_fx_eq", (B, T, NS, chunk))
    Cf.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, T))}


@pytest.mark.parametrize("c", X.EQ_CASES, ids=_ids)
def test_eq(c):
    """every fx_eq_kernel<NS>, NS = 2 ... 8: the fp32 rounding of the fp64 cascade plus the fp64 term.  chunk * 64 == T, a short last
    chunk, empty chunks, one chunk only; per-row sections; in place"""
    x, sec, coef = X.eq_data(c)
    forms = sorted(X.forms_eq(c))
    ref, bound = X.eq(x, sec)
    a, _ = twice(lambda: _run_eq(x, coef, c["NS"], c["chunk"]))
    r = _judge(a["y"], ref, bound, ctx=("rfx_fx_eq", "y", *forms))
    assert np.array_equal(_run_eq(x, coef, c["NS"], c["chunk"], True)["y"], a["y"]), ("rfx_fx_eq", "in place differs", forms)
    report("FX", "eq " + _ids(c), [("y", r)])


# ---- loudness --------------------------------------------------------------------------------------------------------------------------
def _run_loud(x, c, coef, inv, joint):
    L, _, stream = api()
    B, Cc, T = x.shape
    Xb = Guarded.of(x, "x")
    geom = (T, c["chunk"], c["hop"], c["nhop"], c["nblk"])
    nws = int(L.rfx_fx_loudness_joint_ws(B, Cc, *geom)) if joint else int(L.rfx_fx_loudness_ws(B, *geom))
    assert nws == B * Cc * c["nhop"]                                     # nhop hop sums per row
    H, Lu, Ga = Guarded(nws, torch.float64, "hop_ws"), Guarded(B, what="lufs"), Guarded(B, what="gain")
    tail = (c["chunk"], c["hop"], c["nhop"], c["nblk"], inv, host(coef), X.LOUD_TARGET, H.ptr(), Lu.ptr(), Ga.ptr(), stream())
    rc = L.rfx_fx_loudness_joint(Xb.ptr(), B, Cc, T, *tail) if joint else L.rfx_fx_loudness(Xb.ptr(), B, T, *tail)
    sync(rc, "rfx_fx_loudness", (B, Cc, T))
    Xb.unchanged()
    return {"hop": H.np((B * Cc, c["nhop"])), "lufs": Lu.np(), "gain": Ga.np()}


def _judge_loud(entry, got, res, forms):
    return [("hop", _judge(got["hop"], res["hop"], res["hop_bound"], ctx=(entry, "hop_ws", *forms))),
            ("lufs", _judge(got["lufs"], res["lufs"], res["lufs_bound"], ctx=(entry, "lufs", *forms))),
            ("gain", _judge(got["gain"], res["gain"], res["gain_bound"], ctx=(entry, "gain", *forms)))]


@pytest.mark.parametrize("c", X.LOUD_CASES, ids=_ids)
def test_loudness(c):
    """rfx_fx_loudness (C = 1, and the joint entry point at C = 1 too) and rfx_fx_loudness_joint: the hop sums in hop_ws, LUFS and the
    gain.  chunk and hop passed directly: hop borders inside a chunk and on a chunk border, several hops per chunk, samples past the
    hops, a short last chunk, chunk * 64 == T, most chunks empty, one chunk; rows removed by the relative gate, rows below -70 LUFS
    throughout (-inf, gain 100); B = 64, 65, 130.  Both runs are judged by the bound: the hop sums are added with atomics"""
    x, sec, coef, inv = X.loud_data(c)
    forms = sorted(X.forms_loudness(c))
    res = X.loudness(x, sec, c)
    ratios = []
    for joint in ((True,) if c["C"] > 1 else (False, True)):
        for got in twice(lambda: _run_loud(x, c, coef, inv, joint), same_bits=False):
            ratios += _judge_loud("rfx_fx_loudness_joint" if joint else "rfx_fx_loudness", got, res, forms)
    report("FX", "loudness " + _ids(c), ratios)


@pytest.mark.parametrize("c", X.NORM_CASES, ids=_ids)
def test_normalize_rows(c):
    """ws of exactly rfx_fx_normalize_ws_bytes: the hop sums, lufs and gain stay readable there; y[rows[i]] = gain[i] x[i] bit for bit
    given that gain, with a permuted table into a larger state whose other rows keep their NaN; without a table, row i, also in
    place of x"""
    L, _, stream = api()
    x, sec, coef, inv = X.loud_data(c)
    n, T, N, nhop = c["B"], c["T"], c["N"], c["nhop"]
    res = X.loudness(x, sec, c)
    nbytes = int(L.rfx_fx_normalize_ws_bytes(n, nhop))
    assert nbytes == n * nhop * 8 + 2 * n * 4
    rows = None if c["rows"] is None else np.asarray(c["rows"], np.int32)

    def run(inplace=False):
        Xb = Guarded.of(x, "x")
        Y = Xb if inplace else Guarded(N * T, what="y")
        W = Guarded(nbytes // 4, what="ws")
        R = None if rows is None else Guarded.of(rows, "rows")
        rc = L.rfx_fx_normalize_rows(Xb.ptr(), Y.ptr(), R.ptr() if R else None, n, T, c["chunk"], c["hop"], nhop, c["nblk"], inv, host(coef),
                                     X.LOUD_TARGET, W.ptr(), stream())
        sync(rc, "rfx_fx_normalize_rows", (n, T))
        if R:
            R.unchanged()
        if not inplace:
            Xb.unchanged()
        w = W.np()
        return {"y": Y.np((N, T)), "hop": w[:n * nhop * 2].view(np.float64).reshape(n, nhop), "lufs": w[n * nhop * 2:n * nhop * 2 + n],
                "gain": w[n * nhop * 2 + n:]}
    forms = sorted(X.forms_loudness(c))
    ratios = []
    for got in twice(run, same_bits=False) + ((run(True),) if rows is None else ()):
        ratios += _judge_loud("rfx_fx_normalize_rows", got, res, forms)
        target = list(range(n)) if rows is None else list(rows)
        _judge(got["y"][target], X.scale(x[:, 0], got["gain"]), np.zeros((n, T)), ctx=("rfx_fx_normalize_rows", "y", *forms))
        others = [r for r in range(N) if r not in target]
        assert np.isnan(got["y"][others]).all(), "a row outside the table was written"
    report("FX", "normalize_rows " + _ids(c), ratios)


# ---- phaser ----------------------------------------------------------------------------------------------------------------------------
def _run_phaser(x, prm, inplace=False):
    L, _, stream = api()
    B, T = x.shape
    Xb = Guarded.of(x, "x")
    P = [Guarded.of(p, n) for p, n in zip(prm, ("rate", "depth", "centre", "feedback", "mix"))]
    n = int(L.rfx_fx_phaser_ws_floats(B, T))
    assert n == X.phaser_ws_floats(B, T)
    W = Guarded(n, what="ws")
    Y = Xb if inplace else Guarded(x.size, what="y")
    sync(L.rfx_fx_phaser(Xb.ptr(), Y.ptr(), W.ptr(), B, T, X.PHASER_SR, *(p.ptr() for p in P), stream()), "rfx_fx_phaser", (B, T))
    for p in P:
        p.unchanged()
    if not inplace:
        Xb.unchanged()
    return {"y": Y.np((B, T)), "G": W.np((B, n // B))}


@pytest.mark.parametrize("c", X.PHASER_CASES, ids=_ids)
def test_phaser(c):
    """the coefficient stream left in ws, all of it, by the K rule (the padding of a row keeps its NaN); y by the K rule given those
    coefficients -- on the first 4096 samples where T = 2097202 takes the coefficient pass into its second trip.  B = 1, 3, 64, 65, 130;
    T < 32, the prefetch loop with and without tail; mix = 0 gives x bit for bit; in place"""
    x, rate, depth, cen, fb, mix = X.phaser_data(c)
    forms = sorted(X.forms_phaser(c))
    M = (c["T"] + 3) // 4
    G, gb = X.phaser_coef(c["T"], X.PHASER_SR, rate, depth, cen)
    a, _ = twice(lambda: _run_phaser(x, (rate, depth, cen, fb, mix)))
    r1 = _judge(a["G"][:, :M], G, gb, ctx=("rfx_fx_phaser", "ws coefficients", *forms))
    assert np.isnan(a["G"][:, M:]).all(), "the padding of a coefficient row was written"
    n = c.get("prefix", c["T"])
    y, yb = X.phaser(x[:, :n], a["G"], fb, mix)
    r2 = _judge(a["y"][:, :n], y, yb, ctx=("rfx_fx_phaser", "y", *forms))
    assert np.isfinite(a["y"]).all()
    assert np.array_equal(_run_phaser(x, (rate, depth, cen, fb, mix), True)["y"], a["y"]), ("rfx_fx_phaser", "in place differs", forms)
    report("FX", "phaser " + _ids(c), [("G", r1), ("y", r2)])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refusal_table():
    """(entry point, valid arguments, outputs, [(argument index, refused value)]): every -1 condition of the launch code.  The checks are
    on the host: no call of this table launches a kernel"""
    B, T = 2, 8
    f = lambda n, what: Guarded(n, what=what, init=torch.full((n,), 0.5))                        # noqa: E731
    i = lambda n, what, v: Guarded(n, torch.int32, what, torch.full((n,), v, dtype=torch.int32))      # noqa: E731
    out = []
    nul = lambda idx: [(k, None) for k in idx]                                                # noqa: E731
    x, y = f(B * T, "x"), Guarded(B * T, what="y")
    g = f(B, "p")
    dims = [(2, 0), (2, -1), (2, 65536), (3, 0), (3, -1)]
    out.append(("rfx_fx_distortion", [x.ptr(), y.ptr(), B, T, g.ptr()], [y], nul((0, 1, 4)) + dims))
    d = i(B, "delay", 3)
    out.append(("rfx_fx_delay", [x.ptr(), y.ptr(), B, T, d.ptr(), g.ptr(), g.ptr()], [y], nul((0, 1, 4, 5, 6)) + dims + [(1, x.ptr())]))
    out.append(("rfx_fx_chorus", [x.ptr(), y.ptr(), B, T, 48000.0, g.ptr(), g.ptr(), g.ptr(), g.ptr(), g.ptr()], [y],
                nul((0, 1, 5, 6, 7, 8, 9)) + dims + [(4, 3999.0), (4, 2999.0), (4, 81000.0)]))
    w = Guarded(2 * B * T, what="ws")
    out.append(("rfx_fx_compressor", [x.ptr(), y.ptr(), w.ptr(), B, T, g.ptr(), g.ptr(), g.ptr(), g.ptr()], [y, w],
                nul((0, 1, 2, 5, 6, 7, 8)) + [(3, 0), (3, 65536), (4, 0)]))
    out.append(("rfx_fx_reverb", [x.ptr(), y.ptr(), B, T, 48000, g.ptr(), g.ptr(), g.ptr(), g.ptr()], [y],
                nul((0, 1, 5, 6, 7, 8)) + dims + [(4, 7999), (4, 192001), (4, 12543), (4, 143527)]))
    p9 = f(9 * B, "params")
    out.append(("rfx_fx_limiter", [x.ptr(), y.ptr(), w.ptr(), B, T, p9.ptr()], [y, w], nul((0, 1, 2, 5)) + [(3, 0), (3, 65536), (4, 0)]))
    cf = Guarded(B * (10 + 16), torch.float64, "coef", torch.zeros(B * 26, dtype=torch.float64))
    out.append(("rfx_fx_eq", [x.ptr(), y.ptr(), B, T, 2, 1, cf.ptr()], [y],
                nul((0, 1, 6)) + dims + [(4, 1), (4, 9), (4, 0), (5, 0), (5, -1)]))
    x64 = f(B * 65, "x65")                                                                     # T = 65 with chunk 1: chunk * 64 < T
    out.append(("rfx_fx_eq", [x64.ptr(), y.ptr(), B, 65, 2, 1, cf.ptr()], [y], [(5, 1)]))
    x2 = f(B * 2 * T, "x stereo")
    y2 = Guarded(B * 2 * T, what="y stereo")
    out.append(("rfx_fx_widener", [x2.ptr(), y2.ptr(), B, T, g.ptr(), g.ptr()], [y2], nul((0, 1, 4, 5)) + dims))
    xv = Guarded(B * T, what="x in place")
    e = i(B * 2, "seg_end", 4)
    g2 = f(B * 2, "db")
    out.append(("rfx_fx_volume", [xv.ptr(), B, T, 2, e.ptr(), g2.ptr(), g2.ptr()], [xv],
                nul((0, 4, 5, 6)) + [(1, 0), (1, 65536), (2, 0), (3, 0), (3, 65), (3, -1)]))
    pw = Guarded(B * 8, what="phaser ws")
    out.append(("rfx_fx_phaser", [x.ptr(), y.ptr(), pw.ptr(), B, T, 8000.0, g.ptr(), g.ptr(), g.ptr(), g.ptr(), g.ptr()], [y, pw],
                nul((0, 1, 2, 6, 7, 8, 9, 10)) + [(3, 0), (3, 65536), (4, 0), (5, 0.0), (5, -1.0)]))
    out.append(("rfx_fx_scale", [x.ptr(), y.ptr(), B, T, g.ptr()], [y], nul((0, 1, 4)) + dims))
    geom = i(B * 2 * 16, "geom", 70)
    c4 = f(B * 2 * 4, "coef")
    ws = Guarded(B * 2 * T, what="sox ws")
    out.append(("rfx_fx_sox_reverb", [x.ptr(), y2.ptr(), ws.ptr(), B, 1, T, geom.ptr(), c4.ptr(), 840], [y2, ws],
                nul((0, 1, 2, 6, 7)) + [(3, 0), (3, 32768), (5, 0), (4, 0), (4, 3), (8, 11), (8, 40961), (1, x.ptr())]))
    coef = np.zeros(28)
    hop, lu, ga = Guarded(B * 5, torch.float64, "hop_ws"), Guarded(B, what="lufs"), Guarded(B, what="gain")
    # T = 8: chunk 1, hop 2, nhop 4, nblk 1
    la = [x.ptr(), B, T, 1, 2, 4, 1, 0.125, host(coef), -32.0, hop.ptr(), lu.ptr(), ga.ptr()]
    lbad = [(1, 0), (1, 65536), (2, 0), (3, 0), (4, 0), (5, 3), (6, 0), (6, 2)]
    out.append(("rfx_fx_loudness", la, [hop, lu, ga], nul((0, 8, 10, 11, 12)) + lbad))
    out.append(("rfx_fx_loudness", [x64.ptr(), B, 65, 1, 2, 4, 1, 0.125, host(coef), -32.0, hop.ptr(), lu.ptr(), ga.ptr()], [hop, lu, ga], [(3, 1)]))
    lj = [x.ptr(), 1, 2, T, 1, 2, 4, 1, 0.125, host(coef), -32.0, hop.ptr(), lu.ptr(), ga.ptr()]
    out.append(("rfx_fx_loudness_joint", lj, [hop, lu, ga], nul((0, 9, 11, 12, 13)) + [(1, 0), (2, 0), (1, 65536), (3, 0), (4, 0), (5, 0), (6, 3), (7, 0), (7, 2)]))
    nw = Guarded((B * 4 * 8 + 2 * B * 4) // 4, what="normalize ws")
    rows = i(B, "rows", 0)
    na = [x.ptr(), y.ptr(), rows.ptr(), B, T, 1, 2, 4, 1, 0.125, host(coef), -32.0, nw.ptr()]
    out.append(("rfx_fx_normalize_rows", na, [y, nw], nul((0, 1, 10, 12)) + [(3, 0), (3, 65536), (4, 0), (5, 0), (6, 0), (7, 3), (8, 0), (8, 2), (1, x.ptr())]))
    return out, (coef,)


def test_refusals():
    """every -1 condition of the launch code, one call each: the return value is -1 and the outputs keep their NaN fill"""
    L, _, stream = api()
    table, keep = _refusal_table()
    count = 0
    for entry, args, outs, bad in table:
        for idx, val in bad:
            a = list(args)
            a[idx] = val
            rc = getattr(L, entry)(*a, stream())
            torch.cuda.synchronize()
            assert rc == -1, (entry, "argument", idx, "=", val if not isinstance(val, C.c_void_p) else "x", "returned", rc)
            for o in outs:
                o.untouched()
            count += 1
    print(f"\nFX refusals: {count} calls, each -1 with nothing written")
