"""Every training-loss entry point of remfx_amd/csrc/losses.hip that sections 4.21 / 4.22 of DESIGN.md do not pin, through the C ABI on
buffers this test allocates, against tests/loss_ref.py (fp64 and exact rational), per element and per launch form.  The bounds and
where their constants come from are in loss_ref's docstring and DESIGN.md 4.24; none is measured on a kernel.

Buffers (`Guarded` / `judge` of tests/kernel_harness.py): every input, output and workspace sits between NaN guards of 4096
elements, outputs and workspaces are NaN-filled, workspaces are exactly the size rfx_time_sums_ws / rfx_logcosh_ws /
rfx_stft_scaled_loss_ws return (5 R g doubles for rfx_sisdr_sums), inputs have to come back bit for bit, every case runs twice into
fresh buffers: the same bits (all of these kernels are order-free).  The padding between strided rows holds 1e30, so a halo read across
a row end shows in the value.  A failure names the entry point, the forms, the output and the element."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import loss_ref as X
from tests.kernel_harness import Guarded, api, judge, report, stop_after_a_device_error, sync, twice  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

KIND = {k: i for i, k in enumerate(X.KINDS)}
RED = {k: i for i, k in enumerate(X.REDUCTIONS)}
F64 = torch.float64
_judge = functools.partial(judge, exact="value", equal_inf=True)       # -0 == +0; an infinity the reference has too is a result


def _mel(sr, n_fft, n_mels):
    from remfx_amd.losses import mel_filterbank
    return mel_filterbank(sr, n_fft, n_mels).numpy()


def _taps(c):
    return None if c["taps"] is None else X.TAPS[c["taps"]]


def _h(taps):
    return (1, *taps) if taps is not None else (0, 0.0, 1.0, 0.0)


# ---- row sums ----------------------------------------------------------------------------------------------------------------------------
def _run_sums(c, entry, data=None):
    L_, _, stream = api()
    R, L = c["R"], c["L"]
    _, _, (xb, xs), (tb, ts) = data or X.time_data(c)
    Xb, Tb = Guarded.of(xb, "x", c["ox"]), Guarded.of(tb, "t", c["ot"])
    S = Guarded(5 * R, F64, "sums")
    if entry == "rfx_sisdr_sums":
        n, used = int(L_.rfx_sisdr_sums_ws(R, L)), 5 * R * X.time_sums_grid(L)
        assert n == 5 * R * X.SLOTS                            # the restated cap per row and sum, for every L
        W = Guarded(n, F64, "ws")
        rc = L_.rfx_sisdr_sums(Xb.ptr(), Tb.ptr(), R, L, xs, ts, W.ptr(), S.ptr(), stream())
    else:
        n = used = int(L_.rfx_time_sums_ws(R, L))
        assert n == 5 * R * X.time_sums_grid(L)
        W = Guarded(n, F64, "ws")
        rc = L_.rfx_time_sums(Xb.ptr(), Tb.ptr(), R, L, xs, ts, *_h(_taps(c)), W.ptr(), S.ptr(), stream())
    sync(rc, entry, (R, L))
    Xb.unchanged(), Tb.unchanged()
    ws = W.np()
    assert np.isfinite(ws[:used]).all() and np.isnan(ws[used:]).all(), (entry, "slots written", used)
    return {"sums": S.np((R, 5))}


@pytest.mark.parametrize("c", X.TIME_CASES, ids=X.case_id)
def test_time_sums(c):
    """the five sums of the zero-padded three-tap filtered rows (rfx_time_sums, with its taps) and of the rows themselves
    (rfx_sisdr_sums; rfx_time_sums without taps returns its bits)"""
    data = X.time_data(c)
    x, t = data[0], data[1]
    a, _ = twice(lambda: _run_sums(c, "rfx_time_sums", data))
    ref, bound = X.row_sums(x, t, _taps(c))
    r1 = _judge(a["sums"], ref, bound, ctx=("rfx_time_sums", "sums", *sorted(X.forms_time_sums(c))))
    plain = dict(c, taps=None)
    b, _ = twice(lambda: _run_sums(plain, "rfx_sisdr_sums", data))
    ref, bound = X.row_sums(x, t, None)
    r2 = _judge(b["sums"], ref, bound, ctx=("rfx_sisdr_sums", "sums", *sorted(X.forms_sisdr_sums(c))))
    if c["taps"] is None:
        assert np.array_equal(a["sums"].view(np.uint8), b["sums"].view(np.uint8)), "rfx_time_sums without taps is not rfx_sisdr_sums"
    report("LOSS", "sums " + X.case_id(c), [("rfx_time_sums", r1), ("rfx_sisdr_sums", r2)])


def test_sisdr_sums_one_workgroup_past_the_cap():
    """R = 1, L = 128 x 2048 + 1: the row asks for one workgroup more than the capped grid has; ws is exactly rfx_sisdr_sums_ws doubles
    between its guards, the slots of the 128 workgroups written and no other"""
    L = X.SLOTS * 2048 + 1
    assert X.grid_x(L) == X.SLOTS + 1 and X.time_sums_grid(L) == X.SLOTS
    c = dict(next(c for c in X.TIME_CASES if c["R"] == 1 and c["kind"] == "sisdr"), L=L, taps=None, seed=1000 + 7 * L + 1)
    data = X.time_data(c)
    b, _ = twice(lambda: _run_sums(c, "rfx_sisdr_sums", data))
    ref, bound = X.row_sums(data[0], data[1], None)
    r = _judge(b["sums"], ref, bound, ctx=("rfx_sisdr_sums", "sums", "grid_capped"))
    report("LOSS", "sums " + X.case_id(c), [("rfx_sisdr_sums", r)])


# ---- per-row losses, the SI-SDR tail ---------------------------------------------------------------------------------------------------
def _run_rows(sums, L, kind, zm, red, eps=1e-8, coef=True):
    L_, _, stream = api()
    R = sums.shape[0]
    S = Guarded.of(sums, "sums")
    Rw, Cf, O = Guarded(R, what="rows"), Guarded(3 * R, F64, "coef"), Guarded(1, what="out")
    rc = L_.rfx_time_loss_rows(S.ptr(), R, L, KIND[kind], zm, eps, RED[red], Rw.ptr(), Cf.ptr() if coef else None, O.ptr(), stream())
    sync(rc, "rfx_time_loss_rows", (R, L, kind, zm, red))
    S.unchanged()
    out = {"rows": Rw.np()}
    if coef:
        out["coef"] = Cf.np((R, 3))
    else:
        Cf.untouched()
    if red == "none":
        O.untouched()
    else:
        out["out"] = O.np()
    return out


def _run_finish(sums, L, zm, eps=1e-8):
    L_, _, stream = api()
    S, O = Guarded.of(sums, "sums"), Guarded(1, what="out")
    sync(L_.rfx_sisdr_finish(S.ptr(), sums.shape[0], L, zm, eps, O.ptr(), stream()), "rfx_sisdr_finish", (sums.shape[0], L))
    S.unchanged()
    return {"out": O.np()}


ROWS_CASES = [c for c in X.TIME_CASES if c["L"] < 100000]


@pytest.mark.parametrize("c", ROWS_CASES, ids=X.case_id)
def test_time_loss_rows(c):
    """rows, coef and out of all five ratio kinds, centred and not, mean / sum / none, from the reference's sums of the case's signals
    (rounded to fp64: the kernel's input, exact for the reference); rfx_sisdr_finish returns the bits of SI-SDR with "mean".  L = 1 is
    not centred: a one-sample row minus its mean is no signal."""
    x, t, _, _ = X.time_data(c)
    sums, _ = X.row_sums(x, t, _taps(c))
    ratios = {}
    for kind in X.KINDS[:5]:
        for zm in ((0,) if c["L"] == 1 else (0, 1)):
            if kind in ("esr", "dc") and zm:
                continue
            base = X.time_loss_rows(sums, c["L"], kind, zm, 1e-8, "none")
            for red in X.REDUCTIONS:
                info = (kind, zm, red, sorted(X.forms_rows(kind, zm, red, c["R"])))
                ref = X.reduce_rows(base, red)
                a, _ = twice(lambda: _run_rows(sums, c["L"], kind, zm, red))
                for k in ("rows", "coef") + (("out",) if red != "none" else ()):
                    ratios[k] = max(ratios.get(k, 0.0), _judge(a[k], ref[k], ref[k + "_bound"], ctx=("rfx_time_loss_rows", k, *info)))
                if kind == "sisdr" and red == "mean":
                    f, _ = twice(lambda: _run_finish(sums, c["L"], zm))
                    ratios["finish"] = max(ratios.get("finish", 0.0), _judge(f["out"], ref["out"], ref["out_bound"], ctx=("rfx_sisdr_finish", "out", *info)))
                    assert np.array_equal(f["out"].view(np.uint8), a["out"].view(np.uint8)), "rfx_sisdr_finish differs from SI-SDR mean"
    b = _run_rows(sums, c["L"], "sisdr", 1 if c["L"] > 1 else 0, "none", coef=False)
    assert np.isfinite(b["rows"]).all()
    report("LOSS", "rows " + X.case_id(c), sorted(ratios.items()))


# ---- the gradient pass -------------------------------------------------------------------------------------------------------------------
def _run_grad(c, coef, gup, data=None):
    L_, _, stream = api()
    R, L = c["R"], c["L"]
    _, _, (xb, xs), (tb, ts) = data or X.time_data(c)
    Xb, Tb, Cf, G = Guarded.of(xb, "x", c["ox"]), Guarded.of(tb, "t", c["ot"]), Guarded.of(coef, "coef"), Guarded.of(gup, "gup")
    Y = Guarded(R * L, what="gx", off=c["og"])
    rc = L_.rfx_time_loss_grad(Xb.ptr(), Tb.ptr(), R, L, xs, ts, Cf.ptr(), *_h(_taps(c)), G.ptr(), RED[c["red"]], Y.ptr(), stream())
    sync(rc, "rfx_time_loss_grad", (R, L))
    for b in (Xb, Tb, Cf, G):
        b.unchanged()
    return {"gx": Y.np((R, L))}


@pytest.mark.parametrize("c", X.TIME_CASES, ids=X.case_id)
def test_time_loss_grad(c):
    """the adjoint of the zero-padded filter applied to a x~ + b t~ + c per sample, given the coefficients (the reference's, of the
    case's kind, as fp64 bits) and gup: the scalar head and tail, the 16-byte body, both halos from memory and from the shuffle, rows at
    different phases, x / t / gx bases 0 ... 3 floats off"""
    data = X.time_data(c)
    x, t = data[0], data[1]
    sums, _ = X.row_sums(x, t, _taps(c))
    coef = X.time_loss_rows(sums, c["L"], c["kind"], c["zm"] if c["L"] > 1 else 0, 1e-8, "none")["coef"]
    gup = X.gup_of(c)
    a, _ = twice(lambda: _run_grad(c, coef, gup, data))
    ref, bound = X.time_loss_grad(x, t, coef, _taps(c), gup, c["red"])
    report("LOSS", "grad " + X.case_id(c), [("gx", _judge(a["gx"], ref, bound, ctx=("rfx_time_loss_grad", "gx", *sorted(X.forms_time_grad(c)))))])


CHAIN = X.TIME_CASES[10]


@pytest.mark.parametrize("kind", X.KINDS[:5])
def test_time_chain(kind):
    """sums, then rows, then the gradient, each from the device's own buffer of the stage before, judged by the composed bound: the sums'
    bound carried through the rows (every sum an uncertain input of its own), the coefficients' bound through the gradient"""
    c = dict(CHAIN, kind=kind)
    data = X.time_data(c)
    x, t = data[0], data[1]
    s = _run_sums(c, "rfx_time_sums", data)["sums"]
    sref, sb = X.row_sums(x, t, _taps(c))
    _judge(s, sref, sb, ctx=("chain", "sums", kind))
    r = _run_rows(s, c["L"], kind, c["zm"], c["red"])
    ref = X.time_loss_rows(sref, c["L"], kind, c["zm"], 1e-8, c["red"], sums_err=sb)
    ratios = [(k, _judge(r[k], ref[k], ref[k + "_bound"], ctx=("chain", k, kind))) for k in ("rows", "coef", "out")]
    gup = X.gup_of(c)
    g = _run_grad(c, r["coef"], gup, data)["gx"]
    gref, gb = X.time_loss_grad(x, t, ref["coef"], _taps(c), gup, c["red"], coef_err=ref["coef_bound"])
    ratios.append(("gx", _judge(g, gref, gb, ctx=("chain", "gx", kind))))
    report("LOSS", "chain " + kind, ratios)


# ---- log-cosh ------------------------------------------------------------------------------------------------------------------------------
def _run_logcosh(c, x, t, gup):
    L_, _, stream = api()
    R, L = c["R"], c["L"]
    xs = L + c.get("xpad", 0)
    xb = np.full(R * xs, 1.0e30, np.float32)
    xb.reshape(R, xs)[:, :L] = x
    Xb, Tb, G = Guarded.of(xb, "x"), Guarded.of(t, "t"), Guarded.of(gup, "gup")
    n = int(L_.rfx_logcosh_ws(R, L))
    assert n == R * X.time_sums_grid(L)
    W, S, Y = Guarded(n, F64, "ws"), Guarded(R, F64, "sums"), Guarded(R * L, what="gx")
    sync(L_.rfx_logcosh_rows(Xb.ptr(), Tb.ptr(), R, L, xs, L, c["a"], 1e-8, W.ptr(), S.ptr(), stream()), "rfx_logcosh_rows", (R, L))
    sync(L_.rfx_logcosh_grad(Xb.ptr(), Tb.ptr(), R, L, xs, L, c["a"], 1e-8, G.ptr(), RED[c["red"]], Y.ptr(), stream()), "rfx_logcosh_grad", (R, L))
    for b in (Xb, Tb, G):
        b.unchanged()
    assert np.isfinite(W.np()).all()
    return {"sums": S.np((R, 1)), "gx": Y.np((R, L))}


@pytest.mark.parametrize("c", X.LOGCOSH_CASES, ids=lambda c: f"R{c['R']}-L{c['L']}-a{c['a']}")
def test_logcosh(c):
    """log(cosh(a z) + eps) / a summed per row and its gradient, a of 0.5, 1 and 50, |a z| up to 800 (no overflow), z = 0 (gradient
    exactly 0), negative z; then rfx_time_loss_rows(kind LOGCOSH) on the device's sums: rows = sums / L, coef zeros, the reduction"""
    x, t = X.logcosh_data(c)
    gup = (0.5 + np.arange(c["R"] if c["red"] == "none" else 1) % 5 * 0.25).astype(np.float32)
    a, _ = twice(lambda: _run_logcosh(c, x, t, gup))
    forms = sorted(X.forms_logcosh(c))
    ref, bound = X.logcosh_rows(x, t, c["a"])
    r1 = _judge(a["sums"], ref, bound, ctx=("rfx_logcosh_rows", "sums", *forms))
    gref, gb = X.logcosh_grad(x, t, c["a"], 1e-8, gup, c["red"])
    r2 = _judge(a["gx"], gref, gb, ctx=("rfx_logcosh_grad", "gx", *forms))
    rows = _run_rows(a["sums"], c["L"], "logcosh", 0, c["red"])
    rr = X.time_loss_rows(ref, c["L"], "logcosh", 0, 1e-8, c["red"], sums_err=bound)
    r3 = _judge(rows["rows"], rr["rows"], rr["rows_bound"], ctx=("rfx_time_loss_rows", "rows", *forms))
    assert np.array_equal(rows["coef"], np.zeros((c["R"], 3))), "coef of LOGCOSH is zeros"
    if c["red"] != "none":
        _judge(rows["out"], rr["out"], rr["out_bound"], ctx=("rfx_time_loss_rows", "out", *forms))
    report("LOSS", f"logcosh R{c['R']}-L{c['L']}", [("sums", r1), ("gx", r2), ("rows", r3)])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_time_refusals():
    """every -1 condition returns -1 with nothing written: NULL arguments, R / L <= 0, R = 65536 (one grid row per signal row), a bad
    kind or reduction, out == NULL with a reducing reduction, a <= 0 and NaN, pointers off 4-byte alignment"""
    L_, _, stream = api()
    R, L = 2, 8
    x, t = Guarded.of(np.ones(R * L, np.float32), "x"), Guarded.of(np.ones(R * L, np.float32), "t")
    ws, sums, coef = Guarded(5 * R, F64, "ws"), Guarded(5 * R, F64, "sums"), Guarded(3 * R, F64, "coef")
    rows, out, gx, gup = Guarded(R, what="rows"), Guarded(1, what="out"), Guarded(R * L, what="gx"), Guarded.of(np.ones(R, np.float32), "gup")
    sin, cin = Guarded.of(np.ones(5 * R), "sums in"), Guarded.of(np.ones(3 * R), "coef in")
    s = stream()
    P = lambda b: b.ptr()
    nan = float("nan")
    calls = []
    for Rr, Ll in ((0, L), (-1, L), (R, 0), (65536, L)):
        calls += [("sisdr_sums", lambda Rr=Rr, Ll=Ll: L_.rfx_sisdr_sums(P(x), P(t), Rr, Ll, L, L, P(ws), P(sums), s)),
                  ("time_sums", lambda Rr=Rr, Ll=Ll: L_.rfx_time_sums(P(x), P(t), Rr, Ll, L, L, 1, 0.3, 1.0, -0.5, P(ws), P(sums), s)),
                  ("time_loss_grad", lambda Rr=Rr, Ll=Ll: L_.rfx_time_loss_grad(P(x), P(t), Rr, Ll, L, L, P(cin), 0, 0.0, 1.0, 0.0, P(gup), 0, P(gx), s)),
                  ("logcosh_rows", lambda Rr=Rr, Ll=Ll: L_.rfx_logcosh_rows(P(x), P(t), Rr, Ll, L, L, 1.0, 1e-8, P(ws), P(sums), s)),
                  ("logcosh_grad", lambda Rr=Rr, Ll=Ll: L_.rfx_logcosh_grad(P(x), P(t), Rr, Ll, L, L, 1.0, 1e-8, P(gup), 0, P(gx), s))]
        if Rr != 65536:
            calls += [("time_loss_rows", lambda Rr=Rr, Ll=Ll: L_.rfx_time_loss_rows(P(sin), Rr, Ll, 0, 1, 1e-8, 0, P(rows), P(coef), P(out), s)),
                      ("sisdr_finish", lambda Rr=Rr, Ll=Ll: L_.rfx_sisdr_finish(P(sin), Rr, Ll, 1, 1e-8, P(out), s))]
    for k in range(4):
        a = [P(x), P(t), P(ws), P(sums)]
        a[k] = None
        calls += [("sisdr_sums NULL", lambda a=a: L_.rfx_sisdr_sums(a[0], a[1], R, L, L, L, a[2], a[3], s)),
                  ("time_sums NULL", lambda a=a: L_.rfx_time_sums(a[0], a[1], R, L, L, L, 0, 0.0, 1.0, 0.0, a[2], a[3], s)),
                  ("logcosh_rows NULL", lambda a=a: L_.rfx_logcosh_rows(a[0], a[1], R, L, L, L, 1.0, 1e-8, a[2], a[3], s))]
    for k in range(5):
        a = [P(x), P(t), P(cin), P(gup), P(gx)]
        a[k] = None
        calls.append(("time_loss_grad NULL", lambda a=a: L_.rfx_time_loss_grad(a[0], a[1], R, L, L, L, a[2], 0, 0.0, 1.0, 0.0, a[3], 0, a[4], s)))
        if k != 2:
            calls.append(("logcosh_grad NULL", lambda a=a: L_.rfx_logcosh_grad(a[0], a[1], R, L, L, L, 1.0, 1e-8, a[3], 0, a[4], s)))
    for k in range(3):                                                             # one byte / two bytes off: not a float pointer
        a = [x.t.data_ptr(), t.t.data_ptr(), gx.t.data_ptr()]
        a[k] += 1 + k % 2
        calls.append(("time_loss_grad misaligned", lambda a=a: L_.rfx_time_loss_grad(C.c_void_p(a[0]), C.c_void_p(a[1]), R, L - 1, L, L, P(cin), 1, 0.3,
                                                                                       1.0, -0.5, P(gup), 0, C.c_void_p(a[2]), s)))
    for kind, red in ((-1, 0), (6, 0), (0, -1), (0, 3)):
        calls.append(("time_loss_rows kind / reduction", lambda kind=kind, red=red: L_.rfx_time_loss_rows(P(sin), R, L, kind, 1, 1e-8, red, P(rows), P(coef),
                                                                                                          P(out), s)))
    for red in (-1, 3):
        calls += [("time_loss_grad reduction", lambda red=red: L_.rfx_time_loss_grad(P(x), P(t), R, L, L, L, P(cin), 0, 0.0, 1.0, 0.0, P(gup), red, P(gx), s)),
                  ("logcosh_grad reduction", lambda red=red: L_.rfx_logcosh_grad(P(x), P(t), R, L, L, L, 1.0, 1e-8, P(gup), red, P(gx), s))]
    calls += [("time_loss_rows out NULL", lambda red=red: L_.rfx_time_loss_rows(P(sin), R, L, 0, 1, 1e-8, red, P(rows), P(coef), None, s)) for red in (0, 1)]
    calls += [("time_loss_rows NULL", lambda: L_.rfx_time_loss_rows(None, R, L, 0, 1, 1e-8, 0, P(rows), P(coef), P(out), s)),
              ("time_loss_rows NULL", lambda: L_.rfx_time_loss_rows(P(sin), R, L, 0, 1, 1e-8, 0, None, P(coef), P(out), s)),
              ("sisdr_finish NULL", lambda: L_.rfx_sisdr_finish(None, R, L, 1, 1e-8, P(out), s)),
              ("sisdr_finish NULL", lambda: L_.rfx_sisdr_finish(P(sin), R, L, 1, 1e-8, None, s))]
    for a in (0.0, -1.0, nan):
        calls += [("logcosh_rows a", lambda a=a: L_.rfx_logcosh_rows(P(x), P(t), R, L, L, L, a, 1e-8, P(ws), P(sums), s)),
                  ("logcosh_grad a", lambda a=a: L_.rfx_logcosh_grad(P(x), P(t), R, L, L, L, a, 1e-8, P(gup), 0, P(gx), s))]
    for name, call in calls:
        assert call() == -1, name
    torch.cuda.synchronize()
    assert L_.rfx_time_sums_ws(0, L) == 0 and L_.rfx_time_sums_ws(R, 0) == 0 and L_.rfx_logcosh_ws(0, L) == 0 and L_.rfx_logcosh_ws(R, 0) == 0
    for b in (ws, sums, coef, rows, out, gx):
        b.untouched()
    for b in (x, t, gup, sin, cin):
        b.unchanged()
    print(f"\nLOSS time refusals: {len(calls)} calls returned -1 with nothing written")


def test_stft_loss_row_limit():
    """the three STFT-loss cell wrappers (their values are pinned by test_gpu_fft_kernel.py) refuse R = 65536 too, with nothing written"""
    L_, _, stream = api()
    s = stream()
    x, m, sums = Guarded.of(np.ones(16, np.float32), "spectrum"), Guarded.of(np.ones(8, np.float32), "ymag"), Guarded.of(np.ones(3, np.float32), "sums in")
    W, S, G = Guarded(3, F64, "ws"), Guarded(3, what="sums"), Guarded(16, what="gxc")
    eps = float(X.EPS_F)
    assert L_.rfx_stft_loss_reduce(x.ptr(), x.ptr(), 65536, 8, eps, W.ptr(), S.ptr(), s) == -1
    assert L_.rfx_stft_loss_grad(x.ptr(), x.ptr(), 65536, 8, eps, sums.ptr(), 1.0, 1.0, None, G.ptr(), s) == -1
    assert L_.rfx_stft_loss_grad_m(x.ptr(), m.ptr(), 65536, 8, eps, sums.ptr(), 1.0, 1.0, None, G.ptr(), s) == -1
    torch.cuda.synchronize()
    W.untouched(), S.untouched(), G.untouched()
    x.unchanged(), m.unchanged(), sums.unchanged()


# ---- combines ------------------------------------------------------------------------------------------------------------------------------
def _run_combine(sums, n, R, pe, w=None):
    L_, _, stream = api()
    bufs = [Guarded.of(s, f"sums[{k}]") for k, s in enumerate(sums)]
    O = Guarded(1, what="out")
    ptrs = (C.c_void_p * len(bufs))(*[b.t.data_ptr() for b in bufs])
    nn = (C.c_int64 * len(n))(*n)
    if w is None:
        rc = L_.rfx_mrstft_combine(ptrs, nn, len(bufs), R, pe, O.ptr(), stream())
    else:
        rc = L_.rfx_mrstft_combine_w(ptrs, nn, len(bufs), R, pe, w[0], w[1], w[2], O.ptr(), stream())
    sync(rc, "rfx_mrstft_combine" + ("_w" if w else ""), (len(bufs), R))
    for b in bufs:
        b.unchanged()
    return {"out": O.np()}


@pytest.mark.parametrize("c", X.COMBINE_CASES, ids=lambda c: f"nres{c['nres']}-R{c['R']}-pe{c['pe']}")
def test_combines(c):
    """both scalar tails: nres 1, 3, 8; R 1, 64, 65, 130; per example and over the batch; the three weight sets; a weight of 0 leaves
    its term out even when its sums are NaN"""
    ratios = []
    s3, n = X.combine_data(c, 3)
    s3 = [s.astype(np.float32) for s in s3]
    a, _ = twice(lambda: _run_combine(s3, n, c["R"], c["pe"]))
    ref, bound = X.mrstft_combine(s3, n, c["pe"])
    ratios.append(("combine", _judge(a["out"], ref, bound, ctx=("rfx_mrstft_combine", "out", *sorted(X.forms_combine(c))))))
    s4, n = X.combine_data(c, 4)
    for w in X.COMBINE_WEIGHTS:
        a, _ = twice(lambda: _run_combine(s4, n, c["R"], c["pe"], w))
        ref, bound = X.mrstft_combine_w(s4, n, c["pe"], w)
        ratios.append((f"w{w}", _judge(a["out"], ref, bound, ctx=("rfx_mrstft_combine_w", "out", *sorted(X.forms_combine(c, w))))))
        poisoned = [s.copy() for s in s4]
        for s in poisoned:
            if w[0] == 0.0:
                s[:, :2] = np.nan
            if w[1] == 0.0:
                s[:, 2] = np.nan
            if w[2] == 0.0:
                s[:, 3] = np.nan
        b = _run_combine(poisoned, n, c["R"], c["pe"], w)
        assert np.array_equal(a["out"].view(np.uint8), b["out"].view(np.uint8)), ("a term with weight 0 was evaluated", w)
    report("LOSS", f"combines nres{c['nres']}-R{c['R']}", ratios)


def test_combine_refusals():
    """nres 0 and 9, R <= 0, n[k] <= 0, a NULL sums[k], NULL arguments: -1 and out untouched"""
    L_, _, stream = api()
    R = 3
    f32, f64 = Guarded.of(np.ones(3 * R, np.float32), "sums"), Guarded.of(np.ones(4 * R), "sums")
    O = Guarded(1, what="out")
    s = stream()
    count = 0
    for fn, buf, extra in ((L_.rfx_mrstft_combine, f32, ()), (L_.rfx_mrstft_combine_w, f64, (1.0, 1.0, 1.0))):
        ok = (C.c_void_p * 9)(*[buf.t.data_ptr()] * 9)
        hole = (C.c_void_p * 9)(*[buf.t.data_ptr()] * 9)
        hole[1] = None
        n = (C.c_int64 * 9)(*[10] * 9)
        n0 = (C.c_int64 * 9)(*[10, 0] + [10] * 7)
        nneg = (C.c_int64 * 9)(*[10, -5] + [10] * 7)
        for ptrs, nn, nres, Rr, out in ((ok, n, 0, R, O.ptr()), (ok, n, 9, R, O.ptr()), (ok, n, -1, R, O.ptr()), (ok, n, 2, 0, O.ptr()), (ok, n, 2, -1, O.ptr()),
                                        (ok, n0, 2, R, O.ptr()), (ok, nneg, 2, R, O.ptr()), (hole, n, 2, R, O.ptr()), (None, n, 2, R, O.ptr()),
                                        (ok, None, 2, R, O.ptr()), (ok, n, 2, R, None)):
            assert fn(ptrs, nn, nres, Rr, 1, *extra, out, s) == -1, (fn.__name__, nres, Rr)
            count += 1
    torch.cuda.synchronize()
    O.untouched(), f32.unchanged(), f64.unchanged()
    print(f"\nLOSS combine refusals: {count} calls returned -1 with nothing written")


# ---- the scaled family ---------------------------------------------------------------------------------------------------------------------
def _run_scaled(c, x, y, fb, mx_in=None, my_in=None, sums_in=None):
    """forward, and the gradient given mx_in / my_in / sums_in when the case stores"""
    L_, _, stream = api()
    R, frames, bins = c["R"], c["frames"], c["bins"]
    n_out = bins if fb is None else fb.shape[0]
    Xb, Yb = Guarded.of(x, "xc"), Guarded.of(y, "yc")
    ins = [Xb, Yb]
    idx = w = tidx = tw = None
    n_w = 0
    if fb is not None:
        i, wv = X.pack(fb)
        ti, twv = X.pack(fb.T)
        idx, w, tidx, tw = Guarded.of(i, "fb_idx"), Guarded.of(wv, "fb_w"), Guarded.of(ti, "fbt_idx"), Guarded.of(twv, "fbt_w")
        n_w = wv.size
        ins += [idx, w, tidx, tw]
    n = int(L_.rfx_stft_scaled_loss_ws(R, frames))
    assert n == 4 * R * X.scaled_grid(frames)
    W, S = Guarded(n, F64, "ws"), Guarded(4 * R, F64, "sums")
    MX, MY = Guarded(R * frames * n_out, what="mx"), Guarded(R * frames * n_out, what="my")
    p = lambda b: b.ptr() if b is not None else None
    rc = L_.rfx_stft_scaled_loss(Xb.ptr(), Yb.ptr(), R, frames, bins, p(idx), p(w), n_out, n_w, float(X.EPS_F), W.ptr(), S.ptr(),
                                 MX.ptr() if c["store"] else None, MY.ptr() if c["store"] else None, stream())
    sync(rc, "rfx_stft_scaled_loss", (R, frames, bins, n_out))
    ws = W.np()
    out = {"sums": S.np((R, 4))}
    assert np.isfinite(np.delete(ws.reshape(-1, 4), 2, 1)).all(), "a slot of the workspace was not written"
    if c["store"]:
        out["mx"], out["my"] = MX.np((R, frames, n_out)), MY.np((R, frames, n_out))
    else:
        MX.untouched(), MY.untouched()
    if mx_in is not None:
        A, B, Sin = Guarded.of(mx_in, "mx in"), Guarded.of(my_in, "my in"), Guarded.of(sums_in, "sums in")
        U = Guarded.of(np.array([0.75], np.float32), "gup") if c["gup"] else None
        G = Guarded(x.size, what="gxc")
        wsc, wlm, wlin = c["w"]
        rc = L_.rfx_stft_scaled_loss_grad(Xb.ptr(), A.ptr(), B.ptr(), R, frames, bins, p(tidx), p(tw), n_out, float(X.EPS_F), Sin.ptr(), c["pe"],
                                          wsc, wlm, wlin, p(U), G.ptr(), stream())
        sync(rc, "rfx_stft_scaled_loss_grad", (R, frames, bins, n_out))
        ins += [A, B, Sin] + ([U] if U is not None else [])
        out["gxc"] = G.np(x.shape)
    for b in ins:
        b.unchanged()
    return out


@pytest.mark.parametrize("c", X.SCALED_CASES, ids=X.scaled_id)
def test_scaled(c):
    """forward: the four row sums and Mx, My against the dense filter-bank product in fp64, the fp32 arithmetic counted (loss_ref).
    gradient: given the reference's mx, my (rounded to fp32) and sums (fp64) as inputs, so sign(Mx - My) and px > eps are exact on what
    the kernel reads; cells with px just below, at and just above eps"""
    fb = X.bank_of(c, _mel)
    x, y = X.scaled_data(c)
    n_out = c["bins"] if fb is None else fb.shape[0]
    f = X.stft_scaled_loss(x, y, fb, adds=X.scaled_adds(c, n_out))
    mx_in, my_in = f["mx"].astype(np.float32), f["my"].astype(np.float32)
    args = (mx_in, my_in, f["sums"]) if c["store"] else ()
    a, _ = twice(lambda: _run_scaled(c, x, y, fb, *args))
    forms = sorted(X.forms_scaled(c, fb))
    ratios = [("sums", _judge(a["sums"], f["sums"], f["sums_bound"], ctx=("rfx_stft_scaled_loss", "sums", *forms)))]
    if c["store"]:
        ratios += [(k, _judge(a[k], f[k], f[k + "_bound"], ctx=("rfx_stft_scaled_loss", k, *forms))) for k in ("mx", "my")]
        ref, bound = X.stft_scaled_loss_grad(x, mx_in, my_in, f["sums"], fb, c["w"], c["pe"], 0.75 if c["gup"] else None)
        ratios.append(("gxc", _judge(a["gxc"], ref, bound, ctx=("rfx_stft_scaled_loss_grad", "gxc", *forms))))
        assert not a["gxc"][0, 0, 0].any() and not a["gxc"][0, 0, 1].any() and a["gxc"][0, 0, 2].any() == ref[0, 0, 2].any(), "px below / at / above eps"
    report("LOSS", "scaled " + X.scaled_id(c), ratios)


def test_scaled_empty_band():
    """a filter with an empty band: the operation defines M = 0 and a non-finite log term.  The kernel's log sum is non-finite in the same
    way, the other three sums are within their bounds, and the gradient is finite and within its bound wherever the transposed band
    does not list that filter"""
    c = X.EMPTY_CASE
    fb = X.bank_of(c)
    assert (X.pack(fb)[0][:, 1] == 0).sum() == 1
    x, y = X.scaled_data(c)
    f = X.stft_scaled_loss(x, y, fb, adds=X.scaled_adds(c, fb.shape[0]))
    assert not np.isfinite(f["sums"][:, 2]).any()
    mx_in, my_in = f["mx"].astype(np.float32), f["my"].astype(np.float32)
    a, _ = twice(lambda: _run_scaled(c, x, y, fb, mx_in, my_in, f["sums"]))
    assert not np.isfinite(a["sums"][:, 2]).any()
    keep = [0, 1, 3]
    r = _judge(a["sums"][:, keep], f["sums"][:, keep], f["sums_bound"][:, keep], ctx=("rfx_stft_scaled_loss", "sums", "empty band"))
    for k in ("mx", "my"):
        _judge(a[k], f[k], f[k + "_bound"], ctx=("rfx_stft_scaled_loss", k, "empty band"))
    ref, bound = X.stft_scaled_loss_grad(x, mx_in, my_in, f["sums"], fb, c["w"], c["pe"], 0.75)
    fin = np.isfinite(ref)
    assert fin.any() and (~fin).any()
    assert np.isfinite(a["gxc"][fin]).all() and not np.isfinite(a["gxc"][~fin & (np.abs(x) > 0) & (X.px32(x) > X.EPS_F)[..., None]]).any()
    r2 = _judge(a["gxc"][fin], ref[fin], bound[fin], ctx=("rfx_stft_scaled_loss_grad", "gxc", "empty band"))
    report("LOSS", "scaled empty band", [("sums", r), ("gxc", r2)])


def test_scaled_lds_limits_and_refusals():
    """forward at exactly 65536 bytes of LDS (bins 8191, n_w 2: runs) and at 65540 (bins 8192, n_w 1: -1); the gradient's identity at
    n_out = bins = 16385 (65540 bytes: the raised dynamic-LDS limit, runs) and at n_out = 40961 (163844 bytes: -1); R = 65536, NULL
    arguments, mx without my, n_out != bins for the identity: -1 with nothing written"""
    L_, _, stream = api()
    s = stream()
    eps = float(X.EPS_F)
    c = X._s(1, 1, 8191, ("hand", 1, (2,)))
    fb = np.zeros((1, 8191), np.float32)
    fb[0, 8189:] = (0.5, 0.25)
    x, y = X.scaled_data(c)
    f = X.stft_scaled_loss(x, y, fb, adds=X.scaled_adds(c, 1))
    a, _ = twice(lambda: _run_scaled(c, x, y, fb))
    r = [(k, _judge(a[k], f[k], f[k + "_bound"], ctx=("rfx_stft_scaled_loss", k, "lds 65536"))) for k in ("sums", "mx", "my")]
    # 65540 bytes: refused
    big = Guarded.of(np.zeros(2 * 8192 * 2, np.float32), "spectra")
    idx, w = Guarded.of(np.array([[0, 1, 0]], np.int32), "idx"), Guarded.of(np.ones(1, np.float32), "w")
    W, S, MX, MY = Guarded(4, F64, "ws"), Guarded(4, F64, "sums"), Guarded(8, what="mx"), Guarded(8, what="my")
    P = lambda b: b.ptr()
    calls = [lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 8192, P(idx), P(w), 1, 1, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 65536, 1, 2, None, None, 2, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, None, None, 3, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, None, None, 2, 0, eps, P(W), P(S), P(MX), None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, P(idx), None, 1, 1, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, P(idx), P(w), 0, 1, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, P(idx), P(w), 1, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(None, P(big), 1, 1, 2, None, None, 2, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, None, None, 2, 0, eps, None, P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 2, None, None, 2, 0, eps, P(W), None, None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 0, 1, 2, None, None, 2, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 0, 2, None, None, 2, 0, eps, P(W), P(S), None, None, s),
             lambda: L_.rfx_stft_scaled_loss(P(big), P(big), 1, 1, 0, None, None, 0, 0, eps, P(W), P(S), None, None, s)]
    G, Sin = Guarded(8, what="gxc"), Guarded.of(np.ones(4), "sums in")
    calls += [lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 40961, None, None, 40961, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 65536, 1, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 2, None, None, 3, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 2, P(idx), None, 1, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(None, P(big), P(big), 1, 1, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), None, P(big), 1, 1, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), None, 1, 1, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 2, None, None, 2, eps, None, 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, None, s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 0, 2, None, None, 2, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s),
              lambda: L_.rfx_stft_scaled_loss_grad(P(big), P(big), P(big), 1, 1, 2, None, None, 0, eps, P(Sin), 1, 1.0, 1.0, 0.0, None, P(G), s)]
    for k, call in enumerate(calls):
        assert call() == -1, k
    torch.cuda.synchronize()
    assert L_.rfx_stft_scaled_loss_ws(0, 1) == 0 and L_.rfx_stft_scaled_loss_ws(1, 0) == 0
    for b in (W, S, MX, MY, G):
        b.untouched()
    for b in (big, idx, w, Sin):
        b.unchanged()
    # the gradient's identity with one frame of 16385 dM values: 65540 bytes of dynamic LDS
    cg = X._s(1, 1, 16385, None, w=(1.0, 1.0, 0.5), gup=0)
    x, y = X.scaled_data(cg)
    f = X.stft_scaled_loss(x, y, None, adds=X.scaled_adds(cg, 16385))
    mx_in, my_in = f["mx"].astype(np.float32), f["my"].astype(np.float32)
    a, _ = twice(lambda: _run_scaled(cg, x, y, None, mx_in, my_in, f["sums"]))
    ref, bound = X.stft_scaled_loss_grad(x, mx_in, my_in, f["sums"], None, cg["w"], 1, None)
    r.append(("gxc 16385", _judge(a["gxc"], ref, bound, ctx=("rfx_stft_scaled_loss_grad", "gxc", "dynamic lds attribute"))))
    report("LOSS", f"scaled lds limits ({len(calls)} refusals)", r)
