"""tests/loss_ref.py against what the repository already states about the training losses (tests/time_loss_ref.py,
tests/mrstft_scaled_ref.py, remfx_amd.losses.mel_filterbank / pack_banded), against itself (finite differences of its own loss for the
coefficients, its float32 restatement within its own bound, the margins of its decisions) and over its case tables (every form reached
or named, every case new or marked, the bounds small against the reference or the element named).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import loss_ref as X
from tests import mrstft_scaled_ref as M
from tests import time_loss_ref as T


def _mel(sr, n_fft, n_mels):
    from remfx_amd.losses import mel_filterbank
    return mel_filterbank(sr, n_fft, n_mels).numpy()


def _taps(c):
    return None if c["taps"] is None else X.TAPS[c["taps"]]


SMALL = [c for c in X.TIME_CASES if c["R"] * c["L"] <= 20000]


def test_longdouble_is_stated():
    """the reference says which long double it ran with; the bounds carry it either way"""
    assert X.LONGDOUBLE_BITS in (53, 64, 106, 113) and X.REF_U <= X.U64


@pytest.mark.parametrize("c", SMALL, ids=X.case_id)
def test_time_statements_against_torch_restatement(c):
    """sums, per-row losses, coefficients and the adjoint gradient against tests/time_loss_ref.py in fp64 on the same signals.  The
    restatement evaluates the sums form in fp64, so the two agree to its conditioning: 1e-6 relative here, where the exact rational
    reference and the fp64 formula differ by up to 1e-8 on the 80 and 120 dB rows."""
    x, t, _, _ = X.time_data(c)
    xt, tt = torch.from_numpy(x).double(), torch.from_numpy(t).double()
    s, b = X.row_sums(x, t, _taps(c))
    s2 = T.row_sums(xt, tt, _taps(c))
    assert np.all(np.abs(s - s2) <= b + 64 * X.U64 * np.abs(s) * np.sqrt(c["L"]) + 1e-300)
    for kind in X.KINDS[:5]:
        for zm in ((0,) if c["L"] == 1 else (0, 1)):
            r = X.time_loss_rows(s, c["L"], kind, zm, 1e-8, "mean")
            v2 = T.sums_form_value(kind, s, c["L"], zm)
            c2 = T.closed_form_coefficients(kind, s, c["L"], zm)
            assert np.allclose(r["rows"], v2, rtol=1e-6, atol=1e-12), (kind, zm)
            scale = np.abs(c2).max(-1, keepdims=True) + 1e-300
            assert np.all(np.abs(r["coef"] - c2) <= 1e-6 * scale), (kind, zm)
            lit = T.time_loss(kind, xt, tt, bool(zm), 1e-8, "none", _taps(c)).numpy()
            ok = np.isclose(r["rows"], lit, rtol=1e-5, atol=1e-9)
            assert ok.all() or all(c["sig"][i] in ("same", "gain", "db120", "db80") for i in np.nonzero(~ok)[0]), (kind, zm)
    co = X.time_loss_rows(s, c["L"], c["kind"], c["zm"], 1e-8, "none")["coef"]
    g, _ = X.time_loss_grad(x, t, co, _taps(c), np.ones(c["R"], np.float32), "none")
    g2 = T.adjoint_gradient(co, xt, tt, _taps(c)).numpy()
    size = np.abs(co).max(-1, keepdims=True) * 8 * max(float(np.abs(x).max()), float(np.abs(t).max()), 1.0)      # of the terms that cancel
    assert np.all(np.abs(g - g2) <= 1e-13 * size + 1e-300)


def _loss_of_sums(kind, s5, L, zm, eps):
    """the loss's argument as an exact rational of the five raw sums (log kinds: q with loss = -10 log10 q)"""
    sx, st, sxt, sxx, stt = s5
    e, Lf = Fraction(float(eps)), Fraction(int(L))
    if kind == "esr":
        return (stt - 2 * sxt + sxx) / (stt + e)
    if kind == "dc":
        return ((st - sx) / Lf) ** 2 / (stt / Lf + e)
    if zm:
        sxt, sxx, stt = sxt - sx * st / Lf, sxx - sx * sx / Lf, stt - st * st / Lf
    if kind == "snr":
        return stt / (sxx - 2 * sxt + stt + e) + e
    al = sxt / (stt + e)
    res = sxx - 2 * al * sxt + al * al * stt if kind == "sisdr" else sxx - 2 * sxt + stt
    return al * al * stt / (res + e) + e


@pytest.mark.parametrize("kind", X.KINDS[:5])
@pytest.mark.parametrize("zm", (0, 1))
def test_coef_is_the_derivative_of_the_reference_loss(kind, zm):
    """coef = (2 dl/dSxx, dl/dSxt, dl/dSx) by a central difference of the reference's OWN loss in the raw sums, the difference of the
    two logarithms taken as log1p of the exact rational (q+ - q-) / q-; steps of 1e-5 of the residual energy: 1e-7 relative"""
    c = X.TIME_CASES[10]
    x, t, _, _ = X.time_data(c)
    s, _ = X.row_sums(x, t, _taps(c))
    L = c["L"]
    co = X.time_loss_rows(s, L, kind, zm, 1e-8, "none")["coef"]
    for r in range(s.shape[0]):
        s5 = [Fraction(float(v)) for v in s[r]]
        res = float(s5[3] - 2 * s5[2] + s5[4])
        for j, (col, mul) in enumerate(((3, 2.0), (2, 1.0), (0, 1.0))):
            h = Fraction(1e-5 * max(res, 1e-8) * (1.0 if col else np.sqrt(L)))
            up, dn = list(s5), list(s5)
            up[col] += h
            dn[col] -= h
            qp, qm = (_loss_of_sums(kind, v, L, zm, 1e-8) for v in (up, dn))
            if kind in ("esr", "dc"):
                fd = float((qp - qm) / (2 * h))
            else:
                fd = -10.0 / np.log(10.0) * np.log1p(float((qp - qm) / qm)) / float(2 * h)
            ref = co[r, j]
            assert abs(mul * fd - ref) <= 1e-7 * max(abs(ref), np.abs(co[r]).max() * 1e-9), (kind, zm, r, j, mul * fd, ref)


def _ratio(ref, bound):
    with np.errstate(all="ignore"):
        return np.where(bound == 0, 0.0, bound / np.abs(ref))


@pytest.mark.parametrize("c", X.TIME_CASES, ids=X.case_id)
def test_time_bounds_stay_meaningful(c):
    """bound / |reference| < 1e-3 for every element of every output, or the element is named in ILL_CONDITIONED (signal of its row,
    kind, output); named elements are at most 2 % of a case's output and never a whole case"""
    x, t, _, _ = X.time_data(c)
    s, b = X.row_sums(x, t, _taps(c))
    named = 0

    def check(ref, bound, kind, output, per_row=True):
        nonlocal named
        bad = ~(_ratio(ref, bound) < 1e-3)
        if not bad.any():
            return
        rows = np.nonzero(bad.reshape(c["R"], -1).any(1))[0] if per_row else [0]
        for r in rows:
            assert (c["sig"][r], kind, output) in X.ILL_CONDITIONED, (X.case_id(c), c["sig"][r], kind, output, int(r))
        named += int(bad.sum())
        assert bad.sum() <= 0.02 * bad.size and not bad.all(), (X.case_id(c), kind, output, int(bad.sum()), bad.size)

    check(s, b, "-", "sums")
    for kind in X.KINDS[:5]:
        for zm in ((0,) if c["L"] == 1 else (0, 1)):
            r = X.time_loss_rows(s, c["L"], kind, zm, 1e-8, "mean")
            check(r["rows"], r["rows_bound"], kind, "rows")
            for j, n in enumerate("abc"):
                check(r["coef"][:, j], r["coef_bound"][:, j], kind, "coef_" + n)
            assert _ratio(r["out"], r["out_bound"])[0] < 1e-3
    if c["R"] * c["L"] <= 300000:
        co = X.time_loss_rows(s, c["L"], c["kind"], c["zm"] if c["L"] > 1 else 0, 1e-8, "none")["coef"]
        g, gb = X.time_loss_grad(x, t, co, _taps(c), X.gup_of(c), c["red"])
        check(g, gb, c["kind"], "gx")


def test_residual_stays_positive_in_audio_range():
    """finding 1 of DESIGN.md 4.24: x == t at full scale and the bench's longest clip (262144 samples): the value's bound stays below
    0.25 dB and the bound of res + eps reaches eps only at 31 times that energy, for all three logarithmic kinds, centred or not, with
    none, half and all of the energy in the mean: no NaN, no clamp needed"""
    L = 262144
    t = np.where(np.random.default_rng(0).standard_normal((1, L)) >= 0, 1.0, -1.0).astype(np.float32)
    s, b = X.row_sums(t, t, None)
    for kind in ("sisdr", "sdsdr", "snr"):
        for zm in (0, 1):
            r = X.time_loss_rows(s, L, kind, zm, 1e-8, "mean")
            assert np.isfinite(r["rows"]).all() and r["rows_bound"][0] < 0.25, (kind, zm, r["rows"], r["rows_bound"])      # dB, of -134 dB
    lim = X.residual_limit(1e-8)
    print(f"\nres + eps can turn non-positive from Sxx + Stt = {lim:.4e} (eps = 1e-8): {lim / (2 * L):.1f} times full scale at {L} samples")
    assert lim > 10 * 2 * L
    for S in (2.0 * L, lim):                                                   # every kind, centring and row contributes a finite bound
        b = X.residual_bound(S, 1e-8)
        assert set(b) == {(k, z) for k in ("sisdr", "sdsdr", "snr") for z in (0, 1)}
        assert all(e.shape == (len(X.RESIDUAL_ROWS),) and np.isfinite(e).all() and (e > 0).all() and (e <= 1e-8 * (1 + 1e-9)).all() for e in b.values()), b
    assert max(float(e.max()) for e in X.residual_bound(2.0 * lim, 1e-8).values()) > 1e-8
    assert abs(1e-8 / lim - 6.11e-16) < 0.01e-16                               # the constant DESIGN 4.24 and the header state


@pytest.mark.parametrize("c", [c for c in X.LOGCOSH_CASES if c["R"] * c["L"] <= 20000], ids=lambda c: f"R{c['R']}-L{c['L']}-a{c['a']}")
def test_logcosh_statement(c):
    """against torch's log(cosh) in fp64 where cosh does not overflow; bound small against the reference; z = 0 exact"""
    x, t = X.logcosh_data(c)
    s, b = X.logcosh_rows(x, t, c["a"])
    assert np.all(b < 1e-6 * np.abs(s))
    z = c["a"] * (x.astype(np.float64) - t.astype(np.float64))
    if np.abs(z).max() < 700:
        lit = (np.log(np.cosh(z) + 1e-8) / c["a"]).sum(-1)
        assert np.allclose(s[:, 0], lit, rtol=1e-12)
    g, gb = X.logcosh_grad(x, t, c["a"], 1e-8, np.ones(1, np.float32), "sum")
    assert np.isfinite(g).all() and np.all(g[:, 0] == 0) and np.all(gb[:, 0] == 0)
    assert np.all(np.abs(g) <= 1.0 / c["L"] + 1e-12)
    lim = np.tanh(z) / c["L"]
    assert np.allclose(g, lim, rtol=1e-6, atol=1e-9 / c["L"])                 # eps = 1e-8 moves sinh / (cosh + eps) by 1e-8 at the most
    nz = g != 0
    assert np.all(gb[nz] < 1e-3 * np.abs(g[nz]))


@pytest.mark.parametrize("c", X.SCALED_CASES + [X.EMPTY_CASE], ids=X.scaled_id)
def test_pack_reproduces_dense_and_module_pack(c):
    """the band tables reproduce the dense matrix, loss_ref.pack is remfx_amd.losses.pack_banded, for fb and fb^T"""
    from remfx_amd.losses import pack_banded
    fb = X.bank_of(c, _mel)
    if fb is None:
        return
    for d in (fb, fb.T):
        idx, w = X.pack(d)
        i2, w2 = pack_banded(d)
        assert np.array_equal(idx, i2.numpy()) and np.array_equal(w, w2.numpy())
        assert np.array_equal(X.unpack(idx, w, d.shape[1]), d) and np.array_equal(M.unpack_banded(idx, w, d.shape[1]), d)
    if c["bank"][0] == "mel":
        assert np.abs(fb - M.librosa_mel(X.SR, c["bank"][1], c["bank"][2])).max() <= 2 * X.H32 * fb.max()
        assert (X.pack(fb)[0][:, 1] > 0).all()


@pytest.mark.parametrize("c", [c for c in X.SCALED_CASES if c["frames"] * c["bins"] <= 1100], ids=X.scaled_id)
def test_scaled_statement_against_torch_restatement(c):
    """the four terms of tests/mrstft_scaled_ref.py's stft_loss from dense torch matmuls in fp64, and the gradient by autograd"""
    fb = X.bank_of(c, _mel)
    x, y = X.scaled_data(c)
    f = X.stft_scaled_loss(x, y, fb)
    xm = torch.sqrt(torch.clamp(torch.from_numpy(x).double().pow(2).sum(-1), min=float(X.EPS_F)))
    ym = torch.sqrt(torch.clamp(torch.from_numpy(y).double().pow(2).sum(-1), min=float(X.EPS_F)))
    if fb is not None:
        F = torch.from_numpy(fb).double()
        xm, ym = xm @ F.T, ym @ F.T
    lit = torch.stack([(ym - xm).pow(2).sum((1, 2)), ym.pow(2).sum((1, 2)), (xm.log() - ym.log()).abs().sum((1, 2)), (xm - ym).abs().sum((1, 2))], -1)
    assert np.allclose(f["sums"], lit.numpy(), rtol=1e-12)
    # gradient: autograd of w_sc sc + w_lm sum|log| + w_lin sum|lin| with the kernel's weight convention, given the exact mx / my / sums
    X_t = torch.from_numpy(x).double().requires_grad_(True)
    p = X_t.pow(2).sum(-1)
    xm = torch.sqrt(torch.clamp(p, min=float(X.EPS_F)))
    xm = xm @ torch.from_numpy(fb).double().T if fb is not None else xm
    ymd = ym.detach()
    A, B = (ymd - xm).pow(2).sum((1, 2)), ymd.pow(2).sum((1, 2))
    w = [float(np.float32(v)) for v in c["w"]]
    sc = (A.sqrt() / B.sqrt()).sum() if c["pe"] else A.sum().sqrt() / B.sum().sqrt()
    (w[0] * sc + w[1] * (xm.log() - ymd.log()).abs().sum() + w[2] * (xm - ymd).abs().sum()).backward()
    mx32, my32 = f["mx"].astype(np.float32), f["my"].astype(np.float32)
    g, gb = X.stft_scaled_loss_grad(x, mx32, my32, f["sums"], fb, c["w"], c["pe"], None)
    at = X.px32(x) == X.EPS_F                                              # autograd's clamp passes a gradient AT eps, the kernel none
    lit_g = X_t.grad.numpy()
    if c["pe"]:                                                             # autograd's sqrt at A = 0 is NaN; the kernel defines ksc = 0
        same = f["sums"][:, 0] == 0
        assert np.isnan(lit_g[same]).all() and np.isfinite(g[same]).all()
        lit_g[same] = g[same]
    ok = np.isclose(g, lit_g, rtol=2e-5, atol=2e-6 * np.abs(lit_g).max()) | at[..., None] | (np.abs(X.margins(x)) < 4)[..., None]
    assert ok.all(), (np.argwhere(~ok)[:4], g[~ok][:4], lit_g[~ok][:4])


@pytest.mark.parametrize("c", X.SCALED_CASES + [X.EMPTY_CASE], ids=X.scaled_id)
def test_margins(c):
    """no cell's power is within one fp32 rounding of eps, other than the three placed just below, at and just above it"""
    x, _ = X.scaled_data(c)
    m = X.margins(x)
    placed = np.zeros(m.shape, bool)
    for cell in X.placed_cells(c):
        placed[cell] = True
    assert (m[~placed] > 2.0).all(), float(m[~placed].min())
    p = X.px32(x)
    assert p[0, 0, 0] < X.EPS_F and p[0, 0, 1] == X.EPS_F and p[0, 0, 2] > X.EPS_F and p[0, 0, 2] == np.nextafter(X.EPS_F, np.float32(1))
    assert p[0, 0, 0] == np.nextafter(X.EPS_F, np.float32(0))


def test_restate_scaled_within_bound_and_logf_floor():
    """the float32 restatement of the mel forward lies within the counted bound of the fp64 statement in every case; the K rule's floor for
    logf: the largest |restated log term - fp64 log term of the same float32 Mx, My| / (eps32 (|log Mx| + |log My|)), rounded up to the
    next half, is FLOOR['logf']"""
    worst, floor = 0.0, 0.0
    for c in X.SCALED_CASES + [X._s(1, 1, 8191, ("hand", 1, (2,)))]:
        fb = X.bank_of(c, _mel)
        x, y = X.scaled_data(c)
        x, y = x[:, :4], y[:, :4]                                              # every case; of the long ones the first four frames
        f = X.stft_scaled_loss(x, y, fb)
        a, cc, lt = X.restate_scaled(x, y, fb)
        for got, k in ((a, "mx"), (cc, "my")):
            r = np.abs(got.astype(np.float64) - f[k]) / f[k + "_bound"]
            assert r.max() <= 1.0, (X.scaled_id(c), k, float(r.max()))
            worst = max(worst, float(r.max()))
        a64, c64 = a.astype(np.float64), cc.astype(np.float64)
        G = np.abs(np.log(a64)) + np.abs(np.log(c64))
        floor = max(floor, float((np.abs(lt.astype(np.float64) - np.abs(np.log(a64) - np.log(c64))) / (X.EPS32 * G)).max()))
    print(f"\nrestate_scaled: largest error / bound {worst:.3f}; logf floor measured {floor:.3f}")
    assert np.ceil(2 * floor) / 2 <= X.FLOOR["logf"] and X.K_LOGF == 8 * X.FLOOR["logf"] + 8


def test_every_bound_is_finite():
    """an infinite or NaN bound would let any value pass: every bound of every case is finite (the empty band's log sum and the bins that
    gather from the empty filter are the stated exception, and the GPU test masks them)"""
    for c in X.TIME_CASES:
        if c["R"] * c["L"] > 300000:
            continue
        x, t, _, _ = X.time_data(c)
        s, b = X.row_sums(x, t, _taps(c))
        assert np.isfinite(b).all()
        for kind in X.KINDS[:5]:
            for zm in ((0,) if c["L"] == 1 else (0, 1)):
                r = X.time_loss_rows(s, c["L"], kind, zm, 1e-8, "mean", sums_err=b)
                assert all(np.isfinite(r[k]).all() for k in ("rows_bound", "coef_bound", "out_bound")), (X.case_id(c), kind, zm)
    for c in X.LOGCOSH_CASES:
        if c["R"] * c["L"] > 300000:
            continue
        x, t = X.logcosh_data(c)
        assert np.isfinite(X.logcosh_rows(x, t, c["a"])[1]).all() and np.isfinite(X.logcosh_grad(x, t, c["a"], 1e-8, np.ones(1, np.float32), "mean")[1]).all()
    for c in X.SCALED_CASES:
        fb = X.bank_of(c, _mel)
        x, y = X.scaled_data(c)
        f = X.stft_scaled_loss(x, y, fb)
        assert all(np.isfinite(f[k]).all() for k in ("sums_bound", "mx_bound", "my_bound")), X.scaled_id(c)
        gb = X.stft_scaled_loss_grad(x, f["mx"].astype(np.float32), f["my"].astype(np.float32), f["sums"], fb, c["w"], c["pe"], 0.75)[1]
        assert np.isfinite(gb).all(), X.scaled_id(c)
    for c in X.COMBINE_CASES:
        assert np.isfinite(X.mrstft_combine([s.astype(np.float32) for s in X.combine_data(c, 3)[0]], X.combine_data(c, 3)[1], c["pe"])[1]).all()
        for w in X.COMBINE_WEIGHTS:
            assert np.isfinite(X.mrstft_combine_w(*X.combine_data(c, 4), c["pe"], w)[1]).all()


def _all_case_forms():
    out = []
    for c in X.TIME_CASES:
        f = X.forms_sisdr_sums(c) | X.forms_time_sums(c) | X.forms_time_grad(c) | X.forms_finish(1, c["R"]) | X.forms_finish(0, c["R"])
        for kind in X.KINDS[:5]:
            for red in X.REDUCTIONS:
                f |= X.forms_rows(kind, 0, red, c["R"]) | X.forms_rows(kind, 1, red, c["R"])
        out.append(("time " + X.case_id(c), c, f))
    for c in X.LOGCOSH_CASES:
        out.append((f"logcosh R{c['R']}-L{c['L']}", c, X.forms_logcosh(c) | X.forms_rows("logcosh", 0, c["red"], c["R"], coef=False)))
    for c in X.SCALED_CASES:
        out.append(("scaled " + X.scaled_id(c), c, X.forms_scaled(c, X.bank_of(c, _mel))))
    out.append(("scaled empty band", X.EMPTY_CASE, X.forms_scaled(X.EMPTY_CASE, X.bank_of(X.EMPTY_CASE))))
    for c in X.COMBINE_CASES:
        f = X.forms_combine(c)
        for w in X.COMBINE_WEIGHTS:
            f |= X.forms_combine(c, w)
        out.append((f"combine nres{c['nres']}-R{c['R']}", c, f))
    out.append(("lds limits", {}, set(X.LDS_FORMS)))
    return out


def test_every_form_reached_or_named():
    reached = set().union(*[f for _, _, f in _all_case_forms()])
    missing = set(X.ALL_FORMS) - reached - set(X.UNREACHED)
    assert not missing, sorted(missing)
    assert not (reached - set(X.ALL_FORMS)), sorted(reached - set(X.ALL_FORMS))
    assert not (set(X.UNREACHED) & reached), sorted(set(X.UNREACHED) & reached)
    assert all(X.UNREACHED.values())


def test_every_case_reaches_a_new_form_or_is_a_value_case():
    seen = set()
    for name, c, f in _all_case_forms():
        assert (f - seen) or c.get("value"), name
        assert not ((f - seen) and c.get("value")), (name, "marked as a value case but reaches", sorted(f - seen))
        seen |= f


def test_slot_sum_forms_are_named():
    """rfx_slot_sum_kernel<double> is reached only through the entry points above: which case hits which of its forms"""
    hit = {}
    for name, c, f in _all_case_forms():
        for form in f:
            if form.startswith("slot_sum<double>"):
                hit.setdefault(form, name)
    assert set(hit) == {f for f in X.ALL_FORMS if f.startswith("slot_sum<double>")}, sorted(hit)
    assert hit == X.SLOT_SUM_CASES, hit


def test_combines_against_torch_restatement_tail():
    """out = mean_k (w_sc sc_k + w_lm lm_k + w_lin lin_k) written once more in fp64; a zero weight leaves a NaN sum out"""
    c = X.COMBINE_CASES[2]
    sums, n = X.combine_data(c, 4)
    for w in X.COMBINE_WEIGHTS:
        ref, b = X.mrstft_combine_w(sums, n, c["pe"], w)
        lit = np.mean([w[0] * np.mean(np.sqrt(s[:, 0] / s[:, 1])) + w[1] * s[:, 2].sum() / (c["R"] * k) + w[2] * s[:, 3].sum() / (c["R"] * k)
                       for s, k in zip(sums, n)])
        assert abs(ref[0] - lit) < 1e-12 * abs(lit) and b[0] < 1e-6 * abs(ref[0])
    poisoned = [s.copy() for s in sums]
    for s in poisoned:
        s[:, 2] = np.nan
    assert np.isfinite(X.mrstft_combine_w(poisoned, n, c["pe"], (0.5, 0.0, 2.0))[0]).all()
    s3, n3 = X.combine_data(c, 3)
    s3 = [s.astype(np.float32) for s in s3]
    ref, b = X.mrstft_combine(s3, n3, 1)
    lit = np.mean([np.mean(np.sqrt(s[:, 0].astype(np.float64) / s[:, 1])) + s[:, 2].astype(np.float64).sum() / (c["R"] * k) for s, k in zip(s3, n3)])
    assert abs(ref[0] - lit) < 1e-12 * abs(lit) and b[0] < 1e-6 * abs(ref[0])
