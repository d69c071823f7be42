"""rfx_fft_analysis, rfx_fft_synthesis, rfx_fft_synthesis_lossgrad and rfx_stft_pair_loss (remfx_amd/csrc/fft.hip, csrc/fft_any.hip) and
the three cell kernels on their spectra, rfx_stft_loss_reduce / _grad / _grad_m (csrc/losses.hip), through the C ABI on buffers this
test allocates, against tests/fft_ref.py (fp64), per element.  The bounds and where their constants come from are in fft_ref's
docstring and DESIGN.md 4.22; none is measured on a kernel.  The library reads RFX_FFT_OWN, RFX_FFT_OWN_FW,
RFX_FFT_SYN_NB and RFX_FFT_ANA_NB once per process: the tests run at the defaults, which fft_ref.forms_*() mirror.

Buffers: every input and output sits between NaN guards of 4096 elements, outputs are NaN-filled (except out0 under accum), workspaces
are exactly rfx_fft_synthesis_ws / rfx_stft_pair_loss_ws in size and NaN-filled ("no initialisation needed" is part of the contract);
inputs have to come back bit for bit; every case runs twice into fresh buffers: the same bits, except for the atomic overlap-add forms
(fft_synthesis_kernel<*, *, atomic>: the order of fp32 atomics is not fixed).  A failure names the entry point, the forms, the output
and the element (row, frame, bin or sample).  Every case is one the contract allows."""
import ctypes as C
import functools

import pytest
import torch

from tests import fft_ref as F
from tests.kernel_harness import Guarded, api, bits, judge, report, same_bits, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

_judge = functools.partial(judge, exact="value")                        # bound 0: the fp64 value rounded once, -0 == +0


def _cdesc(d):
    from remfx_amd._lib import StftDesc
    c = StftDesc()
    for k in F.FIELDS:
        setattr(c, k, getattr(d, k))
    return c


def _forms_label(forms):
    return sorted(f for f in forms if "<" in f)


# ---- analysis ----------------------------------------------------------------------------------------------------------------------
def _run_analysis(d, x, w, mul, x_off):
    L, _, stream = api()
    X = Guarded(x.numel(), what="x", init=x, off=x_off)
    W = Guarded(w.numel(), what="window", init=w)
    M = Guarded(mul.numel(), what="mul", init=mul) if mul is not None else None
    n_out = 1
    for s in F.layout_shape(d):
        n_out *= s
    O = Guarded(n_out, what="out")
    cd = _cdesc(d)
    rc = L.rfx_fft_analysis(C.byref(cd), X.ptr(), W.ptr(), M.ptr() if M else None, O.ptr(), stream())
    torch.cuda.synchronize()
    for b in (X, W) + ((M,) if M else ()):
        b.unchanged()
    return rc, O


@pytest.mark.parametrize("name", [c["name"] for c in F.ANALYSIS_CASES])
def test_analysis(name):
    """rfx_fft_analysis at every launch form of fft_ref.forms_analysis (both kernel files, every instantiation and output mode, the fast
    and the mapped load path in one launch, a misaligned x, nb = 1 / 2 / 4 with the next batch prefetched over the epilogue, mul, herm,
    both in_modes, extra pads, short bins, frame0, a ragged last batch, R % 8): every cell of every frame within K eps32 of its frame's
    norm; mag / pow / magpow within the image of that interval."""
    c = F._case_by_name(name)
    x, w, mul = F.analysis_inputs(c)
    d0 = c["d"]
    X, mag = F.spectrum(F.with_(d0, mode=F.FM), x, w, mul)
    for mode in c["modes"]:
        d = F.with_(d0, mode=mode)
        forms = F.forms_analysis(d, bool(c["x_off"]), c["mul"])
        ref, bound = F.to_layout(d, X), F.analysis_bound(d, X, mag)

        def run():
            rc, O = _run_analysis(d, x, w, mul, c["x_off"])
            assert rc == 0, ("rfx_fft_analysis", name, rc)
            return {"out": O.cpu()}
        a, b = run(), run()
        same_bits(a, b, ("rfx_fft_analysis", name, F.MODE_NAMES[mode]))
        r = _judge(a["out"], ref, bound, ctx=("rfx_fft_analysis", sorted(forms), "out"))
        report("FFT", "rfx_fft_analysis", {F.MODE_NAMES[mode]: r}, f"{name} {_forms_label(forms)}")


# ---- synthesis ---------------------------------------------------------------------------------------------------------------------
def _ws_buf(L, cd, d):
    n = int(L.rfx_fft_synthesis_ws(C.byref(cd)))
    assert n == F.syn_ws_floats(d), ("rfx_fft_synthesis_ws", n, F.syn_ws_floats(d))
    return Guarded(n, what="ws")


def _run_synthesis(d, spec, w, mul, out0):
    L, _, stream = api()
    S = Guarded(spec.numel(), what="spec", init=spec)
    W = Guarded(w.numel(), what="window", init=w)
    M = Guarded(mul.numel(), what="mul", init=mul) if mul is not None else None
    O = Guarded(d.R * d.T, what="out", init=out0)
    cd = _cdesc(d)
    WS = _ws_buf(L, cd, d)
    rc = L.rfx_fft_synthesis(C.byref(cd), S.ptr(), W.ptr(), M.ptr() if M else None, WS.ptr(), O.ptr(), stream())
    torch.cuda.synchronize()
    for b in (S, W) + ((M,) if M else ()):
        b.unchanged()
    WS.guards_intact()
    return rc, O


@pytest.mark.parametrize("name", [c["name"] for c in F.SYNTHESIS_CASES])
def test_synthesis(name):
    """rfx_fft_synthesis at every form of fft_ref.forms_synthesis: overlap-add by ownership with one, two and three walks (the last
    taking a remainder), the smallest ownership row and the largest atomic one, every sample covered / not (samples no frame covers
    read exactly 0, or out0 under accum), accum, the three layouts, no Nyquist bin, mul, HDemucs' _ispec, the atomic forms (extra pads,
    hop > win, the division path of hop > 4096), and fft_any.hip's mirrored, mirrored-with-extra-pads and offset gathers."""
    c = F._case_by_name(name)
    d = c["d"]
    S, w, mul, out0 = F.synthesis_inputs(c)
    forms = F.forms_synthesis(d, False, c["mul"])
    ref, bound = F.synthesis(d, S, w, mul, out0)
    spec = F.store_layout(d, S)

    def run():
        rc, O = _run_synthesis(d, spec, w, mul, out0)
        assert rc == 0, ("rfx_fft_synthesis", name, rc)
        return {"out": O.cpu()}
    a, b = run(), run()
    if not any(",atomic>" in f for f in forms):
        same_bits(a, b, ("rfx_fft_synthesis", name))
    r = _judge(a["out"], ref, bound, ctx=("rfx_fft_synthesis", sorted(forms), "out"))
    report("FFT", "rfx_fft_synthesis", {"out": r}, f"{name} {_forms_label(forms)}")


# ---- loss gradient inside the synthesis --------------------------------------------------------------------------------------------
def _run_lossgrad(d, xspec, ymag, sums, gup, w, out0):
    L, _, stream = api()
    X = Guarded(xspec.numel(), what="xspec", init=xspec)
    Y = Guarded(ymag.numel(), what="ymag", init=ymag)
    SM = Guarded(sums.numel(), what="sums", init=sums)
    G = Guarded(1, what="gup", init=torch.tensor([gup])) if gup is not None else None
    W = Guarded(w.numel(), what="window", init=w)
    O = Guarded(d.R * d.T, what="out", init=out0)
    cd = _cdesc(d)
    WS = _ws_buf(L, cd, d)
    rc = L.rfx_fft_synthesis_lossgrad(C.byref(cd), X.ptr(), Y.ptr(), SM.ptr(), F.LG_W_SC, F.LG_W_LM, F.LG_EPS, G.ptr() if G else None, W.ptr(),
                                      WS.ptr(), O.ptr(), stream())
    torch.cuda.synchronize()
    for b in (X, Y, SM, W) + ((G,) if G else ()):
        b.unchanged()
    WS.guards_intact()
    return rc, O


@pytest.mark.parametrize("name", [c["name"] for c in F.LOSSGRAD_CASES])
def test_synthesis_lossgrad(name):
    """rfx_fft_synthesis_lossgrad on synthetic xspec / ymag / sums at all four sizes -- n_fft = 4096 (fft_synthesis_kernel<11, true, *>)
    has no forward that feeds it, so nothing else launches that instantiation -- ownership with one and several walks and the atomic
    form, gup null and set, accum, a row whose A is 0 (ksc = 0: only the log term).  Bins 3 and 4 of every frame hold X = 0 and
    |X|^2 == eps exactly, bins 5 and 6 |X|^2 one step below eps and X = (0.375, 0.5) against ymag = 0.625 (no gradient in any of the four:
    the clamp is strict, the sign at equality is 0); three frames of row 0 hold one cell each and zeros: |X|^2 one ulp above eps (the
    full gradient) and ymag one ulp above / below |X|.  No other cell of the inputs lies in the sign band or the eps band
    (test_fft_ref_cpu.py asserts it), so the fp64 reference takes the branches the kernel takes."""
    c = F._case_by_name(name)
    d = c["d"]
    X, ymag, sums, w = F.lossgrad_inputs(c)
    out0 = F.signal(d.R, d.T, c["seed"] + 3) if d.accum else None
    forms = F.forms_synthesis(d, True)
    ref, bound = F.synthesis_lossgrad(d, X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"], w, out0)
    xspec = torch.view_as_real(X.contiguous()).contiguous()

    def run():
        rc, O = _run_lossgrad(d, xspec, ymag, sums, c["gup"], w, out0)
        assert rc == 0, ("rfx_fft_synthesis_lossgrad", name, rc)
        return {"out": O.cpu()}
    a, b = run(), run()
    if not any(",atomic>" in f for f in forms):
        same_bits(a, b, ("rfx_fft_synthesis_lossgrad", name))
    # the two lone one-ulp cells of row 0: the sign of the log term is -1 / +1 if the hardware square root returns |X| = 0.625 exactly
    # (the reference), 0 if it lands on ymag; each frame's two outcomes are closed forms, any of the four combinations is accepted and
    # every other sample is judged the same way under each
    deltas = F.lossgrad_sign_deltas(d, X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"], w)
    last = None
    for drop in ((), (0,), (1,), (0, 1)):
        try:
            r = _judge(a["out"], ref - sum(deltas[i] for i in drop), bound, ctx=("rfx_fft_synthesis_lossgrad", sorted(forms), "out"))
            report("FFT", "rfx_fft_synthesis_lossgrad", {"out": r, "one-ulp cells with sign 0": float(len(drop))}, f"{name} {_forms_label(forms)}")
            return
        except AssertionError as e:
            last = last or e
    raise last


# ---- pair loss ---------------------------------------------------------------------------------------------------------------------
def _run_pair(d, x, y, w, store, scale=1.0):
    L, _, stream = api()
    X = Guarded(x.numel(), what="x", init=x)
    Y = Guarded(y.numel(), what="y", init=y)
    W = Guarded(w.numel(), what="window", init=w)
    cd = _cdesc(F.with_(d, scale=scale))
    nws = int(L.rfx_stft_pair_loss_ws(C.byref(cd)))
    assert nws == 3 * d.R * F.pair_geometry(d)[1], ("rfx_stft_pair_loss_ws", nws)
    WS = Guarded(nws, dtype=torch.float64, what="ws")
    SM = Guarded(3 * d.R, what="sums")
    cells = d.R * d.frames_out * d.bins
    XS = Guarded(2 * cells, what="xspec") if store else None
    YM = Guarded(cells, what="ymag") if store else None
    rc = L.rfx_stft_pair_loss(C.byref(cd), X.ptr(), Y.ptr(), W.ptr(), F.EPS, WS.ptr(), SM.ptr(), XS.ptr() if store else None,
                              YM.ptr() if store else None, stream())
    torch.cuda.synchronize()
    for b in (X, Y, W):
        b.unchanged()
    WS.guards_intact()
    return rc, SM, XS, YM


@pytest.mark.parametrize("name", [c["name"] for c in F.PAIR_CASES])
def test_pair_loss(name):
    """rfx_stft_pair_loss at 512 / 1024 / 2048 on the ragged shapes (fewer frames than a batch, an odd hop, R = 17, every frame an edge
    frame) and on rows with interior batches, spectra stored and not: every cell of the stored spectrum and magnitudes, every row's
    three sums; the row with y == x has exactly 0 in its two numerator sums."""
    c = F._case_by_name(name)
    d = c["d"]
    x, y, w = F.pair_inputs(c)
    ref = F.pair_loss(d, x, y, w, F.EPS)
    dfm = F.with_(d, mode=F.FM)
    ratios = {}
    for store in (True, False):
        forms = F.forms_pair(d, store)

        def run():
            rc, SM, XS, YM = _run_pair(d, x, y, w, store)
            assert rc == 0, ("rfx_stft_pair_loss", name, rc)
            out = {"sums": SM.cpu()}
            if store:
                out.update(xspec=XS.cpu(), ymag=YM.cpu())
            return out
        a, b = run(), run()
        same_bits(a, b, ("rfx_stft_pair_loss", name, store))
        tag = "stored" if store else "sums_only"
        ratios["sums " + tag] = _judge(a["sums"], ref["sums"], ref["sums_bound"], ctx=("rfx_stft_pair_loss", sorted(forms), "sums"))
        if d.R > 1:
            s = a["sums"].view(d.R, 3)
            assert float(s[0, 0]) == 0.0 and float(s[0, 2]) == 0.0, ("rfx_stft_pair_loss", name, "row 0 has y == x", s[0].tolist())
        if store:
            ratios["xspec"] = _judge(a["xspec"], ref["xspec"], ref["xspec_bound"], ctx=("rfx_stft_pair_loss", sorted(forms), "xspec"))
            ratios["ymag"] = _judge(a["ymag"], ref["ymag"], ref["ymag_bound"], ctx=("rfx_stft_pair_loss", sorted(forms), "ymag"))
    report("FFT", "rfx_stft_pair_loss", ratios, f"{name} {_forms_label(F.forms_pair(d, True))}")


@pytest.mark.parametrize("name", [c["name"] for c in F.PAIR_NB_CASES])
def test_pair_loss_many_batches(name):
    """rfx_stft_pair_loss where a workgroup walks nb = 2 / 4 batches (R = 64 at 2021 / 4040 frames of 512 / 16: the forms only the
    benchmark reached): the next batch's loads issued over the epilogue and the group boundaries.  The stored spectra are 0.27 / 0.53 GB
    and the magnitudes half of that, so the per-element judgement is a SAMPLE: all frames of rows 0, 7, 8 and R - 1, and in every row the
    frames on either side of every batch and group boundary (where a wrong prefetch, a wrong `fast` flag or the last-pair rule would
    show); every row's sums are judged, and on the device every element of both outputs must be finite, every guard intact and the
    second run's bits the same.  What the sample cannot see is a wrong cell in the interior of a batch of a row outside the four --
    the code path of such a cell is the one the four rows run in full."""
    c = F._case_by_name(name)
    d = c["d"]
    x, y, w = F.pair_inputs(c)
    ref = F.pair_loss_sampled(d, x, y, w, F.EPS)
    forms = sorted(F.forms_pair(d, True))
    runs = []
    for _ in range(2):
        rc, SM, XS, YM = _run_pair(d, x, y, w, True)
        assert rc == 0, ("rfx_stft_pair_loss", name, rc)
        for b in (SM, XS, YM):
            b.guards_intact()
        assert bool(torch.isfinite(XS.t).all()) and bool(torch.isfinite(YM.t).all()), ("rfx_stft_pair_loss", name, "a stored element is not finite / not written")
        runs.append((SM.t.clone(), XS.t, YM.t))
    for k in range(3):
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), ("rfx_stft_pair_loss", name, ("sums", "xspec", "ymag")[k], "second run differs")
    sums, XS, YM = runs[0]
    X4, Y3 = XS.view(d.R, d.frames_out, d.bins, 2), YM.view(d.R, d.frames_out, d.bins)
    rows, fr = torch.tensor(ref["rows"], device="cuda"), ref["frames"].cuda()
    ratios = {"sums": _judge(sums.cpu(), ref["sums"], ref["sums_bound"], ctx=("rfx_stft_pair_loss", forms, "sums"))}
    assert float(sums.view(d.R, 3)[0, 0]) == 0.0 and float(sums.view(d.R, 3)[0, 2]) == 0.0, ("row 0 has y == x", sums[:3].tolist())

    ex = lambda b: b[..., None].expand(*b.shape, 2).contiguous()                                # noqa: E731
    ratios["xspec rows"] = _judge(X4[rows].cpu(), ref["row_x"], ex(ref["row_bx"]), ctx=("rfx_stft_pair_loss", forms, "xspec", "rows", ref["rows"]))
    ratios["ymag rows"] = _judge(Y3[rows].cpu(), ref["row_ym"], ref["row_bym"], ctx=("rfx_stft_pair_loss", forms, "ymag", "rows", ref["rows"]))
    ratios["xspec boundaries"] = _judge(X4[:, fr].cpu(), ref["fr_x"], ex(ref["fr_bx"]), ctx=("rfx_stft_pair_loss", forms, "xspec", "frames", ref["frames"].tolist()))
    ratios["ymag boundaries"] = _judge(Y3[:, fr].cpu(), ref["fr_ym"], ref["fr_bym"], ctx=("rfx_stft_pair_loss", forms, "ymag", "frames", ref["frames"].tolist()))
    rc, SM, _, _ = _run_pair(d, x, y, w, False)
    assert rc == 0
    ratios["sums, nothing stored"] = _judge(SM.cpu(), ref["sums"], ref["sums_bound"], ctx=("rfx_stft_pair_loss", sorted(F.forms_pair(d, False)), "sums"))
    report("FFT", "rfx_stft_pair_loss", ratios, f"{name} {_forms_label(F.forms_pair(d, True))}")


# ---- the cell kernels of losses.hip ------------------------------------------------------------------------------------------------
def _pairs(Z):
    return torch.view_as_real(Z.contiguous()).contiguous()


# + one row exactly one workgroup past grid_red's cap of REDUCE_SLOTS workgroups of 16384 cells
REDUCE_CASES = [(R, n) for n in F.CELL_N for R in F.CELL_R] + [(1, F.REDUCE_SLOTS * 16384 + 1)]


@pytest.mark.parametrize("R,n", REDUCE_CASES)
def test_loss_reduce(R, n):
    """rfx_stft_loss_reduce on given spectra: the three row sums against fp64 within K eps32 of the terms' first-order magnitude
    (K from the measured floor of their float32 evaluation) plus gamma_8 of the fp32 partial sums of eight cells; the stored float32
    spectra are the inputs, so no cell carries an interval.  n = 1 ... one
    more than a whole unroll-by-eight round (the clamped index at n - 1), several slots and a second grid-stride round, and one workgroup
    more than the capped grid has, with ws exactly as long as rfx_stft_loss_reduce_ws says; X = 0 and |X|^2 at, just below and just
    above eps are among the cells."""
    L, _, stream = api()
    X, Y, _, _ = F.cell_inputs(R, n, 100 * R + n)
    z = torch.zeros(R, n, dtype=torch.float64)
    ref = F.loss_sums(X, Y, F.CELL_EPS)
    bound = F.loss_sums_bound(X.to(torch.complex128), Y.to(torch.complex128), z, z, F.CELL_EPS, group=8)

    def run():
        XB, YB = Guarded(2 * R * n, what="xc", init=_pairs(X)), Guarded(2 * R * n, what="yc", init=_pairs(Y))
        nws = int(L.rfx_stft_loss_reduce_ws(R, n))
        assert nws == 3 * R * F.REDUCE_SLOTS                   # the restated cap per row and sum, for every n
        WS = Guarded(nws, dtype=torch.float64, what="ws")
        SM = Guarded(3 * R, what="sums")
        rc = L.rfx_stft_loss_reduce(XB.ptr(), YB.ptr(), R, n, F.CELL_EPS, WS.ptr(), SM.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, ("rfx_stft_loss_reduce", rc)
        XB.unchanged(), YB.unchanged(), WS.guards_intact()
        return {"sums": SM.cpu()}
    a, b = run(), run()
    same_bits(a, b, ("rfx_stft_loss_reduce", R, n))
    forms = F.forms_cells(n, "reduce")
    r = _judge(a["sums"], ref, bound, ctx=("rfx_stft_loss_reduce", sorted(forms), "sums"))
    print(f"\nFFT rfx_stft_loss_reduce R={R} n={n} {sorted(forms)}: largest error / bound {r:.3f}")


@pytest.mark.parametrize("n", F.CELL_N)
@pytest.mark.parametrize("R", F.CELL_R)
@pytest.mark.parametrize("kernel", ("yc", "ymag"))
def test_loss_grad_cells(kernel, R, n):
    """rfx_stft_loss_grad (target spectrum) and rfx_stft_loss_grad_m (clamped target magnitudes) per cell against
    fft_ref.lossgrad_cells, a function of the stored float32 inputs: K eps32 times the first-order magnitude of the cell's two terms.
    The designated cells: X = 0, |X|^2 just below and exactly at eps give exactly 0; one ulp above eps the full gradient; |X| == ymag
    gives exactly 0 (the sign is 0 and so is the difference); ymag one ulp above / below |X| gives the log term's sign -- exact for
    the magnitude form, while the spectrum form takes its sign from logf(|X|) - logf(|Y|), which may be 0 within an ulp: there either
    closed form is accepted.  gup null and set; a row whose A is 0."""
    L, _, stream = api()
    X, Y, ymag, sums = F.cell_inputs(R, n, 100 * R + n)
    ratios = {}
    for gup in (None, 1.7):
        if kernel == "ymag":
            G, mag = F.lossgrad_cells(X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.CELL_EPS, gup)
        else:
            G, mag = F.stft_loss_grad(X, Y, sums, F.LG_W_SC, F.LG_W_LM, F.CELL_EPS, gup)
        ref, bound = _pairs(G), (F.k_cell() * F.EPS32 * mag)[..., None].expand(-1, -1, 2).contiguous()

        def run():
            XB = Guarded(2 * R * n, what="xc", init=_pairs(X))
            TB = Guarded(2 * R * n, what="yc", init=_pairs(Y)) if kernel == "yc" else Guarded(R * n, what="ymag", init=ymag)
            SM = Guarded(3 * R, what="sums", init=sums)
            U = Guarded(1, what="gup", init=torch.tensor([gup])) if gup is not None else None
            O = Guarded(2 * R * n, what="gxc")
            fn = L.rfx_stft_loss_grad if kernel == "yc" else L.rfx_stft_loss_grad_m
            rc = fn(XB.ptr(), TB.ptr(), R, n, F.CELL_EPS, SM.ptr(), F.LG_W_SC, F.LG_W_LM, U.ptr() if U else None, O.ptr(), stream())
            torch.cuda.synchronize()
            assert rc == 0, (kernel, rc)
            for bb in (XB, TB, SM) + ((U,) if U else ()):
                bb.unchanged()
            return {"gxc": O.cpu()}
        a, b = run(), run()
        same_bits(a, b, ("stft_loss_grad_kernel", kernel, R, n))
        got = a["gxc"].view(R, n, 2).clone()
        if kernel == "yc" and n >= 255:
            # the two one-ulp cells of the spectrum form: the sign term may be absent (logf(|X|) == logf(|Y|)); the other closed form
            G0, _ = F.stft_loss_grad(X, Y, sums, F.LG_W_SC, 0.0, F.CELL_EPS, gup)
            for c in (F.DESIGNATED_COL + 5, F.DESIGNATED_COL + 6):
                alt = _pairs(G0)[:, c]
                use_alt = ((got[:, c].double() - alt).abs() <= bound[:, c]).all(-1)
                ref[:, c] = torch.where(use_alt[:, None], alt, ref[:, c])
        forms = F.forms_cells(n, kernel, gup is not None)
        ratios["gup" if gup else "no_gup"] = _judge(got, ref, bound, ctx=("rfx_stft_loss_grad" + ("_m" if kernel == "ymag" else ""), sorted(forms), "gxc"))
        if n >= 255:
            c = F.DESIGNATED_COL
            assert bool((got[:, c:c + 3] == 0).all()) and bool((got[:, c + 4] == 0).all()), (kernel, "designated cells", got[:, c:c + 7].tolist())
    print(f"\nFFT stft_loss_grad_kernel:{kernel} R={R} n={n}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """What the entry points refuse returns its code and writes nothing (a refusal launches nothing): a null descriptor, an output mode
    the synthesis has no layout for, xspec without ymag, and for the pair loss n_fft = 4096, extra pads, frame0 != 0, short bins and
    scale != 1 (the kernel applies no scale); rfx_fft_synthesis_ws and rfx_stft_pair_loss_ws return -1 for descriptors no kernel covers."""
    L, _, stream = api()
    d = F.desc(3, 3000, 512, 128, 512, mode=F.FM)
    x, w = F.signal(3, 3000, 1), F.hann(512)
    X, W = Guarded(x.numel(), what="x", init=x), Guarded(512, what="window", init=w)
    O = Guarded(3 * d.frames_out * d.bins * 2, what="out")
    assert L.rfx_fft_analysis(None, X.ptr(), W.ptr(), None, O.ptr(), stream()) != 0
    assert L.rfx_fft_synthesis_ws(None) == -1 and L.rfx_stft_pair_loss_ws(None) == -1
    for bad in (F.with_(d, n_fft=500), F.with_(d, n_fft=8), F.with_(d, win=513), F.with_(d, bins=258), F.with_(d, hop=0), F.with_(d, frames_out=0)):
        cd = _cdesc(bad)
        assert L.rfx_fft_analysis(C.byref(cd), X.ptr(), W.ptr(), None, O.ptr(), stream()) != 0, vars(bad)
        assert L.rfx_fft_synthesis_ws(C.byref(cd)) == -1, vars(bad)
    assert L.rfx_stft_pair_loss_ws(C.byref(_cdesc(F.with_(d, n_fft=4096, win=4096, bins=2049)))) == -1
    spec = Guarded(3 * d.frames_out * d.bins * 2, what="spec", init=torch.randn(3 * d.frames_out * d.bins * 2))
    T = Guarded(3 * 3000, what="signal out")
    WS = Guarded(F.syn_ws_floats(d), what="ws")
    assert L.rfx_fft_synthesis(None, spec.ptr(), W.ptr(), None, WS.ptr(), T.ptr(), stream()) != 0
    for mode in (F.MAG, F.POW, F.MAGPOW, 6, -1):
        for n_fft in (512, 256):
            cd = _cdesc(F.with_(d, mode=mode, n_fft=n_fft, win=n_fft, bins=n_fft // 2 + 1))
            assert L.rfx_fft_synthesis(C.byref(cd), spec.ptr(), W.ptr(), None, WS.ptr(), T.ptr(), stream()) == -1, (mode, n_fft)
    cd = _cdesc(d)
    assert L.rfx_fft_synthesis(C.byref(cd), spec.ptr(), W.ptr(), None, None, T.ptr(), stream()) == -1          # the ownership form without scratch
    ym, sm = Guarded(3 * d.frames_out * d.bins, what="ymag", init=torch.ones(3 * d.frames_out * d.bins)), Guarded(9, what="sums", init=torch.ones(9))
    assert L.rfx_fft_synthesis_lossgrad(C.byref(cd), spec.ptr(), None, sm.ptr(), 1.0, 1.0, F.EPS, None, W.ptr(), WS.ptr(), T.ptr(), stream()) == -1
    assert L.rfx_fft_synthesis_lossgrad(C.byref(cd), spec.ptr(), ym.ptr(), None, 1.0, 1.0, F.EPS, None, W.ptr(), WS.ptr(), T.ptr(), stream()) == -1
    assert L.rfx_fft_synthesis_lossgrad(C.byref(_cdesc(F.with_(d, mode=F.COMPLEX))), spec.ptr(), ym.ptr(), sm.ptr(), 1.0, 1.0, F.EPS, None, W.ptr(),
                                        WS.ptr(), T.ptr(), stream()) == -1
    assert L.rfx_fft_synthesis_lossgrad(None, spec.ptr(), ym.ptr(), sm.ptr(), 1.0, 1.0, F.EPS, None, W.ptr(), WS.ptr(), T.ptr(), stream()) == -1
    # pair loss
    PW = Guarded(3 * F.pair_geometry(d)[1], dtype=torch.float64, what="pair ws")
    SM = Guarded(9, what="pair sums")
    XS, YM = Guarded(3 * d.frames_out * d.bins * 2, what="xspec"), Guarded(3 * d.frames_out * d.bins, what="ymag out")
    bads = dict(null=None, n4096=F.with_(d, n_fft=4096, win=4096, bins=2049), pads=F.with_(d, extra_pad_l=3), pad_r=F.with_(d, extra_pad_r=3),
                frame0=F.with_(d, frame0=1, frames_out=d.frames_out - 1), bins=F.with_(d, bins=256), in_mode=F.with_(d, in_mode=1),
                scale=F.with_(d, scale=0.5), scale2=F.with_(d, scale=F.f32(1.0 / 512 ** 0.5)))
    for k, bad in bads.items():
        cd = _cdesc(bad) if bad is not None else None
        rc = L.rfx_stft_pair_loss(C.byref(cd) if cd is not None else None, X.ptr(), X.ptr(), W.ptr(), F.EPS, PW.ptr(), SM.ptr(), XS.ptr(), YM.ptr(), stream())
        assert rc == -1, ("rfx_stft_pair_loss accepted", k, rc)
    cd = _cdesc(d)
    assert L.rfx_stft_pair_loss(C.byref(cd), X.ptr(), X.ptr(), W.ptr(), F.EPS, PW.ptr(), SM.ptr(), XS.ptr(), None, stream()) == -1     # xspec without ymag
    assert L.rfx_stft_pair_loss(C.byref(cd), X.ptr(), X.ptr(), W.ptr(), F.EPS, PW.ptr(), SM.ptr(), None, YM.ptr(), stream()) == -1
    torch.cuda.synchronize()
    for b in (O, T, WS, PW, SM, XS, YM):
        b.untouched()
    for b in (X, W, spec, ym, sm):
        b.unchanged()
    print("\nFFT refusals: refused")
