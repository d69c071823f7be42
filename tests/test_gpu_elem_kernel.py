"""Every entry point of remfx_amd/csrc/elementwise.hip (but rfx_row_affine_add / rfx_fm_cm_affine_g, pinned in test_gpu_multisource.py)
and rfx_l1_grad, through the C ABI on buffers this test allocates, against tests/elem_ref.py (fp64), per element.  The bounds and where
their constants come from are in elem_ref's docstring and DESIGN.md 4.21; none is measured on a kernel.

Buffers: every input and output sits between NaN guards of 4096 elements, outputs are NaN-filled, workspaces are exactly the size the
_ws / _slots call returns; inputs have to come back bit for bit; every case runs twice into fresh buffers: the same bits.  A failure
names the entry point, the output and the element."""
import ctypes

import numpy as np
import pytest
import torch

from tests import elem_ref as E
from tests.kernel_harness import Guarded, api, bits, judge, report, stop_after_a_device_error, twice  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

# ---- flat activations --------------------------------------------------------------------------------------------------------------
def _flat(entry, code, n, off, x, other):
    L, _, stream = api()
    X = Guarded(n, what="x", init=x, off=off)
    Y = Guarded(n, what="y", off=off)
    if entry == "rfx_act_fwd":
        rc = L.rfx_act_fwd(X.ptr(), Y.ptr(), n, code, stream())
        ins = (X,)
    else:
        O = Guarded(n, what="gy" if entry == "rfx_act_bwd" else "res", init=other, off=off)
        fn = L.rfx_act_bwd if entry == "rfx_act_bwd" else L.rfx_act_add_fwd
        rc = fn(X.ptr(), O.ptr(), Y.ptr(), n, code, stream())
        ins = (X, O)
    torch.cuda.synchronize()
    for b in ins:
        b.unchanged()
    return rc, Y


@pytest.mark.parametrize("n", E.FLAT_N)
@pytest.mark.parametrize("code", range(7), ids=E.ACT_NAMES)
def test_flat_activations(code, n):
    """rfx_act_fwd / _bwd / _add_fwd, acts 0 - 6: the float4 body, the n % 4 tail, one workgroup ... grid_for's cap with a second grid-stride
    iteration, and (two sizes) from a view one element into its allocation.  none / ReLU / leaky and their derivatives bit for bit;
    GELU, tanh, sigmoid by the K rule; act_add adds its sum's half-ulp.  act == RFX_ACT_PRELU is refused (no slope argument) and
    nothing is written."""
    x, gy, res = E.act_data(n, 11 + n), E.signs_data(n, 12 + n), E.signs_data(n, 13 + n, 0.1, 3.0)
    ratios = []
    for off in ((0, 1) if n in E.FLAT_OFFSET_N else (0,)):
        for entry, other in (("rfx_act_fwd", None), ("rfx_act_bwd", gy), ("rfx_act_add_fwd", res)):
            if code == E.PRELU:
                rc, Y = _flat(entry, code, n, off, x, other)
                assert rc != 0, (entry, "accepted RFX_ACT_PRELU")
                Y.untouched()
                continue

            def run():
                rc, Y = _flat(entry, code, n, off, x, other)
                assert rc == 0, (entry, rc)
                return {"y": Y.cpu()}
            got = twice(run)[0]["y"]
            if entry == "rfx_act_fwd":
                ref, bound = E.act(x, code), E.act_bound(x, code)
            elif entry == "rfx_act_bwd":
                ref, bound = gy.double() * E.act_grad(x, code), E.act_grad_bound(x, gy, code)
            else:
                ref, bound = E.act(x, code) + res.double(), E.act_add_bound(x, res, code)
            ratios.append((entry, judge(got, ref, bound, ctx=(entry, "y", E.ACT_NAMES[code], "n", n, "offset", off, sorted(E.forms_flat("", n))))))
    report("ELEM", f"flat {E.ACT_NAMES[code]} n={n}", ratios)


# ---- act_rows ----------------------------------------------------------------------------------------------------------------------
def _rows_data(D, T, x16, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(*D, T, generator=g, dtype=torch.float64) * 12.0 - 6.0).float()
    if x16:
        x = x.bfloat16().float()                               # the value the 16 stored bits hold
    return x, E.signs_data(D[0] * D[1] * D[2] * T, seed + 1).view(*D, T)


def _place(flat, logical, D, st, T):
    for i0 in range(D[0]):
        for i1 in range(D[1]):
            for i2 in range(D[2]):
                o = i0 * st[0] + i1 * st[1] + i2 * st[2]
                flat[o:o + T] = logical[i0, i1, i2]
    return flat


def _gather(flat, D, st, T):
    out = torch.empty(*D, T, dtype=flat.dtype)
    for i0 in range(D[0]):
        for i1 in range(D[1]):
            for i2 in range(D[2]):
                o = i0 * st[0] + i1 * st[1] + i2 * st[2]
                out[i0, i1, i2] = flat[o:o + T]
    return out


def _rows(x16, bwd, D, T, code, falsify=None, seed=5):
    """-> (logical result, largest error / bound)"""
    L, _, stream = api()
    lay = E.rows_layout(D, T, x16, falsify)
    xl, gl = _rows_data(D, T, x16, seed + T)
    xdt = torch.bfloat16 if x16 else torch.float32
    odt = torch.bfloat16 if (x16 and bwd) else torch.float32
    xflat = _place(torch.zeros(lay["x_len"]), xl, D, lay["xs"], T)
    gflat = _place(torch.zeros(lay["out_len"]), gl, D, lay["gs"], T)
    forms = E.forms_rows(x16, bwd, D, T, lay["xs"] + lay["os"] + (lay["gs"] if bwd else ()), lay["x_off"] * (2 if x16 else 4),
                         lay["out_off"] * (2 if odt == torch.bfloat16 else 4), lay["gy_off"] * 4)
    info = (E.ACT_NAMES[code], "D", D, "T", T, "falsified", falsify, sorted(forms))
    entry = "rfx_act_rows16" if x16 else "rfx_act_rows"

    def run():
        X = Guarded(lay["x_len"], xdt, "x", xflat, lay["x_off"])
        G = Guarded(lay["out_len"], torch.float32, "gy", gflat, lay["gy_off"]) if bwd else None
        O = Guarded(lay["out_len"], odt, "out", None, lay["out_off"])
        fn = L.rfx_act_rows16 if x16 else L.rfx_act_rows
        rc = fn(X.ptr(), *lay["xs"], G.ptr() if bwd else None, *(lay["gs"] if bwd else (0, 0, 0)), O.ptr(), *lay["os"], *D, T, code, stream())
        torch.cuda.synchronize()
        assert rc == 0, (entry, rc, info)
        X.unchanged()
        if bwd:
            G.unchanged()
        got = O.cpu()
        O.still_fill(got, torch.isnan(ref))
        return {"out": got}
    ref = E.act_rows(xflat, D, lay["xs"], lay["os"], T, code, torch.full((lay["out_len"],), float("nan"), dtype=torch.float64),
                     gflat if bwd else None, lay["gs"])
    got = twice(run)[0]["out"]
    inside = ~torch.isnan(ref)
    xo = _place(torch.zeros(lay["out_len"]), xl, D, lay["os"], T)[inside]
    if not bwd:
        bound = E.act_bound(xo, code)
    else:
        bound = E.act_grad_bound(xo, gflat[inside], code)
        if x16:                                                  # the fp32 value (one rounding for the exact forms), then its bf16 rounding
            b32 = bound + E.HALF * ref[inside].abs()
            bound = b32 + E.bf16_half_ulp(ref[inside].abs() + b32)
    r = judge(got[inside], ref[inside], bound, ctx=(entry, "out", *info))
    return _gather(got, D, lay["os"], T), r


@pytest.mark.parametrize("bwd", (False, True), ids=("fwd", "bwd"))
@pytest.mark.parametrize("x16", (False, True), ids=("f32", "bf16"))
def test_act_rows(x16, bwd):
    """rfx_act_rows / rfx_act_rows16, all eight <VEC, X16> x {forward, backward} forms: out in the permuted (D0, D2, D1) row order at a
    row pitch of T + 4 whose gaps keep their NaN; a wave count that is no multiple of 4; every clause of the vec predicate falsified on
    its own at T = 256 -- each such run is the scalar form and they all return the same bits.  bf16 x is read exactly; the bf16
    gradient adds half a bf16 ulp of the value being rounded."""
    ratios = []
    for D in E.ROWS_D:
        for T in E.ROWS_T_VEC + E.ROWS_T_SCALAR:
            for code in ((E.GELU, E.LEAKY, E.SIGMOID, E.TANH, E.RELU, E.NONE) if T in (256, 255) else (E.GELU,)):
                ratios.append(_rows(x16, bwd, D, T, code)[1])
    scalar = []
    for fal in E.ROWS_FALSIFY:
        if fal == "gy" and not bwd:
            continue
        lay = E.rows_layout(E.ROWS_D[0], 256, x16, fal)
        assert not E.rows_vec(x16, bwd, 256, lay["xs"] + lay["os"] + (lay["gs"] if bwd else ()), lay["x_off"] * (2 if x16 else 4),
                              lay["out_off"] * (2 if (x16 and bwd) else 4), lay["gy_off"] * 4), fal
        out, r = _rows(x16, bwd, E.ROWS_D[0], 256, E.GELU, fal)
        ratios.append(r)
        scalar.append((fal, out))
    for fal, out in scalar[1:]:
        assert torch.equal(bits(out), bits(scalar[0][1])), ("the scalar form's result differs between", scalar[0][0], "and", fal)
    L, _, stream = api()
    X, O = Guarded(64, what="x"), Guarded(64, what="out")
    fn = L.rfx_act_rows16 if x16 else L.rfx_act_rows
    assert fn(X.ptr(), 0, 0, 8, None, 0, 0, 0, O.ptr(), 0, 0, 8, 1, 1, 2, 8, E.PRELU, stream()) != 0
    torch.cuda.synchronize()
    O.untouched()
    report("ELEM", f"act_rows x16={x16} bwd={bwd}", ratios)


# ---- mul / prelu -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.MUL_N)
def test_mul(n):
    """rfx_mul bit for bit: the 16-byte body, the tail of 1 - 3, past the cap of 4096 workgroups, and one view a float off alignment"""
    L, _, stream = api()
    a, b = E.act_data(n, 21 + n).clamp(-12, 12), E.signs_data(n, 22 + n)
    for off in ((0, 1) if n == 1027 else (0,)):
        def run():
            A, B, Y = Guarded(n, what="a", init=a, off=off), Guarded(n, what="b", init=b, off=off), Guarded(n, what="y", off=off)
            assert L.rfx_mul(A.ptr(), B.ptr(), Y.ptr(), n, stream()) == 0
            torch.cuda.synchronize()
            A.unchanged(); B.unchanged()
            return {"y": Y.cpu()}
        judge(twice(run)[0]["y"], a.double() * b.double(), 0.0, ctx=("rfx_mul", "y", "n", n, "offset", off, sorted(E.forms_mul(n))))


@pytest.mark.parametrize("shape", E.PRELU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prelu(shape):
    """rfx_prelu_fwd / _bwd: y and gx bit for bit (slopes of both signs and 0, x with +-0: the >= side is part of the contract), gslope by
    the K rule on sum |g v|; ws is N C doubles and every one is written"""
    L, _, stream = api()
    N, Cc, Ln = shape
    x, gy, slope = E.prelu_data(N, Cc, Ln, 31 + Ln)
    info = (shape, sorted(E.forms_prelu(*shape)))

    def run():
        X, G, S = Guarded(x.numel(), what="x", init=x), Guarded(x.numel(), what="gy", init=gy), Guarded(Cc, what="slope", init=slope)
        Y, GX, GS = Guarded(x.numel(), what="y"), Guarded(x.numel(), what="gx"), Guarded(Cc, what="gslope")
        nws = int(L.rfx_prelu_bwd_ws(N, Cc, Ln))
        assert nws == N * Cc                                   # one slot per (sample, channel)
        WS = Guarded(nws, torch.float64, "ws")
        assert L.rfx_prelu_fwd(X.ptr(), S.ptr(), Y.ptr(), N, Cc, Ln, stream()) == 0
        assert L.rfx_prelu_bwd(X.ptr(), G.ptr(), S.ptr(), GX.ptr(), WS.ptr(), GS.ptr(), N, Cc, Ln, stream()) == 0
        torch.cuda.synchronize()
        for b in (X, G, S):
            b.unchanged()
        ws = WS.cpu()
        assert bool(torch.isfinite(ws).all()), ("rfx_prelu_bwd", "ws", "slot", int((~torch.isfinite(ws)).nonzero()[0]), "not written")
        return {"y": Y.cpu(), "gx": GX.cpu(), "gslope": GS.cpu()}
    got, _ = twice(run)
    judge(got["y"], E.act(x, E.PRELU, slope.double().view(1, -1, 1)), 0.0, ctx=("rfx_prelu_fwd", "y", *info))
    gx, gs, mag = E.prelu_bwd(x, gy, slope)
    judge(got["gx"], gx, 0.0, ctx=("rfx_prelu_bwd", "gx", *info))
    r = judge(got["gslope"], gs, E.k_of("gslope") * E.EPS32 * mag + E.TINY, ctx=("rfx_prelu_bwd", "gslope", *info))
    report("ELEM", f"prelu_bwd gslope {shape}", [r])


# ---- L1 ----------------------------------------------------------------------------------------------------------------------------
def _l1(a, b, n, scale, w, gup):
    L, _, stream = api()
    A, B = Guarded(max(n, 1), what="a", init=a if n else None), Guarded(max(n, 1), what="b", init=b if n else None)
    nws = int(L.rfx_l1_sum_ws(n))
    assert nws == E.L1_SLOTS                                   # the restated cap, for every n (524289 of L1_N: one workgroup past it)
    WS, OUT, GR = Guarded(nws, torch.float64, "ws"), Guarded(1, what="out"), Guarded(max(n, 1), what="g")
    GUP = Guarded(1, what="gup", init=torch.tensor([gup])) if gup is not None else None
    assert L.rfx_l1_sum(A.ptr(), B.ptr(), n, WS.ptr(), scale, OUT.ptr(), stream()) == 0
    rg = L.rfx_l1_grad(A.ptr(), B.ptr(), n, w, GUP.ptr() if GUP else None, GR.ptr(), stream())
    torch.cuda.synchronize()
    A.unchanged(); B.unchanged()
    slots, used = WS.cpu(), E.l1_slots(n)
    assert bool(torch.isfinite(slots[:used]).all()) and bool(torch.isnan(slots[used:]).all()), ("rfx_l1_sum", "ws", "slots written", used)
    return rg, OUT, GR, slots


@pytest.mark.parametrize("gup", (None, 0.37), ids=("nogup", "gup"))
@pytest.mark.parametrize("n", E.L1_N)
def test_l1(n, gup):
    """rfx_l1_sum: 1, 2, 512 and the capped 512 slots, every one below the count written and none beyond; fp64-sum bound (one fp32
    rounding per |a - b|, the additions of the longest path, (float)acc and * scale).  rfx_l1_grad bit for bit, an exactly zero gradient
    where a == b."""
    a, b = E.l1_data(n, 41 + n)
    scale = E.f32(1.0 / n)

    def run():
        rg, OUT, GR, slots = _l1(a, b, n, scale, scale, gup)
        assert rg == 0
        return {"out": OUT.cpu(), "g": GR.cpu(), "slots": slots.nan_to_num(-1.0)}
    got, _ = twice(run)
    total = float(E.l1_terms(a, b).sum())
    bound = E.l1_bound(n, total, scale)
    r = judge(got["out"], torch.tensor([E.l1_sum(a, b, scale)], dtype=torch.float64), torch.tensor([bound], dtype=torch.float64),
              ctx=("rfx_l1_sum", "out", "n", n, sorted(E.forms_l1(n, gup))))
    assert 10.0 * scale > bound                                   # leaving the last element out moves the sum by more than the bound
    judge(got["g"], E.l1_grad(a, b, scale, gup), 0.0, ctx=("rfx_l1_grad", "g", "n", n, "gup", gup))
    if n >= 1025:
        assert bool((got["g"][100:200] == 0).all())
    report("ELEM", f"l1_sum n={n}", [r])


def test_l1_n0():
    """n == 0: rfx_l1_sum writes out[0] = 0 as rfx_sumsq does (whatever the scale) and no slot; rfx_l1_grad refuses a non-positive n"""
    rg, OUT, GR, slots = _l1(None, None, 0, float("inf"), 1.0, None)
    assert rg != 0
    GR.untouched()
    out = OUT.cpu()
    assert float(out) == 0.0 and not bool(torch.signbit(out).any())


# ---- channel_sum -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CHANNEL_CASES, ids=lambda c: c["name"])
def test_channel_sum(case):
    """rfx_channel_sum with the workspace rfx_channel_sum_ws returns for the same arguments (exactly that many doubles, all written, a
    guard behind): the plane kernel by the K rule on sum |x|, the strided kernel by the fp64-sum bound"""
    L, _, stream = api()
    base, off, (N, Cc, A, B), st = E.channel_view(case, 51)
    view = base[off:].as_strided((N, Cc, A, B), st)
    slots, nseg = E.channel_geometry(case["x_off"], N, Cc, A, B, *st)
    info = (case["name"], "slots", slots, "nseg", nseg, sorted(E.forms_channel(case["x_off"], N, Cc, A, B, *st)))

    def run():
        X = Guarded(base.numel(), what="x", init=base)
        assert X.t.data_ptr() % 16 == 0
        count = L.rfx_channel_sum_ws(X.ptr(off), N, Cc, A, B, *st)
        assert count == Cc * slots, ("rfx_channel_sum_ws", count, Cc * slots, info)
        WS, OUT = Guarded(count, torch.float64, "ws"), Guarded(Cc, what="out")
        assert L.rfx_channel_sum(X.ptr(off), N, Cc, A, B, *st, WS.ptr(), OUT.ptr(), stream()) == 0
        torch.cuda.synchronize()
        X.unchanged()
        ws = WS.cpu()
        assert bool(torch.isfinite(ws).all()), ("rfx_channel_sum", "ws", "slot", int((~torch.isfinite(ws)).nonzero()[0]), "not written", info)
        return {"out": OUT.cpu(), "ws": ws}
    got = twice(run)[0]["out"]
    ref, sabs = E.channel_sum(view)
    bound = E.channel_bound(case["x_off"], N, Cc, A, B, *st, sabs)
    if case["const"]:
        bound[1] = float(E.channel_bound(case["x_off"], N, Cc, A, B, *st, sabs[1], const=True))
    assert bool((view[N - 1, :, A - 1, B - 1].double().abs() > bound).all())      # leaving the last element out moves the sum by more than the bound
    report("ELEM", f"channel_sum {case['name']}", [judge(got, ref, bound, ctx=("rfx_channel_sum", "out", *info))])


# ---- add_bcast ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.ADD_CASES, ids=lambda c: c["name"])
def test_add_bcast(case):
    """rfx_add_bcast: the flat form (equal strides; tails, an offset view) and the rows form with every broadcast pattern of the model,
    B in {1, 63, 256, 257}, alpha in {1, -0.5}, 45 rows: 2 half-ulps of |x| + |alpha y| (holds with and without an FMA)"""
    L, _, stream = api()
    N, Cc, A, B, off = case["N"], case["C"], case["A"], case["B"], case["off"]
    x = torch.randn(N, Cc, A, B, generator=torch.Generator().manual_seed(61))
    y, st = E.add_y(case, 62)
    alpha = case["alpha"]

    def run():
        X, Y, O = Guarded(x.numel(), what="x", init=x, off=off), Guarded(y.numel(), what="y", init=y, off=off), Guarded(x.numel(), what="out", off=off)
        assert L.rfx_add_bcast(X.ptr(), Y.ptr(), O.ptr(), N, Cc, A, B, *st, alpha, stream()) == 0
        torch.cuda.synchronize()
        X.unchanged(); Y.unchanged()
        return {"out": O.cpu()}
    ref, mag = E.add_bcast(x, y, st, alpha)
    report("ELEM", f"add_bcast {case['name']}", [judge(twice(run)[0]["out"], ref, E.EPS32 * mag, ctx=("rfx_add_bcast", "out", case["name"], sorted(E.forms_add(case))))])


# ---- span_mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.SPAN_CASES, ids=lambda c: f"{c['R']}x{c['F']}x{c['T']}_t0_{c['t0'][0]}")
def test_span_mask(case):
    """rfx_span_mask in place on a random BIT pattern: +0 inside the spans, every bit kept outside (spans inside, empty, covering F,
    t0 < 0, t1 > T, longer than the 256-thread stride, a row in both)"""
    L, _, stream = api()
    R, F, T = case["R"], case["F"], case["T"]
    pattern = torch.randint(-2 ** 31, 2 ** 31 - 1, (R * F * T,), generator=torch.Generator().manual_seed(71), dtype=torch.int64).to(torch.int32)

    def run():
        X = Guarded(R * F * T, what="x")
        X.t.view(torch.int32).copy_(pattern)
        sp = [Guarded(R, torch.int32, k, torch.tensor(case[k], dtype=torch.int32)) for k in ("f0", "f1", "t0", "t1")]
        assert L.rfx_span_mask(X.ptr(), R, F, T, *(s.ptr() for s in sp), stream()) == 0
        torch.cuda.synchronize()
        for s in sp:
            s.unchanged()
        return {"x": X.cpu()}
    got = bits(twice(run)[0]["x"])
    ref = torch.where(E.span_mask(case).reshape(-1), torch.zeros_like(pattern), pattern)
    bad = got != ref
    assert not bool(bad.any()), ("rfx_span_mask", "x", "element", int(bad.nonzero()[0]), "(r, f, t)",
                                 np.unravel_index(int(bad.nonzero()[0]), (R, F, T)), sorted(E.forms_span(case)))


# ---- blstm_frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1, 2, 3))
@pytest.mark.parametrize("case", E.BLSTM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_blstm_frames(case, mode):
    """rfx_blstm_frames: modes 0, 2 (no skip) and 3 bit for bit (zero where tau >= T), mode 2 with skip one rounding, mode 1
    ceil(width / stride) - 1 half-ulps of its terms added in k order; an odd stride, one frame, whole frames of padding"""
    L, _, stream = api()
    B, Cc, T, nfr, width, stride = case
    nx, nh = B * Cc * T, Cc * width * B * nfr
    nsrc, ndst = (nx, nh) if mode in (0, 3) else (nh, nx)
    g = torch.Generator().manual_seed(81 + mode)
    src, skip = torch.randn(nsrc, generator=g), torch.randn(nx, generator=g)
    ratios = []
    for with_skip in ((False, True) if mode == 2 else (False,)):
        def run():
            S, D = Guarded(nsrc, what="src", init=src), Guarded(ndst, what="dst")
            K = Guarded(nx, what="skip", init=skip) if with_skip else None
            assert L.rfx_blstm_frames(S.ptr(), K.ptr() if K else None, D.ptr(), B, Cc, T, nfr, width, stride, mode, stream()) == 0
            torch.cuda.synchronize()
            S.unchanged()
            if K:
                K.unchanged()
            return {"dst": D.cpu()}
        got = twice(run)[0]["dst"]
        ref, mag, _ = E.blstm_frames(src, skip if with_skip else None, case, mode)
        ratios.append(judge(got, ref, E.blstm_bound(case, mode, with_skip, ref, mag),
                            ctx=("rfx_blstm_frames", "dst", "mode", mode, "skip", with_skip, case, sorted(E.forms_blstm(case, mode, with_skip)))))
    report("ELEM", f"blstm_frames {case} mode {mode}", ratios)


# ---- row_moments / row_affine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", (False, True), ids=("nocoef", "coef"))
@pytest.mark.parametrize("shape", E.MOMENT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_moments(shape, coef):
    """rfx_row_moments: 1, 2, 3 slots, R not a multiple of the finalize workgroup's four rows, a row at mean / std = 1e3 and a constant
    row (std == 0 exactly, a == 1 / eps); sums is rfx_row_moments_ws(R, L) doubles, all written.  coef_a / coef_b are judged as
    functions of the fp32 mean / std the kernel stored."""
    L, _, stream = api()
    R, Ln = shape
    x = E.moments_data(R, Ln, 91 + Ln)
    slots = E.moments_slots(Ln)
    nws = int(L.rfx_row_moments_ws(R, Ln))
    assert nws == 2 * R * slots
    info = (shape, sorted(E.forms_moments(R, Ln, coef)))

    def run():
        X, S = Guarded(R * Ln, what="x", init=x), Guarded(nws, torch.float64, "sums")
        M, D, A, Bc = (Guarded(R, what=k) for k in ("mean", "std", "coef_a", "coef_b"))
        assert L.rfx_row_moments(X.ptr(), R, Ln, S.ptr(), M.ptr(), D.ptr(), E.MOMENT_EPS, A.ptr() if coef else None, Bc.ptr() if coef else None,
                                 stream()) == 0
        torch.cuda.synchronize()
        X.unchanged()
        s = S.cpu()
        assert bool(torch.isfinite(s).all()), ("rfx_row_moments", "sums", "slot", int((~torch.isfinite(s)).nonzero()[0]), "not written", info)
        if not coef:
            A.untouched(); Bc.untouched()
            return {"mean": M.cpu(), "std": D.cpu()}
        return {"mean": M.cpu(), "std": D.cpu(), "a": A.cpu(), "b": Bc.cpu()}
    got, _ = twice(run)
    m, sd, bm, bs = E.row_moments(x)
    ratios = [("mean", judge(got["mean"], m, bm, ctx=("rfx_row_moments", "mean", *info))), ("std", judge(got["std"], sd, bs, ctx=("rfx_row_moments", "std", *info)))]
    if R >= 3:
        assert float(got["std"][R - 1]) == 0.0 and float(got["mean"][R - 1]) == 0.75, "the constant row"
    if coef:
        a, b, ba, bb = E.moments_coef(got["mean"], got["std"], E.MOMENT_EPS)
        ratios += [("coef_a", judge(got["a"], a, ba, ctx=("rfx_row_moments", "coef_a", *info))), ("coef_b", judge(got["b"], b, bb, ctx=("rfx_row_moments", "coef_b", *info)))]
        if R >= 3:
            assert float(got["a"][R - 1]) == float(np.float32(1.0) / np.float32(E.MOMENT_EPS))
    report("ELEM", f"row_moments {shape}", ratios)


@pytest.mark.parametrize("with_b", (False, True), ids=("nob", "b"))
@pytest.mark.parametrize("shape", E.AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_affine(shape, with_b):
    """rfx_row_affine: b == NULL bit for bit (one rounded product); with b 2 half-ulps of |x a| + |b| (holds with and without an FMA)"""
    L, _, stream = api()
    R, Ln = shape
    g = torch.Generator().manual_seed(95 + Ln)
    x, a, b = torch.randn(R, Ln, generator=g), torch.randn(R, generator=g) + 2.0, torch.randn(R, generator=g)

    def run():
        X, A, Bc, O = Guarded(R * Ln, what="x", init=x), Guarded(R, what="a", init=a), Guarded(R, what="b", init=b), Guarded(R * Ln, what="out")
        assert L.rfx_row_affine(X.ptr(), A.ptr(), Bc.ptr() if with_b else None, O.ptr(), R, Ln, stream()) == 0
        torch.cuda.synchronize()
        for t in (X, A, Bc):
            t.unchanged()
        return {"out": O.cpu()}
    ref, mag = E.row_affine(x, a, b if with_b else None)
    bound = E.EPS32 * mag if with_b else torch.zeros_like(mag)
    report("ELEM", f"row_affine {shape} b={with_b}", [judge(twice(run)[0]["out"], ref, bound, ctx=("rfx_row_affine", "out", shape, sorted(E.forms_affine(R, Ln, with_b))))])


# ---- dropout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", E.DROPOUT_SEEDS, ids=("seed_small", "seed_above_2_63"))
@pytest.mark.parametrize("p", E.DROPOUT_P)
@pytest.mark.parametrize("n", E.DROPOUT_N)
def test_dropout(n, p, seed):
    """rfx_dropout: the mask and the kept values bit for bit against the integer restatement of the draw (p = 0 keeps everything, times
    exactly 1); a second launch on a gradient with the same seed keeps the same elements"""
    L, _, stream = api()
    x, g = E.signs_data(n, 101 + n), E.signs_data(n, 102 + n)

    def run():
        out = {}
        for k, v in (("x", x), ("g", g)):
            X, O = Guarded(n, what=k, init=v), Guarded(n, what="out")
            assert L.rfx_dropout(X.ptr(), O.ptr(), n, p, seed, stream()) == 0
            torch.cuda.synchronize()
            X.unchanged()
            out[k] = O.cpu()
        return out
    got, _ = twice(run)
    info = ("n", n, "p", p, "seed", hex(seed), sorted(E.forms_dropout(n, p)))
    refx, keep = E.dropout(x, p, seed)
    judge(got["x"], refx, 0.0, ctx=("rfx_dropout", "out", *info))
    judge(got["g"], E.dropout(g, p, seed)[0], 0.0, ctx=("rfx_dropout", "out (gradient)", *info))
    assert torch.equal(got["g"] != 0, keep) and torch.equal(got["x"] != 0, keep)
    if p == 0.0:
        assert torch.equal(bits(got["x"]), bits(x))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    """every argument check of every entry point returns nonzero and writes nothing: NULL pointers, non-positive sizes, L <= 1, one of
    coef_a / coef_b, mode outside 0 - 3, T beyond the frames, p outside [0, 1) and NaN; n == 0 returns 0 and touches nothing"""
    L, _, stream = api()
    bufs = [Guarded(64, what=f"buf{i}") for i in range(6)]
    wsd = Guarded(1024, torch.float64, "ws")
    ints = [Guarded(4, torch.int32, f"int{i}") for i in range(4)]
    p = [b.ptr() for b in bufs]
    ip = [b.ptr() for b in ints]
    w, s, Z = wsd.ptr(), stream(), None
    nan = float("nan")
    refused = {
        "rfx_act_fwd": [lambda: L.rfx_act_fwd(Z, p[1], 8, 2, s), lambda: L.rfx_act_fwd(p[0], Z, 8, 2, s), lambda: L.rfx_act_fwd(p[0], p[1], -1, 2, s),
                        lambda: L.rfx_act_fwd(p[0], p[1], 8, 4, s)],
        "rfx_act_bwd": [lambda: L.rfx_act_bwd(Z, p[1], p[2], 8, 2, s), lambda: L.rfx_act_bwd(p[0], Z, p[2], 8, 2, s),
                        lambda: L.rfx_act_bwd(p[0], p[1], Z, 8, 2, s), lambda: L.rfx_act_bwd(p[0], p[1], p[2], -1, 2, s),
                        lambda: L.rfx_act_bwd(p[0], p[1], p[2], 8, 4, s)],
        "rfx_act_add_fwd": [lambda: L.rfx_act_add_fwd(Z, p[1], p[2], 8, 2, s), lambda: L.rfx_act_add_fwd(p[0], Z, p[2], 8, 2, s),
                            lambda: L.rfx_act_add_fwd(p[0], p[1], Z, 8, 2, s), lambda: L.rfx_act_add_fwd(p[0], p[1], p[2], -1, 2, s),
                            lambda: L.rfx_act_add_fwd(p[0], p[1], p[2], 8, 4, s)],
        "rfx_act_rows": [lambda: L.rfx_act_rows(Z, 0, 0, 8, Z, 0, 0, 0, p[1], 0, 0, 8, 1, 1, 2, 8, 2, s),
                         lambda: L.rfx_act_rows(p[0], 0, 0, 8, Z, 0, 0, 0, Z, 0, 0, 8, 1, 1, 2, 8, 2, s)] +
                        [lambda d=d: L.rfx_act_rows(p[0], 0, 0, 8, Z, 0, 0, 0, p[1], 0, 0, 8, *d, 2, s)
                         for d in ((0, 1, 2, 8), (1, 0, 2, 8), (1, 1, 0, 8), (1, 1, 2, 0))],
        "rfx_act_rows16": [lambda: L.rfx_act_rows16(Z, 0, 0, 8, Z, 0, 0, 0, p[1], 0, 0, 8, 1, 1, 2, 8, 2, s),
                           lambda: L.rfx_act_rows16(p[0], 0, 0, 8, Z, 0, 0, 0, Z, 0, 0, 8, 1, 1, 2, 8, 2, s),
                           lambda: L.rfx_act_rows16(p[0], 0, 0, 8, Z, 0, 0, 0, p[1], 0, 0, 8, 1, 1, 2, 0, 2, s)],
        "rfx_mul": [lambda: L.rfx_mul(Z, p[1], p[2], 8, s), lambda: L.rfx_mul(p[0], Z, p[2], 8, s), lambda: L.rfx_mul(p[0], p[1], Z, 8, s),
                    lambda: L.rfx_mul(p[0], p[1], p[2], -1, s)],
        "rfx_prelu_fwd": [lambda: L.rfx_prelu_fwd(Z, p[1], p[2], 1, 2, 8, s), lambda: L.rfx_prelu_fwd(p[0], Z, p[2], 1, 2, 8, s),
                          lambda: L.rfx_prelu_fwd(p[0], p[1], Z, 1, 2, 8, s)] +
                         [lambda d=d: L.rfx_prelu_fwd(p[0], p[1], p[2], *d, s) for d in ((0, 2, 8), (1, 0, 8), (1, 2, 0))],
        "rfx_prelu_bwd": [lambda i=i: L.rfx_prelu_bwd(*[Z if j == i else q for j, q in enumerate((p[0], p[1], p[2], p[3], w, p[4]))], 1, 2, 8, s)
                          for i in range(6)] +
                         [lambda d=d: L.rfx_prelu_bwd(p[0], p[1], p[2], p[3], w, p[4], *d, s) for d in ((0, 2, 8), (1, 0, 8), (1, 2, 0))],
        "rfx_l1_sum": [lambda: L.rfx_l1_sum(Z, p[1], 8, w, 1.0, p[2], s), lambda: L.rfx_l1_sum(p[0], Z, 8, w, 1.0, p[2], s),
                       lambda: L.rfx_l1_sum(p[0], p[1], 8, Z, 1.0, p[2], s), lambda: L.rfx_l1_sum(p[0], p[1], 8, w, 1.0, Z, s),
                       lambda: L.rfx_l1_sum(p[0], p[1], -1, w, 1.0, p[2], s)],
        "rfx_l1_grad": [lambda: L.rfx_l1_grad(Z, p[1], 8, 1.0, Z, p[2], s), lambda: L.rfx_l1_grad(p[0], Z, 8, 1.0, Z, p[2], s),
                        lambda: L.rfx_l1_grad(p[0], p[1], 8, 1.0, Z, Z, s), lambda: L.rfx_l1_grad(p[0], p[1], 0, 1.0, Z, p[2], s)],
        "rfx_channel_sum": [lambda: L.rfx_channel_sum(Z, 1, 2, 2, 4, 16, 8, 4, 1, w, p[1], s),
                            lambda: L.rfx_channel_sum(p[0], 1, 2, 2, 4, 16, 8, 4, 1, Z, p[1], s),
                            lambda: L.rfx_channel_sum(p[0], 1, 2, 2, 4, 16, 8, 4, 1, w, Z, s)] +
                           [lambda d=d: L.rfx_channel_sum(p[0], *d, 16, 8, 4, 1, w, p[1], s) for d in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0))] +
                           [lambda d=d: L.rfx_channel_sum_ws(p[0], *d, 16, 8, 4, 1) for d in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0))],
        "rfx_add_bcast": [lambda: L.rfx_add_bcast(Z, p[1], p[2], 1, 2, 2, 4, 16, 8, 4, 1, 1.0, s),
                          lambda: L.rfx_add_bcast(p[0], Z, p[2], 1, 2, 2, 4, 16, 8, 4, 1, 1.0, s),
                          lambda: L.rfx_add_bcast(p[0], p[1], Z, 1, 2, 2, 4, 16, 8, 4, 1, 1.0, s)] +
                         [lambda d=d: L.rfx_add_bcast(p[0], p[1], p[2], *d, 16, 8, 4, 1, 1.0, s) for d in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0))],
        "rfx_span_mask": [lambda i=i: L.rfx_span_mask(*[Z if j == i else q for j, q in enumerate((p[0], 1, 2, 8, *ip))][:8], s) for i in (0, 4, 5, 6, 7)] +
                         [lambda d=d: L.rfx_span_mask(p[0], *d, *ip, s) for d in ((0, 2, 8), (1, 0, 8), (1, 2, 0))],
        "rfx_blstm_frames": [lambda: L.rfx_blstm_frames(Z, Z, p[1], 1, 1, 8, 2, 4, 4, 0, s), lambda: L.rfx_blstm_frames(p[0], Z, Z, 1, 1, 8, 2, 4, 4, 0, s)] +
                            [lambda d=d: L.rfx_blstm_frames(p[0], Z, p[1], *d, s)
                             for d in ((0, 1, 8, 2, 4, 4, 0), (1, 0, 8, 2, 4, 4, 0), (1, 1, 0, 2, 4, 4, 0), (1, 1, 8, 0, 4, 4, 0), (1, 1, 8, 2, 0, 4, 0),
                                       (1, 1, 8, 2, 4, 0, 0), (1, 1, 8, 2, 4, 4, -1), (1, 1, 8, 2, 4, 4, 4),
                                       (1, 1, 9, 2, 4, 4, 0), (1, 1, 9, 2, 4, 4, 1), (1, 1, 9, 2, 4, 4, 2), (1, 1, 9, 2, 4, 4, 3))],   # T > (nfr - 1) stride + width
        "rfx_row_moments": [lambda i=i: L.rfx_row_moments(*[Z if j == i else q for j, q in enumerate((p[0], 2, 8, w, p[1], p[2], 1e-5, p[3], p[4]))], s)
                            for i in (0, 3, 4, 5, 7, 8)] +
                           [lambda: L.rfx_row_moments(p[0], 0, 8, w, p[1], p[2], 1e-5, p[3], p[4], s), lambda: L.rfx_row_moments(p[0], 2, 1, w, p[1], p[2], 1e-5, p[3], p[4], s),
                            lambda: L.rfx_row_moments(p[0], 2, 0, w, p[1], p[2], 1e-5, Z, Z, s)],
        "rfx_row_affine": [lambda: L.rfx_row_affine(Z, p[1], p[2], p[3], 2, 8, s), lambda: L.rfx_row_affine(p[0], Z, p[2], p[3], 2, 8, s),
                           lambda: L.rfx_row_affine(p[0], p[1], p[2], Z, 2, 8, s), lambda: L.rfx_row_affine(p[0], p[1], p[2], p[3], 0, 8, s),
                           lambda: L.rfx_row_affine(p[0], p[1], p[2], p[3], 2, 0, s)],
        "rfx_dropout": [lambda: L.rfx_dropout(Z, p[1], 8, 0.5, 1, s), lambda: L.rfx_dropout(p[0], Z, 8, 0.5, 1, s), lambda: L.rfx_dropout(p[0], p[1], -1, 0.5, 1, s)] +
                       [lambda q=q: L.rfx_dropout(p[0], p[1], 8, q, 1, s) for q in (-0.1, 1.0, 1.5, nan, float("inf"))],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            assert call() != 0, (name, "refusal", i, "was accepted")
    zero = {"rfx_act_fwd": lambda: L.rfx_act_fwd(p[0], p[1], 0, 2, s), "rfx_act_bwd": lambda: L.rfx_act_bwd(p[0], p[1], p[2], 0, 2, s),
            "rfx_act_add_fwd": lambda: L.rfx_act_add_fwd(p[0], p[1], p[2], 0, 2, s), "rfx_mul": lambda: L.rfx_mul(p[0], p[1], p[2], 0, s),
            "rfx_dropout": lambda: L.rfx_dropout(p[0], p[1], 0, 0.5, 1, s)}
    for name, call in zero.items():
        assert call() == 0, (name, "n == 0")
    torch.cuda.synchronize()
    for b in bufs + [wsd] + ints:
        b.untouched()


# ---- rfx_zero ------------------------------------------------------------------------------------------------------------------------
def _zero(nbytes, byte_off, words):
    """rfx_zero on `nbytes` at `byte_off` bytes into a NaN-filled guarded payload of `words` fp32 -> (return code, the buffer)"""
    L, _, stream = api()
    Z = Guarded(words, what="p")
    rc = L.rfx_zero(ctypes.c_void_p(Z.t.data_ptr() + byte_off), nbytes, stream())
    torch.cuda.synchronize()
    return rc, Z


def _zero_check(nbytes, byte_off):
    forms = E.forms_zero(nbytes, byte_off)
    pad = 8                                                    # payload words that stay NaN on either side of the zeroed run
    lo = byte_off // 4
    words = lo + -(-nbytes // 4) + pad
    rc, Z = _zero(nbytes, byte_off, words)
    if forms is None:
        assert rc != 0, ("rfx_zero accepted", nbytes, "bytes at byte offset", byte_off)
        Z.untouched()
        return
    assert rc == 0, ("rfx_zero", rc, nbytes, byte_off, sorted(forms))
    Z.guards_intact()
    b = bits(Z.t)
    n = nbytes // 4
    assert bool((b[lo:lo + n] == 0).all()), ("rfx_zero", nbytes, byte_off, sorted(forms), "a word of the run is not zero")
    keep = torch.cat([b[:lo], b[lo + n:]])
    assert bool((keep == Z.fill).all()), ("rfx_zero", nbytes, byte_off, sorted(forms), "wrote outside its run")


@pytest.mark.parametrize("nbytes", E.ZERO_BYTES)
def test_zero(nbytes):
    """every byte count at bases 0 - 3 words past a 16-byte boundary (head of 0, 3, 2, 1 words) and at two odd byte offsets: a multiple of 4
    at a 4-byte base becomes all-zero bits and nothing around it changes; anything else is refused and nothing is written"""
    for off in [4 * w for w in E.ZERO_WORD_OFFSETS] + [1, 6]:
        _zero_check(nbytes, off)
    report("ELEM", f"rfx_zero nbytes={nbytes}", [] if nbytes % 4 else [0.0])


def test_zero_past_the_grid_cap():
    """one workgroup more than the 16384 of the cap would hold, from a base one word past a 16-byte boundary: head, body, tail"""
    assert E.forms_zero(E.ZERO_BYTES_CAP, 4) == {"head", "vec", "tail", "second_iteration", "grid_capped"}
    _zero_check(E.ZERO_BYTES_CAP, 4)
    L, _, stream = api()
    assert L.rfx_zero(None, 16, stream()) != 0 and L.rfx_zero(None, 0, stream()) == 0
    Z = Guarded(8, what="p")
    assert L.rfx_zero(Z.ptr(), -4, stream()) != 0
    torch.cuda.synchronize()
    Z.untouched()
    report("ELEM", "rfx_zero cap", [0.0])
