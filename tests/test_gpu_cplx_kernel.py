"""Every kernel form of remfx_amd/csrc/cplx.hip through the C ABI -- rfx_cplx_moments, rfx_cplx_coef_fwd / _bwd, rfx_cplx_affine_act_fwd /
_bwd, rfx_cplx_moments_bwd, rfx_bound_mask_fwd / _bwd, rfx_phase_mask_fwd / _bwd -- on buffers this test allocates, against
tests/cplx_ref.py: the fp64 restatement, every kernel fed fixed fp32 inputs (or the device's own fp32 statistics) so that each is judged
alone, PER ELEMENT, at

    |got - ref| <= (8 x floor + 16 fp32 half-ulps) x eps32 x magnitude     (+ the leaky-ReLU sign slack)

with magnitude = sum of |terms| the element was formed from and floor = the error of a CPU float32 restatement with the kernels'
partial sums, in the same units (cplx_ref.floors_*; never measured on the kernel).  The walk of the case tables over the dispatch, the
1e-3 cap on every bound and the 1e-4 cap on the sign band are in tests/test_cplx_ref_cpu.py; floors and findings in DESIGN.md 4.20.

Buffers: every output is NaN-filled between two NaN guards of 4096 elements; `ws` has exactly the size rfx_cplx_moments_ws / rfx_cplx_affine_act_bwd_ws answer, is
NaN-filled and followed by a guard (every slot has to be written: it comes back finite).  A sliced output is a channel slice of a wider
NaN-filled buffer whose neighbouring channels must keep their bits; a sliced gy is read from one (a read outside the slice returns NaN).
Every case runs twice into fresh buffers: plain slot stores and ordered sums, the same bits."""
import functools

import pytest
import torch

from tests import cplx_ref as R
from tests.kernel_harness import Guarded, api, bits, judge, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]          # no GEMM inside: the arithmetic modes agree

EPS = R.GEN_EPS
_judge = functools.partial(judge, exact="value")                        # bound 0: the error is 0, -0 == +0


class _Sliced:
    """(N, 2C, S) as the channels [Cx, Cx + 2C) of a NaN-filled (N, 2C + 2Cx, S) buffer between guards"""

    def __init__(self, N, C, S, Cx, what, init=None):
        self.b = Guarded(N * (2 * C + 2 * Cx) * S, what=what)
        self.wide = self.b.t.view(N, 2 * C + 2 * Cx, S)
        self.t = self.wide[:, Cx:Cx + 2 * C]
        self.ns, self.Cx, self.C = (2 * C + 2 * Cx) * S, Cx, C
        if init is not None:
            self.t.copy_(init)

    def owned(self):
        self.b.guards_intact()
        nb = bits(torch.cat([self.wide[:, :self.Cx], self.wide[:, self.Cx + 2 * self.C:]], 1))
        assert bool((nb == self.b.fill).all()), f"{self.b.what}: a neighbouring channel of the slice was written"
        bad = ~torch.isfinite(self.t)
        assert not bool(bad.any()), f"{self.b.what}: element {tuple(bad.nonzero()[0].tolist())} of the slice not written or not finite"


# ---- the four streaming kernels ---------------------------------------------------------------------------------------------------------
def launch_stream(case, inp, coef, cm):
    L, _ptr, _stream = api()
    N, C, S = case.N, case.C, case.S
    x, coef_d, cm_d = inp["x"].cuda(), coef.cuda().contiguous(), cm.cuda().contiguous()
    nws, nws2 = int(L.rfx_cplx_moments_ws(N, C, S)), int(L.rfx_cplx_affine_act_bwd_ws(N, C, S))
    assert (nws, nws2) == (R.moments_ws(N, C, S), R.affine_bwd_ws(N, C, S)) == (5 * C * R.slots(N, S), 6 * C * R.slots(N, S))
    got = {}
    ws = Guarded(nws, torch.float64, front=False, what="moments ws")
    sums = Guarded(5 * C, torch.float64, what="sums")
    assert L.rfx_cplx_moments(_ptr(x), N, C, S, _ptr(ws.t), _ptr(sums.t), _stream()) == 0
    torch.cuda.synchronize()
    ws.owned(); sums.owned()
    got["sums"], got["moments_ws"] = sums.t.view(C, 5).cpu(), ws.t.cpu()
    if case.sliced:
        y = _Sliced(N, C, S, case.Cx, "y")
        gy = _Sliced(N, C, S, case.Cx, "gy", init=inp["gy"].cuda())
        y_ns, gy_ns = y.ns, gy.ns
    else:
        y = Guarded(N * 2 * C * S, what="y")
        gy = Guarded(N * 2 * C * S, what="gy", init=inp["gy"].cuda())
        y_ns = gy_ns = 2 * C * S
    assert L.rfx_cplx_affine_act_fwd(_ptr(x), _ptr(coef_d), N, C, S, R.SLOPE, _ptr(y.t), y_ns, C, _stream()) == 0
    torch.cuda.synchronize()
    y.owned()
    got["y"] = y.t.reshape(N, 2 * C, S).cpu()
    gx = Guarded(N * 2 * C * S, what="gx")
    ws2 = Guarded(nws2, torch.float64, front=False, what="affine_act_bwd ws")
    gcoef = Guarded(6 * C, what="gcoef")
    gy_bits = gy.b.buf.clone() if case.sliced else gy.buf.clone()
    assert L.rfx_cplx_affine_act_bwd(_ptr(x), _ptr(coef_d), _ptr(gy.t), gy_ns, C, N, C, S, R.SLOPE, _ptr(gx.t), _ptr(ws2.t), _ptr(gcoef.t),
                                     _stream()) == 0
    torch.cuda.synchronize()
    gx.owned(); ws2.owned(); gcoef.owned()
    assert torch.equal((gy.b.buf if case.sliced else gy.buf).view(torch.int32), gy_bits.view(torch.int32)), "gy was written"
    got["gx"], got["gcoef"] = gx.t.view(N, 2 * C, S).cpu(), gcoef.t.view(6, C).cpu()
    gx2 = Guarded(N * 2 * C * S, what="gx (moments_bwd)", init=inp["gx0"].cuda())
    assert L.rfx_cplx_moments_bwd(_ptr(x), _ptr(cm_d), N, C, S, _ptr(gx2.t), _stream()) == 0
    torch.cuda.synchronize()
    gx2.owned()
    got["gx2"] = gx2.t.view(N, 2 * C, S).cpu()
    return got


ENTRY = {"sums": "rfx_cplx_moments", "y": "rfx_cplx_affine_act_fwd", "gx": "rfx_cplx_affine_act_bwd", "gcoef": "rfx_cplx_affine_act_bwd",
         "gx2": "rfx_cplx_moments_bwd"}


@pytest.mark.parametrize("case", R.stream_cases(), ids=lambda c: c.id)
def test_streaming_kernels(case):
    """moments, affine + leaky ReLU forward and backward, moments backward at every S of the chunk / lane / thread edges, C in {1, 3, 65},
    N in {1, 3}, six data classes, contiguous and sliced"""
    inp = R.make_inputs(case)
    coef, cm = R.stream_intermediates(case, inp)
    got = launch_stream(case, inp, coef, cm)
    ref, mag, slack, fl = R.floors_stream(case, inp, coef.double(), cm.double())
    for name in ref:
        _judge(got[name], ref[name], R.tolerance(name, mag, slack, fl), ctx=(ENTRY[name], case.id, name, "floor", fl[name], case.forms()))
    again = launch_stream(case, inp, coef, cm)
    for k in got:
        assert torch.equal(got[k], again[k]), (case.id, k, "second run differs")


# ---- coefficient kernels ------------------------------------------------------------------------------------------------------------------
def launch_coef(ci, C, train):
    L, _ptr, _stream = api()
    d = lambda t, dt=torch.float32: t.to(dt).contiguous().cuda()              # noqa: E731
    W, B = [d(w) for w in ci["W"]], [d(b) for b in ci["B"]]
    wp = [_ptr(t) for t in W + B]
    coef = Guarded(6 * C, what="coef")
    gw = Guarded(5 * C, what="gw")
    gcoef = d(ci["gcoef"])
    got = {}
    if train:
        sums = d(ci["sums"], torch.float64)
        stats = Guarded(5 * C, what="stats_out")
        run = [Guarded(C, what=f"running[{q}]", init=ci["running"][q].cuda()) for q in range(5)]
        assert L.rfx_cplx_coef_fwd(_ptr(sums), ci["inv"], None, *wp, EPS, C, _ptr(coef.t), _ptr(stats.t), *[_ptr(r.t) for r in run],
                                   R.MOMENTUM, _stream()) == 0
        cm = Guarded(5 * C, what="cm")
        assert L.rfx_cplx_coef_bwd(_ptr(sums), ci["inv"], None, *wp, EPS, C, _ptr(gcoef), _ptr(gw.t), _ptr(cm.t), _stream()) == 0
        torch.cuda.synchronize()
        for b in [coef, stats, gw, cm] + run:
            b.owned()
        got.update(stats=stats.t.view(5, C).cpu(), running=torch.stack([r.t for r in run]).cpu(), cm=cm.t.view(5, C).cpu())
    else:
        st_in = d(ci["running"])
        assert L.rfx_cplx_coef_fwd(None, 0.0, _ptr(st_in), *wp, EPS, C, _ptr(coef.t), None, None, None, None, None, None, 0.0, _stream()) == 0
        assert L.rfx_cplx_coef_bwd(None, 0.0, _ptr(st_in), *wp, EPS, C, _ptr(gcoef), _ptr(gw.t), None, _stream()) == 0
        torch.cuda.synchronize()
        coef.owned(); gw.owned()
    got.update(coef=coef.t.view(6, C).cpu(), gw=gw.t.view(5, C).cpu())
    return got


@pytest.mark.parametrize("C", R.COEF_C)
@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
def test_coefficient_kernels(C, train):
    """rfx_cplx_coef_fwd / _bwd alone: fp64 sums the test computed (training: statistics, all five running buffers, stats_out, cm) or
    stats_in with NULL running pointers and cm == NULL (eval); one, two (one lane in the second) and three workgroups; channel c holds
    data class c % 6.  stats_out is judged against the fp64 statistics; coef, gw and cm as functions of the fp32 statistics the kernel
    stored, with the condition-aware magnitude of cplx_ref.coef_mag"""
    ci = R.coef_inputs(C)
    got = launch_coef(ci, C, train)
    cid = f"C={C} {'train' if train else 'eval'} {R.coef_forms(C, train)}"
    st32 = got["stats"] if train else None
    ref, mag, fl = R.floors_coef(ci, train)
    if train:
        _judge(got["stats"], ref["stats"], R.k_of(fl["stats"]) * R.EPS32 * mag["stats"], ctx=("rfx_cplx_coef_fwd", cid, "stats_out", fl))
        ref, mag, _ = R.floors_coef(ci, train, st32=st32)                        # the floors stay the CPU's
        _judge(got["running"], ref["running"], R.k_of(fl["running"]) * R.EPS32 * mag["running"], ctx=("rfx_cplx_coef_fwd", cid, "running", fl))
    _judge(got["coef"], ref["coef"], R.k_of(fl["coef"]) * R.EPS32 * mag["coef"], ctx=("rfx_cplx_coef_fwd", cid, "coef", fl))
    st = st32.double() if train else ci["running"].float().double()
    gw, cm = R.coef_bwd(st, ci["W"], R.f32(EPS), ci["gcoef"], ci["inv"] if train else None, v32=True)
    k = R.k_of(0.5)                                               # fp64 inside: what is left is the rounding of the result
    _judge(got["gw"], gw, k * R.EPS32 * R.coef_bwd_mag(gw), ctx=("rfx_cplx_coef_bwd", cid, "gw"))
    if train:
        _judge(got["cm"], cm, k * R.EPS32 * R.coef_bwd_mag(cm), ctx=("rfx_cplx_coef_bwd", cid, "cm"))
    again = launch_coef(ci, C, train)
    for name in got:
        assert torch.equal(got[name], again[name]), (cid, name, "second run differs")


def test_coefficient_argument_guards():
    """both or neither of sums / stats_in, and a partial set of running pointers, are refused without a launch"""
    L, _ptr, _stream = api()
    C = 3
    f = lambda n, dt=torch.float32: torch.ones(n, device="cuda", dtype=dt)       # noqa: E731
    w = [_ptr(f(C)) for _ in range(5)]
    sums, st, coef, gc, gw = f(5 * C, torch.float64), f(5 * C), Guarded(6 * C, what="coef"), f(6 * C), Guarded(5 * C, what="gw")
    run = [f(C) for _ in range(5)]
    none5 = [None] * 5
    assert L.rfx_cplx_coef_fwd(_ptr(sums), 0.5, _ptr(st), *w, EPS, C, _ptr(coef.t), None, *none5, 0.1, _stream()) != 0
    assert L.rfx_cplx_coef_fwd(None, 0.5, None, *w, EPS, C, _ptr(coef.t), None, *none5, 0.1, _stream()) != 0
    for missing in range(5):
        rp = [None if q == missing else _ptr(run[q]) for q in range(5)]
        assert L.rfx_cplx_coef_fwd(_ptr(sums), 0.5, None, *w, EPS, C, _ptr(coef.t), None, *rp, 0.1, _stream()) != 0, missing
    rp = [_ptr(run[0])] + [None] * 4
    assert L.rfx_cplx_coef_fwd(_ptr(sums), 0.5, None, *w, EPS, C, _ptr(coef.t), None, *rp, 0.1, _stream()) != 0
    assert L.rfx_cplx_coef_bwd(_ptr(sums), 0.5, _ptr(st), *w, EPS, C, _ptr(gc), _ptr(gw.t), None, _stream()) != 0
    assert L.rfx_cplx_coef_bwd(None, 0.5, None, *w, EPS, C, _ptr(gc), _ptr(gw.t), None, _stream()) != 0
    torch.cuda.synchronize()
    coef.untouched(); gw.untouched()                             # a refused call writes nothing


# ---- masks --------------------------------------------------------------------------------------------------------------------------------
def launch_bound_mask(bi, N, P):
    L, _ptr, _stream = api()
    m, g = bi["m"].cuda().contiguous(), bi["g"].cuda().contiguous()
    tf_ns = 2 * P + 5                                             # the product passes tf.stride(0) of a wider tensor
    tfb = torch.full((N, tf_ns), float("nan"), device="cuda")
    tfb[:, :2 * P] = bi["tf"].reshape(N, 2 * P).cuda()
    out, gm = Guarded(N * 2 * P, what="out"), Guarded(N * 2 * P, what="gm")
    assert L.rfx_bound_mask_fwd(_ptr(m), _ptr(tfb), _ptr(out.t), N, P, 2 * P, tf_ns, 2 * P, _stream()) == 0
    assert L.rfx_bound_mask_bwd(_ptr(m), _ptr(tfb), _ptr(g), _ptr(gm.t), N, P, 2 * P, tf_ns, 2 * P, 2 * P, _stream()) == 0
    torch.cuda.synchronize()
    out.owned(); gm.owned()
    return {"out": out.t.view(N, 2, P).cpu(), "gm": gm.t.view(N, 2, P).cpu()}


@pytest.mark.parametrize("NP", R.BOUND_MASK_CASES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_bound_mask(NP):
    """tanh(|m|) m / |m| (*) tf and its backward: one element, a partial workgroup, several, and 4.2 M elements (cx_grid's cap crossed:
    five grid-stride iterations); tf at a sample stride above 2 P.  Half of every sample has |m| in [1e-4, 20], the other half in
    [1e-30, 1e-4] with values on the axes: finite, out -> m tf, gm -> g conj(tf) (the fp64 reference)"""
    N, P = NP
    bi = R.bound_mask_inputs(N, P)
    got = launch_bound_mask(bi, N, P)
    ref, mag, fl = R.floors_bound_mask(bi)
    for name, entry in (("out", "rfx_bound_mask_fwd"), ("gm", "rfx_bound_mask_bwd")):
        q = _judge(got[name], ref[name], R.k_of(fl[name]) * R.EPS32 * mag[name], ctx=(entry, f"{N}x{P}", name, "floor", fl[name]))
        print(f"\nBOUNDMASK {N}x{P} {name}: worst error / bound {q:.3f}, CPU float32 floor {fl[name]:.2f}")
    again = launch_bound_mask(bi, N, P)
    for k in got:
        assert torch.equal(got[k], again[k]), (NP, k, "second run differs")


def test_bound_mask_at_zero():
    """m = 0 is outside the pinned domain (the reference is 0 / 0); the kernels return the limits: out = 0, gm = g conj(tf)"""
    bi = {"m": torch.zeros(1, 2, 3), "tf": torch.tensor([[[1.0, -2.0, 0.5], [0.25, 3.0, -1.0]]]), "g": torch.tensor([[[0.5, 1.0, -1.0], [2.0, -0.5, 0.25]]])}
    got = launch_bound_mask(bi, 1, 3)
    t, g = bi["tf"][0], bi["g"][0]
    assert torch.equal(got["out"], torch.zeros(1, 2, 3))
    assert torch.equal(got["gm"][0], torch.stack([g[0] * t[0] + g[1] * t[1], -g[0] * t[1] + g[1] * t[0]]))


def launch_phase_mask(pi, n):
    L, _ptr, _stream = api()
    xc, mg, g = pi["xc"].cuda(), pi["mag"].cuda(), pi["g"].cuda().contiguous()
    out, gmag = Guarded(2 * n, what="out"), Guarded(n, what="gmag")
    assert L.rfx_phase_mask_fwd(_ptr(mg), _ptr(xc), _ptr(out.t), n, _stream()) == 0
    assert L.rfx_phase_mask_bwd(_ptr(xc), _ptr(g), _ptr(gmag.t), n, _stream()) == 0
    torch.cuda.synchronize()
    out.owned(); gmag.owned()
    return {"out": out.t.view(n, 2).cpu(), "gmag": gmag.t.cpu()}


@pytest.mark.parametrize("n", R.PHASE_MASK_N)
def test_phase_mask(n):
    """mag exp(i atan2(im, re)) and its backward, |x| log-uniform in [1e-30, 1e4], x on the axes, negative mag; exact zeros give
    (mag, 0) and gmag = g.re bit for bit; one element, a partial workgroup, the grid cap crossed"""
    pi = R.phase_mask_inputs(n)
    got = launch_phase_mask(pi, n)
    ref, mag, fl = R.floors_phase_mask(pi)
    for name, entry in (("out", "rfx_phase_mask_fwd"), ("gmag", "rfx_phase_mask_bwd")):
        q = _judge(got[name], ref[name], R.k_of(fl[name]) * R.EPS32 * mag[name], ctx=(entry, n, name, "floor", fl[name]))
        print(f"\nPHASEMASK {n} {name}: worst error / bound {q:.3f}, CPU float32 floor {fl[name]:.2f}")
    z = (pi["xc"] == 0).all(1)
    if bool(z.any()):
        assert torch.equal(got["out"][z], torch.stack([pi["mag"][z], torch.zeros(int(z.sum()))], 1))
        assert torch.equal(got["gmag"][z], pi["g"][z, 0])
    again = launch_phase_mask(pi, n)
    for k in got:
        assert torch.equal(got[k], again[k]), (n, k, "second run differs")
