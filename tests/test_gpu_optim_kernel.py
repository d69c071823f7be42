"""rfx_sumsq, rfx_clip_coef and rfx_adamw_step of remfx_amd/csrc/optim.hip through the C ABI on buffers this test allocates, against
tests/optim_ref.py (fp64), per element.  The bounds and where their constants come from are in optim_ref's docstring and DESIGN.md 4.20;
none is measured on the kernel.  n = 4 194 304 + 1027 crosses gridn's cap of 4096 workgroups (a fifth grid-stride iteration for a quarter
of the threads) with an n % 4 tail of 3; n = 4096 x 1024 + 1 is exactly one workgroup past the cap of rfx_sumsq's own slot count.

Buffers: p, g, m, v sit between NaN guards of 4096 elements; `ws` is NaN-filled, rfx_sumsq_ws(n) doubles plus a guard; g has to come back
bit for bit.  Every case runs twice into fresh buffers: the same bits."""
import math

import pytest
import torch

from tests import optim_ref as O
from tests.kernel_harness import Guarded, api, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]


def _grad(n, seed):
    """mixed scales 1e-4 ... 1e3 (log-uniform per element), random sign; the last three (the n % 4 tail) at 5e2 ... 1e3"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * math.log(1e7) + math.log(1e-4))
    mag[max(n - 3, 0):] = 1e3 * (0.5 + 0.5 * torch.rand(min(n, 3), generator=g, dtype=torch.float64))
    return (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()


def _sumsq(gcpu):
    L, _ptr, _stream = api()
    n = gcpu.numel()
    g = Guarded(max(n, 1), what="g", init=gcpu if n else None)
    nws = int(L.rfx_sumsq_ws(n))
    assert nws == O.SLOTS                                        # the library's size against the restated cap: the same for every n
    ws = Guarded(nws, torch.float64, what="ws")
    out = Guarded(1, torch.float64, what="out")
    assert L.rfx_sumsq(_ptr(g.t), n, _ptr(ws.t), _ptr(out.t), _stream()) == 0
    torch.cuda.synchronize()
    out.owned(); ws.guards_intact()
    g.unchanged()
    slots = ws.t.cpu()
    used = O.forms(n)["slots"]
    assert bool(torch.isfinite(slots[:used]).all()) and bool(torch.isnan(slots[used:]).all()), ("slots written", used)
    return float(out.t.cpu()), slots


SUMSQ_N = O.SUMSQ_N + (O.SLOTS * 1024 + 1,)                     # + the first n that needs more workgroups than there are slots


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq(n):
    """the float4 body, the n % 4 tail, one / two / 4096 workgroups and the multi-slot sum; n = 0 writes 0 and no slot.
    |err| <= 4 x 2^-53 x (additions on the longest path) x sum g^2: the products of two floats are exact in fp64, every addition rounds
    once (optim_ref.sumsq_bound counts them from the decomposition)"""
    g = _grad(n, 100 + n)
    got, slots = _sumsq(g)
    ref = O.sumsq(g)
    bound = O.sumsq_bound(n, ref)
    print(f"\nSUMSQ n={n}: rel err {abs(got - ref) / max(ref, 1e-300):.2e}, bound {bound / max(ref, 1e-300):.2e}, {O.forms(n)}")
    assert abs(got - ref) <= bound, ("rfx_sumsq", n, got, ref, bound, O.forms(n))
    if n:
        # every element is in the sum: leaving the last one out moves it by more than the bound
        assert float(g[-1].double() ** 2) > bound
    again, slots2 = _sumsq(g)
    assert again == got and torch.equal(slots.nan_to_num(-1.0), slots2.nan_to_num(-1.0))


@pytest.mark.parametrize("form", ("above", "below", "max_norm_0", "no_norm_out"))
def test_clip_coef(form):
    """norm above max_norm (coef = max_norm / (norm pre + 1e-6) pre), below it (pre), max_norm == 0 with pre = 0.25 (exactly pre), and
    norm_out == NULL: 16 fp32 half-ulps of the result (sqrt, two products, a sum, a quotient)"""
    L, _ptr, _stream = api()
    total, max_norm, pre = {"above": (1e4, 10.0, 0.5), "below": (400.0, 10.0, 0.25), "max_norm_0": (1e4, 0.0, 0.25),
                            "no_norm_out": (1e4, 10.0, 1.0)}[form]
    ss = torch.tensor([total], device="cuda", dtype=torch.float64)
    coef, norm = Guarded(1, what="coef"), Guarded(1, what="norm")
    assert L.rfx_clip_coef(_ptr(ss), max_norm, pre, _ptr(coef.t), None if form == "no_norm_out" else _ptr(norm.t), _stream()) == 0
    torch.cuda.synchronize()
    coef.owned()
    rc, rn = O.clip_coef(total, max_norm, pre)
    c = float(coef.t.cpu())
    assert abs(c - rc) <= 8 * O.EPS32 * rc, ("rfx_clip_coef", form, c, rc)
    if form in ("below", "max_norm_0"):
        assert c == pre
    if form == "above":
        assert c < pre
    if form == "no_norm_out":
        norm.untouched()                                         # norm_out == NULL: nothing is written
    else:
        norm.owned()
        assert abs(float(norm.t.cpu()) - rn) <= 8 * O.EPS32 * rn


def _adamw(state, n, lr, step, gscale):
    L, _ptr, _stream = api()
    b1, b2 = O.HYPER["betas"]
    bufs = {k: Guarded(n, what=k, init=state[k]) for k in ("p", "g", "m", "v")}
    gs = torch.tensor([gscale], device="cuda") if gscale is not None else None
    out = []
    for s in (step, step + 1):                                   # two consecutive steps on the same buffers: m, v are read back
        assert L.rfx_adamw_step(_ptr(bufs["p"].t), _ptr(bufs["g"].t), _ptr(bufs["m"].t), _ptr(bufs["v"].t), n, lr, b1, b2, O.HYPER["eps"],
                                O.HYPER["wd"], s, _ptr(gs), _stream()) == 0
        torch.cuda.synchronize()
        for b in bufs.values():
            b.owned()
        bufs["g"].unchanged()
        out.append({k: bufs[k].t.cpu() for k in ("p", "m", "v")})
    return out


@pytest.mark.parametrize("gscale", (None, 0.37), ids=("noscale", "gscale"))
@pytest.mark.parametrize("lr", (1e-4, 1e-2))
@pytest.mark.parametrize("step", (1, 2, 1000))
@pytest.mark.parametrize("n", O.ADAMW_N)
def test_adamw_step(n, step, lr, gscale):
    """p, m, v per element against fp64 after each of two consecutive steps (the second from the fp32 state the first left), with the
    project's hyper-parameters as the floats the ABI carries.  Bounds: optim_ref.adamw_bounds (m, v: 2 half-ulps of their terms; p:
    2 half-ulps of |p| + K eps32 |update| + m's bound carried through; K from the float values of the betas)"""
    g = torch.Generator().manual_seed(7 * n + step)
    state = {"p": torch.randn(n, generator=g), "g": torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g)),
             "m": torch.randn(n, generator=g) * 0.1, "v": torch.rand(n, generator=g) * 0.1 + 1e-8}
    got = _adamw(state, n, lr, step, gscale)
    b1, b2 = (O.f32(b) for b in O.HYPER["betas"])
    hp = (O.f32(lr), b1, b2, O.f32(O.HYPER["eps"]), O.f32(O.HYPER["wd"]))
    gs = 1.0 if gscale is None else O.f32(gscale)
    cur = dict(state)
    for i, s in enumerate((step, step + 1)):
        ref = dict(zip("pmv", O.adamw_step(cur["p"], cur["g"], cur["m"], cur["v"], *hp, s, gs)))
        bound = O.adamw_bounds(cur["p"], cur["g"], cur["m"], cur["v"], *hp, s, gs)
        for k in "mvp":
            e = (got[i][k].double() - ref[k]).abs()
            q = e / bound[k].clamp_min(1e-300)
            j = int(q.argmax())
            assert float(q[j]) <= 1.0, ("rfx_adamw_step", k, "element", j, "of", n, "step", s, "error / bound", float(q[j]), "got", float(got[i][k][j]),
                                        "ref", float(ref[k][j]), "K", O.adamw_k(b1, b2, s), O.forms(n))
        cur = {"p": got[i]["p"], "g": state["g"], "m": got[i]["m"], "v": got[i]["v"]}
    if lr == 1e-2 and gscale is None:
        again = _adamw(state, n, lr, step, gscale)
        for i in range(2):
            for k in "pmv":
                assert torch.equal(got[i][k], again[i][k]), (k, "second run differs")


def test_adamw_argument_guards():
    """step < 1 is refused; n == 0 returns 0 and touches nothing"""
    L, _ptr, _stream = api()
    bufs = [Guarded(8, what=k) for k in "pgmv"]
    ptrs = [_ptr(b.t) for b in bufs]
    assert L.rfx_adamw_step(*ptrs, 8, 1e-4, 0.95, 0.999, 1e-6, 1e-3, 0, None, _stream()) != 0
    assert L.rfx_adamw_step(*ptrs, 8, 1e-4, 0.95, 0.999, 1e-6, 1e-3, -3, None, _stream()) != 0
    assert L.rfx_adamw_step(*ptrs, 0, 1e-4, 0.95, 0.999, 1e-6, 1e-3, 1, None, _stream()) == 0
    torch.cuda.synchronize()
    for b in bufs:
        b.untouched()
