"""Every instantiation of the LSTM recurrence (remfx_amd/csrc/lstm.hip) through the C ABI -- rfx_lstm_pack, rfx_lstm_pack_local,
rfx_lstm_fwd, rfx_lstm_bwd with `prec` passed explicitly -- against tests/lstm_ref.py, the fp64 restatement with the SAME operand
rounding, at a bound derived from that reference's own noise floor (lstm_ref.floors: 8 x floor + 16 fp32 half-ulps; what the bound
can and cannot see is tests/test_lstm_ref_cpu.py).  Kernel and reference get the same fp32 xp, weights and gout; the backward sweep
of both gets the KERNEL's saved gates / cstate, so the two sweeps are judged separately.

The case table follows the dispatch of rfx_lstm_fwd / rfx_lstm_bwd: `forms` below mirrors it (and is checked against rfx_lstm_local),
test_case_table_reaches_every_form counts what the table reaches.  tests/test_gpu_lstm.py stays the module-level test (projection
GEMM, weight gradients, torch.nn.LSTM as the reference, whole-mode bounds); the loose assertions here use its bounds."""
import ctypes as C
import functools

import pytest
import torch

from tests import lstm_ref as R
from tests.conftest import check
from tests.kernel_harness import Guarded, stop_after_a_device_error  # noqa: F401

pytestmark = pytest.mark.gpu

F32, BF16X3, BF16 = 0, 1, 2
MODE = {BF16X3: "bf16x3", BF16: "bf16"}
CLUSTER = (0, 0)                                               # rfx_lstm_set_local: never the single-workgroup form

# (H, T, Bn, pin) -- pin = None: the form as shipped
SHAPES = (
    [(H, 5, 33, None) for H in (32, 64)]                       # generic forms, one trip of the ring (the old suite's widths)
    + [(H, 5, 33, None) for H in (96, 160)]                    # fwd<2,0> ring wrap (nks = 6, 10), bwd<1,0> with 3 and 5 rounds
    + [(H, 5, 33, None) for H in (128, 512)]                   # fwd<4,0> ring wrap (nks = 8, 32), bwd<2,0> with 2 and 8 rounds
    + [(H, T, 5, None) for H in (96, 128) for T in (1, 2, 3)]  # no exchange, first use of each ping-pong buffer, start clamps
    + [(H, 4, 33, None) for H in (256, 384)]                   # compile-time forms
    + [(192, 6, Bn, None) for Bn in (1, 15, 16, 17, 31, 32, 33, 64, 65)]   # every tile edge of both forms and the switch
    + [(192, 6, Bn, CLUSTER) for Bn in (16, 17, 64, 65)]       # bf16 cluster form at the same edges
    + [(192, 200, 3, None), (192, 200, 3, CLUSTER)]            # one clip's layer-4 frame
    + [(192, T, 3, pin) for T in (1, 2) for pin in (None, CLUSTER)]
)
CASES = [(H, T, Bn, pin, prec) for H, T, Bn, pin in SHAPES for prec in (BF16, BF16X3) if pin is None or prec == BF16]


def _id(c):
    H, T, Bn, pin, prec = c
    return f"H{H}-T{T}-Bn{Bn}-{MODE[prec]}" + ("-cluster" if pin else "")


def forms(H, prec, Bn, pin):
    """(forward, backward) instantiation rfx_lstm_fwd / rfx_lstm_bwd launch, with the trips of the weight ring per time step"""
    lo = "false" if prec == BF16 else "true"
    lf, lb = (pin if pin is not None else (64, 16))
    if prec == BF16 and H == 192 and Bn <= lf:
        fwd = ("fwd_local<12>", 1)
    else:
        D, NKS = {192: (12, 12), 256: (16, 16) if prec == BF16 else (4, 16), 384: (24, 24) if prec == BF16 else (4, 24)}.get(
            H, (4 if H % 64 == 0 else 2, 0))
        fwd = (f"fwd<{D},{NKS},{lo}>", (H // 16) // D)
    if prec == BF16 and H == 192 and Bn <= (lb if lf > 0 else 0):
        bwd = ("bwd_local<12>", 1)
    else:
        res = {192: (3, 6), 256: (4, 8), 384: (4, 12)} if prec == BF16 else {192: (3, 6)}
        TPC, NWC = res.get(H, (2 if (H // 32) % 2 == 0 else 1, 0))
        bwd = (f"bwd<{TPC},{NWC},{lo},{'true' if NWC else 'false'}>", 1 if NWC else (H // 32) // TPC)
    return fwd, bwd


def test_case_table_reaches_every_form():
    fwd, bwd = {}, {}
    for H, T, Bn, pin, prec in CASES:
        f, b = forms(H, prec, Bn, pin)
        fwd.setdefault(f[0], set()).add(f[1])
        bwd.setdefault(b[0], set()).add(b[1])
    assert set(fwd) == {"fwd_local<12>", "fwd<12,12,false>", "fwd<16,16,false>", "fwd<24,24,false>", "fwd<4,0,false>", "fwd<2,0,false>",
                        "fwd<12,12,true>", "fwd<4,16,true>", "fwd<4,24,true>", "fwd<4,0,true>", "fwd<2,0,true>"}
    assert set(bwd) == {"bwd_local<12>", "bwd<3,6,false,true>", "bwd<4,8,false,true>", "bwd<4,12,false,true>", "bwd<2,0,false,false>",
                        "bwd<1,0,false,false>", "bwd<3,6,true,true>", "bwd<2,0,true,false>", "bwd<1,0,true,false>"}
    for name, trips in list(fwd.items()) + list(bwd.items()):
        if ",0," in name:                                      # runtime trip count: one trip of the ring, and several
            assert 1 in trips and max(trips) > 1, (name, trips)


@pytest.fixture(autouse=True)
def _no_spin_timed_out():
    yield
    from remfx_amd import lstm
    assert not lstm.error_flag()


class _Pin:
    def __init__(self, pin):
        self.pin = pin

    def __enter__(self):
        from remfx_amd import _lib
        if self.pin is not None:
            _lib.lib().rfx_lstm_set_local(*self.pin)

    def __exit__(self, *exc):
        from remfx_amd import _lib
        _lib.lib().rfx_lstm_set_local(-1, -1)


def launch(H, T, Bn, prec, inputs, pin=None, save=True, sweep_back=True):
    """one forward (and backward) sweep on the current stream; returns CPU tensors"""
    from remfx_amd import _lib, lstm
    from remfx_amd._lib import check as rc
    from remfx_amd.ops import _ptr, _stream
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    xp, w0, w1, gout = (t.to(dev).contiguous() for t in inputs)
    nb = L.rfx_lstm_pack_bytes(H)
    assert nb > 0
    pack = torch.zeros(2 * nb, device=dev, dtype=torch.uint8)
    for d, w in enumerate((w0, w1)):
        dst = C.c_void_p(pack.data_ptr() + d * nb)
        rc(L.rfx_lstm_pack(_ptr(w), H, dst, _stream()), "rfx_lstm_pack")
        rc(L.rfx_lstm_pack_local(_ptr(w), H, dst, _stream()), "rfx_lstm_pack_local")
    ws = lstm._workspace(dev, H)
    P = T * Bn
    res = {}
    with _Pin(pin):
        f, b = forms(H, prec, Bn, pin)
        assert L.rfx_lstm_local(H, Bn, prec, 0) == int(f[0].startswith("fwd_local"))     # the mirror of the dispatch holds
        assert L.rfx_lstm_local(H, Bn, prec, 1) == int(b[0].startswith("bwd_local"))
        ob = Guarded(2 * H * P, what="out")
        gb, cb = (Guarded(8 * H * P, what="gates"), Guarded(2 * H * P, what="cstate")) if save else (None, None)
        out, gates, cst = ob.t, (gb.t if save else None), (cb.t if save else None)
        rc(L.rfx_lstm_fwd(_ptr(xp), _ptr(pack), T, Bn, H, _ptr(out), _ptr(gates), _ptr(cst), _ptr(ws), prec, _stream()), "rfx_lstm_fwd")
        ob.owned()
        res["out"] = out.cpu().view(2 * H, P)
        if save:
            gb.owned()
            cb.owned()
            res["gates"], res["cstate"] = gates.cpu().view(2, 4 * H, P), cst.cpu().view(2, H, P)
            if sweep_back:
                db = Guarded(8 * H * P, what="dG")
                dG = db.t
                rc(L.rfx_lstm_bwd(_ptr(gout), _ptr(pack), _ptr(gates), _ptr(cst), T, Bn, H, _ptr(dG), _ptr(ws), prec, _stream()),
                   "rfx_lstm_bwd")
                db.owned()
                res["dG"] = dG.cpu().view(2, 4 * H, P)
    return res


def references(H, T, Bn, prec, inputs, got, loose=True):
    """operand-rounded reference + floors of both sweeps (the backward from the kernel's saved state), and the exact reference"""
    xp, w0, w1, gout = inputs
    mode = MODE[prec]
    ref, fl = R.floors(R.forward_case(xp, w0, w1, T, Bn, mode), mode, H, "out")
    refb, flb = R.floors(R.backward_case(gout, got["gates"], got["cstate"], w0, w1, T, Bn, mode), mode, H, "dG")
    ref.update(refb)
    fl.update(flb)
    exact = None
    if loose:
        exact = R.forward_case(xp, w0, w1, T, Bn, "exact")(0.0, False)
        exact.update(R.backward_case(gout, got["gates"], got["cstate"], w0, w1, T, Bn, "exact")(0.0, False))
    return ref, fl, exact


@functools.lru_cache(maxsize=None)
def _case(H, T, Bn, pin, prec):
    inputs = R.make_inputs(H, T, Bn)
    got = launch(H, T, Bn, prec, inputs, pin)
    return inputs, got, references(H, T, Bn, prec, inputs, got)


def tight(H, prec, Bn, pin, names, got, ref, fl):
    """relative L2 and max-abs per tensor and direction against the operand-rounded reference, at 8 x floor + 16 fp32 half-ulps"""
    f, b = forms(H, prec, Bn, pin)
    for name in names:
        form = (b if name == "dG" else f)[0]
        for (label, g), (_, r) in zip(R.per_direction(name, got[name], H), R.per_direction(name, ref[name], H)):
            for kind, e, floor in zip(("l2", "max"), R.errors(g, r), fl[label]):
                check(e, R.bound(floor), what=f"tight|{form}|{label}|{kind}|floor={R.bound(floor) / R.MARGIN:.3e}")


def _loose_bound(f32, prec):
    """the bounds of tests/test_gpu_lstm.py; bf16: the default of conftest.tol"""
    return f32 if prec != BF16 else min(0.25, max(2e-2, 100.0 * f32))


def _dwhh(dG, out, H, T, Bn):
    """dW_hh of both directions by plain matmuls: gate gradients times h of the step before in the processing order"""
    r = []
    for d in range(2):
        h, g = out[d * H:(d + 1) * H].double().view(H, T, Bn), dG[d].double().view(4 * H, T, Bn)
        hp, gs = (h[:, :-1], g[:, 1:]) if d == 0 else (h[:, 1:], g[:, :-1])
        r.append(gs.reshape(4 * H, -1) @ hp.reshape(H, -1).t())
    return torch.stack(r)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward(case):
    H, T, Bn, pin, prec = case
    inputs, got, (ref, fl, exact) = _case(*case)
    tight(H, prec, Bn, pin, ("out", "gates", "cstate"), got, ref, fl)
    for name in ("out", "gates", "cstate"):
        check(R.errors(got[name], exact[name])[0], _loose_bound(1e-4, prec), what=f"loose|{name}")
    # inference (no saved state) writes the same out, bit for bit
    assert torch.equal(launch(H, T, Bn, prec, inputs, pin, save=False)["out"], got["out"])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward(case):
    H, T, Bn, pin, prec = case
    inputs, got, (ref, fl, exact) = _case(*case)
    tight(H, prec, Bn, pin, ("dG",), got, ref, fl)
    check(R.errors(got["dG"], exact["dG"])[0], _loose_bound(2e-4, prec), what="loose|dG")
    if T > 1:
        check(R.errors(_dwhh(got["dG"], got["out"], H, T, Bn), _dwhh(exact["dG"], exact["out"], H, T, Bn))[0], _loose_bound(3e-4, prec),
              what="loose|dW_hh")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_repeat_after_interference(case):
    """The case, then another (T, Bn) of the same H on the same stream -- it reuses the workspace, the exchange buffers and the arrival
    counters -- then the case again: bit for bit the same (the kernels sum in a fixed order)."""
    H, T, Bn, pin, prec = case
    inputs = R.make_inputs(H, T, Bn)
    first = launch(H, T, Bn, prec, inputs, pin)
    T2, Bn2 = T % 3 + 2, (40 if Bn != 40 else 12)
    launch(H, T2, Bn2, prec, R.make_inputs(H, T2, Bn2, seed=1), pin)
    again = launch(H, T, Bn, prec, inputs, pin)
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_f32_mode_is_the_bf16x3_recurrence():
    """prec = RFX_PREC_F32 runs the bf16x3 split (include/remfx_hip.h: any value but RFX_PREC_BF16)"""
    H, T, Bn = 96, 5, 33
    inputs, got, _ = _case(H, T, Bn, None, BF16X3)
    other = launch(H, T, Bn, F32, inputs)
    for k in got:
        assert torch.equal(got[k], other[k]), k


@pytest.mark.parametrize("H,T,Bn,pin,prec", [(96, 3, 17, None, BF16), (96, 3, 17, None, BF16X3), (192, 6, 17, None, BF16),
                                             (192, 6, 17, CLUSTER, BF16), (192, 6, 17, None, BF16X3)])
def test_directions_are_the_same_recurrence(H, T, Bn, pin, prec):
    """Direction 1 fed direction 0's weights and direction 0's inputs reversed in time computes direction 0's result reversed in time,
    bit for bit: the reverse indexing (t = T - 1 - s, prefetch of the next step, the start clamps) at a ragged sequence tile."""
    xp, w0, _, gout = R.make_inputs(H, T, Bn)
    flip = lambda t, c: t.view(c, T, Bn).flip(1).reshape(c, T * Bn)                      # noqa: E731
    xp = torch.stack([xp[0], flip(xp[0], 4 * H)])
    gout = torch.cat([gout[:H], flip(gout[:H], H)])
    got = launch(H, T, Bn, prec, (xp, w0, w0, gout), pin)
    assert torch.equal(flip(got["out"][H:], H), got["out"][:H])
    for k, c in (("gates", 4 * H), ("cstate", H), ("dG", 4 * H)):
        assert torch.equal(flip(got[k][1], c), got[k][0]), k


@pytest.mark.parametrize("prec", [BF16, BF16X3], ids=lambda p: MODE[p])
def test_saturated_gates(prec):
    """A quarter of the units carry +-30 on one gate's input projection (each gate in turn, both signs): exp runs into its overflow /
    underflow ranges, the gate is 0, 1 or -1 to the last fp32 bit.  Everything stays finite and inside the tight bound, and the
    gradient of a saturated gate's pre-activation is tiny, not NaN."""
    H, T, Bn = 128, 4, 5
    xp, w0, w1, gout = R.make_inputs(H, T, Bn)
    xp = xp.clone().view(2, 4, H, T * Bn)
    for u in range(H // 4):
        xp[:, u // 8, u] += 30.0 if u % 8 < 4 else -30.0
    inputs = (xp.view(2, 4 * H, T * Bn), w0, w1, gout)
    got = launch(H, T, Bn, prec, inputs)                                                 # finiteness: launch() checks every element
    ref, fl, _ = references(H, T, Bn, prec, inputs, got, loose=False)
    tight(H, prec, Bn, None, ("out", "gates", "cstate", "dG"), got, ref, fl)
    sat = got["gates"].view(2, 4, H, -1)
    dG = got["dG"].view(2, 4, H, -1)
    for u in range(H // 4):
        g = u // 8
        s = sat[:, g, u]
        assert bool(((s.abs() < 1e-9) | ((s.abs() - 1).abs() < 1e-6)).all()), (g, u)
        assert float(dG[:, g, u].abs().max()) < 1e-8, (g, u)


@pytest.mark.parametrize("prec", [BF16, BF16X3], ids=lambda p: MODE[p])
def test_ring_wrap_form_over_several_launches(prec):
    """More sequence tiles than one co-resident launch holds, on a form whose weight ring wraps (H = 96): chunked launches that reuse
    the counters and exchange buffers, against the tight reference."""
    H, T, Bn = 96, 2, 8200
    inputs = R.make_inputs(H, T, Bn)
    got = launch(H, T, Bn, prec, inputs)
    ref, fl, _ = references(H, T, Bn, prec, inputs, got, loose=False)
    tight(H, prec, Bn, None, ("out", "gates", "cstate", "dG"), got, ref, fl)


# ---- the parameter glue: rfx_lstm_cat_params, rfx_lstm_grad_scatter ---------------------------------------------------
from tests.kernel_harness import api, judge, report, twice  # noqa: E402


def _glue_inputs(p):
    return {k: Guarded(v.numel(), what=k, init=v) for k, v in p.items()}


@pytest.mark.one_mode
@pytest.mark.parametrize("H,Cin", R.GLUE_CASES)
def test_cat_params(H, Cin):
    """wcat = the two weight blocks bit for bit, bcat = [b_ih + b_hh ; b_ih_r + b_hh_r] rounded once; the six inputs come back unchanged"""
    L, _, stream = api()
    p, _, _ = R.glue_data(H, Cin)
    ref = R.cat_params(p)
    info = ("rfx_lstm_cat_params", (H, Cin), sorted(R.forms_glue(H, Cin)))

    def run():
        I = _glue_inputs(p)
        W, B = Guarded(8 * H * Cin, what="wcat"), Guarded(8 * H, what="bcat")
        rc = L.rfx_lstm_cat_params(*(I[k].ptr() for k in R.GLUE_PARAMS), H, Cin, W.ptr(), B.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, *info)
        for b in I.values():
            b.unchanged()
        W.owned()
        B.owned()
        return {"wcat": W.cpu(), "bcat": B.cpu()}
    got = twice(run)[0]
    report("LSTM", f"rfx_lstm_cat_params H={H} Cin={Cin}", {k: judge(got[k], ref[k], 0, ctx=(*info, k)) for k in ("wcat", "bcat")})


@pytest.mark.one_mode
@pytest.mark.parametrize("H,Cin", R.GLUE_CASES)
def test_grad_scatter(H, Cin):
    """six gradient buffers that start from distinct non-zero contents end at g + d rounded once, both biases of a direction with the same
    addend; dwcat / dbcat unchanged; a second call accumulates again"""
    L, _, stream = api()
    _, d, g0 = R.glue_data(H, Cin)
    once = R.grad_scatter(g0, d)
    second = R.grad_scatter({k: v.float() for k, v in once.items()}, d)
    info = ("rfx_lstm_grad_scatter", (H, Cin), sorted(R.forms_glue(H, Cin)))

    def run():
        D = _glue_inputs(d)
        G = {k: Guarded(g0[k].numel(), what="g_" + k, init=g0[k]) for k in R.GLUE_PARAMS}
        out = {}
        for call in ("first", "second"):
            rc = L.rfx_lstm_grad_scatter(D["dwcat"].ptr(), D["dbcat"].ptr(), H, Cin, *(G[k].ptr() for k in R.GLUE_PARAMS), stream())
            torch.cuda.synchronize()
            assert rc == 0, (rc, call, *info)
            for b in D.values():
                b.unchanged()
            for k in R.GLUE_PARAMS:
                G[k].owned()
                out[f"{call} {k}"] = G[k].cpu().clone()
        return out
    got = twice(run)[0]
    ratios = [(call, judge(got[f"{call} {k}"], ref[k], 0, ctx=(*info, call, k))) for call, ref in (("first", once), ("second", second))
              for k in R.GLUE_PARAMS]
    report("LSTM", f"rfx_lstm_grad_scatter H={H} Cin={Cin}", ratios)


@pytest.mark.one_mode
def test_glue_refusals_write_nothing():
    """each NULL pointer, H = 0 and Cin = 0: nonzero, and neither an output nor a gradient is touched"""
    L, _, stream = api()
    H, Cin = 3, 5
    p, d, g0 = R.glue_data(H, Cin)
    I, D = _glue_inputs(p), _glue_inputs(d)
    W, B = Guarded(8 * H * Cin, what="wcat"), Guarded(8 * H, what="bcat")
    G = {k: Guarded(g0[k].numel(), what="g_" + k, init=g0[k]) for k in R.GLUE_PARAMS}
    cat = [I[k].ptr() for k in R.GLUE_PARAMS] + [H, Cin, W.ptr(), B.ptr()]
    sc = [D["dwcat"].ptr(), D["dbcat"].ptr(), H, Cin] + [G[k].ptr() for k in R.GLUE_PARAMS]
    bad_cat = [cat[:i] + [None] + cat[i + 1:] for i in (0, 1, 2, 3, 4, 5, 8, 9)] + [cat[:6] + [0, Cin] + cat[8:], cat[:6] + [H, 0] + cat[8:]]
    bad_sc = [sc[:i] + [None] + sc[i + 1:] for i in (0, 1, 4, 5, 6, 7, 8, 9)] + [sc[:2] + [0, Cin] + sc[4:], sc[:2] + [H, 0] + sc[4:]]
    assert R.forms_glue(0, Cin) is None and R.forms_glue(H, 0) is None
    for a in bad_cat:
        assert L.rfx_lstm_cat_params(*a, stream()) != 0, a
    for a in bad_sc:
        assert L.rfx_lstm_grad_scatter(*a, stream()) != 0, a
    torch.cuda.synchronize()
    W.untouched()
    B.untouched()
    for b in list(I.values()) + list(D.values()) + list(G.values()):
        b.unchanged()
    report("LSTM", "glue refusals", [])
