"""Every layer-op autograd node of remfx_amd/ops.py and remfx_amd/nnops.py at its seams, per element: the case table
and the variant runner of tests/node_ref.py on the device.  V0 anchors a case against its fp64 reference by the bound of the launched
entry's kernel test; V1 .. V6 move one host decision each -- operand layout, which gradients are asked for, the incoming gradient's
layout, no_grad, the parameter-gradient sink, a second use in one step -- and compare with the anchor by bits (by value where a zeroed
buffer is added to, by the anchor's bound where a launch accumulates in an order of its own)."""
import ast
import contextlib
import os

import pytest
import torch

from tests import node_ref as R
from tests.conftest import mode
from tests.kernel_harness import bits, judge, report, same_bits, stop_after_a_device_error  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("side", "main", "off")
ONE_MODE = [c for c in R.case_table() if not c.gemm]
GEMM = [c for c in R.case_table() if c.gemm]


def _sync():
    torch.cuda.synchronize()


@contextlib.contextmanager
def arm(route, tensors):
    """the parameters in an optim.FlatParams buffer with the sink armed as tests/test_gpu_gradsink.py's `armed` does it (GradSink.MODE =
    route); on exit the buffer is joined, so .grad can be read"""
    from remfx_amd import ops, optim
    prev = ops.GradSink.MODE
    ops.GradSink.MODE = route
    try:
        ps = {k: torch.nn.Parameter(v.to(DEV)) for k, v in tensors.items()}
        flat = optim.FlatParams(list(ps.values()))
        flat.zero_grad()
        assert (ops.SINK is not None) == (route != "off")
        try:
            yield ps
        finally:
            flat.join()
            torch.cuda.synchronize()
    finally:
        ops.GradSink.MODE = prev
    assert ops.SINK is None


@pytest.fixture
def launches():
    """the entry points called while the fixture is live, in order: [(name, arguments)]; the library's symbols are put back after"""
    from remfx_amd import _lib
    L = _lib.lib()
    log, orig = [], {}
    for name in _lib.SIGNATURES:
        fn = getattr(L, name)
        orig[name] = fn
        setattr(L, name, lambda *a, _fn=fn, _n=name: (log.append((_n, a)), _fn(*a))[1])
    try:
        yield log
    finally:
        for name, fn in orig.items():
            setattr(L, name, fn)


def _is_launch(name):
    from remfx_amd import _lib
    import ctypes as C
    a = _lib.SIGNATURES[name]
    return len(a) >= 2 and a[-1] is C.c_void_p


def _variants(case, m):
    from remfx_amd import nnops
    inp, anchor, ratios = R.v0(case, DEV, m, sync=_sync)
    if case.ref is None:
        print(f"\nNODE {case.id} V0: no per-element bound -- {case.note}")
    else:
        report("NODE", case.id, ratios, "V0")
    failed = []
    for v in case.variants:
        if (v == "V3" and not case.diff) or (v in ("V5", "V6") and not case.params):
            continue
        try:                                              # every variant runs: one verdict names all that failed
            if v in ("V5", "V6"):
                r = getattr(R, v.lower())(case, DEV, m, inp, anchor, arm, ROUTES, sync=_sync)
            else:
                r = getattr(R, v.lower())(case, DEV, m, inp, anchor, sync=_sync)
            if v == "V3" and len(anchor.outs) > 1 and all(anchor.requires):
                r.update(R.v3_independent(case, DEV, m, inp, anchor, sync=_sync))
        except AssertionError as e:
            failed.append((v, e.args))
            continue
        if r:
            report("NODE", case.id, r, v)
    assert not failed, failed
    assert not nnops.INTERIM, nnops.INTERIM


@pytest.mark.one_mode
@pytest.mark.parametrize("case", ONE_MODE, ids=lambda c: c.id)
def test_node(case):
    _variants(case, "f32")


@pytest.mark.parametrize("case", GEMM, ids=lambda c: c.id)
def test_gemm_node(case):
    _variants(case, mode())


@pytest.mark.one_mode
@pytest.mark.parametrize("case", R.dconv_cases(), ids=lambda c: c.id)
def test_dconv_node(case, bf16_mode, launches):
    """_DConvLayerFn, (3, 48, 256), both backward forms: the variants against its own anchor run, the entries it launches, and V4 with the
    caller's grad mode passed -- under no_grad the forward gets null h16 / z16 / a_out / stats: nothing is stored for a backward"""
    _variants(case, "bf16")
    del launches[:]
    inp = case.make(0)
    R.run(case, inp, DEV, sync=_sync)
    got = sorted({n for n, _ in launches if _is_launch(n)})
    assert got == R.expected(case, "bf16"), (case.id, got, R.expected(case, "bf16"))
    del launches[:]
    R.run(case, inp, DEV, no_grad=True, sync=_sync)
    (args,) = [a for n, a in launches if n == "rfx_dconv_layer_fwd"]
    assert not any(args[16:20]), ("stored for a backward under no_grad", args[16:20])
    del launches[:]
    R.run(case, inp, DEV, sync=_sync)
    (args,) = [a for n, a in launches if n == "rfx_dconv_layer_fwd"]
    assert all(args[16:20]) == (not case.loose), "h16 / z16 / a_out / stats: stored for the layer-by-layer backward only"


# ---- which entries a case launches ------------------------------------------------------------------------------------------------------
def _literals():
    """the string literals passed as first argument to launch / launch_rc / query / scratch in ops.py and nnops.py"""
    out = set()
    for f in ("ops.py", "nnops.py"):
        tree = ast.parse(open(os.path.join(ROOT, "remfx_amd", f)).read())
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and getattr(n.func, "id", getattr(n.func, "attr", None)) in ("launch", "launch_rc", "query", "scratch", "scratch_size") and n.args:
                for c in ast.walk(n.args[0]):
                    if isinstance(c, ast.Constant) and isinstance(c.value, str):
                        out.add(c.value)
    return out


# entries of ops.py / nnops.py that no V0 of the table reaches, and why
UNREACHED = {
    "rfx_dconv_layer_fwd": "bf16 mode, its own shape: test_dconv_node runs the cases of node_ref.dconv_cases() under the recorder",
    "rfx_dconv_layer_bwd": "as rfx_dconv_layer_fwd", "rfx_dconv_layer_bwd_ws": "as rfx_dconv_layer_fwd",
    "rfx_dconv_layer_ok": "asked by dconv_layer_fused_ok, the caller's routing question (test_gpu_hdemucs_route.py), not by the node",
    "rfx_unpack_add_bias": "written through the armed sink only: V5 / V6 of the conv cases, not V0",
    "rfx_gemm_fwd_variant": "behind ops.TRACE_VARIANT, the measurement hook of bench.py",
    "rfx_gemm_wgrad_variant": "behind ops.TRACE_WGRAD, a hook of the kernel tests",
}
ONLY_IN = {"rfx_glu_bwd_bf16": "bf16", "rfx_localstate_mfma_ok": "bf16", "rfx_localstate_mfma_fwd": "bf16", "rfx_localstate_mfma_bwd": "bf16"}     # reached in that mode only


def test_v0_launches_what_the_table_says_and_the_tables_cover_the_wrappers(launches):
    """V0 of every case under the recorder: each case launches EXPECT's entries (forward then backward), and the union over the table is
    every entry ops.py and nnops.py name in a launch / launch_rc / query / scratch call, but the ones UNREACHED gives a reason for.  Run in every
    GEMM mode: the mode moves the entries of the GLU and attention nodes."""
    from remfx_amd import nnops
    m = mode()
    seen, bad = set(), []
    for case in R.case_table():
        del launches[:]
        R.run(case, case.make(0), DEV, sync=_sync)
        names = [n for n, _ in launches]
        seen.update(names)
        got = [n for n in names if _is_launch(n)]
        got = sorted(set(got)) if case.gemm else sorted(got)
        if got != R.expected(case, m):
            bad.append((case.id, m, "launched", got, "the table says", R.expected(case, m)))
    assert not bad, bad
    lit = _literals()
    missing = {n for n in lit - seen if n not in UNREACHED and ONLY_IN.get(n, m) == m}
    assert not missing, ("entries of ops.py / nnops.py no case reaches and UNREACHED does not name", sorted(missing))
    stale = {n for n in UNREACHED if n in seen}
    assert not stale, ("UNREACHED names entries the table reaches", sorted(stale))
    assert not nnops.INTERIM


def test_no_grad_attention_allocates_no_weights(launches):
    """V4 of _LocalStateFn: under no_grad the resident kernel gets a null `w`"""
    case = R.by_id("localstate-resident")
    R.run(case, case.make(0), DEV, no_grad=True, sync=_sync)
    calls = [a for n, a in launches if n == "rfx_localstate_fwd"]
    assert len(calls) == 1 and not calls[0][9], "w allocated under no_grad"
    del launches[:]
    R.run(case, case.make(0), DEV, sync=_sync)
    assert [bool(a[9]) for n, a in launches if n == "rfx_localstate_fwd"] == [True]


# ---- wrappers that return their input, the eval forward ------------------------------------------------------------------------------------
@pytest.mark.one_mode
def test_wrappers_that_do_nothing_return_their_input(launches):
    from remfx_amd import nnops
    x = torch.randn(2, 3, 5, 7, device=DEV)
    assert nnops.avg_pool2d(x, (1, 1)) is x and nnops.dropout(x, 0.0, True) is x and nnops.dropout(x, 0.3, False) is x
    assert [n for n, _ in launches] == []


@pytest.mark.one_mode
@pytest.mark.parametrize("relu", (False, True))
def test_batchnorm_eval_forward(relu, launches):
    """running statistics, forward only: norm_ref's apply fed rsqrt(var + eps) as the node forms it (one torch op, one rounding)"""
    from remfx_amd import nnops
    from tests import norm_ref as NR
    case = R.by_id("batchnorm-train-none")
    inp = case.make(0)
    t = {k: v.to(DEV) for k, v in inp.items()}
    rm, rv = t["rm"].clone(), t["rv"].clone()
    y = nnops.batch_norm(t["x"], R._BN(t), False, relu=relu)
    torch.cuda.synchronize()
    assert torch.equal(t["rm"], rm) and torch.equal(t["rv"], rv)
    N, C = inp["x"].shape[:2]
    rstd = torch.rsqrt(t["rv"] + R.GN_EPS).cpu()                    # the expression of the node, on the device: the rstd the kernel was given
    c = NR.Case("node", "bn", N, C, 35, C, "relu" if relu else "none", bwd=False, eval=True)
    ni = {"x": inp["x"].reshape(N, C, 35), "gamma": inp["gamma"], "beta": inp["beta"], "res": None, "scale": None, "gy": None, "idx": None}
    ref, mag, slack, fl = NR.floors(ni, inp["rm"].double(), rstd.double(), c)
    r = judge(y.reshape(N, C, 35), ref["y"], NR.tolerance("y", ref, mag, slack, fl))
    report("NODE", "batchnorm-eval", {"y": r}, "relu" if relu else "none")
    yy = nnops.batch_norm(t["x"].clone().requires_grad_(True), R._BN(t), False, relu=relu)
    torch.cuda.synchronize()
    del launches[:]
    with pytest.raises(ValueError):                   # V8: the eval-mode backward is refused before any launch
        nnops._BatchNormFn.backward(yy.grad_fn, torch.ones_like(yy))
    assert [n for n, _ in launches] == []


@pytest.mark.parametrize("cid", ["fork-tap-16to24-3x3", "fork-merged-16to24-k8s4", "fork-phase-12to7-5x3"])
def test_fork_alias_unused(cid):
    """V2 of ConvFork2dFn: with the alias output left out of the backward the gradients are those of a zero residual, by value (the
    engine hands the node zeros, and x + 0 may turn -0 into +0)"""
    import dataclasses
    case = R.by_id(cid)
    inp = case.make(0)
    used = R.run(case, inp, DEV, sync=_sync)
    zero = R.run(case, inp, DEV, gys=[used.gys[0], torch.zeros_like(used.gys[1])], sync=_sync)
    first = dataclasses.replace(case, call=lambda t: case.call(t)[0])
    unused = R.run(first, inp, DEV, gys=[used.gys[0]], sync=_sync)
    for k in case.diff:
        assert torch.equal(unused.grads[k], zero.grads[k]), (cid, k)
    r = R.verdict(case, inp, zero, mode(), names={"d_x", "d_w", "d_b"})
    report("NODE", cid, r, "alias unused")


# ---- V7: the 16-bit and statistics hand-offs of bf16 mode ------------------------------------------------------------------------------------
@pytest.fixture
def bf16_mode():
    from remfx_amd import ops
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16")
    yield
    ops.set_gemm_precision(prev)


def _v7_inputs(shape_x, shape_w, C):
    g = torch.Generator().manual_seed(77)
    r = lambda s, k=1.0: torch.randn(*s, generator=g) * k            # noqa: E731
    cpu = {"x": r(shape_x), "w": r(shape_w, 1.0 / 48 ** 0.5), "b": r((C,), 2.0), "gamma": r((C,), 3.0), "beta": r((C,), 0.2)}
    return cpu, {k: v.to(DEV).requires_grad_(True) for k, v in cpu.items()}


def _judge_all(what, got, refs, exact="bits"):
    return {k: judge(got[k], refs[k][0], refs[k][1], exact=exact, ctx=(what, k)) for k in got}


@pytest.mark.one_mode
@pytest.mark.parametrize("tail", ["group_norm-gelu", "group_norm-glu", "activation", "activation_to"])
def test_v7_out_bf16_hand_off(tail, bf16_mode, launches):
    """conv2d(out_bf16=True) -> group_norm / activation / activation_to in bf16 mode: the conv output and the gradient that comes back
    for it are STORED in 16 bits (the use16 condition of conv2d_forward holds: Cout 24 > 8, OA OB = 56, no activation), the consumer is
    the 16-bit entry, and every stage is judged per element from the values the stage before it stored: the conv by gemm_ref with the
    16-bit store, the consumer by norm_ref's / elem_ref's 16-bit storage bound, the conv backward by gemm_ref fed the stored gradient.
    With ops.BF16_STORE off the same call stores fp32."""
    from remfx_amd import nnops, ops
    from tests import elem_ref as E
    cpu, t = _v7_inputs((2, 16, 2, 30), (24, 16, 1, 3), 24)
    one, zero = (1, 1), (0, 0)
    y = ops.conv2d(t["x"], t["w"], t["b"], one, zero, one, out_bf16=True)
    y.retain_grad()
    assert y.dtype == torch.bfloat16 and y.shape == (2, 24, 2, 28)
    stats = {}
    if tail.startswith("group_norm"):
        gmode = tail.split("-")[1]
        u = nnops.group_norm(y, 2, t["gamma"], t["beta"], R.GN_EPS, gmode)
        stats = {"mean": u.grad_fn.saved_tensors[3].cpu(), "rstd": u.grad_fn.saved_tensors[4].cpu()}
        entry, twin = "rfx_groupnorm_fwd_x16", "rfx_groupnorm_fwd"
    elif tail == "activation":
        u, entry, twin = ops.activation(y, "gelu"), "rfx_act_rows16", "rfx_act_fwd"
    else:
        u, entry, twin = ops.activation_to(y, "gelu", (0, 2, 1)), "rfx_act_rows16", "rfx_act_rows"
    assert u.dtype == torch.float32
    gy = torch.randn(u.shape, generator=torch.Generator().manual_seed(78)) * 0.75
    u.backward(gy.to(DEV))
    torch.cuda.synchronize()
    names = [n for n, _ in launches]
    assert entry in names and twin not in names, (tail, names)
    assert y.grad.dtype == torch.bfloat16, "the gradient of a 16-bit conv output is stored in 16 bits"
    ys, gs = y.detach().cpu(), y.grad.cpu()
    ratios = {}
    # the conv forward, stored in 16 bits
    r = R._gemm_refs("conv", "bf16", None, cpu["x"], cpu["w"], cpu["b"], None, one, zero, one, {"y": "y"}, out16=True)
    ratios.update({"conv " + k: v for k, v in _judge_all(tail, {"y": ys}, r).items()})
    # the consumer, from the stored y
    if tail.startswith("group_norm"):
        got = dict(stats, y=u.detach().cpu(), d_x=gs, d_gamma=t["gamma"].grad.cpu(), d_beta=t["beta"].grad.cpu())
        refs = R._norm_refs({"x": ys, "gamma": cpu["gamma"], "beta": cpu["beta"]}, [gy], got, "gn", 2, gmode, True, True)
        ratios.update(_judge_all(tail, got, refs, exact="value"))
    else:
        got = {"y": u.detach().cpu(), "d_x": gs}
        ratios.update(_judge_all(tail, got, R._act_refs({"x": ys}, [gy], E.GELU, True)))
    # the conv backward, from the stored gradient
    got = {"d_x": t["x"].grad.cpu(), "d_w": t["w"].grad.cpu(), "d_b": t["b"].grad.cpu()}
    refs = R._conv_ref(cpu, [gs.float()], got, "bf16", one, zero, one)
    ratios.update(_judge_all(tail, got, refs))
    report("NODE", "V7 out_bf16 -> " + tail, ratios)
    prev = ops.BF16_STORE
    ops.BF16_STORE = False
    try:
        assert ops.conv2d(t["x"], t["w"], t["b"], one, zero, one, out_bf16=True).dtype == torch.float32
    finally:
        ops.BF16_STORE = prev
    for k, want in (("Cout <= 8", ops.conv2d(t["x"], t["w"][:8], t["b"][:8], one, zero, one, out_bf16=True)),
                    ("OA OB % 4", ops.conv2d(t["x"][..., :29], t["w"], t["b"], one, zero, one, out_bf16=True))):
        assert want.dtype == torch.float32, (k, "stored in 16 bits against the use16 condition")


@pytest.mark.one_mode
@pytest.mark.parametrize("slots", (1, 3))
def test_v7_stat_sums_hand_off(slots, bf16_mode, launches):
    """conv1d(stat_sums=...) -> group_norm(sums=...) in bf16 mode: y stays fp32, the sums fp64; the epilogue's sums are judged from the
    stored y by gemm_ref's staged bound, GroupNorm's statistics as the finalize of those sums, its apply and backward by norm_ref fed
    the node's own statistics, the conv backward by gemm_ref fed the gradient GroupNorm returned"""
    from remfx_amd import nnops, ops
    from tests import gemm_ref as GR
    cpu, t = _v7_inputs((2, 16, 30), (24, 16, 3), 24)
    N = 2
    sums = ops.zeros((N, 2) if slots == 1 else (N, slots, 2), DEV, torch.float64)
    y = ops.conv1d(t["x"], t["w"], t["b"], 1, 1, 1, stat_sums=sums)
    y.retain_grad()
    assert y.dtype == torch.float32 and sums.dtype == torch.float64
    u = nnops.group_norm(y, 1, t["gamma"], t["beta"], R.GN_EPS, "gelu", sums=sums)
    stats = {"mean": u.grad_fn.saved_tensors[3].cpu(), "rstd": u.grad_fn.saved_tensors[4].cpu()}
    gy = torch.randn(u.shape, generator=torch.Generator().manual_seed(79)) * 0.75
    u.backward(gy.to(DEV))
    torch.cuda.synchronize()
    names = [n for n, _ in launches]
    assert "rfx_groupnorm_stat_chunks" not in names, "group_norm formed statistics of its own"
    ys, ss = y.detach().cpu(), sums.cpu()
    x4, w4 = cpu["x"].unsqueeze(2), cpu["w"].unsqueeze(2)
    c = GR.Case("node", "conv", "bf16", (), 16, 24, (1, 30), (1, 3), (1, 1), (0, 1), (1, 1), N=N, bias=True, stat_slots=slots)
    refs = GR.reference(c, {"x": x4, "w": w4, "b": cpu["b"]}, got={"y": ys.unsqueeze(2)})
    ratios = {"conv y": judge(ys.unsqueeze(2), refs["y"].ref, GR.tolerance(refs["y"], GR.k_of(c, "y")), ctx=("stat_sums", "y")),
              "stat": judge(ss.reshape(N, -1, 2).sum(1), refs["stat"].ref, GR.tolerance(refs["stat"], GR.k_of(c, "stat")), ctx=("stat_sums", "stat"))}
    got = dict(stats, y=u.detach().cpu(), d_x=y.grad.cpu(), d_gamma=t["gamma"].grad.cpu(), d_beta=t["beta"].grad.cpu())
    nrefs = R._norm_refs({"x": ys, "gamma": cpu["gamma"], "beta": cpu["beta"]}, [gy], got, "gn", 1, "gelu", False, True, sums=ss)
    ratios.update(_judge_all("stat_sums", got, nrefs, exact="value"))
    got = {"d_x": t["x"].grad.cpu(), "d_w": t["w"].grad.cpu(), "d_b": t["b"].grad.cpu()}
    crefs = R._lift(R._conv_ref, cpu, [y.grad.cpu()], got, "bf16", (1, 1), (0, 1), (1, 1))
    ratios.update(_judge_all("stat_sums", got, crefs))
    report("NODE", f"V7 stat_sums ({slots} slot(s)) -> group_norm", ratios)


# ---- V8: refusals, before any launch -------------------------------------------------------------------------------------------------------
def _refusals():
    from remfx_amd import nnops, ops
    f = lambda *s: torch.randn(*s, device=DEV)                       # noqa: E731
    x4, w, b = f(2, 16, 3, 11), f(24, 16, 3, 3), f(24)
    gam = f(8)
    one = (1, 1)
    yield "conv2d cpu x", lambda: ops.conv2d(x4.cpu(), w, b, one, one, one)
    yield "conv2d fp64 x", lambda: ops.conv2d(x4.double(), w, b, one, one, one)
    yield "conv2d fp64 w", lambda: ops.conv2d(x4, w.double(), b, one, one, one)
    yield "conv2d_glu cpu x", lambda: ops.conv2d_glu(x4.cpu(), w, b, one, one, one)
    yield "convT cpu x", lambda: ops.conv_transpose2d(f(2, 6, 3, 21).cpu(), f(6, 5, 1, 16), None, (1, 8))
    yield "convT fp64 x", lambda: ops.conv_transpose2d(f(2, 6, 3, 21).double(), f(6, 5, 1, 16), None, (1, 8))
    yield "activation fp64", lambda: ops.activation(x4.double(), "gelu")
    yield "activation cpu", lambda: ops.activation(x4.cpu(), "gelu")
    yield "activation_add fp64 res", lambda: ops.activation_add(x4, x4.double(), "gelu")
    yield "activation_to fp64", lambda: ops.activation_to(x4.double(), "gelu", (0, 2, 1))
    yield "group_norm cpu", lambda: nnops.group_norm(f(3, 8, 5, 7).cpu(), 2, gam, gam)
    yield "group_norm fp64", lambda: nnops.group_norm(f(3, 8, 5, 7).double(), 2, gam, gam)
    yield "group_norm fp64 res", lambda: nnops.group_norm(f(3, 8, 5, 7), 2, gam, gam, mode="glu_scale_res", res=f(3, 4, 5, 7).double(), scale=f(4))
    yield "group_norm bf16 res", lambda: nnops.group_norm(f(3, 8, 5, 7), 2, gam, gam, mode="glu_scale_res", res=f(3, 4, 5, 7).bfloat16(), scale=f(4))
    yield "glu odd C", lambda: nnops.glu(f(2, 5, 3, 4), 1)
    yield "glu dim 2", lambda: nnops.glu(f(2, 6, 4, 4), 2)
    yield "glu fp64", lambda: nnops.glu(f(2, 6, 4, 4).double(), 1)
    yield "mul shapes", lambda: nnops.mul(f(2, 3, 35), f(2, 3, 34))
    yield "mul cpu", lambda: nnops.mul(f(2, 3, 35).cpu(), f(2, 3, 35))
    yield "add y of lower rank", lambda: nnops.add(f(2, 3, 4, 5), f(2, 3, 5))
    yield "add fp64 y", lambda: nnops.add(f(2, 3, 4, 5), f(2, 3, 4, 5).double())
    yield "add cpu y", lambda: nnops.add(f(2, 3, 4, 5), f(2, 3, 4, 5).cpu())
    yield "row_affine fp64", lambda: nnops.row_affine(f(3, 1001).double(), f(3), f(3))
    yield "row_affine bf16", lambda: nnops.row_affine(f(3, 1001).bfloat16(), f(3), f(3))
    yield "row_moments fp64", lambda: nnops.row_moments(f(3, 1001).double(), 1e-5)
    yield "avg_pool fp64", lambda: nnops.avg_pool2d(f(2, 3, 5, 7).double(), (2, 3))
    yield "blstm_frame cpu", lambda: nnops.blstm_frame(f(2, 3, 50).cpu(), 6, 16, 8)
    yield "dropout fp64", lambda: nnops.dropout(f(2, 3, 5).double(), 0.3, True)
    yield "attention ch > 104", lambda: nnops.local_state_attention(f(1, 105, 300), f(1, 105, 300), f(1, 105, 300), f(1, 3, 300), 1, 3)
    yield "attention ndecay > 64", lambda: nnops.local_state_attention(f(1, 4, 300), f(1, 4, 300), f(1, 4, 300), f(1, 65, 300), 1, 65)


def test_refusals_launch_nothing(launches):
    """V8: a CPU tensor, an fp64 tensor, odd C for GLU, dim != 1, unequal shapes for mul, y of lower rank for add, the streaming
    attention limits: ValueError before any launch (host-only queries such as rfx_localstate_mfma_ok may run)"""
    for what, call in _refusals():
        del launches[:]
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{what}: accepted")
        assert [n for n, _ in launches if _is_launch(n)] == [], (what, [n for n, _ in launches])


@pytest.mark.one_mode
def test_groupnorm_refuses_a_gradient_that_is_not_fp32():
    from remfx_amd import nnops
    x = torch.randn(3, 8, 5, 7, device=DEV, requires_grad=True)
    y = nnops.group_norm(x, 2, torch.randn(8, device=DEV), torch.randn(8, device=DEV))
    with pytest.raises(ValueError):
        nnops._GroupNormFn.backward(y.grad_fn, torch.randn(3, 8, 5, 7, device=DEV, dtype=torch.float64))
