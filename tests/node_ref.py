"""The autograd nodes of remfx_amd/ops.py and remfx_amd/nnops.py at their seams: one runner, device-agnostic, that
executes a case in variants -- strided operands, partial gradients, gradient layouts, no-grad, the parameter-gradient sink, a second use
in one step -- and the case table of tests/test_gpu_nodes.py with the fp64 reference and the per-element bound of every case.

A case is (make(seed) -> {name: CPU tensor or plain value}, call(inputs on the device) -> output(s), ref(...) -> {name: (fp64 reference,
bound)}).  Output names: "y" ("y0", "y1" for two outputs), "d_<input>" for the gradient of an input, anything else is a side result the
case's `extra` fetched (statistics, running buffers).  Every bound is imported from the module that pins the launched entry
(elem_ref, norm_ref, gemm_ref, attention_ref) or written out here from the number formats; none is measured on a device.

The runner never calls a kernel itself: tests/test_node_ref_cpu.py runs it on `StandIn`, a plain-torch Function with the interface of a
layer op and one switch per host fault, and shows that each variant rejects the fault it is named for."""
import contextlib
import dataclasses

import numpy as np
import torch

from tests.kernel_harness import bits, judge

HALF = 2.0 ** -24
LAYOUTS = ("perm", "slice", "expand", "offset")
GY_FORMS = ("sum", "transposed", "slice")


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def lay(t, kind):
    """(a view of layout `kind` on t's device, the values it holds as a contiguous tensor).  perm: batch and channel axes exchanged in
    memory; slice: a channel slice of a larger NaN-filled tensor (storage offset, non-dense batch stride); expand: the first sample for
    every sample (stride 0); offset: a contiguous view one element into its allocation (base address not 16-byte aligned)."""
    nan = float("nan")
    if kind == "contig":
        return t.contiguous(), t
    if kind == "perm":
        if t.dim() < 2:
            big = t.new_full((2 * t.numel(),), nan)
            big[::2] = t
            return big[::2], t
        return t.transpose(0, 1).contiguous().transpose(0, 1), t
    if kind == "slice":
        d = 1 if t.dim() >= 2 else 0
        shape = list(t.shape)
        shape[d] += 3
        v = t.new_full(shape, nan).narrow(d, 2, t.shape[d])
        v.copy_(t)
        return v, t
    if kind == "expand":
        v = t[:1].expand_as(t)
        return v, v.contiguous()
    if kind == "offset":
        off = max(1, 4 // t.element_size())                                 # one 32-bit word: 16-bit storage stays word-aligned
        v = t.new_full((t.numel() + off,), nan)[off:].view(t.shape)
        v.copy_(t)
        return v, t
    raise ValueError(kind)


def lay_gy(g, form):
    """the incoming gradient in one of the layouts autograd hands a node: transposed (last stride not 1), a slice of a larger tensor"""
    if form == "contig":
        return g.contiguous()
    if form == "transposed":
        a, b = (g.dim() - 1, g.dim() - 2) if g.dim() >= 2 and min(g.shape[-2:]) > 1 else (0, g.dim() - 1)
        return g.transpose(a, b).contiguous().transpose(a, b)
    if form == "slice":
        return lay(g, "slice")[0]
    raise ValueError(form)


# ---- the case ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    id: str
    node: str                          # the Function subclass the case pins
    make: object                       # seed -> {name: CPU tensor | plain value}
    call: object                       # {name: tensor on the device | plain value} -> tensor or tuple of tensors
    ref: object                        # (inputs CPU, gys CPU, got, mode) -> {name: (fp64 reference, bound)}
    diff: tuple                        # the differentiable inputs
    expect: tuple                      # the entry points V0 launches, forward then backward, each once
    ints: dict = dataclasses.field(default_factory=dict)      # the extents a launch passes as separate integers: pairwise distinct
    scales: dict = dataclasses.field(default_factory=dict)    # role -> scale of its draw: pairwise distinct
    params: tuple = ()                 # inputs that are parameters (sink route, second use)
    sinks: object = False              # the node writes parameter gradients through ops.sink_write: True (all of params) or their names
    loose: tuple = ()                  # results a launch sums with atomics in no fixed order: compared by LOOSE_REL, not by bits
    gemm: bool = False                 # a GEMM inside: runs in the three modes; second-use sums are judged by bound
    copied: tuple = None               # inputs the wrapper copies contiguous: a strided one gives V0's bits (default: all tensors)
    layouts: dict = dataclasses.field(default_factory=dict)   # input -> the layouts it takes (default: all four)
    by_bound: bool = False             # a launch with atomics inside: V1..V6 compare by V0's bound, not by bits
    classes: object = None             # () -> the Function classes whose backward returns are recorded
    extra: object = None               # (inputs on the device, outputs) -> {name: tensor}: side results judged like outputs
    variants: tuple = ("V1", "V2", "V3", "V4", "V5", "V6")
    exact: str = "bits"                # how an element whose bound is 0 is compared: norm_ref leaves the sign of a zero open
    note: str = ""

    def tensors(self, inp):
        return [k for k, v in inp.items() if isinstance(v, torch.Tensor)]


@dataclasses.dataclass
class Result:
    outs: list                         # CPU tensors
    grads: dict                        # input -> CPU tensor, or None where the node returned none
    raw: list                          # per recorded backward call: (needs_input_grad, which returns were None)
    gys: list                          # the CPU gradients fed in
    extra: dict
    out_strides: list
    requires: list                     # requires_grad of each output


def draw_gys(outs, seed):
    g = torch.Generator().manual_seed(977 + seed)
    return [torch.randn(o.shape, generator=g) * 0.75 for o in outs]


@contextlib.contextmanager
def recorded_backward(classes):
    """every backward of `classes` also leaves (needs_input_grad, [return is None]) in the list this yields"""
    log, saved = [], []
    for cls in classes:
        orig = cls.__dict__["backward"]
        fn = orig.__func__

        def rec(ctx, *g, _fn=fn):
            ret = _fn(ctx, *g)
            tup = ret if isinstance(ret, tuple) else (ret,)
            log.append((tuple(ctx.needs_input_grad), tuple(r is None for r in tup)))
            return ret
        saved.append((cls, orig))
        cls.backward = staticmethod(rec)
    try:
        yield log
    finally:
        for cls, orig in saved:
            cls.backward = orig


def run(case, inp, dev, layouts=None, need=None, gys=None, gy_form="contig", no_grad=False, params=None, sync=None):
    """One execution into fresh tensors.  layouts: {input: layout}; need: the inputs that ask for a gradient (default case.diff); gys:
    CPU gradients (default: drawn); gy_form: "contig", "sum" (out.sum().backward(): an expanded scalar) or one of lay_gy's; params:
    {input: Parameter on the device} used in place of the drawn tensor."""
    layouts, need = layouts or {}, tuple(case.diff if need is None else need)
    t = {}
    for k, v in inp.items():
        if not isinstance(v, torch.Tensor):
            t[k] = v
        elif params is not None and k in params:
            t[k] = params[k]
        else:
            t[k], _ = lay(v.detach().clone().to(dev), layouts.get(k, "contig"))
    grads = {k: [] for k in need}
    if not no_grad:
        for k in need:
            if not t[k].requires_grad:
                t[k].requires_grad_(True)
            t[k].register_hook(lambda g, k=k: grads[k].append(g) if g is not None else None)
    classes = case.classes() if case.classes else ()
    with recorded_backward(classes) as raw:
        with (torch.no_grad() if no_grad else contextlib.nullcontext()):
            out = case.call(t)
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        extra = case.extra(t, outs) if case.extra else {}
        extra = {k: v.detach().cpu() for k, v in extra.items()}
        requires = [o.requires_grad for o in outs]
        live = [i for i, o in enumerate(outs) if o.requires_grad]
        if gys is None:
            gys = draw_gys(outs, 0) if gy_form != "sum" else [torch.ones(o.shape) for o in outs]
        if live and not no_grad:
            if gy_form == "sum":
                sum(outs[i].sum() for i in live).backward()
            else:
                forms = gy_form if isinstance(gy_form, (list, tuple)) else [gy_form] * len(outs)
                torch.autograd.backward([outs[i] for i in live], [lay_gy(gys[i].to(dev), forms[i]) for i in live])
    if sync is not None:
        sync()
    res = {}
    for k in need:
        assert len(grads[k]) <= 1, (case.id, k, "gradient hook fired", len(grads[k]), "times")
        res[k] = grads[k][0].detach().cpu() if grads[k] else None
    return Result([o.detach().cpu() for o in outs], res, list(raw), gys, extra, [tuple(o.stride()) for o in outs], requires)


def named(res):
    """a Result as {name: tensor}: y / y0, y1; d_<input>; the side results"""
    out = {("y" if len(res.outs) == 1 else f"y{i}"): o for i, o in enumerate(res.outs)}
    out.update({"d_" + k: v for k, v in res.grads.items() if v is not None})
    out.update(res.extra)
    return out


def verdict(case, inp, res, mode, names=None):
    """every output of the run per element against the case's reference -> {name: largest error / bound}"""
    got = named(res)
    if case.ref is None:
        return {}
    refs = case.ref(inp, res.gys, got, mode)
    ratios = {}
    for k, v in got.items():
        if names is not None and k not in names:
            continue
        assert k in refs, (case.id, "no reference for", k)
        r, b = refs[k]
        ratios[k] = judge(v, r, b, exact=case.exact, ctx=(case.id, k))
    return ratios


LOOSE_REL = 4e-2                       # the relative L2 bound tests/test_gpu_dconv_fused.py puts on the fused backward's parameter gradients


def sink_names(case):
    return tuple(case.params) if case.sinks is True else tuple(case.sinks or ())


def same(case, a, b, what, exact="bits"):
    """two runs' outputs: the same bits (or values)"""
    A, B = named(a), named(b)
    assert A.keys() == B.keys(), (case.id, what, sorted(A), sorted(B))
    for k in A:
        if k in case.loose:
            d, n = float((A[k].double() - B[k].double()).norm()), float(B[k].double().norm())
            assert d <= LOOSE_REL * n, (case.id, what, k, "relative L2 difference", d / max(n, 1e-300))
        elif exact == "bits":
            assert A[k].dtype == B[k].dtype and torch.equal(bits(A[k]), bits(B[k])), (case.id, what, k, "differs from the anchor run")
        else:
            assert torch.equal(A[k], B[k]), (case.id, what, k, "differs from the anchor run by value")


def compare(case, inp, got, anchor, mode, what):
    """a variant against its anchor: by bits, or per element by the anchor's bound where the launch accumulates with atomics"""
    if case.by_bound:
        return verdict(case, inp, got, mode)
    same(case, got, anchor, what)
    return {}


# ---- the variants ----------------------------------------------------------------------------------------------------------------------
def v0(case, dev, mode, seed=0, sync=None):
    inp = case.make(seed)
    res = run(case, inp, dev, sync=sync)
    for k in case.diff:
        assert res.grads[k] is not None, (case.id, "V0: no gradient reached", k)
    return inp, res, verdict(case, inp, res, mode)


def v1(case, dev, mode, inp, anchor, sync=None):
    """every tensor input in every layout, one at a time"""
    ratios = {}
    for k in case.tensors(inp):
        for kind in case.layouts.get(k, LAYOUTS):
            view, vals = lay(inp[k], kind)
            if view.is_contiguous() and kind != "offset":
                continue                                                    # the layout is the dense one at this shape
            res = run(case, inp, dev, layouts={k: kind}, gys=anchor.gys, sync=sync)
            inp2 = dict(inp, **{k: vals})
            for n, r in verdict(case, inp2, res, mode).items():
                ratios[n] = max(ratios.get(n, 0.0), r)
            if k in (case.copied if case.copied is not None else case.tensors(inp)) and not case.by_bound:
                base = anchor if kind != "expand" else run(case, inp2, dev, gys=anchor.gys, sync=sync)
                same(case, res, base, f"V1 {k} {kind}")
    return ratios


def subsets(names):
    """the non-empty subsets of `names`, capped at the singles, "all but one" and all"""
    names = tuple(names)
    out = [(n,) for n in names]
    if len(names) > 2:
        out += [tuple(m for m in names if m != n) for n in names]
    if len(names) > 1:
        out.append(names)
    return out


def v2(case, dev, mode, inp, anchor, sync=None):
    """partial gradients: what is returned has the anchor's bits, what was not asked for is None"""
    ratios = {}
    for need in subsets(case.diff):
        res = run(case, inp, dev, need=need, gys=anchor.gys, sync=sync)
        for k in case.diff:
            if k in need:
                assert (res.grads[k] is None) == (anchor.grads[k] is None), (case.id, "V2", need, k, "gradient missing")
        part = Result(anchor.outs, {k: anchor.grads[k] for k in need}, [], anchor.gys, anchor.extra, anchor.out_strides, anchor.requires)
        ratios.update(compare(case, inp, res, part, mode, f"V2 {need}"))
        for needs, none in res.raw:
            for i, (n, z) in enumerate(zip(needs, none)):
                assert n or z, (case.id, "V2", need, "backward returned a tensor in slot", i, "that asked for none")
    return ratios


def v3(case, dev, mode, inp, anchor, sync=None, forms=GY_FORMS):
    """the incoming gradient in the layouts autograd produces: the bits of a run fed the contiguous copy of the same values"""
    ratios = {}
    for form in forms:
        if form == "sum":
            res = run(case, inp, dev, gy_form="sum", sync=sync)
            base = run(case, inp, dev, gys=res.gys, sync=sync)
        else:
            res = run(case, inp, dev, gys=anchor.gys, gy_form=form, sync=sync)
            base = anchor
        if case.by_bound:
            ratios.update(verdict(case, inp, res, mode))
        else:
            same(case, res, base, f"V3 {form}")
    return ratios


def v3_independent(case, dev, mode, inp, anchor, sync=None):
    """two differentiable outputs (ConvFork2dFn): each gradient in each form independently of the other"""
    ratios = {}
    for i in range(len(anchor.outs)):
        for form in GY_FORMS[1:]:
            forms = ["contig"] * len(anchor.outs)
            forms[i] = form
            res = run(case, inp, dev, gys=anchor.gys, gy_form=forms, sync=sync)
            ratios.update(compare(case, inp, res, anchor, mode, f"V3 output {i} {form}"))
    return ratios


def v4(case, dev, mode, inp, anchor, sync=None):
    """under no_grad: the anchor's output bits, no graph"""
    res = run(case, inp, dev, no_grad=True, gys=anchor.gys, sync=sync)
    assert not any(res.requires), (case.id, "V4: an output requires grad under no_grad")
    seen = {k: v for k, v in anchor.extra.items() if k in res.extra}       # what hangs on the graph (saved statistics) is not there
    fwd = Result(anchor.outs, {}, [], anchor.gys, seen, anchor.out_strides, anchor.requires)
    res.grads = {}
    if case.by_bound:
        return verdict(case, inp, res, mode, names=set(named(fwd)))
    same(case, res, fwd, "V4")
    return {}


def v5(case, dev, mode, inp, anchor, arm, routes, sync=None):
    """the parameters in a flat buffer with the sink armed (arm(route, {name: CPU tensor}) -> context yielding {name: Parameter} whose
    .grad is read after the context's exit): every parameter gradient equals the anchor's by value, and the node returned None for it
    wherever it writes through the sink"""
    ratios = {}
    for route in routes:
        with arm(route, {k: inp[k] for k in case.params}) as ps:
            res = run(case, inp, dev, params=ps, gys=anchor.gys, sync=sync)
        for k in case.params:
            got = ps[k].grad.detach().cpu()
            if k in sink_names(case) and route != "off":
                assert res.grads[k] is None, (case.id, "V5", route, k, "written through the sink AND returned to autograd")
            if (case.by_bound or case.gemm) and case.ref is not None:
                r, b = case.ref(inp, anchor.gys, {"d_" + k: got}, mode)["d_" + k]
                ratios[f"d_{k} {route}"] = judge(got, r, b, ctx=(case.id, "V5", route, k))
            if "d_" + k in case.loose:
                same(case, Result([], {k: got}, [], [], {}, [], []), Result([], {k: anchor.grads[k]}, [], [], {}, [], []), f"V5 {route}")
            elif not case.by_bound:
                assert torch.equal(got, anchor.grads[k]), (case.id, "V5", route, k, "differs from the anchor by value",
                                                           float((got - anchor.grads[k]).abs().max()))
        rest = Result(res.outs, {k: v for k, v in res.grads.items() if k not in case.params}, [], res.gys, res.extra, res.out_strides, res.requires)
        base = Result(anchor.outs, {k: v for k, v in anchor.grads.items() if k not in case.params}, [], anchor.gys, anchor.extra,
                      anchor.out_strides, anchor.requires)
        if not case.by_bound:
            same(case, rest, base, f"V5 {route}")
    return ratios


def v6(case, dev, mode, inp, anchor, arm, routes, sync=None):
    """the node applied twice to the same parameters before one backward: p.grad is the sum of the two single-use gradients"""
    inp2 = dict(case.make(1), **{k: inp[k] for k in case.params})
    single2 = run(case, inp2, dev, sync=sync)
    ratios = {}
    for route in routes:
        with arm(route, {k: inp[k] for k in case.params}) as ps:
            two = dataclasses.replace(case, call=lambda t, c=case.call: _twice(c, t, inp2, dev, case.params), extra=None, classes=None)
            run(two, inp, dev, params=ps, gys=list(anchor.gys) + list(single2.gys), need=case.params, sync=sync)
        for k in case.params:
            got = ps[k].grad.detach().cpu()
            a, b = anchor.grads[k].double(), single2.grads[k].double()
            if case.ref is None and k in sink_names(case) and route != "off":
                continue                             # no bound to judge the sink's own accumulation order by: the "off" route carries it
            if "d_" + k in case.loose:
                same(case, Result([], {k: got}, [], [], {}, [], []), Result([], {k: (a + b).float()}, [], [], {}, [], []), f"V6 {route}")
            elif (case.gemm or case.by_bound) and case.ref is not None:           # the sink's kernels add their partial sums to the buffer one by one: not fl(a + b)
                ra, ba = case.ref(inp, anchor.gys, {"d_" + k: anchor.grads[k]}, mode)["d_" + k]
                rb, bb = case.ref(inp2, single2.gys, {"d_" + k: single2.grads[k]}, mode)["d_" + k]
                bound = _t(ba) + _t(bb) + 2 * HALF * (ra.abs() + rb.abs())
                ratios[f"d_{k} {route}"] = judge(got, ra + rb, bound, ctx=(case.id, "V6", route, k))
            else:
                ratios[f"d_{k} {route}"] = judge(got, a + b, 0.0, exact="value", ctx=(case.id, "V6", route, k))
    return ratios


def _t(b):
    return b if isinstance(b, torch.Tensor) else torch.tensor(float(b), dtype=torch.float64)


def _twice(call, t, inp2, dev, params):
    t2 = {k: (t[k] if k in params else (v.to(dev) if isinstance(v, torch.Tensor) else v)) for k, v in inp2.items()}
    a, b = call(t), call(t2)
    a = list(a) if isinstance(a, (tuple, list)) else [a]
    b = list(b) if isinstance(b, (tuple, list)) else [b]
    return tuple(a + b)


# ---- the exchange rule -----------------------------------------------------------------------------------------------------------------
def exchange_rule(case):
    """the problems of a case under the argument-exchange rule: extents a launch passes as separate integers pairwise distinct (so that
    an exchanged pair moves a judged element), inputs of different roles drawn from different scales"""
    bad = []
    for table, what in ((case.ints, "extent"), (case.scales, "scale")):
        seen = {}
        for k, v in table.items():
            if v in seen:
                bad.append(f"{case.id}: {what} {k} = {seen[v]} = {v}")
            seen[v] = k
    return bad


# ---- the stand-in: a plain-torch Function with the interface of a layer op and one switch per host fault ----------------------------
STANDIN_SINK = None                    # {id(parameter): gradient buffer} while armed
FAULTS = ("slot", "ignore_needs", "gy_pointer", "dx_zero_stride", "assign", "double_count", "swap_ints")


class StandIn(torch.autograd.Function):
    """y[n][r][c] = x[n][r][c] w[r] + v[r] + b[c] on x (N, rows * cols), with `rows` and `cols` passed as integers; w, v, b are
    parameters and go to STANDIN_SINK when it holds them.  FAULT: None, or one of FAULTS."""
    FAULT = None

    @staticmethod
    def forward(ctx, x, w, v, b, rows, cols):
        if StandIn.FAULT == "swap_ints":
            rows, cols = cols, rows
        i = torch.arange(rows * cols)
        r, c = (i // cols) % w.numel(), (i % cols) % b.numel()
        xs = x if StandIn.FAULT == "dx_zero_stride" else x.contiguous()
        ctx.save_for_backward(xs, w, v, b, r, c)
        return x * w[r] + v[r] + b[c]

    @staticmethod
    def backward(ctx, gy):
        x, w, v, b, r, c = ctx.saved_tensors
        fault = StandIn.FAULT
        if fault == "gy_pointer":                                           # the data pointer read as if the tensor were dense
            dense = torch.empty(gy.shape).stride()
            gy = torch.as_strided(gy, gy.shape, dense, gy.storage_offset())
        need = ctx.needs_input_grad if fault != "ignore_needs" else (True,) * 6
        dx = dw = dv = db = None
        if need[0]:
            val = gy * w[r]
            if fault == "dx_zero_stride":
                dx = torch.empty_strided(x.shape, x.stride())
                for n in range(x.shape[0]):                                 # sample by sample, as a grid would: the last writer stays
                    dx[n] = val[n]
            else:
                dx = val
        rows, cols = w.numel(), b.numel()
        if need[1]:
            dw = torch.zeros(rows).index_add_(0, r, (gy * x).sum(0))
        if need[2]:
            dv = torch.zeros(rows).index_add_(0, r, gy.sum(0))
        if need[3]:
            db = torch.zeros(cols).index_add_(0, c, gy.sum(0))
        if fault == "slot":
            dw, dv = dv, dw
        sink = STANDIN_SINK
        if sink is not None and all(id(p) in sink for p in (w, v, b)):
            for p, d in ((w, dw), (v, dv), (b, db)):
                if d is not None:
                    if fault == "assign":
                        sink[id(p)].copy_(d)
                    else:
                        sink[id(p)].add_(d)
            if fault != "double_count":
                dw = dv = db = None
        return dx, dw, dv, db, None, None


@contextlib.contextmanager
def standin_arm(route, tensors):
    """the CPU counterpart of an armed optim.FlatParams: parameters whose .grad is a zeroed buffer the stand-in's sink adds into"""
    global STANDIN_SINK
    ps = {k: torch.nn.Parameter(v.clone()) for k, v in tensors.items()}
    for p in ps.values():
        p.grad = torch.zeros_like(p)
    STANDIN_SINK = {id(p): p.grad for p in ps.values()} if route != "off" else None
    try:
        yield ps
    finally:
        STANDIN_SINK = None


def standin_case(rows=3, cols=5, N=4):
    def make(seed):
        g = torch.Generator().manual_seed(10 + seed)
        return {"x": torch.randn(N, rows * cols, generator=g), "w": torch.randn(rows, generator=g) * 3.0, "v": torch.randn(rows, generator=g) * 0.1,
                "b": torch.randn(cols, generator=g) * 10.0, "rows": rows, "cols": cols}

    def ref(inp, gys, got, mode):
        x, w, v, b = (inp[k].double() for k in ("x", "w", "v", "b"))
        g = gys[0].double().view(N, rows, cols)
        x3 = x.view(N, rows, cols)
        y = x3 * w.view(1, -1, 1) + v.view(1, -1, 1) + b.view(1, 1, -1)
        mag = (x3 * w.view(1, -1, 1)).abs() + v.abs().view(1, -1, 1) + b.abs().view(1, 1, -1)
        nsum = lambda t: (t.numel() // t.shape[1]) if t.dim() == 3 else 1      # noqa: E731
        return {"y": (y.view(N, -1), 3 * HALF * mag.view(N, -1)),
                "d_x": ((g * w.view(1, -1, 1)).view(N, -1), 0.0),
                "d_w": ((g * x3).sum((0, 2)), (N * cols + 1) * HALF * (g * x3).abs().sum((0, 2))),
                "d_v": (g.sum((0, 2)), N * cols * HALF * g.abs().sum((0, 2))),
                "d_b": (g.sum((0, 1)), N * rows * HALF * g.abs().sum((0, 1)))}

    return Case(id=f"standin-{rows}x{cols}", node="StandIn", make=make,
                call=lambda t: StandIn.apply(t["x"], t["w"], t["v"], t["b"], t["rows"], t["cols"]), ref=ref, diff=("x", "w", "v", "b"),
                expect=(), ints={"N": N, "rows": rows, "cols": cols}, scales={"x": 1.0, "w": 3.0, "v": 0.1, "b": 10.0},
                params=("w", "v", "b"), sinks=True, copied=("x", "w", "v", "b"), classes=lambda: (StandIn,))


# =======================================================================================================================================
# the case table of tests/test_gpu_nodes.py.  remfx_amd is imported inside the calls only: this module loads without the library.
# =======================================================================================================================================
def _gen(seed, salt):
    return torch.Generator().manual_seed(100003 * salt + seed)


def _rn(g, shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def sum_bound(n, terms_abs):
    """any fp32 summation order of n terms: (n - 1) roundings of partial sums no larger than the sum of |terms|, first order, plus the
    rounding of one further factor"""
    return (n + 1) * HALF * terms_abs


# ---- activations -----------------------------------------------------------------------------------------------------------------------
ACT_KEYS = (None, "none", "relu", "gelu", "tanh", "leaky", "sigmoid")      # "prelu" takes a slope: rfx_act_* refuse it (rfx_prelu_fwd)


def _act_code(key):
    from tests import elem_ref as E
    return {None: E.NONE, "none": E.NONE, "relu": E.RELU, "gelu": E.GELU, "tanh": E.TANH, "leaky": E.LEAKY, "sigmoid": E.SIGMOID}[key]


def _act_refs(inp, gys, code, x16, res=None):
    from tests import elem_ref as E
    x = inp["x"].double()
    y, by = E.act(x, code), E.act_bound(x, code)
    if res is not None:
        y, by = y + res.double(), E.act_add_bound(x, res, code)
    g = gys[0].double()
    dx, bdx = g * E.act_grad(x, code), E.act_grad_bound(x, g, code)
    if x16:                                                               # the gradient is stored in 16 bits
        bdx = bdx + E.bf16_half_ulp(dx.abs() + bdx)
    return {"y": (y, by), "d_x": (dx, bdx)}


def _act_cases():
    from tests.ref_common import bf16_rne
    out = []
    for key in ACT_KEYS:
        code = _act_code(key)

        def make(seed, key=key):
            return {"x": _rn(_gen(seed, 1), (2, 3, 5, 7), 1.5), "act": key}

        def make16(seed, key=key):
            return {"x": bf16_rne(_rn(_gen(seed, 2), (2, 12, 3, 8), 1.5)).to(torch.bfloat16), "act": key}

        def make_add(seed, key=key):
            g = _gen(seed, 3)
            return {"x": _rn(g, (2, 3, 5, 7), 1.5), "res": _rn(g, (2, 3, 5, 7), 0.25), "act": key}

        def ref_add(inp, gys, got, mode, code=code):
            r = _act_refs(inp, gys, code, False, inp["res"])
            r["d_res"] = (gys[0].double(), 0.0)
            return r
        out.append(Case(f"act-{key}", "ActFn", make, lambda t: _ops().activation(t["x"], t["act"]),
                        lambda inp, gys, got, mode, code=code: _act_refs(inp, gys, code, False), ("x",), ("rfx_act_fwd", "rfx_act_bwd"),
                        ints={"n": 210}, classes=lambda: (_ops().ActFn,)))
        out.append(Case(f"act16-{key}", "ActFn", make16, lambda t: _ops().activation(t["x"], t["act"]),
                        lambda inp, gys, got, mode, code=code: _act_refs(inp, gys, code, True), ("x",), ("rfx_act_rows16", "rfx_act_rows16"),
                        ints={"R": 72, "T": 8}, classes=lambda: (_ops().ActFn,)))
        out.append(Case(f"act_add-{key}", "ActAddFn", make_add, lambda t: _ops().activation_add(t["x"], t["res"], t["act"]), ref_add,
                        ("x", "res"), ("rfx_act_add_fwd", "rfx_act_bwd"), ints={"n": 210}, scales={"x": 1.5, "res": 0.25},
                        classes=lambda: (_ops().ActAddFn,)))
    import itertools
    for perm in itertools.permutations(range(3)):
        for x16 in (False, True):
            def make_to(seed, perm=perm, x16=x16):
                x = _rn(_gen(seed, 4), (2, 3, 5, 8), 1.5)
                return {"x": bf16_rne(x).to(torch.bfloat16) if x16 else x, "act": "gelu", "perm": perm}

            def extra_to(t, outs, perm=perm):
                assert outs[0].permute(*perm, 3).is_contiguous(), ("activation_to: memory order", perm, outs[0].stride())
                return {}
            entry = "rfx_act_rows16" if x16 else "rfx_act_rows"
            out.append(Case(f"act_to-{''.join(map(str, perm))}-{'bf16' if x16 else 'f32'}", "ActToFn", make_to,
                            lambda t: _ops().activation_to(t["x"], t["act"], t["perm"]),
                            lambda inp, gys, got, mode, x16=x16: _act_refs(inp, gys, _act_code("gelu"), x16), ("x",), (entry, entry),
                            ints={"D0": 2, "D1": 3, "D2": 5, "T": 8}, copied=(), extra=extra_to, classes=lambda: (_ops().ActToFn,),
                            layouts={"x": ("perm", "slice", "expand", "offset")}))
    return out


def _ops():
    from remfx_amd import ops
    return ops


def _nn():
    from remfx_amd import nnops
    return nnops


# ---- pooling, GLU, add, mul -------------------------------------------------------------------------------------------------------------
def _pool_case():
    from tests import norm_ref as NR
    N, C, H, W, kh, kw = 2, 3, 5, 7, 2, 3

    def make(seed):
        return {"x": _rn(_gen(seed, 5), (N, C, H, W)), "k": (kh, kw)}

    def ref(inp, gys, got, mode):
        y, by = NR.pool_fwd(inp["x"].view(N * C, H, W), kh, kw)
        dx, bdx = NR.pool_bwd(gys[0].view(N * C, H // kh, W // kw), H, W, kh, kw)
        return {"y": (y, by), "d_x": (dx, bdx)}
    return Case("avgpool-2x3", "_AvgPoolFn", make, lambda t: _nn().avg_pool2d(t["x"], t["k"]), ref, ("x",),
                ("rfx_avgpool2d_fwd", "rfx_avgpool2d_bwd"), ints={"NC": N * C, "H": H, "W": W, "kh": kh, "kw": kw},
                classes=lambda: (_nn()._AvgPoolFn,))


def _glu_cases():
    from tests import norm_ref as NR
    out = []
    for shape in ((2, 6, 5, 7), (2, 4, 2, 6)):
        def make(seed, shape=shape):
            return {"x": _rn(_gen(seed, 6), shape, 2.0)}

        def ref(inp, gys, got, mode, shape=shape):
            x3, g3 = inp["x"].reshape(shape[0], shape[1], -1), gys[0].reshape(shape[0], shape[1] // 2, -1)
            return {"y": (NR.glu(x3)["y"], NR.glu_bounds(x3)["y"]), "d_x": (NR.glu(x3, g3)["gx"], NR.glu_bounds(x3, g3)["gx"])}
        out.append(Case("glu-" + "x".join(map(str, shape)), "_GluFn", make, lambda t: _nn().glu(t["x"], 1), ref, ("x",),
                        ("rfx_glu_fwd", "rfx_glu_bwd"), ints={"N": shape[0], "C": shape[1], "S": shape[2] * shape[3]},
                        classes=lambda: (_nn()._GluFn,)))
    return out


ADD_SHAPES = (((2, 3, 4, 300), (2, 3, 4, 300)), ((2, 3, 5, 77), (1, 3, 5, 1)), ((3, 4, 2, 513), (3, 4, 1, 513)), ((2, 5, 1001), (2, 5, 1001)),
              ((2, 5, 7, 3), (1, 1, 7, 3)))                                                       # test_gpu_norm.py::test_add_broadcast


def _add_cases():
    out = []
    for xs, ys in ADD_SHAPES:
        for alpha in (1.0, 0.3):
            def make(seed, xs=xs, ys=ys, alpha=alpha):
                g = _gen(seed, 7)
                return {"x": _rn(g, xs), "y": _rn(g, ys, 4.0), "alpha": alpha}

            def ref(inp, gys, got, mode, xs=xs, ys=ys, alpha=alpha):
                x, y, g = inp["x"].double(), inp["y"].double(), gys[0].double()
                ay = alpha * y.expand(xs)
                a32 = float(np.float32(alpha))
                n = g.numel() // y.numel()
                dy = g.sum_to_size(ys)
                if n == 1:
                    dyr, bdy = g * a32, 0.0                                                   # one rounded product, or the tensor itself
                else:
                    dyr, bdy = dy * alpha, sum_bound(n, g.abs().sum_to_size(ys) * abs(alpha))
                return {"y": (x + ay, 2 * HALF * (x.abs() + ay.abs())), "d_x": (g, 0.0), "d_y": (dyr, bdy)}
            same_shape = xs == ys
            bwd = () if same_shape else (("rfx_channel_sum",) if (ys[0] == 1 and ys[3] == 1 and ys[1:3] == xs[1:3]) else ())
            x4 = xs if len(xs) == 4 else (xs[0], xs[1], 1, xs[2])
            out.append(Case(f"add-{'x'.join(map(str, xs))}+{'x'.join(map(str, ys))}-a{alpha}", "_AddFn", make,
                            lambda t: _nn().add(t["x"], t["y"], t["alpha"]), ref, ("x", "y"), ("rfx_add_bcast",) + bwd,
                            ints={k: v for k, v in zip("NCAB", x4) if x4.count(v) == 1}, scales={"x": 1.0, "y": 4.0}, copied=("x",),
                            classes=lambda: (_nn()._AddFn,), layouts={"y": ("perm", "slice", "offset")},
                            note="d_x is the incoming gradient itself: V3 compares its values"))
    return out


def _mul_case():
    def make(seed):
        g = _gen(seed, 8)
        return {"a": _rn(g, (2, 3, 35)), "b": _rn(g, (2, 3, 35), 5.0)}

    def ref(inp, gys, got, mode):
        a, b, g = inp["a"].double(), inp["b"].double(), gys[0].double()
        return {"y": (a * b, 0.0), "d_a": (g * b, 0.0), "d_b": (g * a, 0.0)}
    return Case("mul-2x3x35", "_MulFn", make, lambda t: _nn().mul(t["a"], t["b"]), ref, ("a", "b"), ("rfx_mul", "rfx_mul", "rfx_mul"),
                ints={"n": 210}, scales={"a": 1.0, "b": 5.0}, classes=lambda: (_nn()._MulFn,))


# ---- row statistics and affine passes ----------------------------------------------------------------------------------------------------
ROWS_R, ROWS_L, ROWS_EPS = 3, 1001, 1e-5


def _row_cases():
    from tests import elem_ref as E

    def make(seed):
        g = _gen(seed, 9)
        return {"x": _rn(g, (ROWS_R, 7, 143), 2.0), "a": torch.rand(ROWS_R, generator=g) + 0.5, "b": _rn(g, (ROWS_R,), 6.0)}

    def ref(inp, gys, got, mode):
        x2 = inp["x"].reshape(ROWS_R, ROWS_L)
        y, mag = E.row_affine(x2, inp["a"], inp["b"])
        dx, _ = E.row_affine(gys[0].reshape(ROWS_R, ROWS_L), inp["a"], None)
        return {"y": (y, 2 * HALF * mag), "d_x": (dx, 0.0)}

    def make_std(seed):
        return {"x": _rn(_gen(seed, 10), (ROWS_R, 7, 143), 2.0) + 0.75, "eps": ROWS_EPS}

    def ref_std(inp, gys, got, mode):
        x2 = inp["x"].reshape(ROWS_R, ROWS_L)
        m, s, bm, bs = E.row_moments(x2)
        out = {"mean": (m, bm), "std": (s, bs)}
        if "a" in got:
            a, b, ba, bb = E.moments_coef(got["mean"], got["std"], ROWS_EPS)
            out.update({"a": (a, ba), "b": (b, bb)})
        if "y" in got:                                                     # staged: the pass applies the coefficients formed from the stored mean / std
            a, b, _, _ = E.moments_coef(got["mean"], got["std"], ROWS_EPS)
            a32, b32 = a.float(), b.float()
            y, mag = E.row_affine(x2, a32, b32)
            # the coefficients themselves are inside 3 and 4 half-ulps of (a, b): carried through y = x a + b
            out["y"] = (y, 2 * HALF * mag + 3 * HALF * (x2.double() * a[:, None]).abs() + 4 * HALF * b.abs()[:, None])
        return out

    def call_std(t):
        return _nn().row_standardize(t["x"], t["eps"])                      # y, mean, std

    def ref_std3(inp, gys, got, mode):
        r = ref_std(inp, gys, {"y": got["y0"].reshape(ROWS_R, ROWS_L), "mean": got["y1"], "std": got["y2"]}, mode)
        return {"y0": (r["y"][0].reshape(got["y0"].shape), r["y"][1].reshape(got["y0"].shape)), "y1": r["mean"], "y2": r["std"]}

    def call_mom(t):
        return _nn().row_moments(t["x"], t["eps"])

    def ref_mom(inp, gys, got, mode):
        named_ = {"mean": got["y0"], "std": got["y1"], "a": got["y2"], "b": got["y3"]}
        r = ref_std(inp, gys, named_, mode)
        return {"y0": r["mean"], "y1": r["std"], "y2": r["a"], "y3": r["b"]}
    ints = {"R": ROWS_R, "L": ROWS_L}
    return [Case("row_affine-3x1001", "_RowAffineFn", make, lambda t: _nn().row_affine(t["x"], t["a"], t["b"]), ref, ("x",),
                 ("rfx_row_affine", "rfx_row_affine"), ints=ints, scales={"x": 2.0, "a": 1.0, "b": 6.0}, classes=lambda: (_nn()._RowAffineFn,)),
            Case("row_standardize-3x1001", "row_standardize", make_std, call_std, ref_std3, (), ("rfx_row_moments", "rfx_row_affine"), ints=ints,
                 variants=("V1", "V4")),
            Case("row_moments-3x1001", "row_moments", make_std, call_mom, ref_mom, (), ("rfx_row_moments",), ints=ints, variants=("V1", "V4"))]


def _row_affine_add_cases():
    out = []
    Q, L = 2, 35
    for group in (1, 3):
        R = Q * group

        def make(seed, R=R, group=group):
            g = _gen(seed, 11)
            return {"x": _rn(g, (R, 5, 7), 2.0), "a": torch.rand(Q, generator=g) + 0.5, "b": _rn(g, (Q,), 6.0), "y": _rn(g, (R, 5, 7), 0.3),
                    "group": group}

        def ref(inp, gys, got, mode, R=R, group=group):
            ar, br = (inp[k].double().repeat_interleave(group)[:, None] for k in ("a", "b"))
            ax, y, g = inp["x"].double().reshape(R, L) * ar, inp["y"].double().reshape(R, L), gys[0].double().reshape(R, L)
            return {"y": (ax + br + y, 2.0 ** -22 * (ax.abs() + br.abs() + y.abs())), "d_x": (g * ar, 0.0), "d_y": (g, 0.0)}
        out.append(Case(f"row_affine_add-g{group}", "_RowAffineAddFn", make,
                        lambda t: _nn().row_affine_add(t["x"], t["a"], t["b"], t["y"], t["group"]), ref, ("x", "y"),
                        ("rfx_row_affine_add", "rfx_row_affine"), ints={"Q": Q, "group": group, "L": L} if group != Q else {"Q": Q, "L": L},
                        scales={"x": 2.0, "a": 1.0, "b": 6.0, "y": 0.3}, classes=lambda: (_nn()._RowAffineAddFn,),
                        note="d_y is the incoming gradient itself"))
    return out


def _cm_fm_cases():
    out = []
    N, bins, Fr = 6, 8, 5
    for group in (1, 3):
        def make(seed, group=group):
            g = _gen(seed, 12)
            return {"x": _rn(g, (N, 2, bins, Fr), 2.0), "a": torch.rand(N // group, generator=g) + 0.5, "b": _rn(g, (N // group,), 6.0),
                    "group": group}

        def ref(inp, gys, got, mode, group=group):
            ar, br = (inp[k].double().repeat_interleave(group)[:, None, None, None] for k in ("a", "b"))
            ax = inp["x"].double() * ar
            return {"y": ((ax + br).permute(0, 3, 2, 1), 2.0 ** -22 * (ax.abs() + br.abs()).permute(0, 3, 2, 1)),
                    "d_x": ((gys[0].double() * ar).permute(0, 3, 2, 1), 0.0)}
        out.append(Case(f"cm_to_fm_affine-g{group}", "_CmToFmAffineFn", make,
                        lambda t: _nn().cm_to_fm_affine(t["x"], t["a"], t["b"], t["group"]), ref, ("x",),
                        ("rfx_fm_cm_affine",) * 2 if group == 1 else ("rfx_fm_cm_affine_g",) * 2,
                        ints={"N": N, "group": group, "bins": bins, "F": Fr, "two": 2}, scales={"x": 2.0, "a": 1.0, "b": 6.0},
                        classes=lambda: (_nn()._CmToFmAffineFn,)))
    return out


# ---- BLSTM framing, dropout ----------------------------------------------------------------------------------------------------------
BLSTM = (2, 3, 50, 6, 16, 8)                       # B, C, T, nfr, width, stride: nfr = ceil((T - width) / stride) + 1 rounded as the caller does


def _blstm_cases():
    from tests import elem_ref as E
    B, C, T, nfr, width, stride = BLSTM
    n = width * B * nfr

    def make_f(seed):
        return {"x": _rn(_gen(seed, 13), (B, C, T)), "nfr": nfr, "width": width, "stride": stride}

    def ref_f(inp, gys, got, mode):
        h, _, _ = E.blstm_frames(inp["x"], None, BLSTM, 0)
        dx, mag, _ = E.blstm_frames(gys[0].reshape(-1), None, BLSTM, 1)
        return {"y": (h.reshape(1, C, n), 0.0), "d_x": (dx, E.blstm_bound(BLSTM, 1, False, dx, mag))}

    def make_u(seed, skip=True):
        g = _gen(seed, 14)
        return {"h": _rn(g, (1, C, n)), "skip": _rn(g, (B, C, T), 5.0) if skip else None, "B": B, "T": T, "nfr": nfr, "width": width, "stride": stride}

    def ref_u(inp, gys, got, mode):
        y, mag, _ = E.blstm_frames(inp["h"].reshape(-1), inp["skip"], BLSTM, 2)
        dh, _, _ = E.blstm_frames(gys[0], None, BLSTM, 3)
        out = {"y": (y, E.blstm_bound(BLSTM, 2, inp["skip"] is not None, y, mag)), "d_h": (dh.reshape(1, C, n), 0.0)}
        if inp["skip"] is not None:
            out["d_skip"] = (gys[0].double(), 0.0)
        return out
    ints = {"B": B, "C": C, "T": T, "nfr": nfr, "width": width, "stride": stride}
    call_u = lambda t: _nn().blstm_unframe(t["h"], t["skip"], t["B"], t["T"], t["nfr"], t["width"], t["stride"])      # noqa: E731
    return [Case("blstm_frame", "_BlstmFrameFn", make_f, lambda t: _nn().blstm_frame(t["x"], t["nfr"], t["width"], t["stride"]), ref_f, ("x",),
                 ("rfx_blstm_frames", "rfx_blstm_frames"), ints=ints, classes=lambda: (_nn()._BlstmFrameFn,)),
            Case("blstm_unframe-skip", "_BlstmUnframeFn", make_u, call_u, ref_u, ("h", "skip"), ("rfx_blstm_frames", "rfx_blstm_frames"), ints=ints,
                 scales={"h": 1.0, "skip": 5.0}, classes=lambda: (_nn()._BlstmUnframeFn,), layouts={"h": ("perm", "slice", "offset")}),
            Case("blstm_unframe-noskip", "_BlstmUnframeFn", lambda seed: make_u(seed, False), call_u, ref_u, ("h",),
                 ("rfx_blstm_frames", "rfx_blstm_frames"), ints=ints, classes=lambda: (_nn()._BlstmUnframeFn,), layouts={"h": ("perm", "slice", "offset")})]


DROPOUT_P, DROPOUT_SEED = 0.3, 1234


def dropout_seed():
    """the seed nnops.dropout draws after torch.manual_seed(DROPOUT_SEED)"""
    state = torch.random.get_rng_state()
    torch.manual_seed(DROPOUT_SEED)
    s = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.random.set_rng_state(state)
    return s


def _dropout_case():
    from tests import elem_ref as E

    def make(seed):
        return {"x": _rn(_gen(seed, 15), (2, 3, 5, 7)) + 3.0, "p": DROPOUT_P}

    def call(t):
        torch.manual_seed(DROPOUT_SEED)
        return _nn().dropout(t["x"], t["p"], True)

    def ref(inp, gys, got, mode):
        s = dropout_seed()
        y, keep = E.dropout(inp["x"].reshape(-1), DROPOUT_P, s)
        dx, _ = E.dropout(gys[0].reshape(-1), DROPOUT_P, s)
        if "d_x" in got:                       # the issue's statement of it: nonzero exactly where y is, gy / (1 - p) rounded once
            nz = got["y"].reshape(-1) != 0
            assert torch.equal(got["d_x"].reshape(-1) != 0, nz & (gys[0].reshape(-1) != 0)), "dropout: gx is not masked as y is"
        return {"y": (y.reshape(inp["x"].shape), 0.0), "d_x": (dx.reshape(inp["x"].shape), 0.0)}
    return Case("dropout-p0.3", "_DropoutFn", make, call, ref, ("x",), ("rfx_dropout", "rfx_dropout"), ints={"n": 210},
                classes=lambda: (_nn()._DropoutFn,))


# ---- GroupNorm / BatchNorm -------------------------------------------------------------------------------------------------------------
GN_SHAPE = (3, 8, 5, 7)
GN_SHAPE16 = (3, 8, 5, 12)             # rfx_groupnorm_fwd_x16 takes S % 4 == 0 only (norm_ref._storages): 5 x 7 is refused with code -1
GN_EPS = 1e-5


def _norm_refs(inp, gys, got, kind, G, mode, x16, bwd, sums=None):
    """norm_ref's reference fed the node's own saved statistics (judged on their own), and its tolerance.  sums: the {sum, sum^2} the
    node was given -- the statistics are then judged as the finalize of those, whatever produced them"""
    from tests import norm_ref as NR
    N, C = inp["x"].shape[:2]
    S = inp["x"].numel() // (N * C)
    case = NR.Case("node", kind, N, C, S, G, mode, x16, bwd=bwd)
    x3 = inp["x"].float().reshape(N, C, S)
    Co = C // 2 if NR.is_glu(mode) else C
    ni = {"x": x3, "gamma": inp["gamma"], "beta": inp["beta"], "idx": None,
          "res": inp["res"].reshape(N, Co, S) if inp.get("res") is not None else None, "scale": inp.get("scale"),
          "gy": gys[0].reshape(N, Co, S) if bwd else None}
    out = {}
    m, r = NR.stats(x3, kind, G, GN_EPS)
    if sums is not None:
        s = sums.double().reshape(N * G, -1, 2).sum(1)
        m, r = NR.finalize(s[:, 0], s[:, 1], (C // G) * S, GN_EPS)
    smag, sfl = NR.stat_magnitudes(x3, kind, G, GN_EPS), NR.stat_floors(x3, kind, G, GN_EPS)
    mk, rk = got["mean"].double().reshape(-1), got["rstd"].double().reshape(-1)
    out["mean"] = (m.reshape(-1), (NR.k_of(sfl["mean"]) * NR.EPS32 * smag["mean"]).reshape(-1))
    out["rstd"] = (r.reshape(-1), (NR.k_of(sfl["rstd"]) * NR.EPS32 * smag["rstd"] * r).reshape(-1))     # norm_ref bounds the RELATIVE error
    ref, mag, slack, fl = NR.floors(ni, mk.view_as(m), rk.view_as(r), case)
    shape = {"y": got["y"].shape, "dx": inp["x"].shape}
    for name, to in (("y", "y"), ("dx", "d_x"), ("dgamma", "d_gamma"), ("dbeta", "d_beta"), ("dscale", "d_scale")):
        if name in ref:
            tol = NR.tolerance(name, ref, mag, slack, fl, x16)
            out[to] = (ref[name].reshape(shape.get(name, ref[name].shape)), tol.reshape(shape.get(name, tol.shape)))
    if mode == "glu_scale_res" and bwd:
        out["d_res"] = (gys[0].double(), 0.0)
    return out


def _gn_cases():
    from tests.ref_common import bf16_rne
    out = []
    for G in (2, 4):
        for mode in ("none", "gelu", "glu", "glu_scale_res"):
            for x16 in (False, True):
                if x16 and (G != 2):
                    continue
                N, C, A, Bb = GN_SHAPE16 if x16 else GN_SHAPE
                Co = C // 2 if mode.startswith("glu") else C

                def make(seed, G=G, mode=mode, x16=x16, Co=Co, N=N, C=C, A=A, Bb=Bb):
                    g = _gen(seed, 16)
                    x = _rn(g, (N, C, A, Bb), 2.0) + 0.5
                    d = {"x": bf16_rne(x).to(torch.bfloat16) if x16 else x, "gamma": _rn(g, (C,), 3.0), "beta": _rn(g, (C,), 0.2), "G": G, "mode": mode}
                    if mode == "glu_scale_res":
                        d["res"], d["scale"] = _rn(g, (N, Co, A, Bb), 7.0), _rn(g, (Co,), 0.6)
                    return d

                def call(t):
                    return _nn().group_norm(t["x"], t["G"], t["gamma"], t["beta"], GN_EPS, t["mode"], res=t.get("res"), scale=t.get("scale"))

                def extra(t, outs):
                    fn = outs[0].grad_fn
                    if fn is None:
                        return {}
                    return {"mean": fn.saved_tensors[3], "rstd": fn.saved_tensors[4]}

                def ref(inp, gys, got, mode_, G=G, mode=mode, x16=x16):
                    if "mean" not in got:                                  # no graph (V4): the statistics are not observable, y by bits
                        return {}
                    return _norm_refs(inp, gys, got, "gn", G, mode, x16, any(k.startswith("d_") for k in got))
                diff = ("x", "gamma", "beta") + (("res", "scale") if mode == "glu_scale_res" else ())
                params = ("gamma", "beta") + (("scale",) if mode == "glu_scale_res" else ())
                e = "_x16" if x16 else ""
                out.append(Case(f"groupnorm-G{G}-{mode}-{'bf16' if x16 else 'f32'}", "_GroupNormFn", make, call, ref, diff,
                                ("rfx_groupnorm_fwd" + e, "rfx_groupnorm_bwd" + e), ints={"N": N, "C": C, "S": A * Bb, "G": G},
                                scales={"x": 2.0, "gamma": 3.0, "beta": 0.2, "res": 7.0, "scale": 0.6}, params=params, sinks=True, extra=extra,
                                classes=lambda: (_nn()._GroupNormFn,), exact="value"))
    return out


def _gn_sums_cases():
    """sums= of both ranks: {sum, sum^2} per (sample, group) in fp64 as a producing GEMM's epilogue leaves them, (N G, 2) and
    (N G, slots, 2) whose slots add up to the same totals (binary fractions: exactly)"""
    out = []
    N, C, A, Bb = GN_SHAPE
    G = 2
    for rank in (2, 3):
        for mode in ("gelu", "glu_scale_res"):
            Co = C // 2 if mode.startswith("glu") else C

            def make(seed, rank=rank, mode=mode, Co=Co):
                g = _gen(seed, 23)
                x = _rn(g, GN_SHAPE, 2.0) + 0.5
                r = x.double().reshape(N * G, -1)
                tot = torch.stack([r.sum(1), (r * r).sum(1)], 1)
                sums = tot if rank == 2 else torch.stack([tot * 0.5, tot * 0.25, tot * 0.25], 1)
                d = {"x": x, "gamma": _rn(g, (C,), 3.0), "beta": _rn(g, (C,), 0.2), "G": G, "mode": mode, "sums": sums}
                if mode == "glu_scale_res":
                    d["res"], d["scale"] = _rn(g, (N, Co, A, Bb), 7.0), _rn(g, (Co,), 0.6)
                return d

            def call(t):
                return _nn().group_norm(t["x"], t["G"], t["gamma"], t["beta"], GN_EPS, t["mode"], res=t.get("res"), scale=t.get("scale"), sums=t["sums"])

            def extra(t, outs):
                fn = outs[0].grad_fn
                return {} if fn is None else {"mean": fn.saved_tensors[3], "rstd": fn.saved_tensors[4]}

            def ref(inp, gys, got, mode_, mode=mode):
                if "mean" not in got:
                    return {}
                return _norm_refs(inp, gys, got, "gn", G, mode, False, any(k.startswith("d_") for k in got))
            diff = ("x", "gamma", "beta") + (("res", "scale") if mode == "glu_scale_res" else ())
            out.append(Case(f"groupnorm-sums{rank}-{mode}", "_GroupNormFn", make, call, ref, diff, ("rfx_groupnorm_fwd", "rfx_groupnorm_bwd"),
                            ints={"N": N, "C": C, "S": A * Bb, "G": G}, scales={"x": 2.0, "gamma": 3.0, "beta": 0.2, "res": 7.0, "scale": 0.6},
                            params=diff[1:3] + diff[4:], sinks=True, extra=extra, classes=lambda: (_nn()._GroupNormFn,), exact="value",
                            layouts={"sums": ("perm", "slice", "offset"), "x": ("perm", "slice", "offset")},
                            note="the sums are those of x: a layout that changes x (expand) would make them another tensor's"))
    return out


BN_SHAPE = (3, 6, 5, 7)


class _BN:
    """the parameter container nnops.batch_norm takes"""

    def __init__(self, t):
        self.weight, self.bias, self.running_mean, self.running_var = t["gamma"], t["beta"], t["rm"], t["rv"]
        self.num_batches_tracked, self.momentum, self.eps = None, 0.1, GN_EPS


def _bn_cases():
    out = []
    N, C, A, Bb = BN_SHAPE
    n = N * A * Bb
    for relu in (False, True):
        def make(seed):
            g = _gen(seed, 17)
            return {"x": _rn(g, BN_SHAPE, 1.5) - 0.3, "gamma": _rn(g, (C,), 3.0), "beta": _rn(g, (C,), 0.2), "rm": _rn(g, (C,), 0.5),
                    "rv": torch.rand(C, generator=g) + 0.5}

        def call(t, relu=relu):
            t["rm"], t["rv"] = t["rm"].clone(), t["rv"].clone()            # the node updates them in place: every run from the same values
            return _nn().batch_norm(t["x"], _BN(t), True, relu=relu)

        def extra(t, outs):
            fn = outs[0].grad_fn
            e = {"rm_out": t["rm"], "rv_out": t["rv"]}
            if fn is not None:
                e.update({"mean": fn.saved_tensors[3], "rstd": fn.saved_tensors[4]})
            return e

        def ref(inp, gys, got, mode_, relu=relu):
            if "mean" not in got:
                return {}
            r = _norm_refs(inp, gys, got, "bn", C, "relu" if relu else "none", False, any(k.startswith("d_") for k in got))
            # running statistics from the kernel's own mean / rstd: (1 - m) old + m new, torch ops in fp32 -- a handful of roundings each
            mk, rk = got["mean"].double(), got["rstd"].double()
            var = 1.0 / (rk * rk) - GN_EPS
            rm = 0.9 * inp["rm"].double() + 0.1 * mk
            rv = 0.9 * inp["rv"].double() + 0.1 * var * (n / (n - 1))
            r["rm_out"] = (rm, 4 * HALF * (0.9 * inp["rm"].double().abs() + 0.1 * mk.abs()))
            r["rv_out"] = (rv, 8 * HALF * (0.9 * inp["rv"].double().abs() + 0.1 * (var.abs() + 2 * GN_EPS + 1.0 / (rk * rk)) * (n / (n - 1))))
            return r
        out.append(Case(f"batchnorm-train-{'relu' if relu else 'none'}", "_BatchNormFn", make, call, ref, ("x", "gamma", "beta"),
                        ("rfx_batchnorm_fwd", "rfx_batchnorm_bwd"), ints={"N": N, "C": C, "S": A * Bb},
                        scales={"x": 1.5, "gamma": 3.0, "beta": 0.2, "rm": 0.5}, params=("gamma", "beta"), sinks=False, extra=extra,
                        classes=lambda: (_nn()._BatchNormFn,), layouts={"rm": (), "rv": ()}, exact="value"))
    return out


# ---- the gather-GEMM nodes -------------------------------------------------------------------------------------------------------------
CONV_ENTRIES = ("rfx_pack_a", "rfx_gemm_fwd", "rfx_gemm_wgrad", "rfx_unpack_set", "rfx_unpack_col")    # forward, dx, (dw, db): as a set
CONVT_ENTRIES = ("rfx_pack_a", "rfx_gemm_fwd", "rfx_gemm_wgrad", "rfx_zero", "rfx_unpack_add", "rfx_channel_sum")


def expected(case, mode):
    """the entries V0 of the case launches in `mode`: a multiset for the single-launch nodes, a set for the GEMM nodes"""
    e = case.expect(mode) if callable(case.expect) else case.expect
    return sorted(set(e)) if case.gemm else sorted(e)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _gemm_refs(kind, mode, inp, x, w, b, g, stride, padding, dilation, names, crop=None, res=None, merged=False, out16=False):
    """gemm_ref's reference and tolerance for one launch family: kind "conv" (y), "dgrad" (dx), "wgrad" (dw, db), "convT" (y)"""
    from tests import gemm_ref as GR
    if kind == "convT":
        cin, cout = w.shape[0], w.shape[1]
    else:
        cout, cin = w.shape[0], w.shape[1]
    c = GR.Case("node", kind, mode, (), cin, cout, tuple(x.shape[2:]), tuple(w.shape[2:]), tuple(stride), tuple(padding), tuple(dilation),
                N=x.shape[0], bias=b is not None, res=res is not None, crop=crop or ((0, 0), (0, 0)), edges=("mg",) if merged else (), out16=out16)
    gi = {"x": x, "w": w}
    if b is not None:
        gi["b"] = b
    if g is not None:
        gi["g"] = g
    if res is not None:
        gi["res"] = res
    refs = GR.reference(c, gi)
    return {to: (refs[k].ref, GR.tolerance(refs[k], GR.k_of(c, k))) for k, to in names.items() if k in refs}


def _merged(ksize, stride, padding, dilation, rows):
    """ops._merge_axis and the row condition of its two callers, restated"""
    if tuple(dilation) != (1, 1):
        return False
    for ax in (0, 1):
        o = 1 - ax
        S, K = stride[ax], ksize[ax]
        if 2 <= S <= 256 and (S & (S - 1)) == 0 and K % S == 0 and stride[o] == 1 and ksize[o] == 1 and padding[o] == 0:
            return rows * S >= 4
    return False


def _conv_ref(inp, gys, got, mode, stride, padding, dilation, fork=False, out16=False):
    x, w, b = inp["x"], inp["w"], inp.get("b")
    yname = "y0" if fork else "y"
    out = _gemm_refs("conv", mode, inp, x, w, b, None, stride, padding, dilation, {"y": yname}, out16=out16)
    if fork:
        out["y1"] = (x.double(), 0.0)
    g = gys[0]
    if "d_x" in got:
        res = gys[1] if fork else None
        out.update(_gemm_refs("dgrad", mode, inp, x, w, None, g, stride, padding, dilation, {"dx": "d_x"}, res=res,
                              merged=_merged(w.shape[2:], stride, padding, dilation, w.shape[1])))
    if "d_w" in got or "d_b" in got:
        out.update(_gemm_refs("wgrad", mode, inp, x, w, b, g, stride, padding, dilation, {"dw": "d_w", "db": "d_b"}))
    return out


#            id                     Cin Cout (IA, IB)  (KA, KB) stride  padding dilation
CONV = (("cm-3to5-dil4",            3,  5,  (1, 37),  (1, 7),  (1, 1), (0, 0), (1, 4)),
        ("tap-16to24-3x3",          16, 24, (3, 11),  (3, 3),  (1, 1), (1, 1), (1, 1)),
        ("merged-16to24-k8s4",      16, 24, (1, 47),  (1, 8),  (1, 4), (0, 2), (1, 1)),
        ("phase-12to7-5x3",         12, 7,  (9, 18),  (5, 3),  (2, 1), (0, 0), (1, 1)),
        ("pruned-24to40-3x3",       24, 40, (1, 96),  (3, 3),  (1, 1), (1, 1), (1, 1)))
CONV_N = 2


def _conv_cases():
    out = []
    for cid, cin, cout, ish, ks, st, pd, dl in CONV:
        for fork in (False, True):
            if fork and cid.startswith(("cm", "pruned")):
                continue

            def make(seed, cin=cin, cout=cout, ish=ish, ks=ks):
                g = _gen(seed, 18)
                return {"x": _rn(g, (CONV_N, cin) + ish), "w": _rn(g, (cout, cin) + ks, 1.0 / (cin * ks[0] * ks[1]) ** 0.5), "b": _rn(g, (cout,), 2.0)}

            def call(t, st=st, pd=pd, dl=dl, fork=fork):
                f = _ops().conv2d_fork if fork else _ops().conv2d
                return f(t["x"], t["w"], t["b"], st, pd, dl)

            def ref(inp, gys, got, mode, st=st, pd=pd, dl=dl, fork=fork):
                return _conv_ref(inp, gys, got, mode, st, pd, dl, fork)
            ints = {"N": CONV_N, "Cin": cin, "Cout": cout, "IB": ish[1]}           # the issue fixes the kernel sizes: k (3, 3) ties with IA = 3
            if ish[0] > 1:
                ints["IA"] = ish[0]
            if ks[0] != ks[1]:                                                  # kh != kw wherever the issue's case has it
                ints.update({"KA": ks[0], "KB": ks[1]} if ks[0] > 1 else {"KB": ks[1]})
            out.append(Case(("fork-" if fork else "conv-") + cid, "ConvFork2dFn" if fork else "Conv2dFn", make, call, ref, ("x", "w", "b"),
                            CONV_ENTRIES + (("rfx_zero",) if cid.startswith("pruned") else ()), ints=ints, scales={"x": 1.0, "w": 1.0 / (cin * ks[0] * ks[1]) ** 0.5, "b": 2.0}, params=("w", "b"), sinks=True, gemm=True,
                            copied=("w", "b"), classes=lambda fork=fork: (_ops().ConvFork2dFn if fork else _ops().Conv2dFn,)))
    return out


def _out16_case():
    """16 -> 24, (2, 30), k (1, 3) with out_bf16: stored in 16 bits in bf16 mode (Cout > 8, OA OB = 56 a multiple of 4, no activation),
    fp32 otherwise; the gradient then arrives in 16 bits too"""
    from tests.ref_common import bf16_rne
    one, zero = (1, 1), (0, 0)

    def make(seed):
        g = _gen(seed, 24)
        return {"x": _rn(g, (2, 16, 2, 30)), "w": _rn(g, (24, 16, 1, 3), 1.0 / 48 ** 0.5), "b": _rn(g, (24,), 2.0)}

    def extra(t, outs):
        want = torch.bfloat16 if _ops().bf16_storage() else torch.float32
        assert outs[0].dtype == want, ("conv2d(out_bf16=True) stored", outs[0].dtype, "the use16 condition says", want)
        return {}

    def ref(inp, gys, got, mode):
        o16 = mode == "bf16"
        return _conv_ref(inp, [bf16_rne(gys[0]) if o16 else gys[0]], got, mode, one, zero, one, out16=o16)
    return Case("conv-out_bf16-16to24", "Conv2dFn", make, lambda t: _ops().conv2d(t["x"], t["w"], t["b"], one, zero, one, out_bf16=True), ref,
                ("x", "w", "b"), CONV_ENTRIES, ints={"N": 2, "Cin": 16, "Cout": 24, "IB": 30, "KB": 3}, scales={"x": 1.0, "w": 1.0 / 48 ** 0.5, "b": 2.0},
                params=("w", "b"), sinks=True, gemm=True, copied=("w", "b"), extra=extra, classes=lambda: (_ops().Conv2dFn,))


def _linear_case():
    def make(seed):
        g = _gen(seed, 19)
        return {"x": _rn(g, (2, 5, 7)), "w": _rn(g, (3, 7), 0.4), "b": _rn(g, (3,), 2.0)}

    def ref(inp, gys, got, mode):
        x4 = inp["x"].reshape(1, 10, 7).transpose(1, 2).unsqueeze(2)
        i4 = {"x": x4, "w": inp["w"].reshape(3, 7, 1, 1), "b": inp["b"]}
        g4 = [gys[0].reshape(1, 10, 3).transpose(1, 2).unsqueeze(2)]
        got4 = {k: v for k, v in got.items()}
        r = _conv_ref(i4, g4, got4, mode, (1, 1), (0, 0), (1, 1))
        back = {"y": lambda t: t.squeeze(2).transpose(1, 2).reshape(2, 5, 3), "d_x": lambda t: t.squeeze(2).transpose(1, 2).reshape(2, 5, 7),
                "d_w": lambda t: t.reshape(3, 7), "d_b": lambda t: t}
        return {k: (back[k](v[0]), back[k](v[1]) if isinstance(v[1], torch.Tensor) else v[1]) for k, v in r.items()}
    return Case("linear-2x5x7to3", "Conv2dFn", make, lambda t: _nn().linear(t["x"], t["w"], t["b"]), ref, ("x", "w", "b"), CONV_ENTRIES,
                ints={"rows": 10, "Cin": 7, "Cout": 3}, scales={"x": 1.0, "w": 0.4, "b": 2.0}, params=("w", "b"), sinks=True, gemm=True,
                copied=("w", "b"), classes=lambda: (_ops().Conv2dFn,))


def _convT_ref(inp, gys, got, mode, st, lo):
    """ConvT2dFn with the crop `lo` on both sides of each axis"""
    x, w, b, g = inp["x"], inp["w"], inp["b"], gys[0]
    ks, cout = tuple(w.shape[2:]), w.shape[1]
    mg = _merged(ks, st, (0, 0), (1, 1), cout) and lo[1 - (0 if st[0] > 1 else 1)] == 0
    out_ = _gemm_refs("convT", mode, inp, x, w, b, None, st, (0, 0), (1, 1), {"y": "y"}, crop=(lo, lo), merged=mg)
    # the backward: dx = conv(g padded by the crop, w) is a forward-family launch gathering g; dw a weight gradient with the roles
    # of x and g exchanged; db = channel_sum(g)
    gp = torch.nn.functional.pad(g, (lo[1], lo[1], lo[0], lo[0]))
    if "d_x" in got:
        out_.update(_gemm_refs("conv", mode, inp, gp, w, None, None, st, (0, 0), (1, 1), {"y": "d_x"}))
    if "d_w" in got:
        out_.update(_gemm_refs("wgrad", mode, inp, gp, w, None, x, st, (0, 0), (1, 1), {"dw": "d_w"}))
    if "d_b" in got:
        n = g.numel() // g.shape[1]
        out_["d_b"] = (g.double().sum((0, 2, 3)), (HALF + 4 * 2.0 ** -53 * n) * g.double().abs().sum((0, 2, 3)))
    return out_


def _lift(ref4, inp, gys, got, mode, *a):
    """a 4-D reference for a 1-D shim: (N, C, T) tensors as (N, C, 1, T), the results squeezed again"""
    i4 = {k: (v.unsqueeze(2) if isinstance(v, torch.Tensor) and v.dim() == 3 else v) for k, v in inp.items()}
    r = ref4(i4, [g.unsqueeze(2) for g in gys], got, mode, *a)
    sq = lambda t: t.squeeze(2) if isinstance(t, torch.Tensor) and t.dim() == 4 else t      # noqa: E731
    return {k: (sq(v[0]), sq(v[1])) for k, v in r.items()}


def _shim_cases():
    """the 1-D wrappers: their own unsqueeze / squeeze and (1, stride), (0, padding), (1, dilation) tuples"""
    out = []

    def mk(salt, xs, ws, wscale, nb):
        def make(seed):
            g = _gen(seed, salt)
            return {"x": _rn(g, xs), "w": _rn(g, ws, wscale), "b": _rn(g, (nb,), 2.0)}
        return make
    sc = lambda ws: {"x": 1.0, "w": ws, "b": 2.0}                                # noqa: E731
    # conv1d: 3 -> 5, T 37, k 7, dilation 4 (channel-major); stride 4, padding 2 on 16 -> 24, T 47, k 8 (merged-phase dgrad) through the fork
    w1 = 1.0 / 21 ** 0.5
    out.append(Case("conv1d-3to5-dil4", "Conv2dFn", mk(30, (2, 3, 37), (5, 3, 7), w1, 5), lambda t: _ops().conv1d(t["x"], t["w"], t["b"], 1, 0, 4),
                    lambda inp, gys, got, mode: _lift(_conv_ref, inp, gys, got, mode, (1, 1), (0, 0), (1, 4)), ("x", "w", "b"), CONV_ENTRIES,
                    ints={"N": 2, "Cin": 3, "Cout": 5, "T": 37, "K": 7, "dil": 4}, scales=sc(w1), params=("w", "b"), sinks=True, gemm=True,
                    copied=("w", "b"), classes=lambda: (_ops().Conv2dFn,)))
    w2 = 1.0 / 128 ** 0.5
    out.append(Case("conv1d_fork-16to24-k8s4", "ConvFork2dFn", mk(31, (2, 16, 47), (24, 16, 8), w2, 24),
                    lambda t: _ops().conv1d_fork(t["x"], t["w"], t["b"], 4, 2, 1),
                    lambda inp, gys, got, mode: _lift(_conv_ref, inp, gys, got, mode, (1, 4), (0, 2), (1, 1), True), ("x", "w", "b"), CONV_ENTRIES,
                    ints={"N": 2, "Cin": 16, "Cout": 24, "T": 47, "K": 8, "stride": 4}, scales=sc(w2), params=("w", "b"), sinks=True, gemm=True,
                    copied=("w", "b"), classes=lambda: (_ops().ConvFork2dFn,)))
    w3 = 1.0 / 48 ** 0.5
    out.append(Case("conv1d_glu-16to24", "ConvGlu2dFn", mk(32, (2, 16, 30), (24, 16, 3), w3, 24), lambda t: _ops().conv1d_glu(t["x"], t["w"], t["b"], 1, 1, 1),
                    None, ("x", "w", "b"), lambda mode: CONV_ENTRIES + (("rfx_glu_bwd_bf16",) if mode == "bf16" else ("rfx_glu_bwd",)),
                    ints={"N": 2, "Cin": 16, "C2": 24, "T": 30, "K": 3}, scales=sc(w3), params=("w", "b"), sinks=True, gemm=True, copied=("w", "b"),
                    variants=("V1", "V2", "V3", "V4", "V5"), classes=lambda: (_ops().ConvGlu2dFn,),
                    note="anchor: the RMS check of tests/test_gpu_conv.py (two chained launches, no importable bound)"))
    # conv_transpose1d: 6 -> 5, T 21, k 16, stride 8, crop 5 on both sides
    w4 = (8 / 96) ** 0.5
    out.append(Case("conv_transpose1d-6to5-k16s8", "ConvT2dFn", mk(33, (2, 6, 21), (6, 5, 16), w4, 5),
                    lambda t: _ops().conv_transpose1d(t["x"], t["w"], t["b"], 8, 1, 5, 166),
                    lambda inp, gys, got, mode: _lift(_convT_ref, inp, gys, got, mode, (1, 8), (0, 5)), ("x", "w", "b"), CONVT_ENTRIES,
                    ints={"N": 2, "Cin": 6, "Cout": 5, "T": 21, "K": 16, "stride": 8}, scales=sc(w4), params=("w", "b"), sinks=True, gemm=True,
                    copied=("w", "b"), classes=lambda: (_ops().ConvT2dFn,)))
    return out


#            id                 N  Cin Cout (IA, IB)  (KA, KB)  stride  crop_lo
CONVT = (("merged-6to5-k16s8",  2, 6,  5,  (3, 21),  (1, 16),  (1, 8), (0, 5)),
         ("phase-12to9-7x5",    2, 12, 9,  (6, 7),   (7, 5),   (2, 2), (3, 2)),
         ("thin-48to2-8x1",     3, 48, 2,  (4, 10),  (8, 1),   (4, 1), (0, 0)))


def _convT_cases():
    from tests import gemm_ref as GR
    out = []
    for cid, Nn, cin, cout, ish, ks, st, lo in CONVT:
        full = tuple((i - 1) * s + k for i, k, s in zip(ish, ks, st))
        olen = tuple(f - 2 * c for f, c in zip(full, lo))                   # the crop on both sides, as the decoders do

        def make(seed, Nn=Nn, cin=cin, cout=cout, ish=ish, ks=ks, st=st):
            g = _gen(seed, 20)
            return {"x": _rn(g, (Nn, cin) + ish), "w": _rn(g, (cin, cout) + ks, (st[0] * st[1] / (cin * ks[0] * ks[1])) ** 0.5), "b": _rn(g, (cout,), 2.0)}

        def call(t, st=st, lo=lo, olen=olen):
            return _ops().conv_transpose2d(t["x"], t["w"], t["b"], st, (1, 1), lo, olen)

        def ref(inp, gys, got, mode, st=st, lo=lo):
            return _convT_ref(inp, gys, got, mode, st, lo)
        out.append(Case("convT-" + cid, "ConvT2dFn", make, call, ref, ("x", "w", "b"), CONVT_ENTRIES,
                        ints={"N": Nn, "Cin": cin, "Cout": cout, "IA": ish[0], "IB": ish[1]},
                        scales={"x": 1.0, "w": (st[0] * st[1] / (cin * ks[0] * ks[1])) ** 0.5, "b": 2.0}, params=("w", "b"), sinks=True, gemm=True, copied=("w", "b"),
                        classes=lambda: (_ops().ConvT2dFn,)))
    return out


def _convglu_cases():
    out = []
    for cin, c2 in ((16, 24), (4, 8)):
        fused = c2 > 8

        def make(seed, cin=cin, c2=c2):
            g = _gen(seed, 21)
            return {"x": _rn(g, (CONV_N, cin, 3, 10)), "w": _rn(g, (c2, cin, 1, 3), 1.0 / (3 * cin) ** 0.5), "b": _rn(g, (c2,), 2.0)}
        out.append(Case(f"convglu-{cin}to{c2}", "ConvGlu2dFn" if fused else "_GluFn", make,
                        lambda t: _ops().conv2d_glu(t["x"], t["w"], t["b"], (1, 1), (0, 1), (1, 1)), None, ("x", "w", "b"),
                        (lambda mode: CONV_ENTRIES + (("rfx_glu_bwd_bf16",) if mode == "bf16" else ("rfx_glu_bwd",))) if fused
                        else CONV_ENTRIES + ("rfx_glu_fwd", "rfx_glu_bwd"),
                        ints={"N": CONV_N, "Cin": cin, "C2": c2, "IA": 3, "IB": 10}, scales={"x": 1.0, "w": 1.0 / (3 * cin) ** 0.5, "b": 2.0},
                        params=("w", "b"), sinks=True, gemm=True, copied=("w", "b"), variants=("V1", "V2", "V3", "V4", "V5"),
                        classes=lambda fused=fused: (_ops().ConvGlu2dFn,) if fused else (_ops().Conv2dFn, _nn()._GluFn),
                        note="anchor: the RMS check of tests/test_gpu_conv.py (two chained launches, no importable bound)"))
    return out


# ---- LocalState attention ---------------------------------------------------------------------------------------------------------------
def _attention_cases():
    from tests import attention_ref as AR
    out = []
    for cid, B, heads, ch, T, nd in (("resident", 2, 2, 4, 19, 3), ("streaming", 2, 2, 4, 257, 3), ("mfma", 2, 2, 16, 33, 4)):
        def make(seed, B=B, heads=heads, ch=ch, T=T, nd=nd):
            g = _gen(seed, 22)
            return {"q": _rn(g, (B, heads * ch, T), 0.8), "k": _rn(g, (B, heads * ch, T), 0.6), "content": _rn(g, (B, heads * ch, T), 1.7),
                    "qd": _rn(g, (B, heads * nd, T), 0.4), "heads": heads, "nd": nd}

        def ref(inp, gys, got, mode, heads=heads, nd=nd, ch=ch, T=T):
            rules = "bf16" if AR.form(ch, T, nd, mode)[0] == AR.MFMA else "exact"
            r, fl, elem = AR.floors(inp["q"], inp["k"], inp["content"], inp["qd"], gys[0], heads, nd, rules)
            names = {"y": "out", "d_q": "dq", "d_k": "dk", "d_content": "dcont", "d_qd": "dqd"}
            return {k: (r[n], AR.MARGIN * elem[n] + AR.TINY) for k, n in names.items() if k in got}
        out.append(Case("localstate-" + cid, "_LocalStateFn", make,
                        lambda t: _nn().local_state_attention(t["q"], t["k"], t["content"], t["qd"], t["heads"], t["nd"]), ref,
                        ("q", "k", "content", "qd"),
                        {"resident": ("rfx_localstate_fwd", "rfx_localstate_bwd"), "streaming": ("rfx_localstate_gen_fwd", "rfx_localstate_gen_bwd"),
                         "mfma": lambda mode: ("rfx_localstate_mfma_fwd", "rfx_localstate_mfma_bwd") if mode == "bf16" else
                         ("rfx_localstate_fwd", "rfx_localstate_bwd")}[cid], ints={"heads": heads, "ch": ch, "T": T, "ndecay": nd},
                        scales={"q": 0.8, "k": 0.6, "content": 1.7, "qd": 0.4}, gemm=True, classes=lambda: (_nn()._LocalStateFn,)))
    return out


# ---- the fused DConv depth layer (bf16 mode) ------------------------------------------------------------------------------------------------
DCONV_PARAMS = ("W1", "b1", "g1w", "g1b", "W2", "b2", "g2w", "g2b", "scale")
DCONV_SMALL = ("d_g1w", "d_g1b", "d_g2w", "d_g2b", "d_scale")


def dconv_cases():
    """(3, 48, 256), dilation 1 and 2, both backward forms; run by test_gpu_nodes.py::test_dconv_node with the bf16 mode set.  The inputs
    are dconv_ref's (every sample and every row of every parameter on a scale of its own).  No V0 bound: dconv_ref judges the kernels
    stage by stage from intermediates the node does not hand out, so the anchor stays test_gpu_dconv_fused.py / test_gpu_dconv_kernel.py and
    the variants carry the node.  The one-launch backward adds the five small parameter gradients with LDS atomics: `loose`."""
    from tests import dconv_ref as D
    out = []
    for dil in (1, 2):
        for fused in (False, True):
            def make(seed, dil=dil):
                inp = D.make_inputs(D.Case(3 + seed, dil))
                d = {k: inp[k][:3] if k == "x" else inp[k] for k in ("x",) + DCONV_PARAMS}
                d["W2"] = d["W2"].unsqueeze(2)
                d["dil"] = dil
                return d

            def call(t, fused=fused):
                nn_ = _nn()
                prev = nn_.DCONV_FUSED_BWD
                nn_.DCONV_FUSED_BWD = fused
                try:
                    return nn_._DConvLayerFn.apply(t["x"], *[t[k] for k in DCONV_PARAMS], t["dil"], D.GEN_EPS, torch.is_grad_enabled())
                finally:
                    nn_.DCONV_FUSED_BWD = prev
            bwd = (("rfx_dconv_layer_bwd",) if fused else ("rfx_groupnorm_bwd_x16", "rfx_pack_a", "rfx_gemm_fwd")) + ("rfx_gemm_wgrad", "rfx_unpack_set", "rfx_unpack_col")
            out.append(Case(f"dconv-d{dil}-{'fused' if fused else 'layers'}", "_DConvLayerFn", make, call, None, ("x",) + DCONV_PARAMS,
                            ("rfx_dconv_layer_fwd",) + bwd, ints={"N": 3, "C": D.C, "T": D.T, "H": D.H}, scales={"x": 1.0, "W1": 1.0 / 12.0, "W2": 0.29},
                            params=DCONV_PARAMS, sinks=("W1", "b1", "W2", "b2"), gemm=True, loose=DCONV_SMALL if fused else (),
                            layouts=dict({"x": ("perm", "slice", "expand")}, **{k: ("perm",) for k in DCONV_PARAMS}),
                            classes=lambda: (_nn()._DConvLayerFn,),
                            note="anchor: tests/test_gpu_dconv_fused.py (RMS) and tests/test_gpu_dconv_kernel.py (the entries per element)"))
    return out


_TABLE = None


def case_table():
    global _TABLE
    if _TABLE is None:
        t = (_act_cases() + [_pool_case()] + _glu_cases() + _add_cases() + [_mul_case()] + _row_cases() + _row_affine_add_cases() + _cm_fm_cases()
             + _blstm_cases() + [_dropout_case()] + _gn_cases() + _bn_cases() + _conv_cases() + [_linear_case()] + _convT_cases() + _convglu_cases()
             + _attention_cases() + _shim_cases() + _gn_sums_cases() + [_out16_case()])
        assert len({c.id for c in t}) == len(t)
        _TABLE = t
    return _TABLE


def by_id(cid):
    return next(c for c in case_table() if c.id == cid)
