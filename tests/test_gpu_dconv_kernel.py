"""Both kernels of remfx_amd/csrc/dconv.hip through the C ABI (rfx_dconv_layer_fwd, rfx_dconv_layer_bwd, rfx_dconv_layer_bwd_ws,
rfx_dconv_layer_ok) against tests/dconv_ref.py: one fused channel-major DConv layer in fp64, rounded to bf16 where the kernels round,
judged PER ELEMENT and in stages at

    |got - ref| <= (8 x floor + 8) x eps32 x magnitude     (+ half a bf16 ulp of the value being rounded for h16, z16, dz, dh)

Forward: h16 and statistics 1 from x; a_out from the fp64 h and the kernel's own statistics 1; z16, statistics 2 and out from the
kernel's own a_out.  Backward: a_out as in the forward; dz and the five GroupNorm-2 / LayerScale sums from the chain continued at the
kernel's own a_out; dh and the two GroupNorm-1 sums from its own dz; gx from its own dh; every row of `partial` against the samples its
workgroup owned (pairs wg, wg + grid, ...) and the fp64 column sums against the sum of all.  Floors, the planted faults and the
conditions are in tests/test_dconv_ref_cpu.py, the measured figures in DESIGN.md 4.26.

Buffers: every tensor a call reads or writes lies between two NaN guards of 4096 elements; outputs are NaN-filled.  Afterwards every
output element is finite, every guard holds its fill and every input its bits.  gx, dz, dh, a_out and every forward output repeat bit
for bit in a second run into fresh buffers.  `partial` does not have to: its accumulators take LDS float atomics from 16 waves in an
order that is not fixed (what still uses atomics), so its two runs are each held to the bound, not to each other's
bits."""
import itertools

import pytest
import torch

from tests import dconv_ref as R
from tests.kernel_harness import Guarded, api, report, same_bits, stop_after_a_device_error, sync  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]          # the kernels have one arithmetic mode

EPS = R.GEN_EPS
C, H, T, ROWS = R.C, R.H, R.T, R.ROWS
F32, BF16 = torch.float32, torch.bfloat16
CASES = R.cases()
PARAMS = ("W1", "b1", "g1w", "g1b", "W2", "b2", "g2w", "g2b", "scale")
SAVES = ("h16", "z16", "a_out", "stats")
FWD_ARGS = ("x", "out") + PARAMS + SAVES                       # the pointer arguments in ABI order
BWD_ARGS = ("x", "gy", "gx") + PARAMS + ("dz", "a_out", "dh", "partial")
_INPUTS = {}


def _inp(case):
    if case not in _INPUTS:
        _INPUTS.clear()                                        # one case's inputs at a time (25 MB each at N = 513)
        _INPUTS[case] = R.make_inputs(case)
    return _INPUTS[case]


class Call:
    """the buffers of one call.  off: every fp32 payload one element, every bf16 payload two elements (4 bytes: dz is written with
    4-byte stores) into its allocation"""

    def __init__(self, inp, N, bwd, train=True, off=False):
        o = {F32: 1, BF16: 2} if off else {F32: 0, BF16: 0}
        self.N, self.bwd = N, bwd
        self.ins = {k: Guarded(inp[k].numel(), F32, k, init=inp[k], off=o[F32]) for k in ("x",) + (("gy",) if bwd else ()) + PARAMS}
        if bwd:
            nws = int(api()[0].rfx_dconv_layer_bwd_ws(N, C, T, 1))    # `partial` is as long as the library says: one row per workgroup
            assert nws == R.bwd_rows(N) * ROWS
            shapes = {"gx": (F32, (N, C, T)), "dz": (BF16, (N, 2 * C, T)), "a_out": (F32, (N, H, T)), "dh": (BF16, (N, H, T)),
                      "partial": (F32, (nws // ROWS, ROWS))}
        else:
            shapes = {"out": (F32, (N, C, T))}
            if train:
                shapes.update(h16=(BF16, (N, H, T)), z16=(BF16, (N, 2 * C, T)), a_out=(F32, (N, H, T)), stats=(F32, (4, N)))
        self.shapes = shapes
        self.outs = {k: Guarded(torch.Size(s).numel(), dt, k, off=o[dt]) for k, (dt, s) in shapes.items()}

    def launch(self, dil, N=None, Cc=C, Tt=T, null=(), eps=EPS):
        lib, _, stream = api()
        p = lambda k: None if k in null or (k not in self.ins and k not in self.outs) else (self.ins.get(k) or self.outs[k]).ptr()   # noqa: E731
        N = self.N if N is None else N
        if self.bwd:
            a = [p(k) for k in BWD_ARGS]
            return lib.rfx_dconv_layer_bwd(*a[:3], N, Cc, Tt, dil, *a[3:12], eps, *a[12:], stream())
        a = [p(k) for k in FWD_ARGS]
        return lib.rfx_dconv_layer_fwd(*a[:2], N, Cc, Tt, dil, *a[2:11], eps, *a[11:], stream())

    def run(self, dil):
        sync(self.launch(dil), "rfx_dconv_layer_" + ("bwd" if self.bwd else "fwd"), (self.N, dil))
        for b in self.outs.values():
            b.owned()
        for b in self.ins.values():
            b.unchanged()
        return {k: b.cpu().view(self.shapes[k][1]) for k, b in self.outs.items()}

    def refused(self, rc, what):
        torch.cuda.synchronize()
        assert rc == -1, (what, "returned", rc)
        for b in self.outs.values():
            b.untouched()
        for b in self.ins.values():
            b.unchanged()


def _show(case, entry, res, label=""):
    report("dconv", entry, {k: q for k, (q, _) in res.items()}, f"{case.id}{' ' + label if label else ''}")
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{case.id} {entry}: outside the bound (error / bound, sample or row): {bad}"


def _forward(case, off=False):
    inp = _inp(case)
    run = lambda train: (lambda: Call(inp, case.N, False, train, off).run(case.dil))     # noqa: E731
    got = run(True)()
    same_bits(got, run(True)(), "train form")
    inf = run(False)()
    same_bits(inf, run(False)(), "inference form")
    assert set(inf) == {"out"}
    same_bits(inf, {"out": got["out"]}, "the inference form's out against the train form's")
    _show(case, "fwd", R.judge_forward(inp, case.dil, got, R.K_of(case.klass(False))), "offset" if off else "")
    return got


def _backward(case, off=False):
    inp = _inp(case)
    run = lambda: Call(inp, case.N, True, off=off).run(case.dil)                         # noqa: E731
    got, again = run(), run()
    assert got["partial"].shape == (R.bwd_rows(case.N), ROWS)
    det = ("gx", "dz", "dh", "a_out")
    same_bits({k: got[k] for k in det}, {k: again[k] for k in det}, "backward")
    K = R.K_of(case.klass(True))
    _show(case, "bwd", R.judge_backward(inp, case.dil, got, K), "offset" if off else "")
    again.update({k: got[k] for k in det})                     # the second run's partial, at the bound
    res = R.judge_backward(inp, case.dil, again, K)
    _show(case, "bwd", {k: res[k] for k in R.SMALL}, "second run" + (" offset" if off else ""))
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_forward(case):
    _forward(case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_backward(case):
    _backward(case)


def test_offsets():
    """payloads one fp32 element / two bf16 elements into their allocations: the same bits as the aligned run"""
    case = R.Case(3, 2)
    inp = _inp(case)
    same_bits(_forward(case, off=True), Call(inp, case.N, False).run(case.dil), "forward at an offset")
    got, ref = _backward(case, off=True), Call(inp, case.N, True).run(case.dil)
    det = ("gx", "dz", "dh", "a_out")
    same_bits({k: got[k] for k in det}, {k: ref[k] for k in det}, "backward at an offset")


def test_backward_feeds_the_weight_gradient_calls():
    """dz / a_out and dh / x through the weight-gradient call nnops makes (ops.conv2d_wgrad, bf16 mode): dW2, db2, dW1, db1 against the
    fp64 sums formed from the kernel's own dz / dh, at the weight-gradient GEMM's own floors"""
    from remfx_amd import ops
    case = R.Case(3, 2)
    inp, N, dil = _inp(case), case.N, case.dil
    call = Call(inp, N, True)
    got = call.run(dil)
    dev = lambda k: (call.outs.get(k) or call.ins[k]).t.view(call.shapes[k][1] if k in call.shapes else (N, C, T)).unsqueeze(2)   # noqa: E731
    prev = ops.gemm_precision()
    ops.set_gemm_precision("bf16")
    try:
        dw2, db2 = ops.conv2d_wgrad(dev("a_out"), dev("dz"), (2 * C, H, 1, 1), (1, 1), (0, 0), (1, 1), True)
        dw1, db1 = ops.conv2d_wgrad(dev("x"), dev("dh"), (H, C, 1, 3), (1, 1), (0, dil), (1, dil), True)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_precision(prev)
    for b in list(call.outs.values()) + list(call.ins.values()):
        b.unchanged() if b.before is not None else b.guards_intact()
    got.update(dw2=dw2.cpu().view(2 * C, H), db2=db2.cpu(), dw1=dw1.cpu().view(H, C, 3), db1=db1.cpu())
    K = {k: R.k_of(f) for k, f in R.FLOORS_WGRAD.items()}
    _show(case, "bwd -> wgrad", R.judge_wgrad(inp, dil, got, K))


def test_bwd_ws():
    """floats of `partial`: a row of 5 C + 2 H per workgroup, a workgroup per pair of samples up to 256; the same for both dilations,
    -1 for what rfx_dconv_layer_bwd refuses"""
    lib = api()[0]
    for N in (1, 2, 3, 511, 512, 513, 100000):
        for dil in (1, 2):
            assert lib.rfx_dconv_layer_bwd_ws(N, C, T, dil) == min(-(-N // 2), 256) * ROWS == R.bwd_rows(N) * ROWS, N
    for bad in ((0, C, T, 1), (-1, C, T, 1), (4, 96, T, 1), (4, C, 255, 1), (4, C, T, 3)):
        assert lib.rfx_dconv_layer_bwd_ws(*bad) == -1, bad


def test_layer_ok():
    lib = api()[0]
    for Cc, Tt, dil in itertools.product((16, 47, 48, 96), (255, 256, 512), (0, 1, 2, 3, 4)):
        assert bool(lib.rfx_dconv_layer_ok(Cc, Tt, dil)) == ((Cc, Tt) == (48, 256) and dil in (1, 2)), (Cc, Tt, dil)


def _refusals(call, required):
    for k in required:
        call.refused(call.launch(1, null=(k,)), f"{k} = NULL")
    for N in (0, -1):
        call.refused(call.launch(1, N=N), f"N = {N}")
    for Cc in (16, 47, 96):
        call.refused(call.launch(1, Cc=Cc), f"C = {Cc}")
    for Tt in (255, 512):
        call.refused(call.launch(1, Tt=Tt), f"T = {Tt}")
    for dil in (0, 3):
        call.refused(call.launch(dil), f"dil = {dil}")


def test_forward_refusals():
    case = R.Case(1, 1)
    call = Call(_inp(case), 1, False)
    _refusals(call, ("x", "out") + PARAMS)
    for n in (1, 2, 3):                                         # the 14 proper non-empty subsets of the four save pointers
        for keep in itertools.combinations(SAVES, n):
            call.refused(call.launch(1, null=tuple(s for s in SAVES if s not in keep)), f"only {keep} of the save pointers")
    report("dconv", "fwd refusals", {})


def test_backward_refusals():
    case = R.Case(1, 1)
    call = Call(_inp(case), 1, True)
    _refusals(call, BWD_ARGS)
    report("dconv", "bwd refusals", {})
