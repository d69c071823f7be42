"""Every kernel form of remfx_amd/csrc/cl_dconv.hip through the shipped launch path (remfx_amd/cldconv.py: layer_forward /
layer_backward -- descriptor, packing tables, pass sequencing, the dx convolution and the weight-gradient calls) against
tests/cldconv_ref.py: one fused layer in fp64, rounded to bf16 where the kernels round, judged PER ELEMENT and in stages at

    |got - ref| <= (8 x floor + 8) x eps32 x magnitude     (+ half a bf16 ulp of the value being rounded for every bf16-stored output)

Forward: hpre and statistics 1 from x; a from the fp64 h and the kernel's own statistics 1; statistics 2 and y from the kernel's own
a.  Backward, fed saved tensors made by the REFERENCE: dz from them; dh, dW2, db2 from the kernel's own dz; dx, dW1, db1 from its own
dh; the five small gradients from the reference chain.  The inference form's y equals the train form's bit for bit.  Floors, the two
power conditions, the planted faults and the walk of the case table over the dispatch are in tests/test_cldconv_ref_cpu.py, the
measured floors and what the bound can see in DESIGN.md 4.16.

Buffers: every tensor the launch path writes is NaN-filled between two NaN guards of 4096 elements (layer_forward / layer_backward
take the allocator); afterwards no output element is NaN, every guard holds its fill, channels H .. HP-1 of a, hpre, dh are exact
zeros, and a second run into fresh buffers gives the same bits.

The four-wave one-pass form (RFX_DEV=1 RFX_CLD_BWD_NW=4) reads its switch once per process: test_four_wave_form_in_a_child_process
runs its cases in one fresh pytest child, which it marks with CHILD_MARK; the cases exist only in that child.  A run that finds the
switch set without the mark (the whole suite started with it) fails: its bwd8<48,12> cases would run another kernel than they name."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import cldconv_ref as R
from tests.kernel_harness import Guarded, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]          # the kernels have one arithmetic mode

EPS = R.GEN_EPS
CHILD_MARK = "RFX_TEST_CLDCONV_FOUR_WAVE_CHILD"                # set by test_four_wave_form_in_a_child_process alone, for its child
FOUR = os.environ.get(CHILD_MARK) == "1"
FWD_CASES = R.forward_cases()
BWD_CASES = R.four_wave_cases() if FOUR else R.backward_cases()
PARAMS = ("W1", "b1", "g1w", "g1b", "W2", "b2", "g2w", "g2b", "scale")


class _Alloc:
    """the allocator handed to layer_forward / layer_backward: every tensor the launch path writes is a Guarded"""

    def __init__(self):
        self.bufs = {}

    def __call__(self, name, shape, dtype, device):
        self.bufs[name] = Guarded(math.prod(shape), dtype, name, device=device)
        return self.bufs[name].t.view(shape)

    def check(self, outputs):
        for name, b in self.bufs.items():
            b.owned() if name in outputs else b.guards_intact()

    def sizes(self, *names):
        """elements of the scratch buffers the launch path sized from the library's queries (absent: not allocated)"""
        return {n: self.bufs[n].n for n in names if n in self.bufs}


def _asked(case, *queries):
    """{field: what the library's query answers for the case's S, C, H, grid, TPS}, fields the call does not use (0) left out"""
    import ctypes
    from remfx_amd import _lib
    d = _lib.ClDconvDesc()
    d.S, d.C, d.H, d.grid, d.TPS = case.nsamp * case.TPS, case.C, case.C // 4, case.g, case.TPS
    got = {q.rsplit("_", 1)[1]: int(getattr(_lib.lib(), q)(ctypes.byref(d))) for q in queries}
    return {k: v for k, v in got.items() if v}


def _layout(case):
    """(Bn, A) of the (Bn, A, L, C) tensor the samples travel in"""
    if case.TPS > 1:
        return case.nsamp, 1
    return (1, case.nsamp) if case.nsamp <= 3 else (2, case.nsamp // 2)


def _dev(case, inp):
    dev = torch.device("cuda", torch.cuda.current_device())
    Bn, A = _layout(case)
    cl = lambda t: t.to(dev).to(torch.bfloat16).view(Bn, A, t.shape[1], t.shape[2]).contiguous()       # noqa: E731  (exact: bf16-representable)
    p = [inp[k].to(dev).contiguous() for k in PARAMS]
    p[4] = p[4].view(p[4].shape[0], p[4].shape[1], 1)           # conv2.weight (2 C, H, 1)
    return dev, cl, p


def _grids(monkeypatch, case):
    from remfx_amd import cldconv
    monkeypatch.setattr(cldconv, "GRID", case.g)
    monkeypatch.setattr(cldconv, "GRID_FWD", case.g)


def _cpu(t, N, H=None):
    t = t.detach().float().cpu()
    t = t.reshape(N, -1, t.shape[-1])
    return t if H is None else t[..., :H]


def run_forward(case, inp, train):
    from remfx_amd import cldconv
    dev, cl, p = _dev(case, inp)
    al = _Alloc()
    y, a, hpre, stats = cldconv.layer_forward(cl(inp["x"]), *p, case.dil, EPS, train, alloc=al)
    torch.cuda.synchronize()
    al.check(("y", "a", "hpre", "stats"))
    # rfx_cl_dconv_fwd_ws_partial against the restated rule: the tile sums [S][2] of the statistics passes, nothing at one tile per sample
    S = case.nsamp * case.TPS
    want = {"part": 2 * S} if case.TPS > 1 else {}
    asked = {"part": v for v in _asked(case, "rfx_cl_dconv_fwd_ws_partial").values()}
    assert al.sizes("part") == asked == want, (case.id, al.sizes("part"), asked, want)
    return y, a, hpre, stats


def run_backward(case, inp, sv):
    from remfx_amd import cldconv
    dev, cl, p = _dev(case, inp)
    H = case.C // 4
    HP = -(-H // 16) * 16
    pad = lambda t: cl(torch.nn.functional.pad(t.float(), (0, HP - H)))     # noqa: E731
    al = _Alloc()
    out = cldconv.layer_backward(cl(inp["gy"]), cl(inp["x"]), pad(sv["a"]), pad(sv["hpre"]), sv["stats"].to(dev).contiguous(), *p,
                                 case.dil, EPS, alloc=al)
    torch.cuda.synchronize()
    al.check(("dx", "dz", "dh", "pg"))
    # rfx_cl_dconv_bwd_ws_partial / _tsum / _sums against the restated rules: a row of 5 C + 2 H per workgroup, min(grid, S) workgroups;
    # in passes the tile sums [S][2] and the sample means [samples][4]
    S, want = case.nsamp * case.TPS, {"partial": min(case.g, case.nsamp * case.TPS) * (5 * case.C + 2 * H)}
    if case.passes:
        want.update(tsum=2 * S, sums=4 * case.nsamp)
    asked = _asked(case, "rfx_cl_dconv_bwd_ws_partial", "rfx_cl_dconv_bwd_ws_tsum", "rfx_cl_dconv_bwd_ws_sums")
    assert al.sizes("partial", "tsum", "sums") == asked == want, (case.id, al.sizes("partial", "tsum", "sums"), asked, want)
    return out


def _report(case, res):
    line = "  ".join(f"{n} {q:.3f}" for n, (q, _) in res.items())
    print(f"{case.id}: error / tolerance  {line}")
    bad = {n: v for n, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{case.id}: outside the bound (error / tolerance, flat index): {bad}"


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c.id)
def test_forward(monkeypatch, case):
    _grids(monkeypatch, case)
    inp = R.make_inputs(case)
    N, H = case.nsamp, case.C // 4
    y, a, hpre, stats = run_forward(case, inp, True)
    assert R.pad_is_zero(a, H) and R.pad_is_zero(hpre, H), "padded hidden channels of a / hpre are not exact zeros"
    y2, a2, hpre2, stats2 = run_forward(case, inp, True)
    for u, v, n in ((y, y2, "y"), (a, a2, "a"), (hpre, hpre2, "hpre"), (stats, stats2, "stats")):
        assert torch.equal(u, v), f"{n}: two runs differ"
    yi, ai, hi, si = run_forward(case, inp, False)              # the inference form: a == hpre == nullptr, TPS = 1 without stats
    assert ai is None and hi is None and (si is None) == (case.TPS == 1)
    assert torch.equal(yi.view(torch.int16), y.view(torch.int16)), "the inference form's y differs from the train form's"
    got = R._got_forward({"hpre": _cpu(hpre, N, H), "a": _cpu(a, N, H), "stats": stats.detach().cpu(), "y": _cpu(y, N)})
    _report(case, R.judge(R.FWD_OUT, R.stage_forward(inp, case.dil, got), got, R.K_of(case)))


def _switch_set():
    """the condition cld_launch reads from the environment (it cannot be asked which kernel it launched)"""
    def num(k):
        try:
            return int(os.environ.get(k, ""))
        except ValueError:
            return 0
    return num("RFX_DEV") == 1 and num("RFX_CLD_BWD_NW") == 4


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c.id)
def test_backward(monkeypatch, case):
    assert _switch_set() == FOUR, "the four-wave switch and the child's mark go together: this case would run another kernel than it names"
    _grids(monkeypatch, case)
    inp = R.make_inputs(case)
    N, Cc, H = case.nsamp, case.C, case.C // 4
    sv = R.saved_tensors(inp, case.dil)
    out = run_backward(case, inp, sv)
    dx, dz, dh, pg, dw1, db1, dw2, db2 = out
    assert R.pad_is_zero(dh, H), "padded hidden channels of dh are not exact zeros"
    for u, v, n in zip(out, run_backward(case, inp, sv), ("dx", "dz", "dh", "pg", "dw1", "db1", "dw2", "db2")):
        assert torch.equal(u, v), f"{n}: two runs differ"
    pgc = pg.detach().cpu()
    got = {"dx": _cpu(dx, N), "dz": _cpu(dz, N), "dh": _cpu(dh, N, H), "dw1": dw1.cpu(), "db1": db1.cpu(),
           "dw2": dw2.cpu().reshape(2 * Cc, H), "db2": db2.cpu(), "dscale": pgc[:Cc], "dgn2w": pgc[Cc:3 * Cc], "dgn2b": pgc[3 * Cc:5 * Cc],
           "dgn1w": pgc[5 * Cc:5 * Cc + H], "dgn1b": pgc[5 * Cc + H:]}
    _report(case, R.judge(R.BWD_OUT, R.stage_backward(inp, sv, case.dil, case.passes, got, case.g), got, R.K_of(case)))


def test_four_wave_form_in_a_child_process():
    """cl_dconv_bwd_kernel<48,12>: its C = 48, TPS = 1 cases in ONE fresh process (the switch is read once per process)"""
    assert not FOUR, "the child's -k selection leaves this test out"
    assert not _switch_set(), "RFX_CLD_BWD_NW is set for the whole run: the one-pass cases of this module would run the four-wave kernel"
    env = dict(os.environ, RFX_DEV="1", RFX_CLD_BWD_NW="4", **{CHILD_MARK: "1"})
    n = len(R.four_wave_cases())
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-k", "test_backward and nw4", "-q", "-s",
                        "-p", "no:cacheprovider"], env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.returncode
    assert f"{n} passed" in r.stdout, "the child did not run every four-wave case"
