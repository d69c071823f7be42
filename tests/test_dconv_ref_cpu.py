"""CPU: what tests/dconv_ref.py (the reference of tests/test_gpu_dconv_kernel.py) is worth.  With rounding off it agrees with torch
float64 autograd on oracle.ref_hdemucs.DConv, forward and every gradient; the column sums of its `partial` are the parameter gradients;
the floors its K come from are re-measured here (the fp32 restatement with the kernels' partial sums against fp64, never the kernel);
the restatement is inside every case's bound; no element's bound rests on the absolute allowance; and every planted fault is rejected
by the GPU test's own judge, by the output dconv_ref.MUTATIONS names for it.

The N = 513 / 514 cases are evaluated here on the samples that make them what they are (Case.cpu_sel / cpu_rows: workgroup 0's walk, its
neighbour's, the last); the GPU test judges every sample and every row."""
import pytest
import torch

from tests import dconv_ref as R
from tests.gemm_ref import FLOORS as GEMM_FLOORS

CASES = R.cases()
_CACHE = {}


def _evaluated(case, bwd):
    """(inputs, the fp32 restatement's outputs, what to judge) of a case, computed once"""
    key = (case, bwd)
    if key not in _CACHE:
        inp = R.make_inputs(case)
        if bwd:
            rows = case.cpu_rows()
            got, need = R.kern32_backward(inp, case.dil, rows)
            _CACHE[key] = (inp, got, {"sel": need, "rows": rows})
        else:
            sel = case.cpu_sel()
            _CACHE[key] = (R.take(inp, sel), R.kern32_forward(inp, case.dil, sel), {})
    return _CACHE[key]


def _judge(case, bwd, inp, got, how, **kw):
    K = None if kw.get("measure") else R.K_of(case.klass(bwd))
    return (R.judge_backward if bwd else R.judge_forward)(inp, case.dil, got, K, **how, **kw)


@pytest.mark.parametrize("case", [R.Case(3, 1), R.Case(3, 2), R.Case(3, 1, bias=True)], ids=lambda c: c.id)
def test_reference_agrees_with_autograd(case):
    """Exact, rounding off, against autograd through one layer of the oracle's DConv in fp64: out and every gradient; the column sums
    of the reference partial are the five small gradients; dW1 / dW2 / db1 / db2 formed from the reference dh / x and dz / a"""
    from oracle import ref_hdemucs
    inp = R.make_inputs(case)
    N = case.N
    net = ref_hdemucs.DConv(R.C, compress=4, depth=2, init=1e-4, attn=False, lstm=False).double()
    layer = net.layers[{1: 0, 2: 1}[case.dil]]
    conv1, gn1, conv2, gn2, ls = layer[0], layer[1], layer[3], layer[4], layer[6]
    assert conv1.dilation == (case.dil,) and conv1.padding == (case.dil,)
    with torch.no_grad():
        for prm, k in ((conv1.weight, "W1"), (conv1.bias, "b1"), (gn1.weight, "g1w"), (gn1.bias, "g1b"), (conv2.bias, "b2"),
                       (gn2.weight, "g2w"), (gn2.bias, "g2b"), (ls.scale, "scale")):
            prm.copy_(inp[k].double())
        conv2.weight.copy_(inp["W2"].double()[:, :, None])
    gn1.eps = gn2.eps = R.f32(R.GEN_EPS)
    x = inp["x"].double().requires_grad_(True)
    y = x + layer(x)
    y.backward(inp["gy"].double())
    scale = lambda t: float(t.detach().abs().max())             # noqa: E731
    f = R.forward(inp, case.dil, R.Exact, False)
    assert float((f["out"] - y.detach()).abs().max()) <= 1e-12 * scale(y)
    b = R.backward(inp, case.dil, R.Exact, False)
    assert float((b["gx"] - x.grad).abs().max()) <= 1e-12 * scale(x.grad)
    G = R.bwd_rows(N)
    partial = torch.stack([b["small"][R.wg_samples(N, wg)].sum(0) for wg in range(G)])
    assert partial.shape == (G, R.ROWS)
    for name, prm in (("dscale", ls.scale), ("dgn2w", gn2.weight), ("dgn2b", gn2.bias), ("dgn1w", gn1.weight), ("dgn1b", gn1.bias)):
        lo, hi = R.SEG[name]
        assert float((partial.sum(0)[lo:hi] - prm.grad).abs().max()) <= 1e-12 * scale(prm.grad), name
    auto = {"dw2": conv2.weight.grad[:, :, 0], "db2": conv2.bias.grad, "dw1": conv1.weight.grad, "db1": conv1.bias.grad}
    w = R.wgrad(inp, case.dil, b["dz"], f["a_out"], b["dh"], rounding=False)
    for k, v in auto.items():
        assert float((w[k] - v).abs().max()) <= 1e-12 * scale(v), k
    # with the GEMM's operand rounding (a, x to bf16, 8 significant bits): 2^-8 of every term
    w = R.wgrad(inp, case.dil, b["dz"], f["a_out"], b["dh"])
    for k, v in auto.items():
        assert bool(((w[k] - v).abs() <= 2.0 ** -8 * w["mag:" + k] + 1e-12 * scale(v)).all()), k


def test_floors():
    """FLOORS is the measurement, rounded up to the next quarter: not below it, and not a figure picked to pass"""
    fl = {}
    for case in CASES:
        for bwd in (False, True):
            inp, got, how = _evaluated(case, bwd)
            d = fl.setdefault(case.klass(bwd), {})
            for k, (v, _) in _judge(case, bwd, inp, got, how, measure=True).items():
                d[k] = max(d.get(k, 0.0), v)
    assert set(fl) == set(R.FLOORS)
    for kl, d in fl.items():
        print(kl, {k: round(v, 3) for k, v in d.items()})
    for kl, d in fl.items():
        assert set(d) == set(R.FLOORS[kl]), kl
        for k, v in d.items():
            assert v <= R.FLOORS[kl][k], (kl, k, v)
            assert R.FLOORS[kl][k] <= max(0.25, 1.5 * v + 0.25), (kl, k, v)
    assert R.FLOORS_WGRAD == {"dw2": GEMM_FLOORS["wgrad_bf16"]["dw"], "db2": GEMM_FLOORS["wgrad_bf16"]["db"],
                              "dw1": GEMM_FLOORS["wgrad_bf16"]["dw"], "db1": GEMM_FLOORS["wgrad_bf16"]["db"]}


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_is_inside_the_bound(case, bwd):
    """the bound has power only if it is a bound: Kern32 passes every case, worst error / bound <= 1 for every output"""
    inp, got, how = _evaluated(case, bwd)
    res = _judge(case, bwd, inp, got, how)
    print(case.id, "bwd" if bwd else "fwd", {k: round(q, 3) for k, (q, _) in res.items()})
    assert set(res) == set(R.BWD_OUT if bwd else R.FWD_OUT)
    assert all(q <= 1.0 for q, _ in res.values()), res


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_no_bound_rests_on_the_absolute_allowance(case):
    """the one absolute allowance, TINY on the bf16-stored outputs: at most 0.1 % of the elements of an output may have a bound of
    which it is more than a thousandth -- asserted on the reference's own values.  (No element is excluded from any comparison.)"""
    inp = R.make_inputs(case)
    sel = case.cpu_sel()
    sub = R.take(inp, sel)
    f = R.forward(sub, case.dil, R.Exact, True)
    b = R.backward(sub, case.dil, R.Exact, True)
    K = {**R.K_of(case.klass(False)), **R.K_of(case.klass(True))}
    for name, ref in (("h16", f), ("z16", f), ("dz", b), ("dh", b)):
        _, t = R._tol(name, ref, K[name])
        share = float((R.TINY > 1e-3 * t).double().mean())
        assert share <= 1e-3, (name, share)


# fault -> (the case that names the edge, backward?  None: both directions)
_PLANT = {
    "dil_1_on_one_tap": (R.Case(3, 2), False),
    "stale_zero_rows": (R.Case(513, 2), False),
    "stale_image": (R.Case(513, 1), False),
    "rows_12_15_next_sample": (R.Case(2, 1), None),              # both directions
    "stats1_one_wave": (R.Case(1, 1), False),
    "glu_swapped": (R.Case(2, 1), False),
    "scale_from_neighbour": (R.Case(1, 2), False),
    "b2_gate_from_value": (R.Case(1, 2), False),
    "dz_pairs_swapped": (R.Case(3, 2), True),
    "dead_sample_dgn2b": (R.Case(513, 1), True),
    "partial_last_row_missing": (R.Case(3, 2), True),
    "dgn1_segments_exchanged": (R.Case(2, 1), True),
    "means_over_parked": (R.Case(513, 1), True),
    "truncating_store": (R.Case(2, 1), True),
    "one_ulp_h16": (R.Case(2, 1), False),
    "one_ulp_z16": (R.Case(3, 2), False),
    "one_ulp_dz": (R.Case(3, 2), True),
    "one_ulp_dh": (R.Case(2, 1), True),
}


def _planted(fault, case, bwd):
    inp = R.make_inputs(case)
    if bwd:
        rows = case.cpu_rows()
        got, need = R.kern32_backward(inp, case.dil, rows, mutate=fault)
        return _judge(case, True, inp, got, {"sel": need, "rows": rows})
    sel = case.cpu_sel()
    return _judge(case, False, R.take(inp, sel), R.kern32_forward(inp, case.dil, sel, mutate=fault), {})


@pytest.mark.parametrize("fault", list(R.MUTATIONS))
def test_bound_rejects_planted_fault(fault):
    assert set(_PLANT) == set(R.MUTATIONS)
    case, bwd = _PLANT[fault]
    res = {}
    for d in ((False, True) if bwd is None else (bwd,)):
        res.update({k: v for k, v in _planted(fault, case, d).items() if v[0] > res.get(k, (0.0,))[0]})
    caught = {k: round(q, 2) for k, (q, _) in res.items() if not q <= 1.0}
    print(f"{fault} at {case.id}: rejected by {caught}")
    missing = [k for k in R.MUTATIONS[fault] if k not in caught]
    assert not missing, (fault, "not rejected by", missing, {k: round(q, 3) for k, (q, _) in res.items()})


def test_case_table_reaches_the_walks():
    """what the issue's table is for, asserted on the restated launch geometry"""
    cs = {(c.N, c.dil) for c in CASES}
    assert {(1, 1), (1, 2), (2, 1), (3, 2), (513, 1), (513, 2), (514, 1)} <= cs
    assert any(c.bias for c in CASES)
    assert R.grid_fwd(513) == 512 and R.bwd_rows(513) == 256 and R.bwd_rows(514) == 256
    assert R.wg_samples(1, 0) == [0] and R.wg_samples(3, 1) == [2]
    assert R.wg_samples(513, 0) == [0, 1, 512] and R.wg_samples(514, 0) == [0, 1, 512, 513] and R.wg_samples(513, 255) == [510, 511]
    assert [R.bwd_rows(n) for n in (1, 2, 3, 511, 512, 513, 100000)] == [1, 1, 2, 256, 256, 256, 256]
    for N in (1, 2, 3, 513, 514):
        assert sorted(n for wg in range(R.bwd_rows(N)) for n in R.wg_samples(N, wg)) == list(range(N))
