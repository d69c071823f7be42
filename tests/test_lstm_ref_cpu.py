"""tests/lstm_ref.py is right, and the bound tests/test_gpu_lstm_kernel.py derives from it can tell a wrong recurrence from a right
one.  No GPU: everything here is the reference against torch.nn.LSTM, against itself, and against deliberately wrong copies."""
import functools

import pytest
import torch
import torch.nn as nn

from tests import lstm_ref as R


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("Bn", [1, 5])
def test_exact_mode_is_torch_lstm(H, T, Bn):
    """Forward outputs, and every gradient derived from dG by plain matmuls (dx, dW_ih, dW_hh, biases), against autograd through
    nn.LSTM in fp64, to 1e-12 relative."""
    torch.manual_seed(H + T + Bn)
    Cin = 24
    m = nn.LSTM(Cin, H, bidirectional=True).double()
    x = torch.randn(T, Bn, Cin, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(T, Bn, 2 * H, dtype=torch.float64)
    y = m(x)[0]
    (y * gy).sum().backward()
    P = T * Bn
    xc = x.detach().permute(2, 0, 1).reshape(Cin, P)
    sfx = ("", "_reverse")
    w_ih = [getattr(m, "weight_ih_l0" + s).detach() for s in sfx]
    w_hh = [getattr(m, "weight_hh_l0" + s).detach() for s in sfx]
    b = [(getattr(m, "bias_ih_l0" + s) + getattr(m, "bias_hh_l0" + s)).detach() for s in sfx]
    xp = torch.stack([w_ih[d] @ xc + b[d][:, None] for d in range(2)])
    out, gates, cst = R.forward(xp, w_hh[0], w_hh[1], T, Bn, "exact")
    assert _rel(out, y.detach().permute(2, 0, 1).reshape(2 * H, P)) < 1e-12
    gout = gy.permute(2, 0, 1).reshape(2 * H, P)
    dG = R.backward(gout, gates, cst, w_hh[0], w_hh[1], T, Bn, "exact")
    dx = sum(w_ih[d].t() @ dG[d] for d in range(2))
    assert _rel(dx, x.grad.permute(2, 0, 1).reshape(Cin, P)) < 1e-12
    for d in range(2):
        assert _rel(dG[d] @ xc.t(), getattr(m, "weight_ih_l0" + sfx[d]).grad) < 1e-12
        assert _rel(dG[d].sum(1), getattr(m, "bias_ih_l0" + sfx[d]).grad) < 1e-12
        assert _rel(dG[d].sum(1), getattr(m, "bias_hh_l0" + sfx[d]).grad) < 1e-12
        if T > 1:
            # h of the step before in the processing order: t - 1 (forward), t + 1 (reverse)
            h = out[d * H:(d + 1) * H].view(H, T, Bn)
            g = dG[d].view(4 * H, T, Bn)
            hp, gs = (h[:, :-1], g[:, 1:]) if d == 0 else (h[:, 1:], g[:, :-1])
            assert _rel(gs.reshape(4 * H, -1) @ hp.reshape(H, -1).t(), getattr(m, "weight_hh_l0" + sfx[d]).grad) < 1e-12
        else:
            assert float(getattr(m, "weight_hh_l0" + sfx[d]).grad.abs().max()) == 0.0


def test_operand_splits_are_the_kernels():
    """The bit rules of lstm.hip on values where they differ: RNE ties go to even, split_hi_lo truncates hi and rounds lo half-up."""
    f = lambda bits: torch.tensor(bits, dtype=torch.int32).view(torch.float32).double()          # noqa: E731
    x = f([0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F808001, 0xBF808000 - (1 << 32)])
    assert R.bf16_rne(x).float().view(torch.int32).tolist() == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F810000, 0xBF800000 - (1 << 32)]
    assert R.bf16_trunc(x).float().view(torch.int32).tolist() == [0x3F800000, 0x3F810000, 0x3F800000, 0x3F800000, 0xBF800000 - (1 << 32)]
    v = torch.randn(4096, dtype=torch.float64).float().double()
    hi, lo = R.split_hi_lo(v)
    assert torch.equal(hi, R.bf16_trunc(v)) and float(((hi + lo) - v).abs().max() / v.abs().max()) < 2.0 ** -15
    assert bool((((v - hi) * v) >= 0).all())                                    # truncation: the residual has the sign of v
    whi, wlo = R.split_w(v)
    assert torch.equal(whi, R.bf16_rne(v)) and torch.equal(wlo, R.bf16_rne(v.float() - whi.float()))


# the GPU test's own H = 192 and H = 96 cases (tests/test_gpu_lstm_kernel.py): tile edge of both forms, ring wrap, ping-pong start,
# one clip's layer-4 frame
CASES = [(192, 6, 17), (192, 6, 65), (192, 2, 3), (192, 200, 3), (96, 5, 33), (96, 2, 5), (96, 3, 5)]


@functools.lru_cache(maxsize=None)
def _case(H, T, Bn, mode):
    xp, w0, w1, gout = R.make_inputs(H, T, Bn)
    ref, fl = R.floors(R.forward_case(xp, w0, w1, T, Bn, mode), mode, H, "out")
    gs, cs = ref["gates"].float(), ref["cstate"].float()                        # what a kernel would have saved
    refb, flb = R.floors(R.backward_case(gout, gs, cs, w0, w1, T, Bn, mode), mode, H, "dG")
    return (xp, w0, w1, gout, gs, cs), {"fwd": ref, "bwd": refb}, {"fwd": fl, "bwd": flb}


def _run(inputs, T, Bn, mode, sweep, **kw):
    xp, w0, w1, gout, gs, cs = inputs
    if sweep == "fwd":
        return R.forward_case(xp, w0, w1, T, Bn, mode, **kw)(0.0, False)
    return R.backward_case(gout, gs, cs, w0, w1, T, Bn, mode, **kw)(0.0, False)


@pytest.mark.parametrize("H,T,Bn", CASES)
@pytest.mark.parametrize("sweep", ["fwd", "bwd"])
def test_noise_floor_is_a_tenth_of_the_operand_rounding(H, T, Bn, sweep):
    """Condition on the inputs: the floor of every compared tensor is below a tenth of the distance between the bf16 and the exact
    reference (with 3 x the weights it is not: 3.6e-4 against 1.2e-3 at H = 192, T = 200 -- saturation comes from xp instead)."""
    inputs, ref, fl = _case(H, T, Bn, "bf16")
    dist = R.differences(ref[sweep], _run(inputs, T, Bn, "exact", sweep), H)
    for k in dist:
        print(f"{k}: floor {fl[sweep][k][0]:.2e} distance {dist[k][0]:.2e}")
        assert fl[sweep][k][0] < 0.1 * dist[k][0], (k, fl[sweep][k], dist[k])


@pytest.mark.parametrize("H,T,Bn", CASES)
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("sweep", ["fwd", "bwd"])
def test_fp32_copy_of_the_reference_meets_the_bound(H, T, Bn, mode, sweep):
    """The same arithmetic carried in fp32 (torch's correctly rounded activations, its own summation order) is inside the bound the GPU
    test uses -- with room: a bound an honest fp32 kernel cannot meet would say nothing about a failing one."""
    inputs, ref, fl = _case(H, T, Bn, mode)
    got = R.differences(ref[sweep], _run(inputs, T, Bn, mode, sweep, dtype=torch.float32), H)
    for k in got:
        for e, f in zip(got[k], fl[sweep][k]):
            assert e < 0.5 * R.bound(f), (k, got[k], fl[sweep][k])


MUTANTS = [(m, mode, sweep) for m, (modes, sweeps) in R.MUTATIONS.items() for mode in modes for sweep in sweeps]


@pytest.mark.parametrize("H,T,Bn", CASES)
@pytest.mark.parametrize("mutation,mode,sweep", MUTANTS)
def test_mutation_clears_the_bound(H, T, Bn, mutation, mode, sweep):
    """Every listed fault moves at least one of the quantities the GPU test compares (relative L2 or max-abs, per tensor and
    direction) past MARGIN x floor + FP32_TERM of that quantity, i.e. the GPU test would fail on a kernel that had it."""
    inputs, ref, fl = _case(H, T, Bn, mode)
    got = R.differences(ref[sweep], _run(inputs, T, Bn, mode, sweep, mutate=mutation), H)
    ratio = max(e / R.bound(f) for k in got for e, f in zip(got[k], fl[sweep][k]))
    print(f"{mutation} {mode} {sweep}: largest difference / bound = {ratio:.1f}")
    assert ratio > 1.0, (mutation, got, fl[sweep])
    if mutation == "reverse_starts_late":                                       # ... and only where the fault is
        assert all(got[k] == (0.0, 0.0) for k in got if k.endswith(".d0"))


# ---- the parameter glue (rfx_lstm_cat_params, rfx_lstm_grad_scatter) ----------------------------------------------------------------
def _once(t64):
    return t64.float()


@pytest.mark.parametrize("H,Cin", R.GLUE_CASES)
def test_glue_reference_is_cat_and_add(H, Cin):
    p, d, g0 = R.glue_data(H, Cin)
    ref = R.cat_params(p)
    assert torch.equal(_once(ref["wcat"]).view(8 * H, Cin), torch.cat([p["w_ih"].view(4 * H, Cin), p["w_ih_r"].view(4 * H, Cin)], 0))
    assert torch.equal(_once(ref["bcat"]), torch.cat([p["b_ih"] + p["b_hh"], p["b_ih_r"] + p["b_hh_r"]]))
    after = R.grad_scatter(g0, d)
    dw, db = d["dwcat"].view(2, 4 * H * Cin), d["dbcat"].view(2, 4 * H)
    for k, add in (("w_ih", dw[0]), ("w_ih_r", dw[1]), ("b_ih", db[0]), ("b_hh", db[0]), ("b_ih_r", db[1]), ("b_hh_r", db[1])):
        assert torch.equal(_once(after[k]), g0[k] + add), k
    # every buffer differs from every other of its size and nothing the gradients start from is zero
    for group in (("w_ih", "w_ih_r"), ("b_ih", "b_hh", "b_ih_r", "b_hh_r")):
        for i, a in enumerate(group):
            assert bool((g0[a] != 0).all())
            for b in group[i + 1:]:
                assert not torch.equal(p[a], p[b]) and not torch.equal(g0[a], g0[b])


@pytest.mark.parametrize("mutation", R.GLUE_MUTATIONS)
def test_glue_mutation_is_not_one_rounding_of_the_reference(mutation):
    """bound 0 = the fp32 rounding of the fp64 value, bit for bit: each planted fault differs from it"""
    H, Cin = 3, 5
    p, d, g0 = R.glue_data(H, Cin)
    same = lambda a, b: all(torch.equal(_once(a[k]), _once(b[k])) for k in a)            # noqa: E731
    assert not (same(R.cat_params(p, mutation), R.cat_params(p)) and same(R.grad_scatter(g0, d, mutation), R.grad_scatter(g0, d)))


def test_glue_case_table_reaches_the_stride_loop():
    forms = {c: R.forms_glue(*c) for c in R.GLUE_CASES}
    assert "stride_loop" in forms[(192, 192)] and 2 * 4 * 192 * 192 == 294912 > R.GLUE_GRID
    assert all("stride_loop" not in forms[c] for c in R.GLUE_CASES[:3])
    assert "ragged_last_block" in forms[(1, 1)] and "ragged_last_block" in forms[(3, 5)] and "ragged_last_block" not in forms[(64, 48)]
    assert R.forms_glue(0, 4) is None and R.forms_glue(4, 0) is None
