"""CPU: what tests/cldconv_ref.py (the reference of tests/test_gpu_cldconv_kernel.py) is worth.  With rounding off it agrees with torch
float64 autograd over the plain composition; the floors its K come from are re-measured here (the fp32 restatement with the kernels'
partial sums against fp64, never the kernel); every case's bound has power; the case table reaches every launched instantiation; and
every planted fault is rejected by the GPU test's own tolerance -- with a record of which of them the whole-tensor assertion of
tests/test_gpu_cldconv.py would have accepted."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import cldconv_ref as R

ALL_CASES = R.forward_cases() + R.backward_cases()
_CACHE = {}


def _evaluated(case):
    """(inputs, fp32 restatement's outputs, staged references) of a case, computed once"""
    if case not in _CACHE:
        inp = R.make_inputs(case)
        if case.bwd:
            sv = R.saved_tensors(inp, case.dil)
            got = R.backward(inp, sv, case.dil, case.passes, R.Kern32, True, grid=case.g)
            _CACHE[case] = (inp, got, R.stage_backward(inp, sv, case.dil, case.passes, got, case.g))
        else:
            got = R._got_forward(R.kern32_forward(inp, case.dil, grid=case.g))
            _CACHE[case] = (inp, got, R.stage_forward(inp, case.dil, got))
    return _CACHE[case]


@pytest.mark.parametrize("case", [R.Case(48, 2, 3, 2, 3), R.Case(96, 1, 1, 3, 2), R.Case(48, 1, 1, 3, 2, sat=True)], ids=lambda c: c.id)
def test_reference_agrees_with_autograd(case):
    inp = R.make_inputs(case)
    d = {k: v.double().requires_grad_(True) for k, v in inp.items()}
    eps = float(torch.tensor(R.GEN_EPS, dtype=torch.float32))
    x = d["x"].transpose(1, 2)
    h = F.conv1d(x, d["W1"], d["b1"], dilation=case.dil, padding=case.dil)
    a = F.gelu(F.group_norm(h, 1, d["g1w"], d["g1b"], eps))
    z = F.conv1d(a, d["W2"][:, :, None], d["b2"])
    y = x + d["scale"][None, :, None] * F.glu(F.group_norm(z, 1, d["g2w"], d["g2b"], eps), 1)
    (y * d["gy"].transpose(1, 2)).sum().backward()
    f = R.forward(inp, case.dil, R.Exact, False)
    scale = lambda t: float(t.detach().abs().max())             # noqa: E731
    assert float((f["y"] - y.detach().transpose(1, 2)).abs().max()) <= 1e-12 * scale(y)
    sv = {"a": f["a"], "hpre": f["h"], "stats": torch.stack([f["mean1"], f["rstd1"], f["mean2"], f["rstd2"]], 1)}
    for passes in (False, True):
        b = R.backward(inp, sv, case.dil, passes, R.Exact, False)
        for k, n in (("dx", "x"), ("dw1", "W1"), ("db1", "b1"), ("dw2", "W2"), ("db2", "b2"), ("dscale", "scale"), ("dgn2w", "g2w"),
                     ("dgn2b", "g2b"), ("dgn1w", "g1w"), ("dgn1b", "g1b")):
            assert float((b[k] - d[n].grad).abs().max()) <= 1e-12 * scale(d[n].grad), (k, passes)


def test_floors():
    """FLOORS is the measurement, rounded up to the next quarter: not below it, and not a figure picked to pass"""
    fl = {}
    for case in ALL_CASES:
        inp, got, st = _evaluated(case)
        m = R.measure(R.BWD_OUT if case.bwd else R.FWD_OUT, st, got)
        d = fl.setdefault(case.klass, {})
        for k, v in m.items():
            d[k] = max(d.get(k, 0.0), v)
    assert set(fl) == set(R.FLOORS)
    for kl, d in fl.items():
        print(kl, {k: round(v, 3) for k, v in d.items()})
        for k, v in d.items():
            assert v <= R.FLOORS[kl][k], (kl, k, v)
            assert R.FLOORS[kl][k] <= max(0.25, 1.5 * v + 0.25), (kl, k, v)


# The issue's condition -- the fp32 slack K eps32 magnitude below half a bf16 ulp of the ELEMENT, so that the whole bound is under one ulp --
# cannot hold at an element whose terms cancel: ulp(ref) > |ref| 2^-8, so it holds wherever magnitude / |ref| < 2^14 / K and fails only
# beyond that fold (a zero crossing has an ulp as small as one likes, which no fp32 sum of terms of size 1 can follow).  It is asserted
# (1) for EVERY element below a fold of FOLD, which holds K of every bf16-stored output under 2^14 / FOLD; (2) as a ceiling on the share
# of elements that miss it, per output; (3) in absolute terms: the slack of every element is below half an ulp at the output's RMS.
# The ceilings are the largest share over the case table, measured on the fp64 reference (a property of the inputs and of K, not of any
# kernel), rounded up: y, dx 0.12 %; hpre 0.32 %; a 3.5 %; dz 3.8 %; dh 6.5 %, and 14.4 % for the pass form at TPS = 1, whose K is 32
# where the others' is 10 - 12.  dh and dz cancel most because their magnitudes carry the two sample means' own error, the same for
# every element, next to values that pass through zero.
FOLD = 400.0
SHARE = {"hpre": 0.5, "a": 4.0, "y": 0.25, "dz": 4.5, "dh": 7.5, "dx": 0.25}
SHARE_PASS_TPS1 = {"dh": 16.0}
# dz with saturated gates: the x 60 gate weights sit in the magnitude of both sample means and so in every element's, value half
# included, while most of the gate half is nearly 0.  Its halves are judged apart with ceilings of their own (measured: 47.5 % of the
# value half, 90.0 % of the gate half).  The value half meets (1), (2) and (3) at its own RMS.  The gate half meets (1) and (2) only: its
# RMS is that of the few gates that are not saturated, and the slack reaches 2.3 half-ulps there.  What pins a saturated gate's dz is
# that it is nearly 0 inside a bound that is small next to the value half, not one under its own ulp: its slack is asserted below 1/32
# of the value half's RMS (measured: 0.005 and 0.023 of it).
SHARE_SAT_DZ = {"value": 52.0, "gate": 93.0}


# y / dx against the branch: the RMS of the bound is under 1/64 of the RMS of the branch.  Element by element it cannot be: the branch's
# RMS is 0.56 - 1.6 (y) and 0.31 - 1.6 (dx), a 64th of it 0.005 - 0.025, and half a bf16 ulp of a stored element of size 2 is 0.0078
# whatever computed it.  The share of elements whose own bound is above that 64th is held to a ceiling (measured: y 1.9 %, dx 11.5 %).
BRANCH_SHARE = {"y": 2.5, "dx": 12.5}


def _power(ref, slack, mag, K, ceiling, what, at_rms=True):
    rms = float(ref.double().pow(2).mean().sqrt())
    ulp = R.ulp(ref, 7)
    miss = slack >= 0.5 * ulp
    share = 100.0 * float(miss.double().mean())
    print(f"{what}: K {K:.0f}; slack / half an ulp at the RMS {float(slack.max()) / (0.5 * float(R.ulp(torch.tensor(rms), 7))):.3f}; "
          f"slack above half the element's own ulp in {share:.2f} % (ceiling {ceiling} %)")
    assert not at_rms or float(slack.max()) < 0.5 * float(R.ulp(torch.tensor(rms), 7)), what
    below = mag < FOLD * ref.abs()
    assert not bool((miss & below).any()), f"{what}: an element that cancels less than {FOLD:.0f}-fold has a bound of an ulp or more"
    assert K < 2.0 ** 14 / FOLD, (what, K)
    assert share <= ceiling, (what, share)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: ("bwd-" if c.bwd else "fwd-") + c.id)
def test_every_case_has_power(case):
    """every bf16-stored output: the three assertions above.  y / dx: the bound stays under 1/64 of the branch alone (y - x, dx - gy),
    RMS against RMS -- per element the branch passes through zero like anything else"""
    inp, got, st = _evaluated(case)
    K = R.K_of(case)
    rms = lambda t: float(t.double().pow(2).mean().sqrt())      # noqa: E731
    for n in (R.BF16_STORED[3:] if case.bwd else R.BF16_STORED[:3]):
        ref, mag = st[n][R._PRE[n]], st[n]["mag:" + n]
        slack = K[n] * R.EPS32 * mag
        if case.sat and n == "dz":
            for half, sl in (("value", slice(0, case.C)), ("gate", slice(case.C, 2 * case.C))):
                _power(ref[..., sl], slack[..., sl], mag[..., sl], K[n], SHARE_SAT_DZ[half], f"{case.id} dz, {half} half", at_rms=half == "value")
            assert float(slack[..., case.C:].max()) < rms(ref[..., :case.C]) / 32.0
            continue
        ceiling = SHARE_PASS_TPS1.get(n, SHARE[n]) if case.klass == "bwd-tps1-pass" else SHARE[n]
        _power(ref, slack, mag, K[n], ceiling, f"{case.id} {n}")
    n, base = ("dx", inp["gy"]) if case.bwd else ("y", inp["x"])
    ref, tol = R._tol(n, st[n], K[n])
    branch = rms(ref - base.double())
    over = 100.0 * float((tol >= branch / 64.0).double().mean())
    print(f"{case.id} {n}: RMS of the bound / RMS of the branch {rms(tol) / branch:.5f} (1/64 = 0.01563); bound of an element above 1/64 of the "
          f"branch's RMS in {over:.2f} % (ceiling {BRANCH_SHARE[n]} %)")
    assert rms(tol) < branch / 64.0, (rms(tol), branch)
    assert over <= BRANCH_SHARE[n], (n, over)


def test_case_table_reaches_every_form():
    """the literal list of what rfx_cl_dconv_fwd / rfx_cl_dconv_bwd can launch against the union over the case table"""
    every = {f"fwd<{C},{C // 4},{ph}>" for C in (48, 96) for ph in (0, 1, 2, 3)} | {"stats", "bwd8<48,12>", "bwd<48,12>", "means", "dh", "pgrad",
                                                                                "cl_conv:dx", "cl_wgrad"} | \
        {f"bwdp<{C},{C // 4},{p}>" for C in (48, 96) for p in (1, 2)}
    seen, G, walks = set(), set(), set()
    for c in ALL_CASES + R.four_wave_cases():
        names, st = c.forms()
        seen |= set(names)
        if c.bwd:
            G.add(st["G"])
        walks.add((st["walk"], st["odd_walk"]))
    assert seen == every, (seen ^ every)
    assert {1, 2, 3, 256} <= G
    assert {(1, True), (2, False)} <= walks                      # one tile per workgroup; two, the second without a successor
    assert any(c.nsamp * c.TPS % min(c.g, c.nsamp * c.TPS) for c in ALL_CASES)     # workgroups of one launch walk different numbers of tiles
    assert {c.TPS for c in ALL_CASES if c.bwd and c.C == 96} == {1, 2, 3} and {c.TPS for c in ALL_CASES if c.bwd and c.C == 48} == {1, 2, 3}
    assert any(c.sat for c in R.forward_cases()) and any(c.sat for c in R.backward_cases())


# fault -> (the case that names the edge, forward?)
_FAULT_CASE = {
    "tap_missing_tile_edge": (R.Case(48, 2, 3, 2, 3), True),
    "halo_from_previous_sample": (R.Case(96, 1, 1, 3, 2), True),
    "stale_buffer": (R.Case(48, 1, 1, 3, 2), True),
    "dil_1_on_one_tap": (R.Case(96, 2, 2, 2, 0), True),
    "stats_one_tile": (R.Case(96, 1, 3, 2, 0), True),
    "scale_from_neighbour": (R.Case(48, 1, 1, 1, 0), True),
    "glu_swapped": (R.Case(96, 2, 1, 1, 0), True),
    "pad_channel_nonzero": (R.Case(48, 1, 1, 1, 0), True),
    "dgn1w_missing_workgroup": (R.Case(96, 1, 3, 2, 3, bwd=True), False),
    "truncating_store": (R.Case(48, 2, 1, 3, 2), True),
    "one_ulp": (R.Case(96, 1, 2, 2, 3, bwd=True), False),
}
# one_ulp again where the bound is K eps32 magnitude + ONE half-ulp -- y, and the one-pass form's dx -- so that a whole ulp is outside
# it at every element test_every_case_has_power does not count among the cancelling ones.  The pass form's dx above carries the staged
# convolution's half-ulp too: there (and on dz, and the pass form's dh) the bound is about one ulp and the fault is rejected at the
# element chosen, not everywhere
_MORE_CASES = {"one_ulp": ((R.Case(48, 2, 1, 3, 2), True), (R.Case(48, 1, 1, 3, 2, bwd=True), False))}
_PLANTED = [(f, c, w) for f in R.MUTATIONS for c, w in (_FAULT_CASE[f],) + _MORE_CASES.get(f, ())]
# what the whole-tensor assertion of tests/test_gpu_cldconv.py (rel L2 < 4e-3 for y / dx, < 5e-3 for a parameter gradient, e16 = 0)
# does with each fault on the same inputs; test_bound_rejects_planted_fault asserts this record
OLD_ACCEPTS = {"tap_missing_tile_edge": False, "halo_from_previous_sample": False, "stale_buffer": False, "dil_1_on_one_tap": False,
               "stats_one_tile": False, "scale_from_neighbour": False, "glu_swapped": False, "pad_channel_nonzero": True,
               "dgn1w_missing_workgroup": False, "truncating_store": False, "one_ulp": True}


@pytest.mark.parametrize("fault,case,fwd", _PLANTED, ids=[f if (c, w) == _FAULT_CASE[f] else f"{f}-{'y' if w else 'dx'}-{c.id}" for f, c, w in _PLANTED])
def test_bound_rejects_planted_fault(fault, case, fwd):
    inp, clean, _ = _evaluated(case)
    K = R.K_of(case)
    H = case.C // 4
    if fault == "pad_channel_nonzero":
        a = F.pad(clean["a"].to(torch.bfloat16), (0, 16 - H))
        assert R.pad_is_zero(a, H)
        a[0, 5, H] = 1e-3
        assert not R.pad_is_zero(a, H)
        old = 0.0                                                # the old assertion looks at no stored tensor
    elif fwd:
        got = R._got_forward(R.kern32_forward(inp, case.dil, mutate=fault, grid=case.g))
        res = R.judge(R.FWD_OUT, R.stage_forward(inp, case.dil, got), got, K)
        assert max(q for q, _ in res.values()) > 1.0, res
        old = R.old_rel(got["y"], clean["y"])
        lim = 4e-3
    else:
        sv = R.saved_tensors(inp, case.dil)
        got = R.backward(inp, sv, case.dil, case.passes, R.Kern32, True, mutate=fault, grid=case.g)
        res = R.judge(R.BWD_OUT, R.stage_backward(inp, sv, case.dil, case.passes, got, case.g), got, K)
        assert max(q for q, _ in res.values()) > 1.0, res
        old, lim = (R.old_rel(got["dgn1w"], clean["dgn1w"]), 5e-3) if fault.startswith("dgn1w") else (R.old_rel(got["dx"], clean["dx"]), 4e-3)
    accepts = True if fault == "pad_channel_nonzero" else old < lim
    print(f"{fault}: at {case.id}; whole-tensor figure {old:.2e} -> the old assertion {'ACCEPTS' if accepts else 'rejects'} it")
    assert accepts == OLD_ACCEPTS[fault], (fault, old)


def test_clean_restatement_is_inside_the_bound():
    """the same judgement accepts the unmutated restatement (a bound that rejects everything rejects the faults too)"""
    for case in (R.Case(48, 2, 3, 2, 3), R.Case(96, 1, 3, 2, 3, bwd=True), R.Case(48, 1, 1, 3, 2, bwd=True)):
        inp, got, st = _evaluated(case)
        res = R.judge(R.BWD_OUT if case.bwd else R.FWD_OUT, st, got, R.K_of(case))
        assert max(q for q, _ in res.values()) <= 1.0, res
        assert math.isfinite(max(q for q, _ in res.values()))
