"""CPU side of the complex-domain / optimiser kernel pins: ties tests/cplx_ref.py to oracle.ref_dcunet and to torch's float64 autograd,
tests/optim_ref.py to torch.optim.AdamW, walks the case tables of tests/test_gpu_cplx_kernel.py / test_gpu_optim_kernel.py over the
dispatch of the kernels, and holds the two properties that keep the per-element bound from being vacuous: no bound above 1e-3 of its
output's scale, and at most 1e-4 of a case's elements inside the leaky-ReLU sign band.  Floors are in DESIGN.md 4.20."""
import math

import pytest
import torch

from tests import cplx_ref as R
from tests import optim_ref as O


def _module(C, seed, train):
    from oracle import ref_dcunet
    g = torch.Generator().manual_seed(seed)
    bn = ref_dcunet.ComplexBatchNorm(C).double()
    with torch.no_grad():
        bn.Wrr.copy_(0.5 + torch.rand(C, generator=g)); bn.Wri.copy_(torch.rand(C, generator=g) * 1.8 - 0.9); bn.Wii.copy_(0.5 + torch.rand(C, generator=g))
        bn.Br.copy_(torch.randn(C, generator=g) * 0.3); bn.Bi.copy_(torch.randn(C, generator=g) * 0.3)
        bn.RMr.copy_(torch.randn(C, generator=g) * 0.05); bn.RMi.copy_(torch.randn(C, generator=g) * 0.05)
        bn.RVrr.copy_(torch.rand(C, generator=g) * 0.5 + 0.75); bn.RVii.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
        bn.RVri.copy_(torch.randn(C, generator=g) * 0.05)
    bn.train(train)
    return bn, g


def _running(bn):
    return torch.stack([bn.RMr, bn.RMi, bn.RVrr, bn.RVri, bn.RVii]).detach().clone()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
def test_chain_matches_oracle_and_autograd(train):
    """moments -> coef_fwd -> affine_act is oracle.ref_dcunet.ComplexBatchNorm + LeakyReLU in .double() (1e-12, all five running buffers
    after one step); affine_act_bwd -> coef_bwd -> moments_bwd is its float64 autograd for x, Wrr, Wri, Wii, Br, Bi (1e-10); eval: no cm"""
    import torch.nn.functional as F
    N, C, H, Wd = 3, 5, 7, 11
    bn, g = _module(C, 5, train)
    x = (torch.randn(N, 2 * C, H, Wd, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    run0 = _running(bn)
    y = bn(torch.complex(x[:, :C], x[:, C:]))
    y = torch.cat([F.leaky_relu(y.real, R.SLOPE), F.leaky_relu(y.imag, R.SLOPE)], 1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    xs, gys = x.detach().reshape(N, 2 * C, -1), gy.reshape(N, 2 * C, -1)
    W, B = (bn.Wrr.detach(), bn.Wri.detach(), bn.Wii.detach()), (bn.Br.detach(), bn.Bi.detach())
    inv = 1.0 / (N * H * Wd)
    slope = R.SLOPE                                              # the fp64 chain takes the double, not its fp32 rounding
    if train:
        coef, st, run = R.coef_fwd((R.moments(xs), inv), W, B, bn.eps, run0, bn.momentum)
        # the oracle's lerp weight is the double 0.1, the ABI's the float: compare with the double
        run = run0 + bn.momentum * (st - run0)
        assert _rel(run, _running(bn)) < 1e-12
    else:
        coef, st, _ = R.coef_fwd(run0, W, B, bn.eps)
    k = [c.view(1, -1, 1) for c in coef]
    a, b = R.halves(xs)
    ur, ui = k[0] * a + k[1] * b + k[4], k[2] * a + k[3] * b + k[5]
    yy = torch.cat([torch.where(ur >= 0, ur, slope * ur), torch.where(ui >= 0, ui, slope * ui)], 1)
    assert _rel(yy, y.detach().reshape(N, 2 * C, -1)) < 1e-12
    assert _rel(R.affine_act(xs, coef), yy) < 1e-8                # the ABI's slope is fl32(0.01)
    gr, gi = R.halves(gys)
    one, sl = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)   # scalars alone would make it float32
    gr, gi = gr * torch.where(ur >= 0, one, sl), gi * torch.where(ui >= 0, one, sl)
    gx = torch.cat([k[0] * gr + k[2] * gi, k[1] * gr + k[3] * gi], 1)
    gcoef = torch.stack([t.sum((0, 2)) for t in (gr * a, gr * b, gi * a, gi * b, gr, gi)])
    gx32, gc32 = R.affine_act_bwd(xs, coef, gys)
    assert _rel(gx32, gx) < 1e-8 and _rel(gc32, gcoef) < 1e-8
    gw, cm = R.coef_bwd(st, W, bn.eps, gcoef, inv if train else None)
    assert (cm is not None) == train
    if train:
        gx = gx + R.moments_bwd(xs, cm)
    assert _rel(gx, x.grad.reshape(N, 2 * C, -1)) < 1e-10
    for i, p in enumerate((bn.Wrr, bn.Wri, bn.Wii, bn.Br, bn.Bi)):
        assert _rel(gw[i], p.grad) < 1e-10, i


def _mask_points(lo, hi, n=4000, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = R._log_uniform(n, lo, hi, g)
    ph = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    return a * torch.cos(ph), a * torch.sin(ph), g


def test_bound_mask_matches_oracle_autograd():
    """|m| in [1e-3, 20]: tanh(|m|) m / |m| * tf as oracle/ref_dcunet.py writes it, and its float64 autograd"""
    mr, mi, g = _mask_points(1e-3, 20.0)
    n = mr.numel()
    m = torch.complex(mr, mi).requires_grad_(True)
    tf = torch.complex(torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64))
    mag = m.abs()
    out = torch.tanh(mag) * m / mag * tf
    go = torch.complex(torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64))
    out.backward(go)
    st = lambda z: torch.stack([z.real, z.imag]).unsqueeze(0).detach()   # noqa: E731  (1, 2, n)
    got = R.bound_mask(st(m), st(tf))
    assert float((got - st(out)).abs().max()) < 1e-13
    gm = R.bound_mask_bwd(st(m), st(tf), st(go))
    assert float((gm - st(m.grad)).abs().max() / st(m.grad).abs().max()) < 1e-10      # autograd divides by |m|^2: 1e-16 / 1e-6


def test_phase_mask_matches_polar_form():
    """|x| in [1e-3, 20]: mag exp(i angle(x)) and its float64 autograd; exact 0 -> (mag, 0), gmag = g.re"""
    xr, xi, g = _mask_points(1e-3, 20.0, seed=1)
    n = xr.numel()
    mag = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
    xc = torch.complex(xr, xi)
    out = mag * torch.exp(1j * torch.angle(xc))
    go = torch.randn(n, 2, generator=g, dtype=torch.float64)
    out.backward(torch.complex(go[:, 0], go[:, 1]))
    x2 = torch.stack([xr, xi], 1)
    assert float((R.phase_mask(mag.detach(), x2) - torch.view_as_real(out.detach())).abs().max()) < 1e-13
    assert float((R.phase_mask_bwd(x2, go) - mag.grad).abs().max()) < 1e-13
    z = torch.zeros(3, 2, dtype=torch.float64)
    mg = torch.tensor([2.0, -3.0, 0.5], dtype=torch.float64)
    assert torch.equal(R.phase_mask(mg, z), torch.stack([mg, torch.zeros(3, dtype=torch.float64)], 1))
    assert torch.equal(R.phase_mask_bwd(z, go[:3]), go[:3, 0])


def test_small_argument_forms():
    """two independent fp64 formulations of k = tanh(a) / a and q = sech^2(a) - k: the truncated series of tanh (cplx_ref.tanhc below
    MASK_SMALL) and the expm1 form (cplx_ref.tanhc_expm1: tanh = -e / (2 + e), sech^2 = 4 (1 + e) / (2 + e)^2, e = expm1(-2 a)).
    a = 1e-30 ... 1e-4: k agrees to 4 eps64 and q to 1e-15 ABSOLUTE (the expm1 form cancels there, the series does not);
    a = 1e-4 ... MASK_SMALL, where that cancellation leaves digits: q agrees to 1e-15 / |q| relative, which pins the series' coefficients
    (the a^4 term of q is 5e-9 of it at 1e-2, the a^6 term 5e-13).  And the whole mask is finite with out -> m tf, gm -> g conj(tf)."""
    g = torch.Generator().manual_seed(2)
    a = R._log_uniform(20000, 1e-30, 1e-4, g)
    ks, qs, th = R.tanhc(a)
    ke, qe = R.tanhc_expm1(a)
    assert float((ks - ke).abs().max()) < 4 * 2.0 ** -52 and float((qs - qe).abs().max()) < 1e-15
    assert float((th / a - 1).abs().max()) < 1e-8
    a = R._log_uniform(20000, 1e-4, R.MASK_SMALL * (1 - 1e-12), g)
    ks, qs, _ = R.tanhc(a)
    ke, qe = R.tanhc_expm1(a)
    assert float((ks - ke).abs().max()) < 4 * 2.0 ** -52
    assert float(((qs - qe).abs() / (1e-15 + 1e-12 * qs.abs())).max()) < 1.0
    # either side of the switch
    a = torch.tensor([R.MASK_SMALL * (1 - 1e-9), R.MASK_SMALL * (1 + 1e-9)], dtype=torch.float64)
    k, q, th = R.tanhc(a)
    assert abs(float(k[0] - k[1])) < 1e-10 and abs(float(q[0] - q[1]) / float(q[0])) < 1e-7
    mr, mi, g = _mask_points(1e-30, 1e-4, seed=3)
    mr[::5] = 0.0
    mi[1::5] = 0.0
    n = mr.numel()
    m, tf, go = torch.stack([mr, mi]).unsqueeze(0), torch.randn(1, 2, n, generator=g, dtype=torch.float64), torch.randn(1, 2, n, generator=g, dtype=torch.float64)
    out, gm = R.bound_mask(m, tf), R.bound_mask_bwd(m, tf, go)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gm).all())
    mt = torch.stack([mr * tf[0, 0] - mi * tf[0, 1], mr * tf[0, 1] + mi * tf[0, 0]]).unsqueeze(0)
    gt = torch.stack([go[0, 0] * tf[0, 0] + go[0, 1] * tf[0, 1], -go[0, 0] * tf[0, 1] + go[0, 1] * tf[0, 0]]).unsqueeze(0)
    assert float(((out - mt).abs() / R.bound_mask_mag(m, tf).clamp_min(1e-300)).max()) < 1e-8
    assert float((gm - gt).abs().max()) < 1e-7
    # the float32 evaluation (what floors_bound_mask measures) is finite there too
    assert bool(torch.isfinite(R.bound_mask(m.float(), tf.float())).all()) and R.bound_mask(m.float(), tf.float()).dtype == torch.float32


def test_adamw_matches_torch_float64():
    """5 steps of torch.optim.AdamW on float64 CPU tensors with the project's hyper-parameters, the gradient clipped by
    clip_grad_norm_ (active in steps 1 - 3: norm above max_norm; inactive in steps 4, 5): 1e-14 relative for p, exp_avg, exp_avg_sq"""
    g = torch.Generator().manual_seed(4)
    n, lr, (b1, b2), eps, wd, max_norm = 1500, 1e-2, O.HYPER["betas"], O.HYPER["eps"], O.HYPER["wd"], 10.0
    p = torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    rp, rm, rv = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    active = []
    for step in range(1, 6):
        grad = torch.randn(n, generator=g, dtype=torch.float64) * (1.0 if step <= 3 else 0.1)
        p.grad = grad.clone()
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        coef, norm = O.clip_coef(O.sumsq(grad), max_norm, 1.0)
        active.append(coef < 1.0)
        assert abs(norm - float(grad.norm())) < 1e-12 * norm
        rp, rm, rv = O.adamw_step(rp, grad, rm, rv, lr, b1, b2, eps, wd, step, coef)
        st = opt.state[p]
        for name, a, b in (("p", rp, p.detach()), ("m", rm, st["exp_avg"]), ("v", rv, st["exp_avg_sq"])):
            assert float((a - b).abs().max() / b.abs().max()) < 1e-14, (step, name)
    assert active == [True, True, True, False, False]
    assert O.clip_coef(4.0, 0.0, 0.25) == (0.25, 0.5)
    c, _ = O.clip_coef(400.0, 10.0, 0.25)                        # norm 20 * 0.25 = 5 below max_norm: pre alone
    assert c == 0.25
    c, _ = O.clip_coef(1e4, 10.0, 0.5)
    assert abs(c - 10.0 / (50.0 + 1e-6) * 0.5) < 1e-16


# ---- the case tables ----------------------------------------------------------------------------------------------------------------------
def test_sizing_rules_by_hand():
    assert R.slots(3, 4096) == 3 and R.slots(3, 4097) == 6 and R.slots(0, 5) == -1 and R.slots(2, 0) == -1
    assert R.moments_ws(3, 65, 8193) == 5 * 65 * 9 and R.affine_bwd_ws(1, 1, 1) == 6
    assert R.mask_grid(3 * 1025) == (4, 4) and R.mask_grid(3 * 1_400_003) == (4096, 5) and R.mask_grid(1) == (1, 1)
    assert O.gridn(4 * 1024 * 1024) == 4096 and O.forms(4_194_304 + 1027)["adamw_iters"] == 5 and O.forms(1025)["workgroups"] == 2


def test_case_tables_reach_every_branch():
    """streaming kernels: every S of the issue's axis, 1 / 2 / 3 chunks, a last chunk of 1, of exactly 4096 and ragged ones, lane and
    thread loops of 0 further / several iterations, a last workgroup of the wave-per-item kernels with 1, 2 and 3 idle waves, C = 65,
    N in {1, 3}, every data class, both output forms.  coefficient kernels: one workgroup (1, 64 channels), two with a single lane in the
    second (65), three (130); both statistic sources.  masks: one thread, several workgroups, and the 4096-workgroup cap crossed.
    optimiser: 0, 1, 2 and 4096 workgroups, the n % 4 tail at 0, 1, 3, a fifth grid-stride iteration."""
    t = R.stream_cases()
    assert len({c.id for c in t}) == len(t)
    f = [c.forms() for c in t]
    assert {c.S for c in t} >= set(R.S_AXIS)
    assert {x["nchunks"] for x in f} == {1, 2, 3, 4}
    assert {1, 4095, 4096, 63, 64, 65, 255, 257} <= {x["last_chunk"] for x in f}
    assert {x["items_mod4"] for x in f} == {0, 1, 2, 3}
    assert {x["lane_iters"] for x in f} >= {1, 2, 4, 5, 64} and {x["thread_iters"] for x in f} >= {1, 2, 16}
    assert {c.C for c in t} == {1, 3, 65} and {c.N for c in t} == {1, 3}
    assert {c.data for c in t} == set(R.DATA)
    for S in (1, 4097):
        assert any(c.sliced and c.S >= S for c in t) and any(not c.sliced and c.S >= S for c in t)
    for d in R.DATA:
        assert {c.sliced for c in t if c.data == d} == {True, False}, d
    assert max(c.N * 2 * c.C * c.S for c in t) <= 2_000_000
    cf = [R.coef_forms(C, tr) for C in R.COEF_C for tr in (True, False)]
    assert {x["workgroups"] for x in cf} == {1, 2, 3} and {x["last_wg_lanes"] for x in cf} == {1, 64, 2}
    assert {(x["stats"], x["cm"]) for x in cf} == {("sums", True), ("stats_in", False)}
    mg = [R.mask_grid(N * P) for N, P in R.BOUND_MASK_CASES]
    assert [b for b, _ in mg] == [1, 1, 4, 4096] and mg[-1][1] > 4 and 3 * 1_400_003 > R.GRID_CAP
    pg = [R.mask_grid(n) for n in R.PHASE_MASK_N]
    assert [b for b, _ in pg] == [1, 1, 4096] and pg[-1][1] > 4
    sf = [O.forms(n) for n in O.SUMSQ_N]
    assert {x["workgroups"] for x in sf} == {0, 1, 2, 4096} and {x["tail"] for x in sf} >= {0, 1, 3}
    assert any(x["capped"] and x["vec_iters"] >= 2 and x["tail"] for x in sf) and any(x["vec_iters"] == 0 and x["tail"] for x in sf)
    af = [O.forms(n) for n in O.ADAMW_N]
    assert {x["workgroups"] for x in af} == {1, 2, 4096} and max(x["adamw_iters"] for x in af) == 5


def _scale(name, ref, mag, n_terms):
    if name in ("sums", "gcoef"):                               # a sum of n terms of random sign is of size sum |terms| / sqrt(n)
        return mag / n_terms ** 0.5
    return ref.pow(2).mean().sqrt()


@pytest.mark.parametrize("case", R.stream_cases(), ids=lambda c: c.id)
def test_stream_case_has_power(case):
    """the bound of every output, from the reference and the CPU floors alone, is below 1e-3 of the output's scale (RMS; for the
    reductions the size of a sum of N S terms of random sign), the floors stay small, and at most 1e-4 of the case's elements -- plus 2 for
    the cases of a few thousand elements -- lie in the leaky-ReLU sign band (fp64 reference alone)"""
    inp = R.make_inputs(case)
    coef, cm = R.stream_intermediates(case, inp)
    ref, mag, slack, fl = R.floors_stream(case, inp, coef.double(), cm.double())
    for k in ref:
        tol = R.k_of(fl[k]) * R.EPS32 * mag[k]                   # without the slack: the band elements are counted below
        rel = float((tol / _scale(k, ref[k], mag[k], case.N * case.S).clamp_min(1e-300)).max())
        assert rel <= 1e-3, (case.id, k, rel, fl)
    assert max(fl.values()) <= (8.0 if case.data == "const" else 4.0), fl   # 64 equal values per lane round the same way every time
    coef64, _, _ = R.coef_fwd((R.moments(inp["x"]), 1.0 / (case.N * case.S)), inp["W"], inp["B"], R.f32(R.GEN_EPS))
    b = R.band(inp["x"], coef64)
    assert int(b.sum()) <= 1e-4 * b.numel() + 2, (case.id, int(b.sum()), b.numel())


@pytest.mark.parametrize("C", R.COEF_C)
@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
def test_coef_case_has_power(C, train):
    """condition-aware: the correlated channels (rho = 0.999, delta = 2e-3 Vrr Vii) carry a magnitude of ~500 |Z| and still stay below
    1e-3 of the channel's |Z|; B' is measured against the size of u = Z x + B'"""
    ci = R.coef_inputs(C)
    ref, mag, fl = R.floors_coef(ci, train)
    coef, mc = ref["coef"], mag["coef"]
    tol = R.k_of(fl["coef"]) * R.EPS32 * mc
    st = R.stats_of(ci["sums"], ci["inv"]) if train else ci["running"].double()
    zmax = coef[:4].abs().max(0).values
    spread = (st[2] + st[4] + 2 * R.GEN_EPS).sqrt()
    scale = torch.cat([zmax.expand(4, C), torch.maximum(coef[4:].abs(), (zmax * spread).expand(2, C))])
    rel = tol / scale
    assert float(rel.max()) <= 1e-3, (C, train, float(rel.max()), int(rel.argmax()), fl)
    if train:
        assert float(mc[0, 2 % C] / coef[0, 2 % C].abs()) > 100 or C < 3          # channel 2 is a correlated one: the magnitude saw it
    assert max(fl.values()) <= 2.0, fl


@pytest.mark.parametrize("NP", R.BOUND_MASK_CASES[:3], ids=str)
def test_mask_case_has_power(NP):
    bi = R.bound_mask_inputs(*NP)
    assert bool(((bi["m"][:, 0] != 0) | (bi["m"][:, 1] != 0)).all())
    ref, mag, fl = R.floors_bound_mask(bi)
    assert max(fl.values()) <= 4.0, fl
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all())
    if NP[1] > 1:
        a = torch.hypot(bi["m"][:, 0].double(), bi["m"][:, 1].double())
        assert float(a[bi["small"]].max()) <= 1.0001e-4 and float(a[~bi["small"]].min()) >= 0.9999e-4 and float(a.min()) < 1e-25
        assert bool(((bi["m"][:, 0] == 0) | (bi["m"][:, 1] == 0)).any())
    pi = R.phase_mask_inputs(257)
    ref, mag, fl = R.floors_phase_mask(pi)
    assert max(fl.values()) <= 4.0, fl
    z = (pi["xc"] == 0).all(1)
    assert int(z.sum()) > 0 and torch.equal(ref["out"][z, 0], pi["mag"][z].double()) and torch.equal(ref["gmag"][z], pi["g"][z, 0].double())
    assert bool(((pi["xc"] == 0).sum(1) == 1).any()) and bool((pi["mag"] < 0).any())


def test_adamw_k_from_the_betas():
    """K of the p bound from the float values of the betas alone: 8 + E(b1) + E(b2) / 2, E = b^step / (1 - b^step)"""
    b1, b2 = O.f32(0.95), O.f32(0.999)
    assert abs((1 - b2) / 1e-3 - 1) > 1e-5                      # 1 - 0.999f is 1.3e-5 off 0.001: why the reference takes the float values
    assert 515 < O.adamw_k(b1, b2, 1) < 530 and 25 < O.adamw_k(b1, b2, 2) * 0.1 < 27 and O.adamw_k(b1, b2, 1000) < 8.3
