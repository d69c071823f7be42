"""tests/elem_ref.py against torch in float64 and against the oracle's BLSTM framing, its case tables against the full list of kernel
forms, its floors (recomputed here from the float32 restatements, printed) against the table the GPU test takes K from, and the power
of every bound on the reference alone.  No device is involved."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_hdemucs
from tests import elem_ref as E

CAP = 1e-3


def _close(a, b, tol=1e-12):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1.0))
    assert err <= tol, err


# ---- the reference against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(7), ids=E.ACT_NAMES)
def test_activation_matches_torch(code):
    """act and act' against torch's float64 functions and their autograd, 1e-12"""
    x = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64)
    x = x[x != 0].clone().requires_grad_(True)                           # torch's ReLU' / PReLU' at 0 is a convention, pinned in the GPU test
    slope = torch.tensor([0.25], dtype=torch.float64)
    fn = {E.NONE: lambda t: t * 1.0, E.RELU: F.relu, E.GELU: F.gelu, E.TANH: torch.tanh, E.PRELU: lambda t: F.prelu(t, slope),
          E.LEAKY: lambda t: F.leaky_relu(t, E.LEAKY_SLOPE), E.SIGMOID: torch.sigmoid}[code]
    y = fn(x)
    (g,) = torch.autograd.grad(y.sum(), x)
    _close(E.act(x.detach(), code, 0.25), y.detach())
    _close(E.act_grad(x.detach(), code, 0.25), g)


def test_prelu_bwd_matches_autograd():
    x, gy, slope = E.prelu_data(3, 5, 257, 1)
    xd, sd = x.double().requires_grad_(True), slope.double().requires_grad_(True)
    F.prelu(xd, sd).backward(gy.double())
    gx, gs, mag = E.prelu_bwd(x, gy, slope)
    nz = x != 0                                                          # at 0 the kernel takes the >= side: gx = gy (torch: slope gy)
    _close(gx[nz], xd.grad[nz])
    assert torch.equal(gx[~nz], gy.double()[~nz])
    _close(gs, sd.grad)
    assert bool((mag >= gs.abs()).all())


def test_sums_match_torch():
    """row_moments against x.mean / x.std(unbiased=True), channel_sum against torch.sum over permuted views, l1 against F.l1_loss and its
    gradient, add_bcast / row_affine against broadcasting"""
    x = E.moments_data(5, 1000, 3)
    m, sd, bm, bs = E.row_moments(x)
    _close(m, x.double().mean(1))
    _close(sd, x.double().std(1, unbiased=True), 1e-9)                  # the constant row: both are 0 up to the mean's rounding
    assert float(sd[4]) == 0.0 and float(sd[1]) > 0.9
    for case in E.CHANNEL_CASES[:6] + E.CHANNEL_CASES[7:]:
        base, off, size, st = E.channel_view(case, 4)
        view = base[off:].as_strided(size, st)
        s, sa = E.channel_sum(view)
        _close(s, view.double().permute(1, 0, 2, 3).reshape(size[1], -1).sum(1))
        assert bool((sa >= s.abs()).all())
    a, b = E.l1_data(1025, 5)
    ad = a.double().requires_grad_(True)
    loss = F.l1_loss(ad, b.double())
    loss.backward()
    _close(torch.tensor(E.l1_sum(a, b, 1.0 / 1025), dtype=torch.float64), loss.detach())
    nz = (a - b) != 0
    _close(E.l1_grad(a, b, E.f32(1.0 / 1025), None).double()[nz], ad.grad[nz], 1e-7)       # w is the float the ABI carries
    assert bool((E.l1_grad(a, b, 1.0, 0.5)[100:200] == 0).all())
    for case in E.ADD_CASES:
        xx = torch.randn(case["N"], case["C"], case["A"], case["B"])
        y, st = E.add_y(case, 6)
        shape = {"same": xx.shape, "freq_emb": (1, case["C"], case["A"], 1), "ncb": (case["N"], case["C"], 1, case["B"]), "n": (case["N"], 1, 1, 1),
                 "b0": (case["N"], case["C"], case["A"], 1)}.get(case["ypat"])
        yv = y[..., ::2].reshape(xx.shape) if case["ypat"] == "yb2" else y.reshape(shape)
        _close(E.add_bcast(xx, y, st, case["alpha"])[0], xx.double() + case["alpha"] * yv.double())
    xa, aa, bb = torch.randn(3, 7), torch.randn(3), torch.randn(3)
    _close(E.row_affine(xa, aa, bb)[0], xa.double() * aa.double()[:, None] + bb.double()[:, None])
    am, bmm, _, _ = E.moments_coef(m.float(), sd.float(), 1e-5)
    _close(am, 1.0 / (E.f32(1e-5) + sd.float().double()))
    _close(bmm, -m.float().double() * am)


def test_act_rows_is_a_permuted_activation():
    D, T = (2, 3, 2), 7
    lay = E.rows_layout(D, T)
    x = torch.randn(*D, T)
    out = E.act_rows(x.reshape(-1), D, lay["xs"], lay["os"], T, E.GELU, torch.full((lay["out_len"],), float("nan"), dtype=torch.float64))
    y = out.view(D[0], D[2], D[1], T + 4)
    _close(y[..., :T], F.gelu(x.double()).permute(0, 2, 1, 3))
    assert bool(torch.isnan(y[..., T:]).all())
    g = torch.randn(lay["out_len"])
    out = E.act_rows(x.reshape(-1), D, lay["xs"], lay["os"], T, E.TANH, torch.full((lay["out_len"],), float("nan"), dtype=torch.float64), g, lay["gs"])
    gl = g.view(D[0], D[2], D[1], T + 4)[..., :T].permute(0, 2, 1, 3)
    _close(out.view(D[0], D[2], D[1], T + 4)[..., :T].permute(0, 2, 1, 3), gl.double() * (1 - torch.tanh(x.double()) ** 2))


class _FrameWeights(nn.Module):
    """stands in for the LSTM + Linear of the oracle's BLSTM: a fixed weight per (step, frame, channel), so that every frame position
    is told apart"""

    def __init__(self, w):
        super().__init__()
        self.w = w

    def forward(self, x):
        return x * self.w, None


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("case", ((2, 3, 23, 6, 8, 4), (1, 2, 31, 6, 12, 6), (2, 2, 1000, 10, 200, 100)), ids=lambda c: "x".join(map(str, c)))
def test_blstm_frames_match_oracle(case, skip):
    """modes 0 and 2 against oracle.ref_hdemucs.BLSTM's framing and stitching at max_steps = width (the oracle's concatenation of parts is
    position-consistent only for width = 2 stride with an even stride, which is what the model uses; the odd stride is tied by the
    adjoint identities alone)"""
    B, C, T, nfr, width, stride = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    w = torch.randn(width, B * nfr, C, generator=g, dtype=torch.float64)
    m = ref_hdemucs.BLSTM(C, layers=1, skip=skip).double()
    m.max_steps, m.lstm, m.linear = width, _FrameWeights(w), nn.Identity()
    want = m(x)
    h, _, _ = E.blstm_frames(x.reshape(-1), None, case, 0)
    hw = h * w.view(width, B, nfr, C).permute(3, 0, 1, 2)
    got, _, cnt = E.blstm_frames(hw.reshape(-1), x.reshape(-1) if skip else None, case, 2)
    _close(got, want)
    assert bool((cnt == 1).all())


@pytest.mark.parametrize("case", E.BLSTM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_blstm_adjoints(case):
    """<A x, y> == <x, A^T y> in fp64 for modes 0 / 1 and 2 / 3; the positions of modes 0 and 3 with tau >= T are 0"""
    B, C, T, nfr, width, stride = case
    g = torch.Generator().manual_seed(8)
    x, h = torch.randn(B * C * T, generator=g, dtype=torch.float64), torch.randn(C * width * B * nfr, generator=g, dtype=torch.float64)
    for fwd, adj in ((0, 1), (2, 3)):
        (src, other) = (x, h) if fwd == 0 else (h, x)
        a = float((E.blstm_frames(src, None, case, fwd)[0].reshape(-1) * other).sum())
        b = float((src * E.blstm_frames(other, None, case, adj)[0].reshape(-1)).sum())
        assert abs(a - b) <= 1e-12 * max(abs(a), 1.0), (case, fwd, a, b)
    for mode in (0, 3):
        hh = E.blstm_frames(x, None, case, mode)[0]
        for k in range(nfr):
            for t in range(width):
                if k * stride + t >= T:
                    assert bool((hh[:, t, :, k] == 0).all())
    assert T <= (nfr - 1) * stride + width                                # what rfx_blstm_frames accepts


def test_span_mask_reference():
    c = E.SPAN_CASES[0]
    m = E.span_mask(c)
    for r in range(c["R"]):
        for f in range(c["F"]):
            for t in (0, 9, 10, 19, 20, 249, 250, 289, 290, 299):
                want = (c["f0"][r] <= f < c["f1"][r]) or (c["t0"][r] <= t < c["t1"][r])
                assert bool(m[r, f, t]) == want


# ---- case tables -------------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_branch():
    """the union of forms over every case table is the full list, but for the one declared exception: add_bcast_kernel, the 64-bit
    fallback (rows ceil(B / 256) > 2^31 - 1: more than 8 GiB per tensor)"""
    reached, full = E.walk_all_cases(), E.all_forms()
    assert E.UNREACHABLE == {"add_bcast_kernel"}
    assert reached == full - E.UNREACHABLE, ("not reached", sorted(full - E.UNREACHABLE - reached), "not listed", sorted(reached - full))
    print("\nforms reached:", len(reached), "of", len(full), "- declared unreachable:", sorted(E.UNREACHABLE))


def test_workspace_geometry_mirrors_the_launch_code():
    """a few geometries worked by hand from channel_sum_geometry / row_moments_slots / grid_for"""
    assert E.channel_geometry(0, 1, 1, 1, 1024, 1024, 1024, 1024, 1) == (1, 1)
    assert E.channel_geometry(0, 3, 5, 1, 16389, 5 * 16392, 16392, 16389, 1) == (48, 16)
    assert E.channel_geometry(0, 3, 683, 1, 16389, 683 * 16392, 16392, 16389, 1) == (3, 1)
    assert E.channel_geometry(4, 3, 5, 1, 1027, 5 * 1028, 1028, 1027, 1) == (1, 0)
    assert E.channel_geometry(0, 2, 3, 100, 200, 60000, 20000, 1, 100) == (2, 0)
    assert [E.moments_slots(v) for v in (2, 16384, 16385, 40001, 10 ** 8)] == [1, 1, 2, 3, 256]
    assert [E.grid_for(v) for v in (1, 1024, 1025, 2048 * 1024 + 1027)] == [1, 1, 2, 2048]
    assert [E.l1_slots(v) for v in (0,) + E.L1_N] == [0, 1, 1, 2, 512, 512]


# ---- floors ------------------------------------------------------------------------------------------------------------------------
def _units(err, mag, tiny=0.0):
    ok = mag > 0
    return float(((err - tiny).clamp_min(0)[ok] / (E.EPS32 * mag[ok])).max()) if bool(ok.any()) else 0.0


def test_floors_are_below_the_table():
    """the error of the float32 restatements in units of eps32 x magnitude, largest over each case class; the GPU test takes K = 8 floor + 8
    from elem_ref.FLOOR, which has to be no smaller than what is measured here"""
    got = {}
    xs = torch.cat([E.act_data(n, 11 + n) for n in (1023, 1025)] + [torch.linspace(-12, 12, 400001, dtype=torch.float64).float()])
    g = E.signs_data(xs.numel(), 2)
    for code in (E.GELU, E.TANH, E.SIGMOID):
        a, d = E.restate_act(xs, code)
        name = E.ACT_NAMES[code]
        got[name] = _units((a.double() - E.act(xs, code)).abs(), E.act_magnitude(xs, code), E.MINNORM)
        gd = (g * d).double() if code != E.GELU else (g.double() * d.double()).float().double()
        got[name + "_grad"] = _units((gd - g.double() * E.act_grad(xs, code)).abs(), E.act_grad_magnitude(xs, g, code), E.MINNORM * (1 + g.double().abs()))
    xg = torch.linspace(-12, 12, 2000001, dtype=torch.float64).float()
    a, d = E.restate_act(xg, E.GELU)
    cdf_err = float((d.double() - E.act_grad(xg, E.GELU)).abs().max())
    print(f"\nGELU restatement over [-12, 12]: |gelu err| {float((a.double() - E.act(xg, E.GELU)).abs().max()):.3e}, |gelu' err| {cdf_err:.3e}")
    plane = {False: 0.0, True: 0.0}
    for case in E.CHANNEL_CASES:
        base, off, (N, C, A, B), st = E.channel_view(case, 51)
        slots, nseg = E.channel_geometry(case["x_off"], N, C, A, B, *st)
        if not nseg:
            continue
        view = base[off:].as_strided((N, C, A, B), st)
        for c in sorted({0, 1 % C, C - 1}):
            tot = sum(E.restate_channel_plane(view[n, c].reshape(-1).numpy(), nseg) for n in range(N))
            ref, sabs = float(view[:, c].double().sum()), float(view[:, c].double().abs().sum())
            const = case["const"] and c == 1
            plane[const] = max(plane[const], abs(float(np.float32(tot)) - ref) / (E.EPS32 * sabs))
    got["channel_plane"], got["channel_plane_const"] = plane[False], plane[True]
    got["gslope"] = 0.0
    for shape in E.PRELU_SHAPES:
        x, gy, slope = E.prelu_data(*shape, 31 + shape[2])
        _, gs, mag = E.prelu_bwd(x, gy, slope)
        r = torch.from_numpy(E.restate_gslope(x, gy)).float().double()
        got["gslope"] = max(got["gslope"], _units((r - gs).abs(), mag))
    print("floors (eps32 x magnitude):", {k: round(v, 3) for k, v in got.items()})
    print("K = 8 floor + 8:", {k: E.k_of(k) for k in E.FLOOR})
    for k, v in got.items():
        assert v <= E.FLOOR[k], (k, v, E.FLOOR[k])
    assert set(got) == set(E.FLOOR)


# ---- power: on the reference alone -------------------------------------------------------------------------------------------------
def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("code", (E.GELU, E.TANH, E.SIGMOID), ids=("gelu", "tanh", "sigmoid"))
def test_flat_case_has_power(code):
    """every K-rule bound of the flat activations is below 1e-3 of the RMS of the reference output, on the dense band (the special values,
    up to 3e19, carry the same formula but would make an RMS meaningless)"""
    for n in (1023, 1025, 2048 * 1024 + 1027):
        x, gy, res = E.act_data(n, 11 + n), E.signs_data(n, 12 + n), E.signs_data(n, 13 + n, 0.1, 3.0)
        b = E.band(x)
        assert float(E.act_bound(x, code)[b].max()) <= CAP * _rms(E.act(x, code)[b])
        assert float(E.act_grad_bound(x, gy, code)[b].max()) <= CAP * _rms((gy.double() * E.act_grad(x, code))[b])
        assert float(E.act_add_bound(x, res, code)[b].max()) <= CAP * _rms((E.act(x, code) + res.double())[b])


def test_rows_case_has_power():
    """act_rows: the fp32 part of every bound is inside the cap; the bf16 gradient's own rounding (2^-8) is the format's and is not"""
    for x16 in (False, True):
        x = (torch.rand(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 12 - 6).float()
        g = E.signs_data(4096, 2)
        for code in (E.GELU, E.TANH, E.SIGMOID):
            assert float(E.act_bound(x, code).max()) <= CAP * _rms(E.act(x, code))
            ref = g.double() * E.act_grad(x, code)
            assert float((E.act_grad_bound(x, g, code) + E.HALF * ref.abs()).max()) <= CAP * _rms(ref)
    assert float(E.bf16_half_ulp(torch.tensor(1.0, dtype=torch.float64))) > CAP


def test_sum_case_has_power():
    """sums: bound < 1e-3 of the output's scale (|sum| or sum |terms| / sqrt(count), whichever is larger) and leaving out the last
    element moves the reference by more than the bound"""
    for n in E.L1_N:
        a, b = E.l1_data(n, 41 + n)
        scale = E.f32(1.0 / n)
        tot = float(E.l1_terms(a, b).sum())
        bound = E.l1_bound(n, tot, scale)
        assert bound <= CAP * tot * scale / math.sqrt(n) or bound <= CAP * E.l1_sum(a, b, scale)
        assert float(E.l1_terms(a, b)[-1]) * scale > bound
    for case in E.CHANNEL_CASES:
        base, off, (N, C, A, B), st = E.channel_view(case, 51)
        view = base[off:].as_strided((N, C, A, B), st)
        ref, sabs = E.channel_sum(view)
        bound = E.channel_bound(case["x_off"], N, C, A, B, *st, sabs)
        if case["const"]:
            bound[1] = float(E.channel_bound(case["x_off"], N, C, A, B, *st, sabs[1], const=True))
        scale = torch.maximum(ref.abs(), sabs / math.sqrt(N * A * B))
        assert bool((bound <= CAP * scale).all()), case["name"]
        assert bool((view[N - 1, :, A - 1, B - 1].double().abs() > bound).all()), case["name"]
    for shape in E.PRELU_SHAPES:
        x, gy, slope = E.prelu_data(*shape, 31 + shape[2])
        _, gs, mag = E.prelu_bwd(x, gy, slope)
        bound = E.k_of("gslope") * E.EPS32 * mag + E.TINY
        cnt = (x < 0).sum((0, 2)).clamp_min(1).double()
        assert bool((bound <= CAP * torch.maximum(gs.abs(), mag / cnt.sqrt()) + E.TINY).all()), shape
    for (R, L) in E.MOMENT_SHAPES:
        x = E.moments_data(R, L, 91 + L)
        m, sd, bm, bs = E.row_moments(x)
        assert bool((bm <= CAP * torch.maximum(m.abs(), x.double().abs().sum(1) / L / math.sqrt(L))).all()), (R, L)
        assert float(bs.max()) <= CAP * _rms(sd), (R, L)
        assert bool((x[:, -1].double().abs() / L > bm - E.HALF * m.abs()).all())        # the last element moves the mean by more than the sum's error


def test_counted_case_has_power():
    for case in E.ADD_CASES:
        x = torch.randn(case["N"], case["C"], case["A"], case["B"], generator=torch.Generator().manual_seed(61))
        y, st = E.add_y(case, 62)
        ref, mag = E.add_bcast(x, y, st, case["alpha"])
        assert float((E.EPS32 * mag).max()) <= CAP * _rms(ref)
    for case in E.BLSTM_CASES:
        B, C, T, nfr, width, stride = case
        g = torch.Generator().manual_seed(82)
        h, skip = torch.randn(C * width * B * nfr, generator=g), torch.randn(B * C * T, generator=g)
        for mode, sk in ((1, False), (2, True)):
            ref, mag, _ = E.blstm_frames(h, skip if sk else None, case, mode)
            assert float(E.blstm_bound(case, mode, sk, ref, mag).max()) <= CAP * _rms(ref)
    x, a, b = torch.randn(13, 79), torch.randn(13) + 2.0, torch.randn(13)
    ref, mag = E.row_affine(x, a, b)
    assert float((E.EPS32 * mag).max()) <= CAP * _rms(ref)


# ---- dropout -----------------------------------------------------------------------------------------------------------------------
def test_dropout_draw():
    """the integer restatement against the published first outputs of splitmix64 from state 0 (seed 0, i = 0, 1, 2 here: the state after
    i + 1 increments), worked from the definition; the uint64 array form against the Python-int form; the keep rate over 2^20 draws"""
    first = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    assert [E.dropout_u24_int(0, i) for i in range(3)] == [v >> 40 for v in first]
    for seed in E.DROPOUT_SEEDS + (0, E.M64):
        u = E.dropout_u24(seed, 300)
        assert [int(v) for v in u[:8]] == [E.dropout_u24_int(seed, i) for i in range(8)]
        assert int(u[299]) == E.dropout_u24_int(seed, 299)
        assert 0 <= int(u.min()) and int(u.max()) < 1 << 24
    n = 1 << 20
    for p in (0.1, 0.5):
        for seed in E.DROPOUT_SEEDS:
            kept = int(E.dropout_keep(seed, n, p).sum())
            assert abs(kept - n * (1 - E.f32(p))) <= 5 * math.sqrt(n * p * (1 - p)), (p, seed, kept)
    x = E.signs_data(1000, 3)
    out, keep = E.dropout(x, 0.0, 5)
    assert bool(keep.all()) and torch.equal(out, x)
    out, keep = E.dropout(x, 0.5, 5)
    assert torch.equal(out[keep], x[keep] * 2) and bool((out[~keep] == 0).all())


def test_zero_case_table_reaches_every_branch():
    """rfx_zero (tests/test_gpu_elem_kernel.py::test_zero): head, vector body, tail, a second grid-stride iteration and the capped grid are
    all reached, the byte counts that are no multiple of 4 and the odd byte bases are the refused ones"""
    reached = set()
    for nb in E.ZERO_BYTES + (E.ZERO_BYTES_CAP,):
        for w in E.ZERO_WORD_OFFSETS:
            f = E.forms_zero(nb, 4 * w)
            assert (f is None) == (nb % 4 != 0), (nb, w)
            reached |= f or set()
        assert E.forms_zero(nb, 1) is None and E.forms_zero(nb, 6) is None
    assert reached == {"head", "vec", "tail", "second_iteration", "grid_capped"}
    assert E.forms_zero(0) == set() and E.forms_zero(4, 4) == {"head"} and E.forms_zero(16, 0) == {"vec"} and E.forms_zero(20, 8) == {"head", "tail"}
    assert {0, 1, 3, 4, 15, 16, 17, 4099} <= set(E.ZERO_BYTES) and "grid_capped" in E.forms_zero(E.ZERO_BYTES_CAP, 4)
