"""tests/norm_ref.py judged on the CPU: the restatement against torch's float64 autograd, what the per-element bound of
tests/test_gpu_norm_kernel.py can see (planted faults, next to the whole-tensor RMS assertion of tests/test_gpu_norm.py), the walk
of the GPU case table over the dispatch of norm_fwd / norm_bwd, the power of every case's bound and the workspace sizes.

tests/golden/ holds whole-network vectors only (no GroupNorm-bearing block), so there is no golden comparison here."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R

TABLE = R.case_table()


def _torch_reference(x, gamma, beta, res, scale, gy, mode, kind, G, eval_stats=None):
    t = [None if v is None else v.double().clone().requires_grad_(True) for v in (x, gamma, beta, res, scale)]
    xr, w, b, rs, sc = t
    if kind == "gn":
        u = F.group_norm(xr, G, w, b, float(torch.tensor(R.GEN_EPS, dtype=torch.float32)))
    else:
        rm, rv = eval_stats if eval_stats else (None, None)
        u = F.batch_norm(xr, rm, rv, w, b, training=eval_stats is None, eps=float(torch.tensor(R.GEN_EPS, dtype=torch.float32)))
    y = {"none": lambda: u, "relu": lambda: F.relu(u), "gelu": lambda: F.gelu(u), "glu": lambda: F.glu(u, 1),
         "glu_scale_res": lambda: rs + sc.view(1, -1, 1) * F.glu(u, 1)}[mode]()
    y.backward(gy.double())
    return y.detach(), xr.grad, w.grad, b.grad, (sc.grad if sc is not None else None)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("mode", R.ALL)
@pytest.mark.parametrize("G", [1, 3, 12])
def test_groupnorm_against_float64_autograd(mode, G):
    case = R.Case("x", "gn", 4, 12, 37, G, mode)
    inp = R.make_inputs(case)
    m, r = R.stats(inp["x"], "gn", G)
    ref = R.reference(inp, m, r, case)
    y, dx, dw, db, dsc = _torch_reference(inp["x"], inp["gamma"], inp["beta"], inp["res"], inp["scale"], inp["gy"], mode, "gn", G)
    # dx through the reference's closed form holds mean / rstd fixed -- it IS the full derivative: the closed form carries their terms
    for name, t in (("y", y), ("dx", dx), ("dgamma", dw), ("dbeta", db), ("dscale", dsc)):
        if t is not None:
            assert _rel(ref[name], t) <= 1e-12, name


@pytest.mark.parametrize("mode", ["none", "relu"])
def test_batchnorm_against_float64_autograd(mode):
    case = R.Case("x", "bn", 5, 6, 41, 6, mode)
    inp = R.make_inputs(case)
    m, r = R.stats(inp["x"], "bn", 6)
    ref = R.reference(inp, m, r, case)
    y, dx, dw, db, _ = _torch_reference(inp["x"], inp["gamma"], inp["beta"], None, None, inp["gy"], mode, "bn", 6)
    for name, t in (("y", y), ("dx", dx), ("dgamma", dw), ("dbeta", db)):
        assert _rel(ref[name], t) <= 1e-12, name
    # eval: running statistics are inputs, forward only
    g = torch.Generator().manual_seed(3)
    rm, rv = torch.randn(6, generator=g).double(), torch.rand(6, generator=g).double() + 0.5
    e = float(torch.tensor(R.GEN_EPS, dtype=torch.float32))
    ye = R.forward(inp["x"].double(), inp["gamma"].double(), inp["beta"].double(), rm, torch.rsqrt(rv + e), mode, kind="bn", G=6)
    u = F.batch_norm(inp["x"].double(), rm, rv, inp["gamma"].double(), inp["beta"].double(), training=False, eps=e)
    assert _rel(ye, F.relu(u) if mode == "relu" else u) <= 1e-12


def test_statistics_and_finalize():
    x = R.make_inputs(R.Case("x", "gn", 3, 6, 4100, 3))["x"]
    m, r = R.stats(x, "gn", 3)
    m2, r2 = R.finalize(*R.moments(x, "gn", 3))
    assert _rel(m2, m) <= 1e-12 and _rel(r2, r) <= 1e-12
    xb = x.view(3, 3, -1)
    assert _rel(m, xb.double().mean(2).reshape(-1)) <= 1e-12
    assert _rel(r, torch.rsqrt(xb.double().var(2, unbiased=False) + float(torch.tensor(1e-5, dtype=torch.float32))).reshape(-1)) <= 1e-12


# ---- what the bound can see --------------------------------------------------------------------------------------------------------
def _case(group, **kw):
    hits = [c for c in TABLE if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]
    assert hits, (group, kw)
    return hits[0]


# fault -> the case of the GPU table that names its edge
PLANTED = {
    "tail_unwritten": _case("rows", S=1028, mode="glu_scale_res", x16=False),
    "stats_last_chunk_missing": _case("stats", S=4100, given=-1, x16=False),
    "beta_from_neighbour": _case("rows", S=260, mode="gelu", x16=False),
    "glu_halves_swapped": _case("rows", S=516, mode="glu", x16=False),
    "dscale_missing_sample": _case("sample", C=96, S=68, mode="glu_scale_res", x16=False),
    "groupsum_over_C": _case("generic", S=13000, mode="gelu", x16=False),
    "gate_dx_sigmoid": _case("sample", C=98, S=256, mode="glu", x16=False),
    "inv_over_C": _case("rows", S=512, mode="none", x16=False),
}
# what `_rms(out, ref) < 1e-5` / `_rms(grad, ref) < 2e-5 * max(1, max |ref|)` of tests/test_gpu_norm.py says of the same faulty outputs
RMS_ACCEPTS = {
    "tail_unwritten": False, "stats_last_chunk_missing": False, "beta_from_neighbour": False, "glu_halves_swapped": False,
    "dscale_missing_sample": False, "groupsum_over_C": False, "gate_dx_sigmoid": False, "inv_over_C": False,
    "one_element_1e-3": True, "last_item_of_one_row_1e-4": True,
}


def _rms_accepts(got, ref):
    ok = True
    for k in ref:
        rms = float(((got[k].double() - ref[k]) ** 2).mean().sqrt())
        ok &= rms < (1e-5 if k == "y" else 2e-5 * max(1.0, float(ref[k].abs().max())))
    return ok


def _bound_accepts(case, got, ref, mag, slack, fl):
    return all(R.worst(got[k], ref[k], R.tolerance(k, ref, mag, slack, fl, case.x16))[0] <= 1.0 for k in ref)


@functools.lru_cache(maxsize=None)
def _clean(case):
    inp = R.make_inputs(case)
    m, r = (t.float().double() for t in R.stats(inp["x"], case.kind, case.G))
    return (inp, m, r) + R.floors(inp, m, r, case)


@pytest.mark.parametrize("fault", R.MUTATIONS)
def test_bound_rejects_planted_fault(fault):
    """the fault planted into the fp32 restatement (the stand-in for a kernel): the unplanted one passes, the planted one does not"""
    case = PLANTED[fault]
    inp, m, r, ref, mag, slack, fl = _clean(case)
    clean = R.reference(inp, m, r, case, dtype=torch.float32, sums=R.Lanes32)
    assert _bound_accepts(case, clean, ref, mag, slack, fl)
    if fault == "stats_last_chunk_missing":
        mt, rt = R.stats(inp["x"], case.kind, case.G)
        smag, sfl = R.stat_magnitudes(inp["x"], case.kind, case.G), R.stat_floors(inp["x"], case.kind, case.G)
        within = lambda mm, rr: (R.worst(mm, mt, R.k_of(sfl["mean"]) * R.EPS32 * smag["mean"])[0] <= 1.0 and               # noqa: E731
                                 R.worst((rr - rt) / rt, torch.zeros_like(rt), R.k_of(sfl["rstd"]) * R.EPS32 * smag["rstd"])[0] <= 1.0)
        assert within(*R.stats32(inp["x"], case.kind, case.G))
        mf, rf = R.stats32(inp["x"], case.kind, case.G, mutate=fault)
        assert not within(mf, rf)
        bad = R.reference(inp, mf.float().double(), rf.float().double(), case, dtype=torch.float32, sums=R.Lanes32)
    else:
        bad = R.reference(inp, m, r, case, dtype=torch.float32, sums=R.Lanes32, mutate=fault)
        assert not _bound_accepts(case, bad, ref, mag, slack, fl)
        if fault == "tail_unwritten":                          # what the GPU test's buffers hold instead of 0
            nan = R.reference(inp, m, r, case, dtype=torch.float32, sums=R.Lanes32, mutate=fault, prefill=float("nan"))
            assert not _bound_accepts(case, nan, ref, mag, slack, fl)
    assert _rms_accepts(clean, ref)
    assert _rms_accepts(bad, ref) == RMS_ACCEPTS[fault]


@pytest.mark.parametrize("name,size,where", [("one_element_1e-3", 1e-3, "one"), ("last_item_of_one_row_1e-4", 1e-4, "item")])
def test_small_edge_faults_pass_the_rms_and_not_the_bound(name, size, where):
    """the faults the issue of the whole-tensor metric is about: one element off by 1e-3, the ragged last item of one row off by 1e-4"""
    case = _case("rows", S=1028, mode="gelu", x16=False)
    inp, m, r, ref, mag, slack, fl = _clean(case)
    bad = {k: v.clone() for k, v in R.reference(inp, m, r, case, dtype=torch.float32, sums=R.Lanes32).items()}
    for k in ("y", "dx"):
        if where == "one":
            bad[k][-1, -1, -1] += size
        else:
            bad[k][-1, -1, 1024:] += size
    assert not _bound_accepts(case, bad, ref, mag, slack, fl)
    assert _rms_accepts(bad, ref) == RMS_ACCEPTS[name]


def test_bf16_store_is_judged_per_element():
    """the stored 16-bit dx: RNE of the fp32 restatement passes, truncation does not"""
    case = _case("rows", S=260, mode="glu", x16=True)
    inp, m, r, ref, mag, slack, fl = _clean(case)
    f32 = R.reference(inp, m, r, case, dtype=torch.float32, sums=R.Lanes32)
    tol = R.tolerance("dx", ref, mag, slack, fl, True)
    assert R.worst(R.bf16_rne(f32["dx"]), ref["dx"], tol)[0] <= 1.0
    trunc = (f32["dx"].contiguous().view(torch.int32) & -65536).view(torch.float32)
    assert R.worst(trunc, ref["dx"], tol)[0] > 1.0


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_form():
    reached, steer = set(), {}
    for c in TABLE:
        f = c.forms()
        assert f is not None, c.id
        reached |= set(f[0])
        for k, v in f[1].items():
            steer.setdefault(k, set()).add(v)
    # every launch of norm_fwd / norm_bwd, both storage types where the kernel has both (diff against the hipLaunchKernelGGL lines)
    assert reached == {
        "stats<f32,slotted>", "stats<bf16,slotted>", "memset+stats<f32,atomic>", "memset+stats<bf16,atomic>", "finalize",
        "rows<f32>", "rows<bf16>", "apply<4>", "apply<1>",
        "partial<f32>", "partial<bf16>", "partial<f32>+slotsum", "partial<bf16>+slotsum", "groupsum", "chansum",
        "chansum_split", "chansum_final", "bwd_rows<f32>", "bwd_rows<bf16>", "bwd_apply<4>", "bwd_apply<1>",
        "sample_wave<12,f32>", "sample_wave<12,bf16>", "sample_wave<24,f32>", "sample_wave<24,bf16>",
        "sample_reg<3,true,f32>", "sample_reg<3,true,bf16>", "sample_reg<6,false,f32>", "sample_reg<6,false,bf16>",
        "sample<f32>", "sample<bf16>"}
    stat = {(c.forms()[1]["nchunks"], c.forms()[1]["last_chunk"] == R.CHUNK) for c in TABLE if "nchunks" in c.forms()[1]}
    assert {(1, False), (2, True), (2, False), (3, False)} <= stat and any(n > 2 for n, _ in stat)
    assert steer["stat_vec"] == {True, False}
    bwdc = {(c.forms()[1]["bwd_nchunks"], c.forms()[1]["bwd_last_chunk"] == R.CHUNK) for c in TABLE if c.bwd}
    assert {(1, False), (2, True), (4, False)} <= bwdc
    rows = {(c.forms()[1]["ipr"], c.forms()[1]["row_exact"]) for c in TABLE if "ipr" in c.forms()[1]}
    assert {(1, False), (1, True), (2, False), (2, True), (3, False), (5, False)} <= rows
    assert steer["NS"] == {(1, False), (1, True), (32, True), (64, True)}
    assert 1 in steer["slots"] and any(1 < s <= 64 for s in steer["slots"]) and any(s > 64 for s in steer["slots"])
    assert any(c.forms()[1].get("gridz", c.N) < c.N for c in TABLE if c.kind == "gn") and \
        any(c.forms()[1].get("gridz", c.N) < c.N for c in TABLE if c.kind == "bn")
    assert steer["partial_branch"] == {"pair_vec", "pair_scalar", "single_vec", "single_scalar"}
    # both sides of every switch of the per-sample dispatch
    per = [c for c in TABLE if c.kind == "gn" and c.G == 1 and c.N >= 512]
    assert {c.C * c.S for c in per} >= {65536} and any(c.C * c.S > 65536 for c in per) and any(c.N == 511 for c in TABLE)
    for glu, edges in ((False, (12, 13, 24, 25)), (True, (48, 49, 96, 97))):
        assert set(edges) <= {(c.C // 2 if glu else c.C) for c in per if R.is_glu(c.mode) == glu and c.S <= 256}
    assert {256, 260} <= {c.S for c in per if not R.is_glu(c.mode)} and {256, 516} <= {c.S for c in per if R.is_glu(c.mode)}
    assert R.forms("gn", 1, 65540, 4, 1, "none", x16=True) is None and R.forms("bn", 3, 4, 8, 4, "none", x16=True) is None
    assert len({c.id for c in TABLE}) == len(TABLE)


def _measure(c):
    """(floors, largest y tolerance over the RMS of y, (count, total) of elements carrying ReLU slack) with the fp32 rounding of the fp64
    statistics; nothing of the case stays resident"""
    inp = R.make_inputs(c)
    m, r = (t.float().double() for t in R.stats(inp["x"], c.kind, c.G))
    ref, mag, slack, fl = R.floors(inp, m, r, c)
    tol = R.tolerance("y", ref, mag, slack, fl)
    band = R.relu_band_count(inp, m, r, c) if c.mode == "relu" and c.bwd else (0, 1)
    return fl, float(tol.max() / ref["y"].pow(2).mean().sqrt().clamp_min(1e-300)), band


@pytest.mark.parametrize("group", sorted({c.group for c in TABLE}))
def test_every_case_has_power(group):
    """no case's y bound, computed from the reference alone, is looser than 1e-3 of the output's RMS (the large-mean rows are judged on
    their statistics: the apply pass, fed the kernel's mean, has no cancellation left); the floors stay where U_BAND assumes them; and
    the ReLU-backward slack stays what it is meant to be, a handful of elements whose sign is undetermined, never a blanket tolerance:
    at most 1e-4 of a case's elements carry it, plus 3 elements for the cases of a few thousand elements where one hit is already more
    than that (expected: the density of u at 0, about 0.2, times 2 U_BAND eps32 mag(u), some 1e-5 of the elements)"""
    for c in (c for c in TABLE if c.group == group):
        fl, rel, band = _measure(c)
        assert rel <= 1e-3, (c.id, rel)
        assert fl["y"] <= 3.0 and max(fl.values()) <= 4.0, (c.id, fl)
        assert band[0] <= 1e-4 * band[1] + 3, (c.id, band)


def test_large_mean_model_bound():
    """the error model of E[x^2] - m^2 from fp32 lane partials, on the CPU restatement: inside the bound at every m, and the mean / std
    ratio at which the bound passes the project's 1e-4 parity figure"""
    rows = {m: R.large_mean_row(m) for m in (0, 10, 100, 1000)}
    for m, (ratio, rt, cpu32, tch, bound) in rows.items():
        assert cpu32 <= bound, (m, cpu32, bound)
    # bound = 0.5 K eps32 (1 + ratio^2) with K = k_of(floor): 1e-4 at ratio = sqrt(2e-4 / (K eps32) - 1)
    K = rows[1000][4] / (0.5 * R.EPS32 * (1 + rows[1000][0] ** 2))
    cross = (2e-4 / (K * R.EPS32) - 1) ** 0.5
    assert 10 < cross < 100 and rows[10][4] < 1e-4 < rows[100][4], (cross, rows)


# ---- workspace sizes ------------------------------------------------------------------------------------------------------------------
def test_workspace_sizes_by_hand():
    # (2, 6, 100), G = 3: partial pairs 2*6*2 = 24, LayerScale partials 2*3 = 6, group sums 2 * max(2*3, 6) = 12; one chunk
    assert R.work_floats(2, 6, 100, 3) == 24 + 6 + 12
    # (600, 4, 16), G = 1: 600*4*2 + 600*2 + 2 * max(600, 4)
    assert R.work_floats(600, 4, 16, 1) == 4800 + 1200 + 1200
    # (2, 4, 8192), G = 1: 16 + 4 + 2*4, and two chunks: 2*4*2*2 = 32 slot pairs + 2*2*2 = 8 LayerScale slots
    assert R.work_floats(2, 4, 8192, 1) == 16 + 4 + 8 + 32 + 8
    # BatchNorm (G = 0) (3, 5, 4099): 30 + 3*2 + 2*5, two chunks: 3*5*2*2 + 3*2*2
    assert R.work_floats(3, 5, 4099, 0) == 30 + 6 + 10 + 60 + 12
    # statistics: a group of (6 / 3) * 4100 = 8200 values is 3 chunks, 2 * 4096 exactly 2, 12 values 1
    assert (R.stat_chunks(6, 4100, 3), R.stat_chunks(4, 4096, 2), R.stat_chunks(8, 12, 8), R.stat_chunks(3, 1367, 1)) == (3, 2, 1, 2)
    # BatchNorm: one slot per (sample, chunk)
    assert (R.bn_stat_slots(70, 231), R.bn_stat_slots(3, 4099), R.bn_stat_slots(65540, 4)) == (70, 6, 65540)


# ---- plain GLU and average pooling (the tail of norm.hip) -----------------------------------------------------------------------------
GLU_TABLE = R.GLU_ROW_CASES + R.GLU_FLAT_CASES + R.GLU_CAP_CASES


def test_glu_reference_against_float64_autograd():
    x, gy = R.glu_data(3, 6, 43)
    xr = x.double().clone().requires_grad_(True)
    y = F.glu(xr, 1)
    y.backward(gy.double())
    sane = x.abs() < 50                                        # autograd's sigmoid' underflows differently at the planted +-88 ... 1e4
    assert _rel(R.glu(x)["y"], y.detach()) <= 1e-12
    assert _rel(torch.where(sane, R.glu(x, gy)["gx"], 0.0), torch.where(sane, xr.grad, 0.0)) <= 1e-12


def test_glu_floors_are_below_the_table():
    """the fp32 restatement 1 / (1 + exp(-v)) (CPU libm) over every case and both storage types: its error in units of eps32 x magnitude is no
    larger than GLU_FLOOR, the bound's K is 8 floor + 4 at least, and the restatement itself passes the bound"""
    from tests import elem_ref as E
    worst = {}
    for (N, C, S) in GLU_TABLE:
        for x16 in (False, True):
            x, gy = R.glu_data(N, C, S, x16=x16)
            for k, v in R.glu_floors(x, gy).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if N * C * S <= 100000:
                for ref, b, r32 in ((R.glu(x), R.glu_bounds(x), R.glu_restate32(x)), (R.glu(x, gy), R.glu_bounds(x, gy), R.glu_restate32(x, gy))):
                    for name in ref:
                        assert R.worst(r32[name], ref[name], b[name])[0] <= 1.0, (N, C, S, x16, name)
    print("\nGLU floors (eps32 x magnitude), measured on the CPU restatement:", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= R.GLU_FLOOR[k], (k, v)
    assert E.k_of("sigmoid") + 1 >= 8 * R.GLU_FLOOR["y"] + 4 and E.k_of("sigmoid") + 1 >= 8 * R.GLU_FLOOR["da"] + 4
    assert E.k_of("sigmoid_grad") + 2 >= 8 * R.GLU_FLOOR["db"] + 4


def test_glu_inputs_hold_what_the_cases_need():
    x, gy = R.glu_data(2, 4, 130)
    a, b = x[:, :2].reshape(-1), x[:, 2:].reshape(-1)
    for v in R.GLU_SPECIALS:
        assert bool((b == torch.tensor(v).float()).any()), v
    assert bool((b.view(torch.int32) == torch.tensor(-0.0).view(torch.int32)).any())
    assert float(a.abs().max()) > 100 and 0 < float(a[a != 0].abs().min()) < 1e-3 and bool((a == 0).any()) and bool((gy == 0).any())
    assert float(b.abs()[len(R.GLU_SPECIALS):].max()) <= 12
    xb, _ = R.glu_data(2, 4, 130, x16=True)
    assert torch.equal(R.bf16_rne(xb), xb)


@pytest.mark.parametrize("fault", ["halves_swapped", "gate_stride_S", "one_minus_sigmoid_dropped"])
def test_glu_bound_rejects_planted_fault(fault):
    """what the per-element bound sees, on the fp32 restatement as the stand-in for a kernel"""
    N, C, S = 2, 6, 43
    x, gy = R.glu_data(N, C, S)
    Co = C // 2
    if fault == "halves_swapped":
        bad = R.glu_restate32(torch.cat([x[:, Co:], x[:, :Co]], 1))["y"]
        ref, b = R.glu(x)["y"], R.glu_bounds(x)["y"]
    elif fault == "gate_stride_S":                             # the gate read one channel after the value instead of Co channels
        xs = x.clone()
        xs[:, Co:] = x[:, 1:Co + 1]
        bad = R.glu_restate32(xs)["y"]
        ref, b = R.glu(x)["y"], R.glu_bounds(x)["y"]
    else:
        s = 1.0 / (1.0 + torch.exp(-x[:, Co:]))
        bad = torch.cat([gy * s, gy * x[:, :Co] * s], 1)
        ref, b = R.glu(x, gy)["gx"], R.glu_bounds(x, gy)["gx"]
    assert R.worst(bad, ref, b)[0] > 1.0


def test_glu_bf16_store_is_judged_per_element():
    x, gy = R.glu_data(2, 4, 130, x16=True)
    ref, b32 = R.glu(x, gy)["gx"], R.glu_bounds(x, gy)["gx"]
    f32 = R.glu_restate32(x, gy)["gx"]
    tol = R.bf16_store_bound(ref, b32)
    assert R.worst(R.bf16_rne(f32), ref, tol)[0] <= 1.0
    trunc = (f32.contiguous().view(torch.int32) & -65536).view(torch.float32)
    assert R.worst(trunc, ref, tol)[0] > 1.0


def test_glu_case_table_reaches_every_form():
    reached = set()
    for entry in R.GLU_ENTRIES:
        for c in R.GLU_ROW_CASES + R.GLU_CAP_CASES[1:]:
            f = R.forms_glu(entry, *c)
            assert f is not None and any(s.endswith(":rows") for s in f), (entry, c)
            reached |= f
            if entry != "bwd_bf16":                            # one element past the 16-byte boundary: the flat kernel
                for i in range(2 if entry == "fwd" else 3):
                    offs = tuple(int(j == i) for j in range(3))
                    assert R.forms_glu(entry, *c, offs) == {f"glu_{entry}_kernel:flat"} | ({"flat:grid_capped"} if c[0] * c[1] // 2 * c[2] > R.GLU_GRID_CAP else set())
                    reached |= R.forms_glu(entry, *c, offs)
            else:                                              # 8-byte x / gx: two bf16 elements still run, one does not; gy needs 16
                assert R.forms_glu(entry, *c, (4, 4, 4)) == f
                for offs in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 2)):
                    assert R.forms_glu(entry, *c, offs) is None, (c, offs)
        for c in R.GLU_FLAT_CASES + R.GLU_CAP_CASES[:1]:
            f = R.forms_glu(entry, *c)
            if entry == "bwd_bf16":
                assert f is None
            else:
                assert f is not None and f"glu_{entry}_kernel:flat" in f
                reached |= f
    assert reached == {"glu_fwd_kernel:flat", "glu_bwd_kernel:flat", "glu_fwd_rows_kernel<f32>:rows", "glu_bwd_rows_kernel<f32>:rows",
                       "glu_bwd_rows_kernel<bf16>:rows", "flat:grid_capped", "rows:ragged_chunk", "rows:several_chunks", "rows:idle_wave"}
    # by hand: (2, 4, 130) has L = 260, two chunks per sample, the second holds one vector
    assert R.forms_glu("fwd", 2, 4, 130) == {"glu_fwd_rows_kernel<f32>:rows", "rows:ragged_chunk", "rows:several_chunks"}
    # (5, 6, 256): 5 x 3 = 15 items, the fourth wave of the last workgroup has none; (2, 4, 130): 4 items, one full workgroup
    assert "rows:idle_wave" in R.forms_glu("bwd", 5, 6, 256) and "rows:idle_wave" not in R.forms_glu("bwd", 2, 4, 130)
    assert R.forms_glu("fwd", 2, 3, 4) is None and R.forms_glu("fwd", 0, 2, 4) is None


POOL_TABLE = R.POOL_CASES + (R.POOL_CAP_FWD, R.POOL_CAP_BWD)


def test_pool_reference_against_float64_autograd():
    for (NC, H, W, kh, kw) in R.POOL_CASES:
        x, gy = R.pool_data(NC, H, W, kh, kw)
        xr = x.double().clone().requires_grad_(True)
        y = F.avg_pool2d(xr[None], (kh, kw))[0]
        y.backward(gy.double())
        assert _rel(R.pool_fwd(x, kh, kw)[0], y.detach()) <= 1e-12
        gx, bound = R.pool_bwd(gy, H, W, kh, kw)
        assert _rel(gx, xr.grad) <= 1e-12
        assert bool((bound[:, (H // kh) * kh:] == 0).all()) and bool((bound[:, :, (W // kw) * kw:] == 0).all())


def test_pool_restatement_is_inside_the_derived_bound():
    """the fp32 sum in the kernel's order times fl(1 / (kh kw)): inside the counted bound at every case (the largest ratio is printed);
    bit for bit the reference where kh kw is a power of two"""
    worst = {"fwd": 0.0, "bwd": 0.0}
    for (NC, H, W, kh, kw) in POOL_TABLE:
        x, gy = R.pool_data(NC, H, W, kh, kw)
        y32, g32 = R.pool_restate32(x, gy, kh, kw)
        ref, b = R.pool_fwd(x, kh, kw)
        q = R.worst(y32, ref, b)[0]
        worst["fwd"] = max(worst["fwd"], q)
        n = kh * kw
        gref = gy.double() / n
        if n & (n - 1) == 0:
            assert torch.equal(g32, gref.float())
        else:
            worst["bwd"] = max(worst["bwd"], R.worst(g32, gref, 2 * 2.0 ** -24 * gref.abs() + 2.0 ** -149)[0])
    print("\npooling, CPU restatement, largest error / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["fwd"] <= 1.0 and worst["bwd"] <= 1.0


def test_pool_bound_rejects_planted_faults():
    NC, H, W, kh, kw = 2, 7, 9, 3, 2
    x, gy = R.pool_data(NC, H, W, kh, kw)
    ref, b = R.pool_fwd(x, kh, kw)
    y32, _ = R.pool_restate32(x, gy, kh, kw)
    assert R.worst(y32 * kw, ref, b)[0] > 1.0                  # inv = 1 / kh
    wrong = F.avg_pool2d(x[None], (kw, kh))[0]                 # oh = h / kw: the window transposed
    assert wrong.shape != ref.shape or R.worst(wrong, ref, b)[0] > 1.0


def test_pool_case_table_reaches_every_form():
    fw, bw = set(), set()
    for c in POOL_TABLE:
        fw |= R.forms_pool(False, *c)
        bw |= R.forms_pool(True, *c)
    assert "grid_capped" in R.forms_pool(False, *R.POOL_CAP_FWD) and "grid_capped" in R.forms_pool(True, *R.POOL_CAP_BWD)
    assert fw == {"avgpool2_fwd_kernel", "grid_capped", "row_remainder", "column_remainder", "inv_rounded"}
    assert bw == {"avgpool2_bwd_kernel", "grid_capped", "row_remainder", "column_remainder", "inv_rounded"}
    assert all(R.forms_pool(b, *c) is None for c in R.POOL_REFUSED for b in (False, True))
    assert "grid_capped" not in set().union(*(R.forms_pool(True, *c) for c in R.POOL_CASES))
