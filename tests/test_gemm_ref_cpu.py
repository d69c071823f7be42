"""CPU: the reference, the bound and the case table of the gather-GEMM kernel tests (tests/gemm_ref.py) -- what
tests/test_gpu_gemm_kernel.py judges the kernels by is itself checked here, without a GPU: the reference against torch's float64
autograd, the floors as measured, the power of the bound, the forms the table reaches (the launchers' own host-side selection), and a
list of planted faults the bound must reject."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R

CASES = R.case_table()
BY_ID = {c.id: c for c in CASES}
_CACHE = {}


def _small(case):
    """the streaming cases are large only because the launcher's threshold says so: one sample has every property of the restatement"""
    return dataclasses.replace(case, N=1) if case.N * case.out_hw[0] * case.out_hw[1] > (1 << 18) else case


def _restate(case, inp, mutate=None):
    if case.kind == "wgrad":
        codes = R.host_forms(case)[2]
        v = R.wgrad_decode([c for c in codes if c >= 0][-1])
        return R.restate_wgrad(case, inp, v["family"], v["splits"], mutate)
    return R.restate_fwd(case, inp, mutate)


def _evaluated(case):
    """(inputs, clean restatement) of a case, once"""
    if case.id not in _CACHE:
        cs = _small(case)
        inp = R.make_inputs(cs)
        _CACHE[case.id] = (cs, inp, _restate(cs, inp))
    return _CACHE[case.id]


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 9, 14, generator=g)
    w = torch.randn(7, 5, 3, 4, generator=g)
    b = torch.randn(7, generator=g)
    st, pd, dl = (2, 1), (1, 2), (1, 2)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xr, wr, br, st, pd, dl)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    base = dict(cin=5, cout=7, ishape=(9, 14), ksize=(3, 4), stride=st, padding=pd, dilation=dl)
    c = R.Case("t", "conv", "f32", (), **base)
    assert float((R.reference(c, {"x": x, "w": w, "b": b})["y"].ref - y.detach()).abs().max()) < 1e-12
    c = R.Case("t", "dgrad", "f32", (), bias=False, **base)
    assert float((R.reference(c, {"x": x, "w": w, "g": gy})["dx"].ref - xr.grad).abs().max()) < 1e-12
    c = R.Case("t", "wgrad", "f32", (), **base)
    r = R.reference(c, {"x": x, "w": w, "g": gy})
    assert float((r["dw"].ref - wr.grad).abs().max()) < 1e-12 and float((r["db"].ref - br.grad).abs().max()) < 1e-12
    # transposed forward with a crop, against torch's own padding / output_padding form
    wt = torch.randn(5, 7, 4, 1, generator=g)
    c = R.Case("t", "convT", "f32", (), 5, 7, (9, 14), (4, 1), stride=(2, 1), crop=((1, 0), (1, 0)))
    yt = F.conv_transpose2d(x.double(), wt.double(), b.double(), (2, 1), (1, 0))
    assert float((R.reference(c, {"x": x, "w": wt, "b": b})["y"].ref - yt).abs().max()) < 1e-12
    # GLU of the stored z
    c = R.Case("t", "conv", "f32", (), 5, 8, (9, 14), (3, 4), glu=True, bias=False)
    w8 = torch.randn(8, 5, 3, 4, generator=g)
    z = F.conv2d(x.double(), w8.double())
    assert float((R.reference(c, {"x": x, "w": w8}, got={"z": z})["glu"].ref - F.glu(z, 1)).abs().max()) < 1e-12
    # every activation: forward and the backward epilogue
    slope = torch.linspace(0.05, 0.45, 7)
    torch_act = {"relu": F.relu, "gelu": F.gelu, "tanh": torch.tanh, "leaky": lambda t: F.leaky_relu(t, 0.01), "sigmoid": torch.sigmoid,
                 "prelu": lambda t: F.prelu(t, slope.double())}
    for act in R.ACTS:
        u = F.conv2d(x.double(), w.double(), b.double(), st, pd, dl).requires_grad_(True)
        a = torch_act[act](u)
        a.backward(gy.double())
        c = R.Case("t", "conv", "f32", (), act=act, **base)
        inp = {"x": x, "w": w, "b": b, "slope": slope, "res": gy}
        assert float((R.reference(c, inp)["y"].ref - a.detach()).abs().max()) < 1e-12, act
        cb = dataclasses.replace(c, bwd=True, gslots=1 if act == "prelu" else 0)
        rb = R.reference(cb, inp)
        assert float((rb["y"].ref - u.grad).abs().max()) < 1e-12, act
        if act == "prelu":
            dslope = (gy.double() * u.detach().clamp_max(0)).sum((0, 2, 3))
            assert float((rb["gparam"].ref - dslope).abs().max()) < 1e-10


def test_operand_rounding_rules():
    """bf16x3: hi + lo reproduces an fp32 value to 2^-16 relative, and values already stored in 16 bits are exact in the bf16 mode"""
    t = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    hi, lo = R.parts(t, "bf16x3")
    assert float(((hi + lo) - t.double()).abs().max() / t.abs().max()) < 2.0 ** -16
    assert torch.equal(R.parts(R.bf16_rne(t), "bf16")[0], R.bf16_rne(t).double())
    assert torch.equal(R.bf16_rne(t), t.to(torch.bfloat16).float())


# ---- floors ---------------------------------------------------------------------------------------------------------------------------------
def test_floors():
    """FLOORS is the measurement rounded up to the next quarter: not below it, and not a figure picked to pass"""
    fl = {}
    for case in CASES:
        cs, inp, got = _evaluated(case)
        d = fl.setdefault(case.klass, {})
        for k, v in R.measure(cs, inp, got).items():
            d[k] = max(d.get(k, 0.0), v)
    assert set(fl) == set(R.FLOORS)
    for kl, d in sorted(fl.items()):
        print(kl, {k: round(v, 3) for k, v in d.items()})
        assert set(d) == set(R.FLOORS[kl]), kl
        for k, v in d.items():
            assert v <= R.FLOORS[kl][k], (kl, k, v)
            assert R.FLOORS[kl][k] <= max(0.25, 1.5 * v + 0.25), (kl, k, v)


def _rms(t):
    return float((t.double() ** 2).mean().sqrt())


def test_every_case_has_power():
    """The fp32 part of the tolerance (K eps32 magnitude + slack) is at most 1e-3 of the output's RMS in every case.  A 16-bit store adds
    half a bf16 ulp of the value, 2^-9 ... 2^-8 relative by the format: there the whole tolerance stays under one bf16 ulp (2^-8) of the
    RMS.  Sign-flip slack touches at most SIGN_SHARE of a case's elements."""
    worst = 0.0
    for case in CASES:
        cs, inp, got = _evaluated(case)
        K = {k: R.k_of(cs, k) for k in R.FLOORS[cs.klass]}
        for k, r in R.reference(cs, inp, got, K).items():
            fp32_part = K[k] * R.EPS32 * r.mag + (r.slack if r.slack is not None else 0.0)
            assert r.flips <= R.SIGN_SHARE, (case.id, k, r.flips)
            if r.slack is not None:                                # the slack itself is judged by its share; the bound elsewhere by its size
                fp32_part = K[k] * R.EPS32 * r.mag
            ratio = _rms(fp32_part) / _rms(r.ref)
            worst = max(worst, ratio)
            assert ratio <= 1e-3, (case.id, k, ratio)
            if r.store16:
                assert _rms(R.tolerance(r, K[k])) <= 2.0 ** -8 * _rms(r.ref), (case.id, k)
    print("largest fp32 tolerance / RMS of the output over the table:", worst)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
# every instantiation rfx_gemm_fwd / rfx_gemm_wgrad can launch (csrc/gemm.hip, gemm_tap.h, gemm_halo.h, gemm_wgrad.hip, gemm_wgrad.h).
# gemm_wgrad_wide_kernel<3, 2, 1, 1> does not exist: the 96 x 256 tile is a bf16-mode shape (the split mode's LDS images would not fit).
ALL_FORMS = (
    ["gemm_thin_fwd_kernel<%d>" % m for m in (1, 2, 4, 8)]
    + ["gemm_fwd_kernel<%d>" % r for r in (1, 2, 3, 4)]
    + ["gemm_tap_kernel<%d, %d>" % (r, p) for r in (1, 2, 3, 4) for p in (1, 2)]
    + ["gemm_tap_kernel<%d, 2, IN16>" % r for r in (1, 2, 3, 4)]
    + ["gemm_tap_stream_kernel<%d, %s>" % (p, s) for p in (1, 2) for s in ("4, 1", "2, 4")]
    + ["gemm_halo_kernel<%d, %d, %d>" % (r, t, i) for r in (1, 2, 3) for t in (9, 3) for i in (0, 1)]
    + ["gemm_thin_wgrad_kernel<%d>" % m for m in (1, 2, 4, 8)]
    + ["gemm_wgrad_kernel<%d, %d>" % (a, b) for a in (1, 2) for b in (1, 2)]
    + ["gemm_wgrad_bf_kernel<%s, %s>" % (s, p) for s in ("3, 1, 1", "1, 2, 1", "1, 1, 1", "2, 2, 2", "2, 1, 2", "1, 2, 2", "1, 1, 2")
       for p in ("1", "2", "2, G16")]
    + ["gemm_wgrad_wide_kernel<%s, %s>" % (s, p) for s in ("3, 1, 1", "1, 2, 1", "1, 1, 1", "2, 2, 2", "1, 2, 2") for p in ("1", "2", "2, G16")]
    + ["gemm_wgrad_wide_kernel<3, 2, 1, %s>" % p for p in ("2", "2, G16")]
)

# edges every family has to meet at least once: family = prefix of the form's name
REQUIRED_EDGES = {
    "gemm_thin_fwd_kernel": {"P%256", "two_phase_in", "two_phase_in2", "res", "bwd_prelu", "bwd_other", "gslots1", "stat1", "stat16", "act2", "stride_a"},
    "gemm_fwd_kernel": {"M31", "M32", "M33", "M95", "M96", "M97", "Kpad", "P%32", "taps_meet_padding_kept", "stride_a", "stride_b", "noncontig_in",
                        "out_slice", "out_phase", "res", "act2", "two_phase_in", "bwd_prelu", "gslots8", "cin<8", "mg4", "mg4_16B", "mg4_res", "mg2", "mg_off-3"},
    "gemm_tap_kernel": {"M31", "M32", "M33", "M95", "M96", "M97", "gpt_pad", "P%32", "P%128", "taps_pruned", "stride_a", "stride_b", "dilation_a",
                        "dilation_b", "noncontig_in", "out_slice", "out_phase", "res", "two_phase_in2", "bwd_prelu", "gslots8", "stat1", "stat16", "glu_f32",
                        "glu16_lean", "glu16_generic", "glu16_unpaired", "glu_ragged25", "store16_lean", "store16_pair_generic", "store16_unpaired", "in16",
                        "mg4", "mg4_16B", "mg4_res", "mg2", "mg8", "mg_axis_a", "mg_axis_b", "mg_off-0", "mg_off-2", "mg_off-3", "mg_off-5", "mg_m<=8_r1"},
    "gemm_tap_stream_kernel": {"stream", "partial_tile_dropped", "store16_lean", "out_slice"},
    "gemm_halo_kernel": {"halo", "dilation_b", "out_slice"},
    "gemm_thin_wgrad_kernel": {"splits1", "splits>1"},
    "gemm_wgrad_kernel": {"ragged_M", "ragged_K", "bias_row", "taps_pruned"},
    "gemm_wgrad_bf_kernel": {"ragged_M", "ragged_K", "bias_row", "wide_refused_OB%4", "g16_refused"},
    "gemm_wgrad_wide_kernel": {"xcd", "splits>=8", "splits1", "splits_capped", "last_split_short", "OB%64", "OA>1", "ragged_M", "ragged_K", "bias_row",
                               "taps_pruned"},
}


def test_case_table_reaches_every_form():
    reached, edges, unpacks = set(), {}, set()
    for case in CASES:
        fwd, wg, codes = R.host_forms(case)
        assert tuple(fwd + wg) == case.form, (case.id, fwd, wg)
        for name in case.form:
            if name == "refused":
                continue
            reached.add(name)
            edges.setdefault(name.split("<")[0], set()).update(case.edges)
        M, (OA, OB) = (case.cout, case.out_hw)
        P = OA * OB
        # the tags say what the geometry is
        for tag, ok in (("P%256", P % 256), ("P%32", P % 32), ("P%128", P % 128), ("OB%64", OB % 64), ("OA>1", OA > 1 and OB % 4 == 0),
                        ("M31", M == 31), ("M32", M == 32), ("M33", M == 33), ("M95", M == 95), ("M96", M == 96), ("M97", M == 97),
                        ("gpt_pad", case.cin % 8), ("cin<8", case.cin < 8), ("wide_refused_OB%4", OA > 1 and OB % 4)):
            if tag in case.edges:
                assert ok, (case.id, tag)
        # the store-path tags are derived from the geometry the kernel tests (gemm_ref.store_paths), the slice / view tags from what launch() does
        store_tags = {t for t in case.edges if t.startswith(("store16_", "glu16_"))}
        if case.kind == "conv" and (case.out16 or store_tags):
            paths = R.store_paths(case, int(case.form[0].split("<")[1].split(",")[0].rstrip(">")) if "stream" not in case.form[0] else 1)
            assert store_tags and store_tags <= paths, (case.id, store_tags, paths)
        assert ("out_slice" in case.edges) == ("slice" in case.view), case.id
        assert ("noncontig_in" in case.edges) == ("perm" in case.view), case.id
        assert ("slice" not in case.id or "slice" in case.view) and ("perm" not in case.id or "perm" in case.view), case.id   # ids say what runs
        merged = case.kind in ("dgrad", "convT") and "mg" in case.edges
        for tag, ok in (("mg4", merged and max(case.stride) == 4), ("mg2", merged and max(case.stride) == 2), ("mg8", merged and max(case.stride) == 8),
                        ("mg4_16B", merged and case.stride[1] == 4),            # G = 4 along the unit-stride axis: the 16-byte store
                        ("mg_axis_a", merged and case.stride[0] > 1), ("mg_axis_b", merged and case.stride[1] > 1),
                        ("mg4_res", merged and case.stride[1] == 4 and case.res), ("in16", case.in16),
                        ("partial_tile_dropped", M % 32 != 0 and M % 2 == 0 and P % 32 == 0)):
            if tag in case.edges:
                assert ok, (case.id, tag)
        if case.kind == "wgrad":
            v = R.wgrad_decode([c for c in codes if c >= 0][-1])
            unpacks.add((case.unpack, v["splits"] > 1))
            K = case.cin * case.ksize[0] * case.ksize[1] + int(case.bias)
            chunks = case.N * OA * -(-OB // 64)
            for tag, ok in (("xcd", v["xcd"]), ("splits>=8", v["splits"] >= 8), ("splits1", v["splits"] == 1), ("splits>1", v["splits"] > 1),
                            ("splits_capped", v["splits"] == case.wsplits), ("last_split_short", chunks % -(-chunks // v["splits"])),
                            ("ragged_M", M % 32), ("ragged_K", K % 64), ("bias_row", case.bias), ("g16_refused", codes[0] == -1)):
                if tag in case.edges:
                    assert ok, (case.id, tag, v)
            assert v["xcd"] == int(v["splits"] >= 8 and v["family"] == 3)
    assert reached == set(ALL_FORMS), (sorted(set(ALL_FORMS) - reached), sorted(reached - set(ALL_FORMS)))
    assert len(ALL_FORMS) == len(set(ALL_FORMS)) == 82
    for fam, need in REQUIRED_EDGES.items():
        assert need <= edges[fam], (fam, sorted(need - edges[fam]))
    # every unpack entry point, with one and with several splits (rfx_unpack_col rides with "set")
    assert {("set", False), ("set", True), ("add", False), ("add", True), ("add_bias", False), ("add_bias", True)} <= unpacks


# ---- what the bound can see -----------------------------------------------------------------------------------------------------------------
# fault -> (case of the table that names the edge, output judged).  All in the mode whose old bound is the loosest the fault can run in.
FAULTS = {
    "tap_missing_first_col": ("tap-r1-m31-bf16", "y"),
    "tap_missing_last_col": ("tap-r1-m31-bf16", "y"),
    "ragged_row_from_neighbour": ("tap-r2-m33-bf16", "y"),
    "bias_by_row": ("convT-mg4-b", "y"),
    "merged_phase_off_by_one": ("convT-mg4-b", "y"),
    "quad_past_mg_len": ("dgrad-mg4-off3-res", "dx"),
    "glu_halves_swapped": ("tap-r1-glu-f32z-bf16", "z"),
    "residual_twice_one_row": ("tap-r3-m96-res-bf16", "y"),
    "lo_hi_dropped": ("tap-r2-m33-bf16x3", "y"),
    "truncating_store": ("st16-lean", "y"),
    "split_missing": ("wg-wide0-bf16", "dw"),
    "bias_col_k_minus_2": ("wg-wide0-bf16", "db"),
    "pruned_tap_nonzero": ("wg-pruned-bf16", "dw"),
    "one_element_off": ("tap-r2-m33-bf16", "y"),
}
# does the whole-tensor RMS assertion of tests/test_gpu_conv.py, in the fault's mode, accept it on the same inputs?
OLD_ACCEPTS = {
    "tap_missing_first_col": True, "tap_missing_last_col": True, "ragged_row_from_neighbour": False, "bias_by_row": False,
    "merged_phase_off_by_one": False, "quad_past_mg_len": False, "glu_halves_swapped": False, "residual_twice_one_row": True,
    "lo_hi_dropped": False, "truncating_store": True, "split_missing": False, "bias_col_k_minus_2": False, "pruned_tap_nonzero": True,
    "one_element_off": True,
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_bound_rejects_planted_fault(fault):
    cid, name = FAULTS[fault]
    cs, inp, clean = _evaluated(BY_ID[cid])
    got = _restate(cs, inp, fault)
    assert not torch.equal(got[name], clean[name]), "the fault changed nothing"
    res = R.judge(cs, inp, got)
    assert res[name][0] > 1.0, (fault, {k: v[0] for k, v in res.items()})
    accepts = R.old_accepts(cs, inp, got, name)
    print(fault, "new error / tolerance", round(res[name][0], 1), "old RMS assertion accepts:", accepts)
    assert accepts == OLD_ACCEPTS[fault], (fault, accepts)


def test_clean_restatement_is_inside_the_bound():
    """the same judgement accepts the unmutated restatement of every case (a bound that rejects everything rejects the faults too)"""
    for case in CASES:
        cs, inp, got = _evaluated(case)
        res = R.judge(cs, inp, got)
        q = max(v[0] for v in res.values())
        assert q <= 1.0 and q == q, (case.id, {k: v[0] for k, v in res.items()})
