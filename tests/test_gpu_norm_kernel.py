"""Every kernel form of remfx_amd/csrc/norm.hip through the C ABI -- rfx_groupnorm_fwd[_x16], rfx_groupnorm_bwd[_x16],
rfx_batchnorm_fwd, rfx_batchnorm_bwd -- on buffers this test allocates, against tests/norm_ref.py: the fp64 restatement, fed the
kernel's own saved fp32 mean / rstd so that statistics, apply and backward are judged separately, PER ELEMENT, at

    |got - ref| <= (8 x floor + 16 fp32 half-ulps) x eps32 x magnitude     (+ half a bf16 ulp for the stored 16-bit dx)

with magnitude = sum of |terms| the element was formed from and floor = the error of a CPU fp32 restatement with the kernels' partial
sums, in the same units (norm_ref.floors; never measured on the kernel).  What that bound can and cannot see, the walk of the case
table over the dispatch of norm_fwd / norm_bwd and the check that no case's bound is looser than 1e-3 of its output are in
tests/test_norm_ref_cpu.py; the measured floors are in DESIGN.md 4.15.

Buffers: every output is filled with NaN and sits between two NaN guards of 4096 elements; `work` and `sums` have exactly the size
the ABI's sizing functions return (which must agree with their restatement in norm_ref), are filled with NaN and followed by a guard.
After the call no output element is NaN and every guard holds its fill bit for bit.  Every case but the atomic-statistics one runs
twice into fresh buffers: all outputs are the same bits.

Cases above norm_ref.CAP elements draw their samples from a small pool (Case.pool): the device sees the full batch, the fp64
reference is evaluated per pool entry, and the kernel has to return the same statistics bits for equal samples.

The tail of norm.hip -- rfx_glu_fwd / _bwd / _bwd_bf16 and rfx_avgpool2d_fwd / _bwd -- is at the end of this module: the same buffers
through tests/kernel_harness.py (Guarded, judge per element, twice, report), the references and derived bounds of norm_ref (DESIGN.md
4.28)."""
import pytest
import torch

from tests import norm_ref as R
from tests.kernel_harness import Guarded, api, report, stop_after_a_device_error, twice, where  # noqa: F401
from tests.kernel_harness import judge as judge_elements

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]          # no GEMM inside: the arithmetic modes agree

EPS = R.GEN_EPS
TABLE = R.case_table()
def _group(name):
    return [c for c in TABLE if c.group == name]


def _id(c):
    return c.id


def _split_sums(s1, s2, k, gen):
    """fp64 [NG][k][2]: the pairs spread unevenly over k slots (some slots hold almost nothing, one is negative)"""
    w = torch.rand(s1.numel(), k, generator=gen, dtype=torch.float64) ** 4
    w[:, 0] = -0.25
    out = torch.stack([s1[:, None] * w, s2[:, None] * w], -1)
    out[:, k - 1] = torch.stack([s1, s2], -1) - out[:, :k - 1].sum(1)
    return out.contiguous()


def launch(case, inp):
    """one forward (and backward) call on the current stream; y / dx stay on the device, the small outputs come back as CPU tensors"""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    L = _lib.lib()
    N, C, S, G, bn = case.N, case.C, case.S, case.G, case.kind == "bn"
    mode = R.MODES[case.mode]
    Co = C // 2 if R.is_glu(case.mode) else C
    dev = torch.device("cuda", torch.cuda.current_device())
    idx = None if inp["idx"] is None else inp["idx"].to(dev)
    batch = lambda t: None if t is None else (t.to(dev) if idx is None else t.to(dev)[idx]).contiguous()      # noqa: E731
    x = batch(inp["x"])
    if case.x16:
        x = x.to(torch.bfloat16)                               # exact: make_inputs rounded it
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    res, gy = batch(inp["res"]), batch(inp["gy"])
    scale = None if inp["scale"] is None else inp["scale"].to(dev)
    nstat = C if bn else N * G
    y = Guarded(N * Co * S, what="y")
    bufs = [y]
    sums = None
    if case.eval:
        g = torch.Generator().manual_seed(C)
        mean_t, rstd_t = torch.randn(C, generator=g).to(dev), torch.rsqrt(torch.rand(C, generator=g) + 0.5).to(dev)
    else:
        mean, rstd = Guarded(nstat, what="mean"), Guarded(nstat, what="rstd")
        mean_t, rstd_t = mean.t, rstd.t
        bufs += [mean, rstd]
        if bn:
            nsums = int(L.rfx_batchnorm_fwd_ws(N, C, S))
            assert nsums == 2 * C * R.bn_stat_slots(N, S)
            sums = Guarded(nsums, torch.float64, front=False, what="sums")
        elif case.given == -1:
            chunks, nsums = L.rfx_groupnorm_stat_chunks(C, S, G), int(L.rfx_groupnorm_fwd_ws(N, C, S, G))
            assert chunks == R.stat_chunks(C, S, G) and nsums == 2 * N * G * chunks
            sums = Guarded(nsums, torch.float64, front=False, what="sums")
        elif case.given == 0:
            sums = Guarded(2 * N * G, torch.float64, front=False, what="sums")
        else:                                                  # an INPUT: what a GEMM epilogue would have left, (NG, 2) or (NG, k, 2)
            s1, s2, _ = R.moments(inp["x"], case.kind, G)
            sums = Guarded(2 * N * G * case.given, torch.float64, front=False, what="sums")
            sums.t.copy_(_split_sums(s1, s2, case.given, torch.Generator().manual_seed(case.given)).reshape(-1))
    sp = _ptr(sums.t) if sums is not None else None
    if bn:
        rc = L.rfx_batchnorm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), N, C, S, EPS, mode, int(case.eval), sp, _ptr(mean_t), _ptr(rstd_t),
                                 _ptr(y.t), _stream())
    else:
        fwd = L.rfx_groupnorm_fwd_x16 if case.x16 else L.rfx_groupnorm_fwd
        rc = fwd(_ptr(x), _ptr(gamma), _ptr(beta), N, C, S, G, EPS, mode, _ptr(res), _ptr(scale), sp, case.given, _ptr(mean_t),
                 _ptr(rstd_t), _ptr(y.t), _stream())
    assert rc == 0, ("forward", rc)
    torch.cuda.synchronize()
    for b in bufs:
        b.owned()
    if sums is not None:
        sums.guards_intact()
    got = {"y": y.t.view(N, Co, S), "mean": mean_t.cpu(), "rstd": rstd_t.cpu()}
    if case.bwd:
        nw = L.rfx_norm_bwd_work_floats(N, C, S, 0 if bn else G)
        assert nw == R.work_floats(N, C, S, 0 if bn else G)
        work = Guarded(nw, front=False, what="work")
        dx = Guarded(N * C * S, torch.bfloat16 if case.x16 else torch.float32, what="dx")
        dgamma, dbeta = Guarded(C, what="dgamma"), Guarded(C, what="dbeta")
        outs = [dx, dgamma, dbeta]
        dscale = None
        if case.mode == "glu_scale_res":
            dscale = Guarded(Co, what="dscale")
            outs.append(dscale)
        if bn:
            rc = L.rfx_batchnorm_bwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean_t), _ptr(rstd_t), _ptr(gy), N, C, S, mode, _ptr(work.t),
                                     _ptr(dx.t), _ptr(dgamma.t), _ptr(dbeta.t), _stream())
        else:
            bwd = L.rfx_groupnorm_bwd_x16 if case.x16 else L.rfx_groupnorm_bwd
            rc = bwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean_t), _ptr(rstd_t), _ptr(gy), N, C, S, G, mode, _ptr(scale), _ptr(work.t),
                     _ptr(dx.t), _ptr(dgamma.t), _ptr(dbeta.t), _ptr(dscale.t if dscale else None), _stream())
        assert rc == 0, ("backward", rc)
        torch.cuda.synchronize()
        for b in outs:
            b.owned()
        work.guards_intact()
        got.update(dx=dx.t.view(N, C, S), dgamma=dgamma.t.cpu(), dbeta=dbeta.t.cpu())
        if dscale:
            got["dscale"] = dscale.t.cpu()
    return got


def _pool_stat(v, idx, P):
    """statistics per pool entry; equal samples must have given the same bits"""
    if idx is None:
        return v
    p = torch.zeros(P, v.numel() // idx.numel(), dtype=v.dtype)
    p[idx] = v.view(idx.numel(), -1)
    assert torch.equal(p[idx].reshape(-1), v), "equal samples, different statistics"
    return p.reshape(-1)


def judge_statistics(case, inp, got):
    x, idx = inp["x"], inp["idx"]
    mk, rk = (_pool_stat(got[k], idx, x.shape[0]).double() for k in ("mean", "rstd"))
    if case.given >= 1 and case.kind == "gn":
        # the sums were handed over: fp64 finalize, then ONE rounding to fp32
        m, r = R.finalize(*R.moments(x, case.kind, case.G), EPS)
        for name, k, ref in (("mean", mk, m), ("rstd", rk, r)):
            q, i = R.worst(k, ref, 0.5 * R.ulp(ref, 23) * (1 + 1e-6) + 1e-300)
            assert q <= 1.0, (case.id, name, "not the fp32 rounding of the fp64 value", i, float(k[i]), float(ref[i]))
        return {}
    m, r = R.stats(x, case.kind, case.G, EPS)
    mag, fl = R.stat_magnitudes(x, case.kind, case.G, EPS), R.stat_floors(x, case.kind, case.G, EPS)
    q, i = R.worst(mk, m, R.k_of(fl["mean"]) * R.EPS32 * mag["mean"])
    assert q <= 1.0, (case.id, case.forms()[0], "mean", i, q, float(mk[i]), float(m[i]), fl)
    rel = (rk - r) / r
    q, i = R.worst(rel, torch.zeros_like(rel), R.k_of(fl["rstd"]) * R.EPS32 * mag["rstd"])
    assert q <= 1.0, (case.id, case.forms()[0], "rstd", i, q, float(rk[i]), float(r[i]), fl)
    return {"rstd_rel": float(rel.abs().max()), "rstd_bound": float((R.k_of(fl["rstd"]) * R.EPS32 * mag["rstd"]).max()), "floors": fl}


def judge(case, inp, got, last4=False):
    """apply and backward per element against the fp64 reference fed the kernel's statistics"""
    idx = inp["idx"]
    P = inp["x"].shape[0]
    mk, rk = (_pool_stat(got[k], idx, P).double() for k in ("mean", "rstd"))
    ref, mag, slack, fl = R.floors(inp, mk, rk, case)
    names = case.forms()[0]
    for name in ref:
        tol = R.tolerance(name, ref, mag, slack, fl, case.x16)
        g, r = got[name], ref[name]
        if name in ("y", "dx"):                                # on the device: the pool cases hold 25 M elements
            r, tol = r.to(g.device), tol.to(g.device)
            if idx is not None:
                r, tol = r[idx.to(g.device)], tol[idx.to(g.device)]
            if last4:
                q, i = R.worst(g[..., -4:], r[..., -4:], tol[..., -4:])
                assert q <= 1.0, (case.id, names, name, "last 4 samples of row", where(i, g[..., -4:].shape)[:2], q)
        q, i = R.worst(g, r, tol)
        assert q <= 1.0, (case.id, names, name, "element", where(i, tuple(g.shape)), "error / bound", q, "got", float(g.reshape(-1)[i]),
                          "ref", float(r.reshape(-1)[i]), "floor", fl[name])
    return fl


def run(case, statistics=True, last4=False):
    inp = R.make_inputs(case)
    got = launch(case, inp)
    info = {}
    if statistics and not case.eval:
        info = judge_statistics(case, inp, got)
    judge(case, inp, got, last4)
    if case.given != 0 or case.kind == "bn":
        again = launch(case, inp)
        for k in got:
            assert torch.equal(got[k], again[k]), (case.id, k, "second run differs")
    return inp, got, info


@pytest.mark.parametrize("case", _group("stats"), ids=_id)
def test_statistics(case):
    """slotted, atomic and handed-over sums ((NG, 2) and (NG, 16, 2)) at every chunk shape; BatchNorm with 70 and 6 slots per channel"""
    run(case)


@pytest.mark.parametrize("case", _group("const"), ids=_id)
def test_constant_rows(case):
    """var = 0 (the clamp), rstd = 1 / sqrt(eps), y = beta exactly"""
    inp, got, _ = run(case, statistics=False)
    N, C, S, G = case.N, case.C, case.S, case.G
    assert torch.equal(got["mean"], inp["x"][:, ::C // G, 0].reshape(-1))
    e = float(torch.tensor(EPS, dtype=torch.float32))
    assert torch.equal(got["rstd"], torch.full((N * G,), 1.0 / e ** 0.5, dtype=torch.float64).float())
    assert torch.equal(got["y"].cpu(), inp["beta"].view(1, C, 1).expand(N, C, S))


@pytest.mark.parametrize("case", _group("largemean"), ids=_id)
def test_large_mean(case):
    """x = m + randn: E[x^2] - m^2 loses log2(1 + m^2 / var) bits.  The kernel has to stay inside the algorithm's error model
    0.5 K eps32 E[x^2] / (var + eps); the apply pass, fed the kernel's statistics, keeps its usual bound"""
    _, _, info = run(case)
    print(f"\nLARGEMEAN {case.id} kernel_rel={info['rstd_rel']:.3e} model_bound={info['rstd_bound']:.3e} floors={info['floors']}")
    if not case.x16:
        ratio, rt, cpu32, tch, bound = R.large_mean_row(int(case.xkind[4:]))
        print(f"LARGEMEAN {case.xkind} mean/std={ratio:.4g} rstd64={rt:.9g} cpu_lanes32_rel={cpu32:.3e} torch_f32_rel={tch:.3e} model_bound={bound:.3e}")


@pytest.mark.parametrize("case", _group("rows"), ids=_id)
def test_row_kernels(case):
    """gn_apply_rows_kernel / gn_bwd_apply_rows_kernel at 1, 1, 1, 2, 2, 3 and 5 items of 256 samples per row, ragged and exact: the
    last item of every row, named on failure"""
    run(case, last4=True)


@pytest.mark.parametrize("case", _group("edge"), ids=_id)
def test_grid_edges(case):
    """scalar grid-stride kernels (S odd), the vector ones (C > 65535), gridDim.z = 65535 < N in both row kernels, BatchNorm eval"""
    run(case)


def test_16_bit_forms_refuse_wide_C():
    """C > 65535 has no row-kernel decode and the grid-stride kernels read fp32: the 16-bit ABI says so instead of launching"""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    L = _lib.lib()
    N, C, S = 1, 65540, 4
    x = torch.zeros(N * C * S, device="cuda", dtype=torch.bfloat16)
    f = lambda n: torch.zeros(n, device="cuda")                # noqa: E731
    g, b, mean, rstd, y, gy = f(C), f(C), f(N), f(N), f(N * C * S), f(N * C * S)
    sums = torch.zeros(2 * N * R.stat_chunks(C, S, 1), device="cuda", dtype=torch.float64)
    assert L.rfx_groupnorm_fwd_x16(_ptr(x), _ptr(g), _ptr(b), N, C, S, 1, EPS, 0, None, None, _ptr(sums), -1, _ptr(mean), _ptr(rstd),
                                   _ptr(y), _stream()) == -1
    work = f(R.work_floats(N, C, S, 1))
    dx = torch.zeros_like(x)
    assert L.rfx_groupnorm_bwd_x16(_ptr(x), _ptr(g), _ptr(b), _ptr(mean), _ptr(rstd), _ptr(gy), N, C, S, 1, 0, None, _ptr(work), _ptr(dx),
                                   _ptr(f(C)), _ptr(f(C)), None, _stream()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", _group("generic"), ids=_id)
def test_generic_backward(case):
    """gn_bwd_partial (+ gn_bwd_slotsum at 4 ragged and 2 exact chunks), group and channel sums, G = C, BatchNorm backward"""
    run(case)


@pytest.mark.parametrize("case", _group("sample"), ids=_id)
def test_per_sample_backward(case):
    """G = 1, N = 513: the wave-per-sample, register-resident and workgroup-per-sample kernels at the edges of their channel and
    sample ranges"""
    run(case)


@pytest.mark.parametrize("case", _group("chansum"), ids=_id)
def test_channel_sums(case):
    """sliced channel sums with NS = 64, 32 and 1 at N >= 2048; N = 511: the generic side of the N >= 512 switch"""
    run(case)


@pytest.mark.parametrize("case", _group("switch"), ids=_id)
def test_sample_size_switch(case):
    """C * S = 65536 (per-sample path) and just above it (generic path)"""
    run(case)


def test_handed_over_sums_through_the_wrapper():
    """nnops.group_norm(sums=...) in both layouts ops.py produces, (N * G, 2) and (N * G, slots, 2): y inside the bound of the
    reference fed the fp32 rounding of the fp64 statistics"""
    from remfx_amd import nnops
    case = R.Case("stats", "gn", 3, 6, 4100, 3, "gelu", bwd=False)
    inp = R.make_inputs(case)
    x, w, b = (inp[k].cuda() for k in ("x", "gamma", "beta"))
    s1, s2, n = R.moments(inp["x"], "gn", 3)
    m, r = (t.float().double() for t in R.finalize(s1, s2, n, EPS))
    ref, mag, slack, fl = R.floors(inp, m, r, case)
    for sums in (torch.stack([s1, s2], -1), _split_sums(s1, s2, 16, torch.Generator().manual_seed(1))):
        y = nnops.group_norm(x, 3, w, b, EPS, "gelu", sums=sums.cuda())
        q, i = R.worst(y.cpu(), ref["y"], R.tolerance("y", ref, mag, slack, fl))
        assert q <= 1.0, (tuple(sums.shape), where(i, tuple(y.shape)), q)


# ---- plain GLU ------------------------------------------------------------------------------------------------------------------------
def _glu_call(entry, N, C, S, x, gy, offs=(0, 0, 0)):
    """one call into fresh guarded buffers -> (return code, the output buffer); the inputs have to come back bit for bit"""
    L, _, stream = api()
    xdt = torch.bfloat16 if entry == "bwd_bf16" else torch.float32
    Co = C // 2
    X = Guarded(max(N, 0) * C * S, xdt, "x", x, offs[0])
    if entry == "fwd":
        O = Guarded(max(N, 0) * Co * S, what="y", off=offs[1])
        rc = L.rfx_glu_fwd(X.ptr(), O.ptr(), N, C, S, stream())
        ins = (X,)
    else:
        G = Guarded(max(N, 0) * Co * S, what="gy", init=gy, off=offs[2])
        O = Guarded(max(N, 0) * C * S, xdt, "gx", off=offs[1])
        fn = L.rfx_glu_bwd_bf16 if entry == "bwd_bf16" else L.rfx_glu_bwd
        rc = fn(X.ptr(), G.ptr(), O.ptr(), N, C, S, stream())
        ins = (X, G)
    torch.cuda.synchronize()
    for b in ins:
        b.unchanged()
    return rc, O


def _glu_case(entry, N, C, S, offs=(0, 0, 0)):
    """-> (the output, largest error / bound)"""
    x16 = entry == "bwd_bf16"
    x, gy = R.glu_data(N, C, S, x16=x16)
    forms = R.forms_glu(entry, N, C, S, offs)
    name = "y" if entry == "fwd" else "gx"
    info = ("rfx_glu_" + entry, (N, C, S), "offsets", offs, sorted(forms))

    def run():
        rc, O = _glu_call(entry, N, C, S, x, gy, offs)
        assert rc == 0, (rc, *info)
        O.owned()
        return {name: O.cpu()}
    got = twice(run)[0][name]
    ref = R.glu(x, None if entry == "fwd" else gy)[name]
    bound = R.glu_bounds(x, None if entry == "fwd" else gy)[name]
    if x16:
        bound = R.bf16_store_bound(ref, bound)
    return got, judge_elements(got, ref, bound, exact="value", ctx=info)


@pytest.mark.parametrize("entry", R.GLU_ENTRIES)
@pytest.mark.parametrize("shape", R.GLU_ROW_CASES, ids=str)
def test_glu_row_kernels(shape, entry):
    """(C / 2) S a multiple of 4 and every base aligned: one vector, a second chunk of one vector (the o >= L exit), a last workgroup
    with an idle wave, two full chunks"""
    assert any(f.endswith(":rows") for f in R.forms_glu(entry, *shape))
    report("NORM", f"rfx_glu_{entry} rows {shape}", [_glu_case(entry, *shape)[1]])


@pytest.mark.parametrize("entry", ("fwd", "bwd"))
@pytest.mark.parametrize("shape", R.GLU_FLAT_CASES, ids=str)
def test_glu_flat_kernels(shape, entry):
    assert f"glu_{entry}_kernel:flat" in R.forms_glu(entry, *shape)
    report("NORM", f"rfx_glu_{entry} flat {shape}", [_glu_case(entry, *shape)[1]])


@pytest.mark.parametrize("entry", ("fwd", "bwd"))
@pytest.mark.parametrize("shape", R.GLU_ROW_CASES, ids=str)
def test_glu_misaligned_base_takes_the_flat_kernel(shape, entry):
    """each base in turn one element past a 16-byte boundary: the flat kernel, the same bound; and, the flat and the row kernel being
    the same arithmetic, the aligned run's bits"""
    aligned = _glu_case(entry, *shape)[0]
    ratios = []
    for i in range(2 if entry == "fwd" else 3):
        offs = tuple(int(j == i) for j in range(3))
        assert R.forms_glu(entry, *shape, offs) == {f"glu_{entry}_kernel:flat"}
        got, q = _glu_case(entry, *shape, offs)
        ratios.append(q)
        assert torch.equal(got.view(torch.int32), aligned.view(torch.int32)), (entry, shape, offs, "differs from the aligned run")
    report("NORM", f"rfx_glu_{entry} misaligned {shape}", ratios)


@pytest.mark.parametrize("shape", R.GLU_CAP_CASES, ids=str)
def test_glu_past_the_grid_cap(shape):
    """more than 4096 x 1024 outputs: the flat kernels' grid-stride loop runs again, the row kernels' grid grows"""
    ratios = []
    for entry in R.GLU_ENTRIES:
        forms = R.forms_glu(entry, *shape)
        if forms is None:
            continue
        assert shape[0] * (shape[1] // 2) * shape[2] > R.GLU_GRID_CAP
        ratios.append((entry, _glu_case(entry, *shape)[1]))
    assert ratios
    report("NORM", f"rfx_glu cap {shape}", ratios)


def test_glu_refusals_write_nothing():
    """the 16-bit form has no flat kernel: every flat shape and every misaligned base is refused; so are an odd C, N = 0 and NULL"""
    L, _, stream = api()
    for shape in R.GLU_FLAT_CASES:
        assert R.forms_glu("bwd_bf16", *shape) is None
        x, gy = R.glu_data(*shape, x16=True)
        rc, O = _glu_call("bwd_bf16", *shape, x, gy)
        assert rc != 0, shape
        O.untouched()
    shape = R.GLU_ROW_CASES[1]
    x, gy = R.glu_data(*shape, x16=True)
    for offs in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2)):
        assert R.forms_glu("bwd_bf16", *shape, offs) is None
        rc, O = _glu_call("bwd_bf16", *shape, x, gy, offs)
        assert rc != 0, offs
        O.untouched()
    for entry in R.GLU_ENTRIES:
        for (N, C, S) in ((2, 3, 4), (0, 2, 4), (2, 0, 4), (2, 2, 0)):
            assert R.forms_glu(entry, N, C, S) is None
            rc, O = _glu_call(entry, N, C, S, torch.ones(N * C * S), torch.ones(N * (C // 2) * S))
            assert rc != 0, (entry, N, C, S)
            O.untouched()
    O = Guarded(16, what="y")
    X = Guarded(32, what="x", init=torch.ones(32))
    assert L.rfx_glu_fwd(None, O.ptr(), 2, 4, 4, stream()) != 0 and L.rfx_glu_fwd(X.ptr(), None, 2, 4, 4, stream()) != 0
    G = Guarded(32, what="gx")
    assert L.rfx_glu_bwd(X.ptr(), None, G.ptr(), 2, 4, 4, stream()) != 0 and L.rfx_glu_bwd(None, X.ptr(), G.ptr(), 2, 4, 4, stream()) != 0
    assert L.rfx_glu_bwd_bf16(X.ptr(), None, G.ptr(), 2, 4, 4, stream()) != 0
    torch.cuda.synchronize()
    O.untouched()
    G.untouched()
    X.unchanged()
    report("NORM", "rfx_glu refusals", [])


# ---- average pooling ------------------------------------------------------------------------------------------------------------------
def _pool_call(bwd, NC, H, W, kh, kw, src, n_out):
    L, _, stream = api()
    I = Guarded(src.numel(), what="gy" if bwd else "x", init=src)
    O = Guarded(n_out, what="gx" if bwd else "y")
    rc = (L.rfx_avgpool2d_bwd if bwd else L.rfx_avgpool2d_fwd)(I.ptr(), O.ptr(), NC, H, W, kh, kw, stream())
    torch.cuda.synchronize()
    I.unchanged()
    return rc, O


def _pool_case(bwd, NC, H, W, kh, kw):
    x, gy = R.pool_data(NC, H, W, kh, kw)
    info = ("rfx_avgpool2d_" + ("bwd" if bwd else "fwd"), (NC, H, W, kh, kw), sorted(R.forms_pool(bwd, NC, H, W, kh, kw)))
    ref, bound = R.pool_bwd(gy, H, W, kh, kw) if bwd else R.pool_fwd(x, kh, kw)

    def run():
        rc, O = _pool_call(bwd, NC, H, W, kh, kw, gy if bwd else x, ref.numel())
        assert rc == 0, (rc, *info)
        O.owned()
        return {"out": O.cpu()}
    return judge_elements(twice(run)[0]["out"], ref, bound, ctx=info)


@pytest.mark.parametrize("shape", R.POOL_CASES, ids=str)
def test_avgpool(shape):
    """forward: the window mean inside its counted half-ulps; backward: bit for bit where kh kw is a power of two (+0 in the remainder
    rows and columns everywhere), two half-ulps otherwise"""
    report("NORM", f"rfx_avgpool2d {shape}", [("fwd", _pool_case(False, *shape)), ("bwd", _pool_case(True, *shape))])


def test_avgpool_past_the_grid_cap():
    assert "grid_capped" in R.forms_pool(False, *R.POOL_CAP_FWD) and "grid_capped" in R.forms_pool(True, *R.POOL_CAP_BWD)
    report("NORM", "rfx_avgpool2d cap", [("fwd", _pool_case(False, *R.POOL_CAP_FWD)), ("bwd", _pool_case(True, *R.POOL_CAP_BWD))])


def test_avgpool_refusals_write_nothing():
    L, _, stream = api()
    for shape in R.POOL_REFUSED:
        NC, H, W, kh, kw = shape
        assert R.forms_pool(False, *shape) is None and R.forms_pool(True, *shape) is None
        for bwd in (False, True):
            rc, O = _pool_call(bwd, NC, H, W, kh, kw, torch.ones(64), 64)
            assert rc != 0, (shape, bwd)
            O.untouched()
    O = Guarded(64, what="out")
    I = Guarded(64, what="in", init=torch.ones(64))
    for fn in (L.rfx_avgpool2d_fwd, L.rfx_avgpool2d_bwd):
        assert fn(None, O.ptr(), 1, 4, 4, 2, 2, stream()) != 0 and fn(I.ptr(), None, 1, 4, 4, 2, 2, stream()) != 0
    torch.cuda.synchronize()
    O.untouched()
    I.unchanged()
    report("NORM", "rfx_avgpool2d refusals", [])
