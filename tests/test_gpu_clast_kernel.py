"""GPU: every launchable form of the channels-last bf16 trunk (csrc/cl_conv.h + cl_conv_m_*.hip, cl_wgrad.hip, cl_elem.hip) through the
shipped launch path (clast.pack / conv / wgrad and the cl_elem wrappers), judged PER ELEMENT against the operand-rounded fp64 reference
of tests/clast_ref.py.  Each case names the instantiation it is meant to reach; the launchers' own variant codes
(rfx_cl_conv_variant / rfx_cl_wgrad_variant) must agree before anything is judged.  Outputs are NaN-filled between NaN guards; every case
runs twice into fresh buffers and must come back bit for bit (nothing here is atomic)."""
import pytest
import torch

from tests import clast_ref as R
from tests.kernel_harness import Arena, stop_after_a_device_error  # noqa: F401
from tests.kernel_harness import guarded as _guarded

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

CONV = R.conv_cases()
WGRAD = R.wgrad_cases()
DEV = "cuda:0"


def _fetch(out, what):
    got = {k: v.float().cpu() for k, v in out.items()}
    for k, v in got.items():
        assert not bool(torch.isnan(v).any()), (what, k, "element left unwritten")
    return got


def _run_conv(case, inp):
    arena = Arena(DEV)
    with R.recorder(False) as tr:
        out, spare = _guarded(lambda: R.launch_conv(case, inp, DEV, arena.alloc), case.id)
        codes = list(tr)
    assert [R.conv_name(c) for k, c in codes] == [case.form], (case.id, codes)
    arena.check()
    for s in spare:
        assert bool(torch.isnan(s).all()), (case.id, "store outside the channel slice / the strided view")
    return _fetch(out, case.id)


@pytest.mark.parametrize("case", CONV, ids=[c.id for c in CONV])
def test_conv_form(case):
    inp = R.conv_inputs(case)
    got = _run_conv(case, inp)
    res = R.conv_judge(case, inp, got, R.K_conv(case))
    print(case.id, case.form, {k: round(v["q"], 3) for k, v in res.items()},
          "fp32", {k: round(R.floor_of(v, got[k], k != "cm"), 3) for k, v in res.items()})   # the error beyond the 16-bit half ulps / the fp32 part
    for k, v in res.items():
        i = v["idx"]
        assert v["q"] <= 1.0, (case.id, k, "error / tolerance", v["q"], "flat index", i, "got", float(got[k].reshape(-1)[i]), "ref",
                               float(v["val"].reshape(-1)[i]))
    again = _run_conv(case, inp)
    for k in got:
        assert torch.equal(got[k], again[k]), (case.id, k, "second run differs")
    # the non-storing variant of a mode computes the same out1 / out0 bit for bit
    twin = {"gelu": "out0", "glu": "out0", "dgelu": "out0", "dglu": "out1"}.get(case.mode)
    if twin and getattr(case, twin):
        import dataclasses
        lean = dataclasses.replace(case, **{twin: False})
        other = _run_conv(lean, inp)
        for k in other:
            assert torch.equal(other[k], got[k]), (case.id, k, "differs without", twin)


def _run_wgrad(case, inp):
    arena = Arena(DEV)
    with R.recorder(False, case.splits) as tr:
        out = _guarded(lambda: R.launch_wgrad(case, inp, DEV, arena.alloc), case.id)
        codes = list(tr)
    assert [R.wgrad_name(c) for k, c in codes] == [(case.form, case.order)], (case.id, codes)
    arena.check()
    return _fetch(out, case.id)


@pytest.mark.parametrize("case", WGRAD, ids=[c.id for c in WGRAD])
def test_wgrad_form(case):
    inp = R.wgrad_inputs(case)
    got = _run_wgrad(case, inp)
    res = R.wgrad_judge(case, inp, got, R.K_wgrad())
    print(case.id, case.form, case.order, {k: round(v["q"], 3) for k, v in res.items()})
    for k, v in res.items():
        i = v["idx"]
        assert v["q"] <= 1.0, (case.id, k, "error / tolerance", v["q"], "flat index", i, "got", float(got[k].reshape(-1)[i]), "ref",
                               float(v["val"].reshape(-1)[i]))
    again = _run_wgrad(case, inp)
    for k in got:
        assert torch.equal(got[k], again[k]), (case.id, k, "second run differs")


# ---- cl_elem.hip: every entry point -----------------------------------------------------------------------------------------------------------
K_ELEM = R.k_of(R.FLOORS["elem"])


def _rand(shape, seed, bf16=True):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return R.bf16_rne(t) if bf16 else t


def _cm_src(x, dtype, strided):
    """channel-major source on the device, optionally a strided view (row and channel strides larger than dense)"""
    x = x.to(dtype)
    if not strided:
        return x.to(DEV)
    N, C, A, B = x.shape
    wide = torch.zeros(N, C + 1, A + 1, B, dtype=dtype)
    wide[:, :C, :A] = x
    return wide.to(DEV)[:, :C, :A]


@pytest.mark.parametrize("mode", ["store", "gelu", "dgelu", "dglu"])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("C,B,src16", [(8, 64, False), (40, 192, True), (48, 64, True), (256, 192, False)])
def test_from_cm(mode, res, C, B, src16):
    from remfx_amd import clast
    N, A = 2, 3
    x = _rand((N, C, A, B), C + B, bf16=src16)
    r = _rand((N, C, A, B), C + B + 1) if res else None
    aux = _rand((N, 2 * C if mode == "dglu" else C, A, B), C + B + 2) if mode in ("dgelu", "dglu") else None
    Co = 2 * C if mode == "dglu" else C
    outs = []
    for rep in range(2):
        arena = Arena(DEV)
        wide = arena.alloc((N, A, B, Co + 16), torch.bfloat16)                      # the destination is a channel slice
        dst = wide[..., 8:8 + Co]
        src = _cm_src(x, torch.bfloat16 if src16 else torch.float32, strided=(C == 40))
        _guarded(lambda: clast.from_cm(src, out=dst, res=None if r is None else R.cl(r).to(torch.bfloat16).to(DEV),
                                       aux=None if aux is None else R.cl(aux).to(torch.bfloat16).to(DEV), mode=mode), "from_cm")
        arena.check()
        assert bool(torch.isnan(wide[..., :8]).all()) and bool(torch.isnan(wide[..., 8 + Co:]).all())
        outs.append(R.cm(dst.float().cpu()))
    assert torch.equal(outs[0], outs[1])
    assert not bool(torch.isnan(outs[0]).any())
    q, i = R.from_cm_judge(mode, x, r, aux, outs[0], K_ELEM)
    print("from_cm", mode, res, C, B, src16, round(q, 3))
    assert q <= 1.0, (q, i)
    if mode == "store" and not res:
        assert torch.equal(outs[0], R.bf16_rne(x.float()))                           # a pure conversion is exact


@pytest.mark.parametrize("dst16", [False, True])
@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("C,B", [(8, 64), (40, 192), (48, 192), (256, 64)])
def test_to_cm(dst16, aux, C, B):
    from remfx_amd import clast
    N, A = 2, 3
    x = _rand((N, C, A, B), 7 * C + B)
    z = _rand((N, C, A, B), 7 * C + B + 1) if aux else None
    outs = []
    dt = torch.bfloat16 if dst16 else torch.float32
    for rep in range(2):
        arena = Arena(DEV)
        wide = arena.alloc((N, C + 1, A + 1, B), dt)                                  # a strided destination
        dst = wide[:, :C, :A]
        z16 = None
        if aux:
            zw = torch.zeros((N, C + 1, A + 1, B), dtype=torch.bfloat16)
            zw[:, :C, :A] = z.to(torch.bfloat16)
            z16 = zw.to(DEV)[:, :C, :A]                                               # dst's strides
        xin = torch.zeros(N, A, B, C + 16, dtype=torch.bfloat16)
        xin[..., 8:8 + C] = R.cl(x).to(torch.bfloat16)
        xs = xin.to(DEV)[..., 8:8 + C]                                                # a channel slice as the source
        _guarded(lambda: clast.to_cm(xs, out=dst, aux16=z16), "to_cm")
        arena.check()
        assert bool(torch.isnan(wide[:, C:]).all()) and bool(torch.isnan(wide[:, :C, A:]).all())
        outs.append(dst.float().cpu())
    assert torch.equal(outs[0], outs[1])
    xd = x.double()
    if not aux:
        assert torch.equal(outs[0].double(), xd)
        return
    val = xd * R.dgelu(z.double())
    t = K_ELEM * R.EPS32 * xd.abs() * R.dgelu_w(z.double())
    if dst16:
        t = t + R.half16(val, t)
    q, i = R.worst(outs[0], val, t)
    print("to_cm", dst16, C, B, round(q, 3))
    assert q <= 1.0, (q, i)


@pytest.mark.parametrize("C,npos", [(8, 64), (40, 192), (256, 64)])
def test_dgelu_dglu(C, npos):
    from remfx_amd import clast
    g = _rand((1, C, 1, npos), C)
    z = _rand((1, C, 1, npos), C + 1)
    zab = _rand((1, 2 * C, 1, npos), C + 2)
    gd, zd, zabd = (R.cl(t).to(torch.bfloat16).to(DEV) for t in (g, z, zab))
    o1 = _guarded(lambda: clast.dgelu(gd, zd), "dgelu")
    o2 = _guarded(lambda: clast.dglu(gd, zabd), "dglu")
    assert torch.equal(o1, _guarded(lambda: clast.dgelu(gd, zd), "dgelu")) and torch.equal(o2, _guarded(lambda: clast.dglu(gd, zabd), "dglu"))
    q1, _ = R.from_cm_judge("dgelu", g, None, z, R.cm(o1.float().cpu()), K_ELEM)
    q2, _ = R.from_cm_judge("dglu", g, None, zab, R.cm(o2.float().cpu()), K_ELEM)
    print("dgelu / dglu", C, npos, round(q1, 3), round(q2, 3))
    assert q1 <= 1.0 and q2 <= 1.0


@pytest.mark.parametrize("N,A,XA,C,B,acc", [(5, 1, 1, 8, 64, False), (3, 1, 4, 40, 192, True), (7, 3, 3, 48, 64, False), (2100, 1, 1, 8, 64, True), (3, 1, 1, 256, 64, False),
                                           (2, 5, 5, 48, 192, True)])
def test_rowsum(N, A, XA, C, B, acc):
    """A == 1 with the rows folded into N, A > 1 (the frequency embedding's gradient), N % G != 0 (N = 2100 on G = 2048), accumulate"""
    from remfx_amd import _lib, clchain
    Nf = N * XA if A == 1 else N                               # samples after clchain.rowsum folded the rows
    G = max(1, min(Nf, -(-2048 // A)))                         # its split, a launch argument: `partial` is G partials of A * C floats
    assert _lib.lib().rfx_cl_rowsum_ws(Nf, A, B, C, G) == G * A * C
    assert _lib.lib().rfx_cl_rowsum_ws(Nf, A, B, 12, G) == -1 and _lib.lib().rfx_cl_rowsum_ws(Nf, A, B, C, 0) == -1
    x = _rand((N, XA, B, C), N + C)
    xd = x.to(torch.bfloat16).to(DEV)
    base = _rand((A, C), 3, bf16=False) * 50
    outs = []
    for rep in range(2):
        arena = Arena(DEV)
        out = arena.alloc((A, C), torch.float32)
        out.copy_(base.to(DEV)) if acc else None
        _guarded(lambda: clchain.rowsum(xd, A, C, out, scale=0.5, accumulate=acc), "rowsum")
        arena.check()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    xs = x.double().reshape(-1, A, B, C) if A == 1 else x.double()
    val = 0.5 * xs.sum((0, 2))
    mag = 0.5 * xs.abs().sum((0, 2))
    if acc:
        val, mag = val + base.double(), mag + base.double().abs()
    q, i = R.worst(outs[0], val, R.k_of(R.FLOORS["rowsum"]) * R.EPS32 * mag)
    print("rowsum", N, A, C, B, acc, round(q, 3))
    assert q <= 1.0, (q, i)


@pytest.mark.parametrize("along_b", [False, True])
@pytest.mark.parametrize("Cs", [1, 2])
def test_im2col_s4(along_b, Cs):
    """exact: a gather of bf16(x); the clipped taps (first / last two rows or positions) read as zero"""
    from remfx_amd import clast
    N, OA, OB = 2, 3, 64
    IA, IB = (OA, 4 * OB) if along_b else (4 * OA, OB)
    x = _rand((N, Cs, IA, IB), 11 + Cs, bf16=False)
    wide = torch.zeros(N, Cs + 1, IA + 1, IB)
    wide[:, :Cs, :IA] = x
    out = _guarded(lambda: clast.im2col_s4(wide.to(DEV)[:, :Cs, :IA], OA, OB, along_b), "im2col_s4")
    ref = R.im2col_ref(x, OA, OB, along_b)
    assert torch.equal(out.cpu().double(), ref)
    assert bool((ref[..., 8 * Cs:] == 0).all())


def test_im2col_fm_direct():
    """rfx_cl_im2col_fm against its own statement (a x + b, rounded once; zero outside [0, bins)), not against im2col_s4"""
    from remfx_amd import clast
    N, Fr, bins = 2, 40, 36
    spec = _rand((N, Fr, bins, 2), 5, bf16=False)
    a = torch.tensor([0.7, 1.3])
    b = torch.tensor([0.1, -0.2])
    out = _guarded(lambda: clast.im2col_fm(spec.to(DEV), a.to(DEV), b.to(DEV)), "im2col_fm").cpu().double()
    lo = spec.double() * a.double().view(N, 1, 1, 1) + b.double().view(N, 1, 1, 1)
    x_cm = lo.permute(0, 3, 2, 1)                                                    # (N, 2, bins, F)
    OA = bins // 4
    xp = torch.nn.functional.pad(x_cm, (0, 0, 2, 6))
    ref = torch.zeros(N, OA, Fr, 16, dtype=torch.float64)
    for k in range(8):
        for c in range(2):
            ref[..., 2 * k + c] = xp[:, c, k:k + 4 * OA:4, :][:, :OA]
    tol = 2 * R.EPS32 * (spec.double().abs().max() * 1.3 + 0.2)
    q, i = R.worst(out, ref, tol + R.half16(ref, tol) * (ref != 0))
    assert q <= 1.0, (q, i)
    assert bool((out[:, 0, :, :4] == 0).all()) and bool((out[:, -1, :, 12:] == 0).all())


def test_pack_with_structural_zeros():
    from remfx_amd import clast, clchain
    f = clchain.form("s4f", 48, 16)
    assert (f.idx < 0).any()
    w = _rand((48, 16, 1, 8), 9, bf16=False)
    ap = _guarded(lambda: clast.pack(f, w.to(DEV)), "pack").cpu().float()
    idx = torch.from_numpy(f.idx).long()
    ref = torch.where(idx >= 0, R.bf16_rne(w.reshape(-1))[idx.clamp_min(0)], torch.zeros(()))
    assert torch.equal(ap, ref)
