"""Every attention kernel form (remfx_amd/csrc/attention.hip, attention_mfma.hip) through the C ABI -- rfx_localstate_fwd / _bwd,
rfx_localstate_mfma_ok / _fwd / _bwd, rfx_localstate_gen_fwd / _bwd, rfx_mha_fwd / _bwd -- against tests/attention_ref.py, the fp64
restatement with the SAME operand rounding, at a bound derived from that reference's own noise floor (attention_ref.floors; what the bound
can and cannot see is tests/test_attention_ref_cpu.py).  Every output lies NaN-filled between NaN guards, the `stat` workspaces are
NaN-filled before the kernels that write them.  The case table (attention_ref.CASES) follows the dispatch, attention_ref.form mirrors
it.  tests/test_gpu_hdemucs.py::test_localstate_mfma_vs_exact and tests/test_gpu_dptnet.py::test_mha_vs_torch stay the module-level
tests (autograd wrappers, session modes); the loose assertions here use their bounds."""
import pytest
import torch

from tests import attention_ref as A
from tests.attention_ref import B, GEN, HEADS, LDS, MFMA, MHA
from tests.conftest import check
from tests.kernel_harness import Guarded, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]


def test_case_table_reaches_every_form():
    reached = {}
    for fam, ch, T, nd in A.CASES:
        for kern in A.kernels_of(fam, ch):
            reached.setdefault(kern, set()).add((fam, ch, T, nd))
    assert set(reached) == (
        {"localstate_fwd_kernel<32>", "localstate_bwd_kernel<16>",
         "localstate_gen_q_kernel<0>", "localstate_gen_q_kernel<1>", "localstate_gen_k_kernel"}
        | {f"ls_mfma_{p}_kernel<{ks}>" for p in ("fwd", "bwd_a", "bwd_b") for ks in (1, 2, 3, 4, 6)})
    assert any(c[0] == MHA for c in A.CASES)
    have = set(A.CASES)
    rows = ([(MFMA, ch, T, 4) for ch in (16, 48, 96) for T in (1, 2, 31, 32, 33, 127, 128, 129, 255, 256)]
            + [(MFMA, ch, T, 4) for ch in (32, 64) for T in (1, 129, 256)] + [(MFMA, 48, 129, 1), (MFMA, 48, 129, 8)]
            + [(LDS, ch, T, nd) for ch in (1, 3, 16) for T in (1, 2, 15, 16, 17, 31, 32, 33) for nd in (1, 3, 8)]
            + [(LDS, 48, T, nd) for T in (255, 256) for nd in (1, 3, 8)] + [(LDS, 96, 128, nd) for nd in (1, 3, 8)]
            + [(GEN, ch, T, nd) for ch in (1, 16, 104) for T in (1, 63, 64, 65, 257) for nd in (1, 9, 64)] + [(GEN, 104, 130, 64)]
            + [(MHA, ch, T, 0) for ch in (16, 24, 104) for T in (1, 64, 65, 130)])
    assert have == set(rows) and len(A.CASES) == len(rows)
    # the mirror of the dispatch sends every MFMA / LDS row to its family in the mode that uses it
    for fam, ch, T, nd in A.CASES:
        if fam == MFMA:
            assert A.form(ch, T, nd, "bf16")[0] == MFMA and A.form(ch, T, nd, "f32")[0] in (LDS, GEN)
        elif fam == LDS:
            assert A.form(ch, T, nd, "f32")[0] == LDS and A.form(ch, T, nd, "bf16x3")[0] == LDS
    assert A.form(104, 130, 4, "f32")[0] == GEN and A.form(96, 256, 4, "f32")[0] == GEN and A.form(16, 33, 9, "bf16")[0] == GEN
    # every regime at an edge shape of every family
    for fam in (MFMA, LDS, GEN, MHA):
        assert {r for c, r in A.REGIME_RUNS if c[0] == fam} >= ({"b", "e"} if fam == MHA else {"b", "c", "d", "e"})
    assert all(c in have for c in A.REGIME_CASES)


def launch(fam, ch, T, nd, inputs, batch=B, heads=HEADS, save_w=True):
    """forward and backward of one family on the current stream through the C ABI; returns CPU tensors"""
    from remfx_amd import _lib
    from remfx_amd._lib import check as rc
    from remfx_amd.ops import _ptr, _stream
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    q, k, cont, qd, gout = (t.to(dev).contiguous() if t is not None else None for t in inputs)
    n, nq, nbt = batch * heads * ch * T, batch * heads * nd * T, batch * heads * T
    bufs = {name: Guarded(n, what=name, device=dev) for name in ("out", "dq", "dk", "dcont")}
    if nd:
        bufs["dqd"] = Guarded(nq, what="dqd", device=dev)
    p = {name: _ptr(b.t) for name, b in bufs.items()}
    res = {}
    if fam == LDS:
        wb = Guarded(nbt * T, what="w", device=dev) if save_w else None
        w = wb.t if save_w else None
        rc(L.rfx_localstate_fwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), batch, heads, ch, T, nd, _ptr(w), p["out"], _stream()),
           "rfx_localstate_fwd")
        bufs["out"].owned()
        if not save_w:
            return {"out": bufs["out"].t.cpu().view(batch, heads * ch, T)}
        wb.owned()
        rc(L.rfx_localstate_bwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), _ptr(w), _ptr(gout), batch, heads, ch, T, nd, p["dq"], p["dk"],
                                p["dcont"], p["dqd"], _stream()), "rfx_localstate_bwd")
        res["w"] = w.cpu().view(batch, heads, T, T)
    elif fam == MFMA:
        assert L.rfx_localstate_mfma_ok(batch, heads, ch, T, nd) == 1
        sb = Guarded(nbt * 4, what="stat", device=dev)
        stat = sb.t
        assert stat.data_ptr() % 16 == 0
        rc(L.rfx_localstate_mfma_fwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), batch, heads, ch, T, nd, p["out"], _stream()),
           "rfx_localstate_mfma_fwd")
        bufs["out"].owned()
        rc(L.rfx_localstate_mfma_bwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), _ptr(gout), batch, heads, ch, T, nd, p["dq"], p["dk"],
                                     p["dcont"], p["dqd"], _ptr(stat), _stream()), "rfx_localstate_mfma_bwd")
        sb.owned()                                             # (max, 1 / sum, delta, D) of every query column
    else:
        sb = Guarded(nbt * 4, what="stat", device=dev)
        stat = sb.t
        if fam == GEN:
            rc(L.rfx_localstate_gen_fwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), batch, heads, ch, T, nd, _ptr(stat), p["out"], _stream()),
               "rfx_localstate_gen_fwd")
        else:
            rc(L.rfx_mha_fwd(_ptr(q), _ptr(k), _ptr(cont), batch, heads, ch, T, _ptr(stat), p["out"], _stream()), "rfx_mha_fwd")
        bufs["out"].owned()
        sb.guards_intact()
        res["stat_fwd"] = stat.cpu().view(nbt, 4)
        out = bufs["out"].t
        if fam == GEN:
            rc(L.rfx_localstate_gen_bwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(qd), _ptr(stat), _ptr(out), _ptr(gout), batch, heads, ch, T, nd,
                                        p["dq"], p["dk"], p["dcont"], p["dqd"], _stream()), "rfx_localstate_gen_bwd")
        else:
            rc(L.rfx_mha_bwd(_ptr(q), _ptr(k), _ptr(cont), _ptr(stat), _ptr(out), _ptr(gout), batch, heads, ch, T, p["dq"], p["dk"],
                             p["dcont"], _stream()), "rfx_mha_bwd")
        sb.guards_intact()
        res["stat"] = stat.cpu().view(nbt, 4)
    for name, b in bufs.items():
        b.owned()
        res[name] = b.t.cpu().view(batch, -1, T)
    return res


_GOT = {}


def _case(fam, ch, T, nd, regime="a"):
    key = (fam, ch, T, nd, regime)
    if key not in _GOT:
        inp, ref, fl, elem = A.reference_case(fam, ch, T, nd, regime)
        _GOT[key] = launch(fam, ch, T, nd, inp)
    return A.reference_case(fam, ch, T, nd, regime) + (_GOT[key],)


def tight(fam, ch, got, ref, fl, elem, what=""):
    """per tensor L2 and max-abs, and every element, against the reference with the family's rule set: all ratios to the bound < 1"""
    kern = A.kernels_of(fam, ch)
    for name, ratios in A.compare(got, ref, fl, elem).items():
        form = kern[0] if name in ("out", "w") else "+".join(kern[1:])
        for kind, r in zip(("l2", "max", "element"), ratios):
            check(r, 1.0, what=f"tight|{fam}|{form}|{name}|{kind}{what}")


def loose(case, regime, inp, got):
    """the module-level tests' whole-tensor RMS bounds against the unrounded operator, wherever the reference itself is inside them"""
    fam, ch, T, nd = case
    q, k, cont, qd, gout = inp
    exact = A.run(q, k, cont, qd, gout, HEADS, nd, "exact", diag=fam != MHA)
    for name in A.loose_names(case, regime, exact):
        A.loose_check(name, got[name], exact, A.LOOSE[A.RULES_OF[fam]], nd)


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_forward_backward(case):
    fam, ch, T, nd = case
    inp, ref, fl, elem, got = _case(*case)
    q, k, cont, qd, gout = inp
    tight(fam, ch, got, ref, fl, elem)
    loose(case, "a", inp, got)
    if T == 1:
        # a single key: the weight is exactly 1 (LocalState: the masked diagonal alone)
        rnd = (lambda t: A.bf16_rne(t.double()).float()) if fam == MFMA else (lambda t: t)
        assert torch.equal(got["out"], rnd(cont)) and torch.equal(got["dcont"], rnd(gout))
        for name in ("dq", "dk", "dqd"):
            if name in got:
                assert bool((got[name] == 0).all()), name
    if fam == LDS:
        # each column of the saved weights sums to 1 within the floor; w = NULL (inference) writes the same out
        assert float((got["w"].double().sum(2) - 1).abs().max()) <= T * A.bound(fl["w"][1])      # T elements, each inside its bound
        assert torch.equal(launch(fam, ch, T, nd, inp, save_w=False)["out"], got["out"])
    if fam in (GEN, MHA):
        st, sf = got["stat"], got["stat_fwd"]
        assert torch.equal(st[:, :2], sf[:, :2]) and bool(torch.isfinite(st[:, :3]).all())      # max, sum survive the backward
        delta = (got["out"].double() * gout.double()).view(B * HEADS, ch, T).sum(1).reshape(-1)
        mag = (got["out"].double() * gout.double()).abs().view(B * HEADS, ch, T).sum(1).reshape(-1)
        assert bool(((st[:, 2].double() - delta).abs() <= 4 * 2.0 ** -24 * max(1.0, ch ** 0.5) * mag + A.TINY).all())   # stat[2] = <out, gout>


@pytest.mark.parametrize("case,regime", A.REGIME_RUNS, ids=lambda v: v if isinstance(v, str) else A.case_id(v))
def test_regime(case, regime):
    fam, ch, T, nd = case
    inp, ref, fl, elem, got = _case(*case, regime)
    tight(fam, ch, got, ref, fl, elem, what=f"|regime {regime}")
    loose(case, regime, inp, got)


EDGE = [(MFMA, 16, 33, 4), (MFMA, 48, 129, 4), (MFMA, 96, 256, 4), (MFMA, 64, 129, 4), (LDS, 3, 17, 3), (LDS, 16, 33, 8), (LDS, 48, 255, 3),
        (GEN, 16, 65, 9), (GEN, 104, 130, 64), (MHA, 24, 65, 0), (MHA, 104, 130, 0)]


@pytest.mark.parametrize("case", EDGE, ids=A.case_id)
def test_rows_are_independent(case):
    """(b, h) of the B = 2, heads = 2 call = the B = 1, heads = 1 call on that slice, bit for bit"""
    fam, ch, T, nd = case
    inp, _, _, _, got = _case(*case)
    for b in range(B):
        for h in range(HEADS):
            sl = [t[b:b + 1, h * c:(h + 1) * c].contiguous() if t is not None else None for t, c in zip(inp, (ch, ch, ch, nd, ch))]
            one = launch(fam, ch, T, nd, sl, batch=1, heads=1)
            for name in A.OUTPUTS:
                if name in got:
                    c = nd if name == "dqd" else ch
                    assert torch.equal(one[name], got[name][b:b + 1, h * c:(h + 1) * c]), (name, b, h)


@pytest.mark.parametrize("case", EDGE, ids=A.case_id)
def test_repeat_after_interference(case):
    """the case again after another shape has churned the allocator (freed NaN-filled blocks get reused): the same bits"""
    fam, ch, T, nd = case
    inp, _, _, _, got = _case(*case)
    T2 = T % 7 + 40
    launch(fam, ch, T2, nd, A.make_inputs(ch, T2, nd, seed=1))
    torch.cuda.empty_cache()
    again = launch(fam, ch, T, nd, inp)
    for name in got:
        a, g = (again[name], got[name]) if not name.startswith("stat") else (again[name][:, :3], got[name][:, :3])    # stat[3] is unused
        assert torch.equal(a, g) or (name == "stat_fwd" and torch.equal(a[:, :2], g[:, :2])), name


@pytest.mark.parametrize("ch,T,nd", [(1, 1, 1), (3, 17, 3), (16, 33, 8), (48, 255, 3), (48, 256, 8), (96, 128, 1)])
def test_lds_and_streaming_kernels_agree(ch, T, nd):
    """where both exact forms accept a shape, both meet the tight bound against the same reference"""
    inp, ref, fl, elem, got = _case(LDS, ch, T, nd)
    tight(LDS, ch, got, ref, fl, elem)
    tight(GEN, ch, launch(GEN, ch, T, nd, inp), ref, fl, elem, what="|lds shape")


@pytest.mark.parametrize("case", EDGE, ids=A.case_id)
def test_time_reversal(case):
    """|t - s| is symmetric: all inputs reversed along t give all outputs reversed, within the tight bound of the unreversed reference"""
    fam, ch, T, nd = case
    inp, ref, fl, elem, _ = _case(*case)
    got = launch(fam, ch, T, nd, [t.flip(-1) if t is not None else None for t in inp])
    tight(fam, ch, {n: got[n].flip(-1) for n in A.OUTPUTS if n in got}, ref, fl, elem, what="|reversed")


def test_rejections_launch_nothing():
    """argument validation only: -1 and every NaN-filled output untouched"""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())

    def call(fam, ch, T, nd, sweep):
        n, nq, nbt = B * HEADS * ch * T, B * HEADS * max(nd, 1) * T, B * HEADS * T
        # q, k, cont, gout, out / w (inputs of the backward sweeps), each large enough for any form the entry point could launch
        x = [torch.zeros(max(B * HEADS * max(ch, 96) * T, nbt * T), device=dev) for _ in range(5)]
        qd = torch.zeros(nq, device=dev)
        o = {name: Guarded(m, what=(fam, ch, T, nd, sweep, name), device=dev) for name, m in
             (("out", n), ("dq", n), ("dk", n), ("dcont", n), ("dqd", nq), ("w", nbt * T), ("stat", nbt * 4))}
        P = {name: _ptr(b.t) for name, b in o.items()}
        q, k, c, g, oin = (_ptr(t) for t in x)
        s = _stream()
        if (fam, sweep) == (LDS, "fwd"):
            r = L.rfx_localstate_fwd(q, k, c, _ptr(qd), B, HEADS, ch, T, nd, P["w"], P["out"], s)
        elif (fam, sweep) == (LDS, "bwd"):
            r = L.rfx_localstate_bwd(q, k, c, _ptr(qd), oin, g, B, HEADS, ch, T, nd, P["dq"], P["dk"], P["dcont"], P["dqd"], s)
        elif (fam, sweep) == (MFMA, "fwd"):
            r = L.rfx_localstate_mfma_fwd(q, k, c, _ptr(qd), B, HEADS, ch, T, nd, P["out"], s)
        elif (fam, sweep) == (MFMA, "bwd"):
            r = L.rfx_localstate_mfma_bwd(q, k, c, _ptr(qd), g, B, HEADS, ch, T, nd, P["dq"], P["dk"], P["dcont"], P["dqd"], P["stat"], s)
        elif (fam, sweep) == (GEN, "fwd"):
            r = L.rfx_localstate_gen_fwd(q, k, c, _ptr(qd), B, HEADS, ch, T, nd, P["stat"], P["out"], s)
        elif (fam, sweep) == (GEN, "bwd"):
            r = L.rfx_localstate_gen_bwd(q, k, c, _ptr(qd), P["stat"], oin, g, B, HEADS, ch, T, nd, P["dq"], P["dk"], P["dcont"], P["dqd"], s)
        elif (fam, sweep) == (MHA, "fwd"):
            r = L.rfx_mha_fwd(q, k, c, B, HEADS, ch, T, P["stat"], P["out"], s)
        else:
            r = L.rfx_mha_bwd(q, k, c, P["stat"], oin, g, B, HEADS, ch, T, P["dq"], P["dk"], P["dcont"], s)
        assert r == -1, (fam, ch, T, nd, sweep, r)
        torch.cuda.synchronize()
        for b in o.values():
            b.untouched()                                      # a rejected call writes nothing

    for sweep in ("fwd", "bwd"):
        for ch, T, nd in ((16, 257, 4), (16, 33, 9), (12289, 1, 4), (97, 127, 4), (48, 257, 4)):
            call(LDS, ch, T, nd, sweep)
        for ch, T, nd in ((8, 33, 4), (80, 33, 4), (112, 33, 4), (48, 33, 9), (48, 257, 4)):
            call(MFMA, ch, T, nd, sweep)
        for ch, T, nd in ((105, 65, 4), (16, 65, 65), (16, 65, 0)):
            call(GEN, ch, T, nd, sweep)
        call(MHA, 105, 65, 0, sweep)
    for ch in (8, 80, 112):
        assert L.rfx_localstate_mfma_ok(B, HEADS, ch, 33, 4) == 0
    assert L.rfx_localstate_mfma_ok(B, HEADS, 48, 33, 9) == 0 and L.rfx_localstate_mfma_ok(B, HEADS, 48, 257, 4) == 0
    for ch in (16, 32, 48, 64, 96):
        for T in (1, 2, 31, 32, 33, 127, 128, 129, 255, 256):
            for nd in (1, 4, 8):
                assert L.rfx_localstate_mfma_ok(B, HEADS, ch, T, nd) == 1, (ch, T, nd)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_dispatch_of_the_autograd_wrapper(mode):
    """nnops.local_state_attention picks the form attention_ref.form predicts (ctx.cfg of the graph node), in every session mode; a head
    width beyond the streaming kernels is a ValueError before anything is launched"""
    from remfx_amd import nnops, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    prev = ops.gemm_precision()
    ops.set_gemm_precision(mode)
    try:
        for ch, T, nd in ((48, 129, 4), (24, 33, 3), (96, 128, 8), (96, 256, 4), (104, 130, 4), (16, 33, 9), (16, 300, 4), (80, 33, 4)):
            q, k, cont, qd, gout = (t.to(dev).requires_grad_(True) for t in A.make_inputs(ch, T, nd))
            y = nnops.local_state_attention(q, k, cont, qd, HEADS, nd)
            fam = A.form(ch, T, nd, mode)[0]
            assert y.grad_fn.cfg == (B, HEADS, ch, T, nd, fam == MFMA, fam == GEN), (ch, T, nd, y.grad_fn.cfg, fam)
            y.backward(gout.detach())
            ref = A.run(*(t.detach().cpu() for t in (q, k, cont, qd, gout)), HEADS, nd, "exact")
            for name, a in zip(A.OUTPUTS, (y.detach(), q.grad, k.grad, cont.grad, qd.grad)):
                rms = float(ref[name].pow(2).mean().sqrt())
                assert float((a.double().cpu() - ref[name]).pow(2).mean().sqrt()) <= A.LOOSE["bf16" if fam == MFMA else "exact"] * rms + 1e-9
        q, k, cont, qd, _ = (t.to(dev).requires_grad_(True) for t in A.make_inputs(105, 257, 4))
        with pytest.raises(ValueError):
            nnops.local_state_attention(q, k, cont, qd, HEADS, 4)
    finally:
        ops.set_gemm_precision(prev)
