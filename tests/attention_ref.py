"""Plain torch, fp64, CPU restatement of the attention operator of remfx_amd/csrc/attention.hip and attention_mfma.hip in the kernels'
interface: channel-major q, k, content, gout (B, heads*ch, T), decay projections qd (B, heads*nd, T).

  dots[t, s] = <k[:, t], q[:, s]> / sqrt(ch) - |t - s| * D[s],   D[s] = sum_f (f + 1) sigmoid(qd[f, s]) / (2 sqrt(nd))
  dots[s, s] = -100 (diag = True),  P = softmax over t,  out[c, s] = sum_t P[t, s] content[c, t]
Plain multi-head attention is the same function with diag = False, nd = 0 (attention.hip:484-505: rfx_mha_* set diag = 0, nd = 0).
Forward and an explicit backward (formulas, not autograd: rounding has no useful gradient and the kernels recompute P).

Rule sets:
  exact   attention.hip -- no operand rounding.  The diagonal is the constant -100 (ls_scores :47, lsg_score :310) and carries no score
          gradient (:205, :367, :433).
  bf16    attention_mfma.hip -- q, k, content, gout are rounded to bf16 (RNE, lm_pk :32-35) wherever they enter an MFMA: lm_ldfrag
          :40-47 for fragments from global memory, lm_fill_nat :57-65 for the LDS tiles.  D, the scores, max, exp, sum, 1 / sum are
          fp32 (here fp64).  P is normalised first (:113-116) and rounded to bf16 afterwards, where it is packed as the B operand of
          content . P (:153-156) and of gout . P^T (:339); dS likewise (:258, :339).
          * delta = sum_t P dP uses the UNROUNDED P: :222 reads acc[R][r], the fp32 normalised weights, before any packing.
          * the decay gradient sum_t dS |t - s| uses the UNROUNDED dS: :253-256 accumulate `ds` itself, pv[e] is packed after.
          * dS = P (dP - delta) is formed from the unrounded P as well (:253, :335), then rounded.

`perturb`: every intermediate (each accumulation, score, exp, sum, reciprocal, P, dS, the outputs) carries an independent relative
error of that size -- see floors().  `fault`: one of FAULTS, a deliberately wrong operator."""
import functools
import math

import torch

from tests.ref_common import bf16_rne, ulp

RULES = ("exact", "bf16")
# name -> rule sets it applies to
FAULTS = {
    "diag_unmasked": RULES,                 # the diagonal keeps its score
    # the -100 diagonal gets a score gradient in the backward.  Visible only where the diagonal competes with its neighbours: D ~ 100,
    # which needs nd = 64 (regime f) -- beyond rfx_localstate_mfma_ok's nd <= 8, so no bf16 case can show it
    "diag_variable_bwd": ("exact",),
    "decay_f_not_f1": RULES,                # decay weight f where f + 1 belongs
    "no_inv_sqrt_nd": RULES,                # 1 / sqrt(nd) missing
    "last_key_omitted": RULES,              # key row T - 1 left out of the softmax
    "padded_key_included": RULES,           # one padded key row (score 0, content 0) leaks exp(0 - m) into the sum
    "dist_wrap_128": RULES,                 # |t - s| wrapped at 128 (a workgroup's columns)
    "next_head_decay": RULES,               # decay projection of head h + 1
    "p_rounded_before_norm": ("bf16",),     # P rounded to bf16 before the multiplication by 1 / sum (the kernel rounds after)
    "softmax_over_s": RULES,                # softmax over the query axis
}
OUTPUTS = ("out", "dq", "dk", "dcont", "dqd")


class _Noise:
    def __init__(self, perturb, seed, before_rounding_only=False):
        self.p, self.pre_only = perturb, before_rounding_only
        self.gen = torch.Generator().manual_seed(seed)

    def _r(self, x):
        return torch.randn(x.shape, generator=self.gen, dtype=torch.float64).to(x.dtype)

    def rel(self, x, scale=1.0, post=False):
        """one rounding: x (1 + perturb * scale * N(0, 1)); post: it happens after the bf16 rounding of P / dS"""
        if not self.p or (post and self.pre_only):
            return x
        return x * (1 + self.p * scale * self._r(x))

    def acc(self, eq, a, b, n, post=False):
        """einsum with the error of a sequential fp32 accumulation of n terms: every add rounds the partial sum, a random walk of the
        terms, so the error is ~ eps sqrt(n / 2) sqrt(sum term^2); FLOOR_PERTURB is 3 x the std of one fp32 rounding, hence the 1/4"""
        r = torch.einsum(eq, a, b)
        if not self.p or (post and self.pre_only):
            return r
        return r + self.p * max(1.0, 0.25 * n ** 0.5) * torch.einsum(eq, a * a, b * b).sqrt() * self._r(r)

    def operand(self, x):
        """the value that is about to be rounded to bf16"""
        if not self.p:
            return x
        return x * (1 + self.p * self._r(x))


def run(q, k, cont, qd, gout, heads, nd, rules="exact", diag=True, perturb=0.0, seed=0, fault=None, dtype=torch.float64,
        before_rounding_only=False, sequential=False, delta_from_out=False):
    """sequential: the score product is summed channel by channel in `dtype`, as the VALU kernels do (a second honest fp32 copy).
    delta_from_out: delta = <out, gout> from the stored out, the streaming kernels' form (attention.hip:337), where the others sum P dP.
    -> {out, dq, dk, dcont, dqd (nd > 0), w = the unrounded P (B, heads, T, T) [t][s], P_r / dS_r = what enters the second products}"""
    assert rules in RULES and fault in (None,) + tuple(FAULTS)
    B, Ctot, T = q.shape
    ch = Ctot // heads
    N = _Noise(perturb, seed, before_rounding_only)
    rnd = bf16_rne if rules == "bf16" else (lambda x: x)
    q4, k4, c4, g4 = (rnd(t.to(dtype)).view(B, heads, ch, T) if t is not None else None for t in (q, k, cont, gout))
    inv = ch ** -0.5
    idx = torch.arange(T, dtype=dtype)
    dist = (idx[:, None] - idx[None, :]).abs()
    if fault == "dist_wrap_128":
        dist = dist % 128
    eye = torch.eye(T, dtype=torch.bool)
    sd = 3 if fault == "softmax_over_s" else 2
    if sequential:
        S = torch.zeros(B, heads, T, T, dtype=dtype)
        for c in range(ch):
            S = S + k4[:, :, c, :, None] * q4[:, :, c, None, :]
    else:
        S = N.acc("bhct,bhcs->bhts", k4, q4, ch)
    if nd:
        sig = N.rel(torch.sigmoid(qd.to(dtype).view(B, heads, nd, T)), 2.0)               # exp and reciprocal; 1 - sig below cancels
        if fault == "next_head_decay":
            sig = sig.roll(-1, dims=1)
        fw = torch.arange(0 if fault == "decay_f_not_f1" else 1, nd + (0 if fault == "decay_f_not_f1" else 1), dtype=dtype).view(1, 1, nd, 1)
        invd = 1.0 if fault == "no_inv_sqrt_nd" else nd ** -0.5
        D = N.rel((fw * sig).sum(2) * (0.5 * invd))                                       # (B, heads, T) per query column s
        v = N.rel(N.rel(S * inv) - N.rel(dist * D[:, :, None, :]))
    else:
        sig, D = None, None
        v = N.rel(S * inv)
    if diag and fault != "diag_unmasked":
        v = v.masked_fill(eye, -100.0)
    if fault == "last_key_omitted" and T > 1:
        v = v.clone()
        v[:, :, T - 1, :] = -float("inf")
    m = v.amax(sd, keepdim=True)
    arg = v - m
    e = N.rel(torch.exp(arg), 1 + arg.abs().clamp(max=1e4))                               # __expf: the error grows with |argument|
    tot = N.rel(e.sum(sd, keepdim=True), max(1.0, 0.25 * T ** 0.5))
    if fault == "padded_key_included":
        tot = tot + torch.exp(-m)
    rinv = N.rel(1.0 / tot)
    if fault == "p_rounded_before_norm":
        P = e * rinv
        Pr = bf16_rne(N.operand(e)) * rinv
    else:
        P = N.rel(e * rinv)                                                               # attention_mfma.hip:116, normalised in fp32
        Pr = rnd(N.operand(P)) if rules == "bf16" else P                                  # :156 packed afterwards
    res = {"w": P, "P_r": Pr}
    res["out"] = N.rel(N.acc("bhts,bhct->bhcs", Pr, c4, T, post=True), post=True).reshape(B, Ctot, T)
    if gout is None:
        return res
    # backward: P is recomputed by the kernels with the same arithmetic (pass B: from the saved max, 1 / sum, delta, D)
    dP = N.acc("bhct,bhcs->bhts", c4, g4, ch)
    delta = N.rel((P * dP).sum(sd, keepdim=True), max(1.0, 0.25 * T ** 0.5))              # unrounded P (attention_mfma.hip:222)
    if delta_from_out:
        delta = (res["out"].view(B, heads, ch, T) * g4).sum(2)[:, :, None, :]
    dS = N.rel(P * N.rel(dP - delta))                                                     # unrounded P (:253, :335)
    if diag and fault != "diag_variable_bwd":
        dS = dS.masked_fill(eye, 0.0)                                                     # the masked diagonal is a constant
    dSr = rnd(N.operand(dS)) if rules == "bf16" else dS                                   # :258, :339
    res["dS_r"] = dSr
    res["dq"] = N.rel(N.acc("bhts,bhct->bhcs", dSr, k4, T, post=True) * inv, post=True).reshape(B, Ctot, T)
    res["dk"] = N.rel(N.acc("bhts,bhcs->bhct", dSr, q4, T, post=True) * inv, post=True).reshape(B, Ctot, T)
    res["dcont"] = N.rel(N.acc("bhts,bhcs->bhct", Pr, g4, T, post=True), post=True).reshape(B, Ctot, T)
    if nd:
        dsum = N.rel((dS * dist).sum(2), max(1.0, 0.25 * T ** 0.5))                       # unrounded dS (:253-256)
        res["dqd"] = N.rel(-fw * (invd * 0.5) * sig * (1 - sig) * dsum[:, :, None, :]).reshape(B, heads * nd, T)
        # the same sum without its cancellation (two neighbours at one distance carry opposite dS): the size its rounding scales with
        res["dqd_terms"] = (fw * (invd * 0.5) * sig * (1 - sig) * (dS.abs() * dist).sum(2)[:, :, None, :]).reshape(B, heads * nd, T)
    return res


# ---- the comparison the tests share ---------------------------------------------------------------------------------------------
# Two measures, both against the reference with the kernel's rule set:
#  * per tensor, L2 and max-abs of the difference at MARGIN x floor (+ TINY), floor = the reference
#    against itself with every intermediate perturbed (FLOOR_PERTURB, the larger of DRAWS draws).  bf16 rules: the rounding of P and dS swallows
#    a 1e-7 perturbation unless the value sits on a rounding boundary, then the operand moves by a whole bf16 ulp (a flip); the flip part
#    of the floor is lstm_ref.floors' construction -- a draw in which flips are common (FLIP_PERTURB on everything that happens BEFORE
#    the rounding of P / dS, nothing after it; nf operands round differently), its L2 scaled by sqrt(max(FLOOR_PERTURB / FLIP_PERTURB, 1 / nf)), its max-abs unscaled.
#  * per element, 100 % of them: |kernel - ref| <= MARGIN x floor[element], floor[element] = the tensor's max-abs floor without flips
#    (absolute) + FLIPS / MARGIN x the largest single flip that can reach this element: a flip of P[t, s] moves out[:, s] by
#    ulp(P[t, s]) content[c, t] and nothing else, so the element's allowance is max_t ulp_bf16(P[t, s]) |content[c, t]| (dcont: over s
#    with gout; dq / dk: dS with k / q, / sqrt(ch)).  An implementation has a given flip or has it not, so flips are not multiplied by
#    the margin; FLIPS = 2 of the largest possible in one column.  A wrong column moves an element by ~P content, 2^8 flips.
# All of it is ABSOLUTE (lstm_ref normalises by the reference's norm): several of these tensors are zero or pure cancellation -- with
# T <= 2 a column has one live key, its softmax is the constant 1 and dq, dk, dqd vanish identically; with a dominant decay the two
# neighbours t = s +- 1 carry all the weight at the same distance, so sum_t dS |t - s| = 0 -- and an error relative to them says nothing.
# Under the exact rules there are no flips and floor[element] is the tensor's max-abs floor: the element check IS the max-abs check there.
# FP32_TERM appears in loose_check only.
DRAWS = 2
FLIPS = 2.0
FP32_TERM = 16 * 2.0 ** -24
_FLIP_SOURCE = {"out": "P_r", "dcont": "P_r", "dq": "dS_r", "dk": "dS_r"}


def errors(a, b):
    """(L2, max-abs) of a - b"""
    d = a.double() - b.double()
    return float(d.norm()), float(d.abs().max())


def sizes(ref):
    return float(ref.double().norm()), float(ref.double().abs().max())


FLOOR_PERTURB, FLIP_PERTURB, MARGIN = 1e-7, 1e-4, 8.0        # lstm_ref.floors' construction, restated: its values and their meaning
TINY = 2.0 ** -126                          # smallest normal fp32: sigmoid(-100) is 0 in fp32 and 4e-44 in fp64 (regime e, dqd)


def bound(floor):
    return MARGIN * floor + TINY


def _ulp_bf16(x):
    a = x.abs().double()
    return torch.where(a > 0, ulp(a, 7, 1e-300), torch.zeros_like(a))


def _flip_allowance(ref, q, k, cont, gout, heads, rules_round):
    """{name: (B, heads*ch, T)} largest single bf16 flip of P / dS that reaches each element"""
    B, Ctot, T = q.shape
    ch = Ctot // heads
    q4, k4, c4, g4 = (rules_round(t.double()).view(B, heads, ch, T).abs() for t in (q, k, cont, gout))
    uP, uS = _ulp_bf16(ref["P_r"]), _ulp_bf16(ref["dS_r"])
    al = {n: torch.zeros(B, heads, ch, T, dtype=torch.float64) for n in _FLIP_SOURCE}
    inv = ch ** -0.5
    for b in range(B):
        for h in range(heads):
            # [c][t][s]
            al["out"][b, h] = (uP[b, h][None] * c4[b, h][:, :, None]).amax(1)
            al["dq"][b, h] = (uS[b, h][None] * k4[b, h][:, :, None]).amax(1) * inv
            al["dcont"][b, h] = (uP[b, h][None] * g4[b, h][:, None, :]).amax(2)
            al["dk"][b, h] = (uS[b, h][None] * q4[b, h][:, None, :]).amax(2) * inv
    return {n: a.reshape(B, Ctot, T) for n, a in al.items()}


def floors(q, k, cont, qd, gout, heads, nd, rules, diag=True, fault=None, dtype=torch.float64):
    """-> (ref, fl, elem): ref = the reference's tensors; fl[name] = (floor_l2, floor_max) as errors() reports them; elem[name] = the
    per-element floor (same shape as the tensor; bound = MARGIN x elem + TINY)"""
    kw = dict(heads=heads, nd=nd, rules=rules, diag=diag, fault=fault, dtype=dtype)
    ref = run(q, k, cont, qd, gout, **kw)
    names = [n for n in OUTPUTS + ("w",) if n in ref]
    fl = {n: (0.0, 0.0) for n in names}
    for d in range(DRAWS):
        noisy = run(q, k, cont, qd, gout, perturb=FLOOR_PERTURB, seed=11 + d, **kw)
        for n in names:
            e = errors(noisy[n], ref[n])
            fl[n] = (max(fl[n][0], e[0]), max(fl[n][1], e[1]))
    elem = {n: torch.full(ref[n].shape, fl[n][1], dtype=torch.float64) for n in names}
    if rules == "bf16":
        # The operand with the error it actually carries: FLIP_PERTURB on everything before the rounding of P / dS, nothing after it.
        # (lstm_ref perturbs h alone; here dS = P (dP - delta) cancels, and what carries it across a rounding boundary is the error of dP
        # and delta, many times its own last rounding: with dS alone perturbed the fp32 copy of the reference is 1.15 x over the L2 bound of
        # dq at ch = 96, T = 255.)
        noisy = run(q, k, cont, qd, gout, perturb=FLIP_PERTURB, seed=5, before_rounding_only=True, **kw)
        for n, src in _FLIP_SOURCE.items():
            nf = int((noisy[src] != ref[src]).sum())
            if nf == 0:
                continue
            s = max(FLOOR_PERTURB / FLIP_PERTURB, 1.0 / nf) ** 0.5
            e = errors(noisy[n], ref[n])
            fl[n] = (max(fl[n][0], s * e[0]), max(fl[n][1], e[1]))
        for n, a in _flip_allowance(ref, q, k, cont, gout, heads, bf16_rne).items():
            elem[n] = elem[n] + (FLIPS / MARGIN) * a
    return ref, fl, elem


def compare(got, ref, fl, elem, names=None):
    """{name: (l2 / bound, max / bound, largest element error / element bound)} -- every ratio has to be <= 1"""
    r = {}
    for n in names or [n for n in fl if n in got]:
        g, x = got[n].double(), ref[n].double()
        e = errors(g, x)
        d = (g - x).abs()
        if float(d.max()) == 0.0:
            r[n] = (0.0, 0.0, 0.0)
            continue
        r[n] = (e[0] / bound(fl[n][0]), e[1] / bound(fl[n][1]), float((d / (MARGIN * elem[n] + TINY)).max()))
    return r


def loose_check(name, got, exact, rel, nd=0):
    """RMS of got - exact <= rel x RMS of exact + 1e-9, the assertion of test_localstate_mfma_vs_exact / test_mha_vs_torch.  At nd = 64
    dqd gets FP32_TERM (16 fp32 half-ulps) x the RMS of its uncancelled terms on top: with so steep a decay the two neighbours t = s +- 1 carry all the weight
    at ONE distance and opposite dS, dqd is 1e-12 of its terms, and no fp32 sum is accurate relative to that -- the fp32 copy of the
    reference misses the literal bound there (tests/test_attention_ref_cpu.py::test_fp32_copy_of_the_reference_meets_the_bound)."""
    rms = lambda x: float(x.double().pow(2).mean().sqrt())                                  # noqa: E731
    extra = FP32_TERM * rms(exact["dqd_terms"]) if name == "dqd" and nd == 64 else 0.0
    err = rms(got.double().cpu() - exact[name])
    assert err <= rel * rms(exact[name]) + 1e-9 + extra, (name, err, rms(exact[name]), extra)


# ---- the operator through autograd (what the exact rules are checked against) ---------------------------------------------------
def localstate_autograd(q, k, cont, qd, gy, heads, nd):
    """fp64 autograd over the operator written out in torch (torchaudio's _LocalState core) -> [out, dq, dk, dcont, dqd] on the CPU"""
    B, Ctot, T = q.shape
    ch = Ctot // heads
    qq, kk, cc, dd = (t.detach().double().cpu().requires_grad_(True) for t in (q, k, cont, qd))
    qh, kh, chh = (t.view(B, heads, ch, T) for t in (qq, kk, cc))
    dots = torch.einsum("bhct,bhcs->bhts", kh, qh) / ch ** 0.5
    idx = torch.arange(T, dtype=torch.float64)
    delta = (idx[:, None] - idx[None, :]).abs()
    dec = torch.sigmoid(dd.view(B, heads, nd, T)) / 2
    pen = -torch.arange(1, nd + 1, dtype=torch.float64).view(-1, 1, 1) * delta / nd ** 0.5
    dots = dots + torch.einsum("fts,bhfs->bhts", pen, dec)
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -100.0)
    w = torch.softmax(dots, dim=2)
    yr = torch.einsum("bhts,bhct->bhcs", w, chh).reshape(B, heads * ch, T)
    yr.backward(gy.double().cpu())
    return [yr.detach(), qq.grad, kk.grad, cc.grad, dd.grad]


# ---- the case table of tests/test_gpu_attention_kernel.py -----------------------------------------------------------------------
B, HEADS = 2, 2                               # batch and head offsets both matter, heads != nd
MFMA, LDS, GEN, MHA = "mfma", "lds", "gen", "mha"
# (family, ch, T, nd)
CASES = (
    [(MFMA, ch, T, 4) for ch in (16, 48, 96) for T in (1, 2, 31, 32, 33, 127, 128, 129, 255, 256)]   # CT = 1 (rows 16..31 zero), 2, 3
    + [(MFMA, ch, T, 4) for ch in (32, 64) for T in (1, 129, 256)]                                   # the remaining KS
    + [(MFMA, 48, 129, nd) for nd in (1, 8)]                                                         # decay-count edges
    + [(LDS, ch, T, nd) for ch in (1, 3, 16) for T in (1, 2, 15, 16, 17, 31, 32, 33) for nd in (1, 3, 8)]   # 16- and 32-column blocks
    + [(LDS, 48, T, nd) for T in (255, 256) for nd in (1, 3, 8)]                                     # ch * T = 12288, the limit
    + [(LDS, 96, 128, nd) for nd in (1, 3, 8)]                                                       # ... on the other axis
    + [(GEN, ch, T, nd) for ch in (1, 16, 104) for T in (1, 63, 64, 65, 257) for nd in (1, 9, 64)]   # 64 boundaries, LDS limit, nd > 9
    + [(GEN, 104, 130, 64)]                                                                          # largest LDS request
    + [(MHA, ch, T, 0) for ch in (16, 24, 104) for T in (1, 64, 65, 130)]                            # streaming kernels, diag = 0
)
RULES_OF = {MFMA: "bf16", LDS: "exact", GEN: "exact", MHA: "exact"}
REGIMES = ("a", "b", "c", "d", "e", "f")         # f: nd = 64 only
# the edge shapes every regime runs at: tile edges of each family, one block and several
REGIME_CASES = ([(MFMA, 48, T, 4) for T in (2, 33, 129, 256)] + [(MFMA, 16, 127, 4), (MFMA, 96, 255, 4), (MFMA, 48, 129, 8)]
                + [(LDS, 16, T, 8) for T in (2, 17, 33)] + [(LDS, 48, 255, 3)]
                + [(GEN, 16, T, nd) for T in (65, 257) for nd in (9, 64)] + [(GEN, 104, 63, 64)]
                + [(MHA, 24, T, 0) for T in (65, 130)])
REGIME_RUNS = [(c, r) for c in REGIME_CASES for r in REGIMES[1:]
               if not (c[0] == MHA and r in "cdf") and not (r == "f" and c[3] != 64)]


# Where the loose RMS bound (2e-2 of the unrounded operator) says nothing: the bf16 REFERENCE is itself outside it.  Peaked scores of +-30
# move by 0.1 when q and k are rounded, and the score gradients feel it first.  Every other tensor of every run carries the assertion;
# And one exact pair: dqd of the streaming form at ch = 104, nd = 64 with peaked scores -- an fp32 copy of the reference that takes
# delta = <out, gout> from the stored out, as those kernels do, is 1.4 x over it (dqd is the remainder of cancelling terms there).
# tests/test_attention_ref_cpu.py::test_loose_bound_is_attainable_everywhere_but_here keeps this list exact.
LOOSE_UNATTAINABLE = {((MFMA, 48, 33, 4), "b"): ("dq", "dk"), ((MFMA, 16, 127, 4), "b"): ("dq", "dk", "dqd"),
                      ((MFMA, 96, 255, 4), "b"): ("dqd",), ((MFMA, 48, 129, 8), "b"): ("dq", "dk"),
                      ((GEN, 104, 63, 64), "b"): ("dqd",)}
LOOSE = {"exact": 2e-5, "bf16": 2e-2}         # the module-level tests' RMS bounds


def loose_names(case, regime, tensors):
    return [n for n in OUTPUTS if n in tensors and n not in LOOSE_UNATTAINABLE.get((case, regime), ())]


def case_id(c):
    return "-".join(str(x) for x in c)


def form(ch, T, nd, mode):
    """the kernels nnops.local_state_attention launches in session mode `mode` (f32 / bf16x3 / bf16): the mirror of _LocalStateFn"""
    if mode == "bf16" and ch % 16 == 0 and 16 <= ch <= 96 and ch != 80 and 0 < T <= 256 and 0 < nd <= 8:
        ks = ch // 16
        return MFMA, tuple(f"ls_mfma_{p}_kernel<{ks}>" for p in ("fwd", "bwd_a", "bwd_b"))
    if T > 256 or ch * T > 12288 or nd > 8:
        return GEN, ("localstate_gen_q_kernel<0>", "localstate_gen_q_kernel<1>", "localstate_gen_k_kernel")
    return LDS, ("localstate_fwd_kernel<32>", "localstate_bwd_kernel<16>")


def kernels_of(family, ch):
    if family == MFMA:
        return form(ch, 1, 1, "bf16")[1]
    if family == LDS:
        return form(1, 1, 1, "f32")[1]
    return form(1, 257, 1, "f32")[1]


def make_inputs(ch, T, nd, regime="a", batch=B, heads=HEADS, seed=0):
    """fp32 (q, k, content, qd, gout).  a: randn * 0.8;  b: peaked -- q, k ~ N(0, 12), so the scores are ~ N(0, 12^2): +-30 at
    2.5 sigma;  c: qd = +6, the decay dominates;  d: qd = -20, decay off;  e: q = 0 and qd = -100 (sigmoid = 0 in fp32, 4e-44 in fp64:
    the penalty is exactly nothing), exactly uniform weights;  f (nd = 64): qd = log(10 / 3), D = 130 sigmoid = 100 -- the neighbours
    t = s +- 1 sit at the diagonal's -100 and the diagonal takes a third of the weight"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * ch + 131 * T + 17 * nd + ord(regime))
    mk = lambda c, s=0.8: torch.randn(batch, heads * c, T, generator=g) * s                # noqa: E731
    q, k, cont = mk(ch), mk(ch), mk(ch)
    qd = mk(max(nd, 1))
    gout = mk(ch, 1.0)
    if regime == "b":
        q, k = q * (12 ** 0.5 / 0.8), k * (12 ** 0.5 / 0.8)
    elif regime == "c":
        qd = torch.full_like(qd, 6.0)
    elif regime == "d":
        qd = torch.full_like(qd, -20.0)
    elif regime == "e":
        q, qd = torch.zeros_like(q), torch.full_like(qd, -100.0)
    elif regime == "f":
        assert nd == 64
        qd = torch.full_like(qd, math.log(10.0 / 3.0))
    return q, k, cont, (qd if nd else None), gout


@functools.lru_cache(maxsize=None)
def reference_case(family, ch, T, nd, regime="a"):
    """inputs, reference with the family's rule set, floors -- computed once, shared, not to be modified"""
    inp = make_inputs(ch, T, nd, regime)
    q, k, cont, qd, gout = inp
    ref, fl, elem = floors(q, k, cont, qd, gout, HEADS, nd, RULES_OF[family], diag=family != MHA)
    return inp, ref, fl, elem
