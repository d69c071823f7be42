"""Plain torch, fp64, CPU reference of the channel-major gather-GEMM family (remfx_amd/csrc/gemm*.hip, gemm*.h) per ELEMENT, the bound
each element is judged by, and the case table that names the instantiation every case is meant to reach.

Reference: torch.nn.functional.conv2d / conv_transpose2d (and torch.nn.grad.conv2d_weight for the weight gradient) in float64 on
operands rounded the way the kernels round them -- nothing of remfx_amd/convplan.py or tests/plan_emulator.py is used, so a planner
error shows as a wrong element:
  f32     operands as they are (v_mfma_f32_32x32x2_f32; the thin kernels' fmaf chains);
  bf16    both operands RNE to bf16 (round8 in gemm_tap.h, pack_a_bf3_kernel's hi half); values already stored in 16 bits are exact;
  bf16x3  hi = rne(v), lo = rne(v - hi) for both operands (split8 in gemm_tap.h, pack_a_bf3_kernel), and the result is the fp64 sum of
          the three convolutions hi.hi + hi.lo + lo.hi (k_step_tap issues exactly these three MFMAs); every product is exact in fp64.
The launchers run plans with fewer than 8 gathered channels, and thin plans (M <= 8 rows, not phase-merged), in exact fp32 whatever the
mode (ops.DevPlan.fwd_prec, rfx_gemm_wgrad): arith() states that rule here, independently of the planner.

Bound, per element:  |got - ref| <= K eps32 magnitude (+ half a bf16 ulp of the value for a 16-bit store) (+ sign-flip slack),
  magnitude  conv(|a|, |b|) + |bias| + |res|, pushed through an activation with the derivative weights tests/norm_ref.py uses (cdf =
             0.5 + 0.5 erf counts as those two terms, 1 - sigmoid as 1 and sigmoid);
  K          8 floor + 8; floor = the largest error, in units of eps32 magnitude, of the fp32 RESTATEMENT below against the fp64
             reference, per case class and output (FLOORS, measured by tests/test_gemm_ref_cpu.py on the CPU, never on a kernel);
  restatement  the products of one MFMA (16 along the reduction for the bf16 instructions, 2 for the fp32 one; 1 for the thin kernels'
             fmaf) summed exactly and rounded ONCE into the fp32 accumulator, K steps in the kernel's order (channel-major for the
             exact kernel, (tap, channel) for the tap-major ones, bf16x3: hi.hi, hi.lo, lo.hi per step); weight gradient: position
             blocks in order inside a split, the splits then added as unpack_add_kernel does (four groups of consecutive splits, each
             in order, then the four sums in order) or unpack_col_kernel (all in order).  The order INSIDE an MFMA is not documented;
             the + 8 is what covers it.  Channel blocking of the tap-major table and pruned taps only move block boundaries.
Staged outputs (judged from the kernel's OWN stored values, as DESIGN.md 4.16): the GLU product of the stored z, stat_sums of the stored y.

`mutate` (restate_*): a deliberately wrong kernel, what the bound has to reject (tests/test_gemm_ref_cpu.py)."""
import contextlib
import dataclasses

import torch
import torch.nn.functional as F

from tests.ref_common import EPS32, bf16_rne, bf16_trunc, gelu_cdf, gelu_pdf, ulp, worst  # noqa: F401

MARGIN = 8.0
EXTRA = 8.0                       # in units of eps32 magnitude: the undocumented order inside an MFMA, v_exp / v_rcp at 1 ulp, the erf polynomial
SIGN_SHARE = 1e-3                 # at most this share of a case's elements may carry sign-flip slack
ACTS = ("relu", "gelu", "tanh", "prelu", "leaky", "sigmoid")


# ---- number formats -------------------------------------------------------------------------------------------------------------------
def arith(mode, gathered_channels, rows, merged=False, wgrad=False):
    """arithmetic a launch runs in: exact fp32 below 8 gathered channels (no tap-major table) and on the thin path"""
    if wgrad:
        return "f32" if rows <= 8 else mode
    if gathered_channels < 8 or (rows <= 8 and not merged):
        return "f32"
    return mode


def parts(t, ar):
    """the bf16 / fp32 pieces (fp64 tensors) the kernels multiply for operand t"""
    t = t.to(torch.float32)
    if ar == "f32":
        return [t.double()]
    hi = bf16_rne(t)
    if ar == "bf16":
        return [hi.double()]
    return [hi.double(), bf16_rne(t - hi).double()]


def term_pairs(a, b, ar, drop=None):
    """[(a piece, b piece)]: the bilinear products whose fp64 sum the kernel computes, in MFMA order (hi.hi, hi.lo, lo.hi)"""
    pa, pb = parts(a, ar), parts(b, ar)
    if ar != "bf16x3":
        return [(pa[0], pb[0])]
    t = [(pa[0], pb[0]), (pa[0], pb[1]), (pa[1], pb[0])]
    if drop is not None:
        del t[drop]
    return t


# ---- the operations in fp64 -------------------------------------------------------------------------------------------------------------
def conv(x, w, stride, padding, dilation):
    return F.conv2d(x, w, None, stride, padding, dilation)


def convT(x, w, stride, dilation, lo, out_len):
    """conv_transpose2d (w: (gathered channels, rows, KA, KB)) cropped to [lo, lo + out_len) on each axis, zero beyond the full output"""
    full = F.conv_transpose2d(x, w, None, stride, 0, 0, 1, dilation)
    pa = max(0, lo[0] + out_len[0] - full.shape[2])
    pb = max(0, lo[1] + out_len[1] - full.shape[3])
    if pa or pb:
        full = F.pad(full, (0, pb, 0, pa))
    return full[:, :, lo[0]:lo[0] + out_len[0], lo[1]:lo[1] + out_len[1]]


def wgrad(x, g, wshape, stride, padding, dilation):
    return torch.nn.grad.conv2d_weight(x, wshape, g, stride, padding, dilation)


def bilinear(op, a, b, ar, drop=None):
    """(value, magnitude) of op over the term pairs"""
    val = mag = None
    for pa, pb in term_pairs(a, b, ar, drop):
        v, m = op(pa, pb), op(pa.abs(), pb.abs())
        val = v if val is None else val + v
        mag = m if mag is None else mag + m
    return val, mag


def act_fwd(u, A, act, slope=None):
    """(act(u), magnitude) -- A = magnitude of u"""
    if act is None:
        return u, A
    if act == "relu":
        return u.clamp_min(0), A
    if act in ("prelu", "leaky"):
        s = slope if act == "prelu" else torch.full_like(u[:1, :, :1, :1], 0.01)
        return torch.where(u >= 0, u, s * u), torch.where(u >= 0, A, s.abs() * A)
    if act == "gelu":
        cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
        return u * gelu_cdf(u), A * (2.0 * cdfm + u.abs() * gelu_pdf(u))
    if act == "tanh":
        t = torch.tanh(u)
        return t, t.abs() + (1.0 - t * t) * A
    if act == "sigmoid":
        s = torch.sigmoid(u)
        return s, s + s * (1.0 - s) * A
    raise ValueError(act)


def act_bwd(u, A, G, act, slope=None):
    """(G act'(u), magnitude, sign-flip slack or None)"""
    if act in ("relu", "prelu", "leaky"):
        s = slope if act == "prelu" else torch.full_like(u[:1, :, :1, :1], 0.0 if act == "relu" else 0.01)
        pos = (u > 0) if act == "relu" else (u >= 0)
        d = torch.where(pos, torch.ones_like(u), s.expand_as(u))
        return G * d, (G * d).abs(), (G.abs() * (1.0 - s).abs(), A)
    if act == "gelu":
        pdf = gelu_pdf(u)
        cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
        return G * (gelu_cdf(u) + u * pdf), G.abs() * (cdfm + u.abs() * pdf + pdf * (2.0 - u * u).abs() * A), None
    if act == "tanh":
        t = torch.tanh(u)
        return G * (1.0 - t * t), G.abs() * (1.0 + t * t + 2.0 * t.abs() * (1.0 - t * t) * A), None
    if act == "sigmoid":
        s = torch.sigmoid(u)
        return G * s * (1.0 - s), G.abs() * s * ((1.0 + s) + (1.0 - s) * (1.0 - 2.0 * s).abs() * A), None
    raise ValueError(act)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """kind: "conv" (forward family through conv_fwd_plan + gemm_fwd with the epilogue options), "dgrad" (ops.conv2d_dgrad), "convT"
    (transposed forward: merged or per-phase), "wgrad" (ops.gemm_wgrad + an unpack entry point).
    form: the instantiation(s) the case is meant to reach, literally, in launch order."""
    id: str
    kind: str
    mode: str
    form: tuple
    cin: int
    cout: int
    ishape: tuple
    ksize: tuple
    stride: tuple = (1, 1)
    padding: tuple = (0, 0)
    dilation: tuple = (1, 1)
    N: int = 2
    bias: bool = True
    act: str = None
    res: bool = False
    act2: str = None
    bwd: bool = False
    gslots: int = 0               # bwd + prelu: gparam [gslots][M] (1: [M])
    stat_slots: int = 0           # 0: no stat_sums, 1: (N, 2), > 1: (N, slots, 2)
    glu: bool = False
    out16: bool = False           # output (conv: y / z) stored as bf16
    in16: bool = False            # gathered operand stored as bf16 (conv) / gradient operand stored as bf16 (wgrad)
    two_phase: str = ""           # "", "in" (second phase gathers the same tensor), "in2" (another tensor)
    crop: tuple = ((0, 0), (0, 0))   # convT: (crop_lo, crop_hi)
    view: str = ""                # "perm": non-contiguous input view; "slice": output is a channel slice of a larger buffer; "perm+slice": both
    halo: bool = False            # lift convplan.HALO_MIN_POSITIONS for this case
    wsplits: int = None           # ops.WGRAD_SPLITS for this case
    unpack: str = "set"           # wgrad: "set" (+ unpack_col), "add", "add_bias"
    edges: tuple = ()
    seed: int = 0

    @property
    def out_hw(self):
        (IA, IB), (KA, KB) = self.ishape, self.ksize
        if self.kind == "convT":
            full = [(i - 1) * s + d * (k - 1) + 1 for i, k, s, d in zip(self.ishape, self.ksize, self.stride, self.dilation)]
            return tuple(f - lo - hi for f, lo, hi in zip(full, self.crop[0], self.crop[1]))
        return tuple((i + 2 * p - d * (k - 1) - 1) // s + 1
                     for i, k, s, p, d in zip(self.ishape, self.ksize, self.stride, self.padding, self.dilation))

    @property
    def klass(self):
        """floor class: kind of launch x arithmetic (x thin / activation where the accumulation differs)"""
        if self.kind == "wgrad":
            ar = arith(self.mode, 0, self.cout, wgrad=True)
            return "wgrad_thin" if self.cout <= 8 else "wgrad_" + ar
        if self.kind == "dgrad":
            merged = "mg" in self.edges
            rows = self.cin * (max(self.stride) if merged else 1)
            return "dgrad_" + arith(self.mode, self.cout, rows, merged)
        if self.kind == "convT":
            merged = "mg" in self.edges
            return "convT_" + arith(self.mode, self.cin, self.cout * (max(self.stride) if merged else 1), merged)
        ar = arith(self.mode, self.cin, self.cout)
        if self.cout <= 8:
            return "fwd_thin"
        return "fwd_" + ar + ("_act" if (self.act in ("gelu", "tanh", "sigmoid") or self.bwd or self.glu) else "")


def make_inputs(case):
    """fp32 CPU tensors of a case, drawn from its seed (weights scaled so that outputs are O(1))"""
    g = torch.Generator().manual_seed(1000 + case.seed)
    (IA, IB), (KA, KB), N = case.ishape, case.ksize, case.N
    r = lambda *s: torch.randn(*s, generator=g)
    inp = {}
    if case.kind == "convT":
        inp["x"] = r(N, case.cin, IA, IB)
        inp["w"] = r(case.cin, case.cout, KA, KB) / (case.cin * KA * KB / max(1, case.stride[0] * case.stride[1])) ** 0.5
    else:
        inp["x"] = r(N, case.cin, IA, IB)
        inp["w"] = r(case.cout, case.cin, KA, KB) / (case.cin * KA * KB) ** 0.5
    OA, OB = case.out_hw
    if case.bias:
        inp["b"] = r(case.cout)
    if case.kind in ("dgrad", "wgrad"):
        inp["g"] = r(N, case.cout, OA, OB)
    if case.kind == "wgrad" and case.unpack != "set":
        inp["dw0"] = r(case.cout, case.cin, KA, KB)
        inp["db0"] = r(case.cout)
    if case.res or case.bwd:
        shape = (N, case.cin, IA, IB) if case.kind == "dgrad" else (N, case.cout, OA, OB)
        inp["res"] = r(*shape)
    if case.act == "prelu":
        inp["slope"] = torch.linspace(0.05, 0.45, case.cout)
    if case.two_phase:
        inp["w2"] = r(case.cout, case.cin, 1, 1) / case.cin ** 0.5
        if case.two_phase == "in2":
            inp["x2"] = r(N, case.cin, IA, IB)
    if case.in16:                                  # a tensor stored in 16 bits holds bf16 values
        k = "g" if case.kind == "wgrad" else "x"
        inp[k] = bf16_rne(inp[k])
    return inp


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Ref:
    ref: torch.Tensor
    mag: torch.Tensor
    slack: torch.Tensor = None    # absolute slack per element (sign flips)
    flips: float = 0.0            # share of elements that carry it
    store16: bool = False
    staged: bool = False


def _shift_of(case):
    """second phase: 1x1 conv of in2[..., b + shift] (the TCN residual crop): centred"""
    return (case.ishape[1] - case.out_hw[1]) // 2


def reference(case, inp, got=None, K=None, drop=None):
    """{output name: Ref}.  Staged outputs ("glu", "stat") need `got` (the kernel's own stored "z" / "y") and are left out without it.
    K (per output name -> units of eps32 magnitude) is only needed for the sign-flip band of the backward epilogue."""
    x, w = inp["x"], inp["w"]
    st, pd, dl = case.stride, case.padding, case.dilation
    out = {}
    if case.kind == "wgrad":
        ar = arith(case.mode, case.cin, case.cout, wgrad=True)
        dw, mdw = bilinear(lambda a, b: wgrad(a, b, tuple(w.shape), st, pd, dl), x, inp["g"], ar, drop)
        gp = parts(inp["g"], ar)                                   # the ones column: 1 = hi, lo = 0 -> g_hi (+ g_lo)
        db, mdb = sum(p.sum((0, 2, 3)) for p in gp), sum(p.abs().sum((0, 2, 3)) for p in gp)
        if case.unpack != "set":
            dw, mdw = dw + inp["dw0"].double(), mdw + inp["dw0"].double().abs()
            db, mdb = db + inp["db0"].double(), mdb + inp["db0"].double().abs()
        out["dw"] = Ref(dw, mdw)
        if case.bias:
            out["db"] = Ref(db, mdb)
        return out
    if case.kind == "dgrad":
        merged = "mg" in case.edges
        ar = arith(case.mode, case.cout, case.cin * (max(st) if merged else 1), merged)
        lo = pd
        dx, m = bilinear(lambda a, b: convT(a, b, st, dl, lo, case.ishape), inp["g"], w, ar, drop)
        if case.res:
            dx, m = dx + inp["res"].double(), m + inp["res"].double().abs()
        out["dx"] = Ref(dx, m)
        return out
    if case.kind == "convT":
        merged = "mg" in case.edges
        ar = arith(case.mode, case.cin, case.cout * (max(st) if merged else 1), merged)
        y, m = bilinear(lambda a, b: convT(a, b, st, dl, case.crop[0], case.out_hw), x, w, ar, drop)
        if case.bias:
            y, m = y + inp["b"].double().view(1, -1, 1, 1), m + inp["b"].double().abs().view(1, -1, 1, 1)
        out["y"] = Ref(y, m)
        return out
    ar = arith(case.mode, case.cin, case.cout)
    u, A = bilinear(lambda a, b: conv(a, b, st, pd, dl), x, w, ar, drop)
    if case.bias:
        u, A = u + inp["b"].double().view(1, -1, 1, 1), A + inp["b"].double().abs().view(1, -1, 1, 1)
    slope = inp["slope"].double().view(1, -1, 1, 1) if "slope" in inp else None
    if case.bwd:
        G = inp["res"].double()
        y, m, sl = act_bwd(u, A, G, case.act, slope)
        r = Ref(y, m)
        if sl is not None:
            band = (u.abs() <= (K["y"] if K else MARGIN * 3 + EXTRA) * EPS32 * sl[1])
            r.slack = sl[0] * band.double()
            r.flips = float(band.double().mean())
        out["y"] = r
        if case.gslots:
            gs = torch.where(u < 0, G * u, torch.zeros_like(u))
            out["gparam"] = Ref(gs.sum((0, 2, 3)), (G.abs() * A * (u < 0).double()).sum((0, 2, 3)),
                                slack=(r.slack * 0 + (G.abs() * A * band.double())).sum((0, 2, 3)) if sl is not None else None)
        return out
    y, m = act_fwd(u, A, case.act, slope)
    if case.two_phase:
        s = _shift_of(case)
        x2 = inp.get("x2", x)[:, :, :, s:s + case.out_hw[1]]
        v2, m2 = bilinear(lambda a, b: conv(a, b, (1, 1), (0, 0), (1, 1)), x2, inp["w2"], ar, drop)
        y, m = y + v2, m + m2
    if case.res:
        y, m = y + inp["res"].double(), m + inp["res"].double().abs()
    if case.act2:
        y, m = act_fwd(y, m, case.act2)
    name = "z" if case.glu else "y"
    out[name] = Ref(y, m, store16=case.out16)
    if got is not None and case.glu:
        z = got["z"].double()
        Ch = case.cout // 2
        sg = torch.sigmoid(z[:, Ch:])
        out["glu"] = Ref(z[:, :Ch] * sg, (z[:, :Ch] * sg).abs(), staged=True)        # exact inputs: one product, one sigmoid
    if got is not None and case.stat_slots:
        v = got["y"].double()
        out["stat"] = Ref(torch.stack([v.sum((1, 2, 3)), (v * v).sum((1, 2, 3))], 1),
                          torch.stack([v.abs().sum((1, 2, 3)), (v * v).sum((1, 2, 3))], 1), staged=True)
    return out


# ---- the fp32 restatement ------------------------------------------------------------------------------------------------------------
def _block(ar, thin=False):
    return 1 if thin else (2 if ar == "f32" else 16)


def _accumulate(terms, order, B):
    """terms: [(W (M, K) fp64, X (N, K, P) fp64)]; K steps of B consecutive entries of `order` (-1 = padding): the block's products
    summed exactly, rounded once into the fp32 accumulator; bf16x3: one rounding per term and step"""
    N, _, P = terms[0][1].shape
    M = terms[0][0].shape[0]
    acc = torch.zeros(N, M, P, dtype=torch.float32)
    for k0 in range(0, len(order), B):
        idx = order[k0:k0 + B]
        idx = idx[idx >= 0]
        if idx.numel() == 0:
            continue
        for W, X in terms:
            acc = (acc.double() + torch.matmul(W[:, idx], X[:, idx, :])).float()
    return acc


def _order(ci, nt, ar, thin=False):
    """reduction order over (channel, tap) columns k = c * nt + t"""
    if ar == "f32" or thin:
        return torch.arange(ci * nt)
    cp = -(-ci // 8) * 8                                         # tap-major, channels in groups of 8 (padding -> -1)
    c = torch.arange(cp)
    o = torch.stack([torch.where(c < ci, c * nt + t, torch.full_like(c, -1)) for t in range(nt)]).reshape(-1)
    return o


def _conv_cols(x, ksize, stride, padding, dilation):
    return F.unfold(x, ksize, dilation, padding, stride)         # (N, C * KA * KB, P), k = c * nt + t


def _transposed_as_conv(x, w, stride, dilation, lo, out_len):
    """(zero-stuffed, padded operand; conv weight (rows, gathered, KA, KB)) with conv(xs, wc, dilation) == the FULL transposed output"""
    N, Cg, IA, IB = x.shape
    KA, KB = w.shape[2:]
    xs = x.new_zeros(N, Cg, (IA - 1) * stride[0] + 1, (IB - 1) * stride[1] + 1)
    xs[:, :, ::stride[0], ::stride[1]] = x
    pa, pb = dilation[0] * (KA - 1), dilation[1] * (KB - 1)
    xs = F.pad(xs, (pb, pb + max(0, lo[1] + out_len[1]), pa, pa + max(0, lo[0] + out_len[0])))
    return xs, w.flip(2, 3).transpose(0, 1).contiguous()


def restate_fwd(case, inp, mutate=None):
    """fp32 restatement of a forward-family case: {name: tensor in the storage type's values (fp32)}"""
    x, w = inp["x"], inp["w"]
    st, pd, dl = case.stride, case.padding, case.dilation
    drop = 2 if mutate == "lo_hi_dropped" else None
    if case.kind == "conv":
        ar = arith(case.mode, case.cin, case.cout)
        thin = case.cout <= 8
        OA, OB = case.out_hw
        nt = case.ksize[0] * case.ksize[1]
        terms = [(pw.reshape(case.cout, -1), _conv_cols(px, case.ksize, st, pd, dl)) for px, pw in term_pairs(x, w, ar, drop)]
        acc = _accumulate(terms, _order(case.cin, nt, ar, thin), _block(ar, thin)).reshape(case.N, case.cout, OA, OB)
        if mutate in ("tap_missing_first_col", "tap_missing_last_col"):
            wt = torch.zeros_like(w)
            t = (case.ksize[1] - 1) if mutate == "tap_missing_first_col" else 0
            wt[:, :, :, t] = w[:, :, :, t]
            col = 0 if mutate == "tap_missing_first_col" else OB - 1
            contrib = bilinear(lambda a, b: conv(a, b, st, pd, dl), x, wt, ar)[0]
            acc[..., col] = (acc[..., col].double() - contrib[..., col]).float()
        if case.bias:
            acc = acc + inp["b"].view(1, -1, 1, 1)
        slope = inp["slope"].view(1, -1, 1, 1) if "slope" in inp else None
        if case.bwd:
            G = inp["res"]
            y = (G.double() * act_bwd(acc.double(), acc.double().abs(), torch.ones_like(G).double(), case.act,
                                      slope.double() if slope is not None else None)[0]).float()
            out = {"y": y}
            if case.gslots:
                out["gparam"] = torch.where(acc < 0, G * acc, torch.zeros_like(acc)).sum((0, 2, 3))
            return out
        y = act_fwd(acc.double(), acc.double(), case.act, slope.double() if slope is not None else None)[0].float()
        if case.two_phase:
            s = _shift_of(case)
            x2 = inp.get("x2", x)[:, :, :, s:s + OB]
            terms2 = [(pw.reshape(case.cout, -1), _conv_cols(px, (1, 1), (1, 1), (0, 0), (1, 1))) for px, pw in term_pairs(x2, inp["w2"], ar, drop)]
            N, M = case.N, case.cout
            a2 = y.reshape(N, M, -1)
            for k0 in range(0, case.cin, _block(ar)):             # the second phase keeps accumulating into act(v)
                for W, X in terms2:
                    a2 = (a2.double() + torch.matmul(W[:, k0:k0 + _block(ar)], X[:, k0:k0 + _block(ar), :])).float()
            y = a2.reshape(N, M, OA, OB)
        if case.res:
            y = y + inp["res"]
            if mutate == "residual_twice_one_row":
                y[:, case.cout - 1] += inp["res"][:, case.cout - 1]
        if case.act2:
            y = act_fwd(y.double(), y.double(), case.act2)[0].float()
        if mutate == "ragged_row_from_neighbour":
            y = y.clone()
            y[:, case.cout - 1] = y[:, case.cout - 2]
        if mutate == "glu_halves_swapped":
            y = y.clone()
            Ch = case.cout // 2
            y[:, Ch - 1], y[:, case.cout - 1] = y[:, case.cout - 1].clone(), y[:, Ch - 1].clone()
        if case.out16:
            y = bf16_trunc(y) if mutate == "truncating_store" else bf16_rne(y)
        if mutate == "one_element_off":
            y = y.clone()
            y.view(-1)[y.numel() // 3] += 1e-3 * float(y.abs().max())
        out = {"z" if case.glu else "y": y}
        if case.glu:
            Ch = case.cout // 2
            out["glu"] = (y[:, :Ch].double() * torch.sigmoid(y[:, Ch:].double())).float()
        if case.stat_slots:
            s1 = torch.zeros(case.N, OA, OB)
            s2 = torch.zeros(case.N, OA, OB)
            for m in range(case.cout):                            # a lane adds its rows in fp32, the wave / slot sums are fp64
                s1 = s1 + y[:, m]
                s2 = s2 + y[:, m] * y[:, m]
            out["stat"] = torch.stack([s1.double().sum((1, 2)), s2.double().sum((1, 2))], 1)
        return out
    # transposed family: dgrad (operand g, weight (Cout, Cin, KA, KB)) and convT (operand x, weight (Cin, Cout, KA, KB))
    merged = "mg" in case.edges
    if case.kind == "dgrad":
        op, rows, gathered, lo, olen = inp["g"], case.cin, case.cout, pd, case.ishape
    else:
        op, rows, gathered, lo, olen = x, case.cout, case.cin, case.crop[0], case.out_hw
    ar = arith(case.mode, gathered, rows * (max(st) if merged else 1), merged)
    thin = rows <= 8 and not merged
    nt = case.ksize[0] * case.ksize[1]
    terms = []
    for po, pw in term_pairs(op, w, ar, drop):
        xs, wc = _transposed_as_conv(po, pw, st, dl, lo, olen)
        terms.append((wc.reshape(rows, -1), _conv_cols(xs, case.ksize, (1, 1), (0, 0), dl)))
        full_hw = (xs.shape[2] - dl[0] * (case.ksize[0] - 1), xs.shape[3] - dl[1] * (case.ksize[1] - 1))
    acc = _accumulate(terms, _order(gathered, nt, ar, thin), _block(ar, thin)).reshape(case.N, rows, *full_hw)
    if mutate == "merged_phase_off_by_one":
        acc = torch.roll(acc, 1, 3 if st[1] > 1 else 2)
    full = acc
    y = acc[:, :, lo[0]:lo[0] + olen[0], lo[1]:lo[1] + olen[1]].clone()
    if case.bias and case.kind == "convT":
        b = inp["b"]
        if mutate == "bias_by_row":
            G = max(st)
            ax = 3 if st[1] > 1 else 2
            o = torch.arange(y.shape[ax]) + lo[ax - 2]
            rowidx = (torch.arange(rows).view(-1, 1) * G + (o % G).view(1, -1)) % rows          # (rows, positions)
            bb = b[rowidx]
            y = y + (bb.view(1, rows, 1, -1) if ax == 3 else bb.view(1, rows, -1, 1))
        else:
            y = y + b.view(1, -1, 1, 1)
    if case.res:
        y = y + inp["res"]
    if mutate == "quad_past_mg_len":                              # the quad that straddles mg_len stored whole: in a contiguous tensor its
        ax = 3 if st[1] > 1 else 2                                # tail lands on the first elements of the next row
        q = (lo[ax - 2] + olen[ax - 2]) % 4 or 2
        if ax == 3:
            y[:, 1:, 0, :q] = full[:, :-1, lo[0], lo[1] + olen[1]:lo[1] + olen[1] + q]
        else:
            y[:, 1:, :q, 0] = full[:, :-1, lo[0] + olen[0]:lo[0] + olen[0] + q, lo[1]]
    if mutate == "one_element_off":
        y.view(-1)[y.numel() // 3] += 1e-3 * float(y.abs().max())
    return {"dx" if case.kind == "dgrad" else "y": y}


def _wave_sum32(t):
    """butterfly over the last axis (64 lanes) in fp32"""
    n = t.shape[-1]
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:2 * n]
    return t[..., 0]


def _unpack_sum(parts_, col=False):
    """sum of the split matrices (list of fp32 tensors) in the unpack kernels' order"""
    S = len(parts_)
    if col:
        s = torch.zeros_like(parts_[0])
        for p in parts_:
            s = s + p
        return s
    per = (S + 3) // 4
    gs = []
    for sg in range(4):
        s = torch.zeros_like(parts_[0])
        for p in parts_[sg * per:min((sg + 1) * per, S)]:
            s = s + p
        gs.append(s)
    return ((gs[0] + gs[1]) + gs[2]) + gs[3]


def restate_wgrad(case, inp, family, splits, mutate=None):
    """fp32 restatement of the weight gradient: family / splits as rfx_gemm_wgrad_variant reports them (host selection, not a kernel)"""
    x, g, w = inp["x"], inp["g"], inp["w"]
    st, pd, dl = case.stride, case.padding, case.dilation
    N, M = case.N, case.cout
    OA, OB = case.out_hw
    P = OA * OB
    ar = arith(case.mode, case.cin, M, wgrad=True)
    drop = 2 if mutate == "lo_hi_dropped" else None
    xc = []
    for i, px in enumerate(parts(x, ar)):                           # (N, K, P); the ones column splits into hi = 1, lo = 0
        cols = _conv_cols(px, case.ksize, st, pd, dl)
        if case.bias:
            cols = torch.cat([cols, torch.full((N, 1, P), 1.0 if i == 0 else 0.0, dtype=torch.float64)], 1)
        xc.append(cols)
    gp = [p.reshape(N, M, P) for p in parts(g, ar)]
    terms = [(xc[0], gp[0])] if ar != "bf16x3" else [(xc[0], gp[0]), (xc[0], gp[1]), (xc[1], gp[0])]
    if drop is not None and ar == "bf16x3":
        del terms[drop]
    K = terms[0][0].shape[1]
    # position blocks: (n, tile) order; tiles of 32 positions of a sample (64-position chunks of one (n, a) row for the wide kernel)
    if family == 3:
        unit, rowlen, nrows = 64, OB, N * OA
    else:
        unit, rowlen, nrows = 32, P, N
    tiles_per_row = -(-rowlen // unit)
    pad = tiles_per_row * unit - rowlen
    def tiled(t):                                                   # (N, R, P) -> (tiles, R, unit)
        R = t.shape[1]
        t = t.reshape(N, R, nrows // N, rowlen)
        t = F.pad(t, (0, pad)).reshape(N, R, nrows // N, tiles_per_row, unit)
        return t.permute(0, 2, 3, 1, 4).reshape(-1, R, unit)
    tt = [(tiled(c), tiled(gg)) for c, gg in terms]
    T = tt[0][0].shape[0]
    if family == 0:                                                 # thin: flattened (n, p) cut into `splits` chunks, 64 lanes of fmaf, butterfly
        total = N * P
        chunk = -(-total // splits)
        cols = [(c.permute(1, 0, 2).reshape(K, total), gg.permute(1, 0, 2).reshape(M, total)) for c, gg in terms]
        outs = []
        for s in range(splits):
            q0, q1 = s * chunk, min((s + 1) * chunk, total)
            L = -(-(q1 - q0) // 64) * 64
            c = F.pad(cols[0][0][:, q0:q1], (0, L - (q1 - q0))).reshape(K, -1, 64)
            gg = F.pad(cols[0][1][:, q0:q1], (0, L - (q1 - q0))).reshape(M, -1, 64)
            acc = torch.zeros(M, K, 64, dtype=torch.float32)
            for i in range(c.shape[1]):
                acc = (acc.double() + gg[:, None, i, :] * c[None, :, i, :]).float()
            outs.append(_wave_sum32(acc))
    else:
        B = 2 if family == 1 else 16
        tpb = -(-T // splits)
        outs = []
        for s in range(splits):
            acc = torch.zeros(M, K, dtype=torch.float32)
            for t in range(s * tpb, min((s + 1) * tpb, T)):
                for b0 in range(0, unit, B):
                    for c, gg in tt:
                        acc = (acc.double() + gg[t][:, b0:b0 + B] @ c[t][:, b0:b0 + B].T).float()
            outs.append(acc)
    if mutate == "split_missing" and len(outs) > 1:
        del outs[len(outs) // 2]
    tot = _unpack_sum(outs)                                         # (M, K)
    nw = K - (1 if case.bias else 0)
    dw = tot[:, :nw].reshape(w.shape).clone()
    out = {}
    if case.bias:
        col = nw - 1 if mutate == "bias_col_k_minus_2" else nw
        db = _unpack_sum([o[:, col] for o in outs], col=(case.unpack == "set"))
        if case.unpack != "set":
            db = inp["db0"] + db
        out["db"] = db
    if case.unpack != "set":
        dw = inp["dw0"] + dw
    if mutate == "pruned_tap_nonzero":
        ref0 = reference(case, inp)["dw"]
        dead = (ref0.mag == 0).nonzero()
        dw[tuple(dead[0])] = 1e-7
    if mutate == "one_element_off":
        dw.view(-1)[dw.numel() // 3] += 1e-3 * float(dw.abs().max())
    out["dw"] = dw
    return out


# ---- bound --------------------------------------------------------------------------------------------------------------------------
# class -> {output: floor}: the restatement's largest error in units of eps32 magnitude over the class's cases, rounded up to the next
# quarter (tests/test_gemm_ref_cpu.py::test_floors measures them and asserts this table is neither below nor far above)
FLOORS = {
    "fwd_thin": {"y": 1.25, "stat": 0.25, "gparam": 0.25},
    "fwd_f32": {"y": 2.0},
    "fwd_f32_act": {"y": 0.75, "gparam": 0.25},
    "fwd_bf16x3": {"y": 1.5, "stat": 0.25},
    "fwd_bf16x3_act": {"y": 0.5, "gparam": 0.25, "z": 1.0, "glu": 0.5},
    "fwd_bf16": {"y": 1.0, "stat": 0.25},
    "fwd_bf16_act": {"y": 0.5, "gparam": 0.25, "z": 0.75, "glu": 0.5},
    "dgrad_f32": {"dx": 2.0},
    "dgrad_bf16x3": {"dx": 1.0},
    "dgrad_bf16": {"dx": 0.75},
    "convT_f32": {"y": 2.25},
    "convT_bf16x3": {"y": 1.0},
    "convT_bf16": {"y": 0.75},
    "wgrad_thin": {"dw": 0.25, "db": 0.25},
    "wgrad_f32": {"dw": 1.5, "db": 0.75},
    "wgrad_bf16x3": {"dw": 1.0, "db": 0.5},
    "wgrad_bf16": {"dw": 0.75, "db": 0.25},
}


def k_of(case, name):
    return MARGIN * FLOORS[case.klass][name] + EXTRA


def tolerance(r, K):
    t = K * EPS32 * r.mag
    if r.slack is not None:
        t = t + r.slack
    if r.store16:
        t = t + 0.5 * ulp(r.ref.abs() + t, 7)                      # RNE store: half a bf16 ulp of the value the kernel rounded
    return t


def measure(case, inp, got):
    """{name: largest |got - ref| / (eps32 magnitude)} (sign-flip slack and the 16-bit store's half ulp taken off first)"""
    refs = reference(case, inp, got)
    fl = {}
    for k, r in refs.items():
        e = (got[k].double() - r.ref).abs()
        if r.slack is not None:
            e = e - r.slack
        if r.store16:
            e = e - 0.5 * ulp(r.ref.abs() + e, 7)
        fl[k] = float((e / (EPS32 * r.mag).clamp_min(1e-300)).clamp_min(0).max())
    return fl


def judge(case, inp, got):
    """{name: (error / tolerance of the worst element, its flat index, Ref)} with the committed floors"""
    K = {k: k_of(case, k) for k in FLOORS[case.klass]}
    refs = reference(case, inp, got, K)
    return {k: worst(got[k], r.ref, tolerance(r, K[k])) + (r,) for k, r in refs.items()}


def old_accepts(case, inp, got, name):
    """would the whole-tensor RMS assertion of tests/test_gpu_conv.py, in this case's mode, accept `got`?  (reference there: torch fp32
    on the CPU of the UNROUNDED operands; rms < tol(mode) max(1, max |ref|), 1e-5 forward / 2e-5 gradients, 2e-2 in bf16 mode)"""
    plain = dataclasses.replace(case, mode="f32")
    ref = reference(plain, {k: (v.float() if torch.is_tensor(v) else v) for k, v in inp.items()}, got)[name].ref
    f32 = 1e-5 if name in ("y", "z") else 2e-5
    bound = f32 if case.mode != "bf16" else min(0.25, max(2e-2, 100.0 * f32))
    rms = float(((got[name].double() - ref) ** 2).mean().sqrt())
    return rms < bound * max(1.0, float(ref.abs().max()))


# ---- instantiation names ------------------------------------------------------------------------------------------------------------
def fwd_name(code, prec):
    """rfx_gemm_fwd_variant code -> the instantiation as the sources spell it (csrc/gemm.hip)"""
    kind, r = code >> 4, code & 15
    if kind == 0:
        return "gemm_thin_fwd_kernel"
    if kind == 1:
        return f"gemm_fwd_kernel<{r}>"
    if kind == 2:
        return f"gemm_tap_kernel<{r}, {prec}>"
    if kind == 3:
        return f"gemm_tap_kernel<{r}, 2, IN16>"
    if kind in (4, 5):
        return f"gemm_tap_stream_kernel<{prec}, {'4, 1' if kind == 4 else '2, 4'}>"
    return f"gemm_halo_kernel<{r}, {9 if kind in (6, 7) else 3}, {kind & 1}>"


_BF = {0: "3, 1, 1", 1: "1, 2, 1", 2: "1, 1, 1", 3: "2, 2, 2", 4: "2, 1, 2", 5: "1, 2, 2", 6: "1, 1, 2"}
_WIDE = {0: "3, 1, 1", 1: "1, 2, 1", 2: "1, 1, 1", 3: "2, 2, 2", 4: "1, 2, 2", 5: "3, 2, 1"}


def wgrad_decode(code):
    return dict(splits=code & 0x1fff, xcd=(code >> 13) & 1, g16=(code >> 14) & 1, shape=(code >> 16) & 15, family=code >> 20)


def wgrad_name(code, prec):
    """rfx_gemm_wgrad_variant code -> instantiation (csrc/gemm_wgrad.hip, gemm_wgrad.h)"""
    v = wgrad_decode(code)
    f, s = v["family"], v["shape"]
    if f == 0:
        return f"gemm_thin_wgrad_kernel<{s}>"
    if f == 1:
        return f"gemm_wgrad_kernel<{s // 2 + 1}, {s % 2 + 1}>"
    fam, tab = ("gemm_wgrad_bf_kernel", _BF) if f == 2 else ("gemm_wgrad_wide_kernel", _WIDE)
    return f"{fam}<{tab[s]}, {prec}{', G16' if v['g16'] else ''}>"


def store_paths(case, R):
    """The 16-bit store branches of fwd_epilogue_store a "conv" case's geometry reaches, restated from csrc/gemm_fwd.h for the outputs
    launch() allocates (unit position stride, no output phase): pairs need an even OB and even strides (rfx_pair16_geo); the lean
    raw-buffer store needs every lane of a wave's 32 positions valid and, plain store, rows full or dropped by the range check (M even,
    rfx_fast_store_geo) / GLU store, rows full (fwd_tile_full without records)."""
    if not case.out16:
        return set()
    OA, OB = case.out_hw
    P, M = OA * OB, case.cout
    extra = 2 if "slice" in case.view else 0
    pair = OB % 2 == 0 and P % 2 == 0 and ((M + extra) * P) % 2 == 0
    pre = "glu16_" if case.glu else "store16_"
    if not pair:
        return {pre + "unpaired"}
    wave_full, wave_ragged = P >= 32, P % 32 != 0              # some wave has all 32 positions / some wave does not
    rows_full = M >= 32 * R if case.glu else (M >= 32 * R or M % 2 == 0)
    rows_ragged = M % (32 * R) != 0 if case.glu else (M % (32 * R) != 0 and M % 2 != 0)
    got = set()
    if wave_full and rows_full:
        got.add(pre + "lean")
    if wave_ragged or rows_ragged:
        got.add(pre + ("generic" if case.glu else "pair_generic"))
    return got


def thin_fwd_name(M):
    return f"gemm_thin_fwd_kernel<{1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8}>"


# ---- the shipped launch path, on the GPU or dry (host selection only) ------------------------------------------------------------------
class _Proxy:
    """libremfx_hip seen through a recorder: notes the row count of every rfx_gemm_fwd (the thin kernels' template argument is not in
    the variant code).  dry: every launch is a no-op; the pure host functions (the two variant queries, pick_r) stay the library's own"""
    HOST = ("rfx_gemm_fwd_variant", "rfx_gemm_wgrad_variant", "rfx_gemm_pick_r", "rfx_abi_version")

    def __init__(self, real, dry_run):
        self.real, self.dry, self.fwd_rows = real, dry_run, []

    def __getattr__(self, name):
        real = getattr(self.real, name)
        if name in self.HOST:
            return real
        if name == "rfx_gemm_fwd":
            def fwd_(desc, *a):
                self.fwd_rows.append(int(desc._obj.M))
                return 0 if self.dry else real(desc, *a)
            return fwd_
        if not self.dry:
            return real
        if name == "rfx_gemm_wgrad":
            def wgrad_(desc, ktab, x, g, ws, cap, ns, prec, stream):
                code = self.real.rfx_gemm_wgrad_variant(desc, cap, prec)
                if code < 0:
                    return -1
                ns._obj.value = code & 0x1fff
                return 0
            return wgrad_
        return lambda *a: 0


@contextlib.contextmanager
def recorder(dry_run):
    """remfx_amd.ops with the library behind a _Proxy.  dry_run: CPU tensors, nothing is launched -- plans, descriptors and the
    launchers' selection are the real ones"""
    from remfx_amd import _lib, ops
    real = _lib.lib()
    saved = (_lib.lib, ops.raw_stream, ops._req)
    proxy = _Proxy(real, dry_run)
    _lib.lib = lambda: proxy
    if dry_run:
        ops.raw_stream, ops._req = (lambda: 0), (lambda *a: None)
    try:
        yield proxy
    finally:
        _lib.lib, ops.raw_stream, ops._req = saved


@contextlib.contextmanager
def case_env(case):
    """arithmetic mode, planner switches and caches of one case; everything restored afterwards"""
    from remfx_amd import convplan, ops
    prev = (ops.gemm_precision(), convplan.HALO_MIN_POSITIONS, ops.WGRAD_SPLITS, ops.TRACE_VARIANT, ops.TRACE_WGRAD, ops.BF16_STORE)
    ops.set_gemm_precision(case.mode)
    if case.halo:
        convplan.HALO_MIN_POSITIONS = 0
    if case.wsplits is not None:
        ops.WGRAD_SPLITS = case.wsplits
    ops._PLANS.clear()
    ops.clear_pack_cache()
    ops.TRACE_VARIANT, ops.TRACE_WGRAD = [], []
    try:
        yield ops.TRACE_VARIANT, ops.TRACE_WGRAD
    finally:
        ops.set_gemm_precision(prev[0])
        convplan.HALO_MIN_POSITIONS, ops.WGRAD_SPLITS, ops.TRACE_VARIANT, ops.TRACE_WGRAD, ops.BF16_STORE = prev[1:]
        ops._PLANS.clear()
        ops.clear_pack_cache()


def _cpu_alloc(shape, dtype, fill=None):
    return torch.empty(shape, dtype=dtype) if fill is None else torch.full(shape, fill, dtype=dtype)


def launch(case, inp, dev="cpu", alloc=_cpu_alloc):
    """One case through remfx_amd.ops (call inside case_env and recorder(); recorder(True) without a GPU).  alloc(shape, dtype[, fill]) hands out the output
    buffers (the GPU test: NaN-filled between guards).  -> {output name: tensor}"""
    from remfx_amd import convplan, ops
    d = lambda t: t.to(dev)
    N, Cin, Cout = case.N, case.cin, case.cout
    (IA, IB), (KA, KB) = case.ishape, case.ksize
    st, pd, dl = tuple(case.stride), tuple(case.padding), tuple(case.dilation)
    OA, OB = case.out_hw
    x, w = d(inp["x"]), d(inp["w"])
    b = d(inp["b"]) if case.bias else None
    if "perm" in case.view:                                         # same values, the two position axes swapped in memory
        x = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    out = {}
    if case.kind == "conv":
        if case.in16:
            x = x.to(torch.bfloat16)
        extra = 2 if "slice" in case.view else 0              # sample stride larger than the tensor; the spare channels must stay untouched
        ybuf = alloc((N, Cout + extra, OA, OB), torch.bfloat16 if case.out16 else torch.float32)
        y = ybuf[:, :Cout]
        if extra:
            out["_gap"] = ybuf[:, Cout:]
        key = ops._key("cf", x.shape, x.stride(), w.shape, st, pd, dl, y.stride())
        dp = ops._plans(key, x.device, lambda: convplan.conv_fwd_plan(tuple(x.shape), x.stride(), tuple(w.shape), st, pd, dl, y.stride()))
        kw = dict(bias=b, act=case.act, act_param=d(inp["slope"]) if "slope" in inp else None, act2=case.act2)
        if case.glu:
            Ch = Cout // 2
            apack = ops.pack_cached(dp, w, tag=2, derive=lambda t: t.reshape(2, Ch, Cin, KA, KB).transpose(0, 1).reshape(Cout, Cin, KA, KB))
            out["glu"] = kw["glu_out"] = alloc((N, Ch, OA, OB), torch.float32)
        else:
            apack = ops.pack_cached(dp, w)
        if case.res or case.bwd:
            kw["res"] = d(inp["res"])
        if case.bwd:
            kw["bwd"] = True
            if case.gslots:
                out["gparam"] = kw["gparam"] = alloc((case.gslots, Cout) if case.gslots > 1 else (Cout,), torch.float32, 0.0)
        if case.stat_slots:
            out["stat"] = kw["stat_sums"] = alloc((N, case.stat_slots, 2) if case.stat_slots > 1 else (N, 2), torch.float64, 0.0)
        if case.two_phase:
            s = _shift_of(case)
            def build2():
                p2 = convplan.shift_plan(tuple(x.shape), x.stride(), Cout, s, (N, Cout, OA, OB), y.stride())
                p2.R, p2.Mpad = dp.p.R, dp.p.Mpad                   # both phases share one launch geometry (remfx_amd/tcn.py)
                return p2
            dp2 = ops._plans(ops._key("sh", x.shape, x.stride(), Cout, s, y.stride()), x.device, build2)
            w2 = d(inp["w2"])
            kw.update(dp2=dp2, apack2=ops.pack_cached(dp2, w2), in2=d(inp["x2"]) if "x2" in inp else None)
        ops.gemm_fwd(dp, apack, x, y, **kw)
        out["z" if case.glu else "y"] = y
        if case.gslots > 1:
            out["gparam"] = out["gparam"].sum(0)
        if case.stat_slots > 1:
            out["stat"] = out["stat"].sum(1)
        return out
    if case.kind == "dgrad":
        g = d(inp["g"])
        dx = alloc((N, Cin, IA, IB), torch.float32)
        res = d(inp["res"]) if case.res else None
        out["dx"] = ops.conv2d_dgrad(g, w, tuple(dx.shape), tuple(dx.stride()), st, pd, dl, dx=dx, res=res)
        return out
    if case.kind == "convT":
        y = alloc((N, Cout, OA, OB), torch.float32)
        ops.convT2d_forward(x, w, b, st, dl, tuple(case.crop[0]), (OA, OB), out=y)
        out["y"] = y
        return out
    # weight gradient: the plan of ops.conv2d_wgrad, ops.gemm_wgrad, then the unpack entry point the case names
    g = d(inp["g"])
    if case.in16:
        g = g.to(torch.bfloat16)
    key = ops._key("cw", x.shape, x.stride(), w.shape, st, pd, dl, g.stride(), case.bias)
    dp = ops._plans(key, x.device, lambda: convplan.conv_fwd_plan(tuple(x.shape), x.stride(), tuple(w.shape), st, pd, dl, g.stride(), bias_row=case.bias))
    p = dp.p
    wg = ops.gemm_wgrad(dp, x, g)
    if case.unpack == "set":
        dw = alloc(tuple(w.shape), torch.float32, None if p.extra.get("dense", True) else 0.0)
        ops.unpack_set(dp, wg, dw)
        if case.bias:
            db = alloc((Cout,), torch.float32)
            ops.launch("rfx_unpack_col", wg.ws, p.M, p.Kpad, p.K - 1, wg.splits, db)
    else:
        dw = alloc(tuple(w.shape), torch.float32, 0.0)
        dw.copy_(d(inp["dw0"]))
        if case.bias:
            db = alloc((Cout,), torch.float32, 0.0)
            db.copy_(d(inp["db0"]))
        if case.unpack == "add_bias":
            ops.launch("rfx_unpack_add_bias", wg.ws, dp.woff, p.w_ms, p.M, p.extra["n_weight_rows"], p.Kpad, dw, p.K - 1, db, wg.splits)
        else:
            ops.unpack_add(dp, wg, dw)
            if case.bias:
                db.add_(ops.unpack_col(dp, wg, p.K - 1))
    out["dw"] = dw
    if case.bias:
        out["db"] = db
    return out


def forms_of(case, tf, tw, rows):
    """names of the launches behind the traced variant codes (+ the rows of every forward launch, for the thin kernels)"""
    prec = {"f32": 0, "bf16x3": 1, "bf16": 2}[case.mode]
    fn = [thin_fwd_name(m) if (c >> 4) == 0 else fwd_name(c, prec if (c >> 4) != 1 else 0) for c, m in zip(tf, rows)]
    return fn, [("refused" if c < 0 else wgrad_name(c, prec)) for c in tw]


def host_forms(case):
    """(forward-family names, weight-gradient names, weight-gradient codes) of the launches a case makes: the launchers' own selection,
    evaluated without a GPU"""
    inp = make_inputs(case)
    with case_env(case) as (tf, tw), recorder(True) as px:
        launch(case, inp)
        tf, tw = list(tf), list(tw)
    return forms_of(case, tf, tw, px.fwd_rows) + (tw,)


# ---- case table -------------------------------------------------------------------------------------------------------------------------
def _c(id, kind, mode, form, cin, cout, ishape, ksize, **kw):
    return Case(id, kind, mode, tuple(form) if isinstance(form, (list, tuple)) else (form,), cin, cout, tuple(ishape), tuple(ksize), **kw)


def case_table():
    T = []
    a = T.append
    # ---- forward family: thin kernels (exact fp32 in every mode), P no multiple of 256
    a(_c("thin1-stat1", "conv", "f32", "gemm_thin_fwd_kernel<1>", 12, 1, (1, 300), (1, 3), padding=(0, 1), stat_slots=1, edges=("P%256", "stat1")))
    a(_c("thin2-two-phase-res", "conv", "bf16", "gemm_thin_fwd_kernel<2>", 10, 2, (1, 333), (1, 5), dilation=(1, 2), act="prelu", two_phase="in", res=True,
         edges=("P%256", "two_phase_in", "res", "dilation_b")))
    a(_c("thin4-bwd-prelu", "conv", "bf16x3", "gemm_thin_fwd_kernel<4>", 9, 3, (1, 301), (1, 3), act="prelu", bwd=True, gslots=1,
         edges=("P%256", "bwd_prelu", "gslots1")))
    a(_c("thin8-2d-stat16", "conv", "f32", "gemm_thin_fwd_kernel<8>", 12, 7, (9, 18), (5, 3), stride=(2, 1), padding=(2, 1), stat_slots=16,
         edges=("stride_a", "stat16", "P%32")))
    a(_c("thin8-bwd-gelu-slots8", "conv", "f32", "gemm_thin_fwd_kernel<8>", 8, 8, (1, 520), (1, 3), act="gelu", bwd=True, edges=("bwd_other",)))
    a(_c("thin4-in2-act2", "conv", "f32", "gemm_thin_fwd_kernel<4>", 6, 4, (1, 270), (1, 3), act="relu", two_phase="in2", act2="tanh",
         edges=("two_phase_in2", "act2")))
    # ---- exact fp32 channel-major kernel: every R, and Cin < 8 in every mode
    a(_c("f32-r1-m31", "conv", "f32", "gemm_fwd_kernel<1>", 5, 31, (1, 200), (1, 7), dilation=(1, 4), edges=("M31", "Kpad", "P%32")))
    a(_c("f32-r1-m32-relu", "conv", "f32", "gemm_fwd_kernel<1>", 12, 32, (3, 50), (3, 3), padding=(1, 1), act="relu", edges=("M32", "taps_meet_padding_kept")))
    a(_c("f32-r2-m33", "conv", "f32", "gemm_fwd_kernel<2>", 16, 33, (17, 23), (3, 3), padding=(1, 1), edges=("M33", "P%32")))
    a(_c("f32-r3-m95-leaky", "conv", "f32", "gemm_fwd_kernel<3>", 10, 95, (1, 260), (1, 7), act="leaky", edges=("M95",)))
    a(_c("f32-r3-m96-res-act2", "conv", "f32", "gemm_fwd_kernel<3>", 9, 96, (16, 40), (8, 1), stride=(4, 1), padding=(2, 0), res=True, act2="relu",
         edges=("M96", "stride_a", "res", "act2")))
    a(_c("f32-r4-m97-sigmoid", "conv", "f32", "gemm_fwd_kernel<4>", 9, 97, (1, 140), (1, 8), stride=(1, 4), padding=(0, 2), act="sigmoid", edges=("M97", "stride_b")))
    a(_c("f32-r1-perm-slice", "conv", "f32", "gemm_fwd_kernel<1>", 9, 24, (6, 50), (1, 3), padding=(0, 2), dilation=(1, 2), view="perm+slice", edges=("noncontig_in", "out_slice")))
    a(_c("f32-r2-slice-tanh", "conv", "f32", "gemm_fwd_kernel<2>", 24, 40, (1, 130), (1, 3), act="tanh", view="slice", edges=("out_slice",)))
    a(_c("f32-r2-two-phase", "conv", "f32", "gemm_fwd_kernel<2>", 16, 48, (1, 200), (1, 7), dilation=(1, 2), act="prelu", two_phase="in",
         edges=("two_phase_in",)))
    a(_c("f32-r1-bwd-prelu-slots8", "conv", "f32", "gemm_fwd_kernel<1>", 16, 24, (1, 400), (1, 3), act="prelu", bwd=True, gslots=8,
         edges=("bwd_prelu", "gslots8")))
    a(_c("cin3-bf16", "conv", "bf16", "gemm_fwd_kernel<1>", 3, 24, (1, 500), (1, 7), dilation=(1, 4), edges=("cin<8",)))
    a(_c("cin7-bf16x3-r2", "conv", "bf16x3", "gemm_fwd_kernel<2>", 7, 48, (64, 10), (10, 1), stride=(4, 1), padding=(3, 0), edges=("cin<8",)))
    # ---- tap-major kernel: R x mode
    for mode, pm in (("bf16x3", 1), ("bf16", 2)):
        a(_c(f"tap-r1-m31-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 20, 31, (6, 50), (1, 3), padding=(0, 1), edges=("M31", "gpt_pad", "P%32")))
        a(_c(f"tap-r1-m32-gelu-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 16, 32, (1, 200), (1, 7), dilation=(1, 2), act="gelu", edges=("M32", "dilation_b")))
        a(_c(f"tap-r2-m33-{mode}", "conv", mode, f"gemm_tap_kernel<2, {pm}>", 24, 33, (17, 23), (3, 3), padding=(1, 1), edges=("M33", "P%32", "P%128")))
        a(_c(f"tap-r3-m95-{mode}", "conv", mode, f"gemm_tap_kernel<3, {pm}>", 48, 95, (8, 20), (8, 1), stride=(4, 1), padding=(2, 0), edges=("M95", "stride_a")))
        a(_c(f"tap-r3-m96-res-{mode}", "conv", mode, f"gemm_tap_kernel<3, {pm}>", 16, 96, (1, 140), (1, 8), stride=(1, 4), padding=(0, 2), res=True, edges=("M96", "stride_b", "res")))
        a(_c(f"tap-r4-m97-{mode}", "conv", mode, f"gemm_tap_kernel<4, {pm}>", 12, 97, (6, 70), (3, 3), padding=(1, 1), dilation=(2, 1), edges=("M97", "dilation_a", "gpt_pad")))
        a(_c(f"tap-r1-pruned-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 24, 24, (1, 96), (3, 3), padding=(1, 1), edges=("taps_pruned",)))
        a(_c(f"tap-r2-two-phase-in2-{mode}", "conv", mode, f"gemm_tap_kernel<2, {pm}>", 16, 48, (1, 200), (1, 7), dilation=(1, 2), act="prelu", two_phase="in2",
             edges=("two_phase_in2",)))
        a(_c(f"tap-r1-bwd-prelu-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 16, 24, (1, 400), (1, 3), act="prelu", bwd=True, gslots=8,
             edges=("bwd_prelu", "gslots8")))
        a(_c(f"tap-r2-stat16-{mode}", "conv", mode, f"gemm_tap_kernel<2, {pm}>", 16, 40, (1, 300), (1, 5), padding=(0, 2), stat_slots=16, edges=("stat16",)))
        a(_c(f"tap-r1-glu-f32z-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 16, 50, (1, 100), (1, 1), glu=True, edges=("glu_f32", "glu_ragged25")))
        a(_c(f"tap-r1-perm-slice-{mode}", "conv", mode, f"gemm_tap_kernel<1, {pm}>", 16, 24, (6, 50), (1, 3), padding=(0, 2), dilation=(1, 2), view="perm+slice",
             edges=("noncontig_in", "out_slice")))
    # 16-bit stores (bf16 mode): lean (full tile), paired generic (ragged rows), unpaired (odd OB); GLU with a 16-bit z lean / generic
    a(_c("st16-lean", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 32, (1, 256), (1, 3), padding=(0, 1), out16=True, stat_slots=1, edges=("store16_lean", "stat1")))
    a(_c("st16-pair-ragged", "conv", "bf16", "gemm_tap_kernel<2, 2>", 24, 45, (1, 200), (1, 3), padding=(0, 1), out16=True, edges=("store16_pair_generic",)))
    a(_c("st16-odd-ob", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 24, (3, 37), (1, 3), padding=(0, 1), out16=True, edges=("store16_unpaired",)))
    a(_c("st16-lean-slice", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 24, (1, 256), (1, 3), padding=(0, 1), out16=True, view="slice",
         edges=("store16_lean", "out_slice", "partial_tile_dropped")))
    a(_c("st16-pair-ragged-slice", "conv", "bf16", "gemm_tap_kernel<2, 2>", 24, 45, (1, 200), (1, 3), padding=(0, 1), out16=True, view="slice",
         edges=("store16_pair_generic", "out_slice")))
    a(_c("glu16-odd-ob", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 48, (3, 37), (1, 3), padding=(0, 1), glu=True, out16=True, edges=("glu16_unpaired",)))
    a(_c("glu16-lean", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 64, (1, 256), (1, 1), glu=True, out16=True, edges=("glu16_lean",)))
    a(_c("glu16-generic", "conv", "bf16", "gemm_tap_kernel<1, 2>", 16, 50, (1, 100), (1, 3), padding=(0, 1), glu=True, out16=True, edges=("glu16_generic", "glu_ragged25")))
    # 16-bit gathered operand
    for r, m, k in ((1, 24, 3), (2, 48, 5), (3, 96, 7), (4, 128, 7)):
        a(_c(f"in16-r{r}", "conv", "bf16", f"gemm_tap_kernel<{r}, 2, IN16>", 16, m, (1, 200), (1, k), stride=(1, 2), padding=(0, 1), in16=True, view="slice" if r == 1 else "",
             edges=("in16",) + (("out_slice",) if r == 1 else ())))
    # streaming kernels: the launcher's own threshold forces N * ceil(P / 128) >= 4096
    for mode, pm in (("bf16x3", 1), ("bf16", 2)):
        a(_c(f"stream41-{mode}", "conv", mode, f"gemm_tap_stream_kernel<{pm}, 4, 1>", 8, 16, (1, 65536), (1, 1), N=8, view="slice" if mode == "bf16" else "",
             edges=("stream", "partial_tile_dropped") + (("out_slice",) if mode == "bf16" else ())))
        a(_c(f"stream24-{mode}", "conv", mode, f"gemm_tap_stream_kernel<{pm}, 2, 4>", 16, 32, (1, 65536 if mode == "bf16x3" else 65568), (1, 3), padding=(0, 1), N=8,   # (bf16: OB % 128 != 0 keeps the halo kernel away)
             out16=(mode == "bf16"), edges=("stream",) + (("store16_lean",) if mode == "bf16" else ())))
    # halo-tile kernel (bf16 mode), every R x {9, 3 taps} x {fp32, 16-bit operand}
    for r, m in ((1, 20), (2, 48), (3, 96)):
        for in16 in (False, True):
            a(_c(f"halo9-r{r}-{int(in16)}", "conv", "bf16", f"gemm_halo_kernel<{r}, 9, {int(in16)}>", 16 if r == 1 else 40, m, (3, 128), (3, 3), padding=(1, 1),
                 in16=in16, halo=True, view="slice" if (r == 1 and not in16) else "", edges=("halo",) + (("out_slice",) if (r == 1 and not in16) else ())))
            a(_c(f"halo3-r{r}-{int(in16)}", "conv", "bf16", f"gemm_halo_kernel<{r}, 3, {int(in16)}>", 48, m, (1, 256), (1, 3), padding=(0, 2), dilation=(1, 2),
                 in16=in16, halo=True, edges=("halo", "dilation_b")))
    # ---- input gradients: per-phase plans (out_a0 / out_b0 / out_sa / out_sb), merged-phase store
    a(_c("dgrad-phases-2d", "dgrad", "f32", ["gemm_fwd_kernel<1>"] * 4, 12, 45, (40, 30), (7, 5), stride=(2, 2), padding=(3, 2), edges=("out_phase",)))
    a(_c("dgrad-phases-bf16", "dgrad", "bf16", ["gemm_tap_kernel<1, 2>"] * 4, 12, 45, (40, 30), (7, 5), stride=(2, 2), padding=(3, 2), edges=("out_phase",)))
    a(_c("dgrad-s1-res", "dgrad", "bf16x3", "gemm_tap_kernel<1, 1>", 24, 33, (17, 23), (3, 3), padding=(1, 1), res=True, edges=("res",)))
    for off in (0, 2, 3, 5):                                       # mg_off = -padding: the G = 4 16-byte path, first and last quads partial
        a(_c(f"dgrad-mg4-off{off}-res", "dgrad", "bf16", "gemm_tap_kernel<1, 2>", 16, 24, (1, 47 + off), (1, 8), stride=(1, 4), padding=(0, off), res=True,
             edges=("mg", "mg4", "mg4_16B", "mg4_res", f"mg_off-{off}")))
    a(_c("dgrad-mg4-nores", "dgrad", "bf16x3", "gemm_tap_kernel<2, 1>", 16, 40, (1, 47), (1, 8), stride=(1, 4), padding=(0, 2), edges=("mg", "mg4", "mg4_16B", "mg_off-2")))
    a(_c("dgrad-mg4-f32", "dgrad", "f32", "gemm_fwd_kernel<1>", 16, 24, (1, 49), (1, 8), stride=(1, 4), padding=(0, 3), res=True, edges=("mg", "mg4", "mg4_16B", "mg4_res", "mg_off-3")))
    a(_c("dgrad-mg2-axis-a", "dgrad", "bf16", "gemm_tap_kernel<1, 2>", 10, 12, (45, 3), (4, 1), stride=(2, 1), padding=(1, 0), res=True, edges=("mg", "mg2", "mg_axis_a")))
    a(_c("dgrad-mg8-axis-b", "dgrad", "bf16x3", "gemm_tap_kernel<1, 1>", 6, 16, (3, 85), (1, 16), stride=(1, 8), padding=(0, 5), edges=("mg", "mg8", "mg_axis_b")))
    # ---- transposed forward: merged (bias per channel) and per-phase
    a(_c("convT-mg4-b", "convT", "bf16", "gemm_tap_kernel<3, 2>", 48, 24, (1, 37), (1, 8), stride=(1, 4), crop=((0, 3), (0, 1)), edges=("mg", "mg4", "mg4_16B", "mg_off-3")))
    a(_c("convT-mg4-a", "convT", "bf16x3", "gemm_tap_kernel<3, 1>", 48, 24, (16, 40), (8, 1), stride=(4, 1), crop=((2, 0), (2, 0)), edges=("mg", "mg4", "mg_axis_a")))
    a(_c("convT-mg2", "convT", "f32", "gemm_fwd_kernel<3>", 64, 48, (1, 257), (1, 4), stride=(1, 2), crop=((0, 1), (0, 1)), edges=("mg", "mg2", "mg_axis_b")))
    a(_c("convT-mg8", "convT", "bf16", "gemm_tap_kernel<1, 2>", 16, 5, (3, 21), (1, 16), stride=(1, 8), crop=((0, 5), (0, 2)), edges=("mg", "mg8")))
    a(_c("convT-mg8-a", "convT", "bf16x3", "gemm_tap_kernel<1, 1>", 16, 5, (21, 3), (16, 1), stride=(8, 1), crop=((5, 0), (2, 0)), edges=("mg", "mg8", "mg_axis_a")))
    a(_c("convT-mg-m8-r1", "convT", "bf16", "gemm_tap_kernel<1, 2>", 48, 2, (16, 40), (8, 1), stride=(4, 1), crop=((2, 0), (2, 0)), edges=("mg", "mg4", "mg_m<=8_r1")))
    a(_c("convT-phases", "convT", "bf16", ["gemm_tap_kernel<2, 2>"] * 2, 20, 45, (9, 17), (5, 3), stride=(2, 1), crop=((2, 1), (2, 1)), edges=("out_phase",)))
    # ---- weight gradient
    for mm, m in ((1, 1), (2, 2), (4, 3), (8, 7)):
        a(_c(f"wg-thin{mm}", "wgrad", "bf16" if mm == 2 else "f32", f"gemm_thin_wgrad_kernel<{mm}>", 12, m, (1, 300 if mm < 8 else 9000), (1, 3), padding=(0, 1),
             edges=("splits1",) if mm < 8 else ("splits>1",)))
    for (tm, tk), (cin, m) in (((1, 1), (9, 33)), ((1, 2), (16, 60)), ((2, 1), (9, 65)), ((2, 2), (16, 97))):
        a(_c(f"wg-f32-{tm}{tk}", "wgrad", "f32", f"gemm_wgrad_kernel<{tm}, {tk}>", cin, m, (6, 50), (1, 5), padding=(0, 2), edges=("ragged_M", "ragged_K", "bias_row")))
    a(_c("wg-f32-pruned-set", "wgrad", "f32", "gemm_wgrad_kernel<1, 2>", 24, 40, (1, 96), (3, 3), padding=(1, 1), edges=("taps_pruned",)))
    for mode, pm in (("bf16x3", 1), ("bf16", 2)):
        g16s = (False, True) if mode == "bf16" else (False,)
        for g16 in g16s:
            sfx = ", G16" if g16 else ""
            tag = f"{mode}{'-g16' if g16 else ''}"
            kw = dict(in16=g16)
            # strided plans (SB = 2): the 32-position kernel
            a(_c(f"wg-bf0-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<3, 1, 1, {pm}{sfx}>", 16, 96, (1, 600), (1, 8), stride=(1, 2), padding=(0, 3), edges=("ragged_K", "bias_row"), **kw))
            a(_c(f"wg-bf1-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<1, 2, 1, {pm}{sfx}>", 24, 24, (1, 600), (1, 8), stride=(1, 2), padding=(0, 3), edges=("ragged_M", "ragged_K"), **kw))
            a(_c(f"wg-bf2-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<1, 1, 1, {pm}{sfx}>", 12, 32, (1, 600), (1, 8), stride=(1, 2), padding=(0, 3), unpack="add", **kw))
            a(_c(f"wg-bf3-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<2, 2, 2, {pm}{sfx}>", 16, 128, (1, 600), (1, 8), stride=(1, 2), padding=(0, 3), unpack="add_bias", **kw))
            a(_c(f"wg-bf4-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<2, 1, 2, {pm}{sfx}>", 8, 96, (1, 600), (1, 4), stride=(1, 2), padding=(0, 1), edges=("ragged_K",), **kw))
            a(_c(f"wg-bf5-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<1, 2, 2, {pm}{sfx}>", 16, 48, (1, 600), (1, 8), stride=(1, 2), padding=(0, 3), edges=("ragged_M",), **kw))
            a(_c(f"wg-bf6-{tag}", "wgrad", mode, f"gemm_wgrad_bf_kernel<1, 1, 2, {pm}{sfx}>", 8, 40, (1, 600), (1, 4), stride=(1, 2), padding=(0, 1), edges=("ragged_M", "ragged_K"), **kw))
            # unit-stride plans: the wide-load kernel
            a(_c(f"wg-wide0-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<3, 1, 1, {pm}{sfx}>", 16, 96, (1, 2048), (1, 3), padding=(0, 1), edges=("xcd", "splits>=8", "bias_row"), unpack="add_bias", **kw))
            a(_c(f"wg-wide1-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<1, 2, 1, {pm}{sfx}>", 48, 12, (1, 860), (1, 3), padding=(0, 2), dilation=(1, 2), N=3,
                 edges=("OB%64", "ragged_M", "ragged_K", "last_split_short"), **kw))
            a(_c(f"wg-wide2-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<1, 1, 1, {pm}{sfx}>", 20, 32, (6, 52), (1, 3), padding=(0, 1), edges=("OA>1", "OB%64"), unpack="add_bias", **kw))
            a(_c(f"wg-wide3-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<2, 2, 2, {pm}{sfx}>", 16, 128, (1, 700), (1, 3), padding=(0, 1), edges=("OB%64",), unpack="add", **kw))
            a(_c(f"wg-wide4-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<1, 2, 2, {pm}{sfx}>", 16, 48, (1, 2048), (1, 3), padding=(0, 1), wsplits=4,
                 edges=("splits_capped", "ragged_M"), **kw))
            if mode == "bf16":
                a(_c(f"wg-wide5-{tag}", "wgrad", mode, f"gemm_wgrad_wide_kernel<3, 2, 1, {pm}{sfx}>", 96, 96, (1, 512), (1, 3), padding=(0, 1), edges=("ragged_K",), **kw))
        # OA > 1 with OB % 4 != 0: the wide kernel refuses, the 32-position kernel runs
        a(_c(f"wg-refusal-{mode}", "wgrad", mode, f"gemm_wgrad_bf_kernel<1, 2, 2, {pm}>", 24, 33, (17, 23), (3, 3), padding=(1, 1), edges=("wide_refused_OB%4",)))
        a(_c(f"wg-pruned-{mode}", "wgrad", mode, f"gemm_wgrad_wide_kernel<1, 2, 2, {pm}>", 24, 40, (1, 96), (3, 3), padding=(1, 1), edges=("taps_pruned", "splits1")))
    # a G16 plan neither 16-bit path takes (odd sample stride): ops.gemm_wgrad widens the gradient and retries
    a(_c("wg-g16-refused", "wgrad", "bf16", ("refused", "gemm_wgrad_bf_kernel<1, 1, 2, 2>"), 8, 33, (1, 75), (1, 4), stride=(1, 2), padding=(0, 1), in16=True,
         edges=("g16_refused",)))
    ids = [c.id for c in T]
    assert len(set(ids)) == len(ids)
    return T
