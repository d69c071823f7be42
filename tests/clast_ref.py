"""Plain torch, CPU reference of the channels-last bf16 trunk: csrc/cl_conv.h (rfx_cl_conv), cl_wgrad.hip (rfx_cl_wgrad +
rfx_cl_wgrad_reduce), cl_elem.hip and the host side remfx_amd/clast.py.

REFERENCE.  float64 F.conv2d / F.conv_transpose2d (the 1-D layers as (1, 8) kernels) and torch's conv weight gradient on the bf16
values of the operands: a product of two bf16 values is exact in fp32, only the fp32 accumulation differs.  Nothing of
ConvForm._build_index / WgradForm._build_map is used: a wrong gather index is a wrong element.  Everything here is channel-major
(N, C, rows, positions); the launch helpers convert at the boundary.

ROUNDING POINTS (read off cl_conv.h's epilogue).  z = bf16(acc + bias).  store + res: bf16(z + res) on the ROUNDED z (the double
rounding of DESIGN 4.16).  gelu: out1 = bf16(gelu(z) + aux0) from the rounded z.  glu: [a | b] = bf16(v) is stored, y = bf16(a
sigmoid(b) + rowadd) from the UNROUNDED fp32 v.  dgelu / dglu: from the rounded (and residual-added, rounded again) gradient.
store_cm: fp32, no rounding.  cl_elem.hip: v and v + res are rounded to bf16 where a stored tensor would have been.

STAGING.  An output computed from a stored tensor is judged from the kernel's own stored tensor (out1 from out0 in gelu / dgelu,
out0 from out1 in dglu, the standalone dglu / dgelu from their inputs).  A rounded value that never leaves the kernel cannot be fed
in: it adds half a bf16 ulp of that value times the derivative of what follows (gelu without out0, dglu without out1, the inner z of
store + res).

BOUND.  Per element |got - ref| <= K eps32 magnitude (+ half a bf16 ulp of the value being rounded per 16-bit store), against the
unrounded fp64 value; K = 8 floor + 8 (k_of).  magnitude = conv(|a|, |b|) + |bias| + |res| pushed through GELU / GLU and
their backward with the derivative weights of 4.15 (cdf = 0.5 + 0.5 |erf|, 1 - sigmoid = 1 + sigmoid).  floor = an fp32 RESTATEMENT
on the CPU against this reference, never a kernel: restate_conv / restate_wgrad / restate_rowsum below; FLOORS holds them."""
import contextlib
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.kernel_harness import GUARD, Arena  # noqa: F401
from tests.ref_common import EPS32, bf16_rne, ulp16, worst  # noqa: F401

SQRT1_2 = 0.7071067811865476


# ---- small helpers ---------------------------------------------------------------------------------------------------------------------
def bf(t):
    """nearest bf16 (ties to even) of the fp32 value of t, widened to fp64"""
    return bf16_rne(t.float()).double()


def bf_trunc(t):
    u = t.float().contiguous().view(torch.int32)
    return (u & -65536).view(torch.float32).double()


def half16(val, t):
    """half a bf16 ulp of the value a kernel rounded: it is within t of val"""
    return 0.5 * ulp16(val.abs() + t)


def cdf(u):
    return 0.5 * (1.0 + torch.erf(u * SQRT1_2))


def cdf_w(u):                      # cdf as fp32 code forms it: 0.5 + 0.5 erf, two terms
    return 0.5 + 0.5 * torch.erf(u * SQRT1_2).abs()


def pdf(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def gelu(u):
    return u * cdf(u)


def dgelu(u):
    return cdf(u) + u * pdf(u)


def dgelu_w(u):
    return cdf_w(u) + u.abs() * pdf(u)


def cl(x_cm):
    """(N, C, A, B) -> channels-last (N, A, B, C)"""
    return x_cm.permute(0, 2, 3, 1).contiguous()


def cm(x_cl):
    return x_cl.permute(0, 3, 1, 2).contiguous()


def fold(t, k=4):
    """channels-last (N, 1, L, C) -> its folded view (N, 1, L / k, k C)"""
    N, A, L, Cc = t.shape
    return t.view(N, A, L // k, k * Cc)


# ---- layer kinds: natural shapes, the fp64 linear map, the shipped form ---------------------------------------------------------------------
# A = rows of the COARSE side (the GEMM's own row count for stride-1 kinds), B = positions of the launch (OB = IB, % 256 == 0)
FOLD_IN = ("s4f", "trfd")
FOLD_OUT = ("s4fd", "trf", "tailb")
IM2COL = ("head", "headb", "taild", "taildb")
MERGED = ("tr", "s4d", "tail")


def shapes(kind, dims, N, A, B):
    """(x shape, y shape, weight shape, (IA, OA, OAo) of the launch), x / y channel-major (N, C, rows, positions)"""
    if kind in ("conv", "glu"):
        Co, Ci, KA, KB = dims
        return (N, Ci, A, B), (N, Co, A, B), (Co, Ci, KA, KB), (A, A, 0)
    if kind == "dgrad":
        Co, Ci, KA, KB = dims
        return (N, Co, A, B), (N, Ci, A, B), (Co, Ci, KA, KB), (A, A, 0)
    if kind == "dx":
        Cc, H, dil = dims
        HP = -(-H // 16) * 16
        return (N, HP, A, B), (N, Cc, A, B), (H, Cc, 1, 3), (A, A, 0)
    if kind == "s4":
        Co, Ci = dims
        return (N, Ci, 4 * A, B), (N, Co, A, B), (Co, Ci, 8, 1), (4 * A, A, 0)
    if kind == "s4d":
        Co, Ci = dims
        return (N, Co, A, B), (N, Ci, 4 * A, B), (Co, Ci, 8, 1), (A, A + 1, 4 * A)
    if kind in ("tr", "tail"):
        Ci, Co = dims
        return (N, Ci, A, B), (N, Co, 4 * A, B), (Ci, Co, 8, 1), (A, A + 1, 4 * A)
    if kind == "trd":
        Ci, Co = dims
        return (N, Co, 4 * A, B), (N, Ci, A, B), (Ci, Co, 8, 1), (4 * A, A, 0)
    if kind == "s4f":
        Co, Ci = dims
        return (N, Ci, 1, 4 * B), (N, Co, 1, B), (Co, Ci, 1, 8), (1, 1, 0)
    if kind == "s4fd":
        Co, Ci = dims
        return (N, Co, 1, B), (N, Ci, 1, 4 * B), (Co, Ci, 1, 8), (1, 1, 0)
    if kind in ("trf", "tailb"):
        Ci, Co = dims
        return (N, Ci, 1, B), (N, Co, 1, 4 * B), (Ci, Co, 1, 8), (1, 1, 0)
    if kind == "trfd":
        Ci, Co = dims
        return (N, Co, 1, 4 * B), (N, Ci, 1, B), (Ci, Co, 1, 8), (1, 1, 0)
    if kind == "head":
        Co, Cs = dims
        return (N, Cs, 4 * A, B), (N, Co, A, B), (Co, Cs, 8, 1), (A, A, 0)
    if kind == "headb":
        Co, Cs = dims
        return (N, Cs, 1, 4 * B), (N, Co, 1, B), (Co, Cs, 1, 8), (1, 1, 0)
    if kind == "taild":
        Cc, Cs = dims
        return (N, Cs, 4 * A, B), (N, Cc, A, B), (Cc, Cs, 8, 1), (A, A, 0)
    if kind == "taildb":
        Cc, Cs = dims
        return (N, Cs, 1, 4 * B), (N, Cc, 1, B), (Cc, Cs, 1, 8), (1, 1, 0)
    raise KeyError(kind)


def lin(kind, dims, x, w):
    """the layer's linear map in fp64 (no bias), channel-major"""
    if kind in ("conv", "glu"):
        return F.conv2d(x, w, padding=(w.shape[2] // 2, w.shape[3] // 2))
    if kind == "dgrad":
        return F.conv_transpose2d(x, w, padding=(w.shape[2] // 2, w.shape[3] // 2))
    if kind == "dx":
        H, dil = dims[1], dims[2]
        return F.conv_transpose2d(x[:, :H], w, padding=(0, dil), dilation=(1, dil))
    if kind in ("s4", "head"):
        return F.conv2d(x, w, stride=(4, 1), padding=(2, 0))
    if kind in ("s4d", "tr", "tail"):
        return F.conv_transpose2d(x, w, stride=(4, 1), padding=(2, 0))
    if kind in ("trd", "taild"):
        return F.conv2d(x, w, stride=(4, 1), padding=(2, 0))       # weight (Cin, Cout, 8, 1) read as (out = Cin, in = Cout)
    if kind in ("s4f", "headb"):
        return F.conv2d(x, w, stride=(1, 4), padding=(0, 2))
    if kind in ("s4fd", "trf", "tailb"):
        return F.conv_transpose2d(x, w, stride=(1, 4), padding=(0, 2))
    if kind in ("trfd", "taildb"):
        return F.conv2d(x, w, stride=(1, 4), padding=(0, 2))
    raise KeyError(kind)


def build_form(kind, dims):
    """the shipped GEMM form of a kind (remfx_amd.clchain's cache where the trunk builds it there)"""
    from remfx_amd import clast, clchain, cldconv
    if kind == "conv":
        return clast.form_conv(*dims)
    if kind == "dx":
        return cldconv._dx_form(*dims)
    name = {"headb": "head", "taildb": "taild", "tailb": "trf"}.get(kind, kind)
    return clchain.form(name, *dims)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class ConvCase:
    id: str
    form: str                      # the instantiation, as the sources spell it
    kind: str
    dims: tuple
    mode: str
    N: int = 1
    A: int = 1
    B: int = 256
    bias: bool = True
    res: bool = False
    aux: bool = False              # gelu: the skip added to out1
    out0: bool = True              # gelu / glu / dgelu: store the pre-activation / the gradient itself
    out1: bool = False             # dglu: store the summed gradient
    rowadd: bool = False
    xslice: bool = False           # the input is a channel slice of a wider tensor (x_c0 = 8, bs = C + 16)
    oslice: bool = False           # outputs are channel slices of wider buffers
    cm_view: bool = False          # store_cm into a strided fp32 view
    edges: tuple = ()
    seed: int = 0


def conv_name(code):
    """rfx_cl_conv_variant code -> cl_conv_kernel<MODE, RW, NT, WM, NTC, KS, DA, DB, HALO> as csrc/cl_conv.h spells it"""
    if code < 0:
        return "refused"
    mode = ("RFX_CL_STORE", "RFX_CL_GELU", "RFX_CL_GLU", "RFX_CL_DGELU", "RFX_CL_DGLU", "RFX_CL_STORE_CM")[code & 7]
    f = lambda s, w: (code >> s) & ((1 << w) - 1)               # noqa: E731
    return f"cl_conv_kernel<{mode}, {f(3, 2)}, {f(5, 2)}, {f(7, 2)}, {f(9, 2)}, {f(11, 2)}, 2, {f(13, 3)}, {'true' if f(16, 1) else 'false'}>"


def wgrad_name(code):
    """rfx_cl_wgrad_variant code -> (cl_wgrad_kernel<RW, WK, PW>, block order)"""
    if code < 0:
        return "refused", ""
    return f"cl_wgrad_kernel<{code & 3}, {(code >> 2) & 7}, {(code >> 5) & 255}>", "grouped" if (code >> 13) & 1 else "plain"


def _gen(seed):
    return torch.Generator().manual_seed(1000 + seed)


def conv_inputs(case):
    g = _gen(case.seed)
    xs, ys, ws, _ = shapes(case.kind, case.dims, case.N, case.A, case.B)
    inp = {"x": torch.randn(xs, generator=g), "w": torch.randn(ws, generator=g) / (ws[1] * ws[2] * ws[3] / 2) ** 0.5}
    if case.kind not in IM2COL:
        inp["x"] = bf16_rne(inp["x"])
    Cy = ys[1]
    if case.bias:
        inp["bias"] = torch.randn(Cy, generator=g) * 0.1
    ysh = ys if case.mode != "glu" else (ys[0], Cy // 2) + ys[2:]
    if case.res:
        inp["res"] = bf16_rne(torch.randn(ysh, generator=g))
    if case.mode == "gelu" and case.aux:
        inp["aux"] = bf16_rne(torch.randn(ys, generator=g))
    if case.mode == "dgelu":
        inp["aux"] = bf16_rne(torch.randn(ys, generator=g))
    if case.mode == "dglu":
        inp["aux"] = bf16_rne(torch.randn((ys[0], 2 * Cy) + ys[2:], generator=g))
    if case.rowadd:
        inp["rowadd"] = torch.randn(ys[2], Cy // 2, generator=g) * 0.3
    return inp


def out_names(case):
    m = case.mode
    if m == "store":
        return ("out0",)
    if m == "store_cm":
        return ("cm",)
    if m in ("gelu", "dgelu", "glu"):
        return (("out0",) if case.out0 else ()) + ("out1",)
    return (("out1",) if case.out1 else ()) + ("out0",)


# ---- reference + tolerance -----------------------------------------------------------------------------------------------------------------
def conv_linear(case, inp):
    """(v, magnitude): fp64 acc + bias of the bf16 operand values and conv(|x|, |w|) + |bias|"""
    x, w = bf(inp["x"]), bf(inp["w"])
    v = lin(case.kind, case.dims, x, w)
    mag = lin(case.kind, case.dims, x.abs(), w.abs())
    if case.bias:
        b = inp["bias"].double().view(1, -1, 1, 1)
        v, mag = v + b, mag + b.abs()
    return v, mag


def conv_judge(case, inp, got, K, lin_cache=None):
    """{name: dict(val, tol, tol32, q, idx)}: every output of the case against its staged fp64 reference.  got: {name: fp tensor,
    channel-major}; K in units of eps32 magnitude"""
    v, mag = lin_cache if lin_cache is not None else conv_linear(case, inp)
    ke = K * EPS32
    gd = lambda k: got[k].double()                              # noqa: E731
    res = {}

    def put(name, val, tol32, extra=0.0, store16=True):
        t = tol32 + extra
        tol = t + half16(val, t) if store16 else t
        q, i = worst(got[name], val, tol)
        res[name] = dict(val=val, tol=tol, tol32=tol32, pre=t + 0 * tol32, q=q, idx=i)     # pre: everything ahead of the final store's half ulp

    m = case.mode
    if m == "store_cm":
        put("cm", v, ke * mag, store16=False)
        return res
    if m == "glu":
        Ch = v.shape[1] // 2
        if case.out0:
            put("out0", v, ke * mag)
        a, b, ma, mb = v[:, :Ch], v[:, Ch:], mag[:, :Ch], mag[:, Ch:]
        s = torch.sigmoid(b)
        val = a * s
        my = ma * s + a.abs() * s * (1 - s) * mb + a.abs() * s
        if case.rowadd:
            ra = inp["rowadd"].double().t().reshape(1, Ch, -1, 1)
            val, my = val + ra, my + ra.abs()
        put("out1", val, ke * my)
        return res
    # the value the epilogue works on: z = bf16(v), with a residual bf16(z + res)
    t_z = ke * mag
    if case.res:
        r = inp["res"].double()
        gval, t_g32 = v + r, ke * (mag + r.abs())
        inner = t_z + half16(v, t_z)                             # the rounded z never leaves the kernel
        g_extra = inner
    else:
        gval, t_g32, g_extra = v, t_z, 0.0
    g_total = t_g32 + g_extra + half16(gval, t_g32 + g_extra)     # all of it, for what is computed from an unstored g
    if m == "store":
        put("out0", gval, t_g32, g_extra)
        return res
    if m == "gelu":
        aux = inp["aux"].double() if "aux" in inp else None
        if case.out0:
            put("out0", gval, t_g32, g_extra)
            z = gd("out0")
            val, m1, ex = gelu(z), z.abs() * cdf_w(z), 0.0
        else:
            val, m1 = gelu(gval), gval.abs() * cdf_w(gval)
            ex = dgelu(gval).abs() * g_total + 0.4 * g_total ** 2   # sup |gelu''| = 2 pdf(0) = 0.798
        if aux is not None:
            val, m1 = val + aux, m1 + aux.abs()
        put("out1", val, ke * m1, ex)
        return res
    if m == "dgelu":
        aux = inp["aux"].double()
        if case.out0:
            put("out0", gval, t_g32, g_extra)
            g, ex = gd("out0"), 0.0
        else:
            g, ex = gval, dgelu(aux).abs() * g_total
        put("out1", g * dgelu(aux), ke * g.abs() * dgelu_w(aux), ex)
        return res
    # dglu
    zab = inp["aux"].double()
    C = zab.shape[1] // 2
    a, b = zab[:, :C], zab[:, C:]
    s = torch.sigmoid(b)
    if case.out1:
        put("out1", gval, t_g32, g_extra)
        g, gt = gd("out1"), 0.0
    else:
        g, gt = gval, g_total
    val = torch.cat([g * s, g * a * s * (1 - s)], 1)
    m0 = torch.cat([g.abs() * s, (g * a).abs() * s * (1 + s)], 1)
    ex = torch.cat([s * gt, (a * s * (1 - s)).abs() * gt], 1) if case.out1 is False else 0.0
    put("out0", val, ke * m0, ex)
    return res


# ---- the GEMM view of a kind: what the fp32 restatement walks ------------------------------------------------------------------------------------
def gemm_weights(kind, dims, w):
    """Wg (M, NTR, NTC, Cg) fp64: the weight of GEMM row m at row tap r, column tap t, GEMM input channel ch -- stated from the layer's
    own formula, not from ConvForm's index functions"""
    if kind == "conv":
        return w.permute(0, 2, 3, 1).contiguous()
    if kind == "glu":
        Wn = w.permute(0, 2, 3, 1)
        Ch = w.shape[0] // 2
        m = torch.arange(w.shape[0])
        return Wn[(m & 1) * Ch + (m >> 1)].contiguous()
    if kind == "dgrad":
        return w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    if kind == "dx":
        Cc, H, dil = dims
        HP = -(-H // 16) * 16
        Wg = torch.zeros(Cc, 1, 3, HP, dtype=w.dtype)
        Wg[:, 0, :, :H] = w[:, :, 0].flip(2).permute(1, 2, 0)
        return Wg
    if kind in ("s4", "trd"):
        return w.permute(0, 2, 3, 1).contiguous()
    if kind in ("tr", "tail", "s4d"):
        # row (psi, c): output row 4 q + psi - 2 takes kernel tap psi + 4 from input row q - 1 (r = 0) and tap psi from row q (r = 1)
        Cr, Cn = w.shape[0], w.shape[1]                           # reduction channels, channels of a phase
        W = w[:, :, :, 0].reshape(Cr, Cn, 2, 4).flip(2)           # [ch, c, r, psi]
        return W.permute(3, 1, 2, 0).reshape(4 * Cn, 2, 1, Cr).contiguous()
    if kind in ("s4f", "trfd"):
        # folded INPUT: GEMM channel j C + c is position 4 p + j; output position q reads p = q + t - 1: kernel tap 4 (t - 1) + j + 2
        M, Cn = w.shape[0], w.shape[1]
        Wg = torch.zeros(M, 1, 3, 4 * Cn, dtype=w.dtype)
        for t in range(3):
            for j in range(4):
                k = 4 * (t - 1) + j + 2
                if 0 <= k < 8:
                    Wg[:, 0, t, j * Cn:(j + 1) * Cn] = w[:, :, 0, k]
        return Wg
    if kind in ("trf", "tailb", "s4fd"):
        # folded OUTPUT: GEMM row j C + c is fine position 4 q + j, fed by coarse position q + t - 1 through kernel tap j + 6 - 4 t
        Cr, Cn = w.shape[0], w.shape[1]
        Wg = torch.zeros(4 * Cn, 1, 3, Cr, dtype=w.dtype)
        for t in range(3):
            for j in range(4):
                k = j + 6 - 4 * t
                if 0 <= k < 8:
                    Wg[j * Cn:(j + 1) * Cn, 0, t, :] = w[:, :, 0, k].t()
        return Wg
    if kind in IM2COL:
        M, Cs = w.shape[0], w.shape[1]
        wk = w.reshape(M, Cs, 8)
        Wg = torch.zeros(M, 1, 1, 16, dtype=w.dtype)
        for k in range(8):
            Wg[:, 0, 0, k * Cs:(k + 1) * Cs] = wk[:, :, k]
        return Wg
    raise KeyError(kind)


def im2col_ref(x, OA, OB, along_b):
    """rfx_cl_im2col_s4: (N, Cs, IA, IB) fp32 -> channels-last (N, OA, OB, 16) fp64 of bf16 values: channel k Cs + c = tap k of channel c"""
    N, Cs, IA, IB = x.shape
    xb = bf(x)
    out = torch.zeros(N, OA, OB, 16, dtype=torch.float64)
    xp = F.pad(xb, (2, 6, 0, 0)) if along_b else F.pad(xb, (0, 0, 2, 6))
    for k in range(8):
        for c in range(Cs):
            if along_b:
                out[..., k * Cs + c] = xp[:, c, :OA, k:k + 4 * OB:4][:, :, :OB]
            else:
                out[..., k * Cs + c] = xp[:, c, k:k + 4 * OA:4, :OB][:, :OA]
    return out


def gemm_input(case, x):
    """the channels-last operand the kernel reads, (N, IA, IB, Cg) fp64"""
    if case.kind in IM2COL:
        _, _, _, (IA, OA, _) = shapes(case.kind, case.dims, case.N, case.A, case.B)
        return im2col_ref(x, OA, case.B, case.kind.endswith("b"))
    xc = cl(bf(x))
    return fold(xc) if case.kind in FOLD_IN else xc


def gemm_to_natural(case, form, acc, extra_rows=0):
    """GEMM rows (N, M, OA, B) -> the layer's own (N, C, rows, positions)"""
    N, M, OA, B = acc.shape
    if case.kind == "glu":
        Ch = M // 2
        m = torch.arange(M)
        out = torch.empty_like(acc)
        out[:, (m & 1) * Ch + (m >> 1)] = acc
        return out
    if case.kind in MERGED:
        Co = M // 4
        t = acc.reshape(N, 4, Co, OA, B).permute(0, 2, 3, 1, 4).reshape(N, Co, 4 * OA, B)
        return t[:, :, 2:2 + 4 * (OA - 1) + extra_rows].contiguous()
    if case.kind in FOLD_OUT:
        Co = M // 4
        return acc.reshape(N, 4, Co, OA, B).permute(0, 2, 3, 4, 1).reshape(N, Co, OA, 4 * B).contiguous()
    return acc


CONV_MUTATIONS = (
    "halo_zero_interior",          # a halo read as zero across an interior tile boundary
    "halo_nonzero_row_end",        # at a row's ends the halo holds the row's other end instead of zeros
    "row_tap_dropped_first",       # the first valid row tap missing at the first output row
    "row_tap_dropped_last",        # the last valid row tap missing at the last output row
    "merged_phase_off_by_one",     # merged rows stored one output row late
    "bias_by_gemm_row",            # bias indexed by GEMM row in interleaved / merged forms
    "rowadd_wrong_row",            # the frequency embedding of the next row
    "ragged_rows_from_neighbour",  # the last 8 rows of a ragged tile computed with the weights 8 rows up
    "last_ptile_skipped",          # the last position tile never written (count no multiple of 8)
    "res_twice_one_row",           # the residual added twice on row 0
    "truncation",                  # 16-bit stores truncate
    "one_ulp",                     # one element of every 16-bit output one bf16 ulp off
    "row_past_oao",                # merged forms: output row OAo is stored too (out0 comes back with OAo + 1 rows; store_guarded places it)
)


def restate_conv(case, inp, form, mutate=None):
    """fp32 restatement of cl_conv_kernel + its epilogue -> {name: channel-major tensor} as the kernel would store them.  One MFMA sums
    its 16 products exactly and rounds once into the fp32 accumulator; MFMAs in the kernel's unit order: valid row taps r_lo .. r_hi,
    chunks of 16 KS channels, then the NTC x KS fragments of the unit."""
    w = bf(inp["w"])
    Wg = gemm_weights(case.kind, case.dims, w)
    xg = gemm_input(case, inp["x"])
    N, IA, IB, Cg = xg.shape
    _, ysh, _, (IA_, OA, OAo) = shapes(case.kind, case.dims, case.N, case.A, case.B)
    assert IA == IA_ and IB == case.B and Cg == form.NCH * 16 * form.KS, (xg.shape, IA_, form.NCH, form.KS)
    M = form.M
    assert Wg.shape == (M, form.NTR, form.NTC, Cg), (Wg.shape, M, form.NTR, form.NTC, Cg)
    if mutate == "ragged_rows_from_neighbour":
        Wg = Wg.clone()
        Wg[M - 8:] = Wg[M - 16:M - 8]
    B = case.B
    acc = torch.zeros(N, M, OA, B, dtype=torch.float32)

    def shifted(row, d):                                         # row (N, B, 16) at positions b + d, zeros outside the row
        if d == 0:
            return row
        out = torch.zeros_like(row)
        if d > 0:
            out[:, :B - d] = row[:, d:]
            if mutate == "halo_nonzero_row_end":
                out[:, B - d:] = row[:, :d]
        else:
            out[:, -d:] = row[:, :B + d]
            if mutate == "halo_nonzero_row_end":
                out[:, :-d] = row[:, B + d:]
        if mutate == "halo_zero_interior":
            b = torch.arange(B)
            lost = ((b % 256 + d < 0) | (b % 256 + d >= 256)) & (b + d >= 0) & (b + d < B)
            out[:, lost] = 0
        return out

    for oa in range(OA):
        base = oa * form.SA + form.da0
        taps = [r for r in range(form.NTR) if 0 <= base + r * form.da_step < IA]
        if taps:
            taps = list(range(taps[0], taps[-1] + 1))
        if mutate == "row_tap_dropped_first" and oa == 0:
            taps = taps[1:]
        if mutate == "row_tap_dropped_last" and oa == OA - 1:
            taps = taps[:-1]
        a32 = acc[:, :, oa]
        for r in taps:
            ia = base + r * form.da_step
            for c in range(form.NCH):
                for t in range(form.NTC):
                    for ks in range(form.KS):
                        ch0 = c * 16 * form.KS + 16 * ks
                        xs = shifted(xg[:, ia, :, ch0:ch0 + 16], form.db0 + t * form.db_step)
                        part = torch.einsum("mk,nbk->nmb", Wg[:, r, t, ch0:ch0 + 16], xs)
                        a32 = (a32.double() + part).float()
        acc[:, :, oa] = a32
    # ---- epilogue in fp32, GEMM-row space first (bias), then natural
    f32 = torch.float32
    if case.bias:
        bv = inp["bias"].float()
        Co = form.Co if form.Co < M else M
        m = torch.arange(M)
        if mutate == "bias_by_gemm_row":
            bi = m.clamp_max(bv.numel() - 1)
        elif case.kind == "glu":
            bi = (m & 1) * (M // 2) + (m >> 1)
        else:
            bi = m % Co
        acc = acc + bv[bi].view(1, M, 1, 1)
    nat = gemm_to_natural(case, form, acc, extra_rows=int(mutate == "row_past_oao"))
    if mutate == "merged_phase_off_by_one":
        nat = torch.roll(nat, 1, 2)
    rnd = (lambda t: bf_trunc(t).float()) if mutate == "truncation" else (lambda t: bf16_rne(t.float()))
    out = {}
    md = case.mode
    if md == "store_cm":
        out["cm"] = nat
    elif md == "glu":
        Ch = nat.shape[1] // 2
        if case.out0:
            out["out0"] = rnd(nat)
        y = nat[:, :Ch] * torch.sigmoid(nat[:, Ch:])
        if case.rowadd:
            ra = inp["rowadd"].float().t().reshape(1, Ch, -1, 1)
            if mutate == "rowadd_wrong_row":
                ra = torch.roll(ra, -1, 2)
            y = y + ra
        out["out1"] = rnd(y)
    else:
        g = rnd(nat)
        if case.res:
            r = inp["res"].float()
            g2 = g + r
            if mutate == "res_twice_one_row":
                g2[:, :, 0] += r[:, :, 0]
            g = rnd(g2)
        if md == "store":
            out["out0"] = g
        elif md == "gelu":
            if case.out0:
                out["out0"] = g
            y = F.gelu(g)
            if "aux" in inp:
                y = y + inp["aux"].float()
            out["out1"] = rnd(y)
        elif md == "dgelu":
            if case.out0:
                out["out0"] = g
            out["out1"] = rnd(g * dgelu(inp["aux"].double()).float())
        else:
            zab = inp["aux"].float()
            C = zab.shape[1] // 2
            s = torch.sigmoid(zab[:, C:])
            if case.out1:
                out["out1"] = g
            out["out0"] = torch.cat([rnd(g * s), rnd(g * zab[:, :C] * s * (1.0 - s))], 1)
    if mutate == "last_ptile_skipped":
        for k in out:
            out[k] = out[k].clone()
            out[k][-1, :, -1, -256 * (4 if case.kind in FOLD_OUT else 1):] = 0.0
    if mutate == "one_ulp":
        for k in out:
            if k != "cm":
                flat = out[k].clone().reshape(-1)
                i = int(flat.abs().argmax())
                flat[i] = flat[i] + ulp16(flat[i].double()).float()
                out[k] = flat.view(out[k].shape)
    return {k: t.to(f32) for k, t in out.items()}


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class WgradCase:
    id: str
    form: str                      # cl_wgrad_kernel<RW, WK, PW>
    order: str                     # "plain" | "grouped" block order (S >= 8)
    kind: str
    dims: tuple
    N: int = 1
    A: int = 1
    B: int = 256
    splits: int = 256              # clast.CLW_SPLITS for the launch
    S: int = 1                     # the split count the launch must come out at
    accumulate: bool = False
    db: bool = True                # kinds that carry the bias column
    pslice: bool = False
    qslice: bool = False
    ahead: int = 0                 # expected prefetch distance of the form (0: not asserted)
    edges: tuple = ()
    seed: int = 0


def wshapes(kind, dims, N, A, B):
    """(P shape, Q shape, weight shape, (OA, IA) of the launch), channel-major naturals; P = rows of D, Q = columns"""
    if kind == "w":
        Co, Ci, KA, KB = dims
        return (N, Co, A, B), (N, Ci, A, B), (Co, Ci, KA, KB), (A, A)
    if kind == "ws4":
        Co, Ci = dims
        return (N, Co, A, B), (N, Ci, 4 * A, B), (Co, Ci, 8, 1), (A, 4 * A)
    if kind == "wtr":
        Ci, Co = dims
        return (N, Ci, A, B), (N, Co, 4 * A, B), (Ci, Co, 8, 1), (A, 4 * A)
    if kind == "ws4f":
        Co, Ci = dims
        return (N, Co, 1, B), (N, Ci, 1, 4 * B), (Co, Ci, 1, 8), (1, 1)
    if kind == "wtrf":
        Ci, Co = dims
        return (N, Ci, 1, B), (N, Co, 1, 4 * B), (Ci, Co, 1, 8), (1, 1)
    if kind == "whead":
        Co, Cs = dims
        return (N, Co, A, B), (N, Cs, 4 * A, B), (Co, Cs, 8, 1), (A, A)
    if kind == "wtail":
        Cc, Cs = dims
        return (N, Cc, A, B), (N, Cs, 4 * A, B), (Cc, Cs, 8, 1), (A, A)
    if kind == "wheadb":                                           # the time branch: one waveform channel, taps along the positions
        Co, Cs = dims
        return (N, Co, 1, B), (N, Cs, 1, 4 * B), (Co, Cs, 1, 8), (1, 1)
    if kind == "wtailb":
        Cc, Cs = dims
        return (N, Cc, 1, B), (N, Cs, 1, 4 * B), (Cc, Cs, 1, 8), (1, 1)
    if kind == "wdc1":                                             # DConv: dW1 of the (dilated) 3-tap convolution, H x C x 3
        H, Cc, dil = dims
        return (N, H, A, B), (N, Cc, A, B), (H, Cc, 1, 3), (A, A)
    raise KeyError(kind)


W_BIAS = {"w": True, "ws4": True, "wtr": False, "ws4f": True, "wtrf": False, "whead": True, "wtail": False, "wheadb": True, "wtailb": False,
          "wdc1": True}
W_IM2COL = ("whead", "wtail", "wheadb", "wtailb")


def build_wform(kind, dims):
    from remfx_amd import clast, clchain
    if kind == "wdc1":
        H, Cc, dil = dims
        key = ("test_wdc1",) + tuple(dims)
        f = clchain._FORMS.get(key)
        if f is None:                                              # cldconv._wforms' first form, with the bias column
            f = clast.WgradForm(H, Cc, 1, 3, 1, 0, -dil, dil, lambda m, r, t, c: (m * Cc + c) * 3 + t, H * Cc * 3)
            clchain._FORMS[key] = f
        return f
    return clchain.form({"wheadb": "whead", "wtailb": "wtail"}.get(kind, kind), *dims)


def wgrad_linear(kind, dims, p, q):
    """(dw, db) in fp64 by torch's own convolution weight gradient, p = D rows operand, q = D columns operand (channel-major fp64)"""
    _, _, ws, _ = wshapes(kind, dims, p.shape[0], 1, 256)
    w = torch.zeros(ws, dtype=torch.float64, requires_grad=True)
    if kind in ("w", "wdc1"):
        dil = dims[2] if kind == "wdc1" else 1
        y = F.conv2d(q, w, padding=(ws[2] // 2, (ws[3] // 2) * dil), dilation=(1, dil))
        y.backward(p)
    elif kind in ("ws4", "whead"):
        F.conv2d(q, w, stride=(4, 1), padding=(2, 0)).backward(p)
    elif kind in ("wtr", "wtail"):
        F.conv_transpose2d(p, w, stride=(4, 1), padding=(2, 0)).backward(q)
    elif kind in ("ws4f", "wheadb"):
        F.conv2d(q, w, stride=(1, 4), padding=(0, 2)).backward(p)
    elif kind in ("wtrf", "wtailb"):
        F.conv_transpose2d(p, w, stride=(1, 4), padding=(0, 2)).backward(q)
    else:
        raise KeyError(kind)
    return w.grad.detach(), p.sum((0, 2, 3))


def wgrad_inputs(case):
    g = _gen(500 + case.seed)
    ps, qs, ws, _ = wshapes(case.kind, case.dims, case.N, case.A, case.B)
    inp = {"p": bf16_rne(torch.randn(ps, generator=g)), "q": torch.randn(qs, generator=g)}
    if case.kind not in W_IM2COL:
        inp["q"] = bf16_rne(inp["q"])
    if case.accumulate:
        inp["dw0"] = torch.randn(ws, generator=g) * 4.0
        inp["db0"] = torch.randn(ps[1], generator=g) * 4.0
    return inp


def wgrad_judge(case, inp, got, K):
    p, q = inp["p"].double(), bf(inp["q"])
    dw, db = wgrad_linear(case.kind, case.dims, p, q)
    mw, mb = wgrad_linear(case.kind, case.dims, p.abs(), q.abs())
    if case.accumulate:
        dw, mw = dw + inp["dw0"].double(), mw + inp["dw0"].double().abs()
        db, mb = db + inp["db0"].double(), mb + inp["db0"].double().abs()
    res = {}
    for name, val, mag in (("dw", dw, mw),) + ((("db", db, mb),) if W_BIAS[case.kind] and case.db else ()):
        tol = K[name] * EPS32 * mag
        qq, i = worst(got[name], val, tol)
        res[name] = dict(val=val, tol=tol, tol32=tol, q=qq, idx=i)
    return res


def wgemm_operands(case, inp):
    """(P (N, OA, B, M), Q (N, IA, B, Cq)) channels-last fp64 as the kernel reads them"""
    k = case.kind
    p, q = cl(inp["p"].double()), inp["q"]
    if k in W_IM2COL:
        _, _, _, (OA, IA) = wshapes(k, case.dims, case.N, case.A, case.B)
        return p, im2col_ref(q, OA, case.B, k.endswith("b"))
    q = cl(bf(q))
    return p, (fold(q) if k in ("ws4f", "wtrf") else q)


def wgemm_to_weight(case, D):
    """D (M, NTR, NTC, Cq) -> the weight tensor's own layout"""
    k = case.kind
    if k in ("w", "wdc1"):
        return D.permute(0, 3, 1, 2).contiguous()
    if k in ("ws4", "wtr"):
        return D.permute(0, 3, 1, 2).contiguous()
    if k in W_IM2COL:
        M, Cs = D.shape[0], case.dims[1]
        w = D[:, 0, 0, :8 * Cs].reshape(M, 8, Cs).permute(0, 2, 1)
        return (w.reshape(M, Cs, 1, 8) if k.endswith("b") else w.reshape(M, Cs, 8, 1)).contiguous()
    # folded Q: column (t, j C + c) is kernel tap 4 (t - 1) + j + 2 of channel c
    M, Cn = D.shape[0], D.shape[3] // 4
    w = torch.zeros(M, Cn, 1, 8, dtype=D.dtype)
    for t in range(3):
        for j in range(4):
            kk = 4 * (t - 1) + j + 2
            if 0 <= kk < 8:
                w[:, :, 0, kk] = D[:, 0, t, j * Cn:(j + 1) * Cn]
    return w


WGRAD_MUTATIONS = (
    "step_dropped",                # one step of a multi-step split missing
    "sample_boundary_stale",       # the step after a sample boundary reads the previous sample
    "ring_row_early",              # one row tap consumed one step early (the Q row of the previous step)
    "source_missing",              # one of the S x WK sources left out of the reduction
    "bias_from_q_column",          # the bias column fed from a Q column instead of ones
    "col_tap_off_by_one",          # one column tap displaced by one position
    "ragged_cq_from_neighbour",    # the last Cq channels of a ragged tile read from the channels one group down
    "rowsum_last_sample",          # (rowsum) the last sample missing
)


def restate_wgrad(case, inp, form, S, PW, mutate=None):
    """fp32 restatement of cl_wgrad_kernel + cl_wgrad_reduce_kernel: positions in groups of 16 (one MFMA, summed exactly, rounded once);
    the K waves of a step take ks = kq, kq + WK, ...; steps in order inside a split; then the S WK sources as the reduction adds them
    (four groups of consecutive sources, each in order, ((g0 + g1) + g2) + g3); accumulate is one more add."""
    P, Q = wgemm_operands(case, inp)
    N, OA, B, M = P.shape
    IA, Cq = Q.shape[1], Q.shape[3]
    NTR, NTC, SA, da0, db0, dbs, WK = form.NTR, form.NTC, form.SA, form.da0, form.db0, form.db_step, form.WK
    nbq = B // PW
    total = N * nbq * OA
    sps = -(-total // S)
    assert -(-total // sps) == S
    ncol = NTR * NTC * Cq + 1
    hb = max(abs(db0 + t * dbs) for t in range(NTC))
    Qp = F.pad(Q, (0, 0, hb, hb))                                   # zero columns outside the row
    srcs = []
    for s in range(S):
        acc = torch.zeros(WK, M, ncol, dtype=torch.float32)
        steps = list(range(s * sps, min((s + 1) * sps, total)))
        if mutate == "step_dropped" and s == S // 2 and len(steps) > 1:
            steps = steps[:1] + steps[2:]
        for si, tau in enumerate(steps):
            col, oa = divmod(tau, OA)
            n, bq = divmod(col, nbq)
            nq = n
            if mutate == "sample_boundary_stale" and n > 0 and bq == 0 and oa == 0:
                nq = n - 1
            b0 = bq * PW
            cols = []
            for r in range(NTR):
                ia = oa * SA + da0 + r
                if mutate == "ring_row_early" and r == NTR - 1 and tau == total // 2:
                    ia -= SA
                for t in range(NTC):
                    d = db0 + t * dbs
                    if mutate == "col_tap_off_by_one" and t == NTC - 1:
                        d -= 1
                    if 0 <= ia < IA:
                        qq = Qp[nq, ia, hb + b0 + d:hb + b0 + d + PW]
                    else:
                        qq = torch.zeros(PW, Cq, dtype=torch.float64)
                    if mutate == "ragged_cq_from_neighbour" and Cq > 8:
                        qq = qq.clone()
                        qq[:, Cq - 8:] = qq[:, Cq - 16:Cq - 8]
                    cols.append(qq)
            ones = torch.ones(PW, 1, dtype=torch.float64)
            if mutate == "bias_from_q_column":
                ones = cols[0][:, :1]
            qcat = torch.cat(cols + [ones], 1)                       # (PW, ncol)
            pp = P[n, oa, b0:b0 + PW]                                # (PW, M)
            part = torch.einsum("gkm,gkc->gmc", pp.reshape(PW // 16, 16, M), qcat.reshape(PW // 16, 16, ncol))
            for ksi in range((PW // 16) // WK):
                acc = (acc.double() + part[ksi * WK:(ksi + 1) * WK]).float()
        srcs += [acc[k] for k in range(WK)]
    if mutate == "source_missing":
        srcs[len(srcs) // 2] = torch.zeros_like(srcs[0])
    nsrc = len(srcs)
    per = -(-nsrc // 4)
    groups = []
    for sg in range(4):
        tot = torch.zeros(M, ncol, dtype=torch.float32)
        for i in range(sg * per, min((sg + 1) * per, nsrc)):
            tot = tot + srcs[i]
        groups.append(tot)
    tot = ((groups[0] + groups[1]) + groups[2]) + groups[3]
    D = tot[:, :-1].reshape(M, NTR, NTC, Cq)
    dw, db = wgemm_to_weight(case, D), tot[:, -1].clone()
    if case.accumulate:
        dw, db = inp["dw0"].float() + dw, inp["db0"].float() + db
    out = {"dw": dw.float()}
    if W_BIAS[case.kind] and case.db:
        out["db"] = db.float()
    return out


# ---- cl_elem.hip ---------------------------------------------------------------------------------------------------------------------------------
def from_cm_judge(mode, x, res, aux, got, K):
    """rfx_cl_from_cm: x (N, C, A, B) fp32 / bf16 values, res (N, C, A, B) bf16 values, aux per mode; got channel-major.  -> (q, idx)"""
    ke = K * EPS32
    v = bf(x)
    if res is not None:
        r = res.double()
        val, t32 = v + r, ke * (v.abs() + r.abs())
        gt = t32 + half16(val, t32)
    else:
        val, t32, gt = v, torch.zeros_like(v), torch.zeros_like(v)
    if mode == "store":
        return worst(got, val, gt)
    # the modes work on the ROUNDED sum, which never leaves the kernel: its half ulp times the derivative of what follows
    if mode == "gelu":
        o, m, ex = gelu(val), val.abs() * cdf_w(val), dgelu(val).abs() * gt + 0.4 * gt ** 2
    elif mode == "dgelu":
        z = aux.double()
        o, m, ex = val * dgelu(z), val.abs() * dgelu_w(z), dgelu(z).abs() * gt
    else:
        z = aux.double()
        C = z.shape[1] // 2
        a, s = z[:, :C], torch.sigmoid(z[:, C:])
        o = torch.cat([val * s, val * a * s * (1 - s)], 1)
        m = torch.cat([val.abs() * s, (val * a).abs() * s * (1 + s)], 1)
        ex = torch.cat([s * gt, (a * s * (1 - s)).abs() * gt], 1)
    t = ke * m + ex
    return worst(got, o, t + half16(o, t))


def restate_rowsum(x, A, G, scale, acc0=None, mutate=None):
    """rfx_cl_rowsum in fp32: x (N, XA, B, C) channels-last values (A == 1: rows folded into N).  Stage 1: thread (pl, grp) walks the
    samples n = g, g + G, ... and positions pl, pl + PT, ... in order; the PT lanes are added in order; stage 2: lane l adds partials
    l, l + 64, ..., then rfx_wave_sum's butterfly (xor 32, 16, ..., 1)."""
    N, XA, B, C = x.shape
    if A == 1 and XA != 1:
        x = x.reshape(N * XA, 1, B, C)
        N = N * XA
    if mutate == "rowsum_last_sample":
        x = x[:N - 1]
        N -= 1
    PT = 256 // (C // 8)
    x = x.float()
    part = torch.zeros(G, A, C, dtype=torch.float32)
    for g in range(G):
        lanes = torch.zeros(PT, A, C, dtype=torch.float32)
        for n in range(g, N, G):
            for b0 in range(0, B, PT):
                blk = x[n, :, b0:b0 + PT].permute(1, 0, 2)          # (<= PT, A, C)
                lanes[:blk.shape[0]] += blk
        s = torch.zeros(A, C, dtype=torch.float32)
        for ql in range(PT):
            s = s + lanes[ql]
        part[g] = s
    lane = torch.zeros(64, A, C, dtype=torch.float32)
    for g in range(G):
        lane[g % 64] += part[g]
    w = 32
    while w:
        lane = lane[:w] + lane[w:2 * w]
        w //= 2
    s = lane[0] * torch.tensor(scale, dtype=torch.float32)
    return s if acc0 is None else acc0.float() + s


# ---- floors measured on the CPU over the case tables (tests/test_clast_ref_cpu.py::test_floors holds them to the measurement), per class the
# largest over its cases and outputs, rounded up to the next 0.25; K = 8 floor + 8
FLOORS = {
    "store": 0.25, "gelu": 1.0, "glu": 0.25, "dgelu": 0.25, "dglu": 0.5, "store_cm": 0.75,
    "dw": 0.75, "db": 0.25, "rowsum": 0.25, "elem": 0.25,
}


def k_of(floor):
    """the bound in units of eps32 * magnitude: 8 x floor + 16 fp32 half-ulps"""
    return 8.0 * floor + 8.0


def K_conv(case):
    return k_of(FLOORS[case.mode])


def K_wgrad():
    return {"dw": k_of(FLOORS["dw"]), "db": k_of(FLOORS["db"])}


def floor_of(entry, got, store16):
    """floor of one output judged at K = 1 (entry from conv_judge / wgrad_judge): the largest |got - val| beyond the 16-bit half ulps, in
    units of eps32 magnitude"""
    e = (got.double() - entry["val"]).abs()
    if store16:
        e = (e - (entry["tol"] - entry["tol32"])).clamp_min(0)
    return float((e / entry["tol32"].clamp_min(1e-300)).max())


# ---- the old assertions, for the planted-fault table ------------------------------------------------------------------------------------------
def old_close(got, ref, ulps=2.0, mag=None):
    """tests/test_gpu_clast.py::_close: True where it accepts"""
    ref, got = ref.double(), got.double()
    scale = (ref.abs() if mag is None else mag.double()).clamp_min(float(ref.abs().mean()) * 1e-2 + 1e-30)
    err = (got - ref).abs() / scale
    rms = float(((got - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt().clamp_min(1e-30))
    return float(err.max()) < ulps * 7.9e-3 and rms < 3.5e-3


def old_wclose(got, ref):
    """tests/test_gpu_clast.py::_wclose"""
    ref, got = ref.double(), got.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    rms = float(((got - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())
    return err < 2e-4 and rms < 2e-5


def rel_rms(got, ref):
    return float(((got.double() - ref.double()) ** 2).mean().sqrt() / (ref.double() ** 2).mean().sqrt().clamp_min(1e-30))


# ---- the shipped launch path, on the GPU or dry (host selection only) --------------------------------------------------------------------------
class _Proxy:
    """libremfx_hip with every launch a no-op; the host-only functions stay the library's own"""
    HOST = ("rfx_cl_conv_variant", "rfx_cl_wgrad_variant", "rfx_cl_wgrad_ws_floats", "rfx_abi_version")

    def __init__(self, real):
        self.real = real

    def __getattr__(self, name):
        real = getattr(self.real, name)
        return real if name in self.HOST else (lambda *a: 0)


def _cl_tensor_any(t, c0=0):
    from remfx_amd._lib import ClTensor
    ct = ClTensor()
    if t is None:
        return ct
    assert t.dtype == torch.bfloat16 and t.dim() == 4 and t.stride(3) == 1
    ct.p = t.data_ptr()
    ct.ns, ct.as_, ct.bs, ct.c0 = t.stride(0), t.stride(1), t.stride(2), c0
    return ct


@contextlib.contextmanager
def recorder(dry_run, splits=None):
    """remfx_amd.clast with TRACE armed (-> the list of ("conv" | "wgrad", variant code)); dry_run: CPU tensors, nothing is launched --
    forms, descriptors and the launchers' selection are the real ones.  splits: clast.CLW_SPLITS for the duration"""
    from remfx_amd import _lib, clast, ops
    saved = (_lib.lib, ops.raw_stream, clast.cl_tensor, clast.TRACE, clast.CLW_SPLITS)
    clast.TRACE = []
    if splits is not None:
        clast.CLW_SPLITS = splits
    if dry_run:
        proxy = _Proxy(_lib.lib())
        _lib.lib = lambda: proxy
        ops.raw_stream = lambda: 0
        clast.cl_tensor = _cl_tensor_any
    try:
        yield clast.TRACE
    finally:
        _lib.lib, ops.raw_stream, clast.cl_tensor, clast.TRACE, clast.CLW_SPLITS = saved


def store_guarded(out_cm, rows, arena, stray_wins):
    """What the GPU test would fetch had a kernel stored the channel-major result out_cm (N, C, rows [+ stray rows], B) into the test's dense
    guarded channels-last buffer of `rows` rows per sample: a row past the last lands on row 0 of the next sample -- it races with that row's
    own store, `stray_wins` says who comes last -- and, from the last sample, on the guard behind the buffer.  -> the fetched (N, C, rows, B)"""
    N, C, R, B = out_cm.shape
    body = arena.alloc((N, rows, B, C), torch.float32)
    flat = arena.bufs[-1].buf[GUARD:]                                              # body + the guard behind it
    x = cl(out_cm.float())
    for first in ((False, True) if stray_wins else (True, False)):  # pass 1 then pass 2: the later store stays
        for nn in range(N):
            for r in range(R):
                if (r >= rows) != first:
                    continue
                o = (nn * rows + r) * B * C
                seg = x[nn, r].reshape(-1)[:max(0, flat.numel() - o)]
                flat[o:o + seg.numel()] = seg
    return cm(body)


def _cpu_alloc(shape, dtype, fill=None):
    return torch.zeros(shape, dtype=dtype) if fill is None else torch.full(shape, fill, dtype=dtype)


def _b16(t):
    return t.to(torch.bfloat16)


def launch_conv(case, inp, dev="cpu", alloc=_cpu_alloc):
    """One case through clast.pack + clast.conv (inside recorder()).  alloc(shape, dtype) hands out the output buffers (the GPU test:
    NaN-filled between guards).  -> ({name: channel-major fp32 tensor}, [spare-channel views that must keep their fill])"""
    from remfx_amd import clast
    kind = case.kind
    form = build_form(kind, case.dims)
    xs, ys, ws, (IA, OA, OAo) = shapes(kind, case.dims, case.N, case.A, case.B)
    N, B = case.N, case.B
    d = lambda t: t.to(dev)                                      # noqa: E731
    w = d(inp["w"])
    if dev == "cpu":
        ap = torch.zeros(form.idx.size, dtype=torch.bfloat16)
    else:
        ap = clast.pack(form, w)
    # operand
    x_c0 = 0
    if kind in IM2COL:
        xop = clast.im2col_s4(d(inp["x"]), OA, B, kind.endswith("b")) if dev != "cpu" else torch.zeros(N, OA, B, 16, dtype=torch.bfloat16)
    else:
        xc = _b16(cl(inp["x"]))
        if case.xslice:
            wide = torch.full(xc.shape[:3] + (xc.shape[3] + 16,), 3.0, dtype=torch.bfloat16)
            wide[..., 8:8 + xc.shape[3]] = xc
            xop, x_c0 = d(wide), 8
        else:
            xop = d(xc)
            if kind in FOLD_IN:
                xop = fold(xop)
    spare = []

    def obuf(Cc, rows, pos):
        """a channels-last output (N, rows, pos, Cc) -- a channel slice of a wider buffer when the case says so -- and its kernel view"""
        if case.oslice:
            wide = alloc((N, rows, pos, Cc + 16), torch.bfloat16)
            spare.extend([wide[..., :8], wide[..., 8 + Cc:]])
            t = wide[..., 8:8 + Cc]
        else:
            t = alloc((N, rows, pos, Cc), torch.bfloat16)
        return t, (fold(t) if kind in FOLD_OUT else t)

    def opnd(t_cm):
        t = d(_b16(cl(t_cm)))
        return fold(t) if kind in FOLD_OUT else t

    Cy, YA, YB = ys[1], ys[2], ys[3]
    kw = dict(OAo=OAo, x_c0=x_c0)
    if case.bias:
        kw["bias"] = d(inp["bias"])
    if case.rowadd:
        kw["rowadd"] = d(inp["rowadd"]).contiguous()
    if case.res:
        kw["res"] = opnd(inp["res"])
    outs = {}
    md = case.mode
    if md == "store_cm":
        if case.cm_view:
            wide = alloc((N, Cy + 1, YA + 1, YB + 32), torch.float32)
            out = wide[:, :Cy, :YA, :YB]
            spare.extend([wide[:, Cy:], wide[:, :Cy, YA:], wide[:, :Cy, :YA, YB:]])
        else:
            out = alloc((N, Cy, YA, YB), torch.float32)
        clast.conv(form, ap, xop, N, IA, B, OA, "store_cm", cm_out=out, cm_fold=kind in FOLD_OUT, **kw)
        return {"cm": out}, spare
    if md == "glu":
        Ch = Cy // 2
        if case.out0:
            outs["out0"], kw["out0"] = obuf(Cy, YA, YB)
        outs["out1"], kw["out1"] = obuf(Ch, YA, YB)
    elif md == "store":
        outs["out0"], kw["out0"] = obuf(Cy, YA, YB)
    elif md in ("gelu", "dgelu"):
        if case.out0:
            outs["out0"], kw["out0"] = obuf(Cy, YA, YB)
        outs["out1"], kw["out1"] = obuf(Cy, YA, YB)
        if "aux" in inp:
            kw["aux0"] = opnd(inp["aux"])
    else:
        outs["out0"], kw["out0"] = obuf(2 * Cy, YA, YB)
        if case.out1:
            outs["out1"], kw["out1"] = obuf(Cy, YA, YB)
        kw["aux0"] = opnd(inp["aux"])
    clast.conv(form, ap, xop, N, IA, B, OA, md, **kw)
    return {k: t.permute(0, 3, 1, 2) for k, t in outs.items()}, spare


def launch_wgrad(case, inp, dev="cpu", alloc=_cpu_alloc):
    """One case through clast.wgrad (inside recorder(splits=case.splits)) -> {dw, db}"""
    from remfx_amd import clast
    form = build_wform(case.kind, case.dims)
    ps, qs, ws, (OA, IA) = wshapes(case.kind, case.dims, case.N, case.A, case.B)
    N, B = case.N, case.B
    d = lambda t: t.to(dev)                                      # noqa: E731
    pc = _b16(cl(inp["p"]))
    p_c0 = q_c0 = 0
    if case.pslice:
        wide = torch.full(pc.shape[:3] + (pc.shape[3] + 16,), 3.0, dtype=torch.bfloat16)
        wide[..., 8:8 + pc.shape[3]] = pc
        pc, p_c0 = wide, 8
    p = d(pc)
    if case.kind in W_IM2COL:
        q = clast.im2col_s4(d(inp["q"]), OA, B, case.kind.endswith("b")) if dev != "cpu" else torch.zeros(N, OA, B, 16, dtype=torch.bfloat16)
    else:
        qc = _b16(cl(inp["q"]))
        if case.qslice:
            wide = torch.full(qc.shape[:3] + (qc.shape[3] + 16,), 3.0, dtype=torch.bfloat16)
            wide[..., 8:8 + qc.shape[3]] = qc
            qc, q_c0 = wide, 8
        q = d(qc)
        if case.kind in ("ws4f", "wtrf"):
            q = fold(q)
    dw = alloc(ws, torch.float32)
    db = alloc((ps[1],), torch.float32) if form.bias else None
    if case.accumulate:
        dw.copy_(d(inp["dw0"]))
        db.copy_(d(inp["db0"]))
    clast.wgrad(form, p, q, N, OA, IA, B, dw, db, accumulate=case.accumulate, p_c0=p_c0, q_c0=q_c0)
    out = {"dw": dw}
    if form.bias and case.db:
        out["db"] = db
    return out


def host_form(case):
    """the instantiation a case launches, by the launchers' own selection, without a GPU"""
    if isinstance(case, ConvCase):
        with recorder(True) as tr:
            launch_conv(case, conv_inputs(case))
            codes = list(tr)
        assert len(codes) == 1 and codes[0][0] == "conv", codes
        return conv_name(codes[0][1])
    with recorder(True, case.splits) as tr:
        launch_wgrad(case, wgrad_inputs(case))
        codes = list(tr)
    assert len(codes) == 1 and codes[0][0] == "wgrad", codes
    return wgrad_name(codes[0][1])


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------------
_TILE = {32: (1, 1, 1), 64: (2, 1, 1), 96: (3, 1, 1), 192: (3, 2, 2)}


def _kname(mode, bm, taps):
    """taps: "halo" (3 column taps), "ks2", "ks1" """
    rw, nt, wm = _TILE[bm]
    deep = rw * wm >= 6
    ntc, ks, db, halo = {"halo": (3, 1, 4 if deep else 6, "true"), "ks2": (1, 2, 3 if deep else 4, "false"), "ks1": (1, 1, 6, "false")}[taps]
    return f"cl_conv_kernel<RFX_CL_{mode.upper()}, {rw}, {nt}, {wm}, {ntc}, {ks}, 2, {db}, {halo}>"


def _taps_of(kind, dims):
    if kind in ("conv", "glu", "dgrad"):
        if dims[3] == 3:
            return "halo"
        cin = dims[0] if kind == "dgrad" else dims[1]
        return "ks2" if cin % 32 == 0 else "ks1"
    if kind in ("dx", "s4f", "s4fd", "trf", "trfd", "tailb"):
        return "halo"
    if kind in IM2COL:
        return "ks1"
    cin = {"s4": 1, "s4d": 0, "tr": 0, "tail": 0, "trd": 1}[kind]
    return "ks2" if dims[cin] % 32 == 0 else "ks1"


def _rows_of(kind, dims):
    if kind in ("conv", "glu"):
        return dims[0]
    if kind == "dgrad":
        return dims[1]
    if kind == "dx":
        return dims[0]
    return {"s4": dims[0], "s4d": 4 * dims[1], "tr": 4 * dims[1], "tail": 4 * dims[1], "trd": dims[0], "s4f": dims[0], "s4fd": 4 * dims[1],
            "trf": 4 * dims[1], "tailb": 4 * dims[1], "trfd": dims[0], "head": dims[0], "headb": dims[0], "taild": dims[0], "taildb": dims[0]}[kind]


def _bm_of(M):
    """remfx_amd.clast.pick_bm at its default switches, restated"""
    if M > 96:
        return 192 if (M % 192 == 0 or M > 288) else 96
    return 96 if M > 64 else (64 if M > 32 else 32)


# the instantiation of every case outside the mode x tile x tap grid, spelled out (the grid's ids carry theirs: grid-<mode>-bm<BM>-<taps>)
CONV_FORM_OF = {
    "rows-m8": "cl_conv_kernel<RFX_CL_STORE, 1, 1, 1, 1, 1, 2, 6, false>",
    "rows-glu-m16": "cl_conv_kernel<RFX_CL_GLU, 1, 1, 1, 3, 1, 2, 6, true>",
    "rows-groups-96": "cl_conv_kernel<RFX_CL_GELU, 3, 1, 1, 3, 1, 2, 6, true>",
    "rows-groups-192": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "tiles-b512-3x3": "cl_conv_kernel<RFX_CL_GLU, 1, 1, 1, 3, 1, 2, 6, true>",
    "tiles-b768-3x3": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-b512-dil2": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-b768-dil8": "cl_conv_kernel<RFX_CL_STORE, 3, 1, 1, 3, 1, 2, 6, true>",
    "tiles-b512-fold": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-count1": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-count7": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-count8": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-count9": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "tiles-count17": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "taps-3rows-ia1": "cl_conv_kernel<RFX_CL_GLU, 1, 1, 1, 3, 1, 2, 6, true>",
    "taps-3rows-ia2": "cl_conv_kernel<RFX_CL_DGELU, 1, 1, 1, 3, 1, 2, 6, true>",
    "taps-s4-oa1": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 1, 2, 2, 4, false>",
    "taps-trd-oa1": "cl_conv_kernel<RFX_CL_DGLU, 2, 1, 1, 1, 1, 2, 6, false>",
    "taps-tr-ia1": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 1, 2, 2, 4, false>",
    "taps-s4d-ia1": "cl_conv_kernel<RFX_CL_DGLU, 2, 1, 1, 1, 2, 2, 4, false>",
    "taps-tr-ia3": "cl_conv_kernel<RFX_CL_STORE, 3, 1, 1, 1, 2, 2, 4, false>",
    "epi-glu-nobias": "cl_conv_kernel<RFX_CL_GLU, 2, 1, 1, 1, 2, 2, 4, false>",
    "epi-merged-bias": "cl_conv_kernel<RFX_CL_GELU, 3, 1, 1, 1, 1, 2, 6, false>",
    "epi-fold-bias": "cl_conv_kernel<RFX_CL_GELU, 3, 1, 1, 3, 1, 2, 6, true>",
    "epi-rowadd": "cl_conv_kernel<RFX_CL_GLU, 3, 1, 1, 1, 1, 2, 6, false>",
    "epi-dglu-res-out1": "cl_conv_kernel<RFX_CL_DGLU, 3, 1, 1, 1, 2, 2, 4, false>",
    "epi-dgelu-res": "cl_conv_kernel<RFX_CL_DGELU, 1, 1, 1, 3, 1, 2, 6, true>",
    "epi-gelu-noaux-noout0": "cl_conv_kernel<RFX_CL_GELU, 1, 1, 1, 1, 1, 2, 6, false>",
    "epi-cm-fold0-co1": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 1, 1, 2, 6, false>",
    "epi-cm-fold0-co2": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 1, 1, 2, 6, false>",
    "epi-cm-fold1-co1": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 3, 1, 2, 6, true>",
    "epi-cm-fold1-co2": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 3, 1, 2, 6, true>",
    "epi-cm-ks2": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 1, 2, 2, 4, false>",
    "view-xslice": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 1, 2, 2, 4, false>",
    "view-xslice-halo": "cl_conv_kernel<RFX_CL_GLU, 1, 1, 1, 3, 1, 2, 6, true>",
    "view-oslice-gelu": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 1, 2, 2, 4, false>",
    "view-oslice-dglu": "cl_conv_kernel<RFX_CL_DGLU, 1, 1, 1, 1, 1, 2, 6, false>",
    "view-oslice-merged": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 1, 2, 2, 4, false>",
    "net48-enc-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 1, 1, 1, 1, 2, 6, false>",
    "net48-enc-rewrite-dgrad": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 1, 2, 2, 4, false>",
    "net48-dec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net48-dec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 2, 1, 1, 3, 1, 2, 6, true>",
    "net48-tdec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net48-tdec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 2, 1, 1, 3, 1, 2, 6, true>",
    "net48-enc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 1, 1, 1, 1, 2, 6, false>",
    "net48-enc-conv-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net48-tenc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net48-tenc-conv-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 2, 2, 3, 1, 2, 4, true>",
    "net48-dec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net48-dec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 1, 1, 1, 1, 2, 6, false>",
    "net48-tdec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net48-tdec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net96-enc-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net96-enc-rewrite-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 1, 1, 1, 2, 2, 4, false>",
    "net96-dec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net96-dec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net96-tdec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net96-tdec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 1, 1, 3, 1, 2, 6, true>",
    "net96-enc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net96-enc-conv-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net96-tenc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net96-tenc-conv-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 2, 2, 3, 1, 2, 4, true>",
    "net96-dec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net96-dec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net96-tdec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net96-tdec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-enc-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-enc-rewrite-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-dec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-dec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-tdec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-tdec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-enc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-enc-conv-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-tenc-conv": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-tenc-conv-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-dec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-dec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net192-tdec-convtr": "cl_conv_kernel<RFX_CL_GELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net192-tdec-convtr-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net384-enc-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 1, 2, 2, 3, false>",
    "net384-enc-rewrite-dgrad": "cl_conv_kernel<RFX_CL_STORE, 3, 2, 2, 1, 2, 2, 3, false>",
    "net384-dec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net384-dec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net384-tdec-rewrite": "cl_conv_kernel<RFX_CL_GLU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net384-tdec-rewrite-dgelu": "cl_conv_kernel<RFX_CL_DGELU, 3, 2, 2, 3, 1, 2, 4, true>",
    "net-head": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 1, 1, 2, 6, false>",
    "net-thead": "cl_conv_kernel<RFX_CL_GELU, 2, 1, 1, 1, 1, 2, 6, false>",
    "net-tail": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 1, 1, 2, 6, false>",
    "net-ttail": "cl_conv_kernel<RFX_CL_STORE_CM, 1, 1, 1, 3, 1, 2, 6, true>",
    "net-tail-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 2, 1, 1, 1, 1, 2, 6, false>",
    "net-ttail-dgrad": "cl_conv_kernel<RFX_CL_DGLU, 2, 1, 1, 1, 1, 2, 6, false>",
    "net48-dconv-dx": "cl_conv_kernel<RFX_CL_STORE, 2, 1, 1, 3, 1, 2, 6, true>",
    "net96-dconv-dx": "cl_conv_kernel<RFX_CL_STORE, 3, 1, 1, 3, 1, 2, 6, true>",
}

def _cc(id, kind, dims, mode, **kw):
    if id.startswith("grid-"):
        bm = 32 if mode == "store_cm" else _bm_of(_rows_of(kind, dims))
        return ConvCase(id, _kname(mode, bm, _taps_of(kind, dims)), kind, tuple(dims), mode, **kw)
    return ConvCase(id, CONV_FORM_OF[id], kind, tuple(dims), mode, **kw)


def conv_cases():
    T = []
    a = T.append
    # ---- the grid: 5 bf16 modes x 4 tile heights x 3 tap forms.  Rows: ragged last tile (48 on 64, 104 on 96, 296 on 192) and M == BM
    opts = {"store": [dict(), dict(res=True, bias=False)],
            "gelu": [dict(aux=True), dict(out0=False)],
            "glu": [dict(), dict(out0=False, bias=False)],
            "dgelu": [dict(bias=False), dict(bias=False, res=True, out0=False)],
            "dglu": [dict(bias=False, out1=True, res=True), dict(bias=False)]}
    rows = {32: (32, 16), 64: (48, 64), 96: (104, 96), 192: (296, 192)}
    for mode in ("store", "gelu", "glu", "dgelu", "dglu"):
        for bm in (32, 64, 96, 192):
            for ti, taps in enumerate(("halo", "ks2", "ks1")):
                M = rows[bm][(ti + (bm == 64)) % 2]
                if mode == "glu" and M % 16:
                    M = rows[bm][1]
                cin = {"halo": 16, "ks2": 32, "ks1": 48}[taps]
                ka = (3, 3) if taps == "halo" else (1, 1)
                kind = "glu" if mode == "glu" else ("dgrad" if mode in ("dgelu", "dglu") else "conv")
                dims = (cin, M) + ka if kind == "dgrad" else (M, cin) + ka
                o = opts[mode][ti % 2]
                a(_cc(f"grid-{mode}-bm{bm}-{taps}", kind, dims, mode, N=1 + (ti == 0), A=2 if taps == "halo" else 1, seed=len(T),
                      edges=("ragged_rows",) if M % bm else ("M==BM",), **o))
    # ---- rows
    a(_cc("rows-m8", "conv", (8, 16, 1, 1), "store", edges=("M8",)))
    a(_cc("rows-glu-m16", "glu", (16, 16, 3, 3), "glu", A=2, edges=("glu_M16",)))
    a(_cc("rows-groups-96", "conv", (200, 16, 3, 3), "gelu", A=2, aux=True, edges=("row_groups", "ragged_rows")))
    a(_cc("rows-groups-192", "glu", (384, 32, 1, 1), "glu", rowadd=True, A=3, edges=("row_groups", "rowadd_rows")))
    # ---- position tiles: halo across interior tile boundaries, dilation 2 and the limit 8; tile counts 1, 7, 8, 9, 17
    a(_cc("tiles-b512-3x3", "glu", (32, 16, 3, 3), "glu", A=2, B=512, edges=("halo_interior",)))
    a(_cc("tiles-b768-3x3", "dgrad", (16, 48, 3, 3), "store", A=2, B=768, res=True, bias=False, edges=("halo_interior",)))
    a(_cc("tiles-b512-dil2", "dx", (48, 24, 2), "store", A=2, B=512, res=True, bias=False, edges=("halo_interior", "dilation2")))
    a(_cc("tiles-b768-dil8", "dx", (96, 24, 8), "store", A=1, B=768, res=True, bias=False, edges=("halo_interior", "dilation8")))
    a(_cc("tiles-b512-fold", "s4f", (48, 16), "gelu", N=2, B=512, edges=("halo_interior", "folded_in")))
    for cnt, (n, rws, b) in {1: (1, 1, 256), 7: (1, 7, 256), 8: (2, 2, 512), 9: (1, 3, 768), 17: (1, 17, 256)}.items():
        a(_cc(f"tiles-count{cnt}", "conv", (48, 16, 3, 3), "store", N=n, A=rws, B=b, seed=cnt, edges=(f"ptiles{cnt}",)))
    # ---- row taps
    a(_cc("taps-3rows-ia1", "glu", (32, 16, 3, 3), "glu", A=1, edges=("3taps_IA1",)))
    a(_cc("taps-3rows-ia2", "dgrad", (32, 16, 3, 3), "dgelu", A=2, bias=False, edges=("3taps_IA2",)))
    a(_cc("taps-s4-oa1", "s4", (48, 32), "gelu", A=1, edges=("s4_OA1",)))
    a(_cc("taps-trd-oa1", "trd", (48, 16), "dglu", A=1, bias=False, edges=("s4_OA1",)))
    a(_cc("taps-tr-ia1", "tr", (32, 16), "gelu", A=1, aux=True, edges=("merged_IA1",)))
    a(_cc("taps-s4d-ia1", "s4d", (32, 16), "dglu", A=1, bias=False, res=True, out1=True, edges=("merged_IA1",)))
    a(_cc("taps-tr-ia3", "tr", (32, 24), "store", N=2, A=3, edges=("merged",)))
    # ---- epilogue variants
    a(_cc("epi-glu-nobias", "glu", (64, 32, 1, 1), "glu", A=2, bias=False, edges=("bias_absent",)))
    a(_cc("epi-merged-bias", "tr", (48, 24), "gelu", A=2, edges=("bias_merged",)))
    a(_cc("epi-fold-bias", "trf", (48, 24), "gelu", aux=True, edges=("bias_merged", "folded_out")))
    a(_cc("epi-rowadd", "glu", (96, 48, 1, 1), "glu", N=2, A=5, rowadd=True, edges=("rowadd_rows",)))
    a(_cc("epi-dglu-res-out1", "s4d", (64, 32), "dglu", A=2, bias=False, res=True, out1=True, edges=("res_dglu", "out1_dglu")))
    a(_cc("epi-dgelu-res", "dgrad", (64, 32, 3, 3), "dgelu", A=2, bias=False, res=True, edges=("res_dgelu",)))
    a(_cc("epi-gelu-noaux-noout0", "s4", (32, 16), "gelu", A=2, out0=False, edges=("gelu_inference",)))
    for fo in (0, 1):
        for co in (1, 2):
            a(_cc(f"epi-cm-fold{fo}-co{co}", "tailb" if fo else "tail", (48, co), "store_cm", N=2, A=1 if fo else 2, cm_view=bool(co == 2), seed=fo * 2 + co,
                  edges=(f"cm_fold{fo}", f"cm_Co{co}") + (("cm_view",) if co == 2 else ())))
    a(_cc("epi-cm-ks2", "tail", (32, 2), "store_cm", A=1, edges=("cm_fold0",)))
    # ---- strided operands
    a(_cc("view-xslice", "conv", (48, 32, 1, 1), "store", A=2, xslice=True, edges=("x_c0",)))
    a(_cc("view-xslice-halo", "glu", (32, 16, 3, 3), "glu", A=2, B=512, xslice=True, oslice=True, edges=("x_c0", "out_slice", "halo_interior")))
    a(_cc("view-oslice-gelu", "s4", (48, 32), "gelu", A=2, oslice=True, aux=True, edges=("out_slice",)))
    a(_cc("view-oslice-dglu", "trd", (32, 16), "dglu", A=1, bias=False, oslice=True, edges=("out_slice",)))
    a(_cc("view-oslice-merged", "tr", (32, 16), "store", A=2, oslice=True, edges=("out_slice", "merged")))
    # ---- every shipped layer form of the cfg/model/demucs.yaml geometry at its real widths, both branches, head and tail
    for Cw in (48, 96, 192, 384):
        s = Cw
        a(_cc(f"net{Cw}-enc-rewrite", "glu", (2 * Cw, Cw, 1, 1), "glu", A=2, rowadd=(Cw == 48), seed=s, edges=("net",)))
        a(_cc(f"net{Cw}-enc-rewrite-dgrad", "dgrad", (2 * Cw, Cw, 1, 1), "store", A=2, bias=False, seed=s, edges=("net",)))
        a(_cc(f"net{Cw}-dec-rewrite", "glu", (2 * Cw, Cw, 3, 3), "glu", A=2, seed=s, edges=("net",)))
        a(_cc(f"net{Cw}-dec-rewrite-dgelu", "dgrad", (2 * Cw, Cw, 3, 3), "dgelu", A=2, bias=False, seed=s, edges=("net",)))
        a(_cc(f"net{Cw}-tdec-rewrite", "glu", (2 * Cw, Cw, 1, 3), "glu", seed=s, edges=("net", "time")))
        a(_cc(f"net{Cw}-tdec-rewrite-dgelu", "dgrad", (2 * Cw, Cw, 1, 3), "dgelu", bias=False, seed=s, edges=("net", "time")))
        if Cw < 384:
            a(_cc(f"net{Cw}-enc-conv", "s4", (2 * Cw, Cw), "gelu", A=1, seed=s, edges=("net",)))
            a(_cc(f"net{Cw}-enc-conv-dgrad", "s4d", (2 * Cw, Cw), "dglu", A=1, bias=False, res=True, out1=(Cw == 48), seed=s, edges=("net",)))
            a(_cc(f"net{Cw}-tenc-conv", "s4f", (2 * Cw, Cw), "gelu", seed=s, edges=("net", "time")))
            a(_cc(f"net{Cw}-tenc-conv-dgrad", "s4fd", (2 * Cw, Cw), "store", bias=False, res=True, seed=s, edges=("net", "time")))
            a(_cc(f"net{Cw}-dec-convtr", "tr", (2 * Cw, Cw), "gelu", A=1, aux=True, seed=s, edges=("net",)))
            a(_cc(f"net{Cw}-dec-convtr-dgrad", "trd", (2 * Cw, Cw), "dglu", A=1, bias=False, seed=s, edges=("net",)))
            a(_cc(f"net{Cw}-tdec-convtr", "trf", (2 * Cw, Cw), "gelu", aux=True, seed=s, edges=("net", "time")))
            a(_cc(f"net{Cw}-tdec-convtr-dgrad", "trfd", (2 * Cw, Cw), "dglu", bias=False, seed=s, edges=("net", "time")))
    a(_cc("net-head", "head", (48, 2), "gelu", A=2, edges=("net", "head")))
    a(_cc("net-thead", "headb", (48, 1), "gelu", edges=("net", "head", "time")))
    a(_cc("net-tail", "tail", (48, 2), "store_cm", A=2, seed=7, edges=("net", "tail")))
    a(_cc("net-ttail", "tailb", (48, 1), "store_cm", seed=8, edges=("net", "tail", "time")))
    a(_cc("net-tail-dgrad", "taild", (48, 2), "dglu", A=2, bias=False, edges=("net", "tail")))
    a(_cc("net-ttail-dgrad", "taildb", (48, 1), "dglu", bias=False, edges=("net", "tail", "time")))
    for Cw in (48, 96):
        a(_cc(f"net{Cw}-dconv-dx", "dx", (Cw, Cw // 4, 1), "store", A=2, bias=False, res=True, seed=Cw, edges=("net",)))
    ids = [c.id for c in T]
    assert len(set(ids)) == len(ids)
    return T


def _wc(id, form, order, kind, dims, **kw):
    return WgradCase(id, form, order, kind, tuple(dims), **kw)


def wgrad_cases():
    T = []
    a = T.append
    K = "cl_wgrad_kernel"
    # ---- all 12 instantiations; PW = 64 through B % 128 != 0 (B = 192)
    a(_wc("wg-214-128", f"{K}<2, 4, 128>", "plain", "w", (40, 24, 1, 1), N=2, A=3, splits=6, S=6, edges=("ragged_M40", "ragged_Cq24")))
    a(_wc("wg-214-64", f"{K}<2, 4, 64>", "plain", "w", (40, 24, 1, 1), N=1, A=2, B=192, S=6, edges=("PW64",)))
    a(_wc("wg-22-128", f"{K}<2, 2, 128>", "plain", "w", (48, 16, 3, 3), N=1, A=3, S=6, ahead=4, edges=("3x3", "PRE2", "ahead4")))
    a(_wc("wg-22-64", f"{K}<2, 2, 64>", "plain", "w", (48, 16, 3, 3), N=1, A=2, B=192, S=6, edges=("PW64", "PRE2")))
    a(_wc("wg-21-128", f"{K}<2, 1, 128>", "grouped", "w", (64, 48, 3, 3), N=2, A=2, S=8, ahead=3, edges=("S8", "grouped", "ahead3")))
    a(_wc("wg-21-64", f"{K}<2, 1, 64>", "plain", "w", (64, 48, 3, 3), N=1, A=2, B=192, S=6, edges=("PW64",)))
    a(_wc("wg-34-128", f"{K}<3, 4, 128>", "plain", "w", (104, 40, 1, 1), N=1, A=2, S=4, edges=("ragged_M104", "ragged_Cq40")))
    a(_wc("wg-34-64", f"{K}<3, 4, 64>", "plain", "w", (96, 16, 1, 1), N=1, A=1, B=192, S=3, edges=("PW64", "S3")))
    a(_wc("wg-32-128", f"{K}<3, 2, 128>", "plain", "w", (96, 16, 3, 3), N=1, A=2, S=4, edges=("3x3",)))
    a(_wc("wg-32-64", f"{K}<3, 2, 64>", "plain", "w", (96, 16, 3, 3), N=1, A=2, B=192, S=6, edges=("PW64",)))
    a(_wc("wg-31-128", f"{K}<3, 1, 128>", "plain", "w", (96, 48, 3, 3), N=1, A=2, S=4, ahead=2, edges=("3x3", "ahead2")))
    a(_wc("wg-31-64", f"{K}<3, 1, 64>", "plain", "w", (96, 48, 3, 3), N=1, A=2, B=192, S=6, edges=("PW64",)))
    # ---- splits through clast.CLW_SPLITS
    a(_wc("wg-s1", f"{K}<2, 2, 128>", "plain", "w", (48, 16, 3, 3), N=2, A=3, splits=1, S=1, edges=("S1", "multi_step", "sample_boundary", "column_boundary", "PRE2")))
    a(_wc("wg-s3", f"{K}<2, 2, 128>", "plain", "w", (48, 16, 3, 3), N=2, A=3, splits=3, S=3, edges=("S3", "multi_step", "sample_boundary")))
    a(_wc("wg-s8", f"{K}<2, 2, 128>", "grouped", "w", (48, 16, 3, 3), N=2, A=4, splits=8, S=8, edges=("S8", "grouped", "multi_step")))
    a(_wc("wg-s11-short", f"{K}<2, 2, 128>", "grouped", "w", (48, 16, 3, 3), N=3, A=7, splits=12, S=11, edges=("S>8", "spx2", "last_split_short")))
    a(_wc("wg-s4-steps", f"{K}<2, 2, 128>", "plain", "ws4", (48, 16), N=2, A=3, B=512, splits=3, S=3, edges=("multi_step", "stride4", "PRE1", "sample_boundary")))
    a(_wc("wg-tr-s1", f"{K}<2, 4, 128>", "plain", "wtr", (32, 16), N=2, A=2, splits=1, S=1, db=False, edges=("stride4", "PRE1", "no_bias_column")))
    # ---- bias column, dilation, slices, accumulate, folded forms
    a(_wc("wg-dil2", f"{K}<2, 2, 128>", "plain", "wdc1", (24, 48, 2), N=1, A=2, B=512, splits=2, S=2, edges=("dilation2", "ragged_M24")))
    a(_wc("wg-dil8", f"{K}<2, 2, 128>", "plain", "wdc1", (24, 48, 8), N=1, A=2, B=256, splits=1, S=1, edges=("dilation8",)))
    a(_wc("wg-slices-acc", f"{K}<2, 2, 128>", "plain", "w", (48, 16, 3, 3), N=2, A=2, splits=3, S=3, pslice=True, qslice=True, accumulate=True,
          edges=("p_c0", "q_c0", "accumulate")))
    a(_wc("wg-fold-s4", f"{K}<2, 2, 128>", "plain", "ws4f", (48, 16), N=2, B=512, splits=3, S=3, edges=("folded", "structural_zeros")))
    a(_wc("wg-fold-tr", f"{K}<2, 2, 128>", "plain", "wtrf", (32, 16), N=2, B=256, splits=2, S=2, db=False, edges=("folded", "structural_zeros")))
    a(_wc("wg-head", f"{K}<2, 4, 128>", "plain", "whead", (48, 2), N=1, A=2, S=4, edges=("net", "head")))
    a(_wc("wg-tail", f"{K}<2, 4, 128>", "plain", "wtail", (48, 2), N=1, A=2, S=4, db=False, edges=("net", "tail")))
    # ---- shipped widths
    for Cw in (48, 96, 192):
        a(_wc(f"wg-net{Cw}-rewrite3", f"{K}<3, 1, 128>", "plain", "w", (2 * Cw, Cw, 3, 3), N=1, A=2, S=4, seed=Cw, edges=("net",)))
        a(_wc(f"wg-net{Cw}-rewrite1", f"{K}<3, 4, 128>", "plain", "w", (2 * Cw, Cw, 1, 1), N=1, A=2, S=4, seed=Cw, edges=("net",)))
        a(_wc(f"wg-net{Cw}-s4", f"{K}<3, 1, 64>", "plain", "ws4", (2 * Cw, Cw), N=1, A=1, S=4, seed=Cw, edges=("net",)))
        a(_wc(f"wg-net{Cw}-tr", f"{K}<3, 1, 64>", "plain", "wtr", (2 * Cw, Cw), N=1, A=1, S=4, db=False, ahead=1 if Cw == 192 else 2, seed=Cw,
              edges=("net",) + (("ahead1",) if Cw == 192 else ())))
    # ---- the rest of the shipped forms: 384-wide rewrites, the time branch's 1 x 3 rewrites, folded stride-4 layers, head and tail
    a(_wc("wg-net384-rewrite3", f"{K}<3, 1, 128>", "plain", "w", (768, 384, 3, 3), N=1, A=2, splits=64, S=1, seed=384, edges=("net", "multi_step", "D_tiles64")))
    a(_wc("wg-net384-rewrite1", f"{K}<3, 4, 128>", "plain", "w", (768, 384, 1, 1), N=1, A=2, S=4, seed=384, edges=("net",)))
    for Cw, form, S in ((48, f"{K}<3, 2, 128>", 8), (96, f"{K}<3, 1, 64>", 16), (192, f"{K}<3, 1, 64>", 16), (384, f"{K}<3, 1, 64>", 8)):
        a(_wc(f"wg-net{Cw}-trewrite", form, "grouped", "w", (2 * Cw, Cw, 1, 3), N=2, A=1, B=512, S=S, seed=Cw + 1,
              edges=("net", "time") + (("multi_step",) if Cw == 384 else ())))
    for Cw in (48, 96, 192):
        a(_wc(f"wg-net{Cw}-s4f", f"{K}<3, 1, 64>", "grouped", "ws4f", (2 * Cw, Cw), N=2, B=256, S=8, seed=Cw + 2, edges=("net", "time", "folded")))
        a(_wc(f"wg-net{Cw}-trf", f"{K}<3, 1, 64>", "grouped", "wtrf", (2 * Cw, Cw), N=2, B=256, S=8, db=False, seed=Cw + 2, edges=("net", "time", "folded")))
    a(_wc("wg-thead", f"{K}<2, 4, 128>", "grouped", "wheadb", (48, 1), N=2, B=512, S=8, edges=("net", "head", "time")))
    a(_wc("wg-ttail", f"{K}<2, 4, 128>", "grouped", "wtailb", (48, 1), N=2, B=512, S=8, db=False, edges=("net", "tail", "time")))
    ids = [c.id for c in T]
    assert len(set(ids)) == len(ids)
    return T
