"""Plain torch, CPU restatement of ONE fused channels-last DConv layer (remfx_amd/csrc/cl_dconv.hip through remfx_amd/cldconv.py:
layer_forward / layer_backward), forward and closed-form backward, no autograd in the tested path.

x: (N, L, C) channels-last samples, L = TPS * 256, H = C / 4, dil in {1, 2}:
    h = conv1d(x; W1 (H, C, 3), b1, dilation d, padding d)       over the whole sample: taps cross tile edges, zeros at its ends
    a = GELU_erf(GN(1, H)(h));  z = W2 a + b2;  y = x + scale * GLU(GN(1, 2C)(z))      value = channels 0..C-1, gate = C..2C-1

Two arithmetics run the same formulas (class Exact: fp64, plain sums; class Kern32: float32 with the kernels' partial sums).  Both round
to bf16 exactly where the kernels do (ROUNDING below) unless `rounding=False`.

ROUNDING POINTS (read off cl_dconv.hip).  Forward: x, W1, W2 bf16 operands; h fp32; hpre = bf16(h); statistics 1 from the UNROUNDED h;
a = bf16(GELU(..)) is GEMM2's operand and what is stored; z fp32; statistics 2 from z; y = bf16(..).  Backward (all forms): z is
recomputed from the stored a, hhat from the stored hpre, with the saved fp32 stats; d(zhat) gamma2 is PARKED as bf16 and the two sample
means of GroupNorm-2's backward are taken over the parked values; dz = bf16(..) is stored and is da's operand.  One-pass forms
(cl_dconv_bwd8_kernel, cl_dconv_bwd_kernel): d(hhat) gamma1 stays fp32, dh = bf16(..), dx = bf16(gy + conv^T(dh)).  Pass form
(cl_dconv_bwdp_kernel<.,.,1|2>, cl_dconv_means_kernel, cl_dconv_dh_kernel): d(hhat) gamma1 is parked as bf16 too, its means are over
the parked values, dh = bf16(..) in place, dx on cl_conv, whose epilogue stages the tile as bf16 BEFORE it adds the residual:
dx = bf16(gy + bf16(conv^T(dh))) -- a second rounding the one-pass forms do not have (found by this suite).  Weight gradients: fp32 from the bf16 dz / a and dh / x.

STAGING (judge_forward / judge_backward): an output is compared with the reference of ITS stage, fed what the tested code itself
produced one stage earlier, so a one-ulp flip of an intermediate is not charged to what follows.  Every bf16-stored output is judged
against the UNROUNDED fp64 value at K eps32 magnitude + half a bf16 ulp of the value being rounded (+ the parked rounding, weighted
by rstd, for dz and the pass form's dh, and the staged convolution's for the pass form's dx: those values never leave the kernels, so
they cannot be fed in).

BOUND.  K = 8 floor + 8 (k_of) in units of eps32 magnitude, as tests/norm_ref.py; magnitude = sum of |terms| an element is formed
from, each weighted by the derivative it enters with; floor = Kern32 against Exact in those units, per case class and output
(floors(); never measured on the kernel).  `mutate`: a deliberately wrong Kern32 (MUTATIONS; tests/test_cldconv_ref_cpu.py)."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.ref_common import EPS32, bf16_rne, bf16_trunc, gelu_cdf, gelu_pdf, ulp, worst  # noqa: F401

T = 256
GEN_EPS = 1e-5
TINY = 2.0 ** -120                # the clamped exp2 keeps sigmoid >= 2^-126 and bf16 stores may flush subnormals: absolute, far below any value here
BF16_STORED = ("hpre", "a", "y", "dz", "dh", "dx")
SMALL = ("dscale", "dgn2w", "dgn2b", "dgn1w", "dgn1b")

MUTATIONS = (
    "tap_missing_tile_edge",      # tap 0 missing at the first, tap 2 at the last position of an interior tile (a wrong halo row)
    "halo_from_previous_sample",  # at a sample's two ends the halo rows hold the previous sample of the walk instead of zeros
    "stale_buffer",               # the last sample computed from the image of sample s - grid
    "dil_1_on_one_tap",           # tap 2 reads at distance 1 where dil = 2
    "stats_one_tile",             # sample 0: statistics 1 over its first tile instead of the whole sample
    "scale_from_neighbour",       # one channel's LayerScale from its neighbour
    "glu_swapped",                # value and gate swapped for one channel
    "pad_channel_nonzero",        # hidden channel H (padding) of `a` holds a value at one position
    "dgn1w_missing_workgroup",    # dgn1w without the partial of the last workgroup
    "truncating_store",           # y / dx stored by truncation instead of round-to-nearest-even
    "one_ulp",                    # one element of y / dx off by one bf16 ulp
)


def _half_ulp16(ref, t):
    return 0.5 * ulp(ref.abs() + t, 7)


# ---- the two arithmetics ---------------------------------------------------------------------------------------------------------------
class Exact:
    """fp64, plain sums"""
    dtype = torch.float64

    @staticmethod
    def tile_sums(t):             # (N, L, Cn) -> (N, TPS): one sum per 256-position tile
        N, L, Cn = t.shape
        return t.reshape(N, L // T, T * Cn).sum(-1)

    @staticmethod
    def sample_mean(ts, n):       # (N, TPS) tile sums -> (N,) mean over the n values of a sample
        return ts.sum(1) / n

    @staticmethod
    def finalize(s1, s2, n, eps):
        raise NotImplementedError  # Exact takes the two-pass variance (stats())

    @staticmethod
    def small(t, grid, drop_last_wg=False):   # (N, L, Cn) -> (Cn,): a parameter-gradient sum over every position
        return t.reshape(-1, t.shape[-1]).sum(0)


def _wave32(t):
    """(..., 32 positions, Cn) fp32 -> (...,): one wave's sum -- lane (position, half) adds its registers in order, then rfx_wave_sum's
    butterfly over the 64 lanes"""
    Cn = t.shape[-1]
    hw = -(-Cn // 2)
    t = F.pad(t, (0, 2 * hw - Cn)).reshape(*t.shape[:-1], 2, hw)
    acc = t[..., 0].clone()
    for i in range(1, hw):
        acc = acc + t[..., i]
    acc = acc.reshape(*acc.shape[:-2], 64)
    w = 32
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


class Kern32:
    """float32 with fp32 partial sums in the kernels' decomposition: per lane, rfx_wave_sum, the eight waves of a tile in order, tile
    sums finalised in fp64 where a sample has several tiles, per-workgroup partials added in workgroup order for the small gradients"""
    dtype = torch.float32

    @staticmethod
    def tile_sums(t):
        N, L, Cn = t.shape
        w = _wave32(t.reshape(N, L // T, 8, 32, Cn))            # (N, TPS, 8)
        acc = w[..., 0].clone()
        for i in range(1, 8):
            acc = acc + w[..., i]
        return acc

    @staticmethod
    def sample_mean(ts, n):
        if ts.shape[1] == 1:
            return ts[:, 0] * torch.tensor(1.0 / n, dtype=torch.float32)
        return (ts.double().sum(1) * (1.0 / n)).float()         # cl_dconv_stats_kernel / cl_dconv_means_kernel

    @staticmethod
    def finalize(s1, s2, n, eps):
        if s1.shape[1] == 1:                                     # PH = 0: in the kernel, fp32
            inv = torch.tensor(1.0 / n, dtype=torch.float32)
            mu = s1[:, 0] * inv
            return mu, torch.rsqrt((s2[:, 0] * inv - mu * mu).clamp_min(0) + torch.tensor(eps, dtype=torch.float32))
        a, b = s1.double().sum(1), s2.double().sum(1)
        mu = a / n
        return mu.float(), (1.0 / torch.sqrt((b / n - mu * mu).clamp_min(0) + float(torch.tensor(eps, dtype=torch.float32)))).float()

    @staticmethod
    def small(t, grid, drop_last_wg=False):
        N, L, Cn = t.shape
        S = N * L // T
        tl = t.reshape(S, 8, 32, Cn)
        w = tl[:, :, 0].clone()                                  # a lane = a channel: it adds its 32 positions (16 registers, two halves)
        for i in range(1, 32):
            w = w + tl[:, :, i]
        G = min(grid, S)
        parts = []
        for g in range(G):                                       # workgroup g walks tiles g, g + G, ...: the accumulators run on across them
            acc = torch.zeros(8, Cn, dtype=torch.float32)
            for s in range(g, S, G):
                acc = acc + w[s]
            p = acc[0].clone()
            for i in range(1, 8):
                p = p + acc[i]
            parts.append(p)
        if drop_last_wg:
            parts = parts[:-1]
        out = parts[0].clone()
        for p in parts[1:]:                                      # cl_dconv_pgrad_kernel (G <= 64: one partial per lane, then the butterfly)
            out = out + p
        return out


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------
def _conv(x, W, dil, taps=(0, 1, 2), dil_of_tap=None):
    """sum over taps t of x(pos + (t - 1) d) W[:, :, t]^T, zeros beyond the sample's ends: (N, L, C) -> (N, L, H)"""
    L = x.shape[1]
    xp = F.pad(x, (0, 0, 2, 2))
    out = 0
    for t in taps:
        d = dil if dil_of_tap is None else dil_of_tap[t]
        o = 2 + (t - 1) * d
        out = out + xp[:, o:o + L] @ W[:, :, t].transpose(0, 1)
    return out


def _conv_t(dh, W, dil):
    """dx - gy: sum over taps of dh(pos - (t - 1) d) W[:, :, t]: (N, L, H) -> (N, L, C)"""
    L = dh.shape[1]
    dp = F.pad(dh, (0, 0, 2, 2))
    out = 0
    for t in range(3):
        o = 2 - (t - 1) * dil
        out = out + dp[:, o:o + L] @ W[:, :, t]
    return out


def stats(t, eps=GEN_EPS):
    """fp64 mean, rstd per sample of (N, L, Cn), two-pass variance: the truth, not the algorithm"""
    r = t.double().reshape(t.shape[0], -1)
    m = r.mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    return m, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))


def _stats(t, ar, eps):
    if ar is Exact:
        return stats(t, eps)
    return ar.finalize(ar.tile_sums(t), ar.tile_sums(t * t), t.shape[1] * t.shape[2], eps)


def stat_mag(t, mag_t, eps=GEN_EPS):
    """mean: mean(mag) (absolute).  rstd: relative, 0.5 x the terms of E[t^2] - m^2 over (var + eps), each with its own error"""
    r, g = t.double().reshape(t.shape[0], -1), mag_t.reshape(t.shape[0], -1)
    m = r.mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    num = (2 * r.abs() * g).mean(1) + (r * r).mean(1) + 2 * m.abs() * g.mean(1) + m * m
    return g.mean(1), 0.5 * num / (var + float(torch.tensor(eps, dtype=torch.float32)))


def _b(s):
    return s[:, None, None]


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
def forward(inp, dil, ar=Exact, rounding=True, stats1=None, a_in=None, stats2=None, eps=GEN_EPS, mutate=None, grid=256):
    """every forward quantity in ar.dtype.  stats1 = (mean1, rstd1), a_in, stats2: the tested code's own values (staging).  Returns the
    UNROUNDED h / a_pre / y_pre next to the rounded hpre / a / y, and (Exact) the magnitudes as 'mag:<name>'."""
    c = lambda t: t.to(ar.dtype)                                # noqa: E731
    rnd = bf16_rne if rounding else (lambda t: t)
    x, W1, b1, g1w, g1b, W2, b2, g2w, g2b, sc = (c(inp[k]) for k in ("x", "W1", "b1", "g1w", "g1b", "W2", "b2", "g2w", "g2b", "scale"))
    N, L, Cc = x.shape
    H, TPS = W1.shape[0], L // T
    o = {}
    xs = x
    if mutate == "stale_buffer":
        xs = x.clone()
        xs[N - 1] = x[N - 1 - (min(grid, N) if TPS == 1 else 1)]
    h = _conv(xs, W1, dil, dil_of_tap=(dil, dil, 1) if mutate == "dil_1_on_one_tap" else None) + b1
    if mutate == "tap_missing_tile_edge":
        h = h.clone()
        h[0, T] -= xs[0, T - dil] @ W1[:, :, 0].transpose(0, 1)
        h[0, 2 * T - 1] -= xs[0, 2 * T - 1 + dil] @ W1[:, :, 2].transpose(0, 1)
    if mutate == "halo_from_previous_sample":
        h = h.clone()
        n, p = N - 1, N - 1 - (min(grid, N) if TPS == 1 else 1)
        for q in range(dil):
            h[n, q] += xs[p, L - dil + q] @ W1[:, :, 0].transpose(0, 1)
            h[n, L - dil + q] += xs[p, q] @ W1[:, :, 2].transpose(0, 1)
    o["h"], o["hpre"] = h, rnd(h)
    m1, r1 = _stats(h, ar, eps)
    if mutate == "stats_one_tile":
        mt, rt = _stats(h[:1, :T], ar, eps)
        m1, r1 = m1.clone(), r1.clone()
        m1[0], r1[0] = mt[0], rt[0]
    o["mean1"], o["rstd1"] = m1, r1
    if stats1 is not None:
        m1, r1 = c(stats1[0]), c(stats1[1])
    hh = h * _b(r1) + _b(-m1 * r1)
    u = hh * g1w + g1b
    o["a_pre"] = u * gelu_cdf(u)
    o["a"] = rnd(o["a_pre"])
    a = o["a"] if a_in is None else c(a_in)
    z = a @ W2.transpose(0, 1) + b2
    o["z"] = z
    m2, r2 = _stats(z, ar, eps)
    o["mean2"], o["rstd2"] = m2, r2
    if stats2 is not None:
        m2, r2 = c(stats2[0]), c(stats2[1])
    zh = z * _b(r2) + _b(-m2 * r2)
    gw, gb, s = g2w, g2b, sc
    if mutate == "scale_from_neighbour":
        s = sc.clone()
        s[Cc // 2] = sc[Cc // 2 + 1]
    w = zh * gw + gb
    v, gt = w[..., :Cc], w[..., Cc:]
    if mutate == "glu_swapped":
        v, gt = v.clone(), gt.clone()
        v[..., Cc // 2], gt[..., Cc // 2] = w[..., Cc + Cc // 2], w[..., Cc // 2]
    sg = torch.sigmoid(gt)
    o["y_pre"] = xs + s * (v * sg)
    if mutate == "truncating_store":
        o["y"] = bf16_trunc(o["y_pre"])
    else:
        o["y"] = rnd(o["y_pre"])
    if mutate == "one_ulp":
        o["y"] = o["y"].clone()
        e = o["y"][N - 1, L // 2, Cc // 3]
        o["y"][N - 1, L // 2, Cc // 3] = e + ulp(e.double(), 7).to(ar.dtype)
    if ar is Exact:
        mh = _conv(x.abs(), W1.abs(), dil) + b1.abs()
        o["mag:hpre"] = mh
        o["mag:mean1"], o["mag:rstd1"] = stat_mag(h, mh, eps)
        Au = (mh + _b(m1.abs())) * _b(r1) * g1w.abs() + g1b.abs()
        cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
        o["mag:a"] = Au * (2.0 * cdfm + u.abs() * gelu_pdf(u))
        mz = a.abs() @ W2.abs().transpose(0, 1) + b2.abs()
        o["mag:mean2"], o["mag:rstd2"] = stat_mag(z, mz, eps)
        Az = (mz + _b(m2.abs())) * _b(r2)
        Aw = Az * g2w.abs() + g2b.abs()
        o["mag:y"] = x.abs() + sc.abs() * sg * (Aw[..., :Cc] + v.abs() * (1.0 - sg) * Aw[..., Cc:])
    return o


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def saved_tensors(inp, dil, eps=GEN_EPS):
    """what the forward pass hands to the backward pass, made by the reference: a, hpre (bf16-representable fp64), stats (N, 4) fp32"""
    f = forward(inp, dil, Exact, True, eps=eps)
    st = torch.stack([f["mean1"], f["rstd1"], f["mean2"], f["rstd2"]], 1).float()
    return {"a": f["a"], "hpre": f["hpre"], "stats": st}


def backward(inp, sv, dil, passes, ar=Exact, rounding=True, dz_in=None, dh_in=None, mutate=None, grid=256):
    """every backward quantity in ar.dtype from the saved tensors sv.  passes: the pass form (d(hhat) gamma1 parked as bf16).  dz_in /
    dh_in: the tested code's own dz / dh (staging: dh, dW2, db2 from dz_in; dx, dW1, db1 from dh_in); the five small gradients always
    follow the chain's own dz.  dz_pre / dh_pre / dx_pre are the UNROUNDED stored values; (Exact) magnitudes as 'mag:<name>' and the
    rounding of the parked values, weighted, as 'park:<name>'."""
    c = lambda t: t.to(ar.dtype)                                # noqa: E731
    rnd = bf16_rne if rounding else (lambda t: t)
    x, W1, g1w, g1b, W2, b2, g2w, g2b, sc, gy = (c(inp[k]) for k in ("x", "W1", "g1w", "g1b", "W2", "b2", "g2w", "g2b", "scale", "gy"))
    a, hpre, st = c(sv["a"]), c(sv["hpre"]), c(sv["stats"])
    N, L, Cc = x.shape
    H = W1.shape[0]
    m1, r1, m2, r2 = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    mag = ar is Exact
    o = {}
    z = a @ W2.transpose(0, 1) + b2
    zh = z * _b(r2) + _b(-m2 * r2)
    w = zh * g2w + g2b
    v, gt = w[..., :Cc], w[..., Cc:]
    sg = torch.sigmoid(gt)
    g0 = gy * sc
    dv = g0 * sg
    dgt = (dv * v) * (1.0 - sg)
    du = torch.cat([dv, dgt], -1)
    o["dscale"] = ar.small(gy * (v * sg), grid)
    o["dgn2b"] = ar.small(du, grid)
    o["dgn2w"] = ar.small(du * zh, grid)
    p_pre = du * g2w
    p = rnd(p_pre)
    n2 = L * 2 * Cc
    pm1, pm2 = ar.sample_mean(ar.tile_sums(p), n2), ar.sample_mean(ar.tile_sums(p * zh), n2)
    o["dz_pre"] = _b(r2) * ((p_pre - _b(pm1)) - zh * _b(pm2))
    o["dz"] = rnd(_b(r2) * ((p - _b(pm1)) - zh * _b(pm2)))

    def hidden(dz):
        da = dz @ W2
        hh = hpre * _b(r1) + _b(-m1 * r1)
        u = hh * g1w + g1b
        gp = gelu_cdf(u) + u * gelu_pdf(u)
        dhn = da * gp
        q_pre = dhn * g1w
        q = rnd(q_pre) if passes else q_pre
        n1 = L * H
        qm1, qm2 = ar.sample_mean(ar.tile_sums(q), n1), ar.sample_mean(ar.tile_sums(q * hh), n1)
        r = {"dhn": dhn, "hh": hh, "u": u, "da": da, "q": q, "q_pre": q_pre, "qm2": qm2,
             "dh_pre": _b(r1) * (q_pre - _b(qm1) - hh * _b(qm2)), "dh": rnd(_b(r1) * (q - _b(qm1) - hh * _b(qm2)))}
        return r

    own = hidden(o["dz"])                                        # the chain's own dz: the small gradients
    o["dgn1b"] = ar.small(own["dhn"], grid)
    o["dgn1w"] = ar.small(own["dhn"] * own["hh"], grid, drop_last_wg=mutate == "dgn1w_missing_workgroup")
    dzk = o["dz"] if dz_in is None else c(dz_in)
    hd = own if dz_in is None else hidden(dzk)
    o["dh_pre"], o["dh"] = hd["dh_pre"], hd["dh"]
    dhk = o["dh"] if dh_in is None else c(dh_in)
    cv = _conv_t(dhk, W1, dil)
    o["dx_pre"] = gy + cv
    # pass form: cl_conv's epilogue stages its tile as bf16 and adds the residual to the ROUNDED values: dx = bf16(gy + bf16(conv))
    dxv = gy + rnd(cv) if passes else o["dx_pre"]
    o["dx"] = bf16_trunc(dxv) if mutate == "truncating_store" else rnd(dxv)
    if mutate == "one_ulp":
        o["dx"] = o["dx"].clone()
        e = o["dx"][N - 1, L // 2, Cc // 3]
        o["dx"][N - 1, L // 2, Cc // 3] = e + ulp(e.double(), 7).to(ar.dtype)
    f2 = lambda t: t.reshape(-1, t.shape[-1])                   # noqa: E731
    o["dw2"] = f2(dzk).transpose(0, 1) @ f2(a)
    o["db2"] = f2(dzk).sum(0)
    xp = F.pad(x, (0, 0, 2, 2))
    o["dw1"] = torch.stack([f2(dhk).transpose(0, 1) @ f2(xp[:, 2 + (t - 1) * dil:2 + (t - 1) * dil + L]) for t in range(3)], -1)
    o["db1"] = f2(dhk).sum(0)
    if mag:
        S = lambda t: t.reshape(-1, t.shape[-1]).sum(0)         # noqa: E731
        mz = a.abs() @ W2.abs().transpose(0, 1) + b2.abs()
        Az = (mz + _b(m2.abs())) * _b(r2)
        Aw = Az * g2w.abs() + g2b.abs()
        Av, Ag = Aw[..., :Cc], Aw[..., Cc:]
        o["mag:dscale"] = S(gy.abs() * sg * (Av + v.abs() * (1.0 - sg) * Ag))
        mdu = torch.cat([g0.abs() * sg * (1.0 + (1.0 - sg) * Ag),
                         g0.abs() * sg * ((1.0 - sg) * Av + v.abs() * ((1.0 + sg) + (1.0 - sg) * (1.0 - 2.0 * sg).abs() * Ag))], -1)
        o["mag:dgn2b"] = S(mdu)
        o["mag:dgn2w"] = S(mdu * zh.abs() + du.abs() * Az)
        mp = mdu * g2w.abs()
        M1 = mp.reshape(N, -1).mean(1)
        M2 = (mp * zh.abs() + p.abs() * Az).reshape(N, -1).mean(1)
        o["mag:dz"] = _b(r2) * (mp + _b(M1) + zh.abs() * _b(M2) + Az * _b(pm2.abs()))
        o["park:dz"] = _b(r2) * 0.5 * ulp(p_pre, 7) if rounding else torch.zeros_like(p)

        def hidden_mag(r, dz):
            mda = dz.abs() @ W2.abs()
            hh, u = r["hh"], r["u"]
            Ah = (hpre.abs() + _b(m1.abs())) * _b(r1)
            Au = Ah * g1w.abs() + g1b.abs()
            pdf = gelu_pdf(u)
            cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
            mdhn = mda * (cdfm + u.abs() * pdf) + r["da"].abs() * pdf * (2.0 - u * u).abs() * Au
            mq = mdhn * g1w.abs()
            Q1 = mq.reshape(N, -1).mean(1)
            Q2 = (mq * hh.abs() + r["q"].abs() * Ah).reshape(N, -1).mean(1)
            return (S(mdhn), S(mdhn * hh.abs() + r["dhn"].abs() * Ah),
                    _b(r1) * (mq + _b(Q1) + hh.abs() * _b(Q2) + Ah * _b(r["qm2"].abs())))
        o["mag:dgn1b"], o["mag:dgn1w"], _ = hidden_mag(own, o["dz"])
        _, _, o["mag:dh"] = hidden_mag(hd, dzk)
        o["park:dh"] = _b(r1) * 0.5 * ulp(hd["q_pre"], 7) if (passes and rounding) else torch.zeros_like(hd["q"])
        o["mag:dx"] = gy.abs() + _conv_t(dhk.abs(), W1.abs(), dil)
        if passes and rounding:
            o["park:dx"] = 0.5 * ulp(cv, 7)
        o["mag:dw2"] = f2(dzk.abs()).transpose(0, 1) @ f2(a.abs())
        o["mag:db2"] = f2(dzk.abs()).sum(0)
        xa = xp.abs()
        o["mag:dw1"] = torch.stack([f2(dhk.abs()).transpose(0, 1) @ f2(xa[:, 2 + (t - 1) * dil:2 + (t - 1) * dil + L]) for t in range(3)], -1)
        o["mag:db1"] = f2(dhk.abs()).sum(0)
    return o


# ---- judging -----------------------------------------------------------------------------------------------------------------------------
FWD_OUT = ("hpre", "mean1", "rstd1", "a", "mean2", "rstd2", "y")
BWD_OUT = ("dz", "dh", "dx", "dw2", "db2", "dw1", "db1") + SMALL
_PRE = {"hpre": "h", "a": "a_pre", "y": "y_pre", "dz": "dz_pre", "dh": "dh_pre", "dx": "dx_pre"}


def _tol(name, ref, k):
    """(reference value, absolute tolerance per element) of output `name` from a staged Exact evaluation `ref`"""
    if name.startswith("rstd"):
        return ref[name], k * EPS32 * ref["mag:" + name] * ref[name]
    val = ref[_PRE.get(name, name)]
    t = k * EPS32 * ref["mag:" + name]
    if name in BF16_STORED:
        if "park:" + name in ref:
            t = t + ref["park:" + name]
        t = t + _half_ulp16(val, t) + TINY
    return val, t


def stage_forward(inp, dil, got, eps=GEN_EPS):
    """the staged Exact references of a forward result `got` {hpre, a, stats (N, 4), y}: {name: evaluation to read `name` from}"""
    gd = lambda k: got[k].double()                              # noqa: E731
    st = gd("stats")
    r0 = forward(inp, dil, Exact, True, eps=eps)
    r1 = forward(inp, dil, Exact, True, stats1=(st[:, 0], st[:, 1]), eps=eps)
    r2 = forward(inp, dil, Exact, True, stats1=(st[:, 0], st[:, 1]), a_in=gd("a"), stats2=(st[:, 2], st[:, 3]), eps=eps)
    return {"hpre": r0, "mean1": r0, "rstd1": r0, "a": r1, "mean2": r2, "rstd2": r2, "y": r2}


def stage_backward(inp, sv, dil, passes, got, grid=256):
    gd = lambda k: got[k].double()                              # noqa: E731
    r0 = backward(inp, sv, dil, passes, Exact, True, grid=grid)
    r1 = backward(inp, sv, dil, passes, Exact, True, dz_in=gd("dz"), grid=grid)
    r2 = backward(inp, sv, dil, passes, Exact, True, dz_in=gd("dz"), dh_in=gd("dh"), grid=grid)
    out = {"dz": r0, "dh": r1, "dw2": r1, "db2": r1, "dx": r2, "dw1": r2, "db1": r2}
    out.update({k: r0 for k in SMALL})
    return out


def _got_forward(got):
    g = dict(got)
    st = got["stats"].double()
    g.update(mean1=st[:, 0], rstd1=st[:, 1], mean2=st[:, 2], rstd2=st[:, 3])
    return g


def judge(names, stages, got, K):
    """{name: (error / tolerance of the worst element, its flat index)}; K: {name: K} in units of eps32 magnitude"""
    res = {}
    for n in names:
        val, t = _tol(n, stages[n], K[n])
        res[n] = worst(got[n], val, t)
    return res


def measure(names, stages, got):
    """{name: floor}: the largest |got - ref| beyond the bf16 half-ulps, in units of eps32 magnitude"""
    fl = {}
    for n in names:
        val, t0 = _tol(n, stages[n], 0.0)
        e = ((got[n].double() - val).abs() - t0).clamp_min(0)
        unit = EPS32 * stages[n]["mag:" + n] * (stages[n][n] if n.startswith("rstd") else 1.0)
        fl[n] = float((e / unit.clamp_min(1e-300)).max())
    return fl


def kern32_forward(inp, dil, mutate=None, grid=256, eps=GEN_EPS):
    f = forward(inp, dil, Kern32, True, eps=eps, mutate=mutate, grid=grid)
    f["stats"] = torch.stack([f["mean1"], f["rstd1"], f["mean2"], f["rstd2"]], 1)
    return f


def floors_forward(inp, dil, grid=256):
    got = kern32_forward(inp, dil, grid=grid)
    st = stage_forward(inp, dil, got)
    return measure(FWD_OUT, st, _got_forward(got))


def floors_backward(inp, dil, passes, grid=256):
    sv = saved_tensors(inp, dil)
    got = backward(inp, sv, dil, passes, Kern32, True, grid=grid)
    st = stage_backward(inp, sv, dil, passes, got, grid)
    return measure(BWD_OUT, st, got)


# ---- floors measured on the CPU over the case table (tests/test_cldconv_ref_cpu.py::test_floors holds them to the measurement; DESIGN.md
# 4.16): per case class and output the largest over the class's cases, rounded up to the next 0.25; K = 8 floor + 8
FLOORS = {
    "fwd-tps1": {"hpre": 0.25, "mean1": 0.5, "rstd1": 0.75, "a": 0.25, "mean2": 0.5, "rstd2": 0.75, "y": 0.75},
    "fwd-tiles": {"hpre": 0.25, "mean1": 0.25, "rstd1": 0.25, "a": 0.25, "mean2": 0.25, "rstd2": 0.25, "y": 0.5},
    "fwd-sat": {"hpre": 0.25, "mean1": 0.5, "rstd1": 0.25, "a": 0.25, "mean2": 0.25, "rstd2": 0.5, "y": 0.25},
    "bwd-tps1": {"dz": 4.0, "dh": 0.5, "dx": 0.5, "dw2": 3.75, "db2": 0.25, "dw1": 3.25, "db1": 0.25, "dscale": 0.25, "dgn2w": 0.25,
                 "dgn2b": 0.25, "dgn1w": 17.75, "dgn1b": 16.75},
    "bwd-tps1-pass": {"dz": 2.0, "dh": 3.0, "dx": 0.25, "dw2": 4.0, "db2": 0.25, "dw1": 2.75, "db1": 0.25, "dscale": 0.25, "dgn2w": 0.25,
                      "dgn2b": 0.25, "dgn1w": 4.5, "dgn1b": 4.0},
    "bwd-tiles-pass": {"dz": 1.0, "dh": 0.25, "dx": 0.25, "dw2": 5.5, "db2": 0.25, "dw1": 3.75, "db1": 0.25, "dscale": 0.25, "dgn2w": 0.25,
                       "dgn2b": 0.25, "dgn1w": 7.75, "dgn1b": 6.0},
    "bwd-sat": {"dz": 0.25, "dh": 0.25, "dx": 0.25, "dw2": 38.75, "db2": 0.5, "dw1": 1.5, "db1": 0.25, "dscale": 0.25, "dgn2w": 0.25,
                "dgn2b": 0.25, "dgn1w": 10.0, "dgn1b": 5.75},
}


def k_of(floor):
    """the bound in units of eps32 * magnitude: 8 x floor + 16 fp32 half-ulps"""
    return 8.0 * floor + 8.0


def K_of(case):
    return {n: k_of(f) for n, f in FLOORS[case.klass].items()}


def pad_is_zero(t, H):
    """channels H .. HP-1 of a stored (.., HP) tensor are exact zeros (cl_wgrad and the dx convolution read all HP channels)"""
    return bool((t[..., H:].contiguous().view(torch.int16) == 0).all()) if t.dtype == torch.bfloat16 else bool((t[..., H:] == 0).all())


def old_rel(got, ref):
    """the whole-tensor figure tests/test_gpu_cldconv.py asserts on (< 4e-3 for y / dx, < 5e-3 for a parameter gradient, at e16 = 0)"""
    return float(((got.double() - ref.double()) ** 2).sum().sqrt() / (ref.double() ** 2).sum().sqrt().clamp_min(1e-30))


# ---- the dispatch of rfx_cl_dconv_fwd / rfx_cl_dconv_bwd, restated ----------------------------------------------------------------------
def forms(Cc, TPS, nsamp, grid, bwd, four=False):
    """(launched instantiations, steering quantities) of one layer_forward (bwd False) or layer_backward call"""
    H, S = Cc // 4, nsamp * TPS
    G = min(grid, S)
    walk = -(-S // G)                                            # tiles the busiest workgroup walks
    st = {"G": G, "walk": walk, "odd_walk": walk % 2 == 1, "TPS": TPS}
    if not bwd:
        if TPS == 1:
            return [f"fwd<{Cc},{H},0>"], st
        return [f"fwd<{Cc},{H},1>", "stats", f"fwd<{Cc},{H},2>", f"fwd<{Cc},{H},3>"], st
    if TPS > 1 or Cc != 48:
        return [f"bwdp<{Cc},{H},1>", "means", f"bwdp<{Cc},{H},2>", "dh", "pgrad", "cl_conv:dx", "cl_wgrad"], st
    return [("bwd" if four else "bwd8") + f"<{Cc},{H}>", "pgrad", "cl_wgrad"], st


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    C: int
    dil: int
    TPS: int
    nsamp: int
    grid: int = 0                 # 0: the default (256)
    sat: bool = False             # GroupNorm-2 gate weights large enough to saturate the gates on both sides
    bwd: bool = False
    four: bool = False            # the four-wave one-pass form (a child process)

    @property
    def id(self):
        s = f"C{self.C}-d{self.dil}-tps{self.TPS}-n{self.nsamp}" + (f"-g{self.grid}" if self.grid else "") + ("-sat" if self.sat else "")
        return s + ("-nw4" if self.four else "")

    @property
    def klass(self):
        return ("bwd" if self.bwd else "fwd") + ("-sat" if self.sat else "-tps1" if self.TPS == 1 else "-tiles") + \
            ("-pass" if self.bwd and self.passes and not self.sat else "")

    @property
    def g(self):
        return self.grid or 256

    @property
    def passes(self):
        return self.TPS > 1 or self.C != 48

    def forms(self):
        return forms(self.C, self.TPS, self.nsamp, self.g, self.bwd, self.four)


_SHAPES = ((1, 1, 0), (1, 3, 2), (1, 258, 0), (2, 2, 0), (2, 2, 3), (3, 2, 0), (3, 2, 3))     # (TPS, samples, grid)


def forward_cases():
    t = [Case(C, d, tps, n, g) for C in (48, 96) for d in (1, 2) for (tps, n, g) in _SHAPES]
    return t + [Case(48, 1, 1, 3, 2, sat=True), Case(96, 2, 2, 2, 3, sat=True)]


def backward_cases():
    t = [Case(48, d, 1, n, g, bwd=True) for d in (1, 2) for (tps, n, g) in _SHAPES if tps == 1]
    t += [Case(96, d, tps, n, g, bwd=True) for d in (1, 2) for (tps, n, g) in _SHAPES]
    t += [Case(48, d, tps, n, g, bwd=True) for d in (1, 2) for (tps, n, g) in _SHAPES if tps > 1]
    return t + [Case(48, 1, 1, 3, 2, sat=True, bwd=True), Case(96, 2, 2, 2, 3, sat=True, bwd=True)]


def four_wave_cases():
    t = [Case(48, d, 1, n, g, bwd=True, four=True) for d in (1, 2) for (tps, n, g) in _SHAPES if tps == 1]
    return t + [Case(48, 1, 1, 3, 2, sat=True, bwd=True, four=True)]


def make_inputs(case):
    """fp32 CPU tensors, bf16-representable where the kernel reads bf16 (x, gy, W1, W2).  Every channel's parameters differ from its
    neighbours'.  Every sample carries large values on its first and last 2 dil positions (a halo from the wrong sample or tile, or one
    not zeroed, moves h by many bounds); samples 1 (3 samples) / 7 and 257 (258 samples) are all zero."""
    g = torch.Generator().manual_seed(1000 * case.C + 100 * case.dil + 10 * case.TPS + case.nsamp + 7 * case.grid + 3 * case.sat)
    Cc, H, N, L, d = case.C, case.C // 4, case.nsamp, case.TPS * T, case.dil
    rn = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    sign = lambda n: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()      # noqa: E731
    x = rn(N, L, Cc)
    x[:, :2 * d] *= 6.0
    x[:, L - 2 * d:] *= 6.0
    for z in {3: (1,), 258: (7, 257)}.get(N, ()):
        x[z] = 0
    inp = {"x": bf16_rne(x), "gy": bf16_rne(rn(N, L, Cc)),
           "W1": bf16_rne(rn(H, Cc, 3) / math.sqrt(3 * Cc)), "b1": rn(H) * 0.5,
           "g1w": sign(H) * (0.6 + 0.9 * torch.rand(H, generator=g)), "g1b": rn(H) * 0.4,
           "W2": bf16_rne(rn(2 * Cc, H) / math.sqrt(H)), "b2": rn(2 * Cc) * 0.5,
           "g2w": sign(2 * Cc) * (0.6 + 0.9 * torch.rand(2 * Cc, generator=g)), "g2b": rn(2 * Cc) * 0.4,
           "scale": sign(Cc) * (0.5 + torch.rand(Cc, generator=g))}
    if case.sat:
        inp["g2w"][Cc:] *= 60.0                                  # gates at +-60 |zhat|: beyond the fminf(., 126) clamp (87.3) and 1 - sigmoid = 0
    return inp
