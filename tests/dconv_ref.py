"""Plain torch, CPU restatement of ONE fused channel-major DConv depth-layer (remfx_amd/csrc/dconv.hip through its C ABI:
rfx_dconv_layer_fwd, rfx_dconv_layer_bwd), forward and closed-form backward, no autograd in the tested path.

x: (N, C = 48, T = 256) channel-major fp32 samples, H = C / 4 = 12, dil in {1, 2}:
    h = conv1d(x; W1 (H, C, 3), b1, dilation d, padding d)       zeros beyond the sample's ends (the two zero rows of the LDS image)
    a = GELU_erf(GN(1, H)(h));  z = W2 a + b2;  out = x + scale * GLU(GN(1, 2C)(z))      value = rows 0..C-1, gate = rows C..2C-1

Two arithmetics run the same formulas (class Exact: fp64, plain sums, two-pass variance; class Kern32: float32 with the kernels'
decomposition of every sum -- per lane in register order, rfx_wave_sum's butterfly, then the 4 waves of the forward / the 8 waves of one
sample in the backward in order, the one-pass variance max(s2 / n - mu^2, 0); the small gradients per (row, 32 position lanes) in
sample and tile order, the skewed 32-term row sum, one row of `partial` per workgroup).  Both round to bf16 exactly where dconv.hip does
unless `rounding=False`.

ROUNDING POINTS (read off dconv.hip).
Forward (dconv_fwd_kernel): x, W1, W2 are bf16 RNE GEMM operands (dc_store_xs / dc_frag8); h = acc + b1 in fp32; statistics 1 from the
UNROUNDED h; h16 = bf16(h) stored.  a = GELU(..) stored as FP32; bf16(a) is GEMM2's operand only.  z = acc + b2 in fp32; statistics 2
from the unrounded z; z16 = bf16(z) stored.  out = fma(scale, zn_value * sigmoid(zn_gate), x) with the UNROUNDED fp32 x.  stats (4, N):
mean1, rstd1, mean2, rstd2.
Backward (dconv_bwd_kernel): the forward is recomputed identically and a_out stored again.  The normalised z and gamma2 d(zn) are
PARKED as bf16 pairs (zh_pk, e_pk); the two sample means m1, m2 of GroupNorm-2's backward are taken over the UNROUNDED fp32 values --
cl_dconv.hip takes them over the parked ones (tests/cldconv_ref.py), this kernel does not.  dz = bf16(rs2 (e_pk - m1 - zh_pk m2)) is
stored and the same rounded value is da's operand.  d(hn) gamma1 stays fp32; dh = bf16(rs1 (e - q1 - hn q2)) is stored and is the
operand of the transposed 3-tap GEMM with bf16 W1^T.  dx = gy + acc in fp32.  The five small gradients are formed from unrounded fp32
values.

STAGING (judge_forward / judge_backward): an output is compared with the reference of ITS stage, fed what the kernel itself produced
one stage earlier, so a one-ulp flip of an intermediate is not charged to what follows.  Forward: h16 and statistics 1 from x; a_out
from the fp64 h and the kernel's own statistics 1; z16, statistics 2 and out from the kernel's own a_out.  Backward: a_out from the
fp64 h (statistics 1 never leave this kernel: the reference's own, their error in the magnitude); dz and the five GroupNorm-2 /
LayerScale sums from the reference chain continued at the kernel's own a_out (whose bf16 rounding is GEMM2's operand: the same staging
as the forward's); dh and the two GroupNorm-1 sums from the kernel's own dz; dx from the kernel's own dh.  Values that never leave the
kernel -- the parked pairs -- cannot be fed in: the reference keeps them unrounded and their rounding enters dz's bound weighted by rstd
(`park:dz`), as in cldconv_ref.

BOUND.  |got - ref| <= K eps32 magnitude (+ half a bf16 ulp of the value being rounded for h16, z16, dz, dh), K = 8 floor + 8 (k_of).
magnitude = sum of |terms| an element is formed from, each weighted by the derivative it enters with; the cancellation s2 / n - mu^2
sits inside the rstd terms (stat_mag), and where a stage uses the reference's statistics instead of the kernel's their error terms
are part of the magnitude (a hidden bias of 8 standard deviations widens the bound through them, not through K).  floor = Kern32
against Exact in those units, per output and case class (FLOORS; tests/test_dconv_ref_cpu.py holds the table to the measurement; never
measured on the kernel).

DEVICE FUNCTIONS.  rfx_gelu / rfx_gelu_grad (common.h; Abramowitz-Stegun erf, v_exp + v_rcp): as tests/norm_ref.py and
tests/cldconv_ref.py take them -- cdf = 0.5 + 0.5 erf counts as those two terms (an absolute error of a few eps32 of 1 whatever is left
of the cancellation: remfx_hip.h at RFX_ACT_GELU, DESIGN.md 4.21: cdf within 2.4 eps32), covered by the + 8 of K (norm_ref
FP32_HALF_ULPS: "16 fp32 half-ulps = 8 eps32 for what a CPU fp32 evaluation does not have -- v_exp_f32 / v_rcp_f32 at 1 ulp each,
exp(x) as exp2(x log2 e), the Abramowitz-Stegun erf"); rsqrtf is inside the same margin, as there.
dc_sigmoid(v) = v_rcp(1 + __expf(-v)) is this file's own form (the same expression as common.h's rfx_sigmoid, whose comment states
"v_exp_f32 + v_rcp_f32 (1 ulp each)").  The kernel guides give no accuracy figure for the two instructions, so the allowance is Kern32
with torch's fp32 sigmoid against Exact (the floor) plus that margin.  What the margin has to hold, from 1 ulp (<= eps32 relative) per
instruction: e = exp(-v) is v_exp(-v log2 e) -- the product's rounding, 2^-24 relative on the argument, is |v| eps32 / 2 relative on e, the
instruction adds eps32; 1 + e rounds at eps32 / 2; v_rcp adds eps32.  With d s / s = -(1 - s) d e / e:
    |d s| / s <= eps32 (1.5 + (1 - s) (1 + |v| / 2)).
The magnitude of every element sigmoid enters holds s (1 + (1 - s) A_gate) with A_gate >= |v| (the gate's own terms), so the 8 eps32 of
the margin cover 2.5 + |v| / 2 of it with room for the GELU and rsqrt terms of the same element.

`mutate`: a deliberately wrong Kern32 (MUTATIONS; tests/test_dconv_ref_cpu.py)."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.ref_common import EPS32, bf16_rne, bf16_trunc, f32, gelu_cdf, gelu_pdf, ulp, worst  # noqa: F401

C = 48
H = 12
T = 256
ROWS = 5 * C + 2 * H              # dscale C | dgn2w 2C | dgn2b 2C | dgn1w H | dgn1b H
SEG = {"dscale": (0, C), "dgn2w": (C, 3 * C), "dgn2b": (3 * C, 5 * C), "dgn1w": (5 * C, 5 * C + H), "dgn1b": (5 * C + H, ROWS)}
SMALL = tuple(SEG)
GEN_EPS = 1e-5
TINY = 2.0 ** -120                # bf16 stores may flush subnormals: absolute, far below any value here
BF16_STORED = ("h16", "z16", "dz", "dh")
FWD_OUT = ("h16", "mean1", "rstd1", "a_out", "z16", "mean2", "rstd2", "out")
BWD_OUT = ("a_out", "dz", "dh", "gx") + SMALL
WGRAD_OUT = ("dw2", "db2", "dw1", "db1")
_PRE = {"h16": "h", "z16": "z", "dz": "dz_pre", "dh": "dh_pre"}
_STATS_OF = {"a_out": ("mean1", "rstd1"), "out": ("mean2", "rstd2"), "dz": ("mean2", "rstd2"), "dh": ("mean1", "rstd1"),
             "dscale": ("mean2", "rstd2"), "dgn2w": ("mean2", "rstd2"), "dgn2b": ("mean2", "rstd2"), "dgn1w": ("mean1", "rstd1"),
             "dgn1b": ("mean1", "rstd1")}

# fault -> the outputs that have to catch it
MUTATIONS = {
    "dil_1_on_one_tap": ("h16",),             # tap 2 read at distance 1 where dil = 2
    "stale_zero_rows": ("h16",),              # the zero rows at a sample's ends hold the previous sample of the walk
    "stale_image": ("h16",),                  # the last sample of workgroup 0 computed from the image of sample s - grid
    "rows_12_15_next_sample": ("h16", "a_out", "dh"),   # rows 12-15 of the hidden tile (zeros) written into rows 0-3 of the next sample
    "stats1_one_wave": ("mean1", "rstd1"),    # statistics 1 over one wave's 64 positions
    "glu_swapped": ("out",),                  # value and gate swapped for one channel
    "scale_from_neighbour": ("out",),         # one channel's LayerScale from its neighbour
    "b2_gate_from_value": ("z16",),           # b2 of the gate rows taken from the value rows
    "dz_pairs_swapped": ("dz",),              # dz with positions (t, t + 1) exchanged for even t, value rows only (a swapped v_perm selector)
    "dead_sample_dgn2b": ("dgn2b",),          # the dead sample of an odd N adds its x = 0 forward into dgn2b
    "partial_last_row_missing": SMALL,        # partial without its last workgroup's row
    "dgn1_segments_exchanged": ("dgn1w", "dgn1b"),
    "means_over_parked": ("dz",),             # m1, m2 over the parked bf16 values instead of the fp32 ones
    "truncating_store": ("dz", "dh"),         # a truncating bf16 store
    "one_ulp_h16": ("h16",), "one_ulp_z16": ("z16",), "one_ulp_dz": ("dz",), "one_ulp_dh": ("dh",),
}
FWD_MUTATIONS = ("dil_1_on_one_tap", "stale_zero_rows", "stale_image", "rows_12_15_next_sample", "stats1_one_wave", "glu_swapped",
                 "scale_from_neighbour", "b2_gate_from_value", "one_ulp_h16", "one_ulp_z16")


def _half_ulp16(ref, t):
    return 0.5 * ulp(ref.abs() + t, 7)


def grid_fwd(N):
    return min(N, 512)


def bwd_rows(N):
    """rows of rfx_dconv_layer_bwd_ws: one workgroup (one row of partial) per pair of samples, 256 at the most"""
    return min((N + 1) // 2, 256)


def wg_samples(N, wg):
    """the live samples backward workgroup `wg` walks, in the order it meets them"""
    G, npairs = bwd_rows(N), (N + 1) // 2
    return [n for p in range(wg, npairs, G) for n in (2 * p, 2 * p + 1) if n < N]


# ---- the two arithmetics ---------------------------------------------------------------------------------------------------------------
_HROWS = ((0, 1, 2, 3, 8, 9, 10, 11), (4, 5, 6, 7))           # hidden rows < H of lane half hh in register order (dc_hrow)


def _zchan(hh):
    """channels of lane half hh in (mt, r) order (dc_chan)"""
    return [16 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh for mt in range(C // 16) for r in range(8)]


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


class Exact:
    """fp64, plain sums"""
    dtype = torch.float64

    @staticmethod
    def sums(u, w, waves):
        return u.reshape(u.shape[0], -1).sum(1), (u * w).reshape(u.shape[0], -1).sum(1)

    @staticmethod
    def stats(t, waves, eps):
        """two-pass variance: the truth, not the algorithm"""
        r = t.reshape(t.shape[0], -1)
        m = r.mean(1)
        return m, 1.0 / torch.sqrt(((r - m[:, None]) ** 2).mean(1) + f32(eps))

    @staticmethod
    def mean(s, n):
        return s / n


class Kern32:
    """float32 with the kernels' partial sums"""
    dtype = torch.float32

    @staticmethod
    def sums(u, w, waves):
        """(sum u, sum u w) per sample of (n, R, T), R = H or 2C.  A lane (position j of a 32-column tile, half hh) adds its registers
        in order (s1 += v; s2 = fma(v, w, s2); value and gate of a channel together for R = 2C), over its two column tiles in the
        forward (waves = 4) or its one in the backward (waves = 8); rfx_wave_sum; the waves in order."""
        n, R = u.shape[0], u.shape[1]
        ctn = T // (32 * waves)
        U, W = u.reshape(n, R, waves, ctn, 32), w.reshape(n, R, waves, ctn, 32)
        a1 = [torch.zeros(n, waves, 32) for _ in range(2)]
        a2 = [torch.zeros(n, waves, 32) for _ in range(2)]
        for ct in range(ctn):
            for hh in range(2):
                if R == H:
                    for m in _HROWS[hh]:
                        a1[hh] = a1[hh] + U[:, m, :, ct]
                        a2[hh] = _fma(U[:, m, :, ct], W[:, m, :, ct], a2[hh])
                else:
                    for c in _zchan(hh):
                        a1[hh] = a1[hh] + (U[:, c, :, ct] + U[:, C + c, :, ct])
                        a2[hh] = _fma(U[:, c, :, ct], W[:, c, :, ct], _fma(U[:, C + c, :, ct], W[:, C + c, :, ct], a2[hh]))

        def fold(a):
            lanes = torch.cat(a, -1)                            # (n, waves, 64): lane = 32 hh + j
            k = 32
            while k:
                lanes = lanes[..., :k] + lanes[..., k:2 * k]
                k //= 2
            wv = lanes[..., 0]
            s = wv[:, 0].clone()
            for i in range(1, waves):
                s = s + wv[:, i]
            return s
        return fold(a1), fold(a2)

    @staticmethod
    def stats(t, waves, eps):
        s1, s2 = Kern32.sums(t, t, waves)
        inv = torch.tensor(1.0 / (t.shape[1] * T), dtype=torch.float32)
        mu = s1 * inv
        return mu, torch.rsqrt((s2 * inv - mu * mu).clamp_min(0) + torch.tensor(eps, dtype=torch.float32))

    @staticmethod
    def mean(s, n):
        return s * torch.tensor(1.0 / n, dtype=torch.float32)


def partial_row32(contrib):
    """one workgroup's row of `partial` in fp32 from the contributions (samples in walk order, ROWS, T) of its samples: the
    accumulators [row][32 position lanes] take every sample's eight position tiles in order (the order of the kernel's LDS atomics
    is not fixed: this is one of them), then each row is summed from a skewed start"""
    acc = torch.zeros(ROWS, 32)
    for s in range(contrib.shape[0]):
        for pt in range(8):
            acc = acc + contrib[s, :, 32 * pt:32 * pt + 32]
    idx = (torch.arange(32)[None, :] + torch.arange(ROWS)[:, None]) & 31
    g = acc.gather(1, idx)
    v = torch.zeros(ROWS)
    for q in range(32):
        v = v + g[:, q]
    return v


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------
def _conv(x, W, dil, dil_of_tap=None):
    """sum over taps k of W[:, :, k] x(t + (k - 1) d), zeros beyond the sample's ends: (n, C, T) -> (n, H, T)"""
    xp = F.pad(x, (2, 2))
    out = 0
    for k in range(3):
        d = dil if dil_of_tap is None else dil_of_tap[k]
        o = 2 + (k - 1) * d
        out = out + torch.matmul(W[:, :, k], xp[:, :, o:o + T])
    return out


def _conv_t(dh, W, dil):
    """dx - gy: sum over taps of W[:, :, k]^T dh(t - (k - 1) d): (n, H, T) -> (n, C, T)"""
    dp = F.pad(dh, (2, 2))
    out = 0
    for k in range(3):
        o = 2 - (k - 1) * dil
        out = out + torch.matmul(W[:, :, k].transpose(0, 1), dp[:, :, o:o + T])
    return out


def stat_mag(t, mag_t, eps=GEN_EPS):
    """mean: mean(mag) (absolute).  rstd: relative, 0.5 x the terms of E[t^2] - m^2 over (var + eps), each with its own error"""
    r, g = t.double().reshape(t.shape[0], -1), mag_t.reshape(t.shape[0], -1)
    m = r.mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    num = (2 * r.abs() * g).mean(1) + (r * r).mean(1) + 2 * m.abs() * g.mean(1) + m * m
    return g.mean(1), 0.5 * num / (var + f32(eps))


def _b(s):
    return s[:, None, None]


def _one_ulp(stored, pre):
    """one element of the last sample one bf16 ulp off: the one whose own rounding error is the largest, moved further the same way"""
    t = stored.clone()
    d = (stored[-1] - pre[-1]).double()
    u = ulp(stored[-1].double(), 7)
    i = int((d.abs() / u).reshape(-1).argmax())
    step = (torch.where(d.reshape(-1)[i] < 0, -1.0, 1.0) * u.reshape(-1)[i]).to(stored.dtype)
    t[-1].view(-1)[i] += step
    return t


def _col(p):
    return p[:, None]


def _params(inp, ar, rnd):
    c = lambda t: t.to(ar.dtype)                                # noqa: E731
    p = {k: c(inp[k]) for k in ("b1", "g1w", "g1b", "b2", "g2w", "g2b", "scale")}
    p["W1"], p["W2"] = rnd(c(inp["W1"])), rnd(c(inp["W2"]))
    return p


def _head(x, p, dil, ar, rnd, waves, eps, mag, ximg=None, halo=None, mutate=None):
    """conv1 and statistics 1 -> o with h, mean1, rstd1 (+ mag:h16, mag:mean1, mag:rstd1)"""
    o = {}
    xi = rnd(x if ximg is None else ximg)
    h = _conv(xi, p["W1"], dil, dil_of_tap=(dil, dil, 1) if mutate == "dil_1_on_one_tap" else None) + _col(p["b1"])
    if halo is not None:                                        # the zero rows hold the previous sample's first / last rows
        h = h.clone()
        hp = rnd(halo)
        for q in range(dil):
            h[:, :, q] += hp[:, :, T - dil + q] @ p["W1"][:, :, 0].transpose(0, 1)
            h[:, :, T - dil + q] += hp[:, :, q] @ p["W1"][:, :, 2].transpose(0, 1)
    o["h"] = h
    o["mean1"], o["rstd1"] = ar.stats(h, waves, eps)
    if mutate == "stats1_one_wave":
        o["mean1"], o["rstd1"] = (s.to(ar.dtype) for s in Exact.stats(h[:, :, :64].double(), waves, eps))
    if mag:
        o["mag:h16"] = _conv(xi.abs(), p["W1"].abs(), dil) + _col(p["b1"].abs())
        o["mag:mean1"], o["mag:rstd1"] = stat_mag(h, o["mag:h16"], eps)
    return o


def _gelu_stage(o, p, m1, r1, mag, stats_fed):
    """a = GELU(gn1(h)) from o["h"] and the statistics (m1, r1) -> hn, u, a_out (+ mag:a_out, Ah)"""
    h = o["h"]
    hn = (h - _b(m1)) * _b(r1)
    u = hn * _col(p["g1w"]) + _col(p["g1b"])
    o["hn"], o["u"], o["a_out"] = hn, u, u * gelu_cdf(u)
    if mag:
        Ah = (o["mag:h16"] + _b(m1.abs())) * _b(r1)
        if not stats_fed:                                       # the reference's own statistics: their error is the element's too
            Ah = Ah + _b(o["mag:mean1"] * r1) + hn.abs() * _b(o["mag:rstd1"])
        Au = Ah * _col(p["g1w"].abs()) + _col(p["g1b"].abs())
        cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
        o["Ah"], o["Au"] = Ah, Au
        o["mag:a_out"] = Au * (2.0 * cdfm + u.abs() * gelu_pdf(u))


def _z_stage(o, a, p, ar, rnd, waves, eps, mag, mutate=None):
    """conv2 and statistics 2 from the fp32 a (its bf16 rounding is the operand) -> z, mean2, rstd2, zh (+ magnitudes)"""
    a16 = rnd(a)
    b2 = p["b2"]
    if mutate == "b2_gate_from_value":
        b2 = torch.cat([b2[:C], b2[:C]])
    z = torch.matmul(p["W2"], a16) + _col(b2)
    o["z"] = z
    m2, r2 = ar.stats(z, waves, eps)
    o["mean2"], o["rstd2"] = m2, r2
    o["zh"] = (z - _b(m2)) * _b(r2)
    if mag:
        mz = torch.matmul(p["W2"].abs(), a16.abs()) + _col(p["b2"].abs())
        o["mag:z16"] = mz
        o["mag:mean2"], o["mag:rstd2"] = stat_mag(z, mz, eps)
        o["Az"] = (mz + _b(m2.abs()) + _b(o["mag:mean2"])) * _b(r2) + o["zh"].abs() * _b(o["mag:rstd2"])
        o["Aw"] = o["Az"] * _col(p["g2w"].abs()) + _col(p["g2b"].abs())


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
def forward(inp, dil, ar=Exact, rounding=True, own=None, eps=GEN_EPS, mutate=None, ximg=None, halo=None):
    """every forward quantity of the samples in inp, in ar.dtype.  own: the tested code's own {stats (4, n), a_out} (staging).  Returns
    the UNROUNDED h / z next to the rounded h16 / z16, and (Exact) the magnitudes as 'mag:<name>'.  ximg / halo: see kern32_forward."""
    rnd = bf16_rne if rounding else (lambda t: t)
    mag = ar is Exact
    x = inp["x"].to(ar.dtype)
    p = _params(inp, ar, rnd)
    o = _head(x, p, dil, ar, rnd, 4, eps, mag, ximg=None if ximg is None else ximg.to(ar.dtype),
              halo=None if halo is None else halo.to(ar.dtype), mutate=mutate)
    o["h16"] = rnd(o["h"])
    fed = own is not None and "stats" in own
    m1, r1 = (own["stats"][0].to(ar.dtype), own["stats"][1].to(ar.dtype)) if fed else (o["mean1"], o["rstd1"])
    _gelu_stage(o, p, m1, r1, mag, fed)
    a = own["a_out"].to(ar.dtype) if own is not None and "a_out" in own else o["a_out"]
    _z_stage(o, a, p, ar, rnd, 4, eps, mag, mutate=mutate)
    o["z16"] = rnd(o["z"])
    w = o["zh"] * _col(p["g2w"]) + _col(p["g2b"])
    v, gt, s = w[:, :C], w[:, C:], p["scale"]
    if mutate == "glu_swapped":
        v, gt = v.clone(), gt.clone()
        v[:, C // 2], gt[:, C // 2] = w[:, C + C // 2], w[:, C // 2]
    if mutate == "scale_from_neighbour":
        s = s.clone()
        s[C // 2] = p["scale"][C // 2 + 1]
    sg = torch.sigmoid(gt)
    o["out"] = x + _col(s) * (v * sg)
    for name in ("h16", "z16"):
        if mutate == "one_ulp_" + name:
            o[name] = _one_ulp(o[name], o[_PRE[name]])
    if mag:
        Aw = o["Aw"]
        o["mag:out"] = x.abs() + _col(p["scale"].abs()) * sg * (Aw[:, :C] + v.abs() * (1.0 - sg) * Aw[:, C:])
    return o


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def backward(inp, dil, ar=Exact, rounding=True, own=None, eps=GEN_EPS, mutate=None):
    """every backward quantity of the samples in inp, in ar.dtype.  own: the tested code's own {a_out, dz, dh} (staging: z and what
    follows from a_out; dh and the GroupNorm-1 sums from dz; gx from dh).  dz_pre / dh_pre are the UNROUNDED stored values (Exact: with
    the parked pairs unrounded too, their rounding in 'park:dz').  'small' (n, ROWS): each sample's share of the five small gradients
    (Exact) -- Kern32 returns 'contrib' (n, ROWS, T), the summands, for partial_row32."""
    rnd = bf16_rne if rounding else (lambda t: t)
    own = own or {}
    mag = ar is Exact
    c = lambda t: t.to(ar.dtype)                                # noqa: E731
    x, gy = c(inp["x"]), c(inp["gy"])
    n = x.shape[0]
    p = _params(inp, ar, rnd)
    g1w, g2w, sc = _col(p["g1w"]), _col(p["g2w"]), _col(p["scale"])
    o = _head(x, p, dil, ar, rnd, 8, eps, mag)
    m1, r1 = o["mean1"], o["rstd1"]
    _gelu_stage(o, p, m1, r1, mag, False)
    a = c(own["a_out"]) if "a_out" in own else o["a_out"]
    _z_stage(o, a, p, ar, rnd, 8, eps, mag)
    r2, zh = o["rstd2"], o["zh"]
    w = zh * g2w + _col(p["g2b"])
    v, gt = w[:, :C], w[:, C:]
    sg = torch.sigmoid(gt)
    g0 = gy * sc
    dv = g0 * sg
    dgt = (g0 * v) * sg * (1.0 - sg)
    du = torch.cat([dv, dgt], 1)
    contrib = [gy * v * sg, du * zh, du]
    e_pre = du * g2w
    n2 = 2 * C * T
    S1, S2 = ar.sums(e_pre, zh, 8)
    pm1, pm2 = ar.mean(S1, n2), ar.mean(S2, n2)
    e_pk, zh_pk = rnd(e_pre), rnd(zh)
    if mutate == "means_over_parked":
        S1, S2 = ar.sums(e_pk, zh_pk, 8)
        pm1, pm2 = ar.mean(S1, n2), ar.mean(S2, n2)
    if mag:
        o["dz_pre"] = _b(r2) * ((e_pre - _b(pm1)) - zh * _b(pm2))
    else:
        o["dz_pre"] = _b(r2) * ((e_pk - _b(pm1)) - zh_pk * _b(pm2))
    o["dz"] = bf16_trunc(o["dz_pre"]) if mutate == "truncating_store" else rnd(o["dz_pre"])
    if mutate == "dz_pairs_swapped":
        sw = o["dz"][:, :C].reshape(n, C, T // 2, 2).flip(-1).reshape(n, C, T)
        o["dz"] = torch.cat([sw, o["dz"][:, C:]], 1)
    dzk = c(own["dz"]) if "dz" in own else o["dz"]
    da = torch.matmul(p["W2"].transpose(0, 1), dzk)
    hn, u = o["hn"], o["u"]
    pdf = gelu_pdf(u)
    gp = gelu_cdf(u) + u * pdf
    dhn = da * gp
    contrib += [dhn * hn, dhn]
    q_pre = dhn * g1w
    n1 = H * T
    Q1, Q2 = ar.sums(q_pre, hn, 8)
    qm1, qm2 = ar.mean(Q1, n1), ar.mean(Q2, n1)
    o["dh_pre"] = _b(r1) * (q_pre - _b(qm1) - hn * _b(qm2))
    o["dh"] = bf16_trunc(o["dh_pre"]) if mutate == "truncating_store" else rnd(o["dh_pre"])
    dhk = c(own["dh"]) if "dh" in own else o["dh"]
    o["gx"] = gy + _conv_t(dhk, p["W1"], dil)
    for name in ("dz", "dh"):
        if mutate == "one_ulp_" + name:
            o[name] = _one_ulp(o[name], o[_PRE[name]])
    if not mag:
        o["contrib"] = torch.cat(contrib, 1)
        return o
    o["small"] = torch.cat(contrib, 1).sum(-1)
    Az, Aw = o["Az"], o["Aw"]
    Av, Ag = Aw[:, :C], Aw[:, C:]
    mdu = torch.cat([g0.abs() * sg * (1.0 + (1.0 - sg) * Ag),
                     g0.abs() * sg * ((1.0 - sg) * Av + v.abs() * ((1.0 + sg) + (1.0 - sg) * (1.0 - 2.0 * sg).abs() * Ag))], 1)
    msmall = [gy.abs() * sg * (Av + v.abs() * (1.0 - sg) * Ag), mdu * zh.abs() + du.abs() * Az, mdu]
    mp = mdu * g2w.abs()
    M1 = mp.reshape(n, -1).mean(1)
    M2 = (mp * zh.abs() + e_pre.abs() * Az).reshape(n, -1).mean(1)
    o["mag:dz"] = _b(r2) * (mp + _b(M1) + zh.abs() * _b(M2) + Az * _b(pm2.abs())) + o["dz_pre"].abs() * _b(o["mag:rstd2"])
    o["park:dz"] = _b(r2) * 0.5 * (ulp(e_pre, 7) + _b(pm2.abs()) * ulp(zh, 7)) if rounding else torch.zeros_like(zh)
    mda = torch.matmul(p["W2"].abs().transpose(0, 1), dzk.abs())
    Ah, Au = o["Ah"], o["Au"]
    cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
    mdhn = mda * (cdfm + u.abs() * pdf) + da.abs() * pdf * (2.0 - u * u).abs() * Au
    msmall += [mdhn * hn.abs() + dhn.abs() * Ah, mdhn]
    mq = mdhn * g1w.abs()
    MQ1 = mq.reshape(n, -1).mean(1)
    MQ2 = (mq * hn.abs() + q_pre.abs() * Ah).reshape(n, -1).mean(1)
    o["mag:dh"] = _b(r1) * (mq + _b(MQ1) + hn.abs() * _b(MQ2) + Ah * _b(qm2.abs())) + o["dh_pre"].abs() * _b(o["mag:rstd1"])
    o["mag:gx"] = gy.abs() + _conv_t(dhk.abs(), p["W1"].abs(), dil)
    o["mag:small"] = torch.cat(msmall, 1).sum(-1)
    return o


def wgrad(inp, dil, dz, a, dh, rounding=True):
    """the two weight gradients and bias gradients in fp64 from the kernel's own dz / a_out and dh and the layer input, the fp32
    operands rounded to bf16 as the weight-gradient GEMM of the bf16 mode reads them -> values and magnitudes"""
    rnd = bf16_rne if rounding else (lambda t: t)
    dz, dh, a16, x16 = dz.double(), dh.double(), rnd(a.double()), rnd(inp["x"].double())
    xp = F.pad(x16, (2, 2))
    sh = lambda t, k: t[:, :, 2 + (k - 1) * dil:2 + (k - 1) * dil + T]     # noqa: E731
    o = {"dw2": torch.einsum("nrt,nht->rh", dz, a16), "db2": dz.sum((0, 2)), "db1": dh.sum((0, 2)),
         "dw1": torch.stack([torch.einsum("nht,nct->hc", dh, sh(xp, k)) for k in range(3)], -1),
         "mag:dw2": torch.einsum("nrt,nht->rh", dz.abs(), a16.abs()), "mag:db2": dz.abs().sum((0, 2)), "mag:db1": dh.abs().sum((0, 2)),
         "mag:dw1": torch.stack([torch.einsum("nht,nct->hc", dh.abs(), sh(xp.abs(), k)) for k in range(3)], -1)}
    return o


# ---- judging -----------------------------------------------------------------------------------------------------------------------------
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


def _k(K, name):
    """K of an output whose magnitude carries the error terms of the reference's statistics: not below theirs"""
    return max([K[name]] + [K[s] for s in _STATS_OF.get(name, ()) if s in K])


def take(inp, idx):
    """the inputs restricted to the samples idx"""
    out = dict(inp)
    for k in ("x", "gy"):
        out[k] = inp[k][idx]
    return out


def _chunks(sel, size):
    return [sel[i:i + size] for i in range(0, len(sel), size)]


def _merge(res, name, q, i):
    if name not in res or q > res[name][0]:
        res[name] = (q, i)


def stage_forward(inp, dil, got, eps=GEN_EPS):
    """the staged Exact reference of a forward result `got` {h16, a_out, z16, out (n, ., T), stats (4, n)} on the same samples"""
    return forward(inp, dil, Exact, True, own={"stats": got["stats"].double(), "a_out": got["a_out"].double()}, eps=eps)


def _split_stats(got):
    g = dict(got)
    st = got["stats"].double()
    g.update(mean1=st[0], rstd1=st[1], mean2=st[2], rstd2=st[3])
    return g


def judge_forward(inp, dil, got, K, sel=None, measure=False, chunk=64):
    """{name: (largest error / tolerance, sample)} over the samples sel of inp / got (all by default), `chunk` at a time.  measure: the
    floor instead -- the largest |got - ref| beyond the bf16 half-ulps in units of eps32 magnitude"""
    N = inp["x"].shape[0]
    res = {}
    for idx in _chunks(list(range(N)) if sel is None else list(sel), chunk):
        g = _split_stats({k: got[k][idx] if k != "stats" else got[k][:, idx] for k in ("h16", "a_out", "z16", "out", "stats")})
        ref = stage_forward(take(inp, idx), dil, g)
        for name in FWD_OUT:
            q, i = _ratio(name, ref, g[name], K, measure)
            _merge(res, name, q, idx[i // max(1, g[name].numel() // len(idx))])
    return res


def _ratio(name, ref, got, K, measure):
    if not measure:
        val, t = _tol(name, ref, _k(K, name))
        return worst(got, val, t)
    val, t0 = _tol(name, ref, 0.0)
    e = ((got.double() - val).abs() - t0).clamp_min(0)
    unit = EPS32 * ref["mag:" + name] * (ref[name] if name.startswith("rstd") else 1.0)
    q = e / unit.clamp_min(1e-300)
    i = int(q.reshape(-1).argmax())
    return float(q.reshape(-1)[i]), i


def judge_backward(inp, dil, got, K, sel=None, rows=None, measure=False, chunk=64, feed=("a_out", "dz", "dh")):
    """as judge_forward for {a_out, dz, dh, gx (n, ., T), partial (G, ROWS)}.  The five small gradients: every row `rows` of partial
    (all by default) against the sum of its workgroup's samples, and -- when every row is judged -- the fp64 column sums against the sum
    of all; the row figure and the column figure share a name, the larger counts.  sel: per-element outputs on these samples only (the
    samples of `rows` are always evaluated).  feed: the kernel's own outputs the stages continue at (all three: the staging of this
    file; fewer: what an unstaged comparison would show)."""
    N = inp["x"].shape[0]
    G = bwd_rows(N)
    rows = list(range(G)) if rows is None else list(rows)
    need = sorted({n for wg in rows for n in wg_samples(N, wg)})
    sel = list(range(N)) if sel is None else list(sel)
    small, msmall = torch.zeros(N, ROWS, dtype=torch.float64), torch.zeros(N, ROWS, dtype=torch.float64)
    res, sel_set = {}, set(sel)
    for idx in _chunks(sorted(sel_set | set(need)), chunk):
        g = {k: got[k][idx] for k in ("a_out", "dz", "dh", "gx")}
        ref = backward(take(inp, idx), dil, Exact, True, own={k: g[k].double() for k in feed})
        small[idx], msmall[idx] = ref["small"], ref["mag:small"]
        keep = [i for i, n in enumerate(idx) if n in sel_set]
        if not keep:
            continue
        for name in ("a_out", "dz", "dh", "gx"):
            sub = {k: v[keep] for k, v in ref.items() if k in (name, _PRE.get(name, name), "mag:" + name, "park:" + name)}
            q, i = _ratio(name, sub, g[name][keep], K, measure)
            _merge(res, name, q, idx[keep[i // (g[name][keep].numel() // len(keep))]])
    part = got["partial"].double()
    ref_rows = torch.stack([small[wg_samples(N, wg)].sum(0) for wg in rows])
    mag_rows = torch.stack([msmall[wg_samples(N, wg)].sum(0) for wg in rows])
    sets = [(part[rows], ref_rows, mag_rows)]
    if len(rows) == G:
        sets.append((part.sum(0, keepdim=True), ref_rows.sum(0, keepdim=True), mag_rows.sum(0, keepdim=True)))
    for gotp, refp, magp in sets:
        for name, (lo, hi) in SEG.items():
            r = {name: refp[:, lo:hi], "mag:" + name: magp[:, lo:hi]}
            q, i = _ratio(name, r, gotp[:, lo:hi], K, measure)
            _merge(res, name, q, rows[i // (hi - lo)] if gotp.shape[0] > 1 or len(rows) == 1 else -1)
    return res


def judge_wgrad(inp, dil, got, K, measure=False):
    ref = wgrad(inp, dil, got["dz"], got["a_out"], got["dh"])
    return {name: _ratio(name, ref, got[name], K, measure) for name in WGRAD_OUT}


# ---- the fp32 restatement, with the planted faults -----------------------------------------------------------------------------------------
def kern32_forward(inp, dil, sel=None, mutate=None, eps=GEN_EPS):
    """Kern32 on the samples sel of inp (all by default) -> got {h16, a_out, z16, out, stats} indexed like sel.  A fault that involves
    another sample of the walk takes it from inp: the last sample of sel is the one workgroup 0 meets second, its predecessor is
    sample sel[-1] - grid."""
    N = inp["x"].shape[0]
    sel = list(range(N)) if sel is None else list(sel)
    sub = take(inp, sel)
    ximg = halo = None
    if mutate in ("stale_image", "stale_zero_rows"):
        prev = sel[-1] - grid_fwd(N)
        assert prev >= 0, "the fault needs a case whose forward walk has a second sample"
        other = inp["x"][[prev]].expand(len(sel), C, T)
        last = torch.zeros(len(sel), 1, 1)
        last[-1] = 1.0
        if mutate == "stale_image":
            ximg = sub["x"] * (1.0 - last) + other * last
        else:
            halo = other * last
    f = forward(sub, dil, Kern32, True, eps=eps, mutate=mutate, ximg=ximg, halo=halo)
    got = {k: f[k] for k in ("h16", "a_out", "z16", "out")}
    got["stats"] = torch.stack([f["mean1"], f["rstd1"], f["mean2"], f["rstd2"]], 0)
    if mutate == "rows_12_15_next_sample":
        assert len(sel) > 1 and sel[1] == sel[0] + 1
        got["h16"], got["a_out"] = got["h16"].clone(), got["a_out"].clone()
        got["h16"][1, :4] = 0
        got["a_out"][1, :4] = 0
    return got


def kern32_backward(inp, dil, rows=None, mutate=None, eps=GEN_EPS):
    """Kern32 on the samples of the workgroups `rows` of inp's N samples (all by default) -> (got {a_out, dz, dh, gx: (N, ., T), zero
    where not evaluated; partial (G, ROWS), zero rows where not evaluated}, the evaluated samples)"""
    N = inp["x"].shape[0]
    G = bwd_rows(N)
    rows = list(range(G)) if rows is None else list(rows)
    need = sorted({n for wg in rows for n in wg_samples(N, wg)})
    f = backward(take(inp, need), dil, Kern32, True, eps=eps, mutate=mutate)
    got = {}
    for k, R in (("a_out", H), ("dz", 2 * C), ("dh", H), ("gx", C)):
        got[k] = torch.zeros(N, R, T)
        got[k][need] = f[k]
    pos = {n: i for i, n in enumerate(need)}
    part = torch.zeros(G, ROWS)
    for wg in rows:
        ctr = f["contrib"][[pos[n] for n in wg_samples(N, wg)]]
        if mutate == "dead_sample_dgn2b" and N % 2 and wg == ((N + 1) // 2 - 1) % G:
            dead = {"x": torch.zeros(1, C, T), "gy": inp["gy"][[N - 1]]}
            fd = backward({**inp, **dead}, dil, Kern32, True, eps=eps)["contrib"].clone()
            lo, hi = SEG["dgn2b"]
            fd[:, :lo] = 0
            fd[:, hi:] = 0
            ctr = torch.cat([ctr, fd], 0)
        part[wg] = partial_row32(ctr)
    if mutate == "partial_last_row_missing":
        part[rows[-1]] = 0
    if mutate == "dgn1_segments_exchanged":
        lo = SEG["dgn1w"][0]
        part = torch.cat([part[:, :lo], part[:, lo + H:], part[:, lo:lo + H]], 1)
    if mutate == "rows_12_15_next_sample":
        assert need[1] == need[0] + 1
        got["dh"][need[1], :4] = 0
        got["a_out"][need[1], :4] = 0
    got["partial"] = part
    return got, need


# ---- floors measured on the CPU over the case table (tests/test_dconv_ref_cpu.py::test_floors holds them to the measurement; DESIGN.md
# 4.26): per case class and output the largest over the class's cases, rounded up to the next 0.25; K = 8 floor + 8
FLOORS = {
    "fwd": {"h16": 0.25, "mean1": 0.25, "rstd1": 0.25, "a_out": 0.5, "z16": 0.75, "mean2": 0.25, "rstd2": 0.5, "out": 0.75},
    "fwd-bias": {"h16": 0.25, "mean1": 0.25, "rstd1": 0.25, "a_out": 0.25, "z16": 0.25, "mean2": 0.25, "rstd2": 0.25, "out": 0.5},
    "bwd": {"a_out": 0.25, "dz": 0.25, "dh": 0.25, "gx": 1.5, "dscale": 0.25, "dgn2w": 0.25, "dgn2b": 0.25, "dgn1w": 0.25, "dgn1b": 0.25},
    "bwd-bias": {"a_out": 0.25, "dz": 0.25, "dh": 0.25, "gx": 0.75, "dscale": 0.25, "dgn2w": 0.25, "dgn2b": 0.5, "dgn1w": 0.25,
                 "dgn1b": 0.25},
}
# the weight-gradient GEMM is judged with its own family's floors (tests/gemm_ref.py FLOORS["wgrad_bf16"])
FLOORS_WGRAD = {"dw2": 0.75, "db2": 0.25, "dw1": 0.75, "db1": 0.25}


def k_of(floor):
    """the bound in units of eps32 * magnitude: 8 x floor + 16 fp32 half-ulps"""
    return 8.0 * floor + 8.0


def K_of(klass):
    return {n: k_of(f) for n, f in FLOORS[klass].items()}


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    N: int
    dil: int
    bias: bool = False            # hidden bias b1 of about 8 standard deviations of h: the one-pass variance cancels 64-fold

    @property
    def id(self):
        return f"n{self.N}-d{self.dil}" + ("-bias" if self.bias else "")

    def klass(self, bwd):
        return ("bwd" if bwd else "fwd") + ("-bias" if self.bias else "")

    def cpu_rows(self):
        """the backward workgroups the CPU test evaluates (the GPU test judges every one): the first, whose walk is the longest and at
        N = 513 ends in the half-dead pair, its neighbour and the last"""
        G = bwd_rows(self.N)
        return sorted({0, min(1, G - 1), G - 1})

    def cpu_sel(self):
        """the forward samples the CPU test evaluates: workgroup 0's walk and the last two"""
        return sorted({n for n in (0, 1, grid_fwd(self.N), self.N - 2, self.N - 1) if 0 <= n < self.N})


def cases():
    """N = 1: forward grid 1, the whole second half of the backward workgroup dead.  2: one full pair.  3: a live pair and a half-dead
    one in different workgroups.  513: the forward's workgroup 0 walks samples 0 and 512 over a stale LDS image; backward, 257 pairs on
    256 workgroups, workgroup 0's second pair half-dead, the x prefetch runs past N.  514: that second pair fully live.  The smallest N
    at which the persistent loops iterate."""
    return [Case(1, 1), Case(1, 2), Case(2, 1), Case(3, 2), Case(513, 1), Case(513, 2), Case(514, 1), Case(3, 1, bias=True)]


def make_inputs(case):
    """fp32 CPU tensors, seeded by the case.  x[n] = m_n + s_n * randn with m_n uniform in [-1.5, 1.5] and s_n uniform in [0.5, 2]
    (every sample differs in mean and amplitude: a stale image or a neighbour's row is far outside the bound), gy[n] likewise with
    s_n in [0.5, 1.5], m_n in [-0.3, 0.3]; positions 0, 1, 254, 255 of both x 6 (the largest values sit where the zero rows and the
    transposed taps matter).  Nothing is bf16-representable: every operand rounding is exercised.  W1 = randn / sqrt(3 C); W2 = randn /
    sqrt(H) with the gate rows x 1.7; b1, b2 = 0.5 randn; gn1w, gn2w of random sign with magnitude uniform in [0.6, 1.5] (away from
    1), gn1b, gn2b = 0.4 randn (away from 0), scale of random sign, magnitude in [0.5, 1.5]: every row's parameters differ.  bias:
    b1 = +-(8 + 0.3 randn) with one sign for all rows and s_n = 1, m_n = 0: |mean(h)| is about 8 std(h)."""
    g = torch.Generator().manual_seed(100000 + 100 * case.N + 10 * case.dil + case.bias)
    N = case.N
    rn = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)          # noqa: E731
    sign = lambda n: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()     # noqa: E731
    x = un(-1.5, 1.5, N, 1, 1) + un(0.5, 2.0, N, 1, 1) * rn(N, C, T)
    gy = un(-0.3, 0.3, N, 1, 1) + un(0.5, 1.5, N, 1, 1) * rn(N, C, T)
    if case.bias:
        x = rn(N, C, T)
    for t in (x, gy):
        t[:, :, :2] *= 6.0
        t[:, :, T - 2:] *= 6.0
    W2 = rn(2 * C, H) / math.sqrt(H)
    W2[C:] *= 1.7
    inp = {"x": x, "gy": gy, "W1": rn(H, C, 3) / math.sqrt(3 * C), "b1": rn(H) * 0.5,
           "g1w": sign(H) * un(0.6, 1.5, H), "g1b": rn(H) * 0.4, "W2": W2, "b2": rn(2 * C) * 0.5,
           "g2w": sign(2 * C) * un(0.6, 1.5, 2 * C), "g2b": rn(2 * C) * 0.4, "scale": sign(C) * un(0.5, 1.5, C)}
    if case.bias:
        inp["b1"] = float(sign(1)) * (8.0 + 0.3 * rn(H))
    return inp
