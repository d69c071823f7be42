"""fp64 restatement of remfx_amd/csrc/elementwise.hip (every entry point but rfx_row_affine_add / rfx_fm_cm_affine_g) and of rfx_l1_grad:
closed forms, no autograd, written as the OPERATION on the logical tensor and not as the kernels' indexing.  forms_*() say which kernel
and which of its branches a case reaches (from the launch code's conditions), restate_*() are float32 evaluations of the same formulas
in the kernels' decomposition (never a kernel) that give the floors, and the *_CASES tables are what the CPU and the GPU test walk.

Bounds, eps32 = 2^-23, one half-ulp = 2^-24 relative; none is measured on a kernel:
  exact        none / ReLU / leaky / slope-PReLU forward, their derivatives times gy, rfx_l1_grad, rfx_mul, rfx_row_affine without b,
               rfx_span_mask, rfx_blstm_frames modes 0, 2 without skip, 3, rfx_dropout: one fp32 rounding of an fp64-exact value (or none).
  one rounding rfx_blstm_frames mode 2 with skip: 2^-24 |result|.
  counted      rfx_add_bcast x + alpha y: 2 half-ulps of |x| + |alpha y| (a rounded product and a rounded sum; one FMA rounds once).
               rfx_row_affine with b: 2 half-ulps of |x a| + |b| (the same).
               rfx_act_add_fwd: the activation's bound + 1 half-ulp of |act| + |res| (+ 1 of |0.01 x| for leaky: product, then sum).
               rfx_blstm_frames mode 1: ceil(width / stride) - 1 half-ulps of sum |terms| (the first term is added to 0).
               coef_a: 3 half-ulps (eps + std, the quotient, their product term); coef_b = -mean a: 4.
  fp64 sums    rfx_l1_sum, channel_sum_kernel, rfx_row_moments: 4 x 2^-53 x (additions on the longest path) x sum |terms|, plus the
               fp32 roundings of the terms (|a - b|: one) and of the result (l1: (float)acc and * scale, two).
               mean: + 2^-24 |mean|.  std: + 2^-24 std, and the cancellation s2 - L m^2 carried through the square root.
  K rule       GELU, tanh, sigmoid and their derivatives, channel_sum_plane_kernel, gslope: K eps32 magnitude, K = 8 floor + 8 with the
               floor of FLOOR below (test_elem_ref_cpu.py recomputes every one from restate_* and asserts it is no larger), plus one
               smallest normal 2^-126 (x (1 + |gy|)) for the activations (expf(-v) overflows where the sigmoid is still a subnormal: the
               formula returns 0 there), one subnormal spacing 2^-149 for gslope."""
import math

import numpy as np
import torch

from tests.ref_common import EPS32, f32  # noqa: F401

HALF = 2.0 ** -24
TINY = 2.0 ** -149
MINNORM = 2.0 ** -126             # 1 / (1 + expf(-v)) returns 0 once expf overflows: results below the smallest normal are not formed
NONE, RELU, GELU, TANH, PRELU, LEAKY, SIGMOID = range(7)
ACT_NAMES = ("none", "relu", "gelu", "tanh", "prelu", "leaky", "sigmoid")
EXACT_ACTS = (NONE, RELU, PRELU, LEAKY)
LEAKY_SLOPE = float(np.float32(0.01))
L1_SLOTS = 512
SQRT2 = math.sqrt(2.0)

# floors in units of eps32 x magnitude, measured on restate_* over the case tables (printed by test_floors_are_below_the_table) and
# rounded up to the next half; K = 8 floor + 8.  Measured: 4.70, 4.42, 0.53, 0.71, 0.98, 1.69, 0.04, 0.00, 0.10
FLOOR = {"gelu": 5.0, "gelu_grad": 4.5, "tanh": 1.0, "tanh_grad": 1.0, "sigmoid": 1.0, "sigmoid_grad": 2.0,
         "channel_plane": 0.5, "channel_plane_const": 0.5, "gslope": 0.5}


def k_of(name):
    return 8.0 * FLOOR[name] + 8.0


# ---- activations -------------------------------------------------------------------------------------------------------------------
def erf_abs(x):
    return torch.erf(x.abs() / SQRT2)


def pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act(x, code, slope=0.0):
    """act(x) in fp64; slope: a double or a tensor broadcast against x (PReLU)"""
    x = x.double()
    if code == RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if code == GELU:
        return x * 0.5 * torch.special.erfc(-x / SQRT2)
    if code == TANH:
        return torch.tanh(x)
    if code == PRELU:
        return torch.where(x >= 0, x, slope * x)
    if code == LEAKY:
        return torch.where(x >= 0, x, LEAKY_SLOPE * x)
    if code == SIGMOID:
        return torch.where(x >= 0, 1.0 / (1.0 + torch.exp(-x.clamp_min(0))), torch.exp(x.clamp_max(0)) / (1.0 + torch.exp(x.clamp_max(0))))
    return x.clone()


def act_grad(x, code, slope=0.0):
    x = x.double()
    one = torch.ones_like(x)
    if code == RELU:
        return torch.where(x > 0, one, 0.0 * one)
    if code == GELU:
        return 0.5 * torch.special.erfc(-x / SQRT2) + x * pdf(x)
    if code == TANH:
        return 1.0 / torch.cosh(x.clamp(-700, 700)) ** 2
    if code == PRELU:
        return torch.where(x >= 0, one, slope * one)
    if code == LEAKY:
        return torch.where(x >= 0, one, LEAKY_SLOPE * one)
    if code == SIGMOID:
        s = act(x, SIGMOID)
        return s * act(-x, SIGMOID)
    return one


def act_magnitude(x, code):
    x = x.double()
    if code == GELU:
        return x.abs() * (0.5 + 0.5 * erf_abs(x))
    return act(x, code).abs()


def act_grad_magnitude(x, g, code):
    """sum of |terms| of gy act'(x), each weighted by the derivative it enters with"""
    x, g = x.double(), g.double().abs()
    if code == GELU:
        return g * (0.5 + 0.5 * erf_abs(x) + x.abs() * pdf(x))
    if code == TANH:
        return g * (1.0 + torch.tanh(x) ** 2)
    if code == SIGMOID:
        s = act(x, SIGMOID)
        return g * s * (1.0 + s)
    return g * act_grad(x, code).abs()


def act_bound(x, code):
    if code in EXACT_ACTS:
        return torch.zeros(x.shape, dtype=torch.float64)
    return k_of(ACT_NAMES[code]) * EPS32 * act_magnitude(x, code) + MINNORM


def act_grad_bound(x, g, code):
    if code in EXACT_ACTS:
        return torch.zeros(x.shape, dtype=torch.float64)
    return k_of(ACT_NAMES[code] + "_grad") * EPS32 * act_grad_magnitude(x, g, code) + MINNORM * (1.0 + g.double().abs())


def act_add_bound(x, res, code):
    a = act(x, code)
    b = act_bound(x, code) + HALF * (a.abs() + res.double().abs())
    if code == LEAKY:
        b = b + HALF * torch.where(x.double() < 0, a.abs(), torch.zeros_like(a))
    return b


def _fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product of two floats is exact in fp64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def restate_gelu(x):
    """rfx_gelu_parts' sequence in float32 with its fp32 constants (exact division and exp for v_rcp / v_exp) -> (gelu, gelu')"""
    f = np.float32
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", under="ignore"):
        ax = np.abs(x) * f(0.70710678118654752440)
        t = (f(1.0) / _fma32(f(0.3275911), ax, f(1.0))).astype(f)
        ex = np.exp((f(-0.5) * x * x).astype(np.float64)).astype(f)
        p = _fma32(f(1.061405429), t, f(-1.453152027))
        p = _fma32(p, t, f(1.421413741))
        p = _fma32(p, t, f(-0.284496736))
        p = _fma32(p, t, f(0.254829592))
        e = (f(1.0) - (p * t) * ex).astype(f)
        cdf = (f(0.5) * (f(1.0) + np.copysign(e, x))).astype(f)
        return (x * cdf).astype(f), _fma32((x * f(0.39894228040143267794)).astype(f), ex, cdf)


def restate_act(x, code):
    """float32 evaluation of the kernels' formula (CPU libm) -> (act, act') as float32 tensors"""
    xf = x.float()
    if code == GELU:
        a, g = restate_gelu(xf.numpy())
        return torch.from_numpy(a), torch.from_numpy(g)
    if code == TANH:
        t = torch.tanh(xf)
        return t, 1.0 - t * t
    if code == SIGMOID:
        s = 1.0 / (1.0 + torch.exp(-xf))
        return s, s * (1.0 - s)
    raise ValueError(code)


def act_data(n, seed):
    """finite fp32 only.  A dense band in [-12, 12]; from n = 1023 on, elements 16 ... hold log-spaced magnitudes 1e-30 ... 3e19 of both
    signs (their squares overflow at the top: the kernel must return the limit), +-0, fp32 subnormals, +-88 and +-104 (sigmoid's expf);
    the last three elements (the n % 4 tail) are of order 1."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g, dtype=torch.float64) * 24.0 - 12.0).float()
    if n >= 1023:
        s = specials()
        x[16:16 + s.numel()] = s
    tail = torch.tensor([0.75, -1.25, 1.5])
    x[max(n - 3, 0):] = tail[:min(n, 3)]
    return x


def specials():
    mags = torch.logspace(-30, math.log10(3e19), 100, dtype=torch.float64).float()
    sub = torch.tensor([2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 1.1e-38], dtype=torch.float64).float()
    edge = torch.tensor([88.0, 104.0, 87.3, 16.7, 9.1, 3.16, 0.042384, 0.06594])
    pos = torch.cat([mags, sub, edge, torch.zeros(1)])
    return torch.cat([pos, -pos])


def band(x):
    """the elements the power statement is made on: the dense band without the special values (whose bound is the same formula, but
    whose values, up to 3e19, would make an RMS meaningless)"""
    m = torch.ones(x.numel(), dtype=torch.bool)
    if x.numel() >= 1023:
        m[16:16 + specials().numel()] = False
    return m


def signs_data(n, seed, lo=0.5, hi=2.0):
    """magnitudes in [lo, hi], random sign: a gradient that is nowhere 0"""
    g = torch.Generator().manual_seed(seed)
    m = lo + (hi - lo) * torch.rand(n, generator=g)
    return (m * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()


def grid_for(n):
    return min(max(-(-n // 1024), 1), 2048)


FLAT_N = (1, 3, 4, 5, 1023, 1025, 2048 * 1024 + 1027)
FLAT_OFFSET_N = (5, 1025)                   # also run from a view one element into its allocation
FLAT_KERNELS = ("act_fwd_kernel", "act_bwd_kernel", "act_add_fwd_kernel")


def forms_flat(kernel, n, grid=None):
    """float4 grid-stride body + scalar n % 4 tail of the flat kernels (grid of 256 threads, grid_for's cap of 2048)"""
    g = grid_for(n) if grid is None else grid
    out = set()
    if n >= 4:
        out.add(kernel + ":vec")
    if n % 4:
        out.add(kernel + ":tail")
    if n // 4 > g * 256:
        out.add(kernel + ":second_iteration")
    if -(-n // 1024) > 2048 and grid is None:
        out.add(kernel + ":grid_capped")
    return out


# ---- act_rows ----------------------------------------------------------------------------------------------------------------------
ROWS_D = ((2, 3, 2), (1, 1, 5))
ROWS_T_VEC = (4, 252, 256, 260, 516)
ROWS_T_SCALAR = (1, 3, 255, 257)
ROWS_FALSIFY = ("stride", "x", "out", "gy")          # one clause of the vec predicate each, at T = 256


def rows_vec(x16, bwd, T, strides, x_off, out_off, gy_off):
    """the `vec` predicate of act_rows_launch; strides: all row strides that are passed; *_off: byte offsets from 16-byte alignment"""
    xal = 7 if x16 else 15
    oal = 7 if (x16 and bwd) else 15
    return (T % 4 == 0 and all(s % 4 == 0 for s in strides) and x_off & xal == 0 and out_off & oal == 0
            and (not bwd or gy_off & 15 == 0))


def forms_rows(x16, bwd, D, T, strides, x_off=0, out_off=0, gy_off=0):
    vec = rows_vec(x16, bwd, T, strides, x_off, out_off, gy_off)
    k = f"act_rows_kernel<{'vec' if vec else 'scalar'},{'bf16' if x16 else 'f32'}>:{'bwd' if bwd else 'fwd'}"
    out = {k}
    if (D[0] * D[1] * D[2] * -(-T // 256)) % 4:
        out.add("act_rows_kernel:idle_waves")
    if T > 256:
        out.add("act_rows_kernel:second_chunk")
    if vec and T % 256:
        out.add("act_rows_kernel:vec_partial_chunk")
    return out


def act_rows(x, D, xs, os_, T, code, out, gy=None, gs=None):
    """gather / scatter over explicit (D0, D1, D2) strides on flat buffers (fp64): out[o(i)] [t] = act(x[x(i)] [t]) (or gy act')"""
    for i0 in range(D[0]):
        for i1 in range(D[1]):
            for i2 in range(D[2]):
                xo = i0 * xs[0] + i1 * xs[1] + i2 * xs[2]
                oo = i0 * os_[0] + i1 * os_[1] + i2 * os_[2]
                row = x[xo:xo + T]
                if gy is None:
                    out[oo:oo + T] = act(row, code)
                else:
                    go = i0 * gs[0] + i1 * gs[1] + i2 * gs[2]
                    out[oo:oo + T] = gy[go:go + T].double() * act_grad(row, code)
    return out


def bf16_half_ulp(v):
    """half a bf16 ulp of the value being rounded (8 significant bits: 2^-8 relative at most; half the subnormal spacing 2^-133)"""
    return v.abs() * 2.0 ** -8 + 2.0 ** -134


# ---- mul, prelu --------------------------------------------------------------------------------------------------------------------
MUL_N = (1, 3, 4, 5, 1027, 4096 * 1024 + 1027)
PRELU_SHAPES = ((1, 1, 1), (3, 5, 255), (2, 3, 257), (3, 2, 4099))


def forms_mul(n):
    out = set()
    if n >= 4:
        out.add("mul_kernel:vec")
    if n % 4:
        out.add("mul_kernel:tail")
    if -(-n // 1024) > 4096:
        out.update(("mul_kernel:grid_capped", "mul_kernel:second_iteration"))
    return out


def forms_prelu(N, C, L):
    out = {"prelu_fwd_kernel", "prelu_bwd_kernel", "rfx_slot_sum_kernel<float>"}
    if L > 256:
        out.update(("prelu_fwd_kernel:second_iteration", "prelu_bwd_kernel:second_iteration"))
    if L < 256:
        out.add("prelu_bwd_kernel:idle_lanes")
    if C % 4:
        out.add("rfx_slot_sum_kernel<float>:partial_workgroup")
    return out


def prelu_data(N, C, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, L, generator=g)
    flat = x.view(-1)
    flat[0::7] = 0.0
    flat[3::7] = -0.0                                                                    # the >= side is part of the contract
    gy = signs_data(N * C * L, seed + 1).view(N, C, L)
    slope = torch.tensor([0.25, -0.5, 0.0, 1.5, -0.125])[:C].clone() if C > 1 else torch.tensor([0.25])
    return x, gy, slope


def prelu_bwd(x, gy, slope):
    """-> gx (fp64), gslope (fp64), mag = sum |g v| over the negative side"""
    xd, gd, s = x.double(), gy.double(), slope.double().view(1, -1, 1)
    neg = xd < 0
    gx = torch.where(neg, s * gd, gd)
    t = torch.where(neg, gd * xd, torch.zeros_like(xd))
    return gx, t.sum((0, 2)), t.abs().sum((0, 2))


def restate_gslope(x, gy):
    """per (n, c) row: 256 fp32 lane accumulators over i, i + 256, ... (a rounded product, a rounded sum), the 64-lane butterfly,
    (p0 + p1) + (p2 + p3); the rows of a channel are added in fp64"""
    N, C, L = x.shape
    xn, gn = x.numpy(), gy.numpy()
    out = np.zeros(C, np.float64)
    for n in range(N):
        for c in range(C):
            acc = np.zeros(256, np.float32)
            for i0 in range(0, L, 256):
                v, g = xn[n, c, i0:i0 + 256], gn[n, c, i0:i0 + 256]
                t = np.where(v >= 0, np.float32(0), (g * v).astype(np.float32))
                acc[:t.size] = (acc[:t.size] + t).astype(np.float32)
            w = acc.reshape(4, 64).copy()
            for o in (32, 16, 8, 4, 2, 1):
                w = (w + w[:, np.arange(64) ^ o]).astype(np.float32)
            p = w[:, 0]
            out[c] += float(np.float32(np.float32(p[0] + p[1]) + np.float32(p[2] + p[3])))
    return out


# ---- L1 ----------------------------------------------------------------------------------------------------------------------------
L1_N = (1, 3, 1025, 524289, 2048 * 1024 + 1027)


def l1_slots(n):
    return min(grid_for(n), L1_SLOTS) if n > 0 else 0


def forms_l1(n, gup):
    s = l1_slots(n)
    out = {"l1_finish_kernel", "l1_grad_kernel" + (":gup" if gup else ":no_gup")} if n else {"l1_finish_kernel:n0"}
    if s == 1:
        out.add("l1_sum_kernel:one_slot")
    if s > 1:
        out.add("l1_sum_kernel:slots")
    if s > 64:
        out.add("l1_finish_kernel:second_round")
    if n and grid_for(n) > L1_SLOTS:
        out.add("l1_sum_kernel:slots_capped")
    if n > l1_slots(n) * 256 > 0:
        out.add("l1_sum_kernel:second_iteration")
    if n > min(max(-(-n // 2048), 1), 512) * 4 * 256:
        out.add("l1_grad_kernel:second_iteration")
    return out


def l1_data(n, seed):
    """Gaussian a, b; a == b on a stretch (an exactly zero gradient there); the last difference is 10 (so that leaving it out shows)"""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n >= 1025:
        b[100:200] = a[100:200]
    b[-1] = a[-1] - 10.0
    return a, b


def l1_terms(a, b):
    """|fl32(a - b)| as doubles: what the kernel adds up"""
    return (a - b).abs().double()


def l1_sum(a, b, scale):
    return float((a.double() - b.double()).abs().sum()) * scale


def l1_adds(n):
    s = max(l1_slots(n), 1)
    return -(-n // (s * 256)) + 8 + -(-s // 64) + 6


def l1_bound(n, total_abs, scale):
    """one fp32 rounding of every |a - b|, the fp64 additions, (float)acc and * scale"""
    return (3 * HALF + 4 * 2.0 ** -53 * l1_adds(n)) * total_abs * abs(scale)


def l1_grad(a, b, w, gup):
    """w, -w or +0 by the sign of fl32(a - b), w = fl32(w gup): exact"""
    wf = float(np.float32(w) * np.float32(gup) if gup is not None else np.float32(w))
    d = a - b
    return torch.where(d > 0, wf, 0.0) - torch.where(d < 0, wf, 0.0)


# ---- channel_sum -------------------------------------------------------------------------------------------------------------------
def channel_geometry(x_off, N, C, A, B, ns, cs, as_, bs):
    """channel_sum_geometry: (slots per channel, nseg); nseg != 0: channel_sum_plane_kernel.  x_off: bytes off 16-byte alignment"""
    total, per = N * A * B, A * B
    if bs == 1 and as_ == B and per >= 1024 and ns % 4 == 0 and cs % 4 == 0 and x_off % 16 == 0:
        nseg = per // (4 * 256 * 16)
        want = -(-2048 // (N * C))
        nseg = max(nseg, want)
        nseg = max(1, min(nseg, per // 1024))
        if N * nseg <= 65535:
            return N * nseg, nseg
    return max(1, min(total // 16384, 64)), 0


def forms_channel(x_off, N, C, A, B, ns, cs, as_, bs):
    slots, nseg = channel_geometry(x_off, N, C, A, B, ns, cs, as_, bs)
    per = A * B
    out = {"rfx_slot_sum_kernel<float>"}
    if C % 4:
        out.add("rfx_slot_sum_kernel<float>:partial_workgroup")
    if nseg:
        k = "channel_sum_plane_kernel"
        out.add(k)
        out.add(k + (":nseg_from_want" if -(-2048 // (N * C)) > per // 16384 else ":nseg_from_per"))
        if nseg == per // 1024 and -(-2048 // (N * C)) > nseg:
            out.add(k + ":nseg_clamped")
        seg4 = -(-(per // 4) // nseg)
        if per % 4:
            out.add(k + ":tail")
        if seg4 > 768:
            out.add(k + ":four_load_loop")
        if seg4 % 1024 > 0 and (seg4 <= 768 or seg4 % 1024 != 0):
            out.add(k + ":single_load_loop")
        if nseg > 1:
            out.add(k + ":segments")
    else:
        k = "channel_sum_kernel"
        plane = bs == 1 and as_ == B
        out.add(k + (":plane_layout" if plane else ":strided"))
        out.add(k + (":one_chunk" if slots == 1 else ":chunks"))
        if plane and per >= 1024:
            out.add(k + (":misaligned" if x_off % 16 else ":pitch_not_4"))
    return out


def channel_sum(x4):
    """x4: a strided (N, C, A, B) view -> (sum, sum |x|) per channel in fp64"""
    d = x4.double()
    return d.sum((0, 2, 3)), d.abs().sum((0, 2, 3))


def channel_adds(N, C, A, B, slots, nseg):
    if nseg:
        return 2 + 8 + -(-slots // 64) + 6
    chunk = -(-(N * A * B) // slots)
    return -(-chunk // 256) + 8 + -(-slots // 64) + 6


def channel_bound(x_off, N, C, A, B, ns, cs, as_, bs, sum_abs, const=False):
    slots, nseg = channel_geometry(x_off, N, C, A, B, ns, cs, as_, bs)
    if nseg:
        return k_of("channel_plane_const" if const else "channel_plane") * EPS32 * sum_abs
    return (HALF + 4 * 2.0 ** -53 * channel_adds(N, C, A, B, slots, nseg)) * sum_abs


def restate_channel_plane(plane, nseg):
    """one contiguous (n, c) plane through channel_sum_plane_kernel's decomposition: per segment 256 lanes x four fp32 accumulators over
    16-byte vectors ((v0 + v1) + (v2 + v3) each), the <= 3 values past the last whole vector into a1 of the last segment, then fp64"""
    f = np.float32
    p = np.asarray(plane, np.float32)
    per = p.size
    per4 = per // 4
    seg4 = -(-per4 // nseg)
    v = p[:per4 * 4].reshape(per4, 4)
    vs = ((v[:, 0] + v[:, 1]).astype(f) + (v[:, 2] + v[:, 3]).astype(f)).astype(f)
    total = 0.0
    for sg in range(nseg):
        q0, q1 = sg * seg4, min(sg * seg4 + seg4, per4)
        a = np.zeros((4, 256), f)
        lane = np.arange(256)
        q = q0 + lane
        while True:
            m = q + 768 < q1
            if not m.any():
                break
            for j in range(4):
                a[j, m] = (a[j, m] + vs[q[m] + 256 * j]).astype(f)
            q = np.where(m, q + 1024, q)
        while True:
            m = q < q1
            if not m.any():
                break
            a[0, m] = (a[0, m] + vs[q[m]]).astype(f)
            q = np.where(m, q + 256, q)
        if sg == nseg - 1:
            t = per4 * 4 + lane
            m = t < per
            a[1, m] = (a[1, m] + p[t[m]]).astype(f)
        total += float(((a[0].astype(np.float64) + a[1]) + (a[2].astype(np.float64) + a[3])).sum())
    return total


def _chan_case(name, N, C, A, B, layout="plane", x_off=0, const=False):
    return dict(name=name, N=N, C=C, A=A, B=B, layout=layout, x_off=x_off, const=const)


CHANNEL_CASES = tuple(
    [_chan_case(f"plane{per}_{N}x{C}", N, C, 1, per) for per in (1024, 1027, 16384 + 5) for (N, C) in ((1, 1), (3, 5))] + [
        _chan_case("plane16389_3x683", 3, 683, 1, 16384 + 5),        # N C = 2049: nseg = per / 16384 = 1, four rounds of the four-load loop
        _chan_case("plane1027_const", 3, 5, 13, 79, const=True),     # per = 1027, one channel constant at 1e3
        _chan_case("per1000", 3, 5, 8, 125),                         # plane layout below 1024: strided kernel
        _chan_case("misaligned", 3, 5, 1, 1027, x_off=4),
        _chan_case("contiguous1027", 3, 5, 1, 1027, layout="contiguous"),      # what a contiguous tensor gives: ns, cs not multiples of 4
        _chan_case("pitch_not_4", 3, 5, 1, 1027, layout="pitch"),    # cs % 4 != 0
        _chan_case("transposed", 3, 5, 7, 33, layout="transposed"),
        _chan_case("addfn_view", 3, 15, 1, 65, layout="contiguous"),                    # the contiguous (N, C A, 1, B) view _AddFn.backward builds (C A = 15)
        _chan_case("total100", 1, 3, 4, 25, layout="transposed"),
        _chan_case("total40000", 2, 3, 100, 200, layout="transposed"),
    ])


def channel_view(case, seed):
    """-> (base allocation (1-D fp32, to be placed in a guarded buffer), element offset, sizes, strides (ns, cs, as, bs)).  The view is
    base[off:].as_strided(sizes, strides)."""
    N, C, A, B = case["N"], case["C"], case["A"], case["B"]
    lay = case["layout"]
    off = case["x_off"] // 4
    if lay == "plane":                                            # contiguous planes at a channel pitch that is a multiple of 4
        cs = (A * B + 3) // 4 * 4
        st = (C * cs, cs, B, 1)
        numel = N * C * cs
    elif lay == "contiguous":
        st = (C * A * B, A * B, B, 1)
        numel = N * C * A * B
    elif lay == "pitch":
        cs = A * B + 2                                            # 1029: cs % 4 != 0 while ns % 4 == 0
        st = ((C * cs + 3) // 4 * 4, cs, B, 1)
        numel = N * st[0]
    elif lay == "transposed":                                     # memory (N, C, B, A)
        st = (C * A * B, A * B, 1, A)
        numel = N * C * A * B
    else:
        raise ValueError(lay)
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(off + numel, generator=g)
    view = base[off:].as_strided((N, C, A, B), st)
    view[N - 1, :, A - 1, B - 1] = 1.5                             # the last element of every channel: leaving it out must show
    if case["const"]:
        view[:, 1] = 1e3
    return base, off, (N, C, A, B), st


# ---- add_bcast ---------------------------------------------------------------------------------------------------------------------
def _ab(name, N, C, A, B, ypat, alpha=1.0, off=0):
    return dict(name=name, N=N, C=C, A=A, B=B, ypat=ypat, alpha=alpha, off=off)


ADD_CASES = tuple(
    [_ab(f"flat{t}", 1, 1, 1, t, "same", a) for t, a in ((3, 1.0), (4, -0.5), (1027, 1.0))] + [_ab("flat_offset", 1, 3, 1, 343, "same", -0.5, 1)] +
    [_ab(f"{p}_B{B}", 3, 5, 3, B, p, a) for B, a in ((1, 1.0), (63, -0.5), (256, 1.0), (257, -0.5))
     for p in ("freq_emb", "ncb", "n", "b0", "yb2")])


def add_y(case, seed):
    """-> (y storage, strides (yn, yc, ya, yb)) for the pattern: same shape; (1, C, A, 1) frequency embedding; (N, C, 1, B); (N, 1, 1, 1);
    a stride-0 b on (N, C, A, 1); a non-unit yb on (N, C, A, 2 B)"""
    N, C, A, B = case["N"], case["C"], case["A"], case["B"]
    shape, st = {"same": ((N, C, A, B), (C * A * B, A * B, B, 1)), "freq_emb": ((C, A), (0, A, 1, 0)), "ncb": ((N, C, B), (C * B, B, 0, 1)),
                 "n": ((N,), (1, 0, 0, 0)), "b0": ((N, C, A), (C * A, A, 1, 0)), "yb2": ((N, C, A, 2 * B), (C * A * 2 * B, A * 2 * B, 2 * B, 2))}[case["ypat"]]
    y = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return y, st


def forms_add(case):
    N, C, A, B = case["N"], case["C"], case["A"], case["B"]
    total, rows, per = N * C * A * B, N * C * A, -(-B // 256)
    if case["ypat"] == "same":
        return {"add_flat_kernel" + s[len("k"):] for s in forms_flat("k", total, grid_for(total // 4 + 1))} | {"add_flat_kernel"}
    if rows * per <= 0x7fffffff:
        out = {"add_bcast_rows_kernel"}
        if (rows * per) % 4:
            out.add("add_bcast_rows_kernel:idle_waves")
        if per > 1:
            out.add("add_bcast_rows_kernel:second_chunk")
        if case["ypat"] in ("b0", "freq_emb", "n"):
            out.add("add_bcast_rows_kernel:yb0")
        if case["ypat"] == "yb2":
            out.add("add_bcast_rows_kernel:yb_not_1")
        return out
    return {"add_bcast_kernel"}


def add_bcast(x, y, st, alpha):
    """x (N, C, A, B) + alpha y through the element strides st (0 = broadcast) -> (result, |x| + |alpha y|) in fp64"""
    yv = y.reshape(-1).as_strided(x.shape, st).double()
    return x.double() + alpha * yv, x.double().abs() + (alpha * yv).abs()


# ---- span_mask ---------------------------------------------------------------------------------------------------------------------
SPAN_CASES = (
    # frequency span inside / empty / all of F; time span longer than the 256-thread stride (row 0 is in both), t1 > T (not on the last
    # row: a missing clamp then lands in the next row of the tensor), empty
    dict(R=3, F=5, T=300, f0=(1, 3, 0), f1=(3, 3, 5), t0=(10, 250, 50), t1=(290, 400, 50)),
    dict(R=3, F=5, T=300, f0=(4, 2, 0), f1=(2, 4, 1), t0=(-7, 120, 299), t1=(20, 100, 300)),        # t0 < 0; empty; the last sample
    dict(R=1, F=1, T=1, f0=(0,), f1=(0,), t0=(0,), t1=(1,)),
    dict(R=1, F=1, T=1, f0=(0,), f1=(1,), t0=(5,), t1=(9,)),
)


def forms_span(c):
    out = {"span_mask_kernel"}
    for r in range(c["R"]):
        f0, f1, t0, t1 = c["f0"][r], c["f1"][r], c["t0"][r], c["t1"][r]
        out.add("span_mask_kernel:freq_empty" if f1 <= f0 else ("span_mask_kernel:freq_all" if f0 <= 0 and f1 >= c["F"] else "span_mask_kernel:freq_inside"))
        if f0 <= 0 and f1 >= c["F"]:
            continue                                                 # every row of the sample is a frequency row: the time span is not read
        if t1 <= t0:
            out.add("span_mask_kernel:time_empty")
        elif t0 < 0:
            out.add("span_mask_kernel:t0_clamped")
        elif t1 > c["T"]:
            out.add("span_mask_kernel:t1_clamped")
        else:
            out.add("span_mask_kernel:time_inside")
        if min(t1, c["T"]) - max(t0, 0) > 256:
            out.add("span_mask_kernel:second_stride")
        if f1 > f0 and t1 > t0:
            out.add("span_mask_kernel:row_in_both")
    return out


def span_mask(c):
    """boolean (R, F, T): True where the element is zeroed"""
    f = torch.arange(c["F"]).view(1, -1, 1)
    t = torch.arange(c["T"]).view(1, 1, -1)
    v = lambda k: torch.tensor(c[k]).view(-1, 1, 1)                  # noqa: E731
    return ((f >= v("f0")) & (f < v("f1"))) | ((t >= v("t0")) & (t < v("t1")))


# ---- blstm_frames ------------------------------------------------------------------------------------------------------------------
#               B  C  T     nfr width stride
BLSTM_CASES = ((2, 3, 23, 6, 8, 4), (1, 2, 20, 7, 7, 3), (3, 1, 5, 1, 5, 5), (2, 2, 1000, 10, 200, 100), (2, 2, 9, 5, 8, 4))


def forms_blstm(case, mode, skip):
    B, C, T, nfr, width, stride = case
    out = {f"blstm_frames_kernel:mode{mode}"}
    if mode == 2 and skip:
        out.add("blstm_frames_kernel:skip")
    if mode in (0, 3) and (nfr - 1) * stride + width > T:
        out.add("blstm_frames_kernel:zero_beyond_T")
    if T < (nfr - 1) * stride:
        out.add("blstm_frames_kernel:whole_frames_of_padding")
    if stride % 2:
        out.add("blstm_frames_kernel:odd_stride")
    if nfr == 1:
        out.add("blstm_frames_kernel:one_frame")
    return out


def stitch_frame(tau, nfr, stride):
    return min(max((tau - stride // 2) // stride, 0), nfr - 1)


def blstm_frames(src, skip, case, mode):
    """explicit loops over (k, t) (all b, c at once).  h is (C, width, B, nfr): position t Bn + b nfr + k of channel c; x is (B, C, T).
    -> (result, sum |terms|, number of terms) in fp64"""
    B, C, T, nfr, width, stride = case
    s = src.double()
    if mode in (0, 3):
        x = s.view(B, C, T)
        h = torch.zeros(C, width, B, nfr, dtype=torch.float64)
        for k in range(nfr):
            for t in range(width):
                tau = k * stride + t
                if tau < T and (mode == 0 or stitch_frame(tau, nfr, stride) == k):
                    h[:, t, :, k] = x[:, :, tau].t()
        return h, h.abs(), torch.ones_like(h)
    h = s.view(C, width, B, nfr)
    x = torch.zeros(B, C, T, dtype=torch.float64)
    mag, cnt = torch.zeros_like(x), torch.zeros_like(x)
    for tau in range(T):
        ks = range(nfr) if mode == 1 else (stitch_frame(tau, nfr, stride),)
        for k in ks:
            t = tau - k * stride
            if 0 <= t < width:
                x[:, :, tau] += h[:, t, :, k].t()
                mag[:, :, tau] += h[:, t, :, k].t().abs()
                cnt[:, :, tau] += 1
    if mode == 2 and skip is not None:
        x = x + skip.double().view(B, C, T)
        mag = mag + skip.double().view(B, C, T).abs()
    return x, mag, cnt


def blstm_bound(case, mode, skip, ref, mag):
    B, C, T, nfr, width, stride = case
    if mode == 1:
        return (-(-width // stride) - 1) * HALF * mag
    if mode == 2 and skip:
        return HALF * ref.abs()
    return torch.zeros_like(ref)


# ---- row_moments / row_affine ------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = ((1, 2), (3, 255), (5, 16385), (2, 40001))
AFFINE_SHAPES = ((1, 1), (13, 79), (3, 699393))                     # totals 1, 1027, 2 098 179
MOMENT_EPS = 1e-5


def moments_slots(L):
    return min(max(-(-L // 16384), 1), 256)


def forms_moments(R, L, coef):
    s = moments_slots(L)
    out = {"row_moments_kernel:" + ("one_slot" if s == 1 else "two_slots" if s == 2 else "slots"), "row_moments_finalize_kernel"}
    if R % 4:
        out.add("row_moments_finalize_kernel:partial_workgroup")
    out.add("row_moments_finalize_kernel:" + ("coef" if coef else "no_coef"))
    if L > s * 256:
        out.add("row_moments_kernel:second_iteration")
    return out


def forms_affine(R, L, b):
    out = {"row_affine_kernel:" + ("b" if b else "no_b")}
    if R * L > grid_for(R * L) * 256:
        out.add("row_affine_kernel:second_iteration")
    return out


def moments_data(R, L, seed):
    """Gaussian rows; row 1 (if any) has mean / std = 1e3; the last row of R >= 3 is constant at 0.75 (every sum exact in fp64: std == 0)"""
    x = torch.randn(R, L, generator=torch.Generator().manual_seed(seed))
    if R >= 2:
        x[1] += 1e3
    if R >= 3:
        x[R - 1] = 0.75
    return x


def row_moments(x):
    """-> mean, unbiased std, and their bounds, in fp64"""
    R, L = x.shape
    d = x.double()
    m = d.mean(1)
    var = ((d - m[:, None]) ** 2).sum(1) / (L - 1)
    std = var.sqrt()
    s = moments_slots(L)
    adds = -(-L // (s * 256)) + 8 + -(-s // 64) + 6
    u = 4 * 2.0 ** -53 * adds
    bm = HALF * m.abs() + u * d.abs().sum(1) / L
    s2 = (d * d).sum(1)
    dvar = u * (s2 + L * m * m) / (L - 1) + 2 * (bm - HALF * m.abs()) * m.abs() * L / (L - 1)
    bs = HALF * std + torch.maximum(std - (var - dvar).clamp_min(0).sqrt(), (var + dvar).sqrt() - std)
    return m, std, bm, bs


def moments_coef(mean32, std32, eps):
    """a = 1 / (eps + std), b = -mean a from the fp32 mean / std the kernel stored -> a, b, bound a (3 half-ulps), bound b (4)"""
    a = 1.0 / (f32(eps) + std32.double())
    b = -mean32.double() * a
    return a, b, 3 * HALF * a.abs(), 4 * HALF * b.abs()


def row_affine(x, a, b):
    """-> (x a + b, |x a| + |b|) in fp64; b None: x a + 0"""
    t = x.double() * a.double()[:, None]
    bb = b.double()[:, None] if b is not None else torch.zeros(1, 1, dtype=torch.float64)
    return t + bb, t.abs() + bb.abs()


# ---- dropout -----------------------------------------------------------------------------------------------------------------------
DROPOUT_N = (1, 255, 257, 2097152 + 259)
DROPOUT_P = (0.0, 0.1, 0.5, 0.999)
DROPOUT_SEEDS = (12345, 0xF123456789ABCDEF)
M64 = (1 << 64) - 1


def dropout_u24_int(seed, i):
    """the draw in Python ints: splitmix64 of seed + golden (i + 1), top 24 bits"""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 40


def dropout_u24(seed, n):
    """the same for i = 0 ... n - 1 in wrapping uint64 arithmetic"""
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (z >> np.uint64(40)).astype(np.int64)


def dropout_keep(seed, n, p):
    """u24 / 2^24 >= p with p the float the ABI carries (both sides exact in fp64)"""
    return torch.from_numpy(dropout_u24(seed, n).astype(np.float64) / 16777216.0 >= float(np.float32(p)))


def dropout(x, p, seed):
    """kept values fl32(x fl32(1 / (1 - p))), dropped ones +0: exact"""
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    keep = dropout_keep(seed, x.numel(), p)
    return torch.where(keep, (x.double() * float(inv)).float(), torch.zeros_like(x)), keep


def forms_dropout(n, p):
    out = {"dropout_kernel"}
    if -(-n // 256) > 8192:
        out.update(("dropout_kernel:grid_capped", "dropout_kernel:second_iteration"))
    if p == 0.0:
        out.add("dropout_kernel:p0")
    return out


# ---- every form --------------------------------------------------------------------------------------------------------------------
UNREACHABLE = {"add_bcast_kernel"}            # the 64-bit fallback: rows * ceil(B / 256) > 2^31 - 1, more than 8 GiB per tensor


def all_forms():
    out = set(UNREACHABLE)
    for k in FLAT_KERNELS:
        out.update(k + s for s in (":vec", ":tail", ":second_iteration", ":grid_capped"))
    for v in ("vec", "scalar"):
        for t in ("bf16", "f32"):
            for d in ("fwd", "bwd"):
                out.add(f"act_rows_kernel<{v},{t}>:{d}")
    out.update("act_rows_kernel:" + s for s in ("idle_waves", "second_chunk", "vec_partial_chunk"))
    out.update("mul_kernel:" + s for s in ("vec", "tail", "grid_capped", "second_iteration"))
    out.update(("prelu_fwd_kernel", "prelu_bwd_kernel", "prelu_fwd_kernel:second_iteration", "prelu_bwd_kernel:second_iteration",
                "prelu_bwd_kernel:idle_lanes", "rfx_slot_sum_kernel<float>", "rfx_slot_sum_kernel<float>:partial_workgroup"))
    out.update(("l1_finish_kernel", "l1_finish_kernel:n0", "l1_finish_kernel:second_round", "l1_sum_kernel:one_slot", "l1_sum_kernel:slots",
                "l1_sum_kernel:slots_capped", "l1_sum_kernel:second_iteration", "l1_grad_kernel:gup", "l1_grad_kernel:no_gup",
                "l1_grad_kernel:second_iteration"))
    out.update(("channel_sum_plane_kernel",) + tuple("channel_sum_plane_kernel:" + s for s in (
        "nseg_from_want", "nseg_from_per", "nseg_clamped", "tail", "four_load_loop", "single_load_loop", "segments")))
    out.update("channel_sum_kernel:" + s for s in ("plane_layout", "strided", "one_chunk", "chunks", "misaligned", "pitch_not_4"))
    out.update(("add_flat_kernel", "add_flat_kernel:vec", "add_flat_kernel:tail", "add_flat_kernel:second_iteration", "add_bcast_rows_kernel", "add_bcast_rows_kernel:idle_waves",
                "add_bcast_rows_kernel:second_chunk", "add_bcast_rows_kernel:yb0", "add_bcast_rows_kernel:yb_not_1"))
    out.update(("span_mask_kernel",) + tuple("span_mask_kernel:" + s for s in (
        "freq_empty", "freq_all", "freq_inside", "time_empty", "t0_clamped", "t1_clamped", "time_inside", "second_stride", "row_in_both")))
    out.update("blstm_frames_kernel:" + s for s in ("mode0", "mode1", "mode2", "mode3", "skip", "zero_beyond_T", "whole_frames_of_padding",
                                                      "odd_stride", "one_frame"))
    out.update(("row_moments_kernel:one_slot", "row_moments_kernel:two_slots", "row_moments_kernel:slots", "row_moments_kernel:second_iteration",
                "row_moments_finalize_kernel", "row_moments_finalize_kernel:partial_workgroup", "row_moments_finalize_kernel:coef",
                "row_moments_finalize_kernel:no_coef", "row_affine_kernel:b", "row_affine_kernel:no_b", "row_affine_kernel:second_iteration"))
    out.update(("dropout_kernel", "dropout_kernel:grid_capped", "dropout_kernel:second_iteration", "dropout_kernel:p0"))
    return out


def rows_layout(D, T, x16=False, falsify=None):
    """the HDemucs layout of ops.ActToFn: x (D0, D1, D2, T) contiguous, out in (D0, D2, D1) row order at a row pitch of T + 4 (NaN in the
    gaps).  falsify: 'stride' makes x's D2 stride = 2 mod 4 (row pitch T + 2); 'x' / 'out' / 'gy' move that pointer 4 bytes.
    -> dict(xs, os, gs, x_len, out_len, x_off, out_off, gy_off) with lengths in elements and offsets in bytes"""
    px = T + 2 if falsify == "stride" else T
    po = T + 4
    xs = (D[1] * D[2] * px, D[2] * px, px)
    os_ = (D[2] * D[1] * po, po, D[1] * po)
    off = lambda w, esize: (4 // esize if falsify == w else 0)        # noqa: E731
    return dict(xs=xs, os=os_, gs=os_, x_len=D[0] * xs[0], out_len=D[0] * os_[0], x_off=off("x", 2 if x16 else 4), out_off=off("out", 4),
                gy_off=off("gy", 4), px=px, po=po)


def walk_all_cases():
    """every case table through its forms function -> the union"""
    out = set()
    for k in FLAT_KERNELS:
        for n in FLAT_N:
            out |= forms_flat(k, n)
    for x16 in (False, True):
        for bwd in (False, True):
            for D in ROWS_D:
                for T in ROWS_T_VEC + ROWS_T_SCALAR:
                    lay = rows_layout(D, T, x16)
                    out |= forms_rows(x16, bwd, D, T, lay["xs"] + lay["os"] + (lay["gs"] if bwd else ()))
            for fal in ROWS_FALSIFY:
                if fal == "gy" and not bwd:
                    continue
                lay = rows_layout(ROWS_D[0], 256, x16, fal)
                out |= forms_rows(x16, bwd, ROWS_D[0], 256, lay["xs"] + lay["os"] + (lay["gs"] if bwd else ()),
                                  lay["x_off"] * (2 if x16 else 4), lay["out_off"] * (2 if (x16 and bwd) else 4), lay["gy_off"] * 4)
    for n in MUL_N:
        out |= forms_mul(n)
    for s in PRELU_SHAPES:
        out |= forms_prelu(*s)
    for n in (0,) + L1_N:
        for gup in (False, True):
            out |= forms_l1(n, gup)
    for c in CHANNEL_CASES:
        _, _, (N, C, A, B), st = channel_view(c, 0)
        out |= forms_channel(c["x_off"], N, C, A, B, *st)
    for c in ADD_CASES:
        out |= forms_add(c)
    for c in SPAN_CASES:
        out |= forms_span(c)
    for c in BLSTM_CASES:
        for mode in range(4):
            for skip in (False, True):
                out |= forms_blstm(c, mode, skip)
    for (R, L) in MOMENT_SHAPES:
        for coef in (False, True):
            out |= forms_moments(R, L, coef)
    for (R, L) in AFFINE_SHAPES:
        for b in (False, True):
            out |= forms_affine(R, L, b)
    for n in DROPOUT_N:
        for p in DROPOUT_P:
            out |= forms_dropout(n, p)
    return out


# ---- rfx_zero (csrc/optim.hip: zero_kernel) ----------------------------------------------------------------------------------------------
# nbytes a multiple of 4 at a 4-byte aligned base; anything else is refused and nothing is written.  The kernel stores up to 3 head words
# to reach a 16-byte boundary, 16-byte vectors in a grid-stride loop, and up to 3 tail words; the grid is capped at 16384 workgroups
# of 256 threads, one workgroup per 4096 words.
ZERO_GRID_CAP_WORDS = 16384 * 4096
ZERO_BYTES = (0, 1, 3, 4, 15, 16, 17, 20, 64, 4099, 4100, 16 * 4096 + 28)     # the issue's counts, and word counts with a body and a tail
ZERO_BYTES_CAP = 4 * (ZERO_GRID_CAP_WORDS + 9)                  # one workgroup more than the cap holds; from a base one word on: head 3, tail 2
ZERO_WORD_OFFSETS = (0, 1, 2, 3)                                 # base past a 16-byte boundary, in words: head of 0, 3, 2, 1 words


def forms_zero(nbytes, byte_off=0):
    """branches of one rfx_zero call at a base `byte_off` bytes past a 16-byte boundary; None: refused; empty: accepted, nothing launched"""
    if nbytes < 0 or nbytes % 4 or byte_off % 4:
        return None
    n = nbytes // 4
    if n == 0:
        return set()
    head = min(((16 - byte_off % 16) % 16) // 4, n)
    n4 = (n - head) // 4
    out = set()
    if head:
        out.add("head")
    if n4:
        out.add("vec")
    if n - head - 4 * n4:
        out.add("tail")
    grid = min(max(-(-n // 4096), 1), 16384)
    if n4 > grid * 256:
        out.add("second_iteration")
    if -(-n // 4096) > 16384:
        out.add("grid_capped")
    return out
