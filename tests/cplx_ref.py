"""Plain torch, fp64, CPU restatement of the kernels of remfx_amd/csrc/cplx.hip in the interface of their C ABI (rfx_cplx_moments,
rfx_cplx_coef_fwd / _bwd, rfx_cplx_affine_act_fwd / _bwd, rfx_cplx_moments_bwd, rfx_bound_mask_fwd / _bwd, rfx_phase_mask_fwd / _bwd).
Closed forms, no autograd; tests/test_cplx_ref_cpu.py ties them to oracle.ref_dcunet and to torch's float64 autograd.

A complex tensor is stacked: x (N, 2C, S), channels [0, C) the real parts, [C, 2C) the imaginary parts.  Per-channel vectors are
(k, C) in the kernels' row order: coef / gcoef (6, C) = Zrr, Zri, Zir, Zii, Br', Bi'; stats / running / cm (5, C) = Mr, Mi, Vrr, Vri, Vii
(cm: d / d raw moment q, times inv); gw (5, C) = d / d Wrr, Wri, Wii, Br, Bi; sums (C, 5) = sum xr, xi, xr^2, xr xi, xi^2.

Every stage TAKES the previous stage's result (sums, stats, coef, gcoef, cm): the GPU test feeds each kernel's reference the device's
own fp32 / fp64 intermediates, so every kernel is judged alone.

The bound of every output is  K * eps32 * magnitude (+ slack),  K = MARGIN * floor + FP32_HALF_ULPS / 2  (DESIGN.md 4.15, 4.20):
  magnitude  per element, the sum of the absolute values of the terms it is formed from, carried through the later operations at
             first order -- for coef that makes it condition-aware: delta = Vrr Vii - Vri^2 enters with |Vrr Vii| + |Vri^2|, which at a
             correlation of 0.999 is 1000 delta.
  floor      the same formulas in float32 on the CPU with the kernels' partial sums (`floors_*`), in units of eps32 * magnitude.  Never
             measured on the kernel.
  slack      leaky ReLU: where |u| <= U_BAND eps32 mag(u) the sign of u is inside u's own error; such an element gets
             |gy| (1 - slope) of absolute slack through the same sums (and (1 - slope) of u's own bound forward)."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.ref_common import EPS32, f32, worst  # noqa: F401

CHUNK = 4096                      # CX_CHUNK
MARGIN = 8.0
FP32_HALF_ULPS = 16
U_BAND = 32.0                     # as DESIGN.md 4.15
GEN_EPS = 1e-5
SLOPE = 0.01
MOMENTUM = 0.1
GRID_CAP = 4096 * 1024            # cx_grid: 4096 workgroups x 256 threads x 4 -- above it the grid-stride loops iterate
MASK_SMALL = 1e-2                 # below it tanh(a) / a and its derivative come from series (no cancelling quotient)


def k_of(floor):
    return MARGIN * floor + FP32_HALF_ULPS / 2


def floor_of(x32, ref, mag, slack=0.0):
    e = ((x32.double() - ref).abs() - slack).clamp_min(0)
    return float((e / (EPS32 * mag).clamp_min(1e-300)).max()) if e.numel() else 0.0


def halves(x):
    C = x.shape[1] // 2
    return x[:, :C], x[:, C:]


# ---- sizing rules and slot layouts, restated ----------------------------------------------------------------------------------------
def nchunks(S):
    return -(-S // CHUNK)


def slots(N, S):
    """slots per channel behind rfx_cplx_moments_ws / rfx_cplx_affine_act_bwd_ws: one per (sample, 4096-value chunk) and channel"""
    return -1 if N <= 0 or S <= 0 else N * nchunks(S)


def moments_ws(N, C, S):
    """doubles of rfx_cplx_moments' ws, laid out [c][n][chunk][5]"""
    return 5 * C * slots(N, S)


def affine_bwd_ws(N, C, S):
    """doubles of rfx_cplx_affine_act_bwd's ws, laid out [6][C][N * nchunks]"""
    return 6 * C * slots(N, S)


def mask_grid(total):
    """(workgroups, grid-stride iterations of the busiest thread) of cx_grid"""
    b = min(max(-(-total // 1024), 1), 4096)
    return b, -(-total // (b * 256))


# ---- the kernels' partial sums in fp32 ------------------------------------------------------------------------------------------------
def _chunk_lanes(t):
    """(..., L) -> (..., nchunks, 64): per-lane partial sums of every 4096-value chunk, lane l adds l, l + 64, ... in order"""
    L = t.shape[-1]
    nfull = L // CHUNK
    parts = []
    if nfull:
        parts.append(t[..., :nfull * CHUNK].reshape(*t.shape[:-1], nfull, CHUNK // 64, 64))
    if L > nfull * CHUNK:
        tail = t[..., nfull * CHUNK:]
        tail = F.pad(tail, (0, (-tail.shape[-1]) % 64))
        parts.append(tail.reshape(*t.shape[:-1], 1, -1, 64))
    out = []
    for p in parts:
        acc = p[..., 0, :].clone()
        for i in range(1, p.shape[-2]):
            acc = acc + p[..., i, :]
        out.append(acc)
    return torch.cat(out, -2)


def _butterfly(acc):
    w = 32
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def _sum_ncs(t, dtype_lanes):
    """(N, C, S) -> (C,) fp64.  dtype_lanes None: exact.  float32: fp32 lane partials; "wide": widened ahead of the butterfly (moments);
    "narrow": fp32 butterfly, then widened (affine_act_bwd).  Chunk sums are added in fp64 in slot order (n, chunk)."""
    if dtype_lanes is None:
        return t.double().sum((0, 2))
    lanes = _chunk_lanes(t.float())                             # (N, C, nch, 64)
    per = _butterfly(lanes.double()) if dtype_lanes == "wide" else _butterfly(lanes).double()
    return per.permute(1, 0, 2).reshape(t.shape[1], -1).sum(1)


# ---- statistics -------------------------------------------------------------------------------------------------------------------------
def moments(x, lanes=None):
    """(C, 5) fp64: the five raw sums per channel"""
    xr, xi = halves(x if lanes else x.double())
    return torch.stack([_sum_ncs(t, lanes) for t in (xr, xi, xr * xr, xr * xi, xi * xi)], 1)


def moments_mag(x):
    xr, xi = halves(x.double().abs())
    return torch.stack([t.sum((0, 2)) for t in (xr, xi, xr * xr, xr * xi, xi * xi)], 1)


def stats_of(sums, inv):
    """(5, C) fp64 from the raw sums: E[.] - mean products (cx_stats ahead of its rounding to fp32)"""
    m0, m1 = sums[:, 0] * inv, sums[:, 1] * inv
    return torch.stack([m0, m1, sums[:, 2] * inv - m0 * m0, sums[:, 3] * inv - m0 * m1, sums[:, 4] * inv - m1 * m1])


def stats_mag(sums, inv):
    """|value| plus what the fp64 cancellation E[x^2] - m^2 leaves (2^-26 eps32 = 8 eps64 of its two terms)"""
    m0, m1 = sums[:, 0] * inv, sums[:, 1] * inv
    st = stats_of(sums, inv).abs()
    c = 2.0 ** -26
    extra = torch.stack([0 * m0, 0 * m1, (sums[:, 2] * inv).abs() + m0 * m0, (sums[:, 3] * inv).abs() + (m0 * m1).abs(),
                         (sums[:, 4] * inv).abs() + m1 * m1])
    return st + c * extra


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------
def _whiten(st, eps, dt, v32=False):
    """U = V^{-1/2} of the 2x2 covariance with eps on its diagonal; v32: Vrr / Vii formed by an fp32 addition (what the kernels do)"""
    e = eps                                                     # callers pass f32(eps), the value the ABI carries
    if v32:
        Vrr, Vii = (st[2].float() + torch.tensor(e, dtype=torch.float32)).to(dt), (st[4].float() + torch.tensor(e, dtype=torch.float32)).to(dt)
    else:
        Vrr, Vii = st[2].to(dt) + e, st[4].to(dt) + e
    Vri = st[3].to(dt)
    tau, delta = Vrr + Vii, Vrr * Vii - Vri * Vri
    s = delta.sqrt()
    t = (tau + 2 * s).sqrt()
    rst = 1 / (s * t)
    return dict(Vrr=Vrr, Vri=Vri, Vii=Vii, s=s, t=t, rst=rst, Urr=(s + Vii) * rst, Uii=(s + Vrr) * rst, Uri=-Vri * rst)


def coef_fwd(stats, W, B, eps=GEN_EPS, running=None, momentum=MOMENTUM, dtype=torch.float64, v32=False):
    """stats: (5, C), or (sums (C, 5), inv).  W = (Wrr, Wri, Wii), B = (Br, Bi).  -> coef (6, C), stats (5, C), running' (5, C) or None.
    dtype float32 is the kernel's algorithm: statistics from the fp64 sums, rounded once, everything after in fp32.
    v32 (the GPU test's setting, with stats = the fp32 statistics the kernel stored): Vrr / Vii = fl32(st + eps), the point the kernel
    whitens at -- the statistics are judged against the fp64 sums on their own, the coefficients as a function of them."""
    st = stats_of(*stats) if isinstance(stats, tuple) else stats.double()
    st = st.to(dtype)
    u = _whiten(st, eps, dtype, v32=v32 or dtype == torch.float32)
    Wrr, Wri, Wii = (w.to(dtype) for w in W)
    Zrr, Zri = Wrr * u["Urr"] + Wri * u["Uri"], Wrr * u["Uri"] + Wri * u["Uii"]
    Zir, Zii = Wri * u["Urr"] + Wii * u["Uri"], Wri * u["Uri"] + Wii * u["Uii"]
    coef = torch.stack([Zrr, Zri, Zir, Zii, B[0].to(dtype) - (Zrr * st[0] + Zri * st[1]), B[1].to(dtype) - (Zir * st[0] + Zii * st[1])])
    run = None
    if running is not None:
        r = running.to(dtype)
        run = r + torch.tensor(f32(momentum), dtype=dtype) * (st - r)
    return coef, st, run


def _z_of(u0, W, dl):
    """Z (4, C) with delta scaled by 1 + dl"""
    Vrr, Vri, Vii = u0["Vrr"], u0["Vri"], u0["Vii"]
    s = ((Vrr * Vii - Vri * Vri) * (1 + dl)).sqrt()
    rst = 1 / (s * (Vrr + Vii + 2 * s).sqrt())
    Urr, Uii, Uri = (s + Vii) * rst, (s + Vrr) * rst, -Vri * rst
    Wrr, Wri, Wii = (w.double() for w in W)
    return torch.stack([Wrr * Urr + Wri * Uri, Wrr * Uri + Wri * Uii, Wri * Urr + Wii * Uri, Wri * Uri + Wii * Uii])


def coef_mag(stats, W, B, eps=GEN_EPS, running=None, momentum=MOMENTUM, v32=False):
    """magnitudes of coef (6, C) and running' (5, C).  Condition-aware: delta = Vrr Vii - Vri^2 is formed from two terms of magnitude
    |Vrr Vii| + Vri^2 (1000 delta at a correlation of 0.999) and reaches every Z through s and 1 / (s t), which all four share -- so it
    enters with |dZ / d log delta| (a central difference in fp64), not with the sum of the |W U| products; those, the terms Z is
    finally added up from, count twice (s + V, the product with rst, the product with W, the sum).  B' = B - Z M carries mag(Z) |M|."""
    st = stats_of(*stats) if isinstance(stats, tuple) else stats.double()
    u = _whiten(st, eps, torch.float64, v32)
    h = 1e-6
    dz = (_z_of(u, W, h) - _z_of(u, W, -h)).abs() / (2 * h)
    cond = ((u["Vrr"] * u["Vii"]).abs() + u["Vri"] * u["Vri"]) / (u["Vrr"] * u["Vii"] - u["Vri"] * u["Vri"])
    Wrr, Wri, Wii = (w.double().abs() for w in W)
    Urr, Uii, Uri = u["Urr"].abs(), u["Uii"].abs(), u["Uri"].abs()
    local = torch.stack([Wrr * Urr + Wri * Uri, Wrr * Uri + Wri * Uii, Wri * Urr + Wii * Uri, Wri * Uri + Wii * Uii])
    mz = dz * cond + 2 * local
    a0, a1 = st[0].abs(), st[1].abs()
    mag = torch.cat([mz, torch.stack([B[0].double().abs() + mz[0] * a0 + mz[1] * a1, B[1].double().abs() + mz[2] * a0 + mz[3] * a1])])
    mrun = None
    if running is not None:
        r = running.double().abs()
        mrun = r + f32(momentum) * (st.abs() + r)
    return mag, mrun


def coef_bwd(stats, W, eps, gcoef, inv=None, v32=False):
    """reverse mode of coef_fwd by hand, fp64.  stats (5, C); gcoef (6, C).  -> gw (5, C), cm (5, C) (training: inv given) or None.
    v32: the derivative is taken where the kernels' forward was evaluated, Vrr = fl32(st2 + eps) -- the GPU test's setting."""
    st, g = stats.double(), gcoef.double()
    u = _whiten(st, eps, torch.float64, v32)
    Vrr, Vri, Vii, s, t, rst, Urr, Uii, Uri = (u[k] for k in ("Vrr", "Vri", "Vii", "s", "t", "rst", "Urr", "Uii", "Uri"))
    Wrr, Wri, Wii = (w.double() for w in W)
    Mr, Mi = st[0], st[1]
    Zrr, Zri = Wrr * Urr + Wri * Uri, Wrr * Uri + Wri * Uii
    Zir, Zii = Wri * Urr + Wii * Uri, Wri * Uri + Wii * Uii
    gB0, gB1 = g[4], g[5]
    gZrr, gZri, gZir, gZii = g[0] - gB0 * Mr, g[1] - gB0 * Mi, g[2] - gB1 * Mr, g[3] - gB1 * Mi
    gw = torch.stack([gZrr * Urr + gZri * Uri, gZrr * Uri + gZri * Uii + gZir * Urr + gZii * Uri, gZir * Uri + gZii * Uii, gB0, gB1])
    if inv is None:
        return gw, None
    gMr, gMi = -(gB0 * Zrr + gB1 * Zir), -(gB0 * Zri + gB1 * Zii)
    gUrr = gZrr * Wrr + gZir * Wri
    gUri = gZrr * Wri + gZri * Wrr + gZir * Wii + gZii * Wri
    gUii = gZri * Wri + gZii * Wii
    # U = (s + V') / (s t): d/dV', d/ds, d/d(s t)
    gVii, gVrr, gVri = gUrr * rst, gUii * rst, -gUri * rst
    gs = (gUrr + gUii) * rst
    gst = -(gUrr * (s + Vii) + gUii * (s + Vrr) - gUri * Vri) * rst * rst
    gs = gs + gst * t
    gtau = gst * s / (2 * t)                                    # t = sqrt(tau + 2 s)
    gs = gs + 2 * gtau
    gdelta = gs / (2 * s)
    gVrr = gVrr + gdelta * Vii + gtau
    gVii = gVii + gdelta * Vrr + gtau
    gVri = gVri - 2 * gdelta * Vri
    cm = torch.stack([gMr - 2 * Mr * gVrr - Mi * gVri, gMi - 2 * Mi * gVii - Mr * gVri, gVrr, gVri, gVii]) * inv
    return gw, cm


def coef_bwd_mag(ref):
    """the kernel evaluates this stage in fp64 on the inputs the reference gets: what is left is the rounding of the result"""
    return ref.abs()


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def _u(x, coef):
    a, b = halves(x)
    k = [c.to(x.dtype).view(1, -1, 1) for c in coef]
    return a, b, k, k[0] * a + k[1] * b + k[4], k[2] * a + k[3] * b + k[5]


def _u_mag(x, coef):
    a, b = halves(x.double().abs())
    k = [c.double().abs().view(1, -1, 1) for c in coef]
    return k[0] * a + k[1] * b + k[4], k[2] * a + k[3] * b + k[5]


def affine_act(x, coef, slope=SLOPE):
    """y (N, 2C, S) = leaky_relu(Z x + B') in the dtype of x"""
    _, _, _, ur, ui = _u(x, coef)
    sl = torch.tensor(f32(slope), dtype=x.dtype)
    return torch.cat([torch.where(ur >= 0, ur, sl * ur), torch.where(ui >= 0, ui, sl * ui)], 1)


def band(x, coef):
    """(N, 2C, S) bool: |u| <= U_BAND eps32 mag(u), the sign of u is undetermined"""
    x = x.double()
    _, _, _, ur, ui = _u(x, [c.double() for c in coef])
    mr, mi = _u_mag(x, coef)
    return torch.cat([ur.abs() <= U_BAND * EPS32 * mr, ui.abs() <= U_BAND * EPS32 * mi], 1)


def affine_act_mag(x, coef, slope=SLOPE):
    """(magnitude, slack) of y"""
    mag = torch.cat(_u_mag(x, coef), 1)
    return mag, band(x, coef).double() * (U_BAND * EPS32 * (1 - f32(slope))) * mag


def affine_act_bwd(x, coef, gy, slope=SLOPE, lanes=None):
    """gx (N, 2C, S) in the dtype of x, gcoef (6, C) fp64"""
    a, b, k, ur, ui = _u(x, coef)
    one, sl = torch.tensor(1.0, dtype=x.dtype), torch.tensor(f32(slope), dtype=x.dtype)
    gyr, gyi = halves(gy.to(x.dtype))
    gr, gi = gyr * torch.where(ur >= 0, one, sl), gyi * torch.where(ui >= 0, one, sl)
    gx = torch.cat([k[0] * gr + k[2] * gi, k[1] * gr + k[3] * gi], 1)
    gcoef = torch.stack([_sum_ncs(t, lanes) for t in (gr * a, gr * b, gi * a, gi * b, gr, gi)])
    return gx, gcoef


def affine_act_bwd_mag(x, coef, gy, slope=SLOPE):
    """({gx, gcoef}: magnitude, {gx, gcoef}: slack)"""
    x = x.double()
    a, b = halves(x.abs())
    _, _, _, ur, ui = _u(x, [c.double() for c in coef])
    k = [c.double().abs().view(1, -1, 1) for c in coef]
    sl = f32(slope)
    gyr, gyi = halves(gy.double().abs())
    one, slt = torch.tensor(1.0, dtype=torch.float64), torch.tensor(sl, dtype=torch.float64)
    gr, gi = gyr * torch.where(ur >= 0, one, slt), gyi * torch.where(ui >= 0, one, slt)
    bd = band(x, coef).double()
    C = x.shape[1] // 2
    sr, si = gyr * bd[:, :C] * (1 - sl), gyi * bd[:, C:] * (1 - sl)

    def both(p, q):
        return (torch.cat([k[0] * p + k[2] * q, k[1] * p + k[3] * q], 1),
                torch.stack([t.sum((0, 2)) for t in (p * a, p * b, q * a, q * b, p, q)]))
    mgx, mgc = both(gr, gi)
    sgx, sgc = both(sr, si)
    return {"gx": mgx, "gcoef": mgc}, {"gx": sgx, "gcoef": sgc}


def moments_bwd(x, cm):
    """the increment rfx_cplx_moments_bwd adds to gx: d(sum_q cm_q moment_q) / dx"""
    a, b = halves(x)
    k = [c.to(x.dtype).view(1, -1, 1) for c in cm]
    return torch.cat([k[0] + 2 * k[2] * a + k[3] * b, k[1] + 2 * k[4] * b + k[3] * a], 1)


def moments_bwd_mag(x, cm, gx0):
    a, b = halves(x.double().abs())
    k = [c.double().abs().view(1, -1, 1) for c in cm]
    return gx0.double().abs() + torch.cat([k[0] + 2 * k[2] * a + k[3] * b, k[1] + 2 * k[4] * b + k[3] * a], 1)


# ---- masks ------------------------------------------------------------------------------------------------------------------------------
def polar(re, im):
    """(nr, ni, mag) with the squares taken after an exact power-of-two scaling: finite and accurate at every finite nonzero value.
    At exactly 0: n = (0, 0), mag = 0."""
    s = torch.maximum(re.abs(), im.abs())
    _, e = torch.frexp(s)
    ur, ui = torch.ldexp(re, -e), torch.ldexp(im, -e)
    h = (ur * ur + ui * ui).sqrt()
    rh = torch.where(h > 0, 1 / h, torch.zeros_like(h))
    return ur * rh, ui * rh, torch.ldexp(h, e)


def tanhc(a):
    """(k, q, th) = (tanh(a) / a, sech^2(a) - tanh(a) / a, tanh(a)); below MASK_SMALL from the series of tanh (Bernoulli numbers):
    k = 1 - a^2/3 + 2 a^4/15 - 17 a^6/315 + 62 a^8/2835, q = -2 a^2/3 + 8 a^4/15 - 34 a^6/105 + 496 a^8/2835 (next terms below 1e-20)"""
    a2 = a * a
    ks = 1 + a2 * (-1 / 3 + a2 * (2 / 15 + a2 * (-17 / 315 + a2 * (62 / 2835))))
    qs = a2 * (-2 / 3 + a2 * (8 / 15 + a2 * (-34 / 105 + a2 * (496 / 2835))))
    th = torch.tanh(a)
    small = a < MASK_SMALL
    kq = th / torch.where(small, torch.ones_like(a), a)
    return torch.where(small, ks, kq), torch.where(small, qs, (1 - th * th) - kq), torch.where(small, a * ks, th)


def tanhc_expm1(a):
    """the same two functions from e = expm1(-2 a): tanh = -e / (2 + e), sech^2 = 4 (1 + e) / (2 + e)^2 -- an independent formulation
    (q cancels here: absolute error a few 1e-16)"""
    e = torch.expm1(-2 * a)
    th = -e / (2 + e)
    k = th / a
    return k, 4 * (1 + e) / (2 + e) ** 2 - k


def bound_mask(m, tf):
    """m, tf (N, 2, P) -> out (N, 2, P) = tanh(|m|) m / |m| (*) tf, in the dtype of m"""
    nr, ni, a = polar(m[:, 0], m[:, 1])
    _, _, th = tanhc(a)
    ar, ai = th * nr, th * ni
    tr, ti = tf[:, 0].to(m.dtype), tf[:, 1].to(m.dtype)
    return torch.stack([ar * tr - ai * ti, ar * ti + ai * tr], 1)


def bound_mask_mag(m, tf):
    m, tf = m.double(), tf.double().abs()
    nr, ni, a = polar(m[:, 0], m[:, 1])
    _, _, th = tanhc(a)
    ar, ai = th * nr.abs(), th * ni.abs()
    return torch.stack([ar * tf[:, 0] + ai * tf[:, 1], ar * tf[:, 1] + ai * tf[:, 0]], 1)


def bound_mask_bwd(m, tf, g):
    """gm (N, 2, P) = k ga + q (ga . n) n with ga = g (*) conj(tf), n = m / |m|"""
    nr, ni, a = polar(m[:, 0], m[:, 1])
    k, q, _ = tanhc(a)
    tr, ti, gr, gi = tf[:, 0].to(m.dtype), tf[:, 1].to(m.dtype), g[:, 0].to(m.dtype), g[:, 1].to(m.dtype)
    gar, gai = gr * tr + gi * ti, -gr * ti + gi * tr
    dot = (gar * nr + gai * ni) * q
    return torch.stack([gar * k + dot * nr, gai * k + dot * ni], 1)


def bound_mask_bwd_mag(m, tf, g):
    """q = sech^2 - k is formed from 1, tanh^2 and k at and above MASK_SMALL (an absolute error of an ulp of 1, whatever the
    cancellation leaves: the rule for 1 - sigmoid of DESIGN.md 4.15); below it from its series, |q|"""
    m, tf, g = m.double(), tf.double().abs(), g.double().abs()
    nr, ni, a = polar(m[:, 0], m[:, 1])
    k, q, th = tanhc(a)
    mq = torch.where(a < MASK_SMALL, q.abs(), 1 + th * th + k)
    gar, gai = g[:, 0] * tf[:, 0] + g[:, 1] * tf[:, 1], g[:, 0] * tf[:, 1] + g[:, 1] * tf[:, 0]
    dot = (gar * nr.abs() + gai * ni.abs()) * mq
    return torch.stack([gar * k + dot * nr.abs(), gai * k + dot * ni.abs()], 1)


def _cs(xc):
    nr, ni, a = polar(xc[:, 0], xc[:, 1])
    return torch.where(a > 0, nr, torch.ones_like(nr)), ni


def phase_mask(mag, xc):
    """mag (n,), xc (n, 2) -> (n, 2) = mag exp(i atan2(im, re)); (mag, 0) only where xc is exactly 0"""
    c, s = _cs(xc)
    return torch.stack([mag.to(xc.dtype) * c, mag.to(xc.dtype) * s], 1)


def phase_mask_bwd(xc, g):
    """gmag (n,) = g.re cos + g.im sin"""
    c, s = _cs(xc)
    return g[:, 0].to(xc.dtype) * c + g[:, 1].to(xc.dtype) * s


def phase_mask_bwd_mag(xc, g):
    c, s = _cs(xc.double())
    return g[:, 0].double().abs() * c.abs() + g[:, 1].double().abs() * s.abs()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def make_w(C, gen):
    """(3, C) = Wrr, Wri, Wii of a well-conditioned affine map (diagonal 0.75 ... 1.25, off-diagonal within +-0.5)"""
    return torch.stack([0.75 + 0.5 * torch.rand(C, generator=gen), torch.rand(C, generator=gen) - 0.5, 0.75 + 0.5 * torch.rand(C, generator=gen)])


DATA = ("gauss", "dc", "corr", "tiny", "const", "mixed")


def make_x(N, C, S, data, gen, per_channel=False):
    """(N, 2C, S) fp32.  per_channel: channel c takes class DATA[c % 6] (the coefficient cases)"""
    zr, zi = torch.randn(N, C, S, generator=gen), torch.randn(N, C, S, generator=gen)
    std = 0.5 + torch.rand(C, generator=gen).view(1, C, 1)
    kinds = [DATA[c % len(DATA)] if per_channel else data for c in range(C)]
    xr, xi = zr * std, zi * std
    for c, kind in enumerate(kinds):
        sd = float(std[0, c, 0])
        if kind == "dc":
            xr[:, c] += 30 * sd
            xi[:, c] -= 10 * sd
        elif kind == "corr":
            rho = 0.999
            xi[:, c] = (rho * zr[:, c] + (1 - rho * rho) ** 0.5 * zi[:, c]) * sd
        elif kind == "tiny":
            xr[:, c], xi[:, c] = zr[:, c] * 1e-3, zi[:, c] * 1e-3
        elif kind == "const" and (per_channel or c == C // 2):
            xr[:, c], xi[:, c] = 0.05, -0.08
        elif kind == "mixed":
            sc = 10.0 ** float(torch.rand((), generator=gen) * 4 - 2)
            xr[:, c] *= sc
            xi[:, c] *= sc * 0.5
    return torch.cat([xr, xi], 1).contiguous()


@dataclasses.dataclass(frozen=True)
class Case:
    N: int
    C: int
    S: int
    data: str = "gauss"
    sliced: bool = False          # out written into / gy read from a channel slice of a wider buffer
    Cx: int = 2                   # the slice's neighbours: Cx channels ahead of the real half, Cx behind the imaginary half

    @property
    def id(self):
        return f"{self.N}x{self.C}x{self.S}-{self.data}" + ("-sliced" if self.sliced else "")

    def forms(self):
        """what steers the four streaming kernels"""
        S, nch = self.S, nchunks(self.S)
        last = S - (nch - 1) * CHUNK
        items = self.N * self.C * nch
        return {"nchunks": nch, "last_chunk": last, "lane_iters": -(-last // 64), "thread_iters": -(-last // 256),
                "ragged64": last % 64 != 0, "ragged256": last % 256 != 0, "items_mod4": items % 4, "blocks4": -(-items // 4),
                "sliced": self.sliced, "C": self.C, "N": self.N}


S_AXIS = (1, 63, 64, 65, 255, 257, 4095, 4096, 4097, 2 * 4096 + 1)


def stream_cases():
    """the S axis at (N, C) = (3, 3), the C and N axes at small S, the data classes at S = 257 and 4097; half of them sliced"""
    t = [Case(3, 3, S, "gauss", sliced=i % 2 == 1) for i, S in enumerate(S_AXIS)]
    t += [Case(N, C, S, "gauss", sliced=S == 65) for C in (1, 3, 65) for N in (1, 3) for S in (65, 4097) if (N, C) != (3, 3)]
    t += [Case(3, 3, S, d, sliced=S == 257) for d in DATA[1:] for S in (257, 4097)]
    t.append(Case(1, 1, 4 * 4096))                              # four exact chunks: the one workgroup of the wave-per-item kernels is full
    return t


def case_seed(c):
    return 7919 * c.N + 131 * c.C + 17 * c.S + 1000003 * DATA.index(c.data) + c.sliced


def make_inputs(case):
    """fp32 CPU tensors: x, gy, gx0 (what gx holds ahead of rfx_cplx_moments_bwd), W (3, C), B (2, C)"""
    g = torch.Generator().manual_seed(case_seed(case))
    N, C, S = case.N, case.C, case.S
    x = make_x(N, C, S, case.data, g)
    W = make_w(C, g)
    B = torch.randn(2, C, generator=g) * 0.3
    return {"x": x, "gy": torch.randn(N, 2 * C, S, generator=g), "gx0": torch.randn(N, 2 * C, S, generator=g), "W": W, "B": B}


def stream_intermediates(case, inp):
    """coef (6, C) and cm (5, C), fp32, as the fp32 restatement of the coefficient kernels produces them: the inputs of the streaming
    kernels (any fp32 values would do; these are the ones a training step would hand over)"""
    inv = 1.0 / (case.N * case.S)
    coef, st, _ = coef_fwd((moments(inp["x"]), inv), inp["W"], inp["B"], f32(GEN_EPS), dtype=torch.float32)
    _, gcoef = affine_act_bwd(inp["x"].double(), coef.double(), inp["gy"])
    _, cm = coef_bwd(st, inp["W"], f32(GEN_EPS), gcoef.float(), inv, v32=True)
    return coef, cm.float()


COEF_C = (1, 64, 65, 130)


def coef_inputs(C, seed=0):
    """per-channel data classes over (2, C, 257): fp64 sums, inv, parameters, running buffers, an upstream gcoef"""
    g = torch.Generator().manual_seed(1009 * C + seed)
    x = make_x(2, C, 257, None, g, per_channel=True)
    W = make_w(C, g)
    B = torch.randn(2, C, generator=g) * 0.3
    run = torch.stack([torch.randn(C, generator=g) * 0.05, torch.randn(C, generator=g) * 0.05, torch.rand(C, generator=g) * 0.5 + 0.75,
                       torch.randn(C, generator=g) * 0.05, torch.rand(C, generator=g) * 0.5 + 0.75])
    return {"x": x, "sums": moments(x), "inv": 1.0 / (2 * 257), "W": W, "B": B, "running": run, "gcoef": torch.randn(6, C, generator=g)}


def coef_forms(C, train):
    return {"workgroups": -(-C // 64), "last_wg_lanes": C - (-(-C // 64) - 1) * 64, "stats": "sums" if train else "stats_in", "cm": train}


BOUND_MASK_CASES = ((1, 1), (2, 255), (3, 1025), (3, 1_400_003))
PHASE_MASK_N = (1, 257, 4_194_304 + 1027)


def _log_uniform(n, lo, hi, gen):
    return torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _complex_of(mag, gen):
    ph = torch.rand(mag.shape, generator=gen, dtype=torch.float64) * (2 * math.pi)
    return (mag * torch.cos(ph)).float(), (mag * torch.sin(ph)).float()


def bound_mask_inputs(N, P):
    """m (N, 2, P), tf (N, 2, P) to be placed at a sample stride above 2 P, g (N, 2, P).  The first half of every sample has |m| log-uniform
    in [1e-4, 20], the second half in [1e-30, 1e-4] with every 7th value on an axis (one part exactly 0); P = 1: one of each."""
    g = torch.Generator().manual_seed(31 * N + P)
    idx = torch.arange(N * P).view(N, P)
    small = (idx % P >= (P + 1) // 2) if P > 1 else (idx % 2 == 1)
    a = torch.where(small.reshape(-1), _log_uniform(N * P, 1e-30, 1e-4, g), _log_uniform(N * P, 1e-4, 20.0, g))
    mr, mi = _complex_of(a, g)
    ax = (small.reshape(-1)) & (torch.arange(N * P) % 7 == 0)
    mr = torch.where(ax & (torch.arange(N * P) % 14 == 0), torch.zeros_like(mr), mr)
    mi = torch.where(ax & (torch.arange(N * P) % 14 == 7), torch.zeros_like(mi), mi)
    keep = (mr != 0) | (mi != 0)
    mr = torch.where(keep, mr, torch.full_like(mr, 1e-30))       # exact 0 is outside the pinned domain
    m = torch.stack([mr.view(N, P), mi.view(N, P)], 1)
    return {"m": m, "tf": torch.randn(N, 2, P, generator=g), "g": torch.randn(N, 2, P, generator=g), "small": small}


def phase_mask_inputs(n):
    """xc (n, 2) with |x| log-uniform in [1e-30, 1e4], every 5th on an axis, every 11th exactly 0; mag (n,) of both signs; g (n, 2)"""
    g = torch.Generator().manual_seed(n)
    xr, xi = _complex_of(_log_uniform(n, 1e-30, 1e4, g), g)
    i = torch.arange(n)
    xr = torch.where(i % 10 == 5, torch.zeros_like(xr), xr)
    xi = torch.where(i % 10 == 0, torch.zeros_like(xi), xi)
    zero = i % 11 == 3
    xr, xi = torch.where(zero, torch.zeros_like(xr), xr), torch.where(zero, torch.zeros_like(xi), xi)
    return {"xc": torch.stack([xr, xi], 1).contiguous(), "mag": torch.randn(n, generator=g), "g": torch.randn(n, 2, generator=g)}


# ---- floors: the same formulas in float32 with the kernels' partial sums, against fp64 ------------------------------------------------
def floors_stream(case, inp, coef, cm):
    """(refs, magnitudes, slacks, floors) of moments, y, gx, gcoef, gx after moments_bwd -- coef (6, C) and cm (5, C) as the device
    (or, on the CPU, the fp32 restatement) produced them"""
    x, gy, gx0 = inp["x"], inp["gy"], inp["gx0"]
    xd = x.double()
    ref, mag, slack = {}, {}, {}
    ref["sums"], mag["sums"] = moments(x), moments_mag(x)
    ref["y"] = affine_act(xd, coef)
    mag["y"], slack["y"] = affine_act_mag(x, coef)
    ref["gx"], ref["gcoef"] = affine_act_bwd(xd, coef, gy)
    m, s = affine_act_bwd_mag(x, coef, gy)
    mag.update(m)
    slack.update(s)
    ref["gx2"], mag["gx2"] = gx0.double() + moments_bwd(xd, cm), moments_bwd_mag(x, cm, gx0)
    c32, cm32 = coef.float(), cm.float()
    got = {"sums": moments(x, "wide"), "y": affine_act(x, c32), "gx2": gx0 + moments_bwd(x, cm32)}
    got["gx"], got["gcoef"] = affine_act_bwd(x, c32, gy, lanes="narrow")
    fl = {k: floor_of(got[k], ref[k], mag[k], slack.get(k, 0.0)) for k in ref}
    return ref, mag, slack, fl


def tolerance(name, mag, slack, fl):
    return k_of(fl[name]) * EPS32 * mag[name] + slack.get(name, 0.0)


def floors_coef(ci, train, st32=None):
    """(refs, magnitudes, floors) of coef, stats, running' of rfx_cplx_coef_fwd.  st32: the fp32 statistics the coefficients are a
    function of (the device's stats_out; on the CPU the fp32 rounding of the fp64 ones; eval: the running buffers)"""
    e = f32(GEN_EPS)
    if train:
        st64 = stats_of(ci["sums"], ci["inv"])
        st32 = st64.float() if st32 is None else st32
    else:
        st32 = ci["running"].float()
    run = ci["running"] if train else None
    coef, _, r = coef_fwd(st32.double(), ci["W"], ci["B"], e, run, v32=True)
    c32, _, r32 = coef_fwd(st32, ci["W"], ci["B"], e, run, dtype=torch.float32)
    mc, mr = coef_mag(st32.double(), ci["W"], ci["B"], e, run, v32=True)
    ref, mag, got = {"coef": coef}, {"coef": mc}, {"coef": c32}
    if train:
        ref.update(stats=st64, running=r)
        mag.update(stats=stats_mag(ci["sums"], ci["inv"]), running=mr)
        got.update(stats=st64.float(), running=r32)
    return ref, mag, {k: floor_of(got[k], ref[k], mag[k]) for k in ref}


def floors_bound_mask(bi):
    m, tf, g = bi["m"], bi["tf"], bi["g"]
    ref = {"out": bound_mask(m.double(), tf.double()), "gm": bound_mask_bwd(m.double(), tf.double(), g.double())}
    mag = {"out": bound_mask_mag(m, tf), "gm": bound_mask_bwd_mag(m, tf, g)}
    got = {"out": bound_mask(m, tf), "gm": bound_mask_bwd(m, tf, g)}                    # float32: libm tanhf
    return ref, mag, {k: floor_of(got[k], ref[k], mag[k]) for k in ref}


def floors_phase_mask(pi):
    xc, mg, g = pi["xc"], pi["mag"], pi["g"]
    ref = {"out": phase_mask(mg.double(), xc.double()), "gmag": phase_mask_bwd(xc.double(), g.double())}
    mag = {"out": ref["out"].abs(), "gmag": phase_mask_bwd_mag(xc, g)}
    got = {"out": phase_mask(mg, xc), "gmag": phase_mask_bwd(xc, g)}
    return ref, mag, {k: floor_of(got[k], ref[k], mag[k]) for k in ref}
