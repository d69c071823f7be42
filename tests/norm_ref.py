"""Plain torch, fp64, CPU restatement of the GroupNorm / BatchNorm kernels of remfx_amd/csrc/norm.hip in the interface of their C ABI
(rfx_groupnorm_fwd[_x16], rfx_groupnorm_bwd[_x16], rfx_batchnorm_fwd, rfx_batchnorm_bwd).  No autograd in the tested path.

x: (N, C, S).  kind "gn": G groups, a group is one contiguous run of (C / G) * S values of one sample, mean / rstd (N * G).
kind "bn": one (mean, rstd) per channel over (N, S).  Modes: none, gelu (erf form), glu, glu_scale_res (res + scale[c] * glu), relu.

Forward and backward TAKE mean / rstd: the GPU tests pass the kernel's own saved fp32 values, so statistics, apply and backward are
judged separately.  The storage type is part of the reference: the 16-bit forms are fed the bf16-rounded x widened to fp64, and their
stored bf16 dx is judged against the unrounded fp64 dx (tolerance(): half a bf16 ulp on top of the fp32 bound).

The bound of every output is  K * eps32 * magnitude (+ slack),  K = MARGIN * floor + FP32_HALF_ULPS / 2:
  magnitudes()  per output element, the sum of the absolute values of the terms it was formed from, each weighted by the derivative it
                enters with (first-order forward error analysis): |xhat gamma| + |beta| ahead of the activation, sum |gy xhat| for
                dgamma, and so on.  cdf = 0.5 + 0.5 erf counts as those two terms and 1 - sigmoid as 1 and sigmoid, because that is how
                fp32 code forms them (an absolute error of one fp32 ulp of 1, whatever is left after the cancellation).
  floors()      the same formulas in float32 on the CPU with fp32 partial sums in the kernels' decomposition (4096 values per chunk,
                64 lanes, lane l adds elements l, l + 64, ..., a butterfly over the lanes, chunks in order) against the fp64 values, as
                a multiple of eps32 * magnitude: the reference's own noise floor.  Never measured on the kernel.
  slack         ReLU backward only: where |u| is inside its own rounding error the sign, and with it du = gy or 0, is undetermined.

`mutate`: one of MUTATIONS, a deliberately wrong kernel (what the bound has to see; tests/test_norm_ref_cpu.py)."""
import dataclasses

import torch
import torch.nn.functional as F

from tests.ref_common import EPS32, bf16_rne, gelu_cdf, gelu_pdf, ulp, worst  # noqa: F401

MODES = {"none": 0, "gelu": 1, "glu": 2, "glu_scale_res": 3, "relu": 4}
CHUNK = 4096                      # GN_CHUNK
MARGIN = 8.0
FP32_HALF_ULPS = 16               # as tests/lstm_ref.py: 16 fp32 half-ulps = 8 eps32 for what a CPU fp32 evaluation does not have --
#                                   v_exp_f32 / v_rcp_f32 at 1 ulp each, exp(x) as exp2(x log2 e), the Abramowitz-Stegun erf (1.5e-7)
GEN_EPS = 1e-5
U_BAND = MARGIN * 3.0 + FP32_HALF_ULPS / 2   # ReLU backward: |u| <= U_BAND eps32 magnitude(u) is inside u's own bound (at a floor of 3: the floors
#                                              of y measured over the case table stay below it, tests/test_norm_ref_cpu.py) -- sign undetermined

MUTATIONS = (
    "tail_unwritten",             # the last 4 samples of one row keep what the buffer held (0 here; the GPU test fills NaN)
    "stats_last_chunk_missing",   # the last 4096-value chunk of one group is missing from the statistics
    "beta_from_neighbour",        # one channel reads its neighbour's beta
    "glu_halves_swapped",         # value and gate half swapped for one channel pair
    "dscale_missing_sample",      # dscale without one sample's contribution
    "groupsum_over_C",            # the two group sums of dx taken over all C channels instead of the group's C / G
    "gate_dx_sigmoid",            # dx of the gate half scaled by sigmoid instead of sigmoid (1 - sigmoid) in one row
    "inv_over_C",                 # inv = 1 / (C S) instead of 1 / ((C / G) S)
)


def is_glu(mode):
    return mode in ("glu", "glu_scale_res")


# ---- sums: exact (fp64) and the kernels' decomposition in fp32 --------------------------------------------------------------------
def _lanes32(t):
    """fp32 sum over the last axis the way one wave does it: lane l adds elements l, l + 64, ... in order, then the butterfly"""
    pad = (-t.shape[-1]) % 64
    if pad:
        t = F.pad(t, (0, pad))
    t = t.reshape(*t.shape[:-1], -1, 64)
    acc = t[..., 0, :].clone()
    for i in range(1, t.shape[-2]):
        acc = acc + t[..., i, :]
    w = 32
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def _chunk_lanes(t):
    """(..., L) -> (..., nchunks, 64) per-lane fp32 partial sums of every 4096-value chunk (the last one may be ragged)"""
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


class Exact:
    """plain sums in the dtype of the operands (the fp64 reference)"""

    @staticmethod
    def row(t):                   # over the samples of a row
        return t.sum(-1)

    @staticmethod
    def over(t, dim):             # over channels of a group / over samples of the batch
        return t.sum(dim)


class Lanes32:
    """fp32, summed the way the kernels do"""

    @staticmethod
    def row(t):
        acc = _chunk_lanes(t)
        w = 32
        while w:
            acc = acc[..., :w] + acc[..., w:2 * w]
            w //= 2
        acc = acc[..., 0]                                       # (..., nchunks)
        out = acc[..., 0].clone()
        for k in range(1, acc.shape[-1]):                       # gn_bwd_slotsum_kernel: chunk order
            out = out + acc[..., k]
        return out

    @staticmethod
    def over(t, dim):
        return _lanes32(t.movedim(dim, -1))


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def _runs(x, kind, G):
    """the runs one (mean, rstd) is taken over: gn (N * G, L); bn (C, N, S)"""
    N, C, S = x.shape
    return x.reshape(N * G, (C // G) * S) if kind == "gn" else x.permute(1, 0, 2)


def moments(x, kind="gn", G=1):
    """fp64 {sum x, sum x^2, count} per statistic"""
    r = _runs(x.double(), kind, G)
    r = r.reshape(r.shape[0], -1)
    return r.sum(1), (r * r).sum(1), r.shape[1]


def finalize(s1, s2, n, eps=GEN_EPS):
    """gn_finalize_kernel in fp64: E[x^2] - m^2, clamped at 0; eps is the fp32 value the ABI receives"""
    m = s1 / n
    var = (s2 / n - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))


def stats(x, kind="gn", G=1, eps=GEN_EPS):
    """mean, rstd in fp64 (two-pass variance: the truth, not the algorithm)"""
    r = _runs(x.double(), kind, G)
    r = r.reshape(r.shape[0], -1)
    m = r.mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    return m, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))


def stats32(x, kind="gn", G=1, eps=GEN_EPS, mutate=None):
    """the algorithm as written: fp32 per-lane partial sums of x and x * x per 4096-value chunk, combined in fp64, E[x^2] - m^2"""
    r = _runs(x.float(), kind, G)
    n = r.reshape(r.shape[0], -1).shape[1]
    p, q = _chunk_lanes(r).double(), _chunk_lanes(r * r).double()     # gn (NG, nch, 64); bn (C, N, nch, 64)
    if mutate == "stats_last_chunk_missing":
        p, q = p.clone(), q.clone()
        p[-1, ..., -1, :] = 0
        q[-1, ..., -1, :] = 0
    p, q = p.reshape(p.shape[0], -1).sum(1), q.reshape(q.shape[0], -1).sum(1)
    return finalize(p, q, n, eps)


def stat_magnitudes(x, kind="gn", G=1, eps=GEN_EPS):
    """mean: sum |x| / n (absolute).  rstd: 0.5 E[x^2] / (var + eps), relative -- d rstd / rstd = -0.5 d var / (var + eps), and var =
    E[x^2] - m^2 carries the absolute error of its two operands, both of size E[x^2]"""
    r = _runs(x.double(), kind, G)
    r = r.reshape(r.shape[0], -1)
    m = r.mean(1)
    var = ((r - m[:, None]) ** 2).mean(1)
    e2 = (r * r).mean(1)
    return {"mean": r.abs().mean(1), "rstd": 0.5 * e2 / (var + float(torch.tensor(eps, dtype=torch.float32)))}


def stat_floors(x, kind="gn", G=1, eps=GEN_EPS):
    m, r = stats(x, kind, G, eps)
    m32, r32 = stats32(x, kind, G, eps)
    mag = stat_magnitudes(x, kind, G, eps)
    return {"mean": float(((m32 - m).abs() / (EPS32 * mag["mean"]).clamp_min(1e-300)).max()),
            "rstd": float((((r32 - r) / r).abs() / (EPS32 * mag["rstd"])).max())}


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def _bc(stat, kind, N, C, G):
    if kind == "bn":
        return stat.view(1, C, 1)
    return stat.view(N, G, 1).repeat_interleave(C // G, 1)


def _pre(x, gamma, beta, mean, rstd, kind, G, mutate=None):
    N, C, S = x.shape
    m, r = _bc(mean.to(x.dtype), kind, N, C, G), _bc(rstd.to(x.dtype), kind, N, C, G)
    xh = (x - m) * r
    b = beta.to(x.dtype)
    if mutate == "beta_from_neighbour":
        b = b.clone()
        b[C // 2 - 1] = beta[C // 2 - 2] if C // 2 >= 2 else beta[C - 1]
    u = xh * gamma.to(x.dtype).view(1, C, 1) + b.view(1, C, 1)
    return xh, u, r


def forward(x, gamma, beta, mean, rstd, mode="none", res=None, scale=None, kind="gn", G=1, mutate=None, prefill=0.0):
    """y in the dtype of x: (N, C, S), GLU modes (N, C / 2, S)"""
    assert mode in MODES and (mutate is None or mutate in MUTATIONS)
    N, C, S = x.shape
    xh, u, _ = _pre(x, gamma, beta, mean, rstd, kind, G, mutate)
    if mode == "none":
        y = u
    elif mode == "relu":
        y = u.clamp_min(0)
    elif mode == "gelu":
        y = u * gelu_cdf(u)
    else:
        ua, ub = u[:, :C // 2], u[:, C // 2:]
        if mutate == "glu_halves_swapped":
            ua, ub = ua.clone(), ub.clone()
            ua[:, -1], ub[:, -1] = u[:, C - 1], u[:, C // 2 - 1]
        y = ua * torch.sigmoid(ub)
        if mode == "glu_scale_res":
            y = res.to(x.dtype) + scale.to(x.dtype).view(1, -1, 1) * y
    if mutate == "tail_unwritten":
        y = y.clone()
        y[N - 1, y.shape[1] - 1, S - 4:] = prefill
    return y


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _du(x, gamma, beta, mean, rstd, gy, mode, scale, kind, G, mutate, want_mag):
    """du (N, C, S) = d loss / d u, gf (mode 3: the terms of dscale), xh, r -- and, want_mag, their magnitudes and the ReLU slack"""
    N, C, S = x.shape
    xh, u, r = _pre(x, gamma, beta, mean, rstd, kind, G)
    gy = gy.to(x.dtype)
    gf = mgf = None
    A = (xh * gamma.to(x.dtype).view(1, C, 1)).abs() + beta.to(x.dtype).abs().view(1, C, 1) if want_mag else None
    mdu = slack = None
    if mode == "none":
        du = gy
        if want_mag:
            mdu = gy.abs()
    elif mode == "relu":
        du = gy * (u > 0).to(x.dtype)
        if want_mag:
            mdu = du.abs()
            slack = gy.abs() * (u.abs() <= U_BAND * EPS32 * A).to(x.dtype)
    elif mode == "gelu":
        pdf = gelu_pdf(u)
        du = gy * (gelu_cdf(u) + u * pdf)
        if want_mag:
            cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
            mdu = gy.abs() * (cdfm + u.abs() * pdf + pdf * (2.0 - u * u).abs() * A)
    else:
        Co = C // 2
        ua, ub = u[:, :Co], u[:, Co:]
        sg = torch.sigmoid(ub)
        g0 = gy
        if mode == "glu_scale_res":
            gf = gy * ua * sg
            g0 = gy * scale.to(x.dtype).view(1, Co, 1)
        dua = g0 * sg
        dub = g0 * ua * sg * (1.0 - sg)
        if mutate == "gate_dx_sigmoid":
            dub = dub.clone()
            dub[N - 1, Co - 1] = (g0 * ua * sg)[N - 1, Co - 1]
        du = torch.cat([dua, dub], 1)
        if want_mag:
            Aa, Ab = A[:, :Co], A[:, Co:]
            glu_mag = sg * (Aa + ua.abs() * (1.0 - sg) * Ab)
            if mode == "glu_scale_res":
                mgf = gy.abs() * glu_mag
            mdu = torch.cat([g0.abs() * sg * (1.0 + (1.0 - sg) * Ab),
                             g0.abs() * sg * ((1.0 - sg) * Aa + ua.abs() * ((1.0 + sg) + (1.0 - sg) * (1.0 - 2.0 * sg).abs() * Ab))], 1)
    return du, gf, xh, r, mdu, mgf, slack


def _reduce(du, gf, xh, r, gamma, kind, G, sums, idx, mutate, sub=1.0):
    """dx, dgamma, dbeta, dscale from du by the closed form; with sub = -1 and operands >= 0 the same code adds the magnitudes up"""
    N, C, S = du.shape
    gm = gamma.to(du.dtype).view(1, C, 1)
    p0, p1 = sums.row(du), sums.row(du * xh)                    # (N, C): the per-(sample, channel) partial pairs of `work`
    take = (lambda t: t) if idx is None else (lambda t: t[idx])
    dbeta, dgamma = sums.over(take(p0), 0), sums.over(take(p1), 0)
    dscale = None
    if gf is not None:
        psc = take(sums.row(gf))
        if mutate == "dscale_missing_sample":
            psc = psc[:-1]
        dscale = sums.over(psc, 0)
    g1, g2 = gm.view(1, C) * p0, gm.view(1, C) * p1
    if kind == "bn":
        s1, s2 = (gm.view(C) * dbeta).view(1, C, 1), (gm.view(C) * dgamma).view(1, C, 1)
        inv = 1.0 / (N * S)
    else:
        Cg = C // G
        s1, s2 = sums.over(g1.view(N, G, Cg), 2), sums.over(g2.view(N, G, Cg), 2)
        if mutate == "groupsum_over_C":
            s1, s2 = sums.over(g1, 1).view(N, 1).expand(N, G), sums.over(g2, 1).view(N, 1).expand(N, G)
        s1, s2 = s1.reshape(N, G, 1).repeat_interleave(Cg, 1), s2.reshape(N, G, 1).repeat_interleave(Cg, 1)
        inv = 1.0 / ((C if mutate == "inv_over_C" else Cg) * S)
    dx = r * (du * gm - sub * (s1 * inv + xh * (s2 * inv)))
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "dscale": dscale}


def backward(x, gamma, beta, mean, rstd, gy, mode="none", scale=None, kind="gn", G=1, idx=None, mutate=None, sums=Exact):
    """{dx, dgamma, dbeta, dscale} by the closed form.  idx (Ntotal,): the batch is x[idx] -- samples drawn from the pool x, each
    pool entry with ITS mean / rstd; dx is per pool entry, the three parameter gradients are sums over the whole batch."""
    assert mode in MODES and (mutate is None or mutate in MUTATIONS) and (idx is None or kind == "gn")
    du, gf, xh, r, _, _, _ = _du(x, gamma, beta, mean, rstd, gy, mode, scale, kind, G, mutate, False)
    return _reduce(du, gf, xh, r, gamma, kind, G, sums, idx, mutate)


def magnitudes(x, gamma, beta, mean, rstd, mode="none", res=None, scale=None, gy=None, kind="gn", G=1, idx=None):
    """({y, dx, dgamma, dbeta, dscale}: magnitude per element, {...}: absolute slack per element); the backward ones need gy"""
    x = x.double()
    N, C, S = x.shape
    xh, u, r = _pre(x, gamma, beta, mean, rstd, kind, G)
    A = (xh * gamma.double().view(1, C, 1)).abs() + beta.double().abs().view(1, C, 1)
    if mode in ("none", "relu"):
        my = A
    elif mode == "gelu":
        cdfm = 0.5 + 0.5 * torch.erf(u.abs() * (0.5 ** 0.5))
        my = A * (2.0 * cdfm + u.abs() * gelu_pdf(u))
    else:
        Co = C // 2
        sg = torch.sigmoid(u[:, Co:])
        my = sg * (A[:, :Co] + u[:, :Co].abs() * (1.0 - sg) * A[:, Co:])
        if mode == "glu_scale_res":
            my = res.double().abs() + scale.double().abs().view(1, Co, 1) * my
    mag, slack = {"y": my}, {}
    if gy is not None:
        _, _, xh, r, mdu, mgf, sl = _du(x, gamma, beta, mean, rstd, gy, mode, scale, kind, G, None, True)
        ag = gamma.double().abs()
        mag.update(_reduce(mdu, mgf, xh.abs(), r, ag, kind, G, Exact, idx, None, sub=-1.0))
        if sl is not None:
            slack = {k: v for k, v in _reduce(sl, None, xh.abs(), r, ag, kind, G, Exact, idx, None, sub=-1.0).items() if v is not None}
    return {k: v for k, v in mag.items() if v is not None}, slack


def reference(inp, mean, rstd, case, dtype=torch.float64, sums=Exact, mutate=None, prefill=0.0):
    """every output of the case from inputs `inp` (make_inputs) and the given statistics, in `dtype`"""
    c = lambda t: None if t is None else t.to(dtype)            # noqa: E731
    x = c(inp["x"])
    out = {"y": forward(x, c(inp["gamma"]), c(inp["beta"]), c(mean), c(rstd), case.mode, c(inp["res"]), c(inp["scale"]), case.kind,
                        case.G, mutate=mutate, prefill=prefill)}
    if case.bwd:
        out.update(backward(x, c(inp["gamma"]), c(inp["beta"]), c(mean), c(rstd), c(inp["gy"]), case.mode, c(inp["scale"]), case.kind,
                            case.G, inp["idx"], mutate=mutate, sums=sums))
    return {k: v for k, v in out.items() if v is not None}


def floors(inp, mean, rstd, case):
    """(fp64 reference, magnitudes, slack, {output: floor}): floor = max over the elements of |fp32 restatement - fp64| (less the
    slack) in units of eps32 * magnitude"""
    ref = reference(inp, mean, rstd, case)
    f32 = reference(inp, mean, rstd, case, dtype=torch.float32, sums=Lanes32)
    mag, slack = magnitudes(inp["x"], inp["gamma"], inp["beta"], mean, rstd, case.mode, inp["res"], inp["scale"],
                            inp["gy"] if case.bwd else None, case.kind, case.G, inp["idx"])
    fl = {}
    for k in ref:
        e = (f32[k].double() - ref[k]).abs() - slack.get(k, 0.0)
        fl[k] = float((e / (EPS32 * mag[k]).clamp_min(1e-300)).clamp_min(0).max())
    return ref, mag, slack, fl


def k_of(floor):
    """the bound in units of eps32 * magnitude: 8 x floor + 16 fp32 half-ulps"""
    return MARGIN * floor + FP32_HALF_ULPS / 2


def tolerance(name, ref, mag, slack, fl, x16=False):
    """absolute tolerance per element of output `name`"""
    t = k_of(fl[name]) * EPS32 * mag[name] + slack.get(name, 0.0)
    if x16 and name == "dx":
        t = t + 0.5 * ulp(ref[name].abs() + t, 7)             # RNE store: half a bf16 ulp of the value the kernel rounded
    return t


# ---- workspace sizes, restated from the header comment ------------------------------------------------------------------------------
def stat_chunks(C, S, G):
    return -(-((C // G) * S) // CHUNK)


def bn_stat_slots(N, S):
    return N * -(-S // CHUNK)


def work_floats(N, C, S, G):
    """N*C*2 + N*(C/2) + 2 max(N*G, C) (G = 0, BatchNorm: 2 C) and, rows longer than one chunk, a slot per (sample, channel, chunk)"""
    nch = -(-S // CHUNK)
    n = N * C * 2 + N * (C // 2) + 2 * (C if G == 0 else max(N * G, C))
    if nch > 1:
        n += N * C * 2 * nch + N * (C // 2) * nch
    return n


# ---- the dispatch of norm_fwd / norm_bwd, line by line --------------------------------------------------------------------------------
def _row_items(rows, S):
    per = -(-S // 256)
    return None if (S & 3) or rows * per > 0x7FFFFFFF else per


def forms(kind, N, C, S, G, mode, x16=False, sums_given=-1, use_given_stats=False, bwd=True):
    """(launched instantiations, steering quantities) of one forward (+ backward) call; None where the ABI returns -1"""
    bn, glu, T = kind == "bn", is_glu(mode), "bf16" if x16 else "f32"
    if x16 and ((S & 3) or bn):
        return None
    names, st = [], {}
    if not use_given_stats:
        L = S if bn else (C // G) * S
        nch = -(-L // CHUNK)
        st.update(nchunks=nch, last_chunk=L - (nch - 1) * CHUNK, stat_vec=L % 4 == 0)
        given = 0 if sums_given == -1 else sums_given
        slots = given if given > 1 else 1
        if not given:
            if sums_given == -1 or bn:
                names.append(f"stats<{T},slotted>")
                slots = N * nch if bn else nch
            else:
                names.append(f"memset+stats<{T},atomic>")
        names.append("finalize")
        st["slots"] = slots
    Cw = C // 2 if glu else C
    ipr = _row_items(N * Cw, S) if C <= 65535 else None
    if ipr is not None:
        names.append(f"rows<{T}>")
        st.update(ipr=ipr, gridz=min(N, 65535), row_exact=S % 256 == 0)
    elif x16:
        return None
    else:
        names.append("apply<4>" if S % 4 == 0 else "apply<1>")
    if not bwd:
        return names, st
    nchb = -(-S // CHUNK)
    st.update(bwd_nchunks=nchb, bwd_last_chunk=S - (nchb - 1) * CHUNK)
    if not bn and G == 1 and N >= 512 and C * S <= 65536:
        if not glu and S <= 256 and C <= 12:
            names.append(f"sample_wave<12,{T}>")
        elif not glu and S <= 256 and C <= 24:
            names.append(f"sample_wave<24,{T}>")
        elif glu and S <= 256 and C // 2 <= 48:
            names.append(f"sample_reg<3,true,{T}>")
        elif glu and S <= 256 and C // 2 <= 96:
            names.append(f"sample_reg<6,false,{T}>")
        else:
            names.append(f"sample<{T}>")
        NS = 64 if N >= 2048 else 1
        while NS > 1 and NS * C * 3 > 2 * N:
            NS >>= 1
        st["NS"] = (NS, N >= 2048)
        names += ["chansum_split", "chansum_final"] if NS > 1 else ["chansum"]
        return names, st
    names.append(f"partial<{T}>" + ("+slotsum" if nchb > 1 else ""))
    st["partial_branch"] = ("pair" if glu else "single") + ("_vec" if S % 4 == 0 else "_scalar")
    if not bn:
        names.append("groupsum")
    names.append("chansum")
    if ipr is not None:
        names.append(f"bwd_rows<{T}>")
    else:
        names.append("bwd_apply<4>" if S % 4 == 0 else "bwd_apply<1>")
    return names, st


# ---- the case table of tests/test_gpu_norm_kernel.py ----------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    group: str                    # which test function runs it
    kind: str
    N: int
    C: int
    S: int
    G: int
    mode: str = "none"
    x16: bool = False
    given: int = -1               # sums_given
    xkind: str = "randn"          # randn: randn * 2 + 0.5; mean<m>: m + randn; const: one constant per group
    bwd: bool = True
    eval: bool = False            # BatchNorm with use_given_stats
    pool: int = 0                 # > 0: the N samples are drawn from this many distinct ones (see make_inputs)

    @property
    def id(self):
        s = f"{self.kind}-{self.N}x{self.C}x{self.S}-G{self.G}-{self.mode}-{'bf16' if self.x16 else 'f32'}"
        if self.given != -1:
            s += f"-given{self.given}"
        if self.xkind != "randn":
            s += f"-{self.xkind}"
        if self.eval:
            s += "-eval"
        return s + ("" if self.bwd else "-fwd")

    def forms(self):
        return forms(self.kind, self.N, self.C, self.S, self.G, self.mode, self.x16, self.given, self.eval, self.bwd)


ALL = ("none", "gelu", "glu", "glu_scale_res", "relu")
SINGLE = ("none", "gelu", "relu")
GLU = ("glu", "glu_scale_res")
CAP = 6_000_000                   # elements whose fp64 reference is evaluated; above it the batch is drawn from a pool


def _storages(S, kind="gn"):
    return (False, True) if S % 4 == 0 and kind == "gn" else (False,)


def case_table():
    t = []
    # statistics and finalize: forward only, mode none
    for (N, C, S, G) in ((3, 6, 4100, 3), (2, 4, 4096, 2), (2, 3, 1367, 1), (5, 8, 12, 8)):
        for x16 in _storages(S):
            for given in (-1, 0, 1, 16):
                t.append(Case("stats", "gn", N, C, S, G, x16=x16, given=given, bwd=False))
    t += [Case("stats", "bn", 70, 4, 231, 4, bwd=False), Case("stats", "bn", 3, 5, 4099, 5, bwd=False)]
    t += [Case("const", "gn", 3, 6, 4100, 3, x16=x16, xkind="const", bwd=False) for x16 in (False, True)]
    t += [Case("largemean", "gn", 4, 8, 1024, 1, x16=x16, xkind=f"mean{m}", bwd=False) for m in (0, 10, 100, 1000) for x16 in (False, True)]
    # row kernels at every ipr, forward and generic backward (N < 512)
    for S in (4, 252, 256, 260, 512, 516, 1028):
        t += [Case("rows", "gn", 3, 10, S, 2, mode, x16) for mode in ALL for x16 in (False, True)]
    t += [Case("edge", "gn", 2, 6, 132, 3, mode, x16) for mode in ALL for x16 in (False, True)]                                # (2, 6, 4, 33): S = 132, still a row kernel
    t += [Case("edge", "gn", 2, 6, 133, 3, mode) for mode in ALL]                                  # (2, 6, 7, 19): S odd, the scalar kernels
    t += [Case("edge", "gn", 1, 65540, 4, G, mode) for G in (1, 2) for mode in ALL]                # C > 65535
    t += [Case("edge", "gn", 65540, 2, 4, 2, mode, x16) for mode in ALL for x16 in (False, True)]   # gridDim.z < N
    t += [Case("edge", "bn", 65540, 1, 4, 1, mode) for mode in ("none", "relu")]
    t += [Case("edge", "bn", 3, 5, S, 5, mode, eval=True, bwd=False) for S in (36, 37) for mode in ("none", "relu")]
    # generic backward
    for (N, C, S, G) in ((2, 6, 13000, 3), (2, 4, 8192, 1)):
        t += [Case("generic", "gn", N, C, S, G, mode, x16) for mode in ALL for x16 in (False, True)]
    t += [Case("generic", "gn", 3, 6, 260, 6, mode, x16) for mode in ALL for x16 in (False, True)]   # G = C
    for (N, C, S) in ((40, 4, 231), (3, 5, 4099), (2, 8, 9100)):
        t += [Case("generic", "bn", N, C, S, C, mode) for mode in ("none", "relu")]
    # per-sample backward, N = 513: the last workgroup of the 4-samples-per-block kernels holds one sample.  Every (C, S) of the table
    # in every mode of its form and both storage types
    SS = (4, 60, 64, 68, 252, 256)
    for C in (1, 11, 12, 13, 24):
        for S in SS:
            t += [Case("sample", "gn", 513, C, S, 1, mode, x16) for mode in SINGLE for x16 in _storages(S)]
    for Ch in (1, 47, 48, 49, 96):
        for S in (4, 68, 256):
            t += [Case("sample", "gn", 513, 2 * Ch, S, 1, mode, x16, pool=_pool(513, 2 * Ch, S)) for mode in GLU for x16 in (False, True)]
    for (C, S, modes) in ((25, 64, SINGLE), (8, 260, SINGLE), (194, 64, GLU), (16, 516, GLU), (25, 63, SINGLE), (16, 517, GLU)):   # the last two: S odd
        t += [Case("sample", "gn", 513, C, S, 1, mode, x16, pool=_pool(513, C, S)) for mode in modes for x16 in _storages(S)]
    # channel sums
    for (N, C, S) in ((2100, 8, 16), (2048, 40, 8), (2048, 700, 4)):
        t += [Case("chansum", "gn", N, C, S, 1, mode, x16) for mode in ALL for x16 in (False, True)]
    t += [Case("chansum", "gn", 511, 12, 64, 1, mode, x16) for mode in ALL for x16 in (False, True)]
    # the C * S <= 65536 switch (an exception to the size cap: 33.5 M elements on the device, a pool on the CPU)
    t += [Case("switch", "gn", 512, C, 4, 1, mode, pool=8) for C in (16384, 16385) for mode in SINGLE]
    t += [Case("switch", "gn", 512, C, 4, 1, mode, pool=8) for C in (16384, 16386) for mode in GLU]
    return t


def _pool(N, C, S):
    return 0 if N * C * S <= CAP else 19


def make_inputs(case):
    """fp32 CPU tensors {x, gamma, beta, res, scale, gy, idx}.  pool > 0: x / res / gy hold `pool` + 1 distinct samples and the batch is
    x[idx]: idx is a fixed random draw from the pool, the LAST sample is the extra entry and occurs once.  x16: x is bf16-rounded."""
    g = torch.Generator().manual_seed(7919 * case.N + 131 * case.C + 17 * case.S + case.G + 1000003 * MODES[case.mode] + case.x16)
    N, C, S = case.N, case.C, case.S
    P = case.pool + 1 if case.pool else N
    if case.xkind == "randn":
        x = torch.randn(P, C, S, generator=g) * 2 + 0.5
    elif case.xkind.startswith("mean"):
        x = float(case.xkind[4:]) + torch.randn(P, C, S, generator=g)
    else:
        x = (torch.arange(P * case.G).float().view(P, case.G, 1, 1) * 0.75 - 3.25).expand(P, case.G, C // case.G, S).reshape(P, C, S).clone()
    if case.x16:
        x = bf16_rne(x)
    Co = C // 2 if is_glu(case.mode) else C
    inp = {"x": x, "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g), "res": None, "scale": None,
           "gy": torch.randn(P, Co, S, generator=g), "idx": None}
    if case.mode == "glu_scale_res":
        inp["res"], inp["scale"] = torch.randn(P, Co, S, generator=g), torch.randn(Co, generator=g)
    if case.pool:
        idx = torch.randint(0, case.pool, (N,), generator=g)
        idx[N - 1] = case.pool
        inp["idx"] = idx
    return inp


def relu_band_count(inp, mean, rstd, case):
    """(count, total) of the elements of u whose sign is inside u's own bound (the only ones that carry slack)"""
    x = inp["x"].double()
    _, u, _ = _pre(x, inp["gamma"].double(), inp["beta"].double(), mean.double(), rstd.double(), case.kind, case.G)
    A = ((u - inp["beta"].double().view(1, -1, 1)).abs() + inp["beta"].double().abs().view(1, -1, 1))
    return int((u.abs() <= U_BAND * EPS32 * A).sum()), u.numel()


def large_mean_row(m, eps=GEN_EPS):
    """x = m + randn over (4, 8, 1024), G = 1, fp32 storage: (mean / std, fp64 rstd, relative rstd error of the algorithm with fp32 lane
    partials on the CPU, of fp32 F.group_norm on the CPU, the model bound) -- the columns of the DESIGN.md table that need no GPU"""
    case = [c for c in case_table() if c.group == "largemean" and c.xkind == f"mean{m}" and not c.x16][0]
    x = make_inputs(case)["x"]
    mt, rt = stats(x, "gn", 1, eps)
    _, r32 = stats32(x, "gn", 1, eps)
    # torch: rstd from y = (x - mean) * rstd with unit weight, at the element furthest from the mean
    yt = F.group_norm(x, 1, eps=eps).double().reshape(x.shape[0], -1)
    xd = (x.double() - mt.view(-1, 1, 1)).reshape(x.shape[0], -1)
    i = xd.abs().argmax(1)[:, None]
    rtorch = yt.gather(1, i)[:, 0] / xd.gather(1, i)[:, 0]
    fl, mag = stat_floors(x, "gn", 1, eps), stat_magnitudes(x, "gn", 1, eps)
    return (float((mt.abs() * rt).max()), float(rt[0]), float(((r32 - rt) / rt).abs().max()), float(((rtorch - rt) / rt).abs().max()),
            float((k_of(fl["rstd"]) * EPS32 * mag["rstd"]).max()))


# ---- plain GLU and average pooling: the tail of norm.hip (rfx_glu_fwd / _bwd / _bwd_bf16, rfx_avgpool2d_fwd / _bwd) -----------------------
# Written as the operation.  Bounds, none measured on a kernel:
#   GLU   the K rule of DESIGN.md 4.21 with elem_ref's sigmoid floors: y = a s(b) and da = g s(b) carry one product more than the
#         sigmoid (one eps32 = a half-ulp pair more), db = g a s(b) (1 - s(b)) two more than the sigmoid's derivative; each keeps the
#         smallest normal per unit of what multiplies the sigmoid (1 / (1 + exp(-v)) is 0 where exp overflows and sigmoid is still a
#         subnormal).  The stored bf16 gx: half a bf16 ulp of the value the kernel rounded on top.
#   pool  forward: kh kw - 1 rounded adds, the product and the rounding of 1 / (kh kw), in half-ulps of sum |x| / (kh kw), plus one
#         subnormal spacing; backward: gy * inv, exact where kh kw is a power of two (inv and the product are), else two half-ulps.
from tests import elem_ref as _E                                # noqa: E402

GLU_GRID_CAP = 4096 * 1024                                      # gn_grid: 4096 workgroups of 256 threads ... 1024 elements each
GLU_ROW_CASES = ((3, 2, 4), (2, 4, 130), (5, 6, 256), (1, 2, 512))
GLU_FLAT_CASES = ((1, 2, 1), (3, 2, 5), (2, 6, 43))
GLU_CAP_CASES = ((1, 2, 4194307), (2, 2, 2097156))             # flat and row, more than GLU_GRID_CAP outputs
GLU_ENTRIES = ("fwd", "bwd", "bwd_bf16")
# floors of glu_restate32 over the case tables in units of eps32 x magnitude, rounded up to the next half.  Measured: 1.48, 1.45, 2.24 --
# above elem_ref's sigmoid floors (1.0 / 2.0) by the extra products, so they are kept here.  The bound keeps K = k_of(sigmoid) + 1 = 17
# and k_of(sigmoid_grad) + 2 = 26, which is tighter than 8 floor + 8 = 20 / 28 and still 8 floor + 4 at least (test_norm_ref_cpu.py)
GLU_FLOOR = {"y": 1.5, "da": 1.5, "db": 2.5}
GLU_SPECIALS = (0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, -(2.0 ** -127), 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


def forms_glu(entry, N, C, S, offs=(0, 0, 0)):
    """the kernel and the branches one call reaches, from the conditions of rfx_glu_fwd / _bwd / _bwd_bf16; None: refused.  offs: how many
    ELEMENTS the bases of (x, y or gx, gy) sit past a 16-byte boundary"""
    if N <= 0 or C <= 0 or C % 2 or S <= 0:
        return None
    L = (C // 2) * S
    per = -(-L // 256)
    x16 = entry == "bwd_bf16"
    esz = (2 if x16 else 4, 2 if x16 else 4, 4)
    need = (8 if x16 else 16, 8 if x16 else 16, 16)
    used = (0, 1) if entry == "fwd" else (0, 1, 2)
    aligned = all((offs[i] * esz[i]) % need[i] == 0 for i in used)
    rows = L % 4 == 0 and N * per <= 0x7FFFFFFF and aligned
    if not rows:
        if x16:
            return None
        out = {f"glu_{entry}_kernel:flat"}
        if N * L > GLU_GRID_CAP:
            out.add("flat:grid_capped")
        return out
    out = {f"glu_{entry[:3]}_rows_kernel<{'bf16' if x16 else 'f32'}>:rows"}
    if L % 256:
        out.add("rows:ragged_chunk")                            # lanes of the last chunk leave at o >= L
    if per > 1:
        out.add("rows:several_chunks")
    if (N * per) % 4:
        out.add("rows:idle_wave")
    return out


def _mixed(n, g):
    """magnitudes 1e-4 ... 1e3, log-uniform, random sign"""
    m = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 7.0 - 4.0)
    return (m * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()


def glu_data(N, C, S, seed=0, x16=False):
    """(x (N, C, S), gy (N, C / 2, S)) fp32.  The value half a: mixed scales with zeros; the gate half b: uniform in [-12, 12] with
    GLU_SPECIALS at its head when there is room -- two visibly different distributions; gy: mixed scales with zeros"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 3 * C + S)
    Co = C // 2
    n = N * Co * S
    a, gy = _mixed(n, g), _mixed(n, g)
    b = (torch.rand(n, generator=g, dtype=torch.float64) * 24.0 - 12.0).float()
    if n >= 2 * len(GLU_SPECIALS):
        b[:len(GLU_SPECIALS)] = torch.tensor(GLU_SPECIALS, dtype=torch.float64).float()
    if n >= 3:
        a[1::11] = 0.0
        gy[2::13] = 0.0
    x = torch.cat([a.view(N, Co, S), b.view(N, Co, S)], 1).contiguous()
    if x16:
        x = bf16_rne(x)
    return x, gy.view(N, Co, S)


def glu(x, gy=None):
    """fp64 {y} or, with gy, {gx}: y = a s(b); da = g s(b), db = g a s(b) (1 - s(b))"""
    x = x.double()
    Co = x.shape[1] // 2
    a, b = x[:, :Co], x[:, Co:]
    s = _E.act(b, _E.SIGMOID)
    if gy is None:
        return {"y": a * s}
    g = gy.double()
    return {"gx": torch.cat([g * s, g * a * _E.act_grad(b, _E.SIGMOID)], 1)}


def glu_bounds(x, gy=None):
    """fp32 bound per element of the same outputs"""
    x = x.double()
    Co = x.shape[1] // 2
    a, b = x[:, :Co], x[:, Co:]
    s = _E.act(b, _E.SIGMOID)
    k = _E.k_of("sigmoid") + 1.0
    if gy is None:
        return {"y": k * EPS32 * (a * s).abs() + a.abs() * _E.MINNORM}
    g = gy.double()
    da = k * EPS32 * (g * s).abs() + g.abs() * _E.MINNORM
    db = (_E.k_of("sigmoid_grad") + 2.0) * EPS32 * a.abs() * _E.act_grad_magnitude(b, g, _E.SIGMOID) + _E.MINNORM * (1.0 + (g * a).abs())
    return {"gx": torch.cat([da, db], 1)}


def bf16_store_bound(ref, b32):
    """a bf16 RNE store of a value inside b32 of ref: half a bf16 ulp of |ref| + b32 on top"""
    return 0.5 * ulp(ref.abs() + b32, 7) + b32


def glu_restate32(x, gy=None):
    """the same formulas in float32 with 1 / (1 + exp(-v)) (CPU libm, never a kernel)"""
    x = x.float()
    Co = x.shape[1] // 2
    a, b = x[:, :Co], x[:, Co:]
    s = 1.0 / (1.0 + torch.exp(-b))
    if gy is None:
        return {"y": a * s}
    g = gy.float()
    return {"gx": torch.cat([g * s, g * a * s * (1.0 - s)], 1)}


def glu_floors(x, gy):
    """{y, da, db}: the restatement's error, less the smallest-normal term, in units of eps32 x the magnitude the bound multiplies"""
    x64 = x.double()
    Co = x.shape[1] // 2
    a, b, g = x64[:, :Co], x64[:, Co:], gy.double()
    s = _E.act(b, _E.SIGMOID)
    ref, r32 = {**glu(x), **glu(x, gy)}, {**glu_restate32(x), **glu_restate32(x, gy)}
    mags = {"y": ((a * s).abs(), a.abs() * _E.MINNORM, ref["y"], r32["y"]),
            "da": ((g * s).abs(), g.abs() * _E.MINNORM, ref["gx"][:, :Co], r32["gx"][:, :Co]),
            "db": (a.abs() * _E.act_grad_magnitude(b, g, _E.SIGMOID), _E.MINNORM * (1.0 + (g * a).abs()), ref["gx"][:, Co:], r32["gx"][:, Co:])}
    out = {}
    for k, (mag, tiny, r, f) in mags.items():
        e = ((f.double() - r).abs() - tiny).clamp_min(0.0)
        out[k] = float((e / (EPS32 * mag).clamp_min(1e-300)).max())
    return out


# ---- average pooling ------------------------------------------------------------------------------------------------------------------
POOL_CASES = ((3, 4, 6, 2, 2), (2, 5, 7, 2, 2), (1, 2, 2, 2, 2), (2, 7, 9, 3, 2), (2, 4, 6, 4, 6), (2, 3, 9, 1, 3), (4, 8, 513, 2, 2))
POOL_CAP_FWD = (4, 2051, 2051, 2, 2)                            # 4 * 1025 * 1025 outputs > GLU_GRID_CAP, both remainders
POOL_CAP_BWD = (1, 2049, 2051, 2, 3)                            # 2049 * 2051 inputs > GLU_GRID_CAP, both remainders, kh kw = 6
POOL_REFUSED = ((2, 3, 6, 4, 2), (2, 4, 5, 2, 6), (2, 4, 6, 0, 2), (2, 4, 6, 2, 0), (0, 4, 6, 2, 2))   # H < kh, W < kw, kh = 0, kw = 0, NC = 0


def forms_pool(bwd, NC, H, W, kh, kw):
    if NC <= 0 or kh <= 0 or kw <= 0 or H < kh or W < kw:
        return None
    total = NC * H * W if bwd else NC * (H // kh) * (W // kw)
    out = {"avgpool2_bwd_kernel" if bwd else "avgpool2_fwd_kernel"}
    if total > GLU_GRID_CAP:
        out.add("grid_capped")
    if H % kh:
        out.add("row_remainder")
    if W % kw:
        out.add("column_remainder")
    if (kh * kw) & (kh * kw - 1):
        out.add("inv_rounded")
    return out


def pool_data(NC, H, W, kh, kw, seed=0):
    """(x (NC, H, W), gy (NC, H / kh, W / kw)) fp32, mixed scales and signs: the windows cancel"""
    g = torch.Generator().manual_seed(100 * seed + NC + 3 * H + 5 * W + 7 * kh + kw)
    return _mixed(NC * H * W, g).view(NC, H, W), _mixed(NC * (H // kh) * (W // kw), g).view(NC, H // kh, W // kw)


def _windows(x, kh, kw):
    NC, H, W = x.shape
    OH, OW = H // kh, W // kw
    return x[:, :OH * kh, :OW * kw].reshape(NC, OH, kh, OW, kw)


def pool_fwd(x, kh, kw):
    """(fp64 means over the kh x kw windows, remainder rows and columns ignored; bound)"""
    w = _windows(x.double(), kh, kw)
    n = kh * kw
    return w.sum((2, 4)) / n, (n + 1) * _E.HALF * w.abs().sum((2, 4)) / n + _E.TINY


def pool_bwd(gy, H, W, kh, kw):
    """(gy / (kh kw) spread over its window, +0 in the remainder; bound: 0 where kh kw is a power of two)"""
    NC, OH, OW = gy.shape
    n = kh * kw
    gx = torch.zeros(NC, H, W, dtype=torch.float64)
    spread = (gy.double() / n).repeat_interleave(kh, 1).repeat_interleave(kw, 2)
    gx[:, :OH * kh, :OW * kw] = spread
    if n & (n - 1) == 0:
        return gx, torch.zeros_like(gx)
    bound = torch.zeros_like(gx)
    bound[:, :OH * kh, :OW * kw] = 2 * _E.HALF * spread.abs() + _E.TINY
    return gx, bound


def pool_restate32(x, gy, kh, kw):
    """float32: the window summed row by row from 0, times fl(1 / (kh kw)); gy times the same"""
    w = _windows(x.float(), kh, kw)
    acc = torch.zeros(w.shape[0], w.shape[1], w.shape[3])
    for a in range(kh):
        for b in range(kw):
            acc = acc + w[:, :, a, :, b]
    inv = torch.tensor(1.0) / torch.tensor(float(kh * kw))
    return acc * inv, gy.float() * inv
