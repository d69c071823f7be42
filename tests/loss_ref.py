"""fp64 statements of every training-loss entry point of remfx_amd/csrc/losses.hip that sections 4.21 / 4.22 do not pin, the forms
their kernels take, per-element bounds and the case tables of tests/test_loss_ref_cpu.py and tests/test_gpu_loss_kernel.py.  numpy only.
Test infrastructure only.

Entry points: rfx_sisdr_sums, rfx_time_sums, rfx_sisdr_finish, rfx_time_loss_rows, rfx_time_loss_grad, rfx_logcosh_rows,
rfx_logcosh_grad, rfx_stft_scaled_loss, rfx_stft_scaled_loss_grad, rfx_mrstft_combine, rfx_mrstft_combine_w (and through them
rfx_slot_sum_kernel<double>).

STATEMENTS.  None of the kernels' decompositions: the filter is applied per sample to zero-padded rows, the adjoint per sample, the
filter bank is a dense matrix, log-cosh is log(cosh(a z) + eps) through logaddexp.  Sums over samples run in numpy.longdouble: the
x87 80-bit format where the platform has it (64-bit significand, `LONGDOUBLE_BITS`); where long double is 64-bit the sums are still
correct to the bound below (the reference's own term then doubles; `REF_U` carries it).  The per-row losses and their
coefficients are functions of five fp64 sums: they are evaluated in EXACT rational arithmetic (fractions.Fraction) on the sums' values
-- the centring, the projection energy and the residual energy carry no rounding at all -- and rounded once; the logarithm is taken of
that correctly rounded ratio.

BOUNDS (eps32 = 2^-23, h = 2^-24 a half-ulp of fp32, u = 2^-53 a half-ulp of fp64; every bound is a per-element vector, none is
measured on a kernel):
  * fp64 arithmetic of the kernels is followed operation by operation by `V`, a value with a first-order running error bound: every
    addition, product and quotient adds u (|result| + carried error) (correctly rounded; a fused multiply-add only removes a rounding),
    a difference carries the errors of both operands in ABSOLUTE terms -- that is what keeps the conditioning of
    Sxx - 2 al Sxt + al^2 Stt, of the centring Sxx - Sx^2 / L and of St - Sx in the bound -- and a quotient divides by |b| - e_b.
    Device libm calls in fp64 (exp, log, log10, sqrt): no accuracy table of the device library is at hand, LIBM_ULP = 4 ulp = 8 u
    relative is ASSUMED.
  * fp64 outputs (sums, coef): that bound plus the reference's own rounding.  fp32 outputs computed in fp64 (rows, out, gx, both
    combines' out, rfx_sisdr_finish): that bound plus a half-ulp of the fp32 result.
  * sums of n terms: every addition a term passes through (trips of the thread's loop + 6 butterfly steps + 2 across the four waves
    + the slot sum's trips + 6) costs u sum |terms|; the term itself is counted (4 u for a three-tap filtered sample, 9 u for a product
    of two, 0 and 1 without taps).
  * the fp32 mel forward is counted in `stft_scaled_loss` (rfx_pow2 2 h, sqrtf h, ceil(len / 8) fused multiply-adds on the lane, three
    butterfly additions, d = c - a; logf by the K rule, `FLOOR`).
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
LONGDOUBLE_BITS = np.finfo(LD).nmant + 1                 # 64 with x87 extended precision, 53 where long double is double
U64, EPS32, H32 = 2.0 ** -53, 2.0 ** -23, 2.0 ** -24
REF_U = 2.0 ** -LONGDOUBLE_BITS                          # a half-ulp of the reference's own sums
LIBM_ULP = 4.0                                           # ASSUMED for device exp / log / log10 / sqrt in fp64
LIBM = LIBM_ULP * 2.0 * U64
SECOND_ORDER = 1.0 + 2.0 ** -16                          # first-order counts are multiplied by this
SLOTS = 128                                              # TIME_SUMS_MAX_SLOTS of losses.hip
MAX_ROWS = 65535                                         # RFX_LOSS_MAX_ROWS
KINDS = ("sisdr", "sdsdr", "snr", "esr", "dc", "logcosh")
REDUCTIONS = ("mean", "sum", "none")
K10 = -4.3429448190325182765                             # the kernel's constant, -10 / ln 10 rounded to fp64
TAPS = ((-0.85, 1.0, 0.0), (0.3, 1.0, -0.5), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
FLOOR = {"logf": 1.5}                                    # measured 1.10 on restate_scaled (test_loss_ref_cpu.py), next half up
K_LOGF = 8.0 * FLOOR["logf"] + 8.0


# ---- grids of the host code --------------------------------------------------------------------------------------------------------
def grid_x(n):
    return int(min(max((n + 2047) // 2048, 1), 512))


def time_sums_grid(L):
    return min(grid_x(L), SLOTS)


def time_stream_grid(units, R):
    want, cap = (units + 1023) // 1024, max(4096 // R, 1)
    return int(max(min(want, cap), 1))


def scaled_grid(frames):
    return int(min(max(frames, 1), 64))


def scaled_grad_grid(frames):
    return int(min(frames, 512))


def slot_sum_grid(n_outputs):
    return (n_outputs + 3) // 4


def sum_adds(trips, g):
    """additions a term passes on its way into a row sum: the thread's loop, the wave butterfly, the four waves, the slot sum"""
    return trips + 6 + 2 + (g + 63) // 64 + 6


# ---- the running error bound ---------------------------------------------------------------------------------------------------------
class V:
    """v: the kernel's formula evaluated in fp64.  Its distance from the exact value, for any fp64 evaluation of the same operations,
    is sum_k t[k] d_k + (something within q) with |d_k| <= 1: one symbol k per rounding, per libm call and per uncertain input, t[k] the
    signed first-order sensitivity of this value to it (so an error two operands share cancels where the formula cancels it, as in
    2 fa Sx + fb St with fb ~ -2 fa), q the second-order remainder.  e = sum_k |t[k]| + q is the bound."""
    _next = [0]

    def __init__(self, v, e=None, t=None, q=0.0):
        self.v = np.asarray(v, np.float64)
        self.t = dict(t) if t else {}
        self.q = np.broadcast_to(np.asarray(q, np.float64), self.v.shape).copy()
        if e is not None and np.any(np.asarray(e) != 0):
            self._sym(np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy())

    def _sym(self, mag):
        V._next[0] += 1
        self.t[V._next[0]] = mag
        return self

    @property
    def e(self):
        out = self.q.copy()
        for c in self.t.values():
            out = out + np.abs(c)
        return out

    def _r(self):
        """one correctly rounded operation"""
        return self._sym(U64 * (np.abs(self.v) + self.e))

    @staticmethod
    def of(a):
        return a if isinstance(a, V) else V(a)

    @staticmethod
    def _lin(a, ca, b, cb):
        t = {k: ca * c for k, c in a.t.items()}
        for k, c in b.t.items():
            t[k] = t[k] + cb * c if k in t else cb * c
        return t

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, t=V._lin(self, 1.0, o, 1.0), q=self.q + o.q)._r()

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, t=V._lin(self, 1.0, o, -1.0), q=self.q + o.q)._r()

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, t={k: -c for k, c in self.t.items()}, q=self.q)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, t=V._lin(self, o.v, o, self.v), q=np.abs(self.v) * o.q + np.abs(o.v) * self.q + self.e * o.e)._r()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            be = o.e
            lo = np.abs(o.v) - be
            ok = lo > 0
            los = np.where(ok, lo, 1.0)
            r = self.v / o.v
            t = V._lin(self, 1.0 / o.v, o, -r / o.v)
            q = np.where(ok, (self.q + np.abs(r) * o.q) / los + (self.e + np.abs(r) * be) * be / (np.abs(o.v) * los), np.inf)
            if not ok.all():
                t = {k: np.where(ok, c, 0.0) for k, c in t.items()}
        return V(r, t=t, q=q)._r()

    def __rtruediv__(self, o):
        return V.of(o) / self

    def log10(self):
        """a libm call: the carried error through f', the remainder through the largest f'' on [v - e, v + e], LIBM of the result"""
        with np.errstate(all="ignore"):
            se = self.e
            lo = self.v - se
            ok = lo > 0
            los = np.where(ok, lo, 1.0)
            r = np.log10(self.v)
            d = 1.0 / (self.v * math.log(10.0))
            t = {k: np.where(ok, d * c, 0.0) for k, c in self.t.items()}
            q = np.where(ok, self.q / (los * math.log(10.0)) + 0.5 * se * se / (los * los * math.log(10.0)), np.where(se > 0, np.inf, 0.0))
        out = V(r, t=t, q=q)
        return out._sym(LIBM * (np.abs(r) + out.e))


def half_ulp32(ref, e=0.0):
    """a half-ulp of the fp32 number the kernel rounds to, which lies within e of ref"""
    m = (np.abs(np.asarray(ref, np.float64)) + e) * (1.0 + EPS32)
    with np.errstate(over="ignore"):
        m32 = np.minimum(m, 3.0e38).astype(np.float32)
    return np.where(m == 0.0, 0.0, 0.5 * np.spacing(m32).astype(np.float64))                  # an exact 0 stays exact


# ---- time family: signals ------------------------------------------------------------------------------------------------------------
def signal_rows(names, R, L, seed):
    """x, t [R, L] float32; row r takes names[r]"""
    rng = np.random.default_rng(seed)
    t = (0.1 * rng.standard_normal((R, L))).astype(np.float32)
    n = rng.standard_normal((R, L))
    x = np.empty_like(t)
    for r in range(R):
        s = names[r]
        if s.startswith("db"):
            x[r] = (t[r].astype(np.float64) + 10.0 ** (-float(s[2:]) / 20.0) * 0.1 * n[r]).astype(np.float32)
        elif s == "gain":
            x[r] = (1.0001 * t[r].astype(np.float64)).astype(np.float32)
        elif s == "same":
            x[r] = t[r]
        elif s == "dc":                                  # a mean 100 times the deviation
            t[r] = (0.5 + 0.005 * n[r]).astype(np.float32)
            x[r] = (t[r].astype(np.float64) + 0.0005 * rng.standard_normal(L)).astype(np.float32)
        elif s == "silent":
            x[r] = t[r]
            t[r] = 0.0
        elif s == "full":                                # full scale
            t[r] = np.where(n[r] >= 0, 1.0, -1.0).astype(np.float32)
            x[r] = t[r] * np.float32(1.0 - 2.0 ** -7)
            x[r, ::7] = -x[r, ::7]
        else:
            raise ValueError(s)
    return x, t


def _c(R, L, taps=None, sig=("db10",), ox=0, ot=0, og=0, xpad=0, tpad=0, kind="sisdr", red="mean", zm=1, **kw):
    names = [sig[r % len(sig)] for r in range(R)]
    for r, s in (kw.pop("special", None) or {}).items():
        names[r] = s
    d = dict(R=R, L=L, taps=taps, sig=tuple(names), ox=ox, ot=ot, og=og, xpad=xpad, tpad=tpad, kind=kind, red=red, zm=zm, seed=1000 + 7 * L + R)
    d.update(kw)
    return d


DBS = ("db10", "db40", "db80", "db120")
SPECIAL = {5: "gain", 11: "same", 17: "dc", 23: "silent", 29: "full"}      # one row each: x == t is 1 of >= 64 rows
TIME_CASES = [
    _c(3, 1, None, ("db10", "db40", "full"), kind="snr", red="sum"),
    _c(3, 2, 0, ("db10", "dc", "db80"), og=1, kind="sisdr", red="none"),
    _c(3, 3, 1, ("db10", "db40", "db80"), og=1, kind="esr"),
    _c(3, 5, 0, ("db10", "full", "db120"), og=1, ox=1, kind="sdsdr", zm=0),
    _c(3, 63, 1, ("db40", "dc", "db10"), ox=1, kind="dc", red="sum"),
    _c(1, 64, 0, ("db10",), kind="snr", zm=0),
    _c(3, 65, 2, ("db10", "db80", "full"), ot=2, kind="sisdr", zm=0, red="none"),
    _c(3, 255, 3, ("db120", "db10", "dc"), og=3, kind="esr", red="none", value="the taps (1, 0, 0), a pure shift: a value case"),
    _c(1, 256, 0, ("db40",), kind="sdsdr", value="exactly one full workgroup, the size below the second trip: a value case"),
    _c(3, 257, 1, ("db10", "db40", "db80"), xpad=3, tpad=5, kind="snr"),
    _c(3, 1003, 0, ("db10", "db40", "db80"), ox=1, ot=2, og=3, kind="sisdr"),
    _c(3, 1027, None, ("db120", "dc", "full"), og=2, ox=1, kind="sdsdr", red="sum"),
    _c(3, 1031, 1, ("db120", "db80", "db10"), ot=3, kind="dc"),
    _c(3, 2049, 1, ("db80", "db10", "full"), xpad=7, kind="snr", red="none"),
    _c(3, 4101, 0, ("db10", "db40", "dc"), og=1, ot=1, kind="esr", red="sum"),
    _c(1, 262147, 0, ("db10",), kind="sisdr"),
    _c(64, 65, None, DBS, special=SPECIAL, kind="sisdr", red="none"),
    _c(65, 66, 0, DBS, special=SPECIAL, og=2, kind="snr"),
    _c(130, 70, 1, DBS, special=SPECIAL, ox=3, ot=1, og=1, xpad=1, kind="sdsdr", red="sum", value="R = 130, a third row per lane of the one-wave tails: a value case"),
    _c(4097, 5, None, ("db10", "db40"), kind="esr"),
    _c(3, 131072, None, ("db10",), kind="dc"),
]


def case_id(c):
    t = "n" if c["taps"] is None else str(c["taps"])
    return f"R{c['R']}-L{c['L']}-t{t}-{c['kind']}-{c['red']}"


def time_data(c):
    """x, t as flat float32 buffers with their row strides (the padding holds 1e30: a halo read across a row end shows), and [R, L] views"""
    x, t = signal_rows(c["sig"], c["R"], c["L"], c["seed"])
    out = []
    for a, pad in ((x, c["xpad"]), (t, c["tpad"])):
        rs = c["L"] + pad
        buf = np.full(c["R"] * rs, 1.0e30, np.float32)
        buf.reshape(c["R"], rs)[:, :c["L"]] = a
        out.append((buf, rs))
    return x, t, out[0], out[1]


def gup_of(c):
    R = c["R"]
    return (0.5 + np.arange(R if c["red"] == "none" else 1) % 5 * 0.25).astype(np.float32) * np.float32(-1.0 if c["red"] == "sum" else 1.0)


# ---- time family: statements --------------------------------------------------------------------------------------------------------
def filt(s, taps):
    """s~[n] = h_prev s[n-1] + h_cur s[n] + h_next s[n+1], zeros outside the row; per sample.  -> (value, sum of |terms|)"""
    s = np.asarray(s, LD)
    if taps is None:
        return s, np.abs(s)
    z = np.zeros(s.shape[:-1] + (1,), LD)
    p = np.concatenate([z, s, z], -1)
    hp, hc, hn = (LD(h) for h in taps)
    return hp * p[..., :-2] + hc * p[..., 1:-1] + hn * p[..., 2:], abs(hp) * np.abs(p[..., :-2]) + abs(hc) * np.abs(p[..., 1:-1]) + abs(hn) * np.abs(p[..., 2:])


def row_sums(x, t, taps):
    """[R, 5] { Sx, St, Sxt, Sxx, Stt } of the filtered rows and the bound of rfx_time_sums / rfx_sisdr_sums"""
    xf, xa = filt(x, taps)
    tf, ta = filt(t, taps)
    L = x.shape[-1]
    g = time_sums_grid(L)
    adds = sum_adds((L + g * 256 - 1) // (g * 256), g)
    c1, c2 = (4, 9) if taps is not None else (0, 1)
    s = np.stack([xf.sum(-1), tf.sum(-1), (xf * tf).sum(-1), (xf * xf).sum(-1), (tf * tf).sum(-1)], -1)
    a = np.stack([xa.sum(-1), ta.sum(-1), (xa * ta).sum(-1), (xa * xa).sum(-1), (ta * ta).sum(-1)], -1).astype(np.float64)
    cnt = np.array([c1, c1, c2, c2, c2], np.float64) + adds
    ref_adds = math.ceil(math.log2(max(L, 2))) + 8 + (L // 128 if LONGDOUBLE_BITS < 64 else 0)
    bound = (U64 * cnt * SECOND_ORDER + REF_U * (cnt + ref_adds)) * a + U64 * np.abs(s.astype(np.float64))
    return s.astype(np.float64), bound


def _frac_rows(kind, s5, L, zm, eps):
    """one row, exact: the loss's rational argument and its derivatives in the raw sums.  -> (val, (a, b, c)) as floats"""
    sx, st, sxt, sxx, stt = (Fraction(float(v)) for v in s5)
    e, Lf = Fraction(float(eps)), Fraction(int(L))
    if kind == "esr":
        return float((stt - 2 * sxt + sxx) / (stt + e)), (float(2 / (stt + e)), float(-2 / (stt + e)), 0.0)
    if kind == "dc":
        d, den = (st - sx) / Lf, stt / Lf + e
        return float(d * d / den), (0.0, 0.0, float(-2 * d / Lf / den))
    if zm:                                               # the energies of x - mean(x), t - mean(t) and their inner product
        sxt, sxx, stt = sxt - sx * st / Lf, sxx - sx * sx / Lf, stt - st * st / Lf
    if kind == "snr":                                    # |t|^2 / (|x - t|^2 + eps) + eps
        den = sxx - 2 * sxt + stt + e
        q, dq_xx, dq_xt = stt / den + e, -stt / den ** 2, 2 * stt / den ** 2
    else:
        al = sxt / (stt + e)                             # the projection al t
        tt, dtt = al * al * stt, 2 * al * stt / (stt + e)
        if kind == "sisdr":                              # |x - al t|^2
            res = sxx - 2 * al * sxt + tt
            dres = -4 * sxt / (stt + e) + dtt
        else:                                            # |x - t|^2
            res, dres = sxx - 2 * sxt + stt, Fraction(-2)
        den = res + e
        q = tt / den + e
        dq_xx, dq_xt = -tt / den ** 2, (dtt * den - tt * dres) / den ** 2
    k = LD(-10.0) / np.log(LD(10.0))
    fa, fb = k * LD(float(dq_xx / q)), k * LD(float(dq_xt / q))
    cc = -(2 * fa * LD(float(sx)) + fb * LD(float(st))) / LD(L) if zm else LD(0.0)
    val = -10.0 * math.log10(float(q)) if q > 0 else float("nan")
    return val, (float(2 * fa), float(fb), float(cc))


def _rows_V(kind, sums, L, zm, eps):
    """the kernel's formulas of time_loss_rows_kernel / sisdr_finish_kernel under V.  -> (val, res + eps or None, ca, cb, cc)"""
    S = sums if isinstance(sums, V) else V(sums)
    col = lambda k: V(S.v[:, k], S.e[:, k])                 # an uncertain input sum is a symbol of its own
    sx, st, sxt, sxx, stt = (col(k) for k in range(5))
    zero = V(np.zeros(S.v.shape[0]))
    Lf = float(L)
    if kind == "esr":
        inv = 1.0 / (stt + eps)
        return (stt - 2.0 * sxt + sxx) * inv, None, 2.0 * inv, -2.0 * inv, zero
    if kind == "dc":
        d, inv = (st - sx) / Lf, 1.0 / (stt / Lf + eps)
        return d * d * inv, None, zero, zero, -2.0 * d / Lf * inv
    if zm:
        sxt, sxx, stt = sxt - sx * st / Lf, sxx - sx * sx / Lf, stt - st * st / Lf
    k10 = V(np.full(S.v.shape[0], K10), U64 * abs(K10))
    if kind == "snr":
        den = sxx - 2.0 * sxt + stt + eps
        q = stt / den + eps
        lg = q.log10()
        fa = k10 / q * (-stt / (den * den))
        fb = -2.0 * fa
    else:
        ia = 1.0 / (stt + eps)
        alpha = sxt / (stt + eps)
        tt = alpha * alpha * stt
        if kind == "sisdr":
            res = sxx - 2.0 * alpha * sxt + tt
            dres = -2.0 * alpha - 2.0 * sxt * ia + 2.0 * alpha * stt * ia
        else:
            res, dres = sxx - 2.0 * sxt + stt, V(np.full(S.v.shape[0], -2.0))
        den = res + eps
        q = tt / den + eps
        lg = q.log10()
        dtt = 2.0 * alpha * stt * ia
        fa = k10 / q * (-tt / (den * den))
        fb = k10 / q * ((dtt * den - tt * dres) / (den * den))
    cc = -(2.0 * fa * sx + fb * st) / Lf if zm else zero
    return -(10.0 * lg), den, 2.0 * fa, fb, cc


RESIDUAL_ROWS = (0.0, 0.5, 1.0)                          # the share of the energy that sits in the mean


def residual_bound(S, eps=1e-8):
    """the bound of res + eps of x == t rows with Sxx + Stt = S, for every logarithmic kind, centred or not, and every share of the energy
    in the mean (1: the centred sums cancel completely and alpha = 0 / eps).  -> {(kind, zm): [bound per row]}.  A bound that is not
    finite says that Stt' + eps, the denominator of alpha, may itself be non-positive: S is beyond the limit then."""
    L = 1000.0
    rows = np.array([[np.sqrt(m * 0.5 * S * L), np.sqrt(m * 0.5 * S * L), 0.5 * S, 0.5 * S, 0.5 * S] for m in RESIDUAL_ROWS])
    out = {}
    for kind in ("sisdr", "sdsdr", "snr"):
        for zm in (0, 1):
            with np.errstate(all="ignore"):
                e = _rows_V(kind, rows, L, zm, eps)[1].e
            out[(kind, zm)] = np.where(np.isfinite(e), e, np.inf)
    return out


def residual_limit(eps=1e-8):
    """the Sxx + Stt beyond which the bound of the residual energy reaches eps, so that res + eps may turn non-positive: the smallest
    over the kinds, centring and rows of `residual_bound`, by bisection (the bound grows with S)"""
    worst = lambda S: max(float(e.max()) for e in residual_bound(S, eps).values())
    lo, hi = 1.0, 1.0e12
    assert worst(lo) < eps < worst(hi)
    for _ in range(60):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if worst(mid) < eps else (lo, mid)
    b = residual_bound(lo, eps)
    assert len(b) == 6 and all(e.shape == (len(RESIDUAL_ROWS),) and np.isfinite(e).all() for e in b.values()), b
    return lo


def _reduce_V(terms, R, mean):
    """acc over the rows in lane order and the butterfly, / R: u per addition on the sum of |terms|"""
    adds = (R + 63) // 64 + 6 + 2
    tot, e = terms.v.sum(), terms.e.sum() + U64 * adds * SECOND_ORDER * (np.abs(terms.v) + terms.e).sum()
    return (tot / R, e / R) if mean else (tot, e)


def time_loss_rows(sums, L, kind, zm=1, eps=1e-8, reduction="mean", sums_err=None):
    """-> dict rows, coef, out (None for "none") and *_bound.  sums_err: a bound of the sums passed in (the chained test)"""
    sums = np.asarray(sums, np.float64)
    R = sums.shape[0]
    if kind == "logcosh":
        rows = sums[:, 0].astype(LD) / LD(L)
        e = (np.zeros(R) if sums_err is None else sums_err[:, 0]) / L + U64 * np.abs(sums[:, 0]) / L
        coef, ce = np.zeros((R, 3)), np.zeros((R, 3))
        val = V(rows.astype(np.float64), e)
    else:
        ex = [_frac_rows(kind, sums[r], L, zm, eps) for r in range(R)]
        rows = np.array([v for v, _ in ex], LD)
        coef = np.array([c for _, c in ex], np.float64)
        with np.errstate(all="ignore"):                  # 0 x inf among the sensitivities of a fully cancelled row; the tests assert finite bounds
            val, _, ca, cb, cc = _rows_V(kind, V(sums, 0.0 if sums_err is None else sums_err), L, zm, eps)
        ce = np.stack([ca.e, cb.e, cc.e], -1) + 4.0 * U64 * np.abs(coef)          # the reference's own roundings
        e = val.e + 3.0 * U64 * np.abs(val.v)
    rows64 = rows.astype(np.float64)
    out = dict(rows=rows64, rows_bound=e + half_ulp32(rows64, e), coef=coef, coef_bound=ce, rows_ld=rows, rows_err=e)
    return reduce_rows(out, reduction)


def reduce_rows(r, reduction):
    """out and its bound for a reduction, from the rows of time_loss_rows (the per-row part is the same for all three)"""
    out = dict(r)
    R = r["rows"].shape[0]
    if reduction != "none":
        tot, te = _reduce_V(V(r["rows"], r["rows_err"]), R, reduction == "mean")
        ref = float(r["rows_ld"].sum() / (R if reduction == "mean" else 1))
        out["out"], out["out_bound"] = np.array([ref]), np.array([te + half_ulp32(ref, te)])
    else:
        out["out"] = None
    return out


def sisdr_finish(sums, L, zm, eps=1e-8):
    r = time_loss_rows(sums, L, "sisdr", zm, eps, "mean")
    return r["out"], r["out_bound"]


def time_loss_grad(x, t, coef, taps, gup, reduction, coef_err=None):
    """gx[r][n] = g_r (h_prev u[n+1] + h_cur u[n] + h_next u[n-1]), u = a x~ + b t~ + c inside the row, 0 outside; per sample.
    Bound: a half-ulp of the fp32 result + u x 12 (6 without taps) x the same expression on absolute values
    (g / R, g coef, three products and two additions of the filter, a x~, two additions, h u, two additions)."""
    R, L = x.shape
    g = np.asarray(gup, np.float64).astype(LD)
    g = g if reduction == "none" else np.full(R, g[0] / (LD(R) if reduction == "mean" else LD(1)))
    co = np.asarray(coef, np.float64).astype(LD) * g[:, None]
    xf, xa = filt(x, taps)
    tf, ta = filt(t, taps)
    u = co[:, 0:1] * xf + co[:, 1:2] * tf + co[:, 2:3]
    ua = np.abs(co[:, 0:1]) * xa + np.abs(co[:, 1:2]) * ta + np.abs(co[:, 2:3])
    ue = None
    if coef_err is not None:
        ce = np.asarray(coef_err, np.float64) * np.abs(g.astype(np.float64))[:, None]
        ue = ce[:, 0:1] * xa.astype(np.float64) + ce[:, 1:2] * ta.astype(np.float64) + ce[:, 2:3]
    if taps is None:
        ref, mag, cnt = u, ua, 6.0
    else:
        hp, hc, hn = (LD(h) for h in taps)
        z = np.zeros((R, 1), LD)
        adj = lambda w, a, b, c: a * np.concatenate([w[:, 1:], z], 1) + b * w + c * np.concatenate([z, w[:, :-1]], 1)
        ref, mag, cnt = adj(u, hp, hc, hn), adj(ua, abs(hp), abs(hc), abs(hn)), 12.0
        if ue is not None:
            ue = adj(ue.astype(LD), abs(hp), abs(hc), abs(hn)).astype(np.float64)
    ref, e = ref.astype(np.float64), (cnt * U64 * SECOND_ORDER + 8 * REF_U) * mag.astype(np.float64)
    if ue is not None:
        e = e + ue
    return ref, e + half_ulp32(ref, e)


# ---- log-cosh -------------------------------------------------------------------------------------------------------------------------
def _logcosh_terms(x, t, a, eps):
    y = np.abs(LD(a) * (np.asarray(x, LD) - np.asarray(t, LD)))
    with np.errstate(divide="ignore"):
        ref = np.logaddexp(np.logaddexp(y, -y) - np.log(LD(2.0)), np.log(LD(eps)))      # log(cosh y + eps)
    y = y.astype(np.float64)
    e1 = np.exp(-y)
    arg = 0.5 * (1.0 + e1 * e1) + eps * e1
    de1 = (LIBM / U64 + 2.0 * y + 2.0)                                                    # of e1, relative, in u: y carries 2 u
    darg = ((2.0 * de1 + 3.0) * e1 * e1 + (de1 + 2.0) * eps * e1 + 2.0 * arg) * U64
    e = 2.0 * U64 * y + darg / arg + LIBM * np.abs(np.log(arg)) + U64 * np.abs(ref.astype(np.float64))
    return ref, e * SECOND_ORDER


def logcosh_rows(x, t, a, eps=1e-8):
    """sums[r] = sum_n log(cosh(a z) + eps) / a and the bound of rfx_logcosh_rows"""
    ref, e = _logcosh_terms(x, t, a, eps)
    L = x.shape[-1]
    g = time_sums_grid(L)
    adds = sum_adds((L + g * 256 - 1) // (g * 256), g) + 2
    s = (ref.sum(-1) / LD(a)).astype(np.float64)
    bound = (e.sum(-1) + (U64 * adds * SECOND_ORDER + REF_U * (adds + 24)) * np.abs(ref.astype(np.float64)).sum(-1)) / a + U64 * np.abs(s)
    return s[:, None], bound[:, None]


def logcosh_grad(x, t, a, eps, gup, reduction):
    """gx = g_r sinh(a z) / (cosh(a z) + eps) / L from the definition (longdouble holds cosh(800)).  z = 0 gives 0 exactly (bound 0)."""
    assert LONGDOUBLE_BITS >= 64 or float(np.abs(a * (x.astype(np.float64) - t)).max()) < 700.0
    R, L = x.shape
    g = np.asarray(gup, np.float64).astype(LD)
    g = g if reduction == "none" else np.full(R, g[0] / (LD(R) if reduction == "mean" else LD(1)))
    z = LD(a) * (np.asarray(x, LD) - np.asarray(t, LD))
    ref = ((g / LD(L))[:, None] * np.sinh(z) / (np.cosh(z) + LD(eps))).astype(np.float64)
    y = np.abs(z).astype(np.float64)
    e1 = np.exp(-y)
    e2 = e1 * e1
    de1 = LIBM / U64 + 2.0 * y + 2.0
    num, den = 1.0 - e2, 1.0 + e2 + 2.0 * eps * e1
    dnum = ((2.0 * de1 + 1.0) * e2 + num) * U64
    dden = ((2.0 * de1 + 1.0) * e2 + 2.0 * eps * e1 * (de1 + 2.0) + 2.0 * den) * U64
    with np.errstate(all="ignore"):
        rel = np.where(num > 0, dnum / np.where(num > 0, num, 1.0), 0.0) + dden / den + 6.0 * U64
    e = np.abs(ref) * rel * SECOND_ORDER
    return ref, np.where(y == 0.0, 0.0, e + half_ulp32(ref, e))


LOGCOSH_CASES = [
    dict(R=3, L=5, a=0.5, red="mean", scale=1.0, seed=1),
    dict(R=3, L=257, a=1.0, red="none", scale=1.0, seed=2, xpad=3),
    dict(R=1, L=2049, a=50.0, red="sum", scale=16.0, seed=3),          # |a z| up to 800
    dict(R=4097, L=5, a=1.0, red="mean", scale=1.0, seed=4),
    dict(R=1, L=262147, a=1.0, red="mean", scale=1.0, seed=5),
]


def logcosh_data(c):
    rng = np.random.default_rng(c["seed"])
    R, L = c["R"], c["L"]
    t = (0.1 * rng.standard_normal((R, L))).astype(np.float32)
    x = (t + 0.05 * rng.standard_normal((R, L))).astype(np.float32)
    x[:, 0] = t[:, 0]                                                   # z = 0
    if L > 2:
        x[:, 1] = t[:, 1] - np.float32(0.25)                            # a negative z
        x[:, 2] = np.nextafter(t[:, 2], np.float32(1))                  # the smallest positive z
    if c["scale"] != 1.0:
        t[:, 3::5], x[:, 3::5] = -np.float32(c["scale"] / 2), np.float32(c["scale"] / 2)      # a z = 50 * 16 = 800
        t[:, 4::5], x[:, 4::5] = np.float32(c["scale"] / 2), -np.float32(c["scale"] / 2)
    return x, t


# ---- combines ---------------------------------------------------------------------------------------------------------------------------
def mrstft_combine(sums, n, per_example):
    """sums: list of [R, 3] float32; out = mean_k (sc_k + lm_k).  Bound: sqrtf and the fp32 quotient are correctly rounded (3 h of each
    sc term; the batch form rounds the two sums to fp32 first: 3 h again), fp64 additions u each, a half-ulp of the result."""
    tot, e = LD(0), 0.0
    for s, nk in zip(sums, n):
        s = np.asarray(s, np.float32).astype(LD)
        R = s.shape[0]
        adds = (R + 63) // 64 + 6 + 4
        sc = (np.sqrt(s[:, 0] / s[:, 1])).sum() / LD(R) if per_example else np.sqrt(s[:, 0].sum() / s[:, 1].sum())
        lm = s[:, 2].sum() / (LD(R) * LD(nk))
        tot = tot + sc + lm
        e += float(abs(sc)) * (3.0 * H32 + U64 * adds) * SECOND_ORDER + float(np.abs(s[:, 2]).sum() / (R * nk)) * U64 * adds + U64 * float(abs(sc) + abs(lm)) * 2
    ref = float(tot / LD(len(sums)))
    e = e / len(sums) + 2 * U64 * abs(ref)
    return np.array([ref]), np.array([e + half_ulp32(ref, e)])


def mrstft_combine_w(sums, n, per_example, w):
    """sums: list of [R, 4] float64; a term whose weight is 0 is left out, whatever its sum holds"""
    tot, e = LD(0), 0.0
    w = [float(np.float32(v)) for v in w]
    for s, nk in zip(sums, n):
        s = np.asarray(s, np.float64).astype(LD)
        R = s.shape[0]
        adds = (R + 63) // 64 + 6 + 4
        cells = LD(R) * LD(nk)
        if w[0] != 0.0:
            sc = (np.sqrt(s[:, 0]) / np.sqrt(s[:, 1])).sum() / LD(R) if per_example else np.sqrt(s[:, 0].sum()) / np.sqrt(s[:, 1].sum())
            tot = tot + LD(w[0]) * sc
            e += abs(w[0]) * float(abs(sc)) * (2 * LIBM + U64 * (adds + 3)) * SECOND_ORDER
        for j, col in ((1, 2), (2, 3)):
            if w[j] != 0.0:
                tot = tot + LD(w[j]) * (s[:, col].sum() / cells)
                e += abs(w[j]) * float(np.abs(s[:, col]).sum() / cells) * U64 * (adds + 3)
    ref = float(tot / LD(len(sums)))
    e = e / len(sums) + 2 * U64 * abs(ref)
    return np.array([ref]), np.array([e + half_ulp32(ref, e)])


COMBINE_CASES = [dict(nres=1, R=1, pe=1), dict(nres=3, R=64, pe=0), dict(nres=8, R=65, pe=1), dict(nres=3, R=130, pe=0, value="R = 130 over the batch: a value case"),
                 dict(nres=1, R=130, pe=1, value="per example with R > 128: a value case")]
COMBINE_WEIGHTS = ((1.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.0, 2.0))


def combine_data(c, cols):
    rng = np.random.default_rng(50 + c["nres"] + c["R"])
    sums = [np.abs(rng.standard_normal((c["R"], cols))) * (10.0 ** k) + 0.1 for k in range(c["nres"])]
    n = [int(1000 * (k + 1) + 17) for k in range(c["nres"])]
    return sums, n


# ---- scaled family ----------------------------------------------------------------------------------------------------------------------
def pack(dense):
    """remfx_amd.losses.pack_banded restated: first non-zero column, length to the last one, offset"""
    d = np.asarray(dense, np.float32)
    idx, w, off = np.zeros((d.shape[0], 3), np.int32), [], 0
    for r in range(d.shape[0]):
        nz = np.nonzero(d[r])[0]
        first, ln = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        idx[r] = (first, ln, off)
        w.append(d[r, first:first + ln])
        off += ln
    w = np.concatenate(w) if off else np.zeros(0, np.float32)
    return idx, (w if w.size else np.zeros(1, np.float32))


def unpack(idx, w, cols):
    d = np.zeros((idx.shape[0], cols), np.float32)
    for r, (first, ln, off) in enumerate(np.asarray(idx)):
        d[r, first:first + ln] = w[off:off + ln]
    return d


def hand_bank(n_out, bins, lens, seed=0):
    """a dense (n_out, bins) bank of bands with the given lengths in turn: neighbours overlap, the last band ends at the last bin"""
    rng = np.random.default_rng(900 + seed + n_out)
    d = np.zeros((n_out, bins), np.float32)
    first = 0
    for f in range(n_out):
        ln = min(lens[f % len(lens)], bins)
        if f == n_out - 1:
            first = bins - ln
        first = min(first, bins - ln)
        d[f, first:first + ln] = (0.05 + rng.random(ln)).astype(np.float32)
        first = min(first + max(ln // 2, 1), bins - 1)
    return d


def _s(R, frames, bins, bank, w=(1.0, 1.0, 0.0), pe=1, store=1, gup=1, **kw):
    d = dict(R=R, frames=frames, bins=bins, bank=bank, w=w, pe=pe, store=store, gup=gup, seed=R * 1000 + frames * 10 + bins)
    d.update(kw)
    return d


LENS = (1, 7, 8, 9, 17)
SCALED_CASES = [
    _s(1, 1, 9, None, store=0),
    _s(3, 2, 9, None, w=(0.5, 0.0, 2.0)),
    _s(1, 1, 9, ("hand", 1, (9,)), w=(0.0, 0.0, 1.0), gup=0),
    _s(3, 2, 9, ("hand", 5, LENS), pe=0),
    _s(1, 64, 257, ("hand", 32, LENS)),
    _s(1, 65, 257, ("hand", 33, LENS), w=(0.5, 0.0, 2.0), pe=0),
    _s(3, 2, 513, ("hand", 80, LENS), value="bins = 513, n_out = 80: a third trip of both loops, a value case"),
    _s(1, 1, 513, ("hand", 300, LENS), w=(0.0, 0.0, 1.0)),
    _s(65, 1, 9, ("hand", 5, LENS), pe=0),
    _s(65, 1, 9, ("hand", 5, LENS), pe=1, gup=0, value="per example at R > 64: a value case"),
    _s(1, 513, 9, ("hand", 5, LENS), w=(0.5, 0.0, 2.0)),
    _s(3, 2, 9, ("mel", 16, 2), value="the module's own mel table at n_fft = 16: a value case"),
    _s(1, 2, 257, ("mel", 512, 40), pe=0, value="the module's own mel table at n_fft = 512: a value case"),
    _s(1, 2, 257, None, store=1, value="the identity at bins > 256: second trip of the bin loop"),
]
EMPTY_CASE = _s(1, 2, 9, ("hand", 5, (3, 0, 4, 2, 5)))
SR = 48000


def scaled_id(c):
    b = "id" if c["bank"] is None else "-".join(str(v) for v in c["bank"][:2])
    return f"R{c['R']}-f{c['frames']}-b{c['bins']}-{b}-pe{c['pe']}-w{c['w'][0]}_{c['w'][1]}_{c['w'][2]}"


def bank_of(c, mel=None):
    """the dense filter bank of a case (None: identity).  mel: remfx_amd.losses.mel_filterbank, passed in by the tests (numpy only here)"""
    b = c["bank"]
    if b is None:
        return None
    if b[0] == "hand":
        return hand_bank(b[1], c["bins"], b[2], c["frames"])
    assert b[0] == "mel" and mel is not None and c["bins"] == b[1] // 2 + 1
    return np.asarray(mel(SR, b[1], b[2]), np.float32)


EPS_F = np.float32(1e-8)


def _placed():
    """(re, im) with rfx_pow2 = fma(im, im, fl32(re re)) exactly nextbelow(eps), eps, nextabove(eps): fl32(re re) is the target or the
    float below it, and im^2 is the difference to a 1e-7 of it, so neither rounding is near a tie"""
    out = []
    for target in (np.nextafter(EPS_F, np.float32(0)), EPS_F, np.nextafter(EPS_F, np.float32(1))):
        re = np.float32(math.sqrt(float(target)))
        while np.float32(np.float64(re) * np.float64(re)) > target:
            re = np.nextafter(re, np.float32(0))
        r = np.float32(np.float64(re) * np.float64(re))
        im = np.float32(math.sqrt(float(target) - float(r)))
        assert float(target) - float(r) <= 2 * float(np.spacing(target))
        out.append((re, im))
    return out


PLACED = _placed()


def scaled_data(c):
    """xc, yc [R, frames, bins, 2] float32.  Cells 0 ... 2 of the first line of x: px placed just below, at and just above eps; cell 3:
    far below eps (clamped); the last line of y equals x's (sign 0; its last cell where there is one line only)"""
    rng = np.random.default_rng(c["seed"])
    sh = (c["R"], c["frames"], c["bins"], 2)
    x = (0.1 * rng.standard_normal(sh)).astype(np.float32)
    y = (x + 0.05 * rng.standard_normal(sh)).astype(np.float32)
    for k, cell in enumerate(PLACED):
        x[0, 0, k] = cell
    x[0, 0, 3] = (1e-6, -2e-6)
    y[0, 0, 4] = (3e-6, 1e-6)
    if c["R"] * c["frames"] > 1:
        y[-1, -1] = x[-1, -1]
    else:
        y[0, 0, -1] = x[0, 0, -1]
    return x, y


def placed_cells(c):
    return [(0, 0, k) for k in range(3)]


def px32(x):
    """rfx_pow2 in float32: fma(im, im, fl32(re re)), the fused sum formed in fp64 (exact unless it needs more than 53 bits, and then
    a tie of the fp32 rounding is 2^-29 away at the least for every cell `margins` admits)"""
    re, im = x[..., 0].astype(np.float64), x[..., 1].astype(np.float64)
    return ((re * re).astype(np.float32).astype(np.float64) + im * im).astype(np.float32)


def margins(x, eps=EPS_F):
    """every cell's distance of the exact power re^2 + im^2 from eps, in fp32 roundings (half-ulps of eps)"""
    p = x[..., 0].astype(LD) ** 2 + x[..., 1].astype(LD) ** 2
    return (np.abs(p - LD(eps)) / LD(0.5 * float(np.spacing(eps)))).astype(np.float64)


def _mags(xc, eps):
    p = xc[..., 0].astype(LD) ** 2 + xc[..., 1].astype(LD) ** 2
    return np.sqrt(np.maximum(p, LD(eps)))


def scaled_adds(c, n_out):
    g = scaled_grid(c["frames"])
    per_frame = (n_out + 31) // 32 if c["bank"] is not None else (c["bins"] + 255) // 256
    return sum_adds(((c["frames"] + g - 1) // g) * per_frame, g)


def stft_scaled_loss(xc, yc, fb, eps=EPS_F, adds=32):
    """M = fb |X| with |X| = sqrt(max(|X|^2, eps)) as a dense product (fb None: the identity).
    -> dict sums [R, 4], mx, my [R, frames, n_out] and their bounds (the count is in the module docstring and DESIGN.md 4.24)"""
    ax, ay = _mags(xc, eps), _mags(yc, eps)
    if fb is None:
        mx, my, dmx, dmy = ax, ay, 2 * H32 * ax, 2 * H32 * ay
    else:
        F = np.asarray(fb, np.float32).astype(LD)
        idx, _ = pack(fb)
        depth = (np.ceil(idx[:, 1] / 8.0) + 2 + 3) * H32 * SECOND_ORDER
        mx, my = ax @ F.T, ay @ F.T
        dmx, dmy = (ax @ np.abs(F).T) * depth, (ay @ np.abs(F).T) * depth
    dmx, dmy = dmx.astype(np.float64), dmy.astype(np.float64)
    a, c = mx.astype(np.float64), my.astype(np.float64)
    d = c - a
    dd = dmx + dmy + H32 * (np.abs(d) + dmx + dmy)
    with np.errstate(all="ignore"):
        la, lc = np.log(mx), np.log(my)
        terms = np.stack([(my - mx) ** 2, my * my, np.abs(la - lc), np.abs(mx - my)], -1)
        G = (np.abs(la) + np.abs(lc)).astype(np.float64)
        bt = np.stack([2 * np.abs(d) * dd + dd * dd, 2 * c * dmy + dmy * dmy, dmx / a + dmy / c + K_LOGF * EPS32 * G, dd], -1)
    sums = terms.sum((1, 2))
    t64 = terms.astype(np.float64)
    sb = bt.sum((1, 2)) + (U64 * adds * SECOND_ORDER + REF_U * 40) * np.abs(t64).sum((1, 2)) + U64 * np.abs(sums.astype(np.float64))
    return dict(sums=sums.astype(np.float64), sums_bound=sb, mx=a, my=c, mx_bound=dmx, my_bound=dmy)


def restate_scaled(xc, yc, fb, eps=EPS_F):
    """the kernel's arithmetic in numpy float32: rfx_pow2 and sqrtf per magnitude, lane j of a filter's eight takes elements j, j + 8, ...
    with a fused multiply-add each (one rounding: the fp64 sum of the exact product and the accumulator, rounded to fp32), the xor
    butterfly 4, 2, 1.  -> mx, my, and the per-cell log terms |logf(a) - logf(c)|"""
    f32 = np.float32
    mag = [np.sqrt(np.maximum(px32(v), eps)).astype(f32) for v in (xc, yc)]
    if fb is None:
        a, c = mag
    else:
        idx, w = pack(fb)
        out = []
        for m in mag:
            M = np.zeros(m.shape[:2] + (idx.shape[0],), f32)
            for f, (first, ln, off) in enumerate(idx):
                part = [np.zeros(m.shape[:2], f32) for _ in range(8)]
                for i in range(ln):
                    j = i % 8
                    part[j] = (np.float64(w[off + i]) * m[..., first + i].astype(np.float64) + part[j].astype(np.float64)).astype(f32)
                for o in (4, 2, 1):
                    part = [(part[j] + part[j ^ o]).astype(f32) for j in range(8)]
                M[..., f] = part[0]
            out.append(M)
        a, c = out
    with np.errstate(all="ignore"):
        lt = np.abs((np.log(a) - np.log(c)).astype(f32))
    return a, c, lt


def stft_scaled_loss_grad(xc, mx, my, sums, fb, w, per_example, gup, eps=EPS_F):
    """gxc = (fb^T dM) X / |X| where px > eps, else 0; dM = ksc (Mx - My) + (w_lm / Mx + w_lin) sign(Mx - My), given mx, my (float32) and
    sums (float64) as passed in: the sign and px > eps are exact on the inputs (px as rfx_pow2 forms it; `margins`).
    Bound: ksc 2 h, the difference and the product 2 h, (w_lm u) / Mx 3 h, + w_lin u 2 h and h, the sum h: dM within
    h (5 |t1| + 4 |w_lm / Mx| + 3 |w_lin|); one fused multiply-add per listed filter (the band's length deep); rfx_pow2, sqrtf, the
    quotient and the product 4 h."""
    R, frames, bins, _ = xc.shape
    u = LD(1.0) if gup is None else LD(float(np.float32(gup)))
    w_sc, w_lm, w_lin = (LD(float(np.float32(v))) * u for v in w)
    S = np.asarray(sums, np.float64).astype(LD)
    A, B = (S[:, 0], S[:, 1]) if per_example else (np.full(R, S[:, 0].sum()), np.full(R, S[:, 1].sum()))
    with np.errstate(all="ignore"):
        ksc = np.where((A > 0) & (B > 0), w_sc / (np.sqrt(A) * np.sqrt(B)), LD(0))[:, None, None]
        a, c = np.asarray(mx, np.float32).astype(LD), np.asarray(my, np.float32).astype(LD)
        t1, t2, sg = ksc * (a - c), w_lm / a, np.sign(a - c)
        dm = t1 + (t2 + w_lin) * sg
        ddm = H32 * (5 * np.abs(t1) + (4 * np.abs(t2) + 3 * abs(w_lin)) * np.abs(sg)) * SECOND_ORDER
        if fb is None:
            d, dd, D = dm, ddm, np.abs(dm)
        else:
            F = np.asarray(fb, np.float32).astype(LD)
            tidx, _ = pack(np.asarray(fb, np.float32).T)
            listed = np.zeros(F.T.shape, bool)                                  # the band of fb^T: interior zeros are listed too
            for b, (first, ln, _) in enumerate(tidx):
                listed[b, first:first + ln] = True
            bad = ~np.isfinite(dm)
            d = np.where(bad, LD(0), dm) @ F
            hit = (bad.astype(np.float64) @ listed.T.astype(np.float64)) > 0
            d = np.where(hit, LD(np.nan), d)
            D = np.where(bad, LD(0), np.abs(dm)) @ np.abs(F)
            dd = np.where(bad, LD(0), ddm) @ np.abs(F) + tidx[:, 1].astype(np.float64) * H32 * D
    px = px32(xc)
    on = px > eps
    p = xc[..., 0].astype(LD) ** 2 + xc[..., 1].astype(LD) ** 2
    with np.errstate(all="ignore"):
        inv = np.where(on, 1 / np.sqrt(np.where(on, p, LD(1))), LD(0))
        g = (np.where(on, d, LD(0)) * inv)[..., None] * xc.astype(LD)
        e = ((dd + 4 * H32 * SECOND_ORDER * D) * inv)[..., None].astype(np.float64) * np.abs(xc.astype(np.float64))
    ref = g.astype(np.float64)
    e = np.where(on[..., None], e, 0.0)
    return ref, np.where(on[..., None], e + half_ulp32(np.where(np.isfinite(ref), ref, 0.0), np.where(np.isfinite(e), e, 0.0)), 0.0)


# ---- forms -------------------------------------------------------------------------------------------------------------------------------
def _sums_forms(k, L, R, xs=None, ts=None):
    g = time_sums_grid(L)
    trips = (L + g * 256 - 1) // (g * 256)
    f = {f"{k}:second_trip" if trips > 1 else f"{k}:one_trip", f"{k}:grid_one" if g == 1 else f"{k}:grid_many"}
    if grid_x(L) > SLOTS:
        f.add(f"{k}:grid_capped")
    if L % 256:
        f.add(f"{k}:partial_last_workgroup")
    if L < 256:
        f.add(f"{k}:idle_waves")
    if xs is not None and (xs != L or ts != L):
        f.add(f"{k}:rows_strided")
    return f, g


def forms_slot_sum(rows, nslots, K):
    f = {"slot_sum<double>:nslots_below_64" if nslots < 64 else ("slot_sum<double>:nslots_64" if nslots == 64 else "slot_sum<double>:nslots_above_64"),
         f"slot_sum<double>:K{K}"}
    if (rows * K) % 4:
        f.add("slot_sum<double>:partial_last_workgroup")
    if slot_sum_grid(rows * K) > 1:
        f.add("slot_sum<double>:many_workgroups")
    return f


def forms_sisdr_sums(c):
    f, g = _sums_forms("sisdr_sums", c["L"], c["R"], c["L"] + c["xpad"], c["L"] + c["tpad"])
    return f | forms_slot_sum(c["R"], g, 5)


def forms_time_sums(c):
    if c["taps"] is None:
        return {"rfx_time_sums:no_taps"} | forms_sisdr_sums(c)
    L = c["L"]
    f, g = _sums_forms("time_sums", L, c["R"], L + c["xpad"], L + c["tpad"])
    f.add("time_sums:halo0_row_start")
    if L > 64:
        f.add("time_sums:halo0_memory")
    if L > 64:
        f.add("time_sums:halo63_memory")
    if L % 64 == 0:
        f.add("time_sums:halo63_row_end")
    else:
        f.add("time_sums:halo_from_lane_past_L")
    if L < 64 or (L % 256) and (L % 256) <= 192:
        f.add("time_sums:lane0_past_L")
    return f | forms_slot_sum(c["R"], g, 5)


def forms_rows(kind, zm, red, R, coef=True):
    f = {f"time_loss_rows:{kind}", f"time_loss_rows:{red}", "time_loss_rows:R_above_64" if R > 64 else "time_loss_rows:R_to_64"}
    if kind in ("sisdr", "sdsdr", "snr"):
        f.add(f"time_loss_rows:zero_mean_{int(bool(zm))}")
    if not coef:
        f.add("time_loss_rows:coef_null")
    return f


def forms_finish(zm, R):
    return {f"sisdr_finish:zero_mean_{int(bool(zm))}", "sisdr_finish:R_above_64" if R > 64 else "sisdr_finish:R_to_64"}


def forms_time_grad(c):
    R, L, taps = c["R"], c["L"], c["taps"] is not None
    k = f"time_loss_grad<{'taps' if taps else 'plain'}>"
    f = {f"row_gup:{c['red']}"}
    xs, ts = L + c["xpad"], L + c["tpad"]
    units = (L + 3) // 4
    g = time_stream_grid(units, R)
    f.add("time_loss_grad:grid_one" if g == 1 else "time_loss_grad:grid_many")                  # the host code, whatever the template
    if (units + 1023) // 1024 > 4096 // R:
        f.add("time_loss_grad:grid_capped")
    if 4096 // R == 0:
        f.add("time_loss_grad:cap_rounds_to_0")
    for r in range(min(R, 8)):
        ph = (c["og"] + r * L) % 4
        head0 = (4 - ph) % 4
        head = min(head0, L)
        nvec = (L - head) // 4
        tail = L - head - 4 * nvec
        f.add(f"{k}:head_{head}")
        if head0 > L:
            f.add(f"{k}:L_below_head")
        f.add(f"{k}:tail_{tail}")
        if nvec == 0:
            f.add(f"{k}:nvec_0")
            continue
        f.add(f"{k}:xvec_{int((c['ox'] + r * xs + head) % 4 == 0)}")
        f.add(f"{k}:tvec_{int((c['ot'] + r * ts + head) % 4 == 0)}")
        if nvec > g * 256:
            f.add(f"{k}:second_trip")
        if nvec % 256:
            f.add(f"{k}:partial_last_workgroup")
        if taps:
            f.add(f"{k}:low_halo_k0_row_start" if head == 0 else f"{k}:low_halo_k0_from_head")
            f.add(f"{k}:high_halo_last_group_row_end" if tail == 0 else f"{k}:high_halo_last_group_from_tail")
            if nvec > 64:
                f.update({f"{k}:low_halo_lane0_memory", f"{k}:high_halo_lane63_memory"})
            if nvec > 1:
                f.add(f"{k}:halo_from_shuffle")
    return f


def forms_logcosh(c):
    f, g = _sums_forms("logcosh_rows", c["L"], c["R"], c["L"] + c.get("xpad", 0), c["L"])
    f |= forms_slot_sum(c["R"], g, 1)
    gg = time_stream_grid(c["L"], c["R"])
    f.add("logcosh_grad:grid_one" if gg == 1 else "logcosh_grad:grid_many")
    if (c["L"] + 1023) // 1024 > 4096 // c["R"]:
        f.add("logcosh_grad:grid_capped")
    if c["L"] > gg * 256:
        f.add("logcosh_grad:second_trip")
    f.add(f"row_gup:{c['red']}")
    if c["scale"] != 1.0:
        f.add("logcosh:az_800")
    return f


def forms_scaled(c, fb):
    R, frames, bins = c["R"], c["frames"], c["bins"]
    k, kg = "stft_scaled_loss", "stft_scaled_loss_grad"
    g = scaled_grid(frames)
    f = {f"{k}:identity" if fb is None else f"{k}:banded", f"{k}:mx_stored" if c["store"] else f"{k}:mx_null",
         f"{k}:frames_wrap" if frames > g else f"{k}:one_frame_per_workgroup"}
    n_out = bins if fb is None else fb.shape[0]
    if bins > 256:
        f.add(f"{k}:bins_above_256")
    f.add(f"{k}:clamped_cell")
    if fb is not None:
        if n_out % 32:
            f.add(f"{k}:idle_filter_lanes")
        if n_out > 32:
            f.add(f"{k}:second_filter_trip")
        for ln in pack(fb)[0][:, 1]:
            f.add(f"{k}:len_0" if ln == 0 else (f"{k}:len_below_8" if ln < 8 else (f"{k}:len_multiple_of_8" if ln % 8 == 0 else f"{k}:len_not_multiple_of_8")))
    f |= forms_slot_sum(R, g, 4)
    if c["store"]:
        f |= {f"{kg}:identity" if fb is None else f"{kg}:banded", f"{kg}:per_example_{c['pe']}", f"{kg}:gup" if c["gup"] else f"{kg}:gup_null",
              f"{kg}:px_below_eps", f"{kg}:px_at_eps", f"{kg}:px_above_eps", f"{kg}:frames_wrap" if frames > scaled_grad_grid(frames) else f"{kg}:one_frame_per_workgroup"}
        if n_out > 256:
            f.add(f"{kg}:n_out_above_256")
        if bins > 256:
            f.add(f"{kg}:bins_above_256")
        if not c["pe"]:
            f.add(f"{kg}:batch_R_above_64" if R > 64 else f"{kg}:batch_R_to_64")
        if c["w"][0] == 0.0:
            f.add(f"{kg}:w_sc_0")
    return f


def forms_combine(c, w=None):
    k = "mrstft_combine" if w is None else "mrstft_combine_w"
    f = {f"{k}:nres_{c['nres']}", f"{k}:per_example_{c['pe']}", f"{k}:R_above_64" if c["R"] > 64 else f"{k}:R_to_64"}
    if w is not None:
        f |= {f"{k}:{n}_left_out" for n, v in zip(("w_sc", "w_lm", "w_lin"), w) if v == 0.0}
    return f


LDS_FORMS = {"stft_scaled_loss:lds_65536", "stft_scaled_loss_grad:dynamic_lds_attribute"}


def _all_forms():
    f = set(LDS_FORMS) | {"rfx_time_sums:no_taps", "logcosh:az_800"}
    for k in ("sisdr_sums", "time_sums", "logcosh_rows"):
        f |= {f"{k}:{n}" for n in ("one_trip", "second_trip", "grid_one", "grid_many", "grid_capped", "partial_last_workgroup", "idle_waves",
                                   "rows_strided")}
    f |= {f"time_sums:{n}" for n in ("halo0_row_start", "halo0_memory", "halo63_memory", "halo63_row_end", "halo_from_lane_past_L",
                                     "lane0_past_L")}
    f |= {f"slot_sum<double>:{n}" for n in ("nslots_below_64", "nslots_64", "nslots_above_64", "K1", "K4", "K5", "partial_last_workgroup",
                                            "many_workgroups")}
    f |= {f"time_loss_rows:{n}" for n in KINDS + REDUCTIONS + ("R_above_64", "R_to_64", "zero_mean_0", "zero_mean_1", "coef_null")}
    f |= {f"sisdr_finish:{n}" for n in ("zero_mean_0", "zero_mean_1", "R_above_64", "R_to_64")}
    f |= {f"row_gup:{n}" for n in REDUCTIONS}
    for k in ("time_loss_grad<taps>", "time_loss_grad<plain>"):
        f |= {f"{k}:{n}" for n in ("L_below_head", "nvec_0", "xvec_0", "xvec_1", "tvec_0", "tvec_1", "second_trip", "partial_last_workgroup")}
        f |= {f"{k}:head_{j}" for j in range(4)} | {f"{k}:tail_{j}" for j in range(4)}
    f |= {f"time_loss_grad<taps>:{n}" for n in ("low_halo_k0_row_start", "low_halo_k0_from_head", "high_halo_last_group_row_end",
                                                "high_halo_last_group_from_tail", "low_halo_lane0_memory", "high_halo_lane63_memory",
                                                "halo_from_shuffle")}
    f |= {f"logcosh_grad:{n}" for n in ("grid_one", "grid_many", "grid_capped", "second_trip")}
    f |= {f"time_loss_grad:{n}" for n in ("grid_one", "grid_many", "grid_capped", "cap_rounds_to_0")}
    k, kg = "stft_scaled_loss", "stft_scaled_loss_grad"
    f |= {f"{k}:{n}" for n in ("identity", "banded", "mx_stored", "mx_null", "frames_wrap", "one_frame_per_workgroup", "bins_above_256",
                               "clamped_cell", "idle_filter_lanes", "second_filter_trip", "len_0", "len_below_8", "len_multiple_of_8",
                               "len_not_multiple_of_8")}
    f |= {f"{kg}:{n}" for n in ("identity", "banded", "per_example_0", "per_example_1", "gup", "gup_null", "px_below_eps", "px_at_eps",
                                "px_above_eps", "frames_wrap", "one_frame_per_workgroup", "n_out_above_256", "bins_above_256",
                                "batch_R_above_64", "batch_R_to_64", "w_sc_0")}
    for k in ("mrstft_combine", "mrstft_combine_w"):
        f |= {f"{k}:{n}" for n in ("nres_1", "nres_3", "nres_8", "per_example_0", "per_example_1", "R_above_64", "R_to_64")}
    f |= {f"mrstft_combine_w:{n}_left_out" for n in ("w_sc", "w_lm", "w_lin")}
    return sorted(f)


ALL_FORMS = _all_forms()
UNREACHED = {}
SLOT_SUM_CASES = {                                       # the first case that hits each form of rfx_slot_sum_kernel<double>
    "slot_sum<double>:K1": "logcosh R3-L5",
    "slot_sum<double>:K4": "scaled R1-f1-b9-id-pe1-w1.0_1.0_0.0",
    "slot_sum<double>:K5": "time R3-L1-tn-snr-sum",
    "slot_sum<double>:many_workgroups": "time R3-L1-tn-snr-sum",
    "slot_sum<double>:nslots_64": "time R3-L131072-tn-dc-mean",
    "slot_sum<double>:nslots_above_64": "time R1-L262147-t0-sisdr-mean",
    "slot_sum<double>:nslots_below_64": "time R3-L1-tn-snr-sum",
    "slot_sum<double>:partial_last_workgroup": "time R3-L1-tn-snr-sum",
}

# elements whose reference bound is not small against the reference (bound / |ref| >= 1e-3), by name: (signal of the row, kind, output).
# x == t makes the first four exactly 0 (SNR: a + b = 0 and c = 0) while the bound of the fp64 evaluation is not; at 120 dB a few
# samples of x and t are the same float, and ESR's gradient a (x - t) is exactly 0 there.
ILL_CONDITIONED = {("same", "esr", "rows"), ("same", "dc", "rows"), ("same", "snr", "coef_c"), ("same", "snr", "gx"), ("db120", "esr", "gx")}
