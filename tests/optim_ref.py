"""fp64 restatement of remfx_amd/csrc/optim.hip: rfx_sumsq, rfx_clip_coef, rfx_adamw_step (torch.optim.AdamW semantics: decoupled decay
first, step_size = lr / bc1, denom = sqrt(v) / sqrt(bc2) + eps).  Hyper-parameters are Python doubles; the GPU test passes the doubles
that equal the fp32 values the C ABI carries (f32()), so that what is judged is the kernel's arithmetic and not the caller's rounding of
0.999 to a float.

Bounds, eps32 = 2^-23, one half-ulp = eps32 / 2 relative:
  m', v'   2 half-ulps of |b1 m| + |(1 - b1) g| (v' likewise): one rounded product and the fused sum, fma(b1, m, (1 - b1) g) and
           fma((1 - b2) g, g, b2 v) -- 0.5 |t| + 0.5 |result| <= the sum of the terms; 1 - b is exact in fp32 for b in [0.5, 1].  (With
           every product rounded, v' = b2 v + ((1 - b2) g) g carries three half-ulps on its g^2 term: the kernel of before this test
           missed the bound by up to 1.31 x at a few of 4 M elements.)  A gradient scale adds the rounding of g * gscale: half an ulp of
           the g term of m', a whole one of the g^2 term of v'.
  p'       2 half-ulps of |p|  +  K eps32 |update|  +  the bound of m' carried through step_size / denom
           (p' = fma(p, decay, -update): decay = fl(1 - lr wd) is within a quarter of an eps32 of its value, the fused sum adds a half),
           K = FP32_HALF_ULPS / 2 + E(b1) + E(b2) / 2,  E(b) = b^step / (1 - b^step):
           the update is step_size m' / denom, with lr / bc1, 1 / sqrtf(bc2), sqrtf(v'), the product, + eps, step m' and the quotient at
           half an ulp to one ulp each (16 half-ulps in all, the allowance of DESIGN.md 4.15 for device sqrtf / division), and
           bc = 1 - powf(b, step): powf is documented at 1 ulp, i.e. eps32 b^step absolute, E(b) eps32 relative to bc.  At step = 1,
           b2 = 0.999f: E = 998, the fp32 bias correction of the second moment is good to 6e-5 relative -- from the float value of the
           beta, not from what the kernel returned.
  sumsq    fp64 accumulation of exactly representable products of two floats: every addition rounds once in fp64.  A thread adds
           ceil(n / (4 stride)) groups of 4 products and a tail value (<= T = 4 ceil(n4 / threads) + 1 additions), then 6 butterfly
           steps, 2 workgroup steps, and the slot sum ceil(slots / 64) + 6: |err| <= (T + 14 + ceil(slots / 64)) 2^-53 sum g^2; the
           test uses 4 x that count."""
import math

from tests.ref_common import EPS32, f32  # noqa: F401

FP32_HALF_ULPS = 16
SLOTS = 4096                      # SUMSQ_MAX_SLOTS of optim.hip
HYPER = dict(betas=(0.95, 0.999), eps=1e-6, wd=1e-3)
SUMSQ_N = (0, 1, 3, 4, 5, 1023, 1025, 4_194_304 + 1027)
ADAMW_N = (1, 5, 1025, 4_194_304 + 1027)


def gridn(n):
    """workgroups of 256 threads: one per 1024 values, at most 4096"""
    return min(max(-(-n // 1024), 1), 4096)


def forms(n):
    """what steers sumsq_kernel / adamw_kernel at n values"""
    g = gridn(n) if n > 0 else 0
    th = g * 256
    return {"workgroups": g, "capped": n > 4096 * 1024, "adamw_iters": -(-n // th) if g else 0, "vec_iters": -(-(n // 4) // th) if g else 0,
            "tail": n % 4, "slots": g}


def sumsq(g):
    return float((g.double() ** 2).sum())


def sumsq_bound(n, total):
    f = forms(n)
    adds = 4 * f["vec_iters"] + 1 + 14 + -(-max(f["slots"], 1) // 64)
    return 4 * 2.0 ** -53 * adds * total


def clip_coef(total, max_norm, pre):
    """(coef, norm): min(1, max_norm / (norm pre + 1e-6)) pre; pre alone when max_norm == 0"""
    norm = math.sqrt(total) * pre
    if max_norm > 0:
        return min(1.0, max_norm / (norm + 1e-6)) * pre, norm
    return pre, norm


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """one step in fp64 -> (p', m', v')"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * gscale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_k(b1, b2, step):
    e = lambda b: b ** step / (1 - b ** step)                   # noqa: E731
    return FP32_HALF_ULPS / 2 + e(b1) + 0.5 * e(b2)


def adamw_bounds(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
    """per-element absolute bounds {p, m, v} of one step from fp32 state (p, g, m, v)"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gs = g * gscale
    mm = (b1 * m).abs() + ((1 - b1) * gs).abs()
    mv = (b2 * v).abs() + (1 - b2) * gs * gs
    if gscale != 1.0:                                           # g * gscale is one more rounding of g
        mm = mm + 0.5 * ((1 - b1) * gs).abs()
        mv = mv + (1 - b2) * gs * gs
    pn, mn, vn = adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, gscale)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = vn.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * mn / denom
    bm, bv = EPS32 * mm, EPS32 * mv
    bp = EPS32 * p.abs() + adamw_k(b1, b2, step) * EPS32 * upd.abs() + (lr / bc1) * bm / denom
    return {"p": bp, "m": bm, "v": bv}
