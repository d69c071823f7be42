"""What the *_ref.py modules share: the number formats' arithmetic (bf16 rounding, ulp, the value a C float carries), GELU's two
functions and the worst-element figure.  Pure CPU.  What is family-specific (k_of, MARGIN, FLOOR*, tolerance, floors*, Case) shares
names between the references, not meaning, and stays with its family."""
import math

import torch

EPS32 = 2.0 ** -23


def f32(v):
    """the value a C float argument carries, as a Python double"""
    return float(torch.tensor(v, dtype=torch.float32))


def bf16_rne(x):
    """nearest bf16, ties to even, of the fp32 value of x, in the dtype of x"""
    u = x.to(torch.float32).contiguous().view(torch.int32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & -65536).view(torch.float32).to(x.dtype)


def bf16_trunc(x):
    u = x.to(torch.float32).contiguous().view(torch.int32)
    return (u & -65536).view(torch.float32).to(x.dtype)


def ulp(v, mant, tiny=2.0 ** -126):
    """spacing of a format with `mant` explicit mantissa bits at |v| (fp64 tensor); |v| below `tiny` counts as `tiny`"""
    e = torch.floor(torch.log2(v.abs().clamp_min(tiny)))
    return torch.exp2(e - mant)


def ulp16(v):
    return ulp(v, 7)


def gelu_cdf(u):
    return 0.5 * (1.0 + torch.erf(u * (0.5 ** 0.5)))


def gelu_pdf(u):
    return torch.exp(-0.5 * u * u) * (1.0 / math.sqrt(2.0 * math.pi))


def worst(got, ref, tol):
    """(error / tolerance, flat index) of the worst element; NaN / inf count as infinitely wrong"""
    e = (got.double() - ref).abs()
    q = torch.where(torch.isfinite(e), e / tol.clamp_min(1e-300), torch.full_like(e, float("inf")))
    q = torch.where((e == 0) & (tol == 0), torch.zeros_like(q), q)
    i = int(q.reshape(-1).argmax()) if q.numel() else 0
    return (float(q.reshape(-1)[i]) if q.numel() else 0.0), i
