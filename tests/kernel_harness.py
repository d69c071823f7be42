"""What every tests/test_gpu_*_kernel.py module shares: the guarded buffer its kernels write into, the per-element verdict,
the printed figure and the rule that nothing more is launched on a device that reported an error.  Not a conftest: a module imports
what it uses, `stop_after_a_device_error` included (an autouse fixture acts in every module that imports it).

Guards and fills are compared as bit patterns against the fill the buffer recorded when it was made, never with isnan: a kernel that
stores another NaN out of bounds is caught.  `Guarded` and `judge` take device="cpu" / CPU arrays, which is how
tests/test_kernel_harness_cpu.py exercises them."""
import ctypes as C

import numpy as np
import pytest
import torch

GUARD = 4096                                                   # elements of the fill on each side of every payload
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32}


def bits(t):
    """the integer view of a tensor's storage (1 / 2 / 4 / 8-byte elements)"""
    return t.contiguous().view(_INT[t.element_size()])


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


class Guarded:
    """n elements of `dtype`, `off` elements into the space between two guards of GUARD elements (front=False: no guard in front; off = 0:
    aligned to 8 KiB at least).  The whole allocation is one NaN (int32 payloads: the float NaN's bits); `fill` then sets the payload
    where a kernel accumulates into it, `init` copies an input into it."""

    def __init__(self, n, dtype=torch.float32, what="", init=None, off=0, front=True, fill=None, device="cuda"):
        self.what, self.n, self.lo = what, n, (GUARD if front else 0) + off
        ftype = {torch.int32: torch.float32}.get(dtype, dtype)
        self.buf = torch.full((self.lo + n + GUARD,), float("nan"), device=device, dtype=ftype)
        self.fill = bits(self.buf[:1]).clone()
        self.t = self.buf[self.lo:self.lo + n]
        if dtype != ftype:
            self.t = self.t.view(dtype)
        if fill is not None:
            self.t.fill_(fill)
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))
        self.before = self.buf.clone() if init is not None or fill is not None else None

    @classmethod
    def of(cls, arr, what, off=0, device="cuda"):
        """a numpy input between guards"""
        arr = np.ascontiguousarray(arr)
        return cls(arr.size, _TORCH[arr.dtype], what, torch.from_numpy(arr), off, device=device)

    def ptr(self, elements=0):
        return C.c_void_p(self.t.data_ptr() + elements * self.t.element_size())

    def guards_intact(self):
        b = bits(self.buf)
        assert bool((b[:self.lo] == self.fill).all()) and bool((b[self.lo + self.n:] == self.fill).all()), f"{self.what}: guard overwritten"

    def owned(self):
        """every element written with a finite value, nothing outside touched"""
        self.guards_intact()
        bad = ~torch.isfinite(self.t)
        assert not bool(bad.any()), f"{self.what}: element {int(bad.nonzero()[0])} of {self.n} not written or not finite"

    def untouched(self):
        assert bool((bits(self.buf) == self.fill).all()), f"{self.what}: written by a call that had to leave it alone"

    def unchanged(self):
        """bit for bit what it was after `init` / `fill`"""
        if self.before is None:
            return self.untouched()
        assert torch.equal(bits(self.buf), bits(self.before)), f"{self.what} was written"

    def still_fill(self, got, where):
        """the elements `where` (bool, cpu) of the fetched payload must still hold the fill"""
        bad = where & (bits(got) != self.fill.cpu())
        assert not bool(bad.any()), f"{self.what}: element {int(bad.nonzero()[0])} is outside the result and was written"

    def cpu(self):
        self.guards_intact()
        return self.t.cpu()

    def np(self, shape=None):
        a = self.cpu().numpy()
        return a.reshape(shape) if shape else a


class Arena:
    """the `alloc(shape, dtype, fill=None)` the launch helpers of gemm_ref / clast_ref take: every buffer a Guarded"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def alloc(self, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.bufs.append(Guarded(n, dtype, f"buffer {len(self.bufs)} {tuple(shape)}", fill=fill, device=self.dev))
        return self.bufs[-1].t.view(shape)

    def check(self):
        for b in self.bufs:
            b.guards_intact()

    def intact(self):
        try:
            self.check()
        except AssertionError:
            return False
        return True


def where(i, shape):
    """flat index -> coordinates"""
    out = []
    for d in reversed(shape):
        out.append(i % d)
        i //= d
    return tuple(reversed(out))


def judge(got, ref, bound, *, exact="bits", equal_inf=False, ctx=()):
    """The verdict on one output (torch tensors or numpy arrays of any float type, compared in fp64), per element:
        bound > 0   |got - ref| <= bound
        bound == 0  got is ref rounded once to got's type: bit for bit (exact="bits"), or by value, -0 == +0 (exact="value")
    got has to be finite (equal_inf: or the infinity the reference has there); every bound finite and non-negative -- an infinite or
    NaN bound would pass any value; got, ref and bound of one element count (a Python number as bound stands for every element).
    -> the largest error / bound"""
    assert exact in ("bits", "value"), exact
    g, r = _tensor(got).detach().cpu().reshape(-1), _tensor(ref).double().cpu().reshape(-1)
    n = g.numel()
    b = torch.full((n,), float(bound), dtype=torch.float64) if isinstance(bound, (int, float)) else _tensor(bound).double().cpu().reshape(-1)
    assert r.numel() == n and b.numel() == n, (*ctx, "element counts of got, ref, bound", n, r.numel(), b.numel())
    bad = ~(torch.isfinite(b) & (b >= 0))
    assert not bool(bad.any()), (*ctx, "bound of element", int(bad.nonzero()[0]), "is", float(b[bad][0]), ": not finite and non-negative")
    if n == 0:
        return 0.0
    g64 = g.double()
    bad, err = ~torch.isfinite(g64), (g64 - r).abs()
    if equal_inf:
        same_inf = torch.isinf(r) & (g64 == r)
        bad, err = bad & ~same_inf, err.masked_fill(same_inf, 0.0)
    assert not bool(bad.any()), (*ctx, "element", int(bad.nonzero()[0]), "of", n, "not written / not finite", int(bad.sum()), "such")
    q, zero = err / b, b == 0
    if bool(zero.any()):
        once = r.to(g.dtype)
        differs = (bits(g) != bits(once)) if exact == "bits" else (g != once)
        q = torch.where(zero, torch.where(differs, float("inf"), 0.0), q)
    j = int(q.argmax())
    if not float(q[j]) <= 1.0:
        raise AssertionError((*ctx, "element", j, "of", n, "got", float(g[j]), "ref", float(r[j]), "bound", float(b[j]), "error / bound",
                              float(q[j]), "elements over", int((~(q <= 1.0)).sum())))
    return float(q[j])


def same_bits(a, b, what=""):
    """two runs' outputs {name: tensor or array}: the same bits"""
    for k in a:
        assert torch.equal(bits(_tensor(a[k])), bits(_tensor(b[k]))), (what, k, "second run differs")


_same_bits = same_bits                                         # twice() has an argument of that name


def twice(run, same_bits=True):
    """run() into fresh buffers, twice -> both results"""
    a, b = run(), run()
    if same_bits:
        _same_bits(a, b)
    return a, b


def report(family, entry, ratios, label=""):
    """the line a run's log is compared by.  ratios: {name: figure}, or figures / (name, figure) pairs of which the largest per name is
    printed; none: the call was refused"""
    pairs = ratios.items() if isinstance(ratios, dict) else [r if isinstance(r, tuple) else ("", r) for r in ratios]
    best = {}
    for k, v in pairs:
        best[k] = max(best.get(k, 0.0), v)
    head = f"\n{family} {entry}{' ' + label if label else ''}: "
    print(head + ("largest error / bound " + ", ".join(f"{k} {v:.3f}".strip() for k, v in best.items()) if best else "refused"))


def api():
    """(the library, tensor -> pointer argument, () -> the current stream argument)"""
    from remfx_amd import _lib
    from remfx_amd.ops import _ptr, _stream
    return _lib.lib(), _ptr, _stream


def sync(rc, entry, info):
    torch.cuda.synchronize()
    assert rc == 0, (entry, "returned", rc, *info)


def host(a):
    """a numpy array as a host pointer argument"""
    return a.ctypes.data_as(C.c_void_p)


def guarded(fn, what):
    """run a launch sequence; a launch error or a device fault ends the session: nothing more is started on this device"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


@pytest.fixture(autouse=True)
def stop_after_a_device_error():
    """nothing more is launched on a device that reported an error: the session ends with the test that met it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further launches: {e}", returncode=3)
