"""ops.launch / ops.launch_rc / ops.query, the one way the package calls into libremfx_hip, against a fake library behind `_lib.lib`
and a patched `ops.raw_stream` (the two seams a test may replace).  CPU only: nothing is loaded, nothing is launched."""
import contextlib
import ctypes as C
import gc
import weakref

import numpy as np
import pytest
import torch

from remfx_amd import _lib, ops

STREAM = 0x5EA7


class _Fake:
    """a library whose every entry point records its arguments and returns `rc`"""

    def __init__(self, rc=0, on_call=None):
        self.rc, self.on_call, self.calls = rc, on_call, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.on_call is not None:
                self.on_call(*args)
            return self.rc
        return entry


@contextlib.contextmanager
def seams(fake, stream=STREAM):
    saved = (_lib.lib, ops.raw_stream)
    _lib.lib, ops.raw_stream = (lambda: fake), (lambda: stream)
    try:
        yield fake
    finally:
        _lib.lib, ops.raw_stream = saved


def test_argument_rule_and_stream_last():
    t = torch.arange(6, dtype=torch.float32)
    p = torch.nn.Parameter(torch.ones(3))
    a = np.arange(4, dtype=np.float64)
    d = _lib.StftDesc()
    ref = C.byref(d)
    c64 = C.c_int64(7)
    with seams(_Fake()) as fake:
        assert ops.launch("rfx_x", t, p, None, a, ref, 3, 2.5, c64, True) is None
    (name, args), = fake.calls
    assert name == "rfx_x" and len(args) == 10
    assert args[0] == t.data_ptr() and type(args[0]) is int          # tensor: its address
    assert args[1] == p.data_ptr() and type(args[1]) is int          # nn.Parameter: a tensor
    assert args[2] is None                                           # None: the null pointer of a `void *` parameter
    assert args[3] == a.ctypes.data and type(args[3]) is int         # numpy array: its host address
    assert args[4] is ref and args[4]._obj is d                      # byref(desc) unchanged: proxies read desc._obj
    assert args[5] == 3 and type(args[5]) is int and args[6] == 2.5 and type(args[6]) is float
    assert args[7] is c64 and args[8] is True                        # ctypes values and other scalars unchanged
    assert args[9] == STREAM                                         # the stream is last and is ops.raw_stream()


def test_none_is_the_null_pointer_for_ctypes():
    assert C.c_void_p.from_param(None) is None and C.c_void_p(None).value is None


def test_stream_is_looked_up_per_call():
    fake = _Fake()
    with seams(fake, 11):
        ops.launch("rfx_a", 1)
        ops.raw_stream = lambda: 22                                  # replaced after the first call: honoured by the next
        ops.launch_rc("rfx_b", 2)
        ops.query("rfx_c", 3)
    assert [c[1] for c in fake.calls] == [(1, 11), (2, 22), (3,)]    # query: host only, no stream


def test_nonzero_code_raises_and_names_the_symbol():
    with seams(_Fake(rc=7)):
        with pytest.raises(RuntimeError, match=r"rfx_some_entry failed with code 7"):
            ops.launch("rfx_some_entry", 1)
    with seams(_Fake(rc=-1)):
        with pytest.raises(RuntimeError, match=r"rfx_other failed with code -1"):
            ops.launch("rfx_other")


def test_launch_rc_returns_the_code_unchecked():
    with seams(_Fake(rc=-1)) as fake:
        assert ops.launch_rc("rfx_gemm_wgrad", 5) == -1
    with seams(_Fake(rc=0)):
        assert ops.launch_rc("rfx_gemm_wgrad", 5) == 0
    assert fake.calls == [("rfx_gemm_wgrad", (5, STREAM))]


def test_query_returns_an_int():
    class _Odd(_Fake):
        def __getattr__(self, name):
            return lambda *a: np.int64(40 + len(a))
    with seams(_Odd()):
        v = ops.query("rfx_x_ws", 1, 2)
    assert v == 42 and type(v) is int
    t = torch.zeros(2)
    with seams(_Fake(rc=True)) as fake:
        v = ops.query("rfx_x_ok", t, None)
    assert v == 1 and type(v) is int and fake.calls == [("rfx_x_ok", (t.data_ptr(), None))]


def test_library_replaced_after_import_is_honoured():
    first, second = _Fake(), _Fake()
    with seams(first):
        ops.launch("rfx_a")
        _lib.lib = lambda: second                                    # a later replacement of the seam, and of a symbol on the object
        ops.launch("rfx_b")
        second.rfx_c = lambda *a: 9
        assert ops.launch_rc("rfx_c") == 9
    assert [c[0] for c in first.calls] == ["rfx_a"] and [c[0] for c in second.calls] == ["rfx_b"]


def test_temporary_is_alive_inside_the_entry_point():
    base = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()
    assert not base.is_contiguous()
    seen = {}

    def on_call(ptr, n, stream):
        gc.collect()
        t = seen["ref"]()
        seen["alive"] = t is not None and t.data_ptr() == ptr
        seen["values"] = t.clone() if t is not None else None

    def call():
        tmp = base.contiguous()
        seen["ref"] = weakref.ref(tmp)
        return tmp

    with seams(_Fake(on_call=on_call)):
        ops.launch("rfx_x", call(), 12)
    assert seen["alive"] and torch.equal(seen["values"], base.contiguous())
    gc.collect()
    assert seen["ref"]() is None                                     # and released once the call has returned


def test_scratch_asks_the_library_and_allocates_what_it_answers():
    """ops.scratch: the named `_ws` query is called with the geometry it was given (tensors and descriptors by the argument rule, no
    stream), and the buffer has exactly the answered number of elements of the stated type"""
    d = _lib.StftDesc()
    ref = C.byref(d)
    for n, dtype in ((37, torch.float64), (0, torch.float32), (5, torch.float32)):
        with seams(_Fake(rc=n)) as fake:
            buf = ops.scratch("rfx_x_ws", 3, 7, ref, device="cpu", dtype=dtype)
        assert fake.calls == [("rfx_x_ws", (3, 7, ref))]
        assert buf.shape == (n,) and buf.dtype == dtype and buf.device.type == "cpu"
    with seams(_Fake(rc=12)) as fake:
        assert ops.scratch_size("rfx_x_ws_partial", ref) == 12
    assert fake.calls == [("rfx_x_ws_partial", (ref,))]


def test_scratch_raises_where_the_launcher_would_refuse():
    for rc in (-1, -5):
        with seams(_Fake(rc=rc)):
            with pytest.raises(RuntimeError, match=r"rfx_x_ws\(4, -2\) = -"):
                ops.scratch("rfx_x_ws", 4, -2, device="cpu", dtype=torch.float32)
            with pytest.raises(RuntimeError, match="rfx_x_ws"):
                ops.scratch_size("rfx_x_ws", 4, -2)
