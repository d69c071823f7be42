"""Both instantiations of both kernels of remfx_amd/csrc/segment.hip through the C ABI -- rfx_segment_split, rfx_segment_merge,
rfx_segment_split_c, rfx_segment_merge_c -- on guarded buffers, against tests/segment_ref.py (numpy float64), per element:

    split   bit for bit (a copy and a +0 fill)
    merge   |got - ref| <= (cover(t) + 2) x 2^-24 x sum_i w_i |y_i| / sum_i w_i      (segment_ref.merge_bound)

The case table (segment_ref.CASES) is built around the kernels' unit of work, a 256-sample chunk of one row, not around file lengths:
tests/test_gpu_segment.py stays the wrapper-level test at real lengths.  Clip i of every row is scaled by 1, 1e3, 1e-3 in turn, so a
neighbouring clip's sample, a weight off by one or a clip counted twice is outside the bound where the loud clip has faded out.  Every
VEC case runs again with its input and with its output one sample past a 16-byte boundary: the dword kernel, the same bits.  Outputs are
NaN-filled between NaN guards and have to come back written everywhere and nowhere else, inputs bit for bit, every case twice with the
same bits.  tests/test_segment_cpu.py holds the bound's check against an fp32 restatement and the walk of the table over the forms."""
import numpy as np
import pytest
import torch

from tests import segment_ref as R
from tests.kernel_harness import Guarded, api, judge, report, same_bits, stop_after_a_device_error, twice  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]


def _id(c):
    return "B{}-C{}-T{}-L{}-ov{}-lead{}-trail{}".format(*c)


def _split_call(grouped, B, C, T, L, hop, S, X, O):
    lib, _, stream = api()
    if grouped:
        return lib.rfx_segment_split_c(X.ptr() if X else None, O.ptr() if O else None, B, C, T, L, hop, S, stream())
    return lib.rfx_segment_split(X.ptr() if X else None, O.ptr() if O else None, B * C, T, L, hop, S, stream())


def _merge_call(grouped, B, C, T, L, hop, lead, trail, S, Y, O):
    lib, _, stream = api()
    if grouped:
        return lib.rfx_segment_merge_c(Y.ptr() if Y else None, O.ptr() if O else None, B, C, T, L, hop, lead, trail, S, stream())
    return lib.rfx_segment_merge(Y.ptr() if Y else None, O.ptr() if O else None, B * C, T, L, hop, lead, trail, S, stream())


def _run_split(case, grouped, x, in_off=0, out_off=0):
    B, C, T, L, overlap, _, _ = case
    hop, S, _, _, _ = R.plan(T, L, overlap)

    def run():
        X = Guarded.of(x, "x", off=in_off)
        O = Guarded(B * C * S * L, what="clips", off=out_off)
        rc = _split_call(grouped, B, C, T, L, hop, S, X, O)
        torch.cuda.synchronize()
        assert rc == 0, ("split", rc, case, grouped)
        X.unchanged()
        O.owned()
        return {"clips": O.cpu()}
    return twice(run)[0]["clips"]


def _run_merge(case, grouped, y, in_off=0, out_off=0):
    B, C, T, L, overlap, lead, trail = case
    hop, S, _, _, To = R.plan(T, L, overlap, lead, trail)

    def run():
        Y = Guarded.of(y, "clips", off=in_off)
        O = Guarded(B * C * To, what="out", off=out_off)
        rc = _merge_call(grouped, B, C, T, L, hop, lead, trail, S, Y, O)
        torch.cuda.synchronize()
        assert rc == 0, ("merge", rc, case, grouped)
        Y.unchanged()
        O.owned()
        return {"out": O.cpu()}
    return twice(run)[0]["out"]


def _layouts(C):
    """the plain entry takes every row as a clip of its own; the _c entry (C > 1) keeps a clip's channels together"""
    return (False, True) if C > 1 else (False,)


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_split(case):
    B, C, T, L, overlap, _, _ = case
    _, S, _, _, _ = R.plan(T, L, overlap)
    x = R.split_input(B, C, T)
    want = R.split(x, L, overlap)                              # [row][segment]
    form = R.forms("split", T, L, overlap)
    ratios = []
    for grouped in _layouts(C):
        ref = R.group(want, B, S, C) if grouped else want
        entry = "rfx_segment_split_c" if grouped else "rfx_segment_split"
        info = (entry, case, form, sorted(R.steering("split", T, L, overlap)))
        got = _run_split(case, grouped, x)
        ratios.append((entry, judge(got, ref, 0, ctx=info)))
        if form == "vec":
            for offs in ((1, 0), (0, 1)):
                assert R.forms("split", T, L, overlap, in_off=offs[0], out_off=offs[1]) == "dword"
                same_bits({"clips": got}, {"clips": _run_split(case, grouped, x, *offs)}, (*info, "base offsets", offs))
    report("SEGMENT", f"split {_id(case)} {form}", ratios)


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_merge(case):
    B, C, T, L, overlap, lead, trail = case
    _, S, _, _, _ = R.plan(T, L, overlap, lead, trail)
    y = R.merge_input(B, C, T, L, overlap, lead, trail)        # [row][segment]
    ref = R.merge(y, T, L, overlap, lead, trail)
    bound = R.merge_bound(y, T, L, overlap, lead, trail)
    form = R.forms("merge", T, L, overlap, lead, trail)
    ratios = []
    for grouped in _layouts(C):
        clips = R.group(y, B, S, C) if grouped else y
        entry = "rfx_segment_merge_c" if grouped else "rfx_segment_merge"
        info = (entry, case, form, sorted(R.steering("merge", T, L, overlap, lead, trail)))
        got = _run_merge(case, grouped, clips)
        ratios.append((entry, judge(got, ref, bound, ctx=info)))
        if form == "vec":
            for offs in ((1, 0), (0, 1)):
                assert R.forms("merge", T, L, overlap, lead, trail, in_off=offs[0], out_off=offs[1]) == "dword"
                same_bits({"out": got}, {"out": _run_merge(case, grouped, clips, *offs)}, (*info, "base offsets", offs))
    report("SEGMENT", f"merge {_id(case)} {form}", ratios)


def test_merge_inverts_split_per_element():
    """the two kernels back to back on the grouped layout: the file again, inside the bound of a merge of its own clips"""
    case = (2, 3, 1284, 512, 128, 0, 0)
    B, C, T, L, overlap, _, _ = case
    x = R.split_input(B, C, T)
    clips = _run_split(case, True, x).numpy().reshape(-1, L)
    back = _run_merge(case, True, clips)
    rows = R.ungroup(clips, B, R.plan(T, L, overlap)[1], C)
    report("SEGMENT", "merge(split(x))", [judge(back, x.astype(np.float64), R.merge_bound(rows, T, L, overlap), ctx=("merge of split", case))])


def test_refusals_write_nothing():
    """S one too small and one too large, hop = 0, hop > L, lead + trail > overlap, To < 1, no rows / channels, a NULL pointer: nonzero,
    and the output keeps its fill.  (rows % C != 0 cannot be said through the ABI: the _c entries pass B * C rows.)"""
    B, C, T, L, overlap, lead, trail = 2, 2, 1284, 512, 128, 8, 12
    hop, S, _, Lp, To = R.plan(T, L, overlap, lead, trail)
    x = R.split_input(B, C, T)
    y = np.ones((B * C * (S + 1), L), np.float32)              # room for every S that is tried, were it accepted
    for grouped in (False, True):
        X, Y = Guarded.of(x, "x"), Guarded.of(y, "clips")
        O = Guarded(B * C * (S + 1) * L, what="out")
        bad_split = [(B, C, T, L, hop, S - 1), (B, C, T, L, hop, S + 1), (B, C, T, L, 0, S), (B, C, T, L, L + 1, S), (B, C, T, L, hop, 0),
                     (0, C, T, L, hop, S), (B, C, 0, L, hop, 1), (B, C, T, 0, hop, S)] + ([(B, 0, T, L, hop, S)] if grouped else [])
        for a in bad_split:
            assert _split_call(grouped, *a, X, O) != 0, ("split", grouped, a)
        assert _split_call(grouped, B, C, T, L, hop, S, None, O) != 0 and _split_call(grouped, B, C, T, L, hop, S, X, None) != 0
        bad_merge = [(B, C, T, L, hop, lead, trail, S - 1), (B, C, T, L, hop, lead, trail, S + 1), (B, C, T, L, 0, lead, trail, S),
                     (B, C, T, L, L + 1, lead, trail, S), (B, C, T, L, hop, overlap, 1, S), (B, C, T, L, hop, overlap + 1, 0, S),
                     (B, C, T, L, hop, -1, 0, S), (B, C, T, L, hop, 0, -1, S), (B, C, 10, 64, 48, 10, 0, 1), (B, C, 12, 64, 48, 8, 4, 1),
                     (0, C, T, L, hop, lead, trail, S)] + ([(B, 0, T, L, hop, lead, trail, S)] if grouped else [])
        for a in bad_merge:
            assert _merge_call(grouped, *a, Y, O) != 0, ("merge", grouped, a)
        assert _merge_call(grouped, B, C, T, L, hop, lead, trail, S, None, O) != 0
        assert _merge_call(grouped, B, C, T, L, hop, lead, trail, S, Y, None) != 0
        torch.cuda.synchronize()
        O.untouched()
        X.unchanged()
        Y.unchanged()
    for args in ((T, L, overlap, overlap, 1), (T, L, overlap, overlap + 1, 0), (10, 64, 16, 10, 0), (12, 64, 16, 8, 4)):
        assert R.forms("merge", *args) is None
    report("SEGMENT", "refusals", [])
