"""tests/kernel_harness.py and tests/ref_common.py carry the GPU tests of every kernel family: what they must catch, on the CPU."""
import pytest
import torch

from tests import ref_common as RC
from tests.kernel_harness import GUARD, Guarded, bits, judge, report, where

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.int32]
_ID = dict(ids=lambda d: str(d).split(".")[-1])
OTHER_NAN = {4: 0x7FC00001, 8: 0x7FF8000000000001, 2: 0x7FC1}     # quiet NaNs that are not torch's: isnan is true of them


def _fails(check):
    with pytest.raises(AssertionError):
        check()


def _written(n, dtype, **kw):
    """a buffer whose payload a kernel has written in full"""
    b = Guarded(n, dtype, "buf", device="cpu", **kw)
    b.t.copy_(torch.arange(1, n + 1).to(dtype))
    return b


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
@pytest.mark.parametrize("off", (0, 3))
def test_a_finite_store_next_to_the_payload_is_seen(dtype, off):
    n = 24
    _written(n, dtype, off=off).owned()
    for at in (GUARD + off - 1, GUARD + off + n):
        b = _written(n, dtype, off=off)
        b.buf[at] = 1.0
        _fails(b.guards_intact)
        _fails(b.owned)
        _fails(b.cpu)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
def test_another_nan_in_a_guard_is_seen(dtype):
    for at in (0, GUARD - 1, GUARD + 8, 2 * GUARD + 7):
        b = _written(8, dtype)
        bits(b.buf)[at] = OTHER_NAN[b.buf.element_size()]
        assert bool(torch.isnan(b.buf[at])), "the planted value is a NaN: an isnan guard check accepts it"
        _fails(b.guards_intact)


@pytest.mark.parametrize("dtype", DTYPES[:3], **_ID)
def test_an_unwritten_payload_element_is_seen(dtype):
    b = _written(16, dtype)
    bits(b.t)[5] = int(b.fill)
    b.guards_intact()
    _fails(b.owned)


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
def test_untouched_and_unchanged(dtype):
    for at in (0, GUARD, GUARD + 63, GUARD + 64, 2 * GUARD + 63):
        b = Guarded(64, dtype, device="cpu")
        b.untouched(), b.unchanged()
        b.buf[at] = 2.0
        _fails(b.untouched)
        _fails(b.unchanged)
    x = torch.arange(64).to(dtype)
    b = Guarded(64, dtype, "x", x, device="cpu")
    b.unchanged()
    assert torch.equal(b.cpu(), x)
    _fails(b.untouched)
    b.t[9] = 77
    _fails(b.unchanged)
    b = Guarded(8, torch.float32, fill=0.0, device="cpu")        # a payload a kernel accumulates into
    assert torch.equal(b.t, torch.zeros(8))
    b.guards_intact(), b.unchanged()


@pytest.mark.parametrize("dtype", DTYPES, **_ID)
def test_offset_and_missing_front_guard(dtype):
    b = Guarded(8, dtype, off=3, device="cpu")
    assert b.ptr().value == b.buf.data_ptr() + (GUARD + 3) * b.buf.element_size() and b.buf.numel() == 2 * GUARD + 3 + 8
    assert b.ptr(2).value == b.ptr().value + 2 * b.t.element_size()
    b.t.fill_(1)
    assert bool((bits(b.buf)[:GUARD + 3] == b.fill).all()) and bool((bits(b.buf)[GUARD + 11:] == b.fill).all())
    b = Guarded(8, dtype, front=False, device="cpu")
    assert b.ptr().value == b.buf.data_ptr() and b.buf.numel() == 8 + GUARD
    b.t.fill_(1)
    b.owned()
    b.buf[8] = 1.0
    _fails(b.guards_intact)


def test_still_fill_and_np():
    b = Guarded(6, device="cpu")
    b.t[:4] = 1.0
    got = b.cpu()
    b.still_fill(got, torch.tensor([False] * 4 + [True] * 2))
    _fails(lambda: b.still_fill(got, torch.tensor([False] * 3 + [True] * 3)))
    assert b.np((2, 3)).shape == (2, 3)
    i = Guarded.of(torch.arange(6, dtype=torch.int32).numpy(), "i", device="cpu")
    assert i.t.dtype == torch.int32 and int(i.fill) == 0x7FC00000 and i.np().tolist() == list(range(6))


# ---- judge -------------------------------------------------------------------------------------------------------------------------
def test_judge_at_and_above_the_bound():
    ref = torch.tensor([1.0, 2.0, -3.0], dtype=torch.float64)
    bound = torch.tensor([0.25, 0.5, 0.125], dtype=torch.float64)
    got = torch.tensor([1.25, 1.75, -3.0])
    assert judge(got, ref, bound) == 1.0                          # error = bound passes
    assert judge(got.numpy(), ref.numpy(), bound.numpy()) == 1.0
    got[0] = 1.2500001
    with pytest.raises(AssertionError, match="element', 0, 'of', 3") as e:
        judge(got, ref, bound, ctx=("entry", "y"))
    assert e.value.args[0][:2] == ("entry", "y") and e.value.args[0][-1] == 1


def test_judge_rejects_what_would_pass_anything():
    one = torch.ones(2, dtype=torch.float64)
    for bad in (float("inf"), float("nan"), -1e-9):
        _fails(lambda: judge(torch.ones(2), one, torch.tensor([1.0, bad], dtype=torch.float64)))
    _fails(lambda: judge(torch.tensor([1.0, float("nan")]), one, one))
    _fails(lambda: judge(torch.ones(2), torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)))
    _fails(lambda: judge(torch.ones(2), one, torch.ones(1, dtype=torch.float64)))
    _fails(lambda: judge(torch.ones(2), torch.tensor([1.0, float("nan")], dtype=torch.float64), one))          # a NaN reference


def test_judge_zero_bound_is_the_once_rounded_value():
    ref = torch.tensor([1.0 / 3.0, 1.0 + 2.0 ** -30], dtype=torch.float64)       # neither is a float
    zero = torch.zeros(2, dtype=torch.float64)
    assert judge(ref.float(), ref, zero) == 0.0 and judge(ref.float(), ref, 0.0, exact="value") == 0.0
    up = ref.float().clone()
    bits(up)[0] += 1
    _fails(lambda: judge(up, ref, zero))
    _fails(lambda: judge(up, ref, zero, exact="value"))
    _fails(lambda: judge(torch.tensor([-0.0]), torch.zeros(1, dtype=torch.float64), 0.0))
    assert judge(torch.tensor([-0.0]), torch.zeros(1, dtype=torch.float64), 0.0, exact="value") == 0.0
    mixed = torch.tensor([0.0, 2.0 ** -20], dtype=torch.float64)                 # zero and positive bounds in one output
    assert judge(up.flip(0), ref.flip(0), mixed) < 1.0
    _fails(lambda: judge(up, ref, mixed))


def test_judge_bf16_zero_bound_is_compared_in_bf16():
    ref = torch.tensor([1.0 + 2.0 ** -8, 3.0], dtype=torch.float64)              # a tie between two bf16 values: to even, 1.0
    got = torch.tensor([1.0, 3.0], dtype=torch.bfloat16)
    assert judge(got, ref, 0.0) == 0.0
    _fails(lambda: judge(got.float(), ref, 0.0))                  # as a float the same value is not the rounded reference
    _fails(lambda: judge(torch.tensor([1.0 + 2.0 ** -7, 3.0], dtype=torch.bfloat16), ref, 0.0))


def test_judge_matching_infinity():
    inf = float("inf")
    ref, bound = torch.tensor([-inf, 1.0], dtype=torch.float64), torch.tensor([1.0, 1.0], dtype=torch.float64)
    got = torch.tensor([-inf, 1.5])
    assert judge(got, ref, bound, equal_inf=True) == 0.5
    _fails(lambda: judge(got, ref, bound))
    _fails(lambda: judge(torch.tensor([inf, 1.5]), ref, bound, equal_inf=True))
    _fails(lambda: judge(got, torch.tensor([1.0, 1.0], dtype=torch.float64), bound, equal_inf=True))


def test_where():
    assert where(0, (2, 3, 4)) == (0, 0, 0) and where(23, (2, 3, 4)) == (1, 2, 3) and where(13, (2, 3, 4)) == (1, 0, 1)


def test_report_prints_the_lines_logs_are_compared_by(capsys):
    report("ELEM", "flat none n=1", [("rfx_act_fwd", 0.0), ("rfx_act_bwd", 0.0), ("rfx_act_fwd", 0.25)])
    report("ELEM", "l1_sum n=5", [0.0625, 0.5])
    report("ELEM", "flat prelu n=1", [])
    report("FX", "compressor B1-T20", [("env", 0.0104), ("y", 0.0)])
    report("FFT", "rfx_fft_synthesis_lossgrad", {"out": 0.0394, "one-ulp cells with sign 0": 0.0},
           f"lg_512_128_512_F16 {['fft_synthesis_kernel<512,LG,own>']}")
    report("LOSS", "sums R3-L1-tn-snr-sum", [("rfx_time_sums", 0.0), ("rfx_sisdr_sums", 0.0)])
    assert capsys.readouterr().out == (
        "\nELEM flat none n=1: largest error / bound rfx_act_fwd 0.250, rfx_act_bwd 0.000\n"
        "\nELEM l1_sum n=5: largest error / bound 0.500\n"
        "\nELEM flat prelu n=1: refused\n"
        "\nFX compressor B1-T20: largest error / bound env 0.010, y 0.000\n"
        "\nFFT rfx_fft_synthesis_lossgrad lg_512_128_512_F16 ['fft_synthesis_kernel<512,LG,own>']: largest error / bound out 0.039, "
        "one-ulp cells with sign 0 0.000\n"
        "\nLOSS sums R3-L1-tn-snr-sum: largest error / bound rfx_time_sums 0.000, rfx_sisdr_sums 0.000\n")


# ---- ref_common --------------------------------------------------------------------------------------------------------------------
def _f(pattern):
    return torch.tensor([pattern], dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_bf16_rounding_by_hand():
    cases = [(0x3F808000, 0x3F800000, 0x3F800000),                # a tie: to the even neighbour below
             (0x3F818000, 0x3F820000, 0x3F810000),                # a tie: to the even neighbour above
             (0x3F808001, 0x3F810000, 0x3F800000),                # just above the tie
             (0x3F807FFF, 0x3F800000, 0x3F800000),                # just below it
             (0x00018000, 0x00020000, 0x00010000),                # a subnormal tie
             (0x7F7FFFFF, 0x7F800000, 0x7F7F0000),                # the largest float rounds to inf, truncates to the largest bf16
             (0x00000000, 0x00000000, 0x00000000), (0x7F800000, 0x7F800000, 0x7F800000)]
    for x, rne, trunc in cases:
        for sign in (0, 0x80000000):
            v = _f(x | sign)
            assert int(bits(RC.bf16_rne(v))) & 0xFFFFFFFF == rne | sign, hex(x)
            assert int(bits(RC.bf16_trunc(v))) & 0xFFFFFFFF == trunc | sign, hex(x)
    assert bool(torch.isnan(RC.bf16_rne(torch.tensor([float("nan")])))) and bool(torch.isnan(RC.bf16_trunc(torch.tensor([float("nan")]))))
    d = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)        # fp64 in: its float value (the tie), in fp64
    assert RC.bf16_rne(d).dtype == torch.float64 and float(RC.bf16_rne(d)) == 1.0


def test_ulp_at_powers_of_two():
    v = torch.tensor([1.0, 1.999, 2.0, -2.0, 0.5, 2.0 ** -126, 2.0 ** -140, 0.0], dtype=torch.float64)
    assert RC.ulp(v, 23).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]
    assert RC.ulp(v, 7).tolist() == RC.ulp16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8] + [2.0 ** -133] * 3
    assert float(RC.ulp(torch.tensor([2.0 ** -140], dtype=torch.float64), 7, 1e-300)) == 2.0 ** -147
    assert RC.f32(0.1) == 0.10000000149011612 and RC.f32(1e40) == float("inf") and RC.EPS32 == 2.0 ** -23
    assert RC.worst(torch.tensor([1.0, float("nan")]), torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64)) == (float("inf"), 1)
