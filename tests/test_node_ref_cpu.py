"""tests/node_ref.py on the CPU: the runner on a plain-torch stand-in Function -- every variant passes for the correct
stand-in and rejects the host fault it is named for -- and the argument-exchange rule over the case tables.  No fault is planted into
anything that runs on a device."""
import pytest
import torch

from tests import node_ref as R

DEV = "cpu"
ROUTES = ("side", "off")


@pytest.fixture
def standin():
    case = R.standin_case()
    R.StandIn.FAULT = None
    inp, anchor, ratios = R.v0(case, DEV, "f32")
    yield case, inp, anchor
    R.StandIn.FAULT = None


def _variant(name, case, inp, anchor):
    if name == "V0":
        return R.v0(case, DEV, "f32")
    if name in ("V5", "V6"):
        return getattr(R, name.lower())(case, DEV, "f32", inp, anchor, R.standin_arm, ROUTES)
    return getattr(R, name.lower())(case, DEV, "f32", inp, anchor)


def test_the_correct_stand_in_passes_every_variant(standin):
    case, inp, anchor = standin
    for v in ("V0", "V1", "V2", "V3", "V4", "V5", "V6"):
        _variant(v, case, inp, anchor)


# fault -> the variants that have to reject it
REJECTED_BY = {"slot": ("V0", "V2"), "ignore_needs": ("V2",), "gy_pointer": ("V3",), "dx_zero_stride": ("V1",), "assign": ("V6",),
               "double_count": ("V5",), "swap_ints": ("V0",)}


def test_every_fault_is_listed():
    assert set(REJECTED_BY) == set(R.FAULTS)


# what the rejecting assertion has to say: a fault does not count as rejected because something else went wrong
SAYS = {("slot", "V0"): "d_w", ("slot", "V2"): "gradient missing", ("ignore_needs", "V2"): "backward returned a tensor in slot",
        ("gy_pointer", "V3"): "V3 transposed", ("dx_zero_stride", "V1"): "d_x", ("assign", "V6"): "V6",
        ("double_count", "V5"): "written through the sink AND returned to autograd", ("swap_ints", "V0"): "'y'"}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_variant_rejects_its_fault(standin, fault):
    case, inp, anchor = standin
    for v in REJECTED_BY[fault]:
        R.StandIn.FAULT = fault
        with pytest.raises(AssertionError) as e:
            if fault == "gy_pointer":                 # the expanded scalar is torch's own refusal: the test below
                R.v3(case, DEV, "f32", inp, anchor, forms=R.GY_FORMS[1:])
            else:
                _variant(v, case, inp, anchor)        # the anchor is the correct stand-in's: a fault cannot hide in its own anchor
        assert SAYS[(fault, v)] in str(e.value), (fault, v, e.value)
        R.StandIn.FAULT = None


@pytest.mark.parametrize("form", R.GY_FORMS)
def test_each_gradient_layout_rejects_the_pointer_read(standin, form):
    """V3, form by form: the expanded scalar has one element of storage (torch refuses the dense read), the other two give wrong values"""
    case, inp, anchor = standin
    R.StandIn.FAULT = "gy_pointer"
    if form == "sum":
        with pytest.raises(RuntimeError, match="out of bounds for storage"):
            R.v3(case, DEV, "f32", inp, anchor, forms=(form,))
    else:
        with pytest.raises(AssertionError, match="V3 " + form):
            R.v3(case, DEV, "f32", inp, anchor, forms=(form,))


@pytest.mark.parametrize("fault", ("ignore_needs", "gy_pointer", "dx_zero_stride", "assign", "double_count"))
def test_the_anchor_alone_does_not_see_the_layout_and_route_faults(standin, fault):
    """why V1..V6 exist: contiguous inputs with every gradient requested (what the RMS tests ran) pass with these faults planted"""
    case, inp, anchor = standin
    R.StandIn.FAULT = fault
    R.v0(case, DEV, "f32")


def test_exchanged_integers_hide_behind_equal_extents():
    """the reason for the exchange rule: rows == cols makes the exchanged stand-in indistinguishable, and the rule flags that table"""
    square = R.standin_case(rows=4, cols=4, N=3)
    assert R.exchange_rule(square) and not R.exchange_rule(R.standin_case())
    R.StandIn.FAULT = "swap_ints"
    try:
        R.v0(square, DEV, "f32")
    finally:
        R.StandIn.FAULT = None


def test_case_tables_obey_the_exchange_rule():
    bad = [b for c in R.case_table() for b in R.exchange_rule(c)]
    assert not bad, bad
    for c in R.case_table():
        inp = c.make(0)
        for k, sc in c.scales.items():
            assert k in inp or k in ("res", "scale", "rm"), (c.id, "scale of an input the case does not have", k)
        if len(c.diff) + len([k for k in c.tensors(inp) if k not in c.diff]) > 1:
            assert len(c.scales) >= 2, (c.id, "several tensor inputs, one scale")


def test_layouts_hold_the_values_they_claim():
    t = torch.randn(3, 4, 5, 6)
    for kind in R.LAYOUTS:
        v, vals = R.lay(t, kind)
        assert torch.equal(v.contiguous(), vals) and v.shape == t.shape
        assert not v.is_contiguous() or kind == "offset"
    assert R.lay(t, "offset")[0].data_ptr() % 16 == 4 and R.lay(t, "expand")[0].stride(0) == 0 and R.lay(t, "slice")[0].storage_offset() > 0
    v, vals = R.lay(torch.randn(7), "perm")
    assert v.stride() == (2,) and torch.equal(v.contiguous(), vals)
    g = torch.randn(2, 3, 4)
    for form in ("transposed", "slice"):
        assert torch.equal(R.lay_gy(g, form), g) and not R.lay_gy(g, form).is_contiguous()
    assert R.lay_gy(g, "transposed").stride(-1) != 1


def test_subsets_are_capped():
    assert R.subsets(("a",)) == [("a",)]
    assert R.subsets(("a", "b")) == [("a",), ("b",), ("a", "b")]
    assert len(R.subsets(("a", "b", "c", "d", "e"))) == 11


def test_every_case_has_a_reference_or_says_why():
    for c in R.case_table():
        assert c.ref is not None or c.note, c.id
        assert c.expect, c.id
