"""GPU: every launchable form of the channel-major gather-GEMM family (csrc/gemm*.hip), through the shipped launch path (plan cache,
pack_cached, gemm_fwd / conv2d_dgrad / _merged_launch / gemm_wgrad + the unpack entry points), judged PER ELEMENT against the
operand-rounded fp64 reference of tests/gemm_ref.py.  Each case names the instantiation it is meant to reach and the
launchers' own variant codes (rfx_gemm_fwd_variant / rfx_gemm_wgrad_variant) must agree before anything is judged.  Outputs are NaN-filled
between NaN guards; every case runs twice into fresh buffers and everything that is not an atomic sum must come back bit for bit."""
import pytest
import torch

from tests import gemm_ref as R
from tests.kernel_harness import Arena, guarded, stop_after_a_device_error  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

CASES = R.case_table()
ATOMIC = ("gparam", "stat")


def _run(case, inp, dev):
    arena = Arena(dev)
    with R.case_env(case) as (tf, tw), R.recorder(False) as px:
        out = guarded(lambda: R.launch(case, inp, dev, arena.alloc), case.id)
        fwd, wg = R.forms_of(case, list(tf), list(tw), px.fwd_rows)
    assert tuple(fwd + wg) == case.form, (case.id, fwd, wg)
    arena.check()
    gap = out.pop("_gap", None)                         # output into a channel slice: the spare channels behind it are not the kernel's
    if gap is not None:
        assert bool(torch.isnan(gap).all()), (case.id, "store past the last channel of the slice")
    got = {k: (v.double() if v.dtype == torch.float64 else v.float()).cpu() for k, v in out.items()}
    for k, v in got.items():
        assert not bool(torch.isnan(v).any()), (case.id, k, "element left unwritten")
    return got


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_form(case):
    dev = torch.device("cuda:0")
    inp = R.make_inputs(case)
    got = _run(case, inp, dev)
    res = R.judge(case, inp, got)
    print(case.id, case.form[-1], {k: round(q, 3) for k, (q, _, _) in res.items()})
    for k, (q, i, r) in res.items():
        assert q <= 1.0, (case.id, k, "error / tolerance", q, "flat index", i, "got", float(got[k].reshape(-1)[i]), "ref", float(r.ref.reshape(-1)[i]))
    again = _run(case, inp, dev)
    for k in got:
        if k not in ATOMIC:
            assert torch.equal(got[k], again[k]), (case.id, k, "second run differs")
