"""The framed-FFT kernels that walk a batch / frame loop at three waves per SIMD keep nothing in private memory: csrc/fft.hip is
compiled for gfx950 (device code only, no GPU needed) and the compiler's own resource remarks and ISA are checked.  A spilled
register inside those loops is reloaded in every batch and, at 64 clips, turned the 1024- and 2048-point loss kernels' 0.56 GB per
launch into 1.7 and 2.1 GB; an edit of the file that brings spills back fails here instead of showing up as a slower
step."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIR = ["fft_pair_loss_kernel<10>", "fft_pair_loss_kernel<11>"]
SYN_LG = ["fft_synthesis_kernel<%d, true, %s>" % (n, o) for n in (8, 9, 10, 11) for o in ("false", "true")]


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.analyse(os.path.join(ROOT, "remfx_amd", "csrc", "fft.hip"))


@pytest.mark.parametrize("name", PAIR + SYN_LG)
def test_no_private_memory_at_three_waves(report, name):
    res, loops = report
    assert name in res, sorted(res)
    r = res[name]
    assert r["scratch"] == 0, r
    assert r["occupancy"] >= 3, r                              # not bought with a lower occupancy
    assert r["lds"] <= 54528, r                                # three workgroups per CU: 160 KB of LDS, allocated in 512-byte units
    assert loops[name] == (0, 0, 0, 0), loops[name]


def test_pair_loss_512_point_form_unchanged(report):
    """n_fft 512 runs at two waves per SIMD by design (53 KB of LDS: two workgroups per CU whatever the registers) and never spilled."""
    r = report[0]["fft_pair_loss_kernel<9>"]
    assert r["scratch"] == 0 and r["occupancy"] >= 2, r
