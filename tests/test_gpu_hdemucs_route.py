"""GPU box, no kernel launched: which path HDemucs.forward takes (remfx_amd/hdemucs.py, HDemucs._route) for the configurations the
suite and bench.py run.  A clause that silently switches the frame-major ends, a fused DConv branch or the second stream off changes
no result beyond the accuracy bounds -- only the step time -- so the whole record is pinned here as literals.

The literals are what the commit before the route record existed selected, read off its launch traces (scripts/launch_trace.py:
which of rfx_cl_dconv_fwd / rfx_dconv_layer_fwd / the channel-major GEMMs follow each layer's head, rfx_cl_im2col_fm / _s4,
wait_stream lines, rfx_fm_cm_affine) and off its routing clauses evaluated one by one.  rfx_cl_dconv_ok accepts C = 48 and 96
only, hence (True, True, False, False) for channels=48 and all False for channels=16."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]
DEV = "cuda:0"
FLAGS = ("CL_TRUNK", "CL_TIME", "CL_ENDS", "FM_ENDS", "CL_DCONV", "CL_TIME_DCONV", "TWO_STREAMS")
T, F = True, False
OFF = (0, 0, (), (), F, F, F, F, F)                  # everything channel-major on one stream
D48, NO4 = (T, T, F, F), (F, F, F, F)

#        model, (Cin, length), mode, flag off   -> (Lc, Lt, dcl, tdcl, im2col, fm, two, cl_tail, cl_tail_t)
CASES = [
    ("remfx48", (1, 262144), "bf16", None,            (4, 4, D48, D48, T, T, T, T, T)),
    ("remfx48", (1, 262144), "f32", None,             OFF),
    ("remfx48", (1, 262144), "bf16", "CL_TRUNK",      OFF),
    ("remfx48", (1, 262144), "bf16", "CL_TIME",       (4, 0, D48, (), T, T, F, T, F)),
    ("remfx48", (1, 262144), "bf16", "CL_ENDS",       (4, 4, D48, (F, T, F, F), F, F, T, F, F)),
    ("remfx48", (1, 262144), "bf16", "FM_ENDS",       (4, 4, D48, D48, T, F, T, T, T)),
    ("remfx48", (1, 262144), "bf16", "CL_DCONV",      (4, 4, NO4, NO4, F, F, T, T, T)),
    ("remfx48", (1, 262144), "bf16", "CL_TIME_DCONV", (4, 4, D48, NO4, T, T, T, T, T)),
    ("remfx48", (1, 262144), "bf16", "TWO_STREAMS",   (4, 4, D48, D48, T, T, F, T, T)),
    ("remfx48", (1, 262144 + 1024), "bf16", None,     OFF),                               # 257 frames: no whole tiles
    ("remfx48", (1, 262144 - 512), "bf16", None,      (4, 0, D48, (), T, T, F, T, F)),    # 256 frames, but no whole time tiles
    ("two16", (1, 262144), "bf16", None,              (4, 4, NO4, NO4, F, F, T, F, T)),   # 4 spectrum channels out: generic; 2 time: node
    ("stereo8", (2, 30000), "bf16", None,             OFF),
    ("stereo8", (2, 30000), "f32", None,              OFF),
]


@pytest.fixture(scope="module")
def nets():
    from remfx_amd.hdemucs import HDemucs
    return {"remfx48": HDemucs(sources=["mixture"], audio_channels=1, nfft=4096, channels=48),
            "two16": HDemucs(sources=["dry", "residual"], audio_channels=1, nfft=4096, channels=16),
            "stereo8": HDemucs(sources=["dry", "residual"], audio_channels=2, channels=8)}


@pytest.mark.parametrize("model,clip,mode,off,want", CASES, ids=[f"{c[0]}-{c[1][1]}-{c[2]}-{c[3] or 'default'}" for c in CASES])
def test_route_is_what_the_scattered_clauses_selected(nets, monkeypatch, model, clip, mode, off, want):
    from remfx_amd import hdemucs, ops
    for k in FLAGS:
        monkeypatch.setattr(hdemucs, k, k != off)
    prev = ops.gemm_precision()
    ops.set_gemm_precision(mode)
    try:
        net, dev = nets[model], torch.device(DEV)
        r = net._route(*clip, dev)
        assert r == hdemucs._Route(*want)
        if -(-clip[1] // net.hop_length) == 256:
            assert net._cl_layers(256, dev) == r.Lc
    finally:
        ops.set_gemm_precision(prev)
