"""Host side of the segmented long-file path (remfx_amd/segment.py: SegmentPlan; scripts/remfx_detect.py: the `+segment_seconds`
overrides) against tests/segment_ref.py.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from tests import segment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L0 = 64
# T below L, equal to L, L + 1, not a multiple of 4, several segments; overlap 0, 0.25, 0.5, 0.75 of L
GRID = [(T, L0, int(L0 * f), lead, trail)
        for T, f in itertools.product((5, 37, 63, 64, 65, 66, 127, 128, 129, 257, 1001, 1024), (0.0, 0.25, 0.5, 0.75))
        for lead, trail in ((0, 0), (int(L0 * f), 0), (int(L0 * f) // 2, int(L0 * f) - int(L0 * f) // 2), (3, 0))
        if lead + trail <= int(L0 * f) and T - lead - trail >= 1]
GRID += [(262144 * 3 + 17, 262144, 65536, 0, 0), (1000, 48, 13, 13, 0), (1000, 48, 13, 6, 7)]


@pytest.mark.parametrize("T,L,overlap,lead,trail", GRID)
def test_plan_properties(T, L, overlap, lead, trail):
    from remfx_amd.segment import SegmentPlan
    p = SegmentPlan(T, L, overlap, lead, trail)
    st = np.asarray(p.starts)
    assert np.array_equal(st, ref.starts(T, L, overlap)) and p.n_segments == len(st)
    assert st[0] == 0 and (np.diff(st) > 0).all()                                  # monotone
    assert p.hop == L - overlap and p.clip_len == L - lead - trail and p.out_len == T - lead - trail
    if T >= L:
        assert st[-1] + L == T                                                     # tail-aligned, not padded
        if len(st) > 1:
            assert st[-2] + L < T                                                  # S is the smallest count that reaches T
    else:
        assert len(st) == 1
    cnt, wsum = ref.cover(T, L, overlap, lead, trail)
    assert cnt.min() >= 1 and cnt.max() <= p.max_cover
    assert cnt.max() == p.max_cover                                                # and the bound is attained
    assert (wsum > 0).all() and (p.weights() > 0).all()
    assert np.array_equal(p.weights(), ref.weights(p.clip_len))


@pytest.mark.parametrize("T,L,overlap", [(t, l, o) for t, l, o, le, tr in GRID if le == 0 and tr == 0 and t < 10000])
def test_reference_merge_inverts_split(T, L, overlap):
    x = np.random.default_rng(T + overlap).standard_normal((3, T))
    clips = ref.split(x, L, overlap)
    assert clips.shape == (3 * len(ref.starts(T, L, overlap)), L)
    if T < L:
        assert (clips[:, T:] == 0).all()
    back = ref.merge(clips, T, L, overlap)
    assert back.shape == x.shape
    assert np.abs(back - x).max() <= 8 * np.finfo(np.float64).eps * np.abs(x).max()


def test_reference_merge_crops_like_the_whole_file():
    """A 'network' that returns its input's valid window (lead / trail dropped) merges to x[lead : T - trail]."""
    T, L, overlap, lead, trail = 1001, 64, 16, 9, 7
    x = np.random.default_rng(1).standard_normal((2, T))
    clips = ref.split(x, L, overlap)[:, lead:L - trail]
    back = ref.merge(clips, T, L, overlap, lead, trail)
    assert np.abs(back - x[:, lead:T - trail]).max() <= 8 * np.finfo(np.float64).eps * np.abs(x).max()


@pytest.mark.parametrize("args", [
    (1000, 64, 64),            # overlap == segment
    (1000, 64, 65),            # overlap > segment
    (1000, 64, -1),
    (1000, 64, 16, 17, 0),     # lead > overlap: the valid windows leave gaps
    (1000, 64, 16, 9, 8),      # lead + trail > overlap
    (1000, 64, 16, -1, 0),
    (10, 64, 16, 10, 0),       # no output sample left
    (12, 64, 16, 8, 4),
    (0, 64, 16),
    (1000, 0, 0),
])
def test_plan_value_errors(args):
    from remfx_amd.segment import SegmentPlan
    with pytest.raises(ValueError):
        SegmentPlan(*args)


def test_overlap_fraction_or_samples():
    from remfx_amd import segment
    assert segment.overlap_samples(262144, 0.25) == 65536
    assert segment.overlap_samples(262144, 1000) == 1000
    with pytest.raises(ValueError):
        segment.overlap_samples(262144, 1.0)


def test_segment_ops_refuse_cpu_tensors():
    import torch
    from remfx_amd import segment
    p = segment.SegmentPlan(100, 32, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        segment.split(torch.randn(1, 1, 100), p)
    with pytest.raises(ValueError, match="no CPU fallback"):
        segment.merge(torch.randn(p.n_segments, 1, 32), p)
    with pytest.raises(ValueError, match="no CPU fallback"):
        segment.apply(lambda z: z, torch.randn(1, 1, 100), 32, 8)


def test_remfx_detect_override_parsing():
    """Without `+segment_seconds` the script takes today's whole-file branch; the new keys arrive as `+key=value` overrides with
    their defaults in the script (cfg/ is not touched)."""
    from remfx_amd import config as rcfg
    from scripts import remfx_detect
    cfg_dir = os.path.join(ROOT, "cfg")
    base = ["+exp=remfx_detect", "+audio_input=in.wav", "+output_path=out.wav"]
    cfg = rcfg.compose(cfg_dir, "config.yaml", base)
    assert remfx_detect.segment_options(cfg) is None
    for k in ("segment_seconds", "overlap", "segment_batch", "detect", "keep_channels"):
        assert k not in cfg
    cfg = rcfg.compose(cfg_dir, "config.yaml", base + ["+segment_seconds=2.5"])
    opt = remfx_detect.segment_options(cfg)
    assert opt == {"segment": int(round(2.5 * cfg["sample_rate"])), "overlap": 0.25, "segment_batch": 64, "detect": "segment",
                   "keep_channels": False}
    cfg = rcfg.compose(cfg_dir, "config.yaml", base + ["+segment_seconds=5.4613333", "+overlap=0.5", "+segment_batch=8",
                                                        "+detect=file", "+keep_channels=true"])
    opt = remfx_detect.segment_options(cfg)
    assert opt == {"segment": 262144, "overlap": 0.5, "segment_batch": 8, "detect": "file", "keep_channels": True}
    with pytest.raises(ValueError):
        remfx_detect.segment_options(rcfg.compose(cfg_dir, "config.yaml", base + ["+overlap=0.5"]))
    with pytest.raises(ValueError):
        remfx_detect.segment_options(rcfg.compose(cfg_dir, "config.yaml", base + ["+segment_seconds=2", "+detect=clip"]))
    with pytest.raises(ValueError):
        remfx_detect.segment_options(rcfg.compose(cfg_dir, "config.yaml", base + ["+segment_seconds=2", "+overlap=1.0"]))


def test_label_timeline_runs():
    import torch
    from scripts.remfx_detect import label_timeline
    names = ["R", "C", "D", "X", "P"]
    lab = torch.tensor([[[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 1, 1], [0, 0, 0, 0, 0]]], dtype=torch.float32)
    lines = label_timeline(lab, [0, 100, 200, 250], 150, 100, names, 400)
    assert len(lines) == 3
    assert "0.00 s" in lines[0] and "2.00 s" in lines[0] and lines[0].endswith("R")
    assert "2.00 s" in lines[1] and "2.50 s" in lines[1] and lines[1].endswith("X, P")
    assert "4.00 s" in lines[2] and lines[2].endswith("none")


# ---- the kernel-side case table of tests/test_gpu_segment_kernel.py -------------------------------------------------
def test_merge_bound_holds_for_the_fp32_restatement_of_the_kernel_order():
    """the per-element bound against float32 numpy, the sum in the kernel's order (products rounded: no FMA), over the whole table; the
    largest error / bound is printed"""
    worst = 0.0
    for (B, C, T, L, overlap, lead, trail) in ref.CASES:
        y = ref.merge_input(B, C, T, L, overlap, lead, trail)
        want = ref.merge(y, T, L, overlap, lead, trail)
        bound = ref.merge_bound(y, T, L, overlap, lead, trail)
        assert bound.shape == want.shape and (bound > 0).all()
        q = float((np.abs(ref.merge_restate32(y, T, L, overlap, lead, trail).astype(np.float64) - want) / bound).max())
        assert q <= 1.0, ((B, C, T, L, overlap, lead, trail), q)
        worst = max(worst, q)
    print("\nsegment merge, CPU restatement, largest error / bound:", round(worst, 3))


@pytest.mark.parametrize("fault,case", [("weights_min_j", ref.CASES[1]), ("tail_after_last", ref.CASES[1]), ("tail_twice", ref.CASES[0])])
def test_merge_bound_rejects_planted_faults_the_global_bound_accepts(fault, case):
    """clip i scaled by 1, 1e3, 1e-3: a weight off by one, the tail clip taken one sample late, a clip counted twice are outside the
    per-element bound; tests/test_gpu_segment.py's global (max_cover + 3) half-ulps of max |y| is what they are compared with"""
    B, C, T, L, overlap, lead, trail = case
    y = ref.merge_input(B, C, T, L, overlap, lead, trail)
    want, bound = ref.merge(y, T, L, overlap, lead, trail), ref.merge_bound(y, T, L, overlap, lead, trail)
    bad = ref.merge_restate32(y, T, L, overlap, lead, trail, mutate=fault).astype(np.float64)
    err = np.abs(bad - want)
    assert not (err <= bound).all()
    cnt, _ = ref.cover(T, L, overlap, lead, trail)
    quiet = np.abs(want) < 1e-2 * np.abs(y).max()              # where a loud clip has faded out: the global bound is blind there
    assert quiet.any()
    glob = (cnt.max() + 3) * 2.0 ** -24 * np.abs(y).max()
    assert (bound[quiet] < glob).all()


def test_grouped_layout_round_trip():
    B, S, C, n = 2, 3, 3, 5
    a = np.arange(B * C * S * n, dtype=np.float32).reshape(B * C * S, n)
    g = ref.group(a, B, S, C)
    assert np.array_equal(ref.ungroup(g, B, S, C), a)
    # clip (b = 1, segment 2, channel 0) sits at row (1 * S + 2) * C + 0 and came from row (1 * C + 0) * S + 2
    assert np.array_equal(g[(1 * S + 2) * C + 0], a[(1 * C + 0) * S + 2])


def test_kernel_case_table_reaches_both_forms_and_every_chunk_edge():
    seen = {"split": set(), "merge": set()}
    steer = {"split": set(), "merge": set()}
    for (B, C, T, L, overlap, lead, trail) in ref.CASES:
        assert T <= 4096
        for kind, args in (("split", (T, L, overlap)), ("merge", (T, L, overlap, lead, trail))):
            f = ref.forms(kind, *args)
            seen[kind].add(f)
            steer[kind] |= ref.steering(kind, *args)
            if f == "vec":                                     # a base one sample past the boundary: dword
                assert ref.forms(kind, *args, in_off=1) == "dword" and ref.forms(kind, *args, out_off=1) == "dword"
    assert seen == {"split": {"vec", "dword"}, "merge": {"vec", "dword"}}
    assert steer["split"] == {"chunks=1", "chunks>1", "ragged_chunk", "exact_chunk", "zero_fill", "tail_on_grid", "tail_off_grid"}
    assert steer["merge"] == {"chunks=1", "chunks>1", "ragged_chunk", "exact_chunk", "tail_on_grid", "tail_off_grid"}
    assert {252, 256, 260} <= {c[3] for c in ref.CASES}
    assert max(int(ref.cover(*c[2:])[0].max()) for c in ref.CASES) == 4
    assert {c[1] for c in ref.CASES} == {1, 2, 3}
    # by hand: lengths multiples of 4 and the hop not -> dword; L' = 491 -> merge dword while split stays vec
    assert ref.forms("split", 1000, 256, 62) == "dword" and ref.forms("merge", 1280, 512, 128, 21, 0) == "dword"
    assert ref.forms("split", 1280, 512, 128) == "vec"
    assert ref.forms("merge", 1000, 64, 16, 9, 8) is None and ref.forms("merge", 10, 64, 16, 10, 0) is None
