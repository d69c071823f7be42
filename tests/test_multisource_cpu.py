"""CPU: multi-source Hybrid Demucs -- construction against the oracle's state_dict, the parameter order optim.FlatParams needs,
the new C-ABI symbols, and the error paths of the channel-grouped segment functions.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rfx_fm_cm_affine_g", "rfx_row_affine_add", "rfx_segment_split_c", "rfx_segment_merge_c"]


def _nets(S, Cin):
    from oracle import ref_hdemucs
    from remfx_amd.hdemucs import HDemucs
    names = [f"s{i}" for i in range(S)]
    torch.manual_seed(0)
    ref = ref_hdemucs.HDemucs(sources=names, audio_channels=Cin, nfft=4096, channels=8)
    net = HDemucs(sources=names, audio_channels=Cin, nfft=4096, channels=8)
    return ref, net


@pytest.mark.parametrize("S,Cin", [(2, 1), (4, 2)])
def test_state_dict_matches_the_oracle(S, Cin):
    ref, net = _nets(S, Cin)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want
    net.load_state_dict(ref.state_dict(), strict=True)
    # the last decoder layers carry the sources: (source, channel, re / im) channels on the frequency side
    assert net.freq_decoder[-1].conv_tr.out_channels == S * Cin * 2
    assert net.time_decoder[-1].conv_tr.out_channels == S * Cin


@pytest.mark.parametrize("S,Cin", [(2, 1), (4, 2)])
def test_forward_use_order_names_every_parameter_once(S, Cin):
    from remfx_amd.optim import FlatParams
    _, net = _nets(S, Cin)
    order = net.forward_use_order()
    trainable = [p for p in net.parameters() if p.requires_grad]
    assert len(order) == len(trainable)
    assert len({id(p) for p in order}) == len(order)
    assert {id(p) for p in order} == {id(p) for p in trainable}
    FlatParams(list(net.parameters()), allow_cpu=True, layout=order)          # raises when the layout misses or repeats a parameter


def test_new_symbols_are_declared_bound_and_exported():
    from remfx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "remfx_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert callable(getattr(L, name)), name


def test_grouped_segment_functions_refuse_cpu_tensors_and_wrong_shapes():
    from remfx_amd import segment
    plan = segment.SegmentPlan(1000, 400, 100)
    with pytest.raises(Exception):
        segment.split_c(torch.zeros(1, 2, 1000), plan)             # no CPU fallback
    with pytest.raises(Exception):
        segment.merge_c(torch.zeros(plan.n_segments, 2, 400), plan)
    with pytest.raises(Exception):
        segment.apply(lambda c: c, torch.zeros(1, 2, 1000), 400, 100, group_channels=True)


def test_separate_checks_the_channel_count():
    _, net = _nets(2, 1)
    with pytest.raises(ValueError):
        net.separate(torch.zeros(1, 2, 1000))
    assert net.training                                         # the mode is restored on every path


def test_separate_script_options_and_checkpoint_keys(tmp_path):
    from scripts import separate
    opt = separate.parse(["+checkpoint=a.ckpt", "audio_input=in.wav", "+output_dir=out", "+sources=dry,wet", "+audio_channels=1",
                          "+segment_seconds=2.5"])
    assert opt["sources"] == ["dry", "wet"] and opt["audio_channels"] == 1 and opt["segment_seconds"] == 2.5
    assert opt["overlap"] == separate.DEFAULTS["overlap"] and opt["checkpoint"] == "a.ckpt"
    for bad in (["+checkpoint=a"], ["+checkpoint=a", "+audio_input=b", "+output_dir=c", "+nonsense=1"],
                ["+checkpoint=a", "+audio_input=b", "+output_dir=c", "+audio_channels=3"]):
        with pytest.raises(ValueError):
            separate.parse(bad)
    sd = {"freq_emb.embedding.weight": torch.zeros(2, 2), "time_decoder.0.conv_tr.bias": torch.ones(3)}
    for prefix, wrap in (("", False), ("model.", True), ("model.model.", True)):
        path = tmp_path / f"c{len(prefix)}.ckpt"
        keyed = {prefix + k: v for k, v in sd.items()}
        torch.save({"state_dict": keyed} if wrap else keyed, path)
        got = separate.load_state(str(path))
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(FileNotFoundError):
        separate.load_state(str(tmp_path / "missing.ckpt"))
    assert separate.fit_channels(torch.ones(1, 5), 2).shape == (2, 5)
    assert torch.equal(separate.fit_channels(torch.tensor([[1.0, 3.0], [3.0, 5.0]]), 1), torch.tensor([[2.0, 4.0]]))
