"""The write protocol of the parameter-gradient sink (ops.GradSink), through its one entry ops.sink_write: what is recognised,
all-or-nothing claims, which stream the body runs on, and when / where / in which order the writes are counted.  No model, no
kernel of the library beyond the fill of the gradient buffer: three tiny parameters in an optim.FlatParams buffer."""
import pytest
import torch

from remfx_amd import ops, optim

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]

SHAPES = ((2, 4), (5,), (3, 4))             # 8, 5, 12 elements: the second view's 5 pad to 8, offsets 0 / 8 / 16


@pytest.fixture
def armed():
    """(flat, parameters, calls, outer): an armed sink whose on_write appends (parameter index, raw handle of the current stream) to
    `calls`; the test body runs with `outer`, a stream of its own, current -- so "the caller's stream" is not the default one."""
    prev = ops.GradSink.MODE
    ops.GradSink.MODE = "side"
    try:
        ps = [torch.nn.Parameter(torch.randn(*s, device="cuda")) for s in SHAPES]
        flat = optim.FlatParams(ps)
        flat.zero_grad()
        calls = []
        flat.sink.on_write = lambda i: calls.append((i, ops.raw_stream()))
        outer = torch.cuda.Stream()
        outer.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(outer):
            yield flat, ps, calls, outer
            flat.join()
        torch.cuda.synchronize()
    finally:
        ops.GradSink.MODE = prev
    assert ops.SINK is None


def test_flat_layout_pads_offsets_to_16_bytes(armed):
    flat = armed[0]
    assert flat.offsets == [0, 8, 16] and flat.numel == 28
    assert ops.SINK is flat.sink and flat.sink.side is not None and flat.sink.writes == [0, 0, 0]


def test_a_recognised_parameter_yields_its_slice_of_the_gradient_buffer(armed):
    flat, ps, calls, _ = armed
    for i, p in enumerate(ps):
        for t in (p, p.detach(), p.unsqueeze(1) if p.dim() == 1 else p.unsqueeze(2)):
            sw = ops.sink_write(t)
            assert sw is not None and len(sw.grads) == 1
            v = sw.grads[0]
            assert v.data_ptr() == flat.grad.data_ptr() + 4 * flat.offsets[i] and v.numel() == p.numel() and v.dim() == 1
            assert v.data_ptr() == p.grad.data_ptr()
    sw = ops.sink_write(ps[2], None, ps[0])              # an absent bias: skipped, a None view in its place
    assert sw is not None and sw.grads[1] is None
    assert [v.data_ptr() for v in (sw.grads[0], sw.grads[2])] == [ps[2].grad.data_ptr(), ps[0].grad.data_ptr()]
    assert flat.sink.writes == [0, 0, 0] and calls == []                  # a claim alone counts nothing


def test_a_refused_claim_counts_nothing_and_touches_no_stream(armed):
    flat, ps, calls, outer = armed
    sink = flat.sink
    streams = dict(sink.write_streams)
    outside = torch.zeros(8, device="cuda")
    refused = [(ps[0].t(),),                             # same start address and numel, not contiguous
               (outside,),                               # not in the buffer
               (ps[0], outside),                         # known + unknown: all or nothing
               (outside, ps[0]),
               (ps[2].detach().view(-1)[:8],),           # a parameter's start address, another numel
               (ps[0].detach().view(torch.int32),),      # not fp32
               (ps[0].detach().cpu(),)]                  # not on the GPU
    for claim in refused:
        assert ops.sink_write(*claim, operands=(outside,)) is None
        assert ops.sink_write(*claim) is None
        assert ops.sink_write(*claim, first_write=True) is None
    assert sink.writes == [0, 0, 0] and calls == []
    assert sink.used_side is False and sink.write_streams == streams
    assert torch.cuda.current_stream() == outer


def test_operands_send_the_body_to_the_side_stream_and_writes_are_counted_outside(armed):
    flat, ps, calls, outer = armed
    sink = flat.sink
    x = torch.ones(4, device="cuda")
    sw = ops.sink_write(ps[1], ps[0], operands=(x, None))
    assert torch.cuda.current_stream() == outer and sink.used_side is False       # nothing happens before the scope is entered
    with sw:
        assert torch.cuda.current_stream() == sink.side
        assert ops.raw_stream() == sink.side.cuda_stream
        assert sink.used_side is True
        assert calls == [] and sink.writes == [0, 0, 0]
    assert torch.cuda.current_stream() == outer
    # once per claimed parameter, in ARGUMENT order, with the caller's stream current
    assert calls == [(1, outer.cuda_stream), (0, outer.cuda_stream)]
    assert sink.writes == [1, 1, 0]
    assert set(sink.write_streams) == {outer.cuda_stream} and sink.side.cuda_stream not in sink.write_streams


def test_without_operands_the_stream_stays(armed):
    flat, ps, calls, outer = armed
    sink = flat.sink
    with ops.sink_write(ps[2]):
        assert torch.cuda.current_stream() == outer and ops.raw_stream() == outer.cuda_stream
        assert calls == []
    assert torch.cuda.current_stream() == outer
    assert sink.used_side is False
    assert calls == [(2, outer.cuda_stream)] and sink.writes == [0, 0, 1]
    assert set(sink.write_streams) == {outer.cuda_stream}


def test_without_a_side_stream_operands_do_not_move_the_body(armed):
    flat, ps, calls, outer = armed
    sink = flat.sink
    side, sink.side = sink.side, None                    # what bench.py / the full-size property test set for the one-stream pass
    try:
        x = torch.ones(4, device="cuda")
        with ops.sink_write(ps[0], ps[1], operands=(x,)):
            assert torch.cuda.current_stream() == outer and ops.raw_stream() == outer.cuda_stream
        assert torch.cuda.current_stream() == outer
        assert sink.used_side is False
        assert calls == [(0, outer.cuda_stream), (1, outer.cuda_stream)] and sink.writes == [1, 1, 0]
        assert set(sink.write_streams) == {outer.cuda_stream}
    finally:
        sink.side = side


def test_first_write_is_refused_after_a_write_accumulate_is_not(armed):
    flat, ps, calls, _ = armed
    sink = flat.sink
    assert ops.sink_write(ps[0], ps[1], first_write=True) is not None      # nothing written yet (and a claim alone writes nothing)
    with ops.sink_write(ps[1], first_write=True):
        pass
    assert sink.writes == [0, 1, 0]
    assert ops.sink_write(ps[1], first_write=True) is None
    assert ops.sink_write(ps[0], ps[1], ps[2], first_write=True) is None    # one written parameter refuses the whole claim
    assert ops.sink_write(ps[0], ps[2], first_write=True) is not None
    assert sink.writes == [0, 1, 0] and len(calls) == 1
    with ops.sink_write(ps[1]):                                             # accumulating writers still get it
        pass
    assert sink.writes == [0, 2, 0] and [c[0] for c in calls] == [1, 1]


def test_a_side_stream_write_is_visible_after_join_and_join_disarms(armed):
    flat, ps, calls, outer = armed
    sink = flat.sink
    x = torch.ones(4, device="cuda")
    with ops.sink_write(ps[1], operands=(x,)) as sw:
        sw.grads[0].add_(1.0)
    assert sink.used_side is True
    flat.join()
    torch.cuda.synchronize()
    assert ps[1].grad.tolist() == [1.0] * 5
    assert flat.grad.tolist() == [0.0] * 8 + [1.0] * 5 + [0.0] * 15         # the padding and the neighbours untouched
    assert ops.SINK is None and sink.write_streams == {} and sink.used_side is False
    assert ops.sink_write(ps[1]) is None and ops.sink_write(ps[1], operands=(x,)) is None
    assert sink.writes == [0, 1, 0] and len(calls) == 1
