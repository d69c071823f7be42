"""Dev tool: one Hybrid Demucs forward (+ backward) with every call into the native library and every Stream.wait_stream
printed in program order -- symbol, scalar arguments, pointers as 0 / p, descriptor fields, the stream as the ordinal of its first
appearance.  No addresses, times or call sites: two commits that route a clip the same way print the same text, so `diff` is the
check for a refactor of the host code.  Host-side queries (symbols without a stream argument) are printed with a leading `#q`.
    python scripts/launch_trace.py --channels 48 --shape 2 1 262144 --mode bf16 [--no-grad] [CL_TRUNK=0 ...] [--dump DIR] > trace.txt"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from remfx_amd import _lib


def is_launch(name):
    """A symbol that enqueues work: its last argument is the stream."""
    a = _lib.SIGNATURES[name]
    return len(a) >= 2 and a[-1] is C.c_void_p


def wrap_library(make, queries=True):
    """Replace every symbol of _lib.SIGNATURES on the loaded library by make(name, fn); queries=False: the launching ones only."""
    L = _lib.lib()
    for name in _lib.SIGNATURES:
        if queries or is_launch(name):
            setattr(L, name, make(name, getattr(L, name)))


def _fields(o):
    out = []
    for name, typ in o._fields_:
        v = getattr(o, name)
        if issubclass(typ, C.Structure):
            out.append(f"{name}={{{_fields(v)}}}")
        elif issubclass(typ, C.Array):
            out.append(f"{name}=[{''.join('p' if e else '0' for e in v)}]")
        else:
            out.append(f"{name}={('p' if v else '0') if typ is C.c_void_p else repr(v)}")
    return " ".join(out)


def _arg(v, typ):
    o = getattr(v, "_obj", None)                     # byref(...)
    if isinstance(o, C.Structure):
        return "{" + _fields(o) + "}"
    v = getattr(v if o is None else o, "value", v)
    return ("p" if v else "0") if typ is C.c_void_p else repr(v)


def install(lines):
    """Append one line per native call and per wait_stream to `lines`."""
    ordinals = {}

    def stream(handle):
        return f"s{ordinals.setdefault(handle or 0, len(ordinals))}"

    def make(name, fn):
        types = _lib.SIGNATURES[name]
        launch = is_launch(name)

        def traced(*args):
            n = len(args) - launch
            text = " ".join(_arg(v, t) for v, t in zip(args[:n], types))
            lines.append(f"{name} {text} {stream(getattr(args[-1], 'value', args[-1]))}" if launch else f"#q {name} {text}")
            return fn(*args)
        return traced

    wrap_library(make)
    wait = torch.cuda.Stream.wait_stream

    def wait_stream(self, other):
        lines.append(f"wait_stream {stream(self.cuda_stream)} <- {stream(other.cuda_stream)}")
        return wait(self, other)
    torch.cuda.Stream.wait_stream = wait_stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", nargs="+", default=["mixture"])
    ap.add_argument("--audio-channels", type=int, default=1)
    ap.add_argument("--nfft", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=48)
    ap.add_argument("--shape", type=int, nargs=3, default=[2, 1, 262144])
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--no-grad", action="store_true", help="eval mode under torch.no_grad(), forward only")
    ap.add_argument("--dump", help="directory for the output and every parameter gradient (dump.pt)")
    ap.add_argument("flags", nargs="*", help="KEY=0 / KEY=1 overrides of the module flags of remfx_amd.hdemucs")
    a = ap.parse_args()
    from remfx_amd import hdemucs, ops
    for kv in a.flags:
        k, v = kv.split("=")
        assert isinstance(getattr(hdemucs, k), bool), k
        setattr(hdemucs, k, v != "0")
    ops.set_gemm_precision(a.mode)
    torch.manual_seed(0)
    net = hdemucs.HDemucs(sources=a.sources, audio_channels=a.audio_channels, nfft=a.nfft, channels=a.channels).to("cuda")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(*a.shape, generator=g) * 0.1).to("cuda")
    gy = torch.randn(a.shape[0], len(a.sources), a.shape[1], a.shape[2], generator=g).to("cuda")
    torch.cuda.synchronize()
    lines = []
    install(lines)
    if a.no_grad:
        net.eval()
        with torch.no_grad():
            y = net(x)
    else:
        y = net(x)
        lines.append("---- backward")
        y.backward(gy)
    torch.cuda.synchronize()
    print("\n".join(lines))
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        out = {"output": y.detach().cpu()}
        out.update({"grad/" + n: p.grad.cpu() for n, p in net.named_parameters() if p.grad is not None})
        torch.save(out, os.path.join(a.dump, "dump.pt"))


if __name__ == "__main__":
    main()
