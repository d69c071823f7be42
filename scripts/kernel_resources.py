"""Dev tool: registers, scratch, occupancy and LDS of every kernel of one HIP source, from the compiler's own resource remarks
(-Rpass-analysis=kernel-resource-usage), compiled for gfx950 with the flags the library is built with.  Needs hipcc, no GPU.
usage: python scripts/kernel_resources.py remfx_amd/csrc/fft.hip [--filter SUBSTR] [--loops] [-D NAME=VALUE ...]
  --filter SUBSTR   only kernels whose demangled name contains SUBSTR
  --loops           also print the private-memory (scratch) loads / stores of the ISA that sit INSIDE a loop: the lines between a label
                    and a later branch back to it.  A spill outside every loop is paid once per workgroup; one inside is paid per
                    frame batch
  -D NAME=VALUE     extra defines (A/B of a build switch)
Importable: analyse(path, defines=()) -> ({demangled name: {"vgprs", "agprs", "sgprs", "scratch", "occupancy", "lds"}},
{demangled name: (loads in loops, stores in loops, loads, stores)}), from one compile."""
import argparse
import os
import re
import subprocess
import tempfile

_FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
           "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def _flags():
    """The library's compile flags without importing the package (which loads torch)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "remfx_amd", "_lib.py")).read()
    ns = {"os": os, "_HERE": os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "remfx_amd")}
    ns["_ROOT"] = os.path.dirname(ns["_HERE"])
    ns["CSRC"] = os.path.join(ns["_HERE"], "csrc")
    ns["INCLUDE"] = os.path.join(ns["_ROOT"], "include")
    m = re.search(r"^HIPCC_FLAGS = \[.*?\]$", src, re.S | re.M)
    exec(m.group(0), ns)
    return ns["HIPCC_FLAGS"]


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _demangle(names):
    names = list(names)
    if not names:
        return {}
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        except OSError:
            continue
        out = r.stdout.splitlines()
        if r.returncode == 0 and len(out) == len(names):
            return {n: re.sub(r"^void ", "", re.sub(r"\(.*\)$", "", o)) for n, o in zip(names, out)}
    return {n: n for n in names}


def analyse(path, defines=()):
    """One device-only compile to ISA with the resource remarks on: ({name: resources}, {name: scratch op counts})."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        cmd = [_hipcc()] + _flags() + ["-D" + d for d in defines] + \
              ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", path, "-o", asm]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stdout)
        text = open(asm).read().splitlines()
    raw, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = raw.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)", line)
        if m and cur is not None and m.group(1).strip() in _FIELDS:
            try:
                cur[_FIELDS[m.group(1).strip()]] = int(m.group(2))
            except ValueError:
                pass
    funcs, cur = {}, None
    for line in text:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                cur.append(line)
    loops = {}
    for name, body in funcs.items():
        labels, inloop = {}, [False] * len(body)
        for i, line in enumerate(body):
            m = re.match(r"^(\.L\w+):", line)
            if m:
                labels[m.group(1)] = i
            m = re.match(r"^\s+s_c?branch\w*\s+(\.L\w+)", line)
            if m and m.group(1) in labels:                       # a branch back: everything from the label to here is a loop
                for j in range(labels[m.group(1)], i + 1):
                    inloop[j] = True
        cnt = [0, 0, 0, 0]
        for i, line in enumerate(body):
            m = re.match(r"^\s+scratch_(load|store)", line)
            if m:
                st = m.group(1) == "store"
                cnt[2 + st] += 1
                if inloop[i]:
                    cnt[st] += 1
        loops[name] = tuple(cnt)
    names = _demangle(set(raw) | set(loops))
    return {names[k]: v for k, v in raw.items()}, {names[k]: v for k, v in loops.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--filter", default="")
    ap.add_argument("--loops", action="store_true")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    args = ap.parse_args()
    res, loops = analyse(args.file, args.defines)
    hdr = f"{'kernel':<58} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'scratch B':>9} {'occ':>4} {'LDS B':>7}"
    if args.loops:
        hdr += f" {'ld/st in loops':>15} {'ld/st all':>10}"
    print(hdr)
    for name in sorted(res):
        if args.filter not in name:
            continue
        v = res[name]
        line = (f"{name:<58} {v.get('vgprs', -1):>5} {v.get('agprs', -1):>5} {v.get('sgprs', -1):>5} {v.get('scratch', -1):>9} "
                f"{v.get('occupancy', -1):>4} {v.get('lds', -1):>7}")
        if args.loops:
            c = loops.get(name, (0, 0, 0, 0))
            line += f" {str(c[0]) + ' / ' + str(c[1]):>15} {str(c[2]) + ' / ' + str(c[3]):>10}"
        print(line)


if __name__ == "__main__":
    main()
