"""Long files through the five-model detect-and-remove chain (cfg/exp/remfx_detect.yaml at random init,
inference_use_all_effect_models=True so the work does not depend on the detector): the whole file as ONE clip
(RemFXChainInference.forward, what scripts/remfx_detect.py does without `+segment_seconds`) against overlapping 262144-sample clips
in batches (RemFXChainInference.sample_long).  Synthetic 48 kHz files of 1, 4 and 10 minutes; per length wall time
per file (host clock around work that ends in a device synchronise) and torch.cuda.max_memory_allocated of both paths, measured
alternately in one process after one warm-up run of each; then the two segment kernels alone (device events) at the longest size with their share
of the 8 TB/s HBM roof (bytes = what the algorithm has to move: file + clips, once each).

    RFX_ALLOW_RANDOM_INIT=1 python scripts/perf_segment.py [--minutes 1 4 10] [--reps 3] [--whole-limit-s 120]

A whole-file run that fails (out of memory) or takes longer than --whole-limit-s is reported and not repeated.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from remfx_amd import config as rcfg, segment  # noqa: E402
from scripts.chain_inference import build  # noqa: E402

SR, L, OVERLAP, BATCH = 48000, 262144, 0.25, 64
HBM = 8.0e12


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 30


def fmt(ts):
    return f"min {min(ts):8.3f}  median {statistics.median(ts):8.3f}  max {max(ts):8.3f} s" if ts else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[1, 4, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--whole-limit-s", type=float, default=120.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = rcfg.compose(os.environ.get("REMFX_CFG_DIR", os.path.join(ROOT, "cfg")), "config.yaml",
                       ["+exp=remfx_detect", "inference_use_all_effect_models=True"])
    model = build(cfg, dev)
    print(f"chain: {list(model.effect_order)}; segments of {L} samples, overlap {OVERLAP}, {BATCH} clips per batch", flush=True)
    x = None
    for minutes in a.minutes:
        T = int(minutes * 60 * SR)
        x = (torch.randn(1, 1, T, generator=torch.Generator().manual_seed(int(minutes * 60))) * 0.1).to(dev)
        plan = segment.SegmentPlan(T, L, segment.overlap_samples(L, OVERLAP))

        def whole():
            model((x, x, None, None), 0)               # detector, chain and the loss forward() ends with: the script's whole-file path

        def segmented():
            model.sample_long(x, segment=L, overlap=OVERLAP, batch=BATCH, detect="segment")
        print(f"{minutes:g} min = {T} samples, {plan.n_segments} segments", flush=True)
        runs = {"whole": [], "segmented": []}
        mem = {"whole": 0.0, "segmented": 0.0}
        whole_ok = True
        for rep in range(a.reps + 1):                                  # rep 0 warms both paths up at this size
            for name, fn in (("whole", whole), ("segmented", segmented)):
                if name == "whole" and not whole_ok:
                    continue
                try:
                    dt, gib = timed(fn)
                except torch.cuda.OutOfMemoryError as e:
                    print(f"  {name}: out of memory ({str(e).splitlines()[0][:120]})", flush=True)
                    whole_ok = whole_ok and name != "whole"
                    torch.cuda.empty_cache()
                    continue
                print(f"  rep {rep} {name:10s} {dt:9.3f} s  peak {gib:7.2f} GiB{'  (warm-up)' if rep == 0 else ''}", flush=True)
                if rep:
                    runs[name].append(dt)
                mem[name] = max(mem[name], gib)
                if name == "whole" and dt > a.whole_limit_s:
                    print(f"  whole-file run over {a.whole_limit_s:g} s: kept as the one measurement, not repeated", flush=True)
                    runs[name] = runs[name] or [dt]
                    whole_ok = False
        for name in runs:
            print(f"  {name:10s} {fmt(runs[name])}  peak {mem[name]:7.2f} GiB")
        if runs["whole"] and runs["segmented"]:
            print(f"  whole / segmented (medians): {statistics.median(runs['whole']) / statistics.median(runs['segmented']):.2f}")
    # the two kernels alone, at the last (longest) size: as it is (a multiple of 4 samples takes the 16-byte path) and one sample
    # shorter (the dword path)
    for xs in (x, x[..., :-1].contiguous()):
        T = xs.shape[-1]
        plan = segment.SegmentPlan(T, L, segment.overlap_samples(L, OVERLAP))
        clips = segment.split(xs, plan)
        nbytes = 4 * (T + clips.numel())
        for name, fn in (("rfx_segment_split", lambda: segment.split(xs, plan)),
                         ("rfx_segment_merge", lambda: segment.merge(clips, plan))):
            for _ in range(5):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
            med = us[len(us) // 2]
            print(f"{name}: T = {T} (T % 4 = {T % 4}), {plan.n_segments} clips, {nbytes / 1e6:.1f} MB: min {us[0]:.1f}  median {med:.1f}  "
                  f"max {us[-1]:.1f} us = {nbytes / (med * 1e-6) / 1e12:.2f} TB/s, {nbytes / (med * 1e-6) / HBM:.2f} of the HBM roof")

if __name__ == "__main__":
    main()
