"""Device-event timings of the effects added to remfx_amd.effects: each effect at 64 x 262144 mono (the widener:
32 stereo clips = 64 rows), the K-weighting loudness measurement and the compressor for comparison, and the whole
RandomAudioEffectsChannel chain at 16 x 2 x 262144.  Prints one JSON line per case.

    python scripts/perf_fx.py [--reps 20] [--out perf_fx.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from remfx_amd import effects as E  # noqa: E402

SR, B, T = 48000, 64, 262144
HBM = 8.0e12


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    x = (0.3 * torch.randn(B, T, generator=g)).to(dev)
    torch.manual_seed(0)
    np.random.seed(0)
    cases = {}
    eq = E.RandomParametricEQ(SR)
    pe = [eq.draw() for _ in range(B)]
    cases["eq"] = (lambda: eq.render(x, pe), None)
    wd = E.RandomStereoWidener(SR)
    pw = [wd.draw() for _ in range(B // 2) for _ in range(2)]
    cases["widener"] = (lambda: wd.render(x, pw), 2 * 4 * B * T)
    va = E.RandomVolumeAutomation(SR)
    pv = [va.draw(T) for _ in range(B)]
    xv = x.clone()
    cases["volume_automation"] = (lambda: va.render(xv, pv), 2 * 4 * B * T)      # in place: read + write
    ph = E.RandomPedalboardPhaser(SR)
    pp = [ph.draw() for _ in range(B)]
    cases["phaser"] = (lambda: ph.render(x, pp), None)
    lm = E.RandomPedalboardLimiter(SR)
    pl = [lm.draw() for _ in range(B)]
    cases["limiter"] = (lambda: lm.render(x, pl), None)
    cp = E.RandomPedalboardCompressor(SR)
    pc = [cp.draw() for _ in range(B)]
    cases["compressor (existing)"] = (lambda: cp.render(x, pc), None)
    ln = E.LoudnessNormalize(SR)
    cases["loudness measure (existing)"] = (lambda: ln.measure(x), None)
    cases["loudness measure joint, 32 x 2"] = (lambda: ln.measure_joint(x.view(B // 2, 2, T)), None)
    rv = E.RandomPedalboardReverb(SR)
    pr = [rv.draw() for _ in range(B)]
    cases["reverb (existing)"] = (lambda: rv.render(x, pr), None)                # 1 bank per clip
    sx = E.RandomSoxReverb(SR)
    ps = [sx.draw() for _ in range(B)]
    cases["sox_reverb, 64 x 1 (128 banks)"] = (lambda: sx.render(x.view(B, 1, T), ps), None)
    cases["sox_reverb, 32 x 2 (128 banks)"] = (lambda: sx.render(x.view(B // 2, 2, T), ps[:B // 2]), None)
    rows = []
    for name, (fn, nbytes) in cases.items():
        ms = _time(fn, a.reps)
        r = dict(case=name, shape=[B, T], ms=round(ms, 4))
        if nbytes:
            r["TB_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
            r["frac_hbm_8TBs"] = round(nbytes / (ms * 1e-3) / HBM, 3)
        print(json.dumps(r), flush=True)
        rows.append(r)
    chain = E.RandomAudioEffectsChannel(SR)
    xc = (0.3 * torch.randn(16, 2, T, generator=g)).to(dev)
    torch.manual_seed(1)
    np.random.seed(1)
    ms = _time(lambda: chain(xc), max(2, a.reps // 4))
    r = dict(case="RandomAudioEffectsChannel (host draws included)", shape=[16, 2, T], ms=round(ms, 3))
    print(json.dumps(r), flush=True)
    rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
