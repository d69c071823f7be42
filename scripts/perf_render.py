"""Dataset rendering, per item against per batch: wall clock of
  (a) the per-item loop: `process_effects` on one (1, T) clip after the other (DynamicEffectDataset.__getitem__, parallel=False),
  (b) `process_effects_batch` over the same B clips (rounds; each round's normalisation is one rfx_fx_normalize_rows call that
      writes through a row table),
  (c) the same rounds with the normalisation done by torch calls (measure, scale, index_copy_) for comparison,
for the dynamic configuration (nothing kept; distortion, compressor, reverb, chorus, delay removed in that order, 0 to 5 of
them) at B = 32, the same with the order shuffled as cfg/exp/5-5_full_cls_dynamic.yaml sets it, and the stock configuration of
cfg/config.yaml at B = 64.  White-noise sources at about -20 dB: no disk involved.  Every timed batch draws fresh plans (the draws
are host time of both paths) and ends with a device synchronisation, so host time counts.

    python scripts/perf_render.py [--T 262144] [--warmup 2] [--batches 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from remfx_amd import datasets as D, effects as E  # noqa: E402

SR = 48000
CONFIGS = {
    "dynamic B=32": (32, dict(effects_to_keep=[], effects_to_remove=["distortion", "compressor", "reverb", "chorus", "delay"],
                              num_kept_effects=[0, 0], num_removed_effects=[0, 5], shuffle_kept_effects=True,
                              shuffle_removed_effects=False)),
    "dynamic shuffled B=32": (32, dict(effects_to_keep=[], effects_to_remove=["distortion", "compressor", "reverb", "chorus", "delay"],
                                       num_kept_effects=[0, 0], num_removed_effects=[0, 5], shuffle_kept_effects=True,
                                       shuffle_removed_effects=True)),
    "stock B=64": (64, dict(effects_to_keep=["reverb", "chorus", "delay"], effects_to_remove=["compressor", "distortion"],
                            num_kept_effects=[2, 2], num_removed_effects=[2, 2], shuffle_kept_effects=True,
                            shuffle_removed_effects=False)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fx = {"reverb": E.RandomPedalboardReverb(SR), "chorus": E.RandomPedalboardChorus(SR), "delay": E.RandomPedalboardDelay(SR),
          "distortion": E.RandomPedalboardDistortion(SR), "compressor": E.RandomPedalboardCompressor(SR)}
    norm = E.LoudnessNormalize(SR, target_lufs_db=-20)
    for label, (B, kw) in CONFIGS.items():
        x = (torch.randn(B, 1, a.T, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
        recipe = D.EffectRecipe(fx, **kw)

        def per_item():
            return [recipe.process(x[b], norm) for b in range(B)]

        def batched(row_tables):
            return D.process_effects_batch(x, [recipe.plan() for _ in range(B)], fx, norm, row_tables=row_tables)

        print(f"{label}, T = {a.T}: ms per batch over {a.batches} batches after {a.warmup} warm-up batches")
        med = {}
        for name, fn in (("(a) per-item loop", per_item), ("(b) batch", lambda: batched(True)),
                         ("(c) batch, torch scatter", lambda: batched(False))):
            torch.manual_seed(7)
            np.random.seed(7)
            times = []
            for i in range(a.warmup + a.batches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[a.warmup:]
            med[name] = statistics.median(times)
            print(f"  {name:28s} min {min(times):9.2f}   median {med[name]:9.2f}   max {max(times):9.2f}")
        print(f"  (a) / (b) median {med['(a) per-item loop'] / med['(b) batch']:.2f}   "
              f"(c) / (b) median {med['(c) batch, torch scatter'] / med['(b) batch']:.3f}")


if __name__ == "__main__":
    main()
