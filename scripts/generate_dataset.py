"""Render the datasets of an experiment and exit, same command line as the reference scripts/generate_dataset.py:
    python scripts/generate_dataset.py +exp=5-5_full
Instantiating the datamodule is what renders: every EffectDataset(render_files=True) with a corpus under DATASET_ROOT writes
its chunks under ``render_root`` (in batches on the device with ``parallel: true``).  Without a corpus the datasets warn and
serve white noise, and nothing is written."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from remfx_amd import config as rcfg  # noqa: E402


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    cfg_dir = os.environ.get("REMFX_CFG_DIR", os.path.join(ROOT, "cfg"))
    cfg = rcfg.compose(cfg_dir, "config.yaml", argv)
    if cfg.get("seed"):                                     # pl.seed_everything: the chunk choice uses all three generators
        random.seed(cfg["seed"])
        np.random.seed(cfg["seed"])
        torch.manual_seed(cfg["seed"])
    return rcfg.instantiate(cfg["datamodule"])


if __name__ == "__main__":
    main()
