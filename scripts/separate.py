"""Multi-source separation of one file with Hybrid Demucs: one output file per source name.
    python scripts/separate.py +checkpoint=model.ckpt +audio_input=in.wav +output_dir=stems \\
        +sources=drums,bass,other,vocals +audio_channels=2 +channels=48
Overrides in the `+key=value` style of scripts/remfx_detect.py (a leading `+` is optional); everything but the three paths has a
default (DEFAULTS below).  The file is decoded with datasets.load_wav, resampled to +sample_rate on the device, brought to
+audio_channels channels (a mono file is repeated, a wider file is mixed down to mono first), run through HDemucs.separate --
overlapping clips of +segment_seconds with their channels kept together, cross-faded on the device (remfx_amd/segment.py) -- and
every source is written as <output_dir>/<source>.wav (float32).

The checkpoint is a torch.save'd state_dict of remfx_amd.hdemucs.HDemucs (the keys of torchaudio.models.HDemucs), bare or under
"state_dict", with or without the `model.` / `model.model.` prefixes of the training wrappers; it is loaded strictly.  No pretrained
weights ship with the project: `+checkpoint=random` runs the seeded (+seed) random initialisation, for plumbing and timing only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from remfx_amd.datasets import load_wav, save_wav  # noqa: E402
from remfx_amd.resample import resample  # noqa: E402

DEFAULTS = {"sources": "drums,bass,other,vocals", "audio_channels": 2, "channels": 48, "nfft": 4096, "depth": 6, "sample_rate": 44100,
            "segment_seconds": 10.0, "overlap": 0.25, "segment_batch": 8, "seed": 0}
REQUIRED = ("checkpoint", "audio_input", "output_dir")


def parse(argv):
    opt = dict(DEFAULTS)
    for arg in argv:
        key, eq, value = arg.lstrip("+").partition("=")
        if not eq or key not in DEFAULTS and key not in REQUIRED:
            raise ValueError(f"separate: expected +key=value with key in {sorted(list(DEFAULTS) + list(REQUIRED))}, got {arg!r}")
        opt[key] = type(DEFAULTS[key])(value) if key in DEFAULTS else value
    missing = [k for k in REQUIRED if k not in opt]
    if missing:
        raise ValueError(f"separate: missing {', '.join('+' + k + '=...' for k in missing)}")
    opt["sources"] = [s for s in opt["sources"].split(",") if s]
    if not opt["sources"] or opt["audio_channels"] not in (1, 2) or opt["segment_seconds"] <= 0 or opt["segment_batch"] < 1:
        raise ValueError(f"separate: bad options {opt}")
    return opt


def load_state(path):
    """The HDemucs state_dict inside a checkpoint file, wrapper prefixes stripped."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"checkpoint {path!r} not found (+checkpoint=random runs on random weights)")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    for prefix in ("model.model.", "model."):
        if all(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items()}
            break
    return sd


def fit_channels(audio, channels):
    """(c, T) -> (channels, T)"""
    if audio.shape[0] == channels:
        return audio
    return audio.mean(0, keepdim=True).expand(channels, -1).contiguous()


def main(argv=None):
    opt = parse(list(sys.argv[1:] if argv is None else argv))
    if not torch.cuda.is_available():
        raise RuntimeError("separate needs the GPU: the network has no CPU path")
    from remfx_amd.hdemucs import HDemucs
    device = torch.device("cuda", 0)
    torch.manual_seed(opt["seed"])
    net = HDemucs(sources=opt["sources"], audio_channels=opt["audio_channels"], channels=opt["channels"], nfft=opt["nfft"],
                  depth=opt["depth"])
    if opt["checkpoint"] != "random":
        net.load_state_dict(load_state(opt["checkpoint"]), strict=True)
    net = net.to(device)
    audio, sr = load_wav(opt["audio_input"])                   # (channels, samples) float32
    audio = audio.to(device)
    if sr != opt["sample_rate"]:
        audio = resample(audio, sr, opt["sample_rate"])
    mix = fit_channels(audio, opt["audio_channels"]).unsqueeze(0)
    segment = int(round(opt["segment_seconds"] * opt["sample_rate"]))
    stems = net.separate(mix, segment=segment, overlap=opt["overlap"], batch=opt["segment_batch"])[0]      # (S, channels, T)
    os.makedirs(opt["output_dir"], exist_ok=True)
    paths = []
    for name, stem in zip(opt["sources"], stems):
        paths.append(os.path.join(opt["output_dir"], name + ".wav"))
        print("Saving", paths[-1])
        save_wav(paths[-1], stem.cpu(), opt["sample_rate"])
    return paths


if __name__ == "__main__":
    main()
