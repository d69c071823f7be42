"""Single-file detect-and-remove, same command line as the reference scripts/remfx_detect.py:13-61 (`remfx_detect.sh`):
    python scripts/remfx_detect.py +exp=remfx_detect +audio_input=in.wav +output_path=out.wav
No Trainer: the five effect-specific removal models and the Cnn14 detector are instantiated from cfg.ckpts /
cfg.classifier, their checkpoints loaded strictly, the file is decoded, resampled to cfg.sample_rate ON THE DEVICE
(remfx_amd.resample: the polyphase filter bank of torchaudio.transforms.Resample as one strided gather-GEMM), mixed to
mono, run through RemFXChainInference.forward(batch, 0, verbose=True) at its full length (any length: the attention kernels stream
the keys beyond 256 frames), and written as a float32 WAV (torchaudio.save's default for float tensors).

Long files: `+segment_seconds=<float>` cuts the file into overlapping clips of that length instead (5.46 s = the 262144 samples the
networks were trained on at 48 kHz), runs them in batches and cross-fades the results (RemFXChainInference.sample_long,
remfx_amd/segment.py): the cost grows linearly with the length and the detected effects may change along the file.  With it,
`+overlap=<fraction, default 0.25>`, `+segment_batch=<clips per launch, default 64>`, `+detect=segment|file` (one label set per
clip, or the clips' averaged probabilities thresholded once) and `+keep_channels=true` (every channel is processed on its own and
the output keeps the input's channel count instead of the mono mix).  Without `+segment_seconds` nothing changes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from remfx_amd import config as rcfg  # noqa: E402
from remfx_amd.datasets import load_wav, save_wav  # noqa: E402
from remfx_amd.resample import resample  # noqa: E402
from scripts.chain_inference import build  # noqa: E402


SEGMENT_DEFAULTS = {"overlap": 0.25, "segment_batch": 64, "detect": "segment", "keep_channels": False}


def segment_options(cfg):
    """The long-file overrides of a composed config, or None for the whole-file path (no `+segment_seconds`).  Their defaults live
    here: the cfg/ tree mirrors the reference's."""
    if cfg.get("segment_seconds") is None:
        extra = [k for k in SEGMENT_DEFAULTS if k in cfg]
        if extra:
            raise ValueError(f"{', '.join('+' + k for k in extra)} need +segment_seconds=<seconds>")
        return None
    opt = {k: cfg.get(k, v) for k, v in SEGMENT_DEFAULTS.items()}
    opt["segment"] = int(round(float(cfg["segment_seconds"]) * cfg["sample_rate"]))
    opt["overlap"], opt["segment_batch"] = float(opt["overlap"]), int(opt["segment_batch"])
    if opt["segment"] < 1 or not 0.0 <= opt["overlap"] < 1.0 or opt["segment_batch"] < 1 or opt["detect"] not in ("segment", "file"):
        raise ValueError(f"bad long-file options: {opt}")
    return opt


def label_timeline(seg_labels, starts, segment, sample_rate, effects, total):
    """One line per run of equal clip labels of every row: start, end (seconds), effects.  A run ends where the next one starts."""
    lines = []
    for r, rows in enumerate(seg_labels.tolist()):
        i = 0
        while i < len(rows):
            j = i
            while j + 1 < len(rows) and rows[j + 1] == rows[i]:
                j += 1
            end = starts[j + 1] if j + 1 < len(rows) else min(starts[j] + segment, total)
            names = [e for e, on in zip(effects, rows[i]) if on == 1.0] or ["none"]
            lines.append(f"row {r}: {starts[i] / sample_rate:8.2f} s - {end / sample_rate:8.2f} s  {', '.join(names)}")
            i = j + 1
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    cfg = rcfg.compose(os.environ.get("REMFX_CFG_DIR", os.path.join(ROOT, "cfg")), "config.yaml", argv)
    seg = segment_options(cfg)
    if not torch.cuda.is_available():
        raise RuntimeError("remfx_detect needs the GPU: the removal networks have no CPU path")
    device = torch.device("cuda", 0)
    print("Loading models...")
    inference_model = build(cfg, device)                       # remfx_detect.py:15-41
    audio_file = cfg["audio_input"]
    print("Loading", audio_file)
    audio, sr = load_wav(audio_file)                           # (channels, samples) float32, remfx_detect.py:45
    audio = audio.to(device)
    if sr != cfg["sample_rate"]:
        audio = resample(audio, sr, cfg["sample_rate"])                             # :47
    if seg is not None and seg["keep_channels"]:
        audio = audio.unsqueeze(0)                             # (1, channels, T): every channel a row of its own
    else:
        audio = audio.mean(0, keepdim=True).unsqueeze(0)       # mono + batch dim, :49-51
    if seg is None:
        batch = [audio, audio, None, None]
        _, y = inference_model(batch, 0, verbose=True)         # :55
    else:
        from remfx_amd.models import ALL_EFFECT_NAMES
        y, seg_labels = inference_model.sample_long(audio, segment=seg["segment"], overlap=seg["overlap"], batch=seg["segment_batch"],
                                                    detect=seg["detect"], verbose=True)
        plan = inference_model.last_plan
        print(f"Label timeline ({plan.n_segments} segments of {seg['segment']} samples, hop {plan.hop}):")
        for line in label_timeline(seg_labels.cpu(), plan.starts.tolist(), seg["segment"], cfg["sample_rate"], ALL_EFFECT_NAMES,
                                   plan.T):
            print(line)
    output_path = cfg["output_path"] if "output_path" in cfg else "./output.wav"
    print("Saving output to", output_path)
    save_wav(output_path, y[0].cpu(), cfg["sample_rate"])
    return output_path


if __name__ == "__main__":
    main()
