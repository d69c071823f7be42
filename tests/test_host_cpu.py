"""CPU: host-side logic -- config composer (Hydra subset), target aliasing / instantiate, the C-ABI
library exports, synthetic datamodule, flat parameter views, and the N>1 gradient exchange over
gloo (world_size 2)."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from remfx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "remfx_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(rfx_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = ctypes.CDLL(_lib.build())                      # hipcc cross-compiles without a GPU
    for name in declared:
        assert hasattr(L, name), name
    assert L.rfx_abi_version() == 1
    from remfx_amd import convplan
    for M in (1, 8, 9, 32, 45, 48, 90, 96, 128, 135, 192, 256, 384, 1536, 3072):
        for K in (12, 64, 65, 1792):
            assert L.rfx_gemm_pick_r(M, K) == convplan.pick_r(M, K), (M, K)


def test_ops_refuse_cpu_tensors():
    from remfx_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.conv1d(torch.randn(1, 2, 16), torch.randn(3, 2, 3))


def _write_cfg(tmp_path):
    (tmp_path / "model").mkdir(); (tmp_path / "exp").mkdir(); (tmp_path / "logger").mkdir()
    (tmp_path / "config.yaml").write_text(textwrap.dedent("""
        defaults:
          - _self_
          - model: null
          - logger: csv
        seed: 7
        sample_rate: 48000
        logs_dir: "./logs"
        root: ${oc.env:RFX_TEST_ROOT,/data}
        stamp: ${now:%Y}
        accelerator: null
        trainer:
          accelerator: ${accelerator}
          max_steps: 10
        datamodule:
          train_batch_size: 16
          dataset: {rate: "${sample_rate}", root: "${root}"}
    """))
    (tmp_path / "model" / "a.yaml").write_text("# @package _global_\nmodel:\n  name: a\n  sr: ${sample_rate}\n")
    (tmp_path / "model" / "b.yaml").write_text("# @package _global_\nmodel:\n  name: b\nnet: ${model}\n")
    (tmp_path / "logger" / "csv.yaml").write_text("# @package _global_\nlogger:\n  dir: ${logs_dir}\n")
    (tmp_path / "exp" / "e1.yaml").write_text(textwrap.dedent("""
        # @package _global_
        defaults:
          - override /model: a
        accelerator: "gpu"
        datamodule:
          train_batch_size: 4
    """))
    return str(tmp_path)


def test_config_composer(tmp_path):
    from remfx_amd import config
    d = _write_cfg(tmp_path)
    c = config.compose(d, "config.yaml", [])
    assert "model" not in c and c["logger"] == {"dir": "./logs"} and c["trainer"]["accelerator"] is None
    assert c["root"] == "/data" and len(str(c["stamp"])) == 4
    c = config.compose(d, "config.yaml", ["+exp=e1"])
    assert c["model"] == {"name": "a", "sr": 48000} and c["trainer"]["accelerator"] == "gpu"
    assert c["datamodule"]["train_batch_size"] == 4 and c["datamodule"]["dataset"] == {"rate": 48000, "root": "/data"}
    c = config.compose(d, "config.yaml", ["+exp=e1", "model=b", "datamodule.train_batch_size=64",
                                          "+new.key=[1,2]", "trainer.max_steps=3", "accelerator=null"])
    assert c["model"] == {"name": "b"} and c["net"] == {"name": "b"}          # node interpolation
    assert c["datamodule"]["train_batch_size"] == 64 and c["new"] == {"key": [1, 2]}
    assert c["trainer"] == {"accelerator": None, "max_steps": 3}
    assert config._yaml("lr: 1e-4")["lr"] == 1e-4 and config._parse_value("3e-5") == 3e-5
    with pytest.raises(KeyError):
        config.compose(d, "config.yaml", ["nope.key=1"])
    os.environ["RFX_TEST_ROOT"] = "/x"
    try:
        assert config.compose(d, "config.yaml", [])["root"] == "/x"
    finally:
        del os.environ["RFX_TEST_ROOT"]


def test_repo_cfg_instantiates_reference_targets():
    """cfg/model/*.yaml use the reference's _target_ strings (remfx.models.RemFX ...)."""
    from remfx_amd import config, models
    c = config.compose(os.path.join(ROOT, "cfg"), "config.yaml", ["+exp=reverb", "model=tcn", "datamodule.train_batch_size=2",
                                                                   "datamodule.train_dataset.total_chunks=4", "datamodule.num_workers=0",
                                                                   "model.network.nblocks=2", "model.network.channel_width=8"])
    model = config.instantiate(c["model"])
    assert isinstance(model, models.RemFX) and isinstance(model.model, models.TCNModel)
    assert list(model.state_dict())[0] == "model.model.process_blocks.0.conv1.weight"
    dm = config.instantiate(c["datamodule"])
    x, y, dry, wet = next(iter(dm.train_dataloader()))
    assert x.shape == (2, 1, 262144) and y.shape == x.shape and dry.shape == (2, 5) and wet.shape == (2, 5)
    c = config.compose(os.path.join(ROOT, "cfg"), "config.yaml", ["+exp=5-5_full_cls"])
    cls = config.instantiate(c["model"])
    assert isinstance(cls, models.FXClassifier) and sum(p.numel() for p in cls.network.parameters()) == 79684165
    import remfx.models                       # alias package for `from remfx.models import ...`
    assert remfx.models.RemFXChainInference is models.RemFXChainInference


def test_flat_params_views():
    from remfx_amd.optim import FlatParams
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    ref = [p.detach().clone() for p in net.parameters()]
    flat = FlatParams(list(net.parameters()), allow_cpu=True)
    for p, r, o in zip(net.parameters(), ref, flat.offsets):
        assert torch.equal(p, r) and o % 4 == 0 and p.data_ptr() == flat.data.data_ptr() + 4 * o
    net(torch.randn(4, 5)).sum().backward()
    assert flat.grad.abs().sum() > 0           # autograd accumulated straight into the flat buffer
    flat.zero_grad()
    assert flat.grad.abs().sum() == 0 and all(p.grad.abs().sum() == 0 for p in net.parameters())


WORKER = """
import os, sys, torch
sys.path.insert(0, {root!r})
import torch.distributed as dist
from remfx_amd import ddp
from remfx_amd.optim import FlatParams
rank, local, world = ddp.init_from_env(backend="gloo")
assert world == 2
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 4), torch.nn.Linear(4, 1))
flat = FlatParams(list(net.parameters()), allow_cpu=True)
flat.data += rank                     # replicas differ until the broadcast
ddp.broadcast_parameters(flat.data)
sync = ddp.GradSync(flat, bucket_mb=1e-4, overlap=bool(int(os.environ["OVERLAP"])))   # several tiny buckets
assert len(sync.buckets) >= 2
g = torch.Generator().manual_seed(100 + rank)
x = torch.randn(8, 6, generator=g)
for step in range(2):
    flat.zero_grad()
    net(x).pow(2).mean().backward()
    pre = sync.finish()
    assert pre == 0.5
# reference: average of both ranks' gradients computed locally
refs = []
for r in range(2):
    torch.manual_seed(0)
    n2 = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 4), torch.nn.Linear(4, 1))
    xr = torch.randn(8, 6, generator=torch.Generator().manual_seed(100 + r))
    n2(xr).pow(2).mean().backward()
    refs.append(torch.cat([p.grad.reshape(-1) for p in n2.parameters()]))
want = (refs[0] + refs[1]) / 2
got = torch.cat([p.grad.reshape(-1) for p in net.parameters()]) * pre
assert torch.allclose(got, want, atol=1e-6), (got - want).abs().max()
m = ddp.all_reduce_mean_scalar(torch.tensor(float(rank)))
assert abs(float(m) - 0.5) < 1e-6
if sync.overlap:
    # the gradient-sink route (GPU: kernels write parameter gradients in place, once per USE of the parameter), driven by hand:
    # a step that writes a parameter MORE often than the calibration step did.  Before its bucket launched -> the bucket is held
    # back until finish() (correct result); after -> finish() must refuse the step (the extra write is rank-local).
    n = len(flat.params)
    flat.zero_grad()
    sync.expected, sync.hooked, sync._seen = [1] * n, [False] * n, [0] * n
    last = sync.bucket_of[n - 1]
    first_in_last = min(i for i in range(n) if sync.bucket_of[i] == last)
    sync._sink_write(first_in_last); sync._sink_write(first_in_last)        # one write too many, bucket not yet complete
    for i in range(n - 1, -1, -1):
        if i != first_in_last:
            sync._sink_write(i)
    assert sync.buckets[last].get("hold") and not sync.buckets[last].get("launched")
    assert sync.finish() == 0.5 and sync.expected is None                   # reduced at finish(), counts re-learned next step
    sync.expected, sync.hooked, sync._seen = [1] * n, [False] * n, [0] * n
    for i in range(n - 1, -1, -1):
        sync._sink_write(i)
    assert all(b.get("launched") for b in sync.buckets)
    sync._sink_write(0)                                                     # lands behind the queued all-reduce
    try:
        sync.finish()
        raise SystemExit("late write was not refused")
    except RuntimeError as e:
        assert "after its bucket" in str(e)
dist.barrier()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("overlap", [0, 1])
def test_grad_sync_world2_gloo(tmp_path, overlap):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    env = dict(os.environ, OVERLAP=str(overlap), MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(29511 + overlap), str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2


# ---- the reference's own configs (tests/golden/cfg_composed.json, made by scripts/gen_cfg_fixtures.py) -------------
def _composed():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "cfg_composed.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["config1_umx", "config2_tcn", "config3_demucs_bf16", "config4_dcunet",
                                  "config5_remfx_detect", "cls_5-5_full_cls", "cls_mixup", "cls_16k", "remfx_all",
                                  "chain_inference_aug"])
def test_reference_configs_instantiate(name, recwarn):
    """Every node the reference's entry points instantiate (scripts/train.py:15-44, chain_inference.py:21-32) builds from
    the reference's OWN composed config: datamodule (EffectDataset x3 with the effect objects of cfg/effects/all.yaml),
    model, trainer, logger, and for the chain configs the classifier and the per-effect removal models."""
    from remfx_amd import config, datasets, effects, models
    from remfx_amd.classifier import Cnn14
    cfg = _composed()[name]["cfg"]
    dm = config.instantiate(cfg["datamodule"])
    assert isinstance(dm, datasets.EffectDatamodule)
    for ds in (dm.train_dataset, dm.val_dataset, dm.test_dataset):
        assert isinstance(ds, datasets.EffectDataset) and ds.synthetic is not None     # DATASET_ROOT unset: white noise
        assert all(type(e) in effects.Pedalboard_Effects for e in ds.effects.values()) and len(ds.effects) == 5
    x, y, dry, wet = dm.train_dataset[0]
    assert x.shape == (1, cfg["chunk_size"]) and y.shape == x.shape and dry.shape == (5,) and wet.shape == (5,)
    model = config.instantiate(cfg["model"])
    assert isinstance(model, (models.RemFX, models.FXClassifier))
    trainer = config.instantiate(cfg["trainer"], callbacks=[], logger=config.instantiate(cfg["logger"]))
    assert trainer.max_steps == cfg["trainer"]["max_steps"]
    if name == "config3_demucs_bf16":
        assert trainer.gemm_mode == "bf16" and cfg["trainer"]["devices"] == 8
    if name.startswith("cls_"):
        assert isinstance(model.network, Cnn14)
        assert model.network.specaugment == cfg["model"]["network"].get("specaugment", False)
    if "callbacks" in cfg:                                 # observability: skipped, not an error
        assert all(config.instantiate(cb) is None for cb in cfg["callbacks"].values() if "_target_" in cb)
    if "ckpts" in cfg:
        if "classifier" in cfg:                            # oracle-label chains (chain_inference_aug) have none
            cls = config.instantiate(cfg["classifier"])
            assert isinstance(cls.network, Cnn14)
            if name == "config5_remfx_detect":
                assert cls.network.specaugment is True     # cfg/exp/remfx_detect.yaml:60: must construct
        nets = {k: config.instantiate(v["model"]) for k, v in cfg["ckpts"].items()}
        assert set(nets) <= set(models.ALL_EFFECT_NAMES) and len(nets) >= 1
        assert list(cfg["inference_effects_ordering"]) == [n for n in cfg["inference_effects_ordering"] if n in models.ALL_EFFECT_NAMES]


def test_dptnet_and_hear_configs_instantiate():
    """cfg/model/dptnet.yaml builds the DPTNet removal wrapper with asteroid's state_dict names (83 tensors, 2 851 393 parameters
    -- the oracle restatement's count); cfg/model/cls_vggish.yaml needs the pretrained HEAR package, absent here: ImportError,
    as upstream's module import would fail."""
    from oracle import ref_dptnet
    from remfx_amd import config, models
    cfg = _composed()["dptnet"]["cfg"]
    model = config.instantiate(cfg["model"])
    assert isinstance(model.model, models.DPTNetModel)
    net = model.model.model
    kw = {k: v for k, v in cfg["model"]["network"].items() if k not in ("_target_", "num_bins")}
    ref = ref_dptnet.DPTNet(**{**kw, "sample_rate": 48000})
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys()) and len(ref.state_dict()) == 83
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters()) == 2851393
    net.load_state_dict(ref.state_dict(), strict=True)
    with pytest.raises(ImportError, match="hearbaseline"):
        config.instantiate(_composed()["cls_vggish"]["cfg"]["model"])


def test_dynamic_effect_config_instantiates():
    """cfg/exp/5-5_full_cls_dynamic.yaml (on-the-fly augmentation): the train split is a DynamicEffectDataset holding the
    five effect objects and a -20 LUFS normaliser (datasets.py:205-262); val / test stay EffectDatasets."""
    from remfx_amd import config, datasets, effects
    cfg = _composed()["cls_dynamic"]["cfg"]
    with pytest.warns(UserWarning):
        dm = config.instantiate(cfg["datamodule"])
    tr = dm.train_dataset
    assert isinstance(tr, datasets.DynamicEffectDataset) and len(tr) == 8000 and tr.renders_on_device
    assert isinstance(tr.normalize, effects.LoudnessNormalize) and tr.normalize.target_lufs_db == -20
    assert tr.effects_to_remove == ["distortion", "compressor", "reverb", "chorus", "delay"] and tr.num_removed_effects == [0, 5]
    assert all(type(e) in effects.Pedalboard_Effects for e in tr.effects.values()) and tr.shuffle_removed_effects is True
    assert isinstance(dm.val_dataset, datasets.EffectDataset) and isinstance(dm.test_dataset, datasets.EffectDataset)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="renders on the GPU"):
            tr[0]


def _cfg_digest(cfg):
    import hashlib
    import json
    import re
    plain = lambda o: ({str(k): plain(v) for k, v in o.items()} if isinstance(o, dict) else
                       [plain(v) for v in o] if isinstance(o, (list, tuple)) else o)
    text = re.sub(r"\d{4}-\d\d-\d\d-\d\d-\d\d-\d\d", "<now>", json.dumps(plain(cfg), sort_keys=True))
    return hashlib.sha256(text.encode()).hexdigest()


def test_own_cfg_tree_matches_reference_composition(monkeypatch):
    """The repo's OWN cfg/ (written by scripts/write_cfg_tree.py) composes every command line of BASELINE.md section 5 -- incl.
    config 4's `+exp=5-5_full model=dcunet` -- to exactly the dictionary the reference's tree gives (tests/golden/cfg_composed.json,
    recorded from /root/reference/cfg), and every experiment / model / logger file of the tree to the recorded digest
    (tests/golden/cfg_digests.json): no REMFX_CFG_DIR needed."""
    import json
    from remfx_amd import config
    for v in ("DATASET_ROOT", "WANDB_PROJECT", "WANDB_ENTITY"):
        monkeypatch.delenv(v, raising=False)
    own = os.path.join(ROOT, "cfg")
    for name, rec in _composed().items():
        assert _cfg_digest(config.compose(own, "config.yaml", rec["argv"])) == _cfg_digest(rec["cfg"]), name
    with open(os.path.join(ROOT, "tests", "golden", "cfg_digests.json")) as f:
        digests = json.load(f)
    assert len(digests) == 45
    for argv, d in digests.items():
        assert _cfg_digest(config.compose(own, "config.yaml", argv.split())) == d, argv
    n_files = sum(len(fs) for _, _, fs in os.walk(own))
    assert n_files == 48                                   # config + 28 experiments + 16 models + effects + 2 loggers


def test_bench_final_line_is_compact(tmp_path, monkeypatch, capsys):
    """bench.py's last stdout line is what the driver parses: one JSON object under 4 KB with the contract's keys, whatever the
    size of the full record (which goes to a file).  Round 5's 24 KB line was unparseable for the driver."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    spec.loader.exec_module(bench)
    monkeypatch.setenv("RFX_BENCH_FULL_DIR", str(tmp_path))
    fat = [{"kernel": f"cl_conv_kernel<{i}, 3, 2, 2, 3, 1, 2, 4, true>", "frac": 0.1, "pad": "x" * 300} for i in range(80)]
    out = {"metric": "audio-seconds/sec fwd+bwd (whole job)", "value": 3500.0, "unit": "audio-seconds/sec", "n_gpus": 1, "steps": 20,
           "warmup": 5, "ms_per_step": 99.0, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "bf16 (fp32 accumulate)", "data": "synthetic",
           "config": {"workload": "Hybrid Demucs", "clips_per_gpu": 64, "global_batch": 64, "parallelism": "dp1", "junk": fat},
           "roofline": {"bound": "mfma", "kernel": "k", "achieved": 1.0, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.2, "frac_mfma": 0.2,
                        "frac_hbm": 0.1, "traffic": 1, "algorithmic_bytes_per_launch": 1, "avg_launch_us": 1.0, "launches_per_step": 1.0,
                        "by_kernel": fat},
           "step_roofline": bench.step_roofline("demucs", "bf16", 64, 0.099, 2500.0, 337e9),
           "cpu_baseline": {"value": 4.0, "unit": "audio-seconds/sec", "cores": 32, "kind": "port", "sample": "s" * 1000},
           "phases_s": {"timed": 2.0}}
    bench.emit(out, "unit")
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert len(line) < 4096
    rec = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "step_roofline"):
        assert k in rec, k
    assert "by_kernel" not in rec["roofline"] and rec["config"]["workload"] == "Hybrid Demucs"
    sr = rec["step_roofline"]
    assert abs(sr["frac_mfma"] - 3 * 117.33e9 * 64 / 0.099 / 2.5e15) < 1e-3 and sr["traffic_ratio"] > 5
    full = json.load(open(os.path.join(tmp_path, "bench_full_unit.json")))
    assert len(full["roofline"]["by_kernel"]) == 80


def test_effect_label_order_and_alias():
    import remfx.effects as alias
    from remfx_amd import effects, models
    assert [c.__name__ for c in effects.Pedalboard_Effects] == models.ALL_EFFECT_NAMES      # effects.py:699-707
    assert alias.RandomPedalboardChorus is effects.RandomPedalboardChorus
    fx = effects.RandomPedalboardDelay(48000, min_delay_seconds=0.1, max_delay_sconds=1.0)
    torch.manual_seed(0)
    p = fx.draw()
    assert 0.1 <= p["delay_seconds"] <= 1.0 and list(p) == ["delay_seconds", "feedback", "mix"]       # the reference's draw order
    torch.manual_seed(7)
    u = [float(torch.rand(1)) for _ in range(4)]
    torch.manual_seed(7)
    q = effects.RandomPedalboardCompressor(48000).draw()          # effects.py:323-326: threshold, ratio, attack, release
    assert abs(q["threshold_db"] - (u[0] * 36.0 - 42.0)) < 1e-4 and abs(q["release_ms"] - (u[3] * 240.0 + 10.0)) < 1e-3
    with pytest.raises(TypeError):
        effects.RandomPedalboardReverb(48000, min_nonsense=1.0)
    with pytest.raises(ValueError, match="no CPU path"):          # rendering runs on the GPU only
        fx(torch.zeros(1, 8))


def test_effect_dataset_reads_rendered_layout(tmp_path):
    """{render_root}/processed/{effects_string}/{mode}/{idx}/{input.wav,target.wav,dry_effects.pt,wet_effects.pt}
    (reference datasets.py:370-380, 445-468)."""
    from remfx_amd import datasets, effects
    fx = {"distortion": effects.RandomPedalboardDistortion(48000), "reverb": effects.RandomPedalboardReverb(48000)}
    kw = dict(root=None, sample_rate=48000, chunk_size=4096, total_chunks=99, effect_modules=fx, effects_to_keep=["reverb"],
              effects_to_remove=["distortion"], num_kept_effects=[0, 1], num_removed_effects=[1, 1], render_files=False,
              render_root=str(tmp_path), mode="val")
    proc = tmp_path / "processed" / "reverb___distortion___0_1___1_1" / "val"
    g = torch.Generator().manual_seed(3)
    clips = []
    for i in range(3):
        d = proc / str(i)
        d.mkdir(parents=True)
        wet, dry = torch.randn(1, 4096, generator=g) * 0.1, torch.randn(1, 4096, generator=g) * 0.1
        datasets.save_wav(d / "input.wav", wet, 48000)
        datasets.save_wav(d / "target.wav", dry, 48000)
        lab = torch.zeros(5); lab[3] = 1.0
        torch.save(torch.zeros(5), d / "dry_effects.pt"); torch.save(lab, d / "wet_effects.pt")
        clips.append((wet, dry, lab))
    ds = datasets.EffectDataset(**kw)
    assert len(ds) == 3 and ds.synthetic is None
    for i, (wet, dry, lab) in enumerate(clips):
        x, y, dl, wl = ds[i]
        assert torch.equal(x, wet) and torch.equal(y, dry) and torch.equal(wl, lab) and float(dl.sum()) == 0.0
    with pytest.raises(ValueError):
        datasets.EffectDataset(**dict(kw, effects_to_remove=["chorus"]))
    if not torch.cuda.is_available():                       # a corpus to render: device-side rendering needs the GPU
        with pytest.raises(RuntimeError, match="renders on the GPU"):
            datasets.EffectDataset(**dict(kw, root=str(tmp_path), render_files=True, mode="train"))


def test_multistep_lr_and_optimizer_state_layout():
    """Scheduler = torch's chainable MultiStepLR (fires only on equality, so the reference's float milestones 0.8 * max_steps
    never fire when non-integer); optimiser state dict is torch.optim.AdamW's layout (Lightning's ckpt["optimizer_states"])."""
    from remfx_amd.optim import FlatAdamW, FlatParams, MultiStepLR
    net = torch.nn.Linear(5, 3)
    tnet = torch.nn.Linear(5, 3)
    for max_steps in (10, 3, 7):
        ms = [0.8 * max_steps, 0.95 * max_steps]
        opt = FlatAdamW(FlatParams(list(net.parameters()), allow_cpu=True), lr=1e-2)
        sched = MultiStepLR(opt, ms, gamma=0.1)
        topt = torch.optim.AdamW(tnet.parameters(), lr=1e-2)
        tsched = torch.optim.lr_scheduler.MultiStepLR(topt, ms, gamma=0.1)
        for _ in range(max_steps + 2):
            topt.step(); sched.step(); tsched.step()
            assert abs(opt.param_groups[0]["lr"] - topt.param_groups[0]["lr"]) < 1e-15, (max_steps, sched.last_epoch)
    tnet(torch.randn(2, 5)).sum().backward()
    topt.step()
    sd = opt.state_dict()
    tsd = topt.state_dict()
    assert set(sd) == set(tsd) and set(sd["state"][0]) == set(tsd["state"][0])
    assert set(tsd["param_groups"][0]) <= set(sd["param_groups"][0]) | {"decoupled_weight_decay", "initial_lr"}
    opt.m.normal_(); opt.v.uniform_(); opt.step_count = 7
    opt2 = FlatAdamW(FlatParams(list(torch.nn.Linear(5, 3).parameters()), allow_cpu=True), lr=1.0)
    opt2.load_state_dict(opt.state_dict())
    a, b = opt.state_dict()["state"], opt2.state_dict()["state"]          # (alignment padding of the flat buffer is not state)
    assert all(torch.equal(a[i][k], b[i][k]) for i in a for k in ("exp_avg", "exp_avg_sq")) and opt2.step_count == 7
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    torch.optim.AdamW(net.parameters(), lr=1e-2).load_state_dict(sd)     # torch accepts the layout


def test_missing_checkpoint_is_an_error(monkeypatch, tmp_path):
    from remfx_amd.trainer import load_checkpoint_file
    monkeypatch.delenv("RFX_ALLOW_RANDOM_INIT", raising=False)
    with pytest.raises(FileNotFoundError):
        load_checkpoint_file(str(tmp_path / "nope.ckpt"))
    monkeypatch.setenv("RFX_ALLOW_RANDOM_INIT", "1")
    with pytest.warns(UserWarning):
        assert load_checkpoint_file(str(tmp_path / "nope.ckpt")) is None


def _mixup_case():
    import numpy as np
    from oracle.gen_golden import tiny_heads_forward, tiny_heads_state      # the fixture's stand-in network (pure torch, no reference import)
    g = np.load(os.path.join(ROOT, "tests", "golden", "mixup.npz"))
    return g, tiny_heads_forward, tiny_heads_state


def test_mixup_replays_reference_draws():
    """`remfx_amd.models.mixup` against the seeded fixture recorded from the imported reference (oracle/gen_golden.py::gen_mixup;
    reference remfx/models.py:393-420): same numpy / torch draw order, so the same per-clip weights, the same mixing decision, the same
    partners; labels OR-ed.  Eight seeds, both branches."""
    import numpy as np
    from remfx_amd.models import mixup
    g, _, _ = _mixup_case()
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    branches = set()
    for s in g["seeds"]:
        np.random.seed(int(s))
        torch.manual_seed(int(s))
        mx, my, lam = mixup(x, y)
        branches.add(bool(g[f"did{s}"]))
        assert (mx is x) == (not bool(g[f"did{s}"]))
        assert torch.equal(lam, torch.from_numpy(g[f"lam{s}"])) and torch.equal(my, torch.from_numpy(g[f"my{s}"]))
        assert torch.equal(mx, torch.from_numpy(g[f"mx{s}"])), s             # same arithmetic order -> bit equal on the CPU
    assert branches == {True, False}
    np.random.seed(0)
    assert mixup(x, y, alpha=0.0)[2] == 1                                    # alpha <= 0: no weights drawn


def test_fxclassifier_mixup_training_branch_matches_reference():
    """The mixup branch of `FXClassifier.common_step` (reference remfx/models.py:491-500): loss = sum over the 5 heads of BCE against
    the OR-ed labels of the MIXED clips, accuracies against the unmixed labels; loss, parameter gradients and every logged scalar of
    both branches against the values recorded from the reference's own class."""
    import numpy as np
    from remfx_amd.classifier import Cnn14
    from remfx_amd.models import FXClassifier
    g, heads_forward, heads_state = _mixup_case()

    class Tiny(Cnn14):                                 # isinstance(network, Cnn14) selects BCELoss + per-effect accuracy, as upstream
        def __init__(self, st):
            torch.nn.Module.__init__(self)
            self.w, self.b = torch.nn.Parameter(st["w"].clone()), torch.nn.Parameter(st["b"].clone())

        def forward(self, z, train=False):
            return heads_forward(z, self.w, self.b)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    for s in (1, 4):
        net = Tiny(heads_state())
        cls = FXClassifier(3e-4, 1e-3, 48000, net, mixup=True)
        np.random.seed(s)
        torch.manual_seed(s)
        loss = cls.training_step((x, None, None, y), 0)
        loss.backward()
        assert abs(float(loss) - float(g[f"cls_loss{s}"])) < 1e-6 * max(1.0, abs(float(loss)))
        assert torch.allclose(net.w.grad, torch.from_numpy(g[f"cls_gw{s}"]), rtol=1e-5, atol=1e-7)
        assert torch.allclose(net.b.grad, torch.from_numpy(g[f"cls_gb{s}"]), rtol=1e-5, atol=1e-7)
        names = sorted(cls.logged)
        assert names == list(g[f"cls_log_names{s}"])
        got = np.array([float(cls.logged[k]) for k in names], dtype=np.float32)
        assert np.allclose(got, g[f"cls_log_vals{s}"], rtol=1e-5, atol=1e-6), (names, got, g[f"cls_log_vals{s}"])


def test_cfg_tree_is_what_its_author_script_writes(tmp_path, monkeypatch):
    """cfg/ is written by scripts/write_cfg_tree.py (experiments as rows of a table): the committed files are exactly its output."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("write_cfg_tree", os.path.join(ROOT, "scripts", "write_cfg_tree.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "CFG", str(tmp_path))
    mod.main()
    n = 0
    for d, _, fs in os.walk(os.path.join(ROOT, "cfg")):
        for f in fs:
            rel = os.path.relpath(os.path.join(d, f), os.path.join(ROOT, "cfg"))
            with open(os.path.join(d, f)) as a, open(os.path.join(tmp_path, rel)) as b:
                assert a.read() == b.read(), rel
            n += 1
    assert n == 48 and sum(len(fs) for _, _, fs in os.walk(tmp_path)) == 48


def test_product_crops_match_reference_golden():
    """`remfx_amd.utils.center_crop` / `causal_crop` (the product's own, not the oracle's) against the values recorded from the imported
    reference (`remfx/utils.py:202-211`; `causal_crop` drops the LAST sample); views, no copy."""
    import numpy as np
    from remfx_amd import utils
    import remfx.utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "utils_small.npz"))
    x = torch.from_numpy(g["crop_in"])
    c, k = utils.center_crop(x, 7), utils.causal_crop(x, 7)
    assert torch.equal(c, torch.from_numpy(g["center7"])) and torch.equal(k, torch.from_numpy(g["causal7"]))
    assert c.data_ptr() == x[..., (20 - 7) // 2:].data_ptr() and k.data_ptr() == x[..., 20 - 1 - 7:].data_ptr()
    assert remfx.utils.causal_crop is utils.causal_crop and utils.crop_start(True, 20, 7) == 12 and utils.crop_start(False, 20, 7) == 6


def test_flat_layout_follows_forward_use_order_and_buckets_complete_in_backward_order():
    """Hybrid Demucs registers every frequency layer before the time layers it interleaves with and the frequency embedding last; in
    registration order the FIRST gradient bucket (taken from the high end of the flat buffer) would hold the embedding and the time
    encoders, whose gradients arrive at the very end of backward, and hold back the in-order all-reduces of all other buckets.
    `HDemucs.forward_use_order()` + `FlatParams(layout=...)` put memory in execution order: every bucket's parameters are used later
    in forward (= finished earlier in backward) than those of the next bucket; indices, views and the optimiser's parameter order stay."""
    from remfx_amd import ddp
    from remfx_amd.hdemucs import HDemucs
    from remfx_amd.optim import FlatParams
    net = HDemucs(sources=["mixture"], audio_channels=1, nfft=4096, channels=16)
    plist = list(net.parameters())
    order = net.forward_use_order()
    assert len(order) == len(plist) and {id(p) for p in order} == {id(p) for p in plist}
    use = {id(p): k for k, p in enumerate(order)}
    ref = [p.detach().clone() for p in plist]
    flat = FlatParams(plist, allow_cpu=True, layout=order)
    assert [id(p) for p in flat.params] == [id(p) for p in plist]                       # optimiser order unchanged
    for p, r, o in zip(plist, ref, flat.offsets):
        assert torch.equal(p, r) and p.data_ptr() == flat.data.data_ptr() + 4 * o and p.grad.data_ptr() == flat.grad.data_ptr() + 4 * o
    assert sorted(range(len(plist)), key=lambda i: flat.offsets[i]) == [next(i for i, q in enumerate(plist) if q is p) for p in order]
    sync = ddp.GradSync(flat, bucket_mb=0.25)
    assert len(sync.buckets) >= 4
    lo_use = [min(use[id(plist[i])] for i in range(len(plist)) if sync.bucket_of[i] == b) for b in range(len(sync.buckets))]
    hi_use = [max(use[id(plist[i])] for i in range(len(plist)) if sync.bucket_of[i] == b) for b in range(len(sync.buckets))]
    assert all(lo_use[b] > hi_use[b + 1] for b in range(len(sync.buckets) - 1))       # bucket b is used strictly later than bucket b + 1
    names = {id(p): n for n, p in net.named_parameters()}
    assert names[id(order[0])].startswith("time_encoder.0") and names[id(order[-1])].startswith("time_decoder.4")
    with pytest.raises(ValueError):
        FlatParams(plist, allow_cpu=True, layout=order[:-1])


def test_every_entry_point_is_pinned():
    """tests/abi_census.py: its keys are the ABI, every value is an existing tests/test_gpu_*.py (this module for host-only queries), and
    the entry's name stands in that module, in a tests/*_ref.py it imports or in the remfx_amd wrapper it imports -- for the entries
    no test names, in the wrapper VIA records"""
    from remfx_amd import _lib
    from tests import abi_census as A
    assert set(A.PINNED_BY) == set(_lib.SIGNATURES), set(A.PINNED_BY) ^ set(_lib.SIGNATURES)
    here = os.path.join(ROOT, "tests")
    for entry, module in A.PINNED_BY.items():
        assert re.fullmatch(r"test_gpu_\w+\.py", module) or module == A.HOST_ONLY, (entry, module)
        assert os.path.exists(os.path.join(here, module)), (entry, module)
        found = A.names(entry, module)
        assert found, (entry, "is not named by", module, "or by anything it imports")
        if entry in A.VIA:
            assert A.VIA[entry][0] in found, (entry, found)
        else:
            assert any(not f.startswith("remfx_amd/") for f in found), (entry, "only named by a wrapper: record it in VIA", found)
    assert set(A.VIA) <= set(A.PINNED_BY)
    # the host-only queries are called here, without a device
    for entry, module in A.PINNED_BY.items():
        if module == A.HOST_ONLY:
            assert entry in ("rfx_abi_version", "rfx_gemm_pick_r", "rfx_lstm_ws_bytes"), entry


def test_lstm_workspace_bytes():
    """rfx_lstm_ws_bytes, a host-only query: 256 bytes of flags, 64 bytes of counters for each of the 768 / (H / 32) clusters the
    workspace is laid out for, and per cluster two exchange buffers of (H / 32)^2 tiles of 4096 bytes; H has to be a multiple of 32 up
    to 512"""
    from remfx_amd import _lib
    L = _lib.lib()
    for H in range(32, 513, 32):
        nwc = H // 32
        clusters = 768 // nwc
        assert L.rfx_lstm_ws_bytes(H) == 256 + clusters * 64 + clusters * 2 * nwc * nwc * 4096, H
    for H in (0, -32, 16, 33, 544, 1024):
        assert L.rfx_lstm_ws_bytes(H) == -1, H


def test_every_autograd_node_is_pinned():
    """tests/node_census.py: its keys are the torch.autograd.Function subclasses under remfx_amd/ (found with ast), every value is an
    existing tests/test_gpu_*.py.  For test_gpu_nodes.py the case table of tests/node_ref.py must hold a case of the class.  For the
    other modules the check is only that the file mentions the class or the name VIA records (often just the module under test): that
    keeps the map from pointing at a file that never touches the code, it does not prove the backward is judged there -- the map was
    filled by reading"""
    import ast
    from tests import node_census as N
    found = set()
    pkg = os.path.join(ROOT, "remfx_amd")
    for f in sorted(os.listdir(pkg)):
        if not f.endswith(".py"):
            continue
        for n in ast.walk(ast.parse(open(os.path.join(pkg, f)).read())):
            if isinstance(n, ast.ClassDef) and any(ast.unparse(b) in ("torch.autograd.Function", "autograd.Function", "Function") for b in n.bases):
                found.add(f"{f[:-3]}.{n.name}")
    assert found == set(N.PINNED_BY), found ^ set(N.PINNED_BY)
    here = os.path.join(ROOT, "tests")
    from tests import node_ref
    tabled = {c.node for c in node_ref.case_table() + node_ref.dconv_cases()}
    for node, module in N.PINNED_BY.items():
        assert re.fullmatch(r"test_gpu_\w+\.py", module) and os.path.exists(os.path.join(here, module)), (node, module)
        cls = node.split(".")[1]
        if module == N.NODES:
            assert node.split(".")[0] in ("ops", "nnops") and cls in tabled, (node, "has no case in tests/node_ref.py")
        else:
            text = open(os.path.join(here, module)).read()
            assert cls in text or (node in N.VIA and N.VIA[node] in text), (node, "is not named by", module)
    assert set(N.VIA) <= set(N.PINNED_BY)
