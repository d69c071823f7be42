"""Host side of batched dataset rendering (remfx_amd.datasets plan_effects / read_wav_chunk, scripts/generate_dataset.py):
what must hold without a device -- the draw order, the chunk reader's values and random calls, the declared symbols."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000
NAMES = ["reverb", "chorus", "delay", "distortion", "compressor"]


def _stub_effects(log):
    """The five real classes with a ``draw()`` that records itself and what it drew (rand / loguniform like the originals: they
    ARE the originals' draws), and a ``forward`` that draws and leaves the clip alone: `process_effects` runs with them on the
    host and makes exactly the per-item path's random calls."""
    from remfx_amd import effects as E
    classes = {"reverb": E.RandomPedalboardReverb, "chorus": E.RandomPedalboardChorus, "delay": E.RandomPedalboardDelay,
               "distortion": E.RandomPedalboardDistortion, "compressor": E.RandomPedalboardCompressor}
    out = {}
    for name, base in classes.items():
        fx = base(SR)

        def draw(_name=name, _fx=fx, _base=base):
            p = _base.draw(_fx)
            log.append((_name, {k: float(v) for k, v in p.items()}))
            return p
        fx.draw = draw                                        # on the instance: type(fx) stays the class the labels look up
        fx.forward = lambda x, _draw=draw: (_draw(), x)[1]
        out[name] = fx
    return out


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("kept,removed", [([0, 0], [0, 0]), ([2, 2], [2, 2]), ([0, 0], [0, 5]), ([1, 1], [1, 4])])
def test_plan_effects_draws_in_the_per_item_order(shuffle, kept, removed):
    """The counts of the issue's list ([0, 0], [2, 2], [0, 5], [1, 4]) as the removed range, shuffling on and off: under one
    seed `process_effects` (the per-item path itself, on stubs) and `plan_effects` record the same draws with the same values,
    give the same labels and leave both generators in the same state."""
    from remfx_amd import datasets as D
    keep, remove = ["reverb", "chorus", "delay"], ["compressor", "distortion", "reverb", "chorus", "delay"]
    x = torch.zeros(1, 16)
    runs = []
    for planned in (False, True):
        log = []
        fx = _stub_effects(log)
        torch.manual_seed(21)
        np.random.seed(21)
        labels = []
        for _ in range(6):                                   # several clips: the sequence runs on from clip to clip
            if planned:
                k, r, dl, wl = D.plan_effects(fx, keep, remove, kept, removed, shuffle, shuffle)
                assert [n for n, _ in k] + [n for n, _ in r] == [n for n, _ in log[len(log) - len(k) - len(r):]]
                assert kept[0] <= len(k) <= kept[1] and removed[0] <= len(r) <= removed[1]
            else:
                _, _, dl, wl = D.process_effects(x, fx, keep, remove, kept, removed, shuffle, shuffle, lambda t: t)
            labels.append((dl, wl))
        runs.append((log, labels, torch.rand(1).item(), np.random.rand()))
    (log_a, lab_a, t_a, n_a), (log_b, lab_b, t_b, n_b) = runs
    assert log_a == log_b and len(log_a) >= 6 * (kept[0] + removed[0])
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(lab_a, lab_b))
    assert t_a == t_b and n_a == n_b                        # no random call the per-item path does not make


def _write(path, data, sr):
    from scipy.io import wavfile
    wavfile.write(str(path), sr, data)


@pytest.mark.parametrize("kind", ["pcm16", "pcm32", "float32"])
@pytest.mark.parametrize("channels", [1, 2])
def test_chunk_reader_equals_the_decoded_file(tmp_path, kind, channels):
    from remfx_amd import datasets as D
    rng = np.random.default_rng(3)
    v = rng.standard_normal((30000, channels)) * 0.2
    data = {"pcm16": (v * 32767).clip(-32768, 32767).astype(np.int16),
            "pcm32": (v * 2147483647).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32),
            "float32": v.astype(np.float32)}[kind]
    path = tmp_path / f"{kind}.wav"
    _write(path, data[:, 0] if channels == 1 else data, 44100)
    whole, sr = D.load_wav(path)
    assert sr == 44100 and whole.shape == (channels, 30000)
    for a, b in ((0, 30000), (17, 4113), (29999, 30000), (12000, 12000)):
        got = D.read_wav_chunk(path, a, b)
        assert got.dtype == torch.float32 and torch.equal(got, whole[:, a:b])


def test_select_random_chunk_keeps_its_values_and_random_calls(tmp_path):
    """`select_random_chunk` reads only the chunk now: same chunk, same generator state afterwards as the whole-file decode it
    replaces (restated here), for an accepted chunk, a file that is too short and a nearly silent chunk."""
    from remfx_amd import datasets as D

    def before(path, chunk_size, sample_rate):                # the parent's select_random_chunk, without the resampling
        audio, sr = D.load_wav(path)
        n = int(chunk_size * (sr / sample_rate))
        if n >= audio.shape[-1]:
            return None
        start = torch.randint(0, audio.shape[-1] - n, (1,)).item()
        chunk = audio[:, start:start + n]
        return None if torch.mean(torch.abs(chunk)) < 1e-4 else chunk

    rng = np.random.default_rng(5)
    loud = (rng.standard_normal(20000) * 3000).astype(np.int16)
    quiet = np.zeros(20000, dtype=np.int16)
    quiet[::100] = 1
    for name, data, chunk_size in (("loud", loud, 4096), ("short", loud, 30000), ("quiet", quiet, 4096)):
        path = tmp_path / f"{name}.wav"
        _write(path, data, SR)                               # at the target rate: no resampling, no device
        for seed in (0, 1, 2):
            torch.manual_seed(seed)
            want = before(path, chunk_size, SR)
            state = torch.get_rng_state()
            torch.manual_seed(seed)
            got = D.select_random_chunk(path, chunk_size, SR)
            assert torch.equal(torch.get_rng_state(), state)
            assert (want is None) == (got is None) and (want is None or torch.equal(want, got))
        assert (want is None) == (name != "loud")


def test_normalize_rows_symbols_are_declared_and_exported():
    from remfx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "remfx_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(rfx_[a-z0-9_]+)\s*\(", hdr))
    want = {"rfx_fx_normalize_rows", "rfx_fx_normalize_ws_bytes"}
    assert want <= declared and want <= set(_lib.SIGNATURES)
    L = ctypes.CDLL(_lib.build())
    for name in want:
        assert hasattr(L, name), name
    L.rfx_fx_normalize_ws_bytes.restype = ctypes.c_int64
    assert L.rfx_fx_normalize_ws_bytes(ctypes.c_int32(3), ctypes.c_int32(10)) == 3 * 10 * 8 + 2 * 3 * 4


def test_row_table_is_checked_on_the_host():
    from remfx_amd.effects import row_table
    assert row_table([2, 0, 5], 6, "cpu").tolist() == [2, 0, 5] and row_table([2, 0, 5], 6, "cpu").dtype == torch.int32
    for bad in ([], [0, 6], [-1], [1, 1]):
        with pytest.raises(ValueError, match="row table"):
            row_table(bad, 6, "cpu")


@pytest.mark.parametrize("exp", ["5-5_full", "5-5_full_cls_dynamic"])
def test_generate_dataset_script_reaches_the_datamodule(tmp_path, exp):
    """scripts/generate_dataset.py composes the experiment from the repo's cfg/ and instantiates the datamodule; with no
    corpus that is the white-noise warning and exit status 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("DATASET_ROOT", "REMFX_CFG_DIR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "generate_dataset.py"), f"+exp={exp}"], cwd=tmp_path, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "no corpus (DATASET_ROOT)" in r.stdout and "white-noise" in r.stdout, r.stdout
    assert not (tmp_path / "data" / "processed").exists()


def test_parallel_flag_selects_the_batch_loader():
    """parallel=False: the loader the parent builds (a collating DataLoader over the dataset); parallel=True: items are whole
    batches, ceil(len / batch_size) of them.  No rendering happens until the loader is iterated."""
    from remfx_amd import datasets as D
    log = []
    kw = dict(root=None, sample_rate=SR, chunk_size=65536, total_chunks=7, effect_modules=_stub_effects(log),
              effects_to_keep=[], effects_to_remove=NAMES, num_kept_effects=[0, 0], num_removed_effects=[0, 5])
    with pytest.warns(UserWarning, match="white-noise"):
        plain, batched = D.DynamicEffectDataset(parallel=False, **kw), D.DynamicEffectDataset(parallel=True, **kw)
    a = D.EffectDatamodule(plain, plain, plain, train_batch_size=3).train_dataloader()
    b = D.EffectDatamodule(batched, batched, batched, train_batch_size=3).train_dataloader()
    assert type(a) is type(b) is torch.utils.data.DataLoader
    assert a.dataset is plain and a.batch_size == 3 and len(a) == 3
    assert b.batch_size is None and len(b) == 3 and b.dataset.dataset is batched
    assert log == []
