"""GPU: dataset clips rendered in batches (remfx_amd.datasets process_effects_batch / render_batch, `parallel=True`) with the
round normalisation of csrc/fx.hip (rfx_fx_normalize_rows).  The contract: under the same seeds the batched path gives the
clips and labels of the per-item path bit for bit, with a launch count that follows the plan structure and not the batch size."""
import math
import random

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.one_mode]
DEV = "cuda:0"
SR = 48000
ORDER = ["distortion", "compressor", "reverb", "chorus", "delay"]          # cfg/exp/5-5_full_cls_dynamic.yaml
CONFIGS = {       # effects_to_keep, effects_to_remove, num_kept, num_removed, shuffle_kept, shuffle_removed
    "stock": (["reverb", "chorus", "delay"], ["compressor", "distortion"], [2, 2], [2, 2], True, False),
    "dynamic": ([], ORDER, [0, 0], [0, 5], True, False),
    "ragged": (["reverb", "chorus", "delay"], ["compressor", "distortion", "reverb", "chorus"], [0, 3], [1, 4], True, True),
}


def _fx():
    from remfx_amd import effects as E
    return {"reverb": E.RandomPedalboardReverb(SR), "chorus": E.RandomPedalboardChorus(SR), "delay": E.RandomPedalboardDelay(SR),
            "distortion": E.RandomPedalboardDistortion(SR), "compressor": E.RandomPedalboardCompressor(SR)}


def _noise(B, T, seed):
    return (torch.randn(B, 1, T, generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)     # about -20 dB


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name,seed", [("stock", 3), ("dynamic", 7), ("ragged", 1)])
def test_batch_equals_the_per_item_path(name, seed):
    from remfx_amd import datasets as D, effects as E
    fx, norm, cfg = _fx(), E.LoudnessNormalize(SR, target_lufs_db=-20), CONFIGS[name]
    B, T = 9, 65536
    x = _noise(B, T, 100 + seed)
    _seed(seed)
    single = [D.process_effects(x[b], fx, *cfg, norm) for b in range(B)]
    _seed(seed)
    plans = [D.plan_effects(fx, *cfg) for _ in range(B)]
    counts = [len(p[1]) for p in plans]
    if name == "dynamic":                                     # the empty and the full chain are both in the batch
        assert 0 in counts and 5 in counts, counts
        assert all([n for n, _ in p[1]] == ORDER[:len(p[1])] and not p[0] for p in plans)
    if name == "ragged":
        assert len(set(counts)) > 1 and len({len(p[0]) for p in plans}) > 1
    dry, wet, dl, wl = D.process_effects_batch(x, plans, fx, norm)
    assert dry.shape == wet.shape == (B, 1, T) and dl.shape == wl.shape == (B, 5)
    for b, (d1, w1, dl1, wl1) in enumerate(single):
        assert torch.equal(d1, dry[b]), (name, b, "dry")
        assert torch.equal(w1, wet[b]), (name, b, "wet", [n for n, _ in plans[b][1]])
        assert torch.equal(dl1, dl[b]) and torch.equal(wl1, wl[b])
        assert int(wl[b].sum()) == counts[b]
    # the same rounds with torch indexing instead of row tables: the comparison variant of scripts/perf_render.py
    dry2, wet2, _, _ = D.process_effects_batch(x, plans, fx, norm, row_tables=False)
    assert torch.equal(dry2, dry) and torch.equal(wet2, wet)


def test_normalize_rows_writes_its_rows_only_and_null_table_is_the_old_entry_points():
    """Rows of the state that sit a round out keep their bits (a NaN payload as the sentinel); the addressed rows get what
    rfx_fx_loudness + rfx_fx_scale give (the per-item path's calls); without a table the call equals those two bit for bit."""
    from remfx_amd import effects as E
    norm = E.LoudnessNormalize(SR, target_lufs_db=-20)
    N, T, rows = 6, 30011, [4, 1, 3]
    state = _noise(N, T, 7).squeeze(1).contiguous()
    sentinel = torch.full((T,), 0x7FC0BEEF, dtype=torch.int32, device=DEV).view(torch.float32)
    for r in (0, 2, 5):
        state[r] = sentinel
    before = state.clone()
    clips = (_noise(len(rows), T, 8).squeeze(1) * torch.tensor([[0.3], [1.0], [4.0]], device=DEV)).contiguous()
    kept = clips.clone()
    want = norm(clips.unsqueeze(1)).squeeze(1)
    assert torch.equal(norm.normalize_rows(clips, torch.empty_like(clips)), want)
    assert norm.normalize_rows(clips, state, rows) is state and torch.equal(clips, kept)
    for i, r in enumerate(rows):
        assert torch.equal(state[r], want[i])
    for r in (0, 2, 5):
        assert torch.equal(_bits(state[r]), _bits(before[r]))
    for bad in ([0, 0, 1], [0, N, 1], [0, 1]):
        with pytest.raises(ValueError, match="row table|rows for"):
            norm.normalize_rows(clips, state, bad)
    with pytest.raises(ValueError, match="outside the state"):
        norm.normalize_rows(state[:3], state, rows)
    assert torch.equal(_bits(state[0]), _bits(before[0]))


def _counted(fx, norm):
    """Wrap every effect object's ``render`` and the normaliser's measurements (``measure`` of the per-item calls,
    ``normalize_rows`` of the batched rounds) with counters."""
    count = {}

    def wrap(obj, attr, key):
        fn = getattr(obj, attr)

        def counted(*a, **k):
            count[key] = count.get(key, 0) + 1
            return fn(*a, **k)
        setattr(obj, attr, counted)
    for name, e in fx.items():
        wrap(e, "render", name)
    wrap(norm, "measure", "normalize")
    wrap(norm, "normalize_rows", "normalize")
    return count


def test_one_launch_per_round_and_effect_whatever_the_batch_size():
    from remfx_amd import datasets as D, effects as E
    T = 32768
    _seed(12)
    base = [D.plan_effects(_fx(), *CONFIGS["ragged"]) for _ in range(4)]
    rounds = {}                                              # effect name -> the (phase, round) pairs it occurs in
    for p in base:
        for phase in (0, 1):
            for k, (name, _) in enumerate(p[phase]):
                rounds.setdefault(name, set()).add((phase, k))
    nrounds = sum(max(len(p[phase]) for p in base) for phase in (0, 1))
    assert nrounds >= 4 and len(rounds) >= 3
    seen = []
    for B in (4, 32):
        fx, norm = _fx(), E.LoudnessNormalize(SR, target_lufs_db=-20)
        count = _counted(fx, norm)
        plans = [base[b % 4] for b in range(B)]              # the same plan structure, eight times over
        dry, wet, _, _ = D.process_effects_batch(_noise(B, T, B), plans, fx, norm)
        assert dry.shape == (B, 1, T) and bool(torch.isfinite(wet).all())
        for name, c in count.items():
            if name != "normalize":
                assert c <= len(rounds[name]), (B, name, c, rounds[name])
        assert count["normalize"] == nrounds + 1, (B, count)            # one per round, one for the 2 B final rows
        seen.append(count)
    assert seen[0] == seen[1], seen


def _corpus(tmp_path):
    from remfx_amd import datasets as D
    corpus = tmp_path / "corpus" / "audio_mono-mic"
    corpus.mkdir(parents=True)
    g = torch.Generator().manual_seed(9)
    for k in range(3):
        D.save_wav(corpus / f"0{k}_clip.wav", torch.randn(1, 44100 * 3, generator=g) * 0.1, 44100)       # resampled on the device
    return str(tmp_path / "corpus")


def test_rendered_files_are_the_same_with_and_without_parallel(tmp_path):
    from remfx_amd import datasets as D
    keep, remove, nk, nr, sk, sr_ = CONFIGS["ragged"]
    kw = dict(root=_corpus(tmp_path), sample_rate=SR, chunk_size=32768, total_chunks=7, effect_modules=_fx(), effects_to_keep=keep,
              effects_to_remove=remove, num_kept_effects=nk, num_removed_effects=nr, shuffle_kept_effects=sk,
              shuffle_removed_effects=sr_, mode="train")
    sets = []
    for parallel in (False, True):
        _seed(31)
        ds = D.EffectDataset(render_files=True, render_root=str(tmp_path / f"render{int(parallel)}"), parallel=parallel,
                             render_batch_size=3, **kw)
        assert len(ds) == 7
        sets.append(ds)
    a, b = sets
    assert a.proc_root != b.proc_root and sorted(p.name for p in b.proc_root.iterdir()) == [str(i) for i in range(7)]
    nwet = set()
    for i in range(7):
        for f in ("input.wav", "target.wav"):
            (xa, ra), (xb, rb) = D.load_wav(a.proc_root / str(i) / f), D.load_wav(b.proc_root / str(i) / f)
            assert ra == rb == SR and xa.shape == (1, 32768) and torch.equal(xa, xb), (i, f)
        for f in ("dry_effects.pt", "wet_effects.pt"):
            la, lb = torch.load(a.proc_root / str(i) / f), torch.load(b.proc_root / str(i) / f)
            assert la.shape == (5,) and la.dtype == lb.dtype and torch.equal(la, lb), (i, f)
        nwet.add(int(lb.sum()))
    assert len(nwet) > 1
    back = D.EffectDataset(render_files=False, render_root=str(tmp_path / "render1"), **kw)
    assert len(back) == 7
    for i in (0, 6):
        got, want = back[i], a[i]
        assert all(torch.equal(g, w) for g, w in zip(got, want))


def _dynamic(parallel, total_chunks=10, T=65536):
    from remfx_amd import datasets as D
    keep, remove, nk, nr, sk, sr_ = CONFIGS["dynamic"]
    with pytest.warns(UserWarning, match="white-noise"):
        return D.DynamicEffectDataset(root=None, sample_rate=SR, chunk_size=T, total_chunks=total_chunks, effect_modules=_fx(),
                                      effects_to_keep=keep, effects_to_remove=remove, num_kept_effects=nk, num_removed_effects=nr,
                                      shuffle_kept_effects=sk, shuffle_removed_effects=True, mode="train", parallel=parallel)


def test_dynamic_dataset_serves_rendered_batches():
    from oracle import ref_effects as R
    from remfx_amd import datasets as D
    bs, total, T = 4, 10, 65536
    _seed(8)
    ds = _dynamic(True, total, T)
    loader = D.EffectDatamodule(ds, ds, ds, train_batch_size=bs, test_batch_size=bs, num_workers=4).train_dataloader()
    assert len(loader) == math.ceil(total / bs)
    sizes, effects, differ = [], 0, 0
    for wet, dry, dl, wl in loader:
        n = wet.shape[0]
        sizes.append(n)
        assert wet.shape == dry.shape == (n, 1, T) and dl.shape == wl.shape == (n, 5)
        assert wet.is_cuda and dry.is_cuda and dl.is_cuda and wl.is_cuda and wet.dtype == torch.float32
        assert float(dl.sum()) == 0
        for t in (wet, dry):
            for b in range(n):
                assert abs(R.integrated_loudness(t[b, 0].cpu().numpy(), SR) + 20.0) < 0.05
        for b in range(n):
            if float(wl[b].sum()) == 0:                      # nothing removed: the wet clip is the dry clip
                assert torch.equal(wet[b], dry[b])
        differ += int((wet - dry).abs().amax(dim=(1, 2)).gt(1e-3).sum())
        effects += int(wl.sum())
    assert sizes == [4, 4, 2] and effects >= 5 and differ >= 3
    plain = _dynamic(False, total, T)
    before = D.EffectDatamodule(plain, plain, plain, train_batch_size=bs, num_workers=4).train_dataloader()
    assert type(before) is torch.utils.data.DataLoader and before.dataset is plain and before.batch_size == bs
    assert len(before) == math.ceil(total / bs) and before.num_workers == 0
    xb, yb, dlb, wlb = next(iter(before))
    assert xb.shape == (bs, 1, T) and xb.is_cuda and wlb.shape == (bs, 5)


def test_render_batch_is_deterministic_and_matches_getitem():
    runs = []
    for _ in range(2):
        _seed(17)
        runs.append(_dynamic(True).render_batch(16))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    _seed(17)
    ds = _dynamic(False)
    for b in range(16):
        wet, dry, dl, wl = ds[b]
        assert torch.equal(wet, runs[0][0][b]) and torch.equal(dry, runs[0][1][b])
        assert torch.equal(dl, runs[0][2][b].cpu()) and torch.equal(wl, runs[0][3][b].cpu())
