"""GPU: the segmented long-file path -- rfx_segment_split / rfx_segment_merge (csrc/segment.hip) against the float64
restatement tests/segment_ref.py, segment.apply against a network run on the whole clip, RemFXChainInference.sample_long with
stand-in networks, and scripts/remfx_detect.py with `+segment_seconds`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import segment_ref as ref
from tests.conftest import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, T, L, overlap): the 16-byte path needs T, L and hop to be multiples of 4, everything else takes the dword path
SPLIT_SHAPES = [
    (2, 3, 4096 * 5, 4096, 1024),              # rows > 1, 16-byte path
    (1, 1, (1 << 22) + 17, 262144, 65536),     # a long file of odd length: dword path, tail-aligned last segment
    (3, 1, 10001, 1000, 250),                  # hop = 750, not a multiple of 4
    (1, 2, 10000, 1000, 250),                  # T and L multiples of 4 but the hop is not
    (2, 1, 3000, 4096, 1024),                  # shorter than one segment: zero-padded, 16-byte path
    (1, 2, 3001, 4096, 0),                     # the same on the dword path, no overlap
    (1, 1, 4096, 4096, 2048),                  # exactly one segment
    (1, 1, 4097, 4096, 0),                     # one sample more: two segments that overlap in all but one sample
    (1, 2, 8192 * 3, 8192, 6144),              # overlap 0.75: four clips per sample
]
# + (lead, trail)
MERGE_SHAPES = [s + (0, 0) for s in SPLIT_SHAPES] + [
    (2, 2, 20000, 4096, 1024, 1024, 0),        # a causal lead equal to the overlap, 16-byte path
    (1, 2, 20000, 4096, 1024, 20, 0),          # L' = 4076, still multiples of 4
    (1, 2, 20000, 4096, 1024, 21, 0),          # dword path
    (2, 1, 20001, 4096, 2048, 500, 524),       # centre crop
    (1, 1, 3000, 4096, 1024, 100, 0),          # short file with a lead
]


def _x(B, C, T, seed=0):
    return torch.randn(B, C, T, generator=torch.Generator().manual_seed(seed)) * 0.3


@pytest.mark.one_mode
@pytest.mark.parametrize("B,C,T,L,overlap", SPLIT_SHAPES)
def test_split_equals_reference(B, C, T, L, overlap):
    from remfx_amd import segment
    x = _x(B, C, T)
    plan = segment.SegmentPlan(T, L, overlap)
    got = segment.split(x.to(DEV), plan)
    want = ref.split(x.reshape(B * C, T).numpy(), L, overlap)
    assert got.shape == (B * C * plan.n_segments, 1, L)
    assert torch.equal(got.cpu().reshape(-1, L), torch.from_numpy(want))           # a copy: bit for bit


@pytest.mark.one_mode
@pytest.mark.parametrize("B,C,T,L,overlap,lead,trail", MERGE_SHAPES)
def test_merge_against_float64_reference(B, C, T, L, overlap, lead, trail):
    """max error < (max_cover + 3) * 2^-24 * max|y|: the kernel rounds once per product w * y, once per add and once for the
    divide (weights and their sum are exact integers); each of those errors is at most 2^-24 of sum(w) * max|y| before the
    divide, i.e. 2^-24 * max|y| after it.  Derived from the arithmetic, not measured."""
    from remfx_amd import segment
    plan = segment.SegmentPlan(T, L, overlap, lead, trail)
    rows, S, Lp = B * C, plan.n_segments, plan.clip_len
    y = torch.randn(rows * S, 1, Lp, generator=torch.Generator().manual_seed(T + lead))
    want = ref.merge(y.reshape(rows * S, Lp).numpy(), T, L, overlap, lead, trail)
    yd = y.to(DEV)
    out = torch.full((B, C, plan.out_len), float("nan"), device=DEV)
    got = segment.merge(yd, plan, channels=C, out=out)
    assert got.shape == (B, C, T - lead - trail)
    assert torch.isfinite(got).all()                           # every sample stored: no reliance on a zero fill
    again = segment.merge(yd, plan, channels=C)
    assert torch.equal(got, again)                             # deterministic
    err = np.abs(got.cpu().numpy().reshape(rows, -1).astype(np.float64) - want).max()
    bound = (plan.max_cover + 3) * 2.0 ** -24 * float(y.abs().max())
    print(f"merge T={T} L={L} overlap={overlap} lead={lead} trail={trail}: max err {err:.3e}, bound {bound:.3e}")
    assert err < bound, (err, bound)


@pytest.mark.one_mode
@pytest.mark.parametrize("B,C,T,L,overlap", SPLIT_SHAPES)
def test_merge_of_split_returns_the_input(B, C, T, L, overlap):
    from remfx_amd import segment
    x = _x(B, C, T, seed=3)
    plan = segment.SegmentPlan(T, L, overlap)
    xd = x.to(DEV)
    back = segment.merge(segment.split(xd, plan), plan, channels=C)
    assert back.shape == x.shape
    err = float((back.cpu().double() - x.double()).abs().max())
    bound = (plan.max_cover + 3) * 2.0 ** -24 * float(x.abs().max())
    print(f"merge(split) T={T} L={L} overlap={overlap}: max err {err:.3e}, bound {bound:.3e}")
    assert err < bound, (err, bound)
    same = segment.apply(lambda z: z, xd, L, overlap, batch=3)
    assert torch.equal(same, back)


def test_causal_tcn_segmented_equals_whole_clip():
    """A causal TCN is translation-invariant with finite support: clip by clip with overlap >= receptive field - 1 and
    align="end" it computes, in exact arithmetic, what it computes on the whole clip.  RMS difference < 2e-5: twice the 1e-5
    that tests/test_gpu_conv.py::test_tcn_golden allows each side against the oracle (the two sides may take different
    gather-GEMM kernels, convplan picks by size)."""
    from oracle import ref_tcn
    from remfx_amd import segment
    from remfx_amd.tcn import TCN
    cfg = dict(ninputs=1, noutputs=1, nblocks=3, channel_width=16, kernel_size=5, stack_size=2, dilation_growth=3, causal=True)
    sd = ref_tcn.tcn_init_state_dict(1, 1, 3, 16, 5, seed=5)
    for k in [k for k in sd if k.endswith("relu.weight")]:
        sd[k] = torch.linspace(0.05, 0.45, sd[k].numel())
    net = TCN(**cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    lead = net.receptive_field - 1
    T, L, overlap = 20001, 4096, 1024
    x = _x(2, 1, T, seed=9).to(DEV)
    with torch.no_grad():
        whole = net(x)
        seg = segment.apply(net, x, L, overlap, batch=4, align="end")
    assert whole.shape == (2, 1, T - lead) and seg.shape == whole.shape
    rms = float((seg - whole).pow(2).mean().sqrt())
    print(f"causal TCN, {segment.SegmentPlan(T, L, overlap, lead).n_segments} segments: rms diff {rms:.3e} "
          f"(output rms {float(whole.pow(2).mean().sqrt()):.3e})")
    check(rms, 2e-5, what="segmented vs whole-clip causal TCN")
    with pytest.raises(ValueError):
        segment.apply(net, x, L, overlap, align="same")                 # the network returns fewer samples
    with pytest.raises(ValueError):
        segment.apply(net, x, L, lead - 1, align="end")                 # overlap below the lead: windows would leave gaps


class _Tag(nn.Module):
    def __init__(self, mul):
        super().__init__()
        self.mul = mul

    def sample(self, z):
        return z * self.mul


class _Holder(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.model = m


LOUD = (0.93, 0.12, 0.12, 0.93, 0.12)        # a loud clip: reverb + distortion
QUIET = (0.12, 0.81, 0.12, 0.31, 0.12)       # a quiet one: chorus
ENERGY = 1e-2


class _EnergyDetector(nn.Module):
    """Stand-in detector keyed on the clip's mean square."""

    def forward(self, z):
        loud = (z.pow(2).mean((1, 2)) > ENERGY).float()[:, None]
        p = loud * torch.tensor(LOUD, device=z.device) + (1 - loud) * torch.tensor(QUIET, device=z.device)
        return [p[:, k:k + 1] for k in range(5)]


ORDER = ["RandomPedalboardDistortion", "RandomPedalboardCompressor", "RandomPedalboardReverb", "RandomPedalboardChorus",
         "RandomPedalboardDelay"]


def _expected_long(x, L, overlap, mode, muls, names):
    """numpy: the same stand-ins clip by clip (float32 products in chain order), float64 merge."""
    rows, T = x.shape
    clips = ref.split(x, L, overlap)
    S = clips.shape[0] // rows
    loud = (clips.astype(np.float64) ** 2).mean(1) > ENERGY
    probs = np.where(loud[:, None], np.asarray(LOUD, np.float32), np.asarray(QUIET, np.float32))
    if mode == "file":
        probs = np.repeat(probs.reshape(rows, S, 5).mean(1, keepdims=True), S, 1).reshape(rows * S, 5)
    labels = (probs > 0.5).astype(np.float32)
    out = clips.copy()
    for i, lab in enumerate(labels):
        for e in ORDER:
            if lab[names.index(e)] == 1.0:
                out[i] = out[i] * np.float32(muls[e])
    return ref.merge(out, T, L, overlap), labels.reshape(rows, S, 5), out


@pytest.mark.one_mode
def test_sample_long_with_stand_in_networks():
    from remfx_amd import models, segment
    names = models.ALL_EFFECT_NAMES
    muls = {n: 1.0 + 0.1 * (i + 1) for i, n in enumerate(names)}
    mods = {n: _Holder(_Tag(muls[n])) for n in names}
    chain = models.RemFXChainInference(mods, 48000, 1025, list(ORDER), classifier=_EnergyDetector())
    T, L, overlap = 30001, 4096, 0.25
    g = torch.Generator().manual_seed(11)
    amp = torch.where(torch.arange(T) < T // 2, 0.5, 0.01)
    x = torch.stack([torch.randn(T, generator=g) * amp, torch.randn(T, generator=g) * amp.flip(0)])[None]      # (1, 2, T)
    xn = x[0].numpy()
    for mode in ("segment", "file"):
        out, labels = chain.sample_long(x.to(DEV), segment=L, overlap=overlap, batch=5, detect=mode)
        plan = chain.last_plan
        want, want_labels, want_clips = _expected_long(xn, L, 1024, mode, muls, names)
        assert np.array_equal(plan.starts, ref.starts(T, L, 1024)) and plan.n_segments >= 3
        assert out.shape == (1, 2, T) and labels.shape == (2, plan.n_segments, 5)
        assert np.array_equal(labels.cpu().numpy(), want_labels)
        lab = labels.cpu().numpy()
        if mode == "segment":
            # the labels change where the input does: loud clips first in row 0, last in row 1
            assert lab[0, 0].tolist() == [1, 0, 0, 1, 0] and lab[0, -1].tolist() == [0, 1, 0, 0, 0]
            assert lab[1, 0].tolist() == [0, 1, 0, 0, 0] and lab[1, -1].tolist() == [1, 0, 0, 1, 0]
            changes = (np.abs(np.diff(lab[0], axis=0)).sum(1) > 0).nonzero()[0]
            assert len(changes) == 1                                   # one change, at the clip where the loud half ends
            i = int(changes[0])
            assert plan.starts[i] < T // 2 <= plan.starts[i + 1] + L
        else:
            assert (lab == lab[:, :1]).all()                           # one chain throughout each row
        err = np.abs(out.cpu().numpy()[0].astype(np.float64) - want).max()
        bound = (plan.max_cover + 3) * 2.0 ** -24 * float(np.abs(want_clips).max())
        print(f"sample_long detect={mode}: max err {err:.3e}, bound {bound:.3e}")
        assert err < bound, (mode, err, bound)
    # without a classifier the labels are required and broadcast to the clips
    bare = models.RemFXChainInference(mods, 48000, 1025, list(ORDER))
    with pytest.raises(ValueError):
        bare.sample_long(x.to(DEV), segment=L)
    out, labels = bare.sample_long(x.to(DEV), segment=L, overlap=overlap, labels=[[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]])
    assert labels[0].eq(torch.tensor([0, 0, 1, 0, 0.], device=DEV)).all() and labels[1].eq(0).all()
    k = np.float32(muls["RandomPedalboardDelay"])
    bound = 5 * 2.0 ** -24 * float(np.abs(xn).max()) * float(k)
    assert np.abs(out.cpu().numpy()[0, 0].astype(np.float64) - (xn[0] * k).astype(np.float64)).max() < bound
    assert np.abs(out.cpu().numpy()[0, 1].astype(np.float64) - xn[1]).max() < bound


def test_forward_unchanged_by_the_refactor(golden_dir):
    """RemFXChainInference.forward on an ordinary batch after its label -> chain -> sub-batch part moved into a helper: the same
    labels, output and loss as tests/golden/flow.npz records (what tests/test_gpu_classifier_chain.py checks), and the output bit
    for bit what the stand-ins give in float32 (one rounding per multiply and per add, in chain order)."""
    from remfx_amd import models
    g = np.load(os.path.join(golden_dir, "flow.npz"))

    class Tag(nn.Module):
        def __init__(self, mul, add):
            super().__init__()
            self.mul, self.add = mul, add

        def sample(self, z):
            return z * self.mul + self.add
    names = models.ALL_EFFECT_NAMES
    mods = {n: _Holder(Tag(1.0 + 0.1 * (i + 1), 0.01 * (i + 1))) for i, n in enumerate(names)}
    probs = torch.from_numpy(g["probs"]).to(DEV)

    class FakeCls(nn.Module):
        def forward(self, z):
            return [probs[:, k:k + 1] for k in range(5)]
    chain = models.RemFXChainInference(mods, 48000, 1025, list(ORDER), classifier=FakeCls())
    xc, yc = torch.from_numpy(g["xc"]).to(DEV), torch.from_numpy(g["yc"]).to(DEV)
    closs, cout = chain.forward((xc, yc, None, None), 0)
    assert chain.last_labels.cpu().tolist() == [[1, 0, 0, 1, 0], [0, 1, 0, 0, 1], [0, 0, 0, 0, 0]]
    np.testing.assert_allclose(cout.cpu().numpy(), g["chain_out"], rtol=1e-6, atol=1e-6)
    check(abs(float(closs) - float(g["chain_loss"])), 1e-4, abs(float(g["chain_loss"])))
    want = g["xc"].copy()
    for i, lab in enumerate(chain.last_labels.cpu().tolist()):
        for e in ORDER:
            k = names.index(e)
            if lab[k] == 1.0:
                want[i] = want[i] * np.float32(1.0 + 0.1 * (k + 1)) + np.float32(0.01 * (k + 1))
    assert np.array_equal(cout.cpu().numpy(), want)


@pytest.mark.one_mode
def test_remfx_detect_script_segmented_keeps_channels(tmp_path):
    """scripts/remfx_detect.py with `+segment_seconds=2 +keep_channels=true` on the 7 s stereo 44.1 kHz file of
    tests/test_gpu_train_script.py::test_remfx_detect_script_whole_file: 336000 samples at 48 kHz in 96000-sample clips with a
    72000-sample hop = 5 segments per channel; a float32 WAV with both channels, the resampled length, the label timeline."""
    from scipy.io import wavfile
    sr_in, secs = 44100, 7.0
    t = np.arange(int(sr_in * secs)) / sr_in
    rng = np.random.default_rng(0)
    a = np.stack([0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * rng.standard_normal(t.size),
                  0.2 * np.sin(2 * np.pi * 331.0 * t)], 1)
    src, dst = os.path.join(tmp_path, "in.wav"), os.path.join(tmp_path, "out.wav")
    wavfile.write(src, sr_in, (a * 32767).astype(np.int16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "remfx_detect.py"), "+exp=remfx_detect",
                        f"+audio_input={src}", f"+output_path={dst}", "inference_use_all_effect_models=True",
                        "+segment_seconds=2.0", "+keep_channels=true", "+segment_batch=4"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, RFX_ALLOW_RANDOM_INIT="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Loading models..." in r.stdout and "Saving output to" in r.stdout
    assert "Label timeline (5 segments of 96000 samples, hop 72000):" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("row ")]
    assert any(ln.startswith("row 0:") for ln in lines) and any(ln.startswith("row 1:") for ln in lines)
    assert " 0.00 s" in lines[0] and " 7.00 s" in lines[-1]
    sr_out, y = wavfile.read(dst)
    n = int(np.ceil(a.shape[0] * 48000 / sr_in))
    assert sr_out == 48000 and y.dtype == np.float32 and y.ndim == 2 and y.shape[1] == 2
    assert abs(y.shape[0] - n) <= 1 and np.isfinite(y).all()
