"""Records tests/golden/fx_channel.npz from the reference's remfx/effects.py (needs the reference tree; CPU only).

The reference module is loaded with oracle.gen_golden's import shims plus stand-ins for what it imports at module level:
pedalboard (plugins record their keyword arguments and return the input unchanged), torchvision.transforms.Compose /
RandomApply (torchvision's semantics: a stage is skipped when p < torch.rand(1)) and pyloudnorm.Meter (a constant).
RandomParametricEQ, RandomStereoWidener and RandomVolumeAutomation then render for real (scipy / torch on the CPU).
Every value the reference draws (rand, randint, loguniform, np.random.dirichlet) is logged in order.

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_fx_golden.py
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, install_shims  # noqa: E402
from tests.fx_channel_ref import fixture_input  # noqa: E402

SR, T = 48000, 8192
LOG, CALLS, TRACE = [], [], []
PLUGINS = ("Chorus", "Reverb", "Compressor", "Phaser", "Delay", "Distortion", "Limiter")


def _logged(fn):
    def wrapped(*a, **k):
        v = fn(*a, **k)
        LOG.append(float(v))
        return v
    return wrapped


class _Board(list):
    def __call__(self, x, sample_rate):
        return x


def _plugin(name):
    def init(self, **kw):
        CALLS.append((name, {k: float(v) for k, v in kw.items()}))
    return type(name, (), {"__init__": init})


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class _RandomApply(torch.nn.Module):
    def __init__(self, transforms, p=0.5):
        super().__init__()
        self.transforms, self.p = transforms, p

    def forward(self, x):
        if self.p < torch.rand(1):
            return x
        for t in self.transforms:
            mark = len(LOG)
            x = t(x)
            TRACE.append((type(t).__name__, LOG[mark:]))
        return x


class _Meter:
    def __init__(self, rate):
        pass

    def integrated_loudness(self, x):
        return -20.0


def load_reference():
    install_shims()
    pb = sys.modules["pedalboard"]
    pb.Pedalboard = _Board
    for n in PLUGINS:
        setattr(pb, n, _plugin(n))
    tv = sys.modules["torchvision.transforms"]
    tv.Compose, tv.RandomApply = _Compose, _RandomApply
    sys.modules["pyloudnorm"].Meter = _Meter
    spec = importlib.util.spec_from_file_location("_reference_effects", os.path.join(REF, "remfx", "effects.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.rand, m.randint, m.loguniform = _logged(m.rand), _logged(m.randint), _logged(m.loguniform)
    dirichlet = np.random.dirichlet

    def logged_dirichlet(*a, **k):
        v = dirichlet(*a, **k)
        LOG.extend(float(u) for u in np.ravel(v))
        return v
    np.random.dirichlet = logged_dirichlet
    eq = m.parametric_eq

    def recorded_eq(x, sample_rate, **kw):
        CALLS.append(("parametric_eq", {k: [float(u) for u in v] if isinstance(v, list) else float(v) for k, v in kw.items()}))
        return eq(x, sample_rate, **kw)
    m.parametric_eq = recorded_eq
    return m


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    del LOG[:], CALLS[:], TRACE[:]


def main():
    m = load_reference()
    out = {}
    # biqaud: all three filter types, range ends of the reference's draws
    cases = [(g, f, q, kind) for kind in ("low_shelf", "peaking", "high_shelf")
             for g, f, q in ((-6.0, 20.0, 0.1), (6.0, 200.0, 4.0), (2.5, 1000.0, 0.707), (-3.3, 16000.0, 1.9))]
    out["biq_params"] = np.array([[g, f, q] for g, f, q, _ in cases])
    out["biq_kinds"] = np.array([k for *_, k in cases])
    coefs = [m.biqaud(g, f, q, SR, k) for g, f, q, k in cases]
    out["biq_b"], out["biq_a"] = np.array([b for b, _ in coefs]), np.array([a for _, a in coefs])
    meta = {}
    # RandomParametricEQ, mono and stereo
    for name, ch, seed in (("eq_mono", 1, 11), ("eq_stereo", 2, 12)):
        _seed(seed)
        y = m.RandomParametricEQ(SR)(fixture_input(100 + seed, ch, T))
        out[name + "_y"] = y.numpy()
        meta[name] = dict(seed=seed, input_seed=100 + seed, channels=ch, draws=list(LOG), params=CALLS[0][1])
    # RandomStereoWidener
    _seed(21)
    y = m.RandomStereoWidener(SR)(fixture_input(121, 2, T))
    out["widener_y"] = y.numpy()
    meta["widener"] = dict(seed=21, input_seed=121, draws=list(LOG))
    # RandomVolumeAutomation: two ordinary draws and the first seed that yields a zero-length segment
    vol = m.RandomVolumeAutomation(SR)
    zero = None
    for s in range(1000, 5000):
        _seed(s)
        vol(torch.zeros(1, T))
        n = int(LOG[0])                                # LOG = [n, n concentrations, n Dirichlet weights, n gains]
        if (T * np.array(LOG[1 + n:1 + 2 * n])).astype("int").min() == 0:
            zero = s
            break
    assert zero is not None
    meta["volume"] = []
    ys = []
    for k, s in enumerate((31, 32, zero)):
        _seed(s)
        x = fixture_input(131 + k, 1, T)
        y = vol(x)
        assert y is x
        ys.append(y.numpy().copy())
        meta["volume"].append(dict(seed=s, input_seed=131 + k, draws=list(LOG)))
    out["volume_y"] = np.stack(ys)
    # RandomAudioEffectsChannel: the draw trace
    chain = m.RandomAudioEffectsChannel(SR)
    meta["chain"] = []
    for s in range(40, 60):
        _seed(s)
        chain(fixture_input(7, 2, T))
        meta["chain"].append(dict(seed=s, stages=[n for n, _ in TRACE], draws=[d for _, d in TRACE],
                                  plugins=[[n, kw] for n, kw in CALLS]))
    meta["T"], meta["sample_rate"] = T, SR
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "fx_channel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; zero-length volume segment at seed", zero)


if __name__ == "__main__":
    main()
