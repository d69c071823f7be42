"""Audio effects of the data side, rendered ON THE DEVICE (reference remfx/effects.py:297-616, 619-629, 699-707).

The reference renders its five training effects on the CPU with pedalboard (JUCE C++) and normalises loudness
with pyloudnorm while it builds the dataset (datasets.py:109-202) or augments on the fly (datasets.py:205-330).
Here the same classes -- same names (they are the dict keys of RemFXChainInference.model and of cfg ``ckpts:`` /
``inference_effects_ordering``, models.py:81,96), same constructor arguments (``cfg/effects/all.yaml`` instantiates
unchanged), same parameter ranges, same random draws in the same order (``rand`` = torch.rand(1), ``loguniform`` =
scipy) -- render through the HIP kernels of csrc/fx.hip, one launch per effect for a whole batch of clips with
per-clip parameters.  ``forward(x)`` takes the reference's ``(channels, samples)`` tensor or a batch
``(B, 1, samples)``; tensors must live on the GPU: the library raises otherwise.

Algorithms are restatements of the published JUCE / pedalboard / pyloudnorm code (oracle/ref_effects.py lists
them; both packages are absent here, parity unpinned).
"""
import math

import numpy as np
import torch

from .ops import launch, query, scratch


def loguniform(low=0, high=1):                         # effects.py:25-26
    import scipy.stats
    return scipy.stats.loguniform.rvs(low, high)


def rand(low=0, high=1):                               # effects.py:29-30
    return (torch.rand(1).numpy()[0] * (high - low)) + low


def randint(low=0, high=1):                            # effects.py:33-34
    return torch.randint(low, high + 1, (1,)).numpy()[0]


def require_device(x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise ValueError("remfx_amd.effects render on the GPU: pass a CUDA tensor (there is no CPU path)")


def _check_clips(x):
    require_device(x)
    if x.dim() not in (2, 3):
        raise ValueError(f"effects take (channels, samples) or (batch, channels, samples), got {tuple(x.shape)}")


def _rows(x):
    """(..., T) -> contiguous (N, T) fp32; ``.view(x.shape)`` restores the shape of a result."""
    return x.reshape(-1, x.shape[-1]).to(torch.float32).contiguous()


def _vec(vals, device, dtype=torch.float32):
    return torch.tensor(np.asarray(vals), dtype=dtype).to(device)


def _col(params, f, device, dtype=torch.float32):
    """One value per parameter set -- ``p[f]`` for a key, ``f(p)`` for a function -- as a device vector."""
    return _vec([p[f] if isinstance(f, str) else f(p) for p in params], device, dtype)


def row_table(rows, nstate, device):
    """A host sequence of row numbers -> the int32 device table rfx_fx_normalize_rows reads.  Checked HERE, on the host: the
    kernel indexes the state buffer with these values and cannot see its size."""
    rows = [int(r) for r in rows]
    if not rows or min(rows) < 0 or max(rows) >= nstate or len(set(rows)) != len(rows):
        raise ValueError(f"row table {rows}: needs distinct rows in [0, {nstate})")
    return torch.tensor(rows, dtype=torch.int32).to(device)


class _RandomEffect(torch.nn.Module):
    """Keeps every ``min_* / max_*`` range of the reference constructor.  ``draw()`` samples ONE parameter set with the
    reference's calls in the reference's order; ``forward`` draws one set per clip of a batch (one set for all channels of
    a 2-D input, as pedalboard applies one board to all channels) and renders."""

    defaults = {}
    renders_clips = False     # True: render takes (B, C, T) clips with one parameter set each, not (N, T) rows with one per row
    in_place = False          # True: render scales its rows in place, and forward hands back x itself with the result in it
    check_input = staticmethod(_check_clips)          # raises ValueError for what forward does not take

    def __init__(self, sample_rate: float, **ranges):
        super().__init__()
        unknown = set(ranges) - set(self.defaults)
        if unknown:                                   # same failure mode as a wrong kwarg upstream
            raise TypeError(f"{type(self).__name__}.__init__() got unexpected keyword arguments {sorted(unknown)}")
        self.sample_rate = sample_rate
        self.ranges = dict(self.defaults)
        self.ranges.update(ranges)
        for k, v in self.ranges.items():
            setattr(self, k, v)

    def draw(self):
        raise NotImplementedError

    def render(self, clips, params):
        """clips: (N, T) device tensor; params: list of N dicts (draw()).  Returns (N, T)."""
        raise NotImplementedError

    def draw_for(self, T):
        """The parameter set of one clip of T samples."""
        return self.draw()

    def forward(self, x: torch.Tensor):
        self.check_input(x)
        nsets = x.shape[0] if x.dim() == 3 else 1
        sets = [self.draw_for(x.shape[-1]) for _ in range(nsets)]
        self.last_params = sets
        if self.renders_clips:
            y = self.render(x.reshape(nsets, x.shape[-2], x.shape[-1]).to(torch.float32).contiguous(), sets)
            return y if x.dim() == 3 else y[0]
        rows = _rows(x)
        y = self.render(rows, [s for s in sets for _ in range(rows.shape[0] // nsets)])
        if not self.in_place:
            return y.view(x.shape)
        if y.data_ptr() != x.data_ptr():
            x.copy_(y.view(x.shape))
        return x


class RandomPedalboardReverb(_RandomEffect):
    defaults = dict(min_room_size=0.0, max_room_size=1.0, min_damping=0.0, max_damping=1.0, min_wet_dry=0.0,
                    max_wet_dry=0.7, min_width=0.0, max_width=1.0)

    def draw(self):                                    # effects.py:579-583
        return dict(room_size=rand(self.min_room_size, self.max_room_size), damping=rand(self.min_damping, self.max_damping),
                    wet_dry=rand(self.min_wet_dry, self.max_wet_dry), width=rand(self.min_width, self.max_width))

    def render(self, clips, params):
        dev = clips.device
        damp = _col(params, lambda p: p["damping"] * 0.4, dev)                       # juce::Reverb::setParameters
        fb = _col(params, lambda p: p["room_size"] * 0.28 + 0.7, dev)
        wet1 = _col(params, lambda p: 0.5 * (p["wet_dry"] * 3.0) * (1.0 + p["width"]), dev)
        dry = _col(params, lambda p: (1.0 - p["wet_dry"]) * 2.0, dev)
        y = torch.empty_like(clips)
        launch("rfx_fx_reverb", clips, y, clips.shape[0], clips.shape[1], int(self.sample_rate), damp, fb, wet1, dry)
        return y


_SOX_COMBS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)       # SoX reverb.c: filter lengths at 44100 Hz
_SOX_ALLPASSES = (225, 341, 441, 556)
_SOX_LDS_FLOATS = 160 * 1024 // 4                                    # one bank's delay lines share a workgroup's LDS


def sox_reverb_plan(params, sample_rate):
    """SoX `reverb`'s derived quantities of ONE drawn parameter set (reverb.c: reverb_create / filter_array_create): the pre-delay
    in samples, comb feedback, damping and bank gain as the C floats SoX keeps, and the 8 comb + 4 all-pass lengths of the two
    banks (wet channel 0: offset 0; wet channel 1: offset stereo_depth / 100).  SoX reads each value as a double from the
    reference's f-string, so a float32 draw counts with its printed digits."""
    params = {k: float(f"{v}") for k, v in params.items()}
    scale = params["room_scale"] / 100.0 * 0.9 + 0.1
    depth = params["stereo_depth"] / 100.0
    a = -1.0 / math.log(1.0 - 0.3)                      # reverberance 0 -> feedback 0.3
    b = 100.0 / (math.log(1.0 - 0.98) * a + 1.0)        # reverberance 100 -> feedback 0.98
    r = sample_rate * (1.0 / 44100.0)
    combs = [[int(scale * r * (t + 12 * off) + 0.5) for t in _SOX_COMBS] for off in (0.0, depth)]
    allpasses = [[int(r * (t + 12 * off) + 0.5) for t in _SOX_ALLPASSES] for off in (0.0, depth)]
    return dict(delay=int(params["pre_delay"] / 1000.0 * sample_rate + 0.5),
                feedback=float(np.float32(1.0 - math.exp((params["reverberance"] - b) / (a * b)))),
                damp=float(np.float32(params["high_freq_damping"] / 100.0 * 0.3 + 0.2)), gain=float(np.float32(0.015)),
                wet_dry=float(params["wet_dry"]), comb_lengths=combs, allpass_lengths=allpasses,
                lds_floats=max(sum(c) + sum(p) for c, p in zip(combs, allpasses)),
                min_lag=min(min(c + p) for c, p in zip(combs, allpasses)))


class RandomSoxReverb(_RandomEffect):
    """effects.py:516-572: SoX `reverb ... --wet-only` (restated from SoX's reverb.c, parity unpinned: csrc/fx.hip,
    tests/sox_reverb_ref.py) and the wet / dry mix.  The one effect with a STEREO result: ``(1, T)`` or ``(2, T)`` -> ``(2, T)``,
    ``(B, 1, T)`` or ``(B, 2, T)`` -> ``(B, 2, T)``, one parameter set per clip; a mono clip is the dry part of both channels."""
    defaults = dict(min_reverberance=10.0, max_reverberance=100.0, min_high_freq_damping=0.0, max_high_freq_damping=100.0,
                    min_wet_dry=0.0, max_wet_dry=1.0, min_room_scale=5.0, max_room_scale=100.0, min_stereo_depth=20.0,
                    max_stereo_depth=100.0, min_pre_delay=0.0, max_pre_delay=100.0)
    renders_clips = True

    def draw(self):                                    # effects.py:549-554
        return dict(reverberance=rand(self.min_reverberance, self.max_reverberance),
                    high_freq_damping=rand(self.min_high_freq_damping, self.max_high_freq_damping),
                    room_scale=rand(self.min_room_scale, self.max_room_scale),
                    stereo_depth=rand(self.min_stereo_depth, self.max_stereo_depth),
                    wet_dry=rand(self.min_wet_dry, self.max_wet_dry), pre_delay=rand(self.min_pre_delay, self.max_pre_delay))

    def render(self, clips, params):
        """clips: (B, Cin, T) device tensor, Cin = 1 or 2; params: list of B dicts (draw()).  Returns (B, 2, T)."""
        B, Cin, T = clips.shape
        geom, coef, lds = [], [], 0
        for b, p in enumerate(params):
            if not p["stereo_depth"] > 0:
                raise ValueError("SoX reverb with stereo_depth 0 renders one wet channel: not modelled")
            q = sox_reverb_plan(p, self.sample_rate)
            if q["min_lag"] < 1 or q["lds_floats"] > _SOX_LDS_FLOATS or q["delay"] < 0:
                raise ValueError(f"SoX reverb at {self.sample_rate} Hz, room_scale {p['room_scale']}: shortest filter lag "
                                 f"{q['min_lag']} samples, {q['lds_floats']} samples of delay lines per bank (1 and {_SOX_LDS_FLOATS} "
                                 f"are the limits), pre-delay {q['delay']}")
            lds = max(lds, q["lds_floats"])
            for c in range(Cin):
                for w in range(2):
                    geom.append([q["delay"]] + q["comb_lengths"][w] + q["allpass_lengths"][w] + [b * Cin + c, 0, 0])
                    coef.append([q["feedback"], q["damp"], q["gain"], q["wet_dry"]])
        dev = clips.device
        geom, coef = _vec(geom, dev, torch.int32), _vec(coef, dev)
        ws = torch.empty(query("rfx_fx_sox_reverb_ws_floats", B, Cin, T), device=dev, dtype=torch.float32)
        y = torch.empty((B, 2, T), device=dev, dtype=torch.float32)
        launch("rfx_fx_sox_reverb", clips, y, ws, B, Cin, T, geom, coef, lds)
        return y

    @staticmethod
    def check_input(x):
        require_device(x)
        if x.dim() not in (2, 3) or x.shape[-2] not in (1, 2):
            raise ValueError(f"the SoX reverb takes (1 or 2, samples) or (batch, 1 or 2, samples), got {tuple(x.shape)} "
                             "(beyond two channels SoX drops the stereo depth: not modelled)")


class RandomPedalboardChorus(_RandomEffect):
    defaults = dict(min_rate_hz=0.25, max_rate_hz=4.0, min_depth=0.0, max_depth=0.6, min_centre_delay_ms=5.0,
                    max_centre_delay_ms=10.0, min_feedback=0.1, max_feedback=0.6, min_mix=0.1, max_mix=0.7)

    def draw(self):                                    # effects.py:398-402
        return dict(rate_hz=rand(self.min_rate_hz, self.max_rate_hz), depth=rand(self.min_depth, self.max_depth),
                    centre_delay_ms=rand(self.min_centre_delay_ms, self.max_centre_delay_ms),
                    feedback=rand(self.min_feedback, self.max_feedback), mix=rand(self.min_mix, self.max_mix))

    def render(self, clips, params):
        cols = [_col(params, k, clips.device) for k in ("rate_hz", "depth", "centre_delay_ms", "feedback", "mix")]
        y = torch.empty_like(clips)
        launch("rfx_fx_chorus", clips, y, clips.shape[0], clips.shape[1], float(self.sample_rate), *cols)
        return y


class RandomPedalboardDelay(_RandomEffect):
    # `max_delay_sconds` is the reference's own spelling (effects.py:346; cfg/effects/all.yaml)
    defaults = dict(min_delay_seconds=0.1, max_delay_sconds=1.0, min_feedback=0.05, max_feedback=0.6, min_mix=0.0,
                    max_mix=0.7)

    def draw(self):                                    # effects.py:362-364
        return dict(delay_seconds=loguniform(self.min_delay_seconds, self.max_delay_sconds),
                    feedback=rand(self.min_feedback, self.max_feedback), mix=rand(self.min_mix, self.max_mix))

    def render(self, clips, params):
        dev = clips.device
        d = _col(params, lambda p: int(p["delay_seconds"] * self.sample_rate), dev, torch.int32)
        y = torch.empty_like(clips)
        launch("rfx_fx_delay", clips, y, clips.shape[0], clips.shape[1], d, _col(params, "feedback", dev), _col(params, "mix", dev))
        return y


class RandomPedalboardDistortion(_RandomEffect):
    defaults = dict(min_drive_db=-20.0, max_drive_db=12.0)

    def draw(self):                                    # effects.py:495
        return dict(drive_db=rand(self.min_drive_db, self.max_drive_db))

    def render(self, clips, params):
        g = _col(params, lambda p: 10.0 ** (p["drive_db"] / 20.0), clips.device)
        y = torch.empty_like(clips)
        launch("rfx_fx_distortion", clips, y, clips.shape[0], clips.shape[1], g)
        return y


def _ballistics_cte(ms, sample_rate):
    """juce::dsp::BallisticsFilter coefficient of an attack / release time."""
    return 0.0 if ms < 1e-3 else math.exp(-2.0 * math.pi * 1000.0 / float(sample_rate) / ms)


class RandomPedalboardCompressor(_RandomEffect):
    defaults = dict(min_threshold_db=-42.0, max_threshold_db=-6.0, min_ratio=1.5, max_ratio=4.0, min_attack_ms=1.0,
                    max_attack_ms=50.0, min_release_ms=10.0, max_release_ms=250.0)

    def draw(self):                                    # effects.py:323-326
        return dict(threshold_db=rand(self.min_threshold_db, self.max_threshold_db), ratio=rand(self.min_ratio, self.max_ratio),
                    attack_ms=rand(self.min_attack_ms, self.max_attack_ms), release_ms=rand(self.min_release_ms, self.max_release_ms))

    def render(self, clips, params):
        dev = clips.device
        thr = _col(params, lambda p: 10.0 ** (p["threshold_db"] / 20.0), dev)
        ratio = _col(params, "ratio", dev)
        ca = _col(params, lambda p: _ballistics_cte(p["attack_ms"], self.sample_rate), dev)
        cr = _col(params, lambda p: _ballistics_cte(p["release_ms"], self.sample_rate), dev)
        N, T = clips.shape
        y = torch.empty_like(clips)
        ws = scratch("rfx_fx_compressor_ws", N, T, device=dev, dtype=torch.float32)
        launch("rfx_fx_compressor", clips, y, ws, N, T, thr, ratio, ca, cr)
        return y


def _k_weighting(rate):
    """pyloudnorm "K-weighting": high shelf (+4 dB, 1500 Hz, Q 1/sqrt2) then high pass (38 Hz, Q 0.5), normalised by a0."""
    w0 = 2.0 * np.pi * (38.0 / rate)
    alpha = np.sin(w0) / (2.0 * 0.5)
    c = np.cos(w0)
    b = [(1 + c) / 2, -(1 + c), (1 + c) / 2]
    a = [1 + alpha, -2 * c, 1 - alpha]
    high_pass = np.array(b, dtype=np.float64) / a[0], np.array(a, dtype=np.float64) / a[0]
    return biqaud(4.0, 1500.0, 1.0 / np.sqrt(2.0), rate, "high_shelf"), high_pass


def _transition(sections, steps):
    """Zero-input state transition over `steps` samples of biquads (b, a) in series, transposed direct form II, states
    (s_0a, s_0b, s_1a, ...): y_k = b_k[0] y_(k-1) + s_ka, s_ka' = b_k[1] y_(k-1) - a_k[1] y_k + s_kb, s_kb' = b_k[2] y_(k-1) - a_k[2] y_k
    with y_(-1) = 0 (no input).  Every y_k is carried as a row of coefficients over the states."""
    D = 2 * len(sections)
    A = np.zeros((D, D))
    y = np.zeros(D)
    for k, (b, a) in enumerate(sections):
        ea, eb = np.zeros(D), np.zeros(D)
        ea[2 * k], eb[2 * k + 1] = 1.0, 1.0
        yk = b[0] * y + ea
        A[2 * k] = b[1] * y - a[1] * yk + eb
        A[2 * k + 1] = b[2] * y - a[2] * yk
        y = yk
    return np.linalg.matrix_power(A, int(steps))


class LoudnessNormalize(torch.nn.Module):
    """effects.py:619-629: scale to `target_lufs_db` by the BS.1770 integrated loudness (pyloudnorm.Meter).

    A ``(C, T)`` clip with C > 1 is measured jointly, as pyloudnorm measures a multichannel clip (block power = sum of the
    channels' mean squares) and scaled by one gain.  Known difference: a ``(B, C, T)`` batch is measured and scaled row by
    row, every channel on its own."""

    def __init__(self, sample_rate: float, target_lufs_db: float = -32.0) -> None:
        super().__init__()
        self.sample_rate, self.target_lufs_db = sample_rate, target_lufs_db
        self._cache = {}

    def _plan(self, T):
        """(hops per row, the launch arguments every measuring entry point takes ahead of the target level) of T-sample clips."""
        p = self._cache.get(T)
        if p is None:
            rate = self.sample_rate
            T_g, step = 0.4, 0.25
            if T < T_g * rate:
                raise ValueError("Audio must have length greater than the block size.")      # pyloudnorm's own error
            nblk = int(np.round(((T / rate - T_g) / (T_g * step))) + 1)
            hop = int(round(T_g * step * rate))
            for j in range(nblk):        # the kernel sums 100 ms hops: pyloudnorm's block bounds must be hop multiples
                if int(T_g * (j * step) * rate) != j * hop or int(T_g * (j * step + 1) * rate) != (j + 4) * hop:
                    raise NotImplementedError(f"loudness blocks are not multiples of a 100 ms hop at {rate} Hz")
            chunk = -(-T // 64)
            (b1, a1), (b2, a2) = _k_weighting(rate)
            M = _transition([(b1, a1), (b2, a2)], chunk)
            coef = np.concatenate([b1, a1, b2, a2, M.reshape(-1)]).astype(np.float64)
            p = nblk + 3, (chunk, hop, nblk + 3, nblk, 1.0 / (T_g * rate), coef)         # the cache keeps coef alive
            self._cache[T] = p
        return p

    def measure(self, clips):
        """(N, T) device clips -> (lufs (N,), gain (N,)) device tensors."""
        N, T = clips.shape
        _, plan = self._plan(T)
        hop_ws = scratch("rfx_fx_loudness_ws", N, T, *plan[:4], device=clips.device, dtype=torch.float64)
        lufs = torch.empty(N, device=clips.device, dtype=torch.float32)
        gain = torch.empty_like(lufs)
        launch("rfx_fx_loudness", clips, N, T, *plan, float(self.target_lufs_db), hop_ws, lufs, gain)
        return lufs, gain

    def measure_joint(self, clips):
        """(B, C, T) device clips -> (lufs (B,), gain (B,)): every clip's C channels measured together."""
        B, Ch, T = clips.shape
        _, plan = self._plan(T)
        hop_ws = scratch("rfx_fx_loudness_joint_ws", B, Ch, T, *plan[:4], device=clips.device, dtype=torch.float64)
        lufs = torch.empty(B, device=clips.device, dtype=torch.float32)
        gain = torch.empty_like(lufs)
        launch("rfx_fx_loudness_joint", clips, B, Ch, T, *plan, float(self.target_lufs_db), hop_ws, lufs, gain)
        return lufs, gain

    def normalize_rows(self, clips, state, rows=None):
        """One round's normalisation in one call: measure the n compact rows of ``clips`` (n, T) and store gain[i] * clips[i] into
        row rows[i] of ``state`` (N, T) (rows None: row i, state is (n, T)).  ``rows``: a host sequence (checked and uploaded) or
        a table from `row_table`.  The other rows of ``state`` are not touched.  Returns ``state``."""
        n, T = clips.shape
        if (clips.dtype != torch.float32 or state.dtype != torch.float32 or not clips.is_contiguous() or not state.is_contiguous()
                or state.dim() != 2 or state.shape[1] != T or state.device != clips.device):
            raise ValueError("normalize_rows takes contiguous fp32 (n, T) clips and a (N, T) state on one device")
        if rows is None:
            if state.shape[0] != n:
                raise ValueError("normalize_rows without a row table: state and clips need the same number of rows")
        else:
            if not isinstance(rows, torch.Tensor):
                rows = row_table(rows, state.shape[0], state.device)
            if rows.dtype != torch.int32 or rows.shape != (n,) or rows.device != state.device or n > state.shape[0]:
                raise ValueError(f"normalize_rows: a table of {tuple(rows.shape)} rows for {n} clips")
            if clips.untyped_storage().data_ptr() == state.untyped_storage().data_ptr():
                raise ValueError("normalize_rows: the clips must live outside the state buffer")
        nhop, plan = self._plan(T)
        ws = torch.empty(query("rfx_fx_normalize_ws_bytes", n, nhop) // 8 + 1, device=clips.device, dtype=torch.float64)
        launch("rfx_fx_normalize_rows", clips, state, rows, n, T, *plan, float(self.target_lufs_db), ws)
        return state

    @staticmethod
    def _scale(rows, gain):
        """(N, T) rows times their (N,) gains, as a new tensor."""
        y = torch.empty_like(rows)
        launch("rfx_fx_scale", rows, y, rows.shape[0], rows.shape[1], gain)
        return y

    def normalize_joint(self, clips):
        """(B, C, T) contiguous fp32 device clips -> the same shape: every clip measured jointly and scaled by its one gain."""
        B, Ch, T = clips.shape
        _, gain = self.measure_joint(clips)
        return self._scale(clips.view(B * Ch, T), gain.repeat_interleave(Ch)).view(B, Ch, T)

    def forward(self, x: torch.Tensor):
        _check_clips(x)
        rows = _rows(x)
        if x.dim() == 2 and x.shape[0] != 1:
            return self.normalize_joint(rows.unsqueeze(0)).view(x.shape)
        return self._scale(rows, self.measure(rows)[1]).view(x.shape)


_RBJ = {    # RBJ cookbook biquads as (b0, b1, b2, a0, a1, a2) of (A, cos w0, alpha, sqrt A)
    "high_shelf": lambda A, c, al, sA: (A * ((A + 1) + (A - 1) * c + 2 * sA * al), -2 * A * ((A - 1) + (A + 1) * c),
                                        A * ((A + 1) + (A - 1) * c - 2 * sA * al), (A + 1) - (A - 1) * c + 2 * sA * al,
                                        2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - 2 * sA * al),
    "low_shelf": lambda A, c, al, sA: (A * ((A + 1) - (A - 1) * c + 2 * sA * al), 2 * A * ((A - 1) - (A + 1) * c),
                                       A * ((A + 1) - (A - 1) * c - 2 * sA * al), (A + 1) + (A - 1) * c + 2 * sA * al,
                                       -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - 2 * sA * al),
    "peaking": lambda A, c, al, sA: (1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A),
}


def biqaud(gain_db: float, cutoff_freq: float, q_factor: float, sample_rate: float, filter_type: str):
    """effects.py:37-91 (the reference's spelling): (b, a) float64 coefficients, normalised by a0, of a "low_shelf",
    "high_shelf" or "peaking" biquad."""
    A = 10 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * (cutoff_freq / sample_rate)
    alpha = np.sin(w0) / (2.0 * q_factor)
    b0, b1, b2, a0, a1, a2 = _RBJ[filter_type](A, np.cos(w0), alpha, np.sqrt(A))
    return np.array([b0, b1, b2]) / a0, np.array([a0, a1, a2]) / a0


def _eq_sections(p, sample_rate):
    """The biquads of one parametric_eq parameter set, in the reference's order: low shelf, bands, high shelf."""
    secs = [biqaud(p["low_shelf_gain_db"], p["low_shelf_cutoff_freq"], p["low_shelf_q_factor"], sample_rate, "low_shelf")]
    secs += [biqaud(g, f, q, sample_rate, "peaking")
             for g, f, q in zip(p["band_gains_db"], p["band_cutoff_freqs"], p["band_q_factors"])]
    secs.append(biqaud(p["high_shelf_gain_db"], p["high_shelf_cutoff_freq"], p["high_shelf_q_factor"], sample_rate, "high_shelf"))
    return secs


def _eq_render(clips, params, sample_rate):
    """(N, T) device clips, one parametric_eq parameter set per row -> (N, T): rfx_fx_eq with the per-row transition."""
    N, T = clips.shape
    chunk = -(-T // 64)
    rows, done = [], {}
    for p in params:
        if id(p) not in done:
            secs = _eq_sections(p, sample_rate)
            if not 2 <= len(secs) <= 8:
                raise ValueError(f"parametric EQ: 0 to 6 bands, got {len(secs) - 2}")
            coef = [np.array([b[0], b[1], b[2], a[1], a[2]]) for b, a in secs]
            done[id(p)] = (len(secs), np.concatenate(coef + [_transition(secs, chunk).reshape(-1)]))
        rows.append(done[id(p)])
    nsec = rows[0][0]
    if any(n != nsec for n, _ in rows):
        raise ValueError("parametric EQ: every clip of one launch needs the same number of bands")
    coef = torch.from_numpy(np.stack([r for _, r in rows])).to(clips.device)
    y = torch.empty_like(clips)
    launch("rfx_fx_eq", clips, y, N, T, nsec, chunk, coef)
    return y


def parametric_eq(x, sample_rate: float, low_shelf_gain_db: float = 0.0, low_shelf_cutoff_freq: float = 80.0,
                  low_shelf_q_factor: float = 0.707, band_gains_db=(0.0,), band_cutoff_freqs=(300.0,), band_q_factors=(0.707,),
                  high_shelf_gain_db: float = 0.0, high_shelf_cutoff_freq: float = 1000.0, high_shelf_q_factor: float = 0.707,
                  dtype=np.float32):
    """effects.py:94-150: low shelf -> bands -> high shelf along the last axis, rendered on the device in fp64.  A numpy array
    (read as fp32) gives a numpy array of `dtype`; a CUDA tensor gives a CUDA fp32 tensor."""
    assert len(band_gains_db) == len(band_cutoff_freqs) == len(band_q_factors)
    p = dict(low_shelf_gain_db=low_shelf_gain_db, low_shelf_cutoff_freq=low_shelf_cutoff_freq, low_shelf_q_factor=low_shelf_q_factor,
             band_gains_db=list(band_gains_db), band_cutoff_freqs=list(band_cutoff_freqs), band_q_factors=list(band_q_factors),
             high_shelf_gain_db=high_shelf_gain_db, high_shelf_cutoff_freq=high_shelf_cutoff_freq,
             high_shelf_q_factor=high_shelf_q_factor)
    is_np = isinstance(x, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() if is_np else x
    require_device(t)
    flat = _rows(t)
    y = _eq_render(flat, [p] * flat.shape[0], sample_rate).view(t.shape)
    return y.cpu().numpy().astype(dtype) if is_np else y


class RandomParametricEQ(_RandomEffect):
    defaults = dict(num_bands=3, min_gain_db=-6.0, max_gain_db=6.0, min_cutoff_freq=1000.0, max_cutoff_freq=10000.0,
                    min_q_factor=0.1, max_q_factor=4.0)

    def draw(self):                                    # effects.py:182-198
        p = dict(low_shelf_gain_db=rand(self.min_gain_db, self.max_gain_db), low_shelf_cutoff_freq=loguniform(20.0, 200.0),
                 low_shelf_q_factor=rand(self.min_q_factor, self.max_q_factor))
        p.update(high_shelf_gain_db=rand(self.min_gain_db, self.max_gain_db), high_shelf_cutoff_freq=loguniform(8000.0, 16000.0),
                 high_shelf_q_factor=rand(self.min_q_factor, self.max_q_factor))
        p.update(band_gains_db=[], band_cutoff_freqs=[], band_q_factors=[])
        for _ in range(self.num_bands):
            p["band_gains_db"].append(rand(self.min_gain_db, self.max_gain_db))
            p["band_cutoff_freqs"].append(loguniform(self.min_cutoff_freq, self.max_cutoff_freq))
            p["band_q_factors"].append(rand(self.min_q_factor, self.max_q_factor))
        return p

    def render(self, clips, params):
        return _eq_render(clips, params, self.sample_rate)


def _widener_gains(width):
    """stereo_widener's mid / side factors, evaluated in the type of `width` like the reference's scalars."""
    return 2 * (1 - width), 2 * width


def _check_stereo(x):
    require_device(x)
    if x.dim() not in (2, 3) or x.shape[-2] != 2:
        raise ValueError(f"the stereo widener takes (2, samples) or (batch, 2, samples), got {tuple(x.shape)}")


def stereo_widener(x: torch.Tensor, width):
    """effects.py:217-235 on the device: x (2, T) or (B, 2, T) CUDA, width a number or one per clip.  Returns a new tensor."""
    _check_stereo(x)
    flat = _rows(x)
    widths = list(width) if isinstance(width, (list, tuple)) else [width] * (flat.shape[0] // 2)
    return _widener_render(flat, widths).view(x.shape)


def _widener_render(rows, widths):
    g = [_widener_gains(w) for w in widths]
    gm, gs = _vec([a for a, _ in g], rows.device), _vec([b for _, b in g], rows.device)
    y = torch.empty_like(rows)
    launch("rfx_fx_widener", rows, y, rows.shape[0] // 2, rows.shape[1], gm, gs)
    return y


class RandomStereoWidener(_RandomEffect):
    """effects.py:238-252.  Stereo only: any other channel count raises ValueError (upstream: IndexError for mono, channels
    beyond two silently dropped)."""
    defaults = dict(min_width=0.0, max_width=1.0)
    check_input = staticmethod(_check_stereo)

    def draw(self):                                    # effects.py:251
        return dict(width=rand(self.min_width, self.max_width))

    def render(self, clips, params):
        """clips: (2 N, T), rows 2i and 2i + 1 = left and right of clip i."""
        if clips.shape[0] % 2:
            raise ValueError("the stereo widener renders (left, right) row pairs")
        return _widener_render(clips, [p["width"] for p in params[::2]])


class RandomVolumeAutomation(_RandomEffect):
    """effects.py:255-294: piecewise-linear dB ramps over Dirichlet-drawn segments.  Like upstream, ``forward`` scales ``x`` IN
    PLACE and returns it."""
    defaults = dict(min_segments=1, max_segments=3, min_gain_db=-6.0, max_gain_db=6.0)
    in_place = True

    def draw(self, T):                                 # effects.py:274-291
        n = randint(self.min_segments, self.max_segments)
        lengths = (T * np.random.dirichlet([rand(0, 10) for _ in range(n)], 1)).astype("int")[0]
        gains = [rand(self.min_gain_db, self.max_gain_db) for _ in range(n)]
        return dict(num_segments=int(n), segment_lengths=[int(v) for v in lengths], end_gains_db=gains)

    def draw_for(self, T):                             # the one draw that depends on the clip: segment lengths in samples
        return self.draw(T)

    def render(self, clips, params):
        """Scales the (N, T) fp32 clips in place and returns them."""
        S = max(p["num_segments"] for p in params)
        if S > 64:
            raise ValueError("volume automation: at most 64 segments")
        ends, d0, d1 = [], [], []
        for p in params:
            e = np.cumsum(p["segment_lengths"]).tolist()
            g = list(p["end_gains_db"])
            pad = S - len(e)                           # zero-length segments after the last one
            ends += e + [e[-1]] * pad
            d0 += [0.0] + g[:-1] + [0.0] * pad
            d1 += g + [0.0] * pad
        dev = clips.device
        # launch holds the three tables until the launch is queued: a freed block would be handed to the next _vec
        launch("rfx_fx_volume", clips, clips.shape[0], clips.shape[1], S, _vec(ends, dev, torch.int32), _vec(d0, dev), _vec(d1, dev))
        return clips


class RandomPedalboardPhaser(_RandomEffect):
    defaults = dict(min_rate_hz=0.25, max_rate_hz=5.0, min_depth=0.1, max_depth=0.6, min_centre_frequency_hz=200.0,
                    max_centre_frequency_hz=600.0, min_feedback=0.1, max_feedback=0.6, min_mix=0.1, max_mix=0.7)

    def draw(self):                                    # effects.py:448-454; the centre draw spans (min, min) upstream
        return dict(rate_hz=rand(self.min_rate_hz, self.max_rate_hz), depth=rand(self.min_depth, self.max_depth),
                    centre_frequency_hz=rand(self.min_centre_frequency_hz, self.min_centre_frequency_hz),
                    feedback=rand(self.min_feedback, self.max_feedback), mix=rand(self.min_mix, self.max_mix))

    def render(self, clips, params):
        dev = clips.device
        N, T = clips.shape
        cols = [_col(params, k, dev) for k in ("rate_hz", "depth", "centre_frequency_hz", "feedback", "mix")]
        ws = torch.empty(query("rfx_fx_phaser_ws_floats", N, T), device=dev, dtype=torch.float32)
        y = torch.empty_like(clips)
        launch("rfx_fx_phaser", clips, y, ws, N, T, float(self.sample_rate), *cols)
        return y


class RandomPedalboardLimiter(_RandomEffect):
    defaults = dict(min_threshold_db=-32.0, max_threshold_db=-6.0, min_release_ms=10.0, max_release_ms=300.0)

    def draw(self):                                    # effects.py:486-487
        return dict(threshold_db=rand(self.min_threshold_db, self.max_threshold_db),
                    release_ms=rand(self.min_release_ms, self.max_release_ms))

    def stages(self, p):
        """juce::dsp::Limiter::update: the two compressor stages' parameters and the make-up gain of one draw."""
        makeup = min(10.0 ** (10.0 * (1.0 - 1.0 / 4.0) / 40.0), 10.0 ** (-p["threshold_db"] / 20.0))
        return (dict(threshold_db=-10.0, ratio=4.0, attack_ms=2.0, release_ms=200.0),
                dict(threshold_db=p["threshold_db"], ratio=1000.0, attack_ms=0.001, release_ms=p["release_ms"]), makeup)

    def render(self, clips, params):
        N, T = clips.shape
        cols = []
        for p in params:
            s1, s2, makeup = self.stages(p)
            col = []
            for s in (s1, s2):
                col += [10.0 ** (s["threshold_db"] / 20.0), s["ratio"], _ballistics_cte(s["attack_ms"], self.sample_rate),
                        _ballistics_cte(s["release_ms"], self.sample_rate)]
            cols.append(col + [makeup])
        prm = _vec(np.asarray(cols).T.copy(), clips.device)
        ws = scratch("rfx_fx_limiter_ws", N, T, device=clips.device, dtype=torch.float32)
        y = torch.empty_like(clips)
        launch("rfx_fx_limiter", clips, y, ws, N, T, prm)
        return y


class RandomAudioEffectsChannel(torch.nn.Module):
    """effects.py:632-696: the reference's augmentation chain on stereo clips -- ten stages, each applied with its probability
    (torchvision RandomApply: skipped when p < torch.rand(1)), then LoudnessNormalize measured jointly over both channels.

    ``forward`` takes ``(2, T)`` or ``(B, 2, T)`` CUDA tensors and returns a new tensor.  Draws go clip by clip, so a batch equals
    B successive single-clip calls under the same seed; each stage then renders in ONE launch over the clips that drew it."""

    def __init__(self, sample_rate: float, parametric_eq_prob: float = 0.7, distortion_prob: float = 0.01, delay_prob: float = 0.1,
                 chorus_prob: float = 0.01, phaser_prob: float = 0.01, compressor_prob: float = 0.4, reverb_prob: float = 0.2,
                 stereo_widener_prob: float = 0.3, limiter_prob: float = 0.3, vol_automation_prob: float = 0.7,
                 target_lufs_db: float = -32.0) -> None:
        super().__init__()
        self.sample_rate = sample_rate
        self.stages = [(RandomParametricEQ(sample_rate), parametric_eq_prob), (RandomPedalboardDistortion(sample_rate), distortion_prob),
                       (RandomPedalboardDelay(sample_rate), delay_prob), (RandomPedalboardChorus(sample_rate), chorus_prob),
                       (RandomPedalboardPhaser(sample_rate), phaser_prob), (RandomPedalboardCompressor(sample_rate), compressor_prob),
                       (RandomPedalboardReverb(sample_rate), reverb_prob), (RandomStereoWidener(sample_rate), stereo_widener_prob),
                       (RandomPedalboardLimiter(sample_rate), limiter_prob), (RandomVolumeAutomation(sample_rate), vol_automation_prob)]
        self.normalize = LoudnessNormalize(sample_rate, target_lufs_db=target_lufs_db)

    def plan(self, B, T):
        """The host-side draws of B clips of T samples: per clip, the (stage class name, parameters) that fire, in order."""
        out = []
        for _ in range(B):
            fired = []
            for fx, p in self.stages:
                if p < torch.rand(1):
                    continue
                fired.append((type(fx).__name__, fx.draw_for(T)))
            out.append(fired)
        return out

    def forward(self, x: torch.Tensor):
        _check_stereo(x)
        B, Ch, T = (1,) + tuple(x.shape) if x.dim() == 2 else tuple(x.shape)
        plan = self.plan(B, T)
        self.last_plan = plan
        y = x.reshape(B * Ch, T).to(torch.float32).clone()
        for fx, _ in self.stages:
            name = type(fx).__name__
            sel = [(b, prm) for b, fired in enumerate(plan) for n, prm in fired if n == name]
            if not sel:
                continue
            params = [prm for _, prm in sel for _ in range(Ch)]
            if len(sel) == B:
                y = fx.render(y, params)
            else:
                idx = torch.tensor([b * Ch + c for b, _ in sel for c in range(Ch)], device=y.device)
                y.index_copy_(0, idx, fx.render(y.index_select(0, idx), params))
        return self.normalize.normalize_joint(y.view(B, Ch, T)).view(x.shape)


# label order: column k of dry / wet label tensors (effects.py:699-707)
Pedalboard_Effects = [
    RandomPedalboardReverb,
    RandomPedalboardChorus,
    RandomPedalboardDelay,
    RandomPedalboardDistortion,
    RandomPedalboardCompressor,
]
