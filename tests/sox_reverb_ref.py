"""Sample-by-sample numpy restatement of SoX's `reverb` effect as the reference uses it (remfx/effects.py:516-572:
`reverb <reverberance> <hf_damping> <room_scale> <stereo_depth> <pre_delay> --wet-only` through torchaudio, then a wet / dry mix
in torch) for tests/test_sox_reverb_cpu.py and tests/test_gpu_sox_reverb.py.  Test infrastructure only.

SoX and torchaudio are not available to pin it: this is SoX's reverb.c as recalled, parity unpinned.

  delay    = (int)(pre_delay_ms / 1000 * sr + .5)            samples of silence fed first
  scale    = room_scale / 100 * .9 + .1;   depth = stereo_depth / 100
  a = -1 / ln(1 - .3);  b = 100 / (ln(1 - .98) * a + 1);  feedback = 1 - exp((reverberance - b) / (a * b))      (0.3 .. 0.98)
  damp     = hf_damping / 100 * .3 + .2;   gain = .015      (wet gain 0 dB);   feedback, damp and gain are stored as C floats
  bank(offset): 8 combs {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617} of (int)(scale * r * (tuning + 12 * offset) + .5) samples
                and 4 all-passes {225, 341, 441, 556} of (int)(r * (tuning + 12 * offset) + .5), r = sr / 44100
      comb:    o = buf[p]; store = o + (store - o) * damp; buf[p] = in + store * feedback; return o
      allpass: o = buf[p]; buf[p] = in + .5 * o; return o - in
      out = gain * allpass_0(allpass_1(allpass_2(allpass_3(comb_7 + comb_6 + ... + comb_0))))      (both loops run from the last
      filter to the first; float arithmetic)
  every input channel is clipped to [-1, 1] (conversion to SoX samples), delayed, and fed to two banks with offsets 0 and depth;
  wet channel w = bank w of the one input channel, or .5 * (channel 0's bank w + channel 1's bank w); clipped to [-1, 1] on the way
  back; the input's length (no drain).  Not modelled: the quantisation to 32-bit integer samples at both conversions.
"""
import math

import numpy as np

COMBS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASSES = (225, 341, 441, 556)
STEREO_ADJUST = 12
GAIN = 0.015


def plan(reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, sample_rate):
    """The derived quantities of one parameter set: delay (samples), feedback, damp, gain (as float32 values, SoX keeps them in
    floats), and per bank (offsets 0 and depth) the 8 comb and 4 all-pass lengths."""
    scale = room_scale / 100.0 * 0.9 + 0.1
    depth = stereo_depth / 100.0
    a = -1.0 / math.log(1.0 - 0.3)
    b = 100.0 / (math.log(1.0 - 0.98) * a + 1.0)
    r = sample_rate * (1.0 / 44100.0)
    banks = []
    for offset in (0.0, depth):
        banks.append(dict(combs=[int(scale * r * (t + STEREO_ADJUST * offset) + 0.5) for t in COMBS],
                          allpasses=[int(r * (t + STEREO_ADJUST * offset) + 0.5) for t in ALLPASSES]))
    return dict(delay=int(pre_delay / 1000.0 * sample_rate + 0.5),
                feedback=float(np.float32(1.0 - math.exp((reverberance - b) / (a * b)))),
                damp=float(np.float32(high_freq_damping / 100.0 * 0.3 + 0.2)), gain=float(np.float32(GAIN)), banks=banks)


def bank(x, combs, allpasses, feedback, damp, gain, dtype=np.float64):
    """One filter bank over the (already clipped and delayed) samples x, in `dtype` arithmetic."""
    f = float if np.dtype(dtype) == np.float64 else np.float32          # python floats are IEEE doubles
    fb, dp, gn, half = f(feedback), f(damp), f(gain), f(0.5)
    cbuf = [[f(0.0)] * n for n in combs]
    abuf = [[f(0.0)] * n for n in allpasses]
    cpos, apos = [0] * len(combs), [0] * len(allpasses)
    store = [f(0.0)] * len(combs)
    y = np.empty(len(x), dtype=dtype)
    xs = [f(v) for v in np.asarray(x, dtype=dtype)]
    for n, inp in enumerate(xs):
        out = f(0.0)
        for j in range(len(combs) - 1, -1, -1):
            buf, p = cbuf[j], cpos[j]
            o = buf[p]
            s = o + (store[j] - o) * dp
            store[j] = s
            buf[p] = inp + s * fb
            cpos[j] = p + 1 if p + 1 < len(buf) else 0
            out = out + o
        for j in range(len(allpasses) - 1, -1, -1):
            buf, p = abuf[j], apos[j]
            o = buf[p]
            buf[p] = out + half * o
            apos[j] = p + 1 if p + 1 < len(buf) else 0
            out = o - out
        y[n] = out * gn
    return y


def wet_unclipped(x, sample_rate, reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, dtype=np.float64):
    """x: (channels, T), 1 or 2 channels -> (2, T) wet signal before the clip to [-1, 1]."""
    x = np.asarray(x, dtype=dtype)
    assert x.ndim == 2 and x.shape[0] in (1, 2) and stereo_depth > 0
    p = plan(reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, sample_rate)
    T = x.shape[1]
    wet = np.zeros((2, T), dtype=dtype)
    for c in range(x.shape[0]):
        fed = np.zeros(T, dtype=dtype)
        d = min(p["delay"], T)
        fed[d:] = np.clip(x[c], -1.0, 1.0)[:T - d]
        for w in range(2):
            wet[w] += bank(fed, p["banks"][w]["combs"], p["banks"][w]["allpasses"], p["feedback"], p["damp"], p["gain"], dtype)
    if x.shape[0] == 2:
        wet *= np.dtype(dtype).type(0.5)
    return wet


def sox_reverb(x, sample_rate, reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, dtype=np.float64):
    """The wet-only SoX output, (2, T), clipped to [-1, 1]."""
    return np.clip(wet_unclipped(x, sample_rate, reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, dtype),
                   -1.0, 1.0)


def random_sox_reverb(x, sample_rate, reverberance, high_freq_damping, room_scale, stereo_depth, wet_dry, pre_delay,
                      dtype=np.float64):
    """RandomSoxReverb.forward for one drawn parameter set: x * (1 - wet_dry) + y * wet_dry, a mono x broadcast over both channels."""
    x = np.asarray(x, dtype=dtype)
    y = sox_reverb(x, sample_rate, reverberance, high_freq_damping, room_scale, stereo_depth, pre_delay, dtype)
    t = np.dtype(dtype).type
    return x * t(1.0 - wet_dry) + y * t(wet_dry)
