"""Float64 restatements for tests/test_gpu_effects_channel.py (test infrastructure only), and the seeded inputs that
tests/golden/fx_channel.npz was recorded on (scripts/gen_fx_golden.py).

Recalled sources (pedalboard / JUCE are not available to pin them, as for oracle/ref_effects.py):
  * juce::dsp::Phaser: 6 FirstOrderTPTFilter all-passes (G = g / (1 + g), g = tan(pi fc / sr); v = G (u - s), y = v + s, s = y + v,
    output 2 y - u).  The cutoff is updated every 4th sample (maxUpdateCounter = 4) from a sine Oscillator prepared at sr / 4
    whose phase starts at -pi; the LFO times depth / 2 (oscVolume) plus normCentre = mapFromLog10(centre, 20, min(20000, 0.49 sr)),
    clamped to [0, 1], mapped back with mapToLog10.  Feedback is NEGATIVE: the stage input is x - lastOutput with
    lastOutput = output * feedback.  Linear dry / wet mix.  prepare() ends in reset(), which snaps every SmoothedValue (osc
    frequency, oscVolume, feedback, mix) to its target, so the 50 ms ramps do not act on a freshly prepared plugin.
  * juce::dsp::Limiter: Compressor(-10 dB, ratio 4, attack 2 ms, release 200 ms) -> Compressor(threshold_db, ratio 1000,
    attack 0.001 ms, release_ms) -> make-up gain min(10^(10 (1 - 1/4) / 40), 10^(-threshold_db / 20)) -> clip to [-1, 1].
  * pyloudnorm.Meter on a multichannel clip: block power = sum over channels (weight 1 for L, R) of the mean square.
"""
import numpy as np
import scipy.signal
import torch

from oracle import ref_effects as R

SR = 48000


def fixture_input(seed, channels, T):
    """The inputs of tests/golden/fx_channel.npz: 0.3 x standard normal from a seeded generator."""
    return 0.3 * torch.randn(channels, T, generator=torch.Generator().manual_seed(seed))


def eq(x, sections):
    """scipy.signal.lfilter cascade in float64 along the last axis (the reference's parametric_eq before its fp32 cast)."""
    y = np.asarray(x, dtype=np.float64)
    for b, a in sections:
        y = scipy.signal.lfilter(b, a, y)
    return y


def phaser(x, sample_rate, rate_hz, depth, centre_frequency_hz, feedback, mix):
    x = np.asarray(x, dtype=np.float64)
    fmax = min(20000.0, 0.49 * sample_rate)
    nc = np.log10(centre_frequency_hz / 20.0) / np.log10(fmax / 20.0)
    s = [0.0] * 6
    last, G = 0.0, 0.0
    y = np.empty_like(x)
    for n in range(x.shape[-1]):
        if n % 4 == 0:
            lfo = np.sin(2.0 * np.pi * rate_hz * (n // 4) / (sample_rate / 4.0) - np.pi) * depth * 0.5
            f = 20.0 * (fmax / 20.0) ** min(max(lfo + nc, 0.0), 1.0)
            g = np.tan(np.pi * f / sample_rate)
            G = g / (1.0 + g)
        u = x[n] - last
        for k in range(6):
            v = G * (u - s[k])
            yk = v + s[k]
            s[k] = yk + v
            u = 2.0 * yk - u
        last = u * feedback
        y[n] = (1.0 - mix) * x[n] + mix * u
    return y


def limiter(x, sample_rate, threshold_db, release_ms):
    y = R.compressor(x, sample_rate, -10.0, 4.0, 2.0, 200.0)
    y = R.compressor(y, sample_rate, threshold_db, 1000.0, 0.001, release_ms)
    makeup = min(10.0 ** (10.0 * (1.0 - 1.0 / 4.0) / 40.0), 10.0 ** (-threshold_db / 20.0))
    return np.clip(y * makeup, -1.0, 1.0)


def integrated_loudness_multichannel(x, rate):
    """pyloudnorm.Meter(rate).integrated_loudness of a (C, T) clip, channel weights 1."""
    x = np.asarray(x, dtype=np.float64)
    T_g, step = 0.4, 0.25
    for b, a in R.k_weighting_coefficients(rate):
        x = scipy.signal.lfilter(b, a, x, axis=-1)
    dur = x.shape[-1] / rate
    nblk = int(np.round(((dur - T_g) / (T_g * step))) + 1)
    z = np.zeros((x.shape[0], nblk))
    for j in range(nblk):
        lo, hi = int(T_g * (j * step) * rate), int(T_g * (j * step + 1) * rate)
        z[:, j] = (1.0 / (T_g * rate)) * np.sum(np.square(x[:, lo:hi]), axis=-1)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z.sum(axis=0))
        J = [j for j in range(nblk) if l[j] >= -70.0]
        gamma_r = -0.691 + 10.0 * np.log10(np.mean(z[:, J], axis=1).sum()) - 10.0
        J = [j for j in range(nblk) if l[j] > gamma_r and l[j] > -70.0]
        return -0.691 + 10.0 * np.log10(np.mean(z[:, J], axis=1).sum())
