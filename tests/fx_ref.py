"""fp64 statements of the operation of every entry point of remfx_amd/csrc/fx.hip (distortion, delay, chorus, compressor, limiter, reverb,
SoX reverb bank and mix, loudness single and joint, scale, normalize_rows, EQ, widener, volume, phaser), written from the formulas in
fx.hip's comments and the header as the plain per-sample recurrence on the logical signal: numpy only, vectorised over ROWS and never
over time where there is a recurrence.  None of the kernels' decompositions is used: no chunked two-pass filter, no wave scan, no
closed-form unrolling of the delay line.  The host-side inputs (RBJ biquads, the chunk-step state transition, ballistics constants, the
limiter's nine rows, SoX geometry rows) are built here, in fp64, without remfx_amd.effects.

forms_*() mirror every launch condition and in-kernel branch and say what a case reaches; restate_*() are float32 evaluations, in
fixed-order IEEE arithmetic (numpy float32 scalars and arrays, fma = one rounding of the fp64 product-sum), of the kernels' arithmetic
decomposition -- never a kernel, never torch -- and give the floors; the *_CASES tables are what the CPU and the GPU test walk.

Bounds, eps32 = 2^-23, one half-ulp = 2^-24 relative; none is measured on a kernel, every one is a per-element vector:
  exact     scale with and without a row table (one rounding of an fp64-exact product); the tail of volume past the table; mix = 0 of
            chorus and phaser ((1 - 0) x + 0 pop = x for finite pop, fused or not); the compressor / limiter below the threshold
            (gain 1); widener against restate_widener: the build has no fast-math flag, so hipcc's default of correctly rounded fp32
            division holds, and fx_rounded keeps every product from being fused: the float32 restatement in the reference's order
            is what the kernel computes, bit for bit.
  counted   delay: acc takes one fma per tap (a half-ulp of sum |terms| each) and the k-th weight fb^(k-1) carries k - 1 roundings;
            the mix adds 3 half-ulps of |(1 - m) x| and 2 of |m| sum |terms|.
            fx_sox_mix_kernel given the banks in ws: 3 half-ulps of |x dry|, 2 (3 with Cin = 2) of |wet wd|.
            fx_comp_gain given the envelope: 1 / th, e * ti (2 half-ulps in the base, times |ex|), ex = 1 / ratio - 1 (2 roundings, times
            |ln base|), powf by the K rule, the product with x.  The limiter's output given stage 2's envelope and stage 1's output
            (both stay in ws): the same plus the make-up product; the clip is 1-Lipschitz.
            volume: the dB ramp v carries 3 half-ulps of |end - start| and one of |v|, v / 20 one more; 10^u turns an absolute
            error du into a relative one of ln(10) du; powf by the K rule; the product with x.
  fp64 sums EQ and K-weighting: every rounding of either pass or of the chain of chunk states is a perturbation of the state that the
            filter itself carries on: 2^-53 x (operations per sample) x sum_n |A^n| (the state transition's own l-infinity gain,
            computed here) x the largest intermediate value, plus the final fp32 rounding for EQ.  Hop sums: 2 |w| dw per sample and
            2^-53 per addition.  LUFS: the hop bound through 10 log10, plus its fp32 rounding; gain: counted, powf by the K rule.
  K rule    K eps32 magnitude, K = 8 floor + 8 with the floor of FLOOR below (test_fx_ref_cpu.py recomputes every one from restate_*):
            distortion (tanhf), the compressor envelope, chorus, reverb, the SoX bank, the phaser and its coefficient stream, powf.
            For a recurrence the magnitude is the majorant of the same recurrence, run in fp64 on |x| with |coefficients|; the phaser's
            all-pass chain has no finite majorant of that kind (2 y - u with |.| grows by (1 + 2 G) per sample), so its magnitude is the
            running maximum of every intermediate value of the fp64 run over 1 - |feedback|.  Chorus adds dd |slope| carried through
            the same recurrence: dd is the fp32 uncertainty of the delay in samples, slope the larger difference of the interpolated
            pair and of its two neighbour pairs (the interpolation is continuous across an integer delay, so no sample is excluded).

Decisions that are not continuous: only the loudness gates; loud_margins() gives every block's distance from -70 LUFS and from the
relative gate and the margin the hop-sum bound implies, asserted on the CPU for every loudness case.  The compressor's attack / release
choice is continuous: with a between the two envelopes y (fp64) and y' (float32), the branches differ by cr p + ca q with p + q =
|y - y'|, no more than max(ca, cr) |y - y'|: a contraction like either branch.  The threshold branch is continuous (pow(1, ex) = 1) and
is judged given the SAME envelope bits; the clip is 1-Lipschitz."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -23
HALF = 2.0 ** -24
TINY = 2.0 ** -149
U64 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10                     # second-order terms of a counted bound

# floors in units of eps32 x magnitude, measured on restate_* over the case tables (printed by test_floors_are_below_the_table) and
# rounded up to the next half; K = 8 floor + 8.  Measured: tanh 0.69, powf 0.85, comp_env 0.39, chorus 0.83, reverb 0.82, sox_bank 0.69,
# phaser 1.78, phaser_coef 0.50
FLOOR = {"tanh": 1.0, "powf": 1.0, "comp_env": 0.5, "chorus": 1.0, "reverb": 1.0, "sox_bank": 1.0, "phaser": 2.0, "phaser_coef": 0.5}


def k_of(name):
    return 8.0 * FLOOR[name] + 8.0


def fma32(a, b, c):
    """one rounding of a b + c (the fp64 product of two float32 is exact; the double rounding of the sum is rarer than 2^-29)"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def signal(B, T, seed, amp=0.5, lo=0.05):
    """(B, T) float32, |x| in [lo amp, amp], no zeros"""
    g = np.random.default_rng(seed)
    return (g.uniform(lo, 1.0, (B, T)) * np.where(g.random((B, T)) < 0.5, -1.0, 1.0) * amp).astype(F32)


def uniform(n, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, n).astype(F32)


# ---- launch geometry -------------------------------------------------------------------------------------------------------------------
def fx_grid(T, per_block):
    return max(1, min(2048, -(-T // per_block)))


def forms_stream(kernel, T, per_block, vec, B=1, off=0):
    """a grid-stride stream over T: 256 threads, `per_block` samples per block and trip, 16-byte body and scalar tail where vec"""
    out = {kernel + ":first_trip"}
    if T > 2048 * per_block:
        out |= {kernel + ":second_trip", kernel + ":grid_capped"}
    if vec:
        out.add(kernel + (":tail_only" if T < 4 else ":body16"))
        if T % 4 and T >= 4:
            out.add(kernel + ":scalar_tail")
        if B > 1 and T % 4:
            out.add(kernel + ":rows_not_16B_aligned")
        if off % 4:
            out.add(kernel + ":payload_offset_%d" % (off % 4))
    return out


def forms_lanes(kernel, B, T=None):
    """one clip per lane, 64 per workgroup"""
    out = {kernel + ":workgroups_%s" % ("1" if B <= 64 else "2" if B <= 128 else "3"), kernel + (":partial_wave" if B % 64 else ":full_wave")}
    if T is not None:
        out.add(kernel + (":tail_only" if T < 32 else ":prefetch32"))
        if T >= 32 and T % 32:
            out.add(kernel + ":scalar_tail")
    return out


# ---- distortion ------------------------------------------------------------------------------------------------------------------------
DIST_CASES = (dict(B=1, T=3), dict(B=3, T=37), dict(B=2, T=64, off=1), dict(B=1, T=2048 * 1024 + 5), dict(B=2, T=130, off=3), dict(B=1, T=9, off=2))


def dist_data(c, seed=1):
    return signal(c["B"], c["T"], seed + c["T"], 2.0), uniform(c["B"], 0.1, 4.0, seed + 7)


def distortion(x, gain):
    return np.tanh(gain.astype(F64)[:, None] * x.astype(F64))


def distortion_bound(x, gain):
    u = gain.astype(F64)[:, None] * x.astype(F64)
    t = np.tanh(u)
    return k_of("tanh") * EPS32 * (np.abs(t) + np.abs(u) * (1.0 - t * t)) + TINY


def restate_distortion(x, gain):
    return np.tanh((gain[:, None] * x).astype(F32)).astype(F32)


def forms_distortion(c):
    return forms_stream("fx_distortion_kernel", c["T"], 1024, True, c["B"], c.get("off", 0))


# ---- widener ---------------------------------------------------------------------------------------------------------------------------
WIDE_CASES = (dict(B=1, T=3), dict(B=3, T=37), dict(B=2, T=64, off=1), dict(B=1, T=2048 * 1024 + 5), dict(B=2, T=130, off=2), dict(B=1, T=9, off=3))


def wide_data(c, seed=2):
    w = uniform(c["B"], 0.0, 1.0, seed + 3).astype(F64)
    return signal(c["B"] * 2, c["T"], seed + c["T"], 1.0).reshape(c["B"], 2, c["T"]), (2 * (1 - w)).astype(F32), (2 * w).astype(F32)


def widener(x, gm, gs):
    x, r2 = x.astype(F64), math.sqrt(2.0)
    mid = (x[:, 0] + x[:, 1]) / r2 * gm.astype(F64)[:, None]
    side = (x[:, 0] - x[:, 1]) / r2 * gs.astype(F64)[:, None]
    return np.stack([(mid + side) / r2, (mid - side) / r2], 1)


def restate_widener(x, gm, gs):
    """the reference's float32 operation order: every quotient, product, sum rounded on its own"""
    r2 = F32(1.41421356237309515)
    mid = ((x[:, 0] + x[:, 1]) / r2) * gm[:, None]
    side = ((x[:, 0] - x[:, 1]) / r2) * gs[:, None]
    return np.stack([(mid + side) / r2, (mid - side) / r2], 1).astype(F32)


def forms_widener(c):
    return forms_stream("fx_widener_kernel", c["T"], 1024, True, 2 * c["B"], c.get("off", 0))


# ---- scale -----------------------------------------------------------------------------------------------------------------------------
SCALE_CASES = (dict(B=3, T=37), dict(B=1, T=2048 * 256 + 100))


def scale_data(c, seed=3):
    return signal(c["B"], c["T"], seed + c["T"], 1.0), uniform(c["B"], 0.01, 30.0, seed)


def scale(x, gain):
    return gain.astype(F64)[:, None] * x.astype(F64)          # exact in fp64: the float32 result is its one rounding


def forms_scale(c, rows=False):
    return forms_stream("fx_scale_kernel", c["T"], 256, False) | {"fx_scale_kernel:" + ("row_table" if rows else "dense")}


# ---- delay -----------------------------------------------------------------------------------------------------------------------------
DELAY_CASES = (dict(B=6, T=50, D=(0, -3, 1, 7, 50, 60)), dict(B=1, T=2048 * 256 + 300, D=(200000,)))


def delay_data(c, seed=4):
    return (signal(c["B"], c["T"], seed + c["T"], 1.0), np.asarray(c["D"], np.int32), uniform(c["B"], 0.05, 0.9, seed + 1),
            uniform(c["B"], 0.0, 0.7, seed + 2))


def delay(x, D, fb, mix):
    """the line itself: delayed[n] = w[n - D], w[n] = x[n] + fb delayed[n], D samples at a time (they do not depend on each other).
    -> y, bound"""
    B, T = x.shape
    x64 = x.astype(F64)
    y, bound = np.empty((B, T)), np.empty((B, T))
    for b in range(B):
        d, f, m = int(D[b]), float(fb[b]), float(mix[b])
        dl, S, R = np.zeros(T), np.zeros(T), np.zeros(T)         # delayed, sum |terms|, sum (k - 1) |term_k|
        if d > 0:
            w, wa = x64[b].copy(), np.abs(x64[b])
            for n0 in range(d, T, d):
                n1 = min(n0 + d, T)
                dl[n0:n1] = w[n0 - d:n1 - d]
                S[n0:n1] = wa[n0 - d:n1 - d]
                R[n0:n1] = abs(f) * (R[n0 - d:n1 - d] + S[n0 - d:n1 - d])
                w[n0:n1] = x64[b, n0:n1] + f * dl[n0:n1]
                wa[n0:n1] = np.abs(x64[b, n0:n1]) + abs(f) * S[n0:n1]
        taps = np.arange(T) // d if d > 0 else np.zeros(T)
        y[b] = (1.0 - m) * x64[b] + m * dl
        acc_err = HALF * (taps * S + R)
        bound[b] = (HALF * (3.0 * abs(1.0 - m) * np.abs(x64[b]) + 2.0 * abs(m) * S) + abs(m) * acc_err) * SLACK + TINY
    return y, bound


def forms_delay(c):
    out = forms_stream("fx_delay_kernel", c["T"], 256, False)
    for d in c["D"]:
        out.add("fx_delay_kernel:" + ("D<=0" if d <= 0 else "D>=T" if d >= c["T"] else "0<D<T"))
        if d == 1:
            out.add("fx_delay_kernel:D==1")
    return out


# ---- volume ----------------------------------------------------------------------------------------------------------------------------
VOL_CASES = (
    dict(B=3, T=100, ends=((30, 30, 70), (1, 2, 100), (40, 90, 130))),
    dict(B=2, T=37, ends=((20,), (50,))),
    dict(B=1, T=200, ends=(tuple(3 * (i + 1) for i in range(64)),)),
    dict(B=1, T=2048 * 256 + 300, ends=((300000, 2048 * 256 + 400),)),
)


def vol_data(c, seed=5):
    S = len(c["ends"][0])
    return (signal(c["B"], c["T"], seed + c["T"], 1.0), np.asarray(c["ends"], np.int32), uniform(c["B"] * S, -6, 6, seed + 1).reshape(c["B"], S),
            uniform(c["B"] * S, -6, 6, seed + 2).reshape(c["B"], S))


def _vol_segments(ends, T):
    """per sample n < min(ends[-1], T): its segment (the first with n < end), the segment's start and length"""
    filled = min(int(ends[-1]), T)
    n = np.arange(filled)
    s = np.searchsorted(np.asarray(ends, np.int64), n, side="right")
    lo = np.where(s > 0, np.asarray(ends, np.int64)[np.maximum(s - 1, 0)], 0)
    return filled, n, s, lo, np.asarray(ends, np.int64)[s] - lo


def volume(x, ends, d0, d1):
    """-> y, bound (0 past the table: untouched)"""
    B, T = x.shape
    y, bound = x.astype(F64).copy(), np.zeros((B, T))
    for b in range(B):
        filled, n, s, lo, steps = _vol_segments(ends[b], T)
        st, en, i = d0[b].astype(F64)[s], d1[b].astype(F64)[s], n - lo
        step = np.where(steps > 1, (en - st) / np.maximum(steps - 1, 1), 0.0)
        v = np.where(steps > 1, np.where(i < steps // 2, st + step * i, en - step * (steps - i - 1)), st)
        dv = np.where(steps > 1, HALF * (3.0 * np.abs(en - st) + np.abs(v)), 0.0)
        du = dv / 20.0 + HALF * np.abs(v / 20.0)
        y[b, :filled] = x[b, :filled].astype(F64) * 10.0 ** (v / 20.0)
        bound[b, :filled] = np.abs(y[b, :filled]) * ((math.log(10.0) * du + HALF) * SLACK + k_of("powf") * EPS32) + TINY
    return y, bound


def restate_volume(x, ends, d0, d1):
    B, T = x.shape
    y = x.copy()
    for b in range(B):
        filled, n, s, lo, steps = _vol_segments(ends[b], T)
        st, en, i = d0[b][s], d1[b][s], n - lo
        step = ((en - st) / np.maximum(steps - 1, 1).astype(F32)).astype(F32)
        v = np.where(i < steps // 2, fma32(step, i.astype(F32), st), fma32(-step, (steps - i - 1).astype(F32), en))
        v = np.where(steps > 1, v, st).astype(F32)
        y[b, :filled] = x[b, :filled] * np.power(F32(10.0), (v / F32(20.0)).astype(F32)).astype(F32)
    return y


def forms_volume(c):
    T, S = c["T"], len(c["ends"][0])
    out = forms_stream("fx_volume_kernel", min(T, max(e[-1] for e in c["ends"])), 256, False)
    out.add("fx_volume_kernel:S_%s" % ("1" if S == 1 else "64" if S == 64 else "between"))
    for e in c["ends"]:
        out.add("fx_volume_kernel:table_ends_" + ("before_T" if e[-1] < T else "at_T" if e[-1] == T else "after_T"))
        lo = 0
        for end in e:
            steps = end - lo
            if steps == 0:
                out.add("fx_volume_kernel:zero_length_segment")
            elif steps == 1 and lo < T:
                out.add("fx_volume_kernel:steps==1")
            elif lo < T:
                out.add("fx_volume_kernel:first_half")
                if min(end, T) - lo > steps // 2:
                    out.add("fx_volume_kernel:second_half")
            lo = end
    return out


# ---- powf (the gain stages) -------------------------------------------------------------------------------------------------------------
def restate_powf(base, ex):
    return np.power(base.astype(F32), ex.astype(F32)).astype(F32)


def powf_data(seed=6):
    g = np.random.default_rng(seed)
    return (np.concatenate([g.uniform(1.0, 40.0, 4000), np.full(2000, 10.0)]).astype(F32),
            np.concatenate([g.uniform(-1.0, -0.2, 4000), g.uniform(-6.0, 2.0, 2000)]).astype(F32))


# ---- compressor ------------------------------------------------------------------------------------------------------------------------
def ballistics(ms, sr):
    """juce::dsp::BallisticsFilter: exp(-2 pi 1000 / (sr ms)), 0 below a microsecond"""
    return 0.0 if ms < 1e-3 else math.exp(-2.0 * math.pi * 1000.0 / (float(sr) * ms))


COMP_CASES = (dict(B=1, T=20), dict(B=3, T=77), dict(B=65, T=40), dict(B=130, T=100), dict(B=1, T=2048 * 256 + 40), dict(B=64, T=36))


def comp_data(c, seed=7):
    B, T = c["B"], c["T"]
    g = np.random.default_rng(seed + T)
    x = signal(B, T, seed + T + 1, 1.0, 0.001)
    x *= np.repeat(g.choice([0.02, 1.0], (B, -(-T // 8))), 8, axis=1)[:, :T].astype(F32)     # loud and quiet stretches: both branches of both choices
    sr = 8000.0
    ca = np.asarray([ballistics(v, sr) for v in g.uniform(1.0, 50.0, B)], F32)
    cr = np.asarray([ballistics(v, sr) for v in g.uniform(10.0, 250.0, B)], F32)
    thr = (10.0 ** (g.uniform(-42.0, -6.0, B) / 20.0)).astype(F32)
    return x, thr, g.uniform(1.5, 4.0, B).astype(F32), ca, cr


def comp_env(x, ca, cr):
    """env[n] = a + c (env[n - 1] - a), a = |x[n]|, c = attack where a > env[n - 1].  -> env, its majorant G[n] = max(a, env[n - 1]) +
    max(ca, cr) G[n - 1] (what a step's three roundings are proportional to, carried on by the contraction)"""
    B, T = x.shape
    a = np.abs(x.astype(F64))
    env, mag = np.empty((B, T)), np.empty((B, T))
    if B == 1:                                                  # python floats are IEEE doubles: the long single row without numpy's call cost
        ca_, cr_, y, G = float(ca[0]), float(cr[0]), 0.0, 0.0
        cm, e, m_ = max(ca_, cr_), [], []
        for an in a[0].tolist():
            G = (an if an > y else y) + cm * G
            y = an + (ca_ if an > y else cr_) * (y - an)
            e.append(y)
            m_.append(G)
        env[0], mag[0] = e, m_
        return env, mag
    ca, cr = ca.astype(F64), cr.astype(F64)
    cm, y, G = np.maximum(ca, cr), np.zeros(B), np.zeros(B)
    for n in range(T):
        an = a[:, n]
        G = np.maximum(an, y) + cm * G
        y = an + np.where(an > y, ca, cr) * (y - an)
        env[:, n], mag[:, n] = y, G
    return env, mag


def comp_env_bound(mag):
    return k_of("comp_env") * EPS32 * mag + TINY


def restate_comp_env(x, ca, cr):
    B, T = x.shape
    a = np.abs(x)
    env, y = np.empty((B, T), F32), np.zeros(B, F32)
    for n in range(T):
        an = a[:, n]
        y = fma32(np.where(an > y, ca, cr), y - an, an)
        env[:, n] = y
    return env


def comp_gain(env, thr, ratio):
    """-> gain, its relative bound given THESE envelope values (0 below the threshold: gain 1)"""
    th, ra = thr.astype(F64)[:, None], ratio.astype(F64)[:, None]
    e = env.astype(F64)
    ex = 1.0 / ra - 1.0
    base = np.maximum(e / th, 1e-300)
    above = e >= th
    g = np.where(above, base ** ex, 1.0)
    rel = HALF * (2.0 * np.abs(ex) + (1.0 / ra + np.abs(ex)) * np.abs(np.log(base))) * SLACK + k_of("powf") * EPS32
    return g, np.where(above, rel, 0.0)


def compressor_y(x, env, thr, ratio):
    """y = gain(env) x given the envelope -> y, bound"""
    g, rel = comp_gain(env, thr, ratio)
    y = g * x.astype(F64)
    return y, np.where(rel > 0, np.abs(y) * (rel + HALF * SLACK) + TINY, 0.0)


def forms_comp_env(x, ca, cr, kernel="fx_comp_env_kernel"):
    env, _ = comp_env(x, ca, cr)
    prev = np.concatenate([np.zeros((x.shape[0], 1)), env[:, :-1]], 1)
    att = np.abs(x.astype(F64)) > prev
    return ({kernel + ":attack"} if att.any() else set()) | ({kernel + ":release"} if (~att).any() else set())


def forms_compressor(c):
    x, thr, ratio, ca, cr = comp_data(c)
    env, _ = comp_env(x, ca, cr)
    out = forms_lanes("fx_comp_env_kernel", c["B"], c["T"]) | forms_comp_env(x, ca, cr) | forms_stream("fx_comp_gain_kernel", c["T"], 256, False)
    ab = env >= thr.astype(F64)[:, None]
    return out | ({"fx_comp_gain:above_threshold"} if ab.any() else set()) | ({"fx_comp_gain:below_threshold"} if (~ab).any() else set())


# ---- limiter ---------------------------------------------------------------------------------------------------------------------------
LIMIT_CASES = (dict(B=3, T=77), dict(B=65, T=40), dict(B=1, T=2048 * 256 + 40))


def limiter_rows(threshold_db, release_ms, sr, makeup=None, dtype=F32):
    """juce::dsp::Limiter::update: the nine parameter rows (thr1 ratio1 ca1 cr1 thr2 ratio2 ca2 cr2 make-up), (9, B)"""
    rows = []
    for t, r in zip(threshold_db, release_ms):
        mk = min(10.0 ** (10.0 * (1.0 - 1.0 / 4.0) / 40.0), 10.0 ** (-t / 20.0))
        rows.append([10.0 ** (-10.0 / 20.0), 4.0, ballistics(2.0, sr), ballistics(200.0, sr), 10.0 ** (t / 20.0), 1000.0, ballistics(0.001, sr),
                     ballistics(r, sr), mk])
    p = np.asarray(rows, F64).T.copy()
    if makeup is not None:
        p[8] = makeup
    return p.astype(dtype)


def limit_data(c, seed=8):
    B, T = c["B"], c["T"]
    g = np.random.default_rng(seed + T)
    x = signal(B, T, seed + T + 1, 3.0, 0.001)
    x *= np.repeat(g.choice([0.02, 1.0], (B, -(-T // 8))), 8, axis=1)[:, :T].astype(F32)
    # thresholds up to +6 dB with the unclamped make-up 10^(7.5 / 20) on odd rows: the clip engages
    p = limiter_rows(g.uniform(-20.0, 6.0, B), g.uniform(10.0, 300.0, B), 8000.0)
    p[8, 1::2] = F32(10.0 ** (7.5 / 20.0))
    return x, p


def limiter_stage1(x, p):
    """-> y1, bound: the stage-1 compressor, its envelope's K-rule bound carried through the gain computer's slope |ex| g / e"""
    env, mag = comp_env(x, p[2], p[3])
    de = comp_env_bound(mag)
    y1, own = compressor_y(x, env, p[0], p[1])
    th, ex = p[0].astype(F64)[:, None], np.abs(1.0 / p[1].astype(F64)[:, None] - 1.0)
    g_lo, _ = comp_gain(np.maximum(env - de, 0.0), p[0], p[1])
    g_hi, _ = comp_gain(env + de, p[0], p[1])
    slope = np.where(env + de >= th, ex * np.maximum(np.maximum(g_lo, g_hi), 1.0) / np.maximum(th, env - de), 0.0)
    _, rel = comp_gain(np.maximum(env, th), p[0], p[1])           # the gain's own roundings, also where only the device is above
    own = np.where(env + de >= th, np.abs(x.astype(F64)) * np.maximum(np.maximum(g_lo, g_hi), 1.0) * (rel + HALF * SLACK), own)
    return y1, np.abs(x.astype(F64)) * slope * de * SLACK + own + TINY


def limiter_out(y1, env2, p):
    """-> y, bound given stage 2's envelope and stage 1's output"""
    g, rel = comp_gain(env2, p[4], p[5])
    v = g * y1.astype(F64) * p[8].astype(F64)[:, None]
    return np.clip(v, -1.0, 1.0), np.abs(v) * (rel + 2.0 * HALF * SLACK) + TINY, np.abs(v) > 1.0


def forms_limiter(c):
    x, p = limit_data(c)
    env1, _ = comp_env(x, p[2], p[3])
    y1, _ = compressor_y(x, env1, p[0], p[1])
    y1 = y1.astype(F32)
    env2, _ = comp_env(y1, p[6], p[7])
    _, _, clipped = limiter_out(y1, env2.astype(F32), p)
    out = forms_lanes("fx_comp_env_kernel", c["B"], c["T"]) | forms_stream("fx_limit_out_kernel", c["T"], 256, False)
    out |= forms_stream("fx_comp_gain_kernel", c["T"], 256, False)
    out |= {f.replace("fx_comp_env_kernel", "limiter_stage1") for f in forms_comp_env(x, p[2], p[3])}
    out |= {f.replace("fx_comp_env_kernel", "limiter_stage2") for f in forms_comp_env(y1, p[6], p[7])}
    for name, e, th in (("limiter_stage1", env1, p[0]), ("limiter_stage2", env2, p[4])):
        ab = e >= th.astype(F64)[:, None]
        out |= ({name + ":above_threshold"} if ab.any() else set()) | ({name + ":below_threshold"} if (~ab).any() else set())
    return out | ({"fx_limit_out_kernel:clip_active"} if clipped.any() else set()) | ({"fx_limit_out_kernel:clip_idle"} if (~clipped).any() else set())


# ---- chorus ----------------------------------------------------------------------------------------------------------------------------
FX_CH_RING = 4096
CHORUS_CASES = (dict(sr=4000.0, B=2, T=4200), dict(sr=48000.0, B=3, T=4200), dict(sr=66000.0, B=1, T=4200), dict(sr=80000.0, B=1, T=4200),
                dict(sr=48000.0, B=2, T=100, mix0=True), dict(sr=80000.0, B=2, T=4200, long=True))


def chorus_blk(sr):
    return min(64, int(F32(sr) / F32(1000.0)) - 2)


def chorus_data(c, seed=9):
    B, T = c["B"], c["T"]
    x = signal(B, T, seed + T + int(c["sr"]), 1.0)
    rate = uniform(B, 0.25, 4.0, seed + 1) * F32(c["sr"] / 48000.0 * (40.0 if T > 1000 else 1.0))      # some LFO periods inside the clip
    depth, cen = uniform(B, 0.3, 0.6, seed + 2), uniform(B, 5.0, 10.0, seed + 3)
    depth[0], cen[0] = 0.6, 5.0                                  # 20 ms x depth / 2 = 6 ms below a centre of 5: the 1 ms floor is reached
    fb, mix = uniform(B, 0.1, 0.6, seed + 4), uniform(B, 0.1, 0.7, seed + 5)
    if c.get("mix0"):
        mix[:] = 0.0
    if c.get("long"):                                            # 34 ... 46 ms: beyond the reference's ranges, within the ring's 50 ms
        depth[:], cen[:] = 0.6, 40.0
    return x, rate, depth, cen, fb, mix


def chorus_delay(c_sr, T, rate, depth, cen):
    """(B, T) delay in samples (fp64 of the float32 parameters) and its float32 uncertainty dd: (float)ph (2 pi half-ulps), sinf (4),
    its product with depth / 2 (1), 20 lfo (1 of |20 lfo|), + centre (1 of |dms|), * sr and / 1000 (2 of d)"""
    sr = float(F32(c_sr))
    n = np.arange(T, dtype=F64)[None, :]
    dep = 0.5 * depth.astype(F64)[:, None]
    lfo = np.sin(2.0 * math.pi * rate.astype(F64)[:, None] / sr * n - math.pi) * dep
    dms = np.maximum(1.0, 20.0 * lfo + cen.astype(F64)[:, None])
    d = dms * sr / 1000.0
    dd = (20.0 * dep * HALF * (2.0 * math.pi + 5.0) + HALF * (20.0 * np.abs(lfo) + dms)) * sr / 1000.0 + 2.0 * HALF * d
    return d, dd * SLACK, dms == 1.0


def _take(a, idx):
    """a[b, idx[b]] or 0 where idx < 0"""
    return np.where(idx >= 0, a[np.arange(a.shape[0]), np.maximum(idx, 0)], 0.0)


def chorus_parts(x, sr, rate, depth, cen, fb, mix):
    """pushed[n] = x[n] - fb popped[n - 1]; popped[n] = pushed interpolated at n - d[n]; y = (1 - mix) x + mix popped.
    -> y, the majorant's magnitude, dd |slope| carried through the recurrence"""
    B, T = x.shape
    x64, f, m = x.astype(F64), fb.astype(F64), mix.astype(F64)
    d, dd, _ = chorus_delay(sr, T, rate, depth, cen)
    di = np.floor(d).astype(np.int64)
    fr = d - di
    pushed, P, E = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
    pop, Q, Ep = np.zeros(B), np.zeros(B), np.zeros(B)
    y, mag, extra = np.empty((B, T)), np.empty((B, T)), np.empty((B, T))
    for n in range(T):
        pushed[:, n], P[:, n], E[:, n] = x64[:, n] - f * pop, np.abs(x64[:, n]) + np.abs(f) * Q, np.abs(f) * Ep
        i1 = n - di[:, n]
        i2 = i1 - 1
        v1, v2, w = _take(pushed, i1), _take(pushed, i2), fr[:, n]
        pop = v1 + w * (v2 - v1)
        Q = (1.0 - w) * _take(P, i1) + w * _take(P, i2)
        slope = np.maximum(np.abs(v2 - v1), np.maximum(np.abs(_take(pushed, i1 + 1) - v1), np.abs(v2 - _take(pushed, i2 - 1))))
        Ep = (1.0 - w) * _take(E, i1) + w * _take(E, i2) + dd[:, n] * slope
        y[:, n] = (1.0 - m) * x64[:, n] + m * pop
        mag[:, n], extra[:, n] = np.abs(1.0 - m) * np.abs(x64[:, n]) + np.abs(m) * Q, np.abs(m) * Ep * SLACK
    return y, mag, extra


def chorus(x, sr, rate, depth, cen, fb, mix):
    """-> y, bound = K eps32 magnitude + the delay's uncertainty; 0 at mix = 0: (1 - 0) x + 0 pop = x"""
    y, mag, extra = chorus_parts(x, sr, rate, depth, cen, fb, mix)
    return y, np.zeros_like(y) if not mix.any() else k_of("chorus") * EPS32 * mag + extra + TINY


def restate_chorus(x, sr, rate, depth, cen, fb, mix):
    """float32, the kernel's arithmetic: the phase reduced in fp64, sinf in float32, the delay in float32.  A block's samples do not
    depend on each other, so sample by sample is the kernel's own order."""
    B, T = x.shape
    sr = F32(sr)
    n = np.arange(T, dtype=F64)[None, :]
    ph = (2.0 * 3.14159265358979323846 * rate.astype(F64)[:, None] / float(sr)) * n
    ph -= np.floor(ph * 0.15915494309189535) * 6.283185307179586
    lfo = (-np.sin(ph.astype(F32)).astype(F32) * (F32(0.5) * depth)[:, None]).astype(F32)
    dms = np.maximum(F32(1.0), fma32(F32(20.0), lfo, cen[:, None]))
    d = ((dms * sr).astype(F32) / F32(1000.0)).astype(F32)
    di = d.astype(np.int64)
    fr = (d - di.astype(F32)).astype(F32)
    pushed = np.zeros((B, T), F32)
    pop = np.zeros(B, F32)
    y = np.empty((B, T), F32)
    one_m = (F32(1.0) - mix).astype(F32)
    for k in range(T):
        pushed[:, k] = fma32(-fb, pop, x[:, k])
        i1 = k - di[:, k]
        v1, v2 = _take(pushed, i1).astype(F32), _take(pushed, i1 - 1).astype(F32)
        pop = fma32(fr[:, k], (v2 - v1).astype(F32), v1)
        y[:, k] = fma32(mix, pop, (one_m * x[:, k]).astype(F32))
    return y


def forms_chorus(c):
    x, rate, depth, cen, fb, mix = chorus_data(c)
    blk, T = chorus_blk(c["sr"]), c["T"]
    dly, _, floor_ = chorus_delay(c["sr"], T, rate, depth, cen)
    out = {"fx_chorus_kernel:blk_%s" % ("64_capped" if int(c["sr"] / 1000) - 2 > 64 else str(blk) if blk in (2, 46, 64) else "other"),
           "fx_chorus_kernel:ring_" + ("wrapped" if T > FX_CH_RING else "not_wrapped"), "fx_chorus_kernel:taps_before_the_clip"}
    out.add("fx_chorus_kernel:" + ("partial_last_block" if T % blk else "full_last_block"))
    if blk < 64:
        out.add("fx_chorus_kernel:idle_lanes")
    if floor_.any():
        out.add("fx_chorus_kernel:delay_floor_1ms")
    if dly.max() > FX_CH_RING // 2:
        out.add("fx_chorus_kernel:delay_beyond_half_ring")
    if not mix.any():
        out.add("fx_chorus_kernel:mix0")
    return out


# ---- Freeverb banks: JUCE reverb and SoX reverb ----------------------------------------------------------------------------------------
COMB_T = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
AP_T_JUCE = (556, 441, 341, 225)
GAIN_015 = float(F32(0.015))


def reverb_lengths(sr):
    return [(sr * t) // 44100 for t in COMB_T], [(sr * t) // 44100 for t in AP_T_JUCE]


def reverb_rate_range():
    """the rates rfx_fx_reverb renders: every ring at least a 64-sample block long, the twelve rings within 160 KB of LDS"""
    lo = next(sr for sr in range(8000, 20000) if min(sum(reverb_lengths(sr), [])) >= 64)
    hi = next(sr for sr in range(192000, 8000, -1) if 4 * sum(sum(reverb_lengths(sr), [])) <= 160 * 1024)
    return lo, hi


def freeverb(inp, lens, damp, fbk, reverse=False):
    """inp (R, T) fp64; lens (R, 12) comb then all-pass lengths; per sample and filter, the plain recurrences
         comb:    o = buf[p]; last = o (1 - damp) + last damp; buf[p] = in + last fbk; out += o
         allpass: o = buf[p]; buf[p] = out + 0.5 o; out = o - out
    reverse: SoX's order (comb 7..0, all-pass 3..0).  -> out (R, T), majorant (R, T): the same run on |in| with |coefficients| and o + out"""
    R, T = inp.shape
    lens = np.asarray(lens, np.int64).reshape(R, 12)
    r2 = np.arange(2 * R)
    lens2 = np.concatenate([lens, lens])
    sgn = np.concatenate([np.ones(R), -np.ones(R)])                  # rows R..2R: the majorant
    x2 = np.concatenate([inp, np.abs(inp)])
    dm = np.concatenate([damp.astype(F64), np.abs(damp.astype(F64))])
    om = np.concatenate([1.0 - damp.astype(F64), np.abs(1.0 - damp.astype(F64))])
    fb = np.concatenate([fbk.astype(F64), np.abs(fbk.astype(F64))])
    buf = np.zeros((12, 2 * R, int(lens.max())))
    pos = np.zeros((12, 2 * R), np.int64)
    last = np.zeros((8, 2 * R))
    out_all = np.empty((2 * R, T))
    corder = range(7, -1, -1) if reverse else range(8)
    aorder = range(11, 7, -1) if reverse else range(8, 12)
    for n in range(T):
        xin = x2[:, n]
        out = np.zeros(2 * R)
        for j in corder:
            p = pos[j]
            o = buf[j, r2, p]
            last[j] = o * om + last[j] * dm
            buf[j, r2, p] = xin + last[j] * fb
            out = out + o
            p += 1
            p[p >= lens2[:, j]] = 0
        for j in aorder:
            p = pos[j]
            o = buf[j, r2, p]
            buf[j, r2, p] = out + 0.5 * o
            out = o - sgn * out
            p += 1
            p[p >= lens2[:, j]] = 0
        out_all[:, n] = out
    return out_all[:R], out_all[R:]


def restate_freeverb(inp, lens, damp, fbk, reverse=False):
    """float32, the kernels' decomposition of one bank per row: blocks of blk = min(64, shortest ring) samples on 64 lanes, the damping
    one-pole as the six-step weighted wave scan with damp^(2^s), the carried state through damp^(lane + 1) (powf)"""
    R, T = inp.shape
    lens = np.asarray(lens, np.int64).reshape(R, 12)
    out_all = np.zeros((R, T), F32)
    lane = np.arange(64)
    for r in range(R):
        L = lens[r]
        blk = int(min(64, L.min()))
        inb = lane < blk
        dp, fb = F32(damp[r]), F32(fbk[r])
        dpw = [dp]
        for s in range(1, 6):
            dpw.append(F32(dpw[-1] * dpw[-1]))
        dl1 = np.power(dp, (lane + 1).astype(F32)).astype(F32)
        om = F32(F32(1.0) - dp)
        bufs = [np.zeros(int(l), F32) for l in L]
        pos, last = [0] * 12, [F32(0.0)] * 8
        xin = np.zeros(-(-T // blk) * blk + 64, F32)
        xin[:T] = inp[r]
        for n0 in range(0, T, blk):
            xv = np.where(inb, xin[n0:n0 + 64], F32(0.0)).astype(F32)
            out = np.zeros(64, F32)
            for j in (range(7, -1, -1) if reverse else range(8)):
                idx = (pos[j] + lane) % L[j]
                o = np.where(inb, bufs[j][idx], F32(0.0)).astype(F32)
                v = (om * o).astype(F32)
                for s in range(6):
                    u = np.concatenate([np.zeros(1 << s, F32), v[:64 - (1 << s)]])
                    v = np.where(lane >= (1 << s), fma32(dpw[s], u, v), v).astype(F32)
                v = fma32(dl1, last[j], v)
                bufs[j][idx[inb]] = fma32(v, fb, xv)[inb]
                last[j] = v[blk - 1]
                pos[j] = (pos[j] + blk) % L[j]
                out = (out + o).astype(F32)
            for j in (range(11, 7, -1) if reverse else range(8, 12)):
                idx = (pos[j] + lane) % L[j]
                o = np.where(inb, bufs[j][idx], F32(0.0)).astype(F32)
                bufs[j][idx[inb]] = fma32(F32(0.5), o, out)[inb]
                out = (o - out).astype(F32)
                pos[j] = (pos[j] + blk) % L[j]
            m = min(blk, T - n0)
            out_all[r, n0:n0 + m] = out[:m]
    return out_all


REVERB_CASES = (dict(sr=12544, B=3, T=2000), dict(sr=48000, B=2, T=3700), dict(sr=12544, B=1, T=50), dict(sr=12544, B=1, T=64))


def reverb_data(c, seed=10):
    B = c["B"]
    return (signal(B, c["T"], seed + c["T"], 1.0), uniform(B, 0.0, 0.4, seed + 1), uniform(B, 0.7, 0.98, seed + 2), uniform(B, 0.0, 2.0, seed + 3),
            uniform(B, 0.6, 2.0, seed + 4))


def reverb(x, sr, damp, fbk, wet1, dry):
    """in = 0.015 x; out = the bank; y = wet1 out + dry x.  -> y, bound"""
    B = x.shape[0]
    cl, al = reverb_lengths(sr)
    inp = x.astype(F64) * GAIN_015
    out, maj = freeverb(inp, [cl + al] * B, damp, fbk)
    w, d = wet1.astype(F64)[:, None], dry.astype(F64)[:, None]
    return out * w + x.astype(F64) * d, k_of("reverb") * EPS32 * (np.abs(w) * maj + np.abs(d * x.astype(F64))) + TINY


def restate_reverb(x, sr, damp, fbk, wet1, dry):
    cl, al = reverb_lengths(sr)
    out = restate_freeverb((x * F32(0.015)).astype(F32), [cl + al] * x.shape[0], damp, fbk)
    return fma32(out, wet1[:, None], (x * dry[:, None]).astype(F32))


def forms_reverb(c):
    cl, al = reverb_lengths(c["sr"])
    out = {"fx_reverb_kernel:rate_%s" % ("lowest" if min(al) == 64 else "48000" if c["sr"] == 48000 else "other")}
    for j, l in enumerate(cl + al):
        out.add("fx_reverb_kernel:ring%d_%s" % (j, "wrapped" if c["T"] > l else "not_wrapped"))
    out.add("fx_reverb_kernel:" + ("partial_last_block" if c["T"] % 64 else "full_last_block"))
    return out


# SoX: geometry rows passed directly.  bank = (pre-delay, 8 comb lengths, 4 all-pass lengths)
_L64 = (64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75)
_L63 = (63, 65, 66, 67, 68, 69, 70, 71, 64, 73, 74, 75)
_L7 = (9, 11, 13, 8, 15, 17, 19, 21, 7, 10, 12, 14)
_L1 = (3, 5, 2, 4, 6, 8, 1, 9, 2, 3, 1, 5)
_L65 = (65, 66, 90, 77, 68, 99, 70, 71, 72, 73, 80, 75)
SOX_CASES = (
    dict(B=2, Cin=1, T=300, banks=((0, _L64), (0, _L63), (5, _L7), (400, _L1))),
    dict(B=2, Cin=2, T=150, banks=((3, _L65), (3, _L7), (3, _L63), (3, _L64), (150, _L1), (150, _L7), (0, _L1), (0, _L65))),
    dict(B=1, Cin=1, T=64, banks=((0, _L64), (63, _L65))),
)


def sox_data(c, seed=11):
    B, Cin, T = c["B"], c["Cin"], c["T"]
    x = signal(B * Cin, T, seed + T, 1.6).reshape(B, Cin, T)                 # beyond [-1, 1]: the input clip acts
    R = B * Cin * 2
    geom = np.zeros((R, 16), np.int32)
    for r, (dly, L) in enumerate(c["banks"]):
        geom[r, 0], geom[r, 1:13], geom[r, 13] = dly, L, r // 2
    coef = np.stack([uniform(R, 0.3, 0.98, seed + 1), uniform(R, 0.2, 0.5, seed + 2), np.full(R, 0.015, F32), np.repeat(uniform(B, 0.2, 1.0, seed + 3), Cin * 2)], 1)
    return x, geom, coef.astype(F32), int(max(sum(L) for _, L in c["banks"]))


def sox_bank_input(x, geom):
    R, T = geom.shape[0], x.shape[-1]
    xr = x.reshape(-1, T).astype(F64)
    inp = np.zeros((R, T))
    for r in range(R):
        d = int(geom[r, 0])
        if d < T:
            inp[r, d:] = np.clip(xr[geom[r, 13]], -1.0, 1.0)[:T - d]
    return inp


def sox_banks(x, geom, coef):
    """ws row r = gain bank_r(clip(x[row_r][n - delay_r])).  -> ws (R, T), bound"""
    out, maj = freeverb(sox_bank_input(x, geom), geom[:, 1:13], coef[:, 1], coef[:, 0], reverse=True)
    g = coef[:, 2].astype(F64)[:, None]
    return out * g, k_of("sox_bank") * EPS32 * np.abs(g) * maj + TINY


def restate_sox_banks(x, geom, coef):
    out = restate_freeverb(sox_bank_input(x, geom).astype(F32), geom[:, 1:13], coef[:, 1], coef[:, 0], reverse=True)
    return (out * coef[:, 2][:, None]).astype(F32)


def sox_mix(x, ws, coef, Cin):
    """y[b, w] = x[b, min(w, Cin - 1)] (1 - wet_dry) + clip(mean_c ws[(b Cin + c) 2 + w]) wet_dry, given the banks.  -> y (B, 2, T), bound"""
    B, T = x.shape[0], x.shape[-1]
    w4 = ws.astype(F64).reshape(B, Cin, 2, T)
    wet = np.clip(w4.mean(axis=1), -1.0, 1.0)
    wd = coef.reshape(B, Cin * 2, 4)[:, 0, 3].astype(F64)[:, None, None]
    xs = x.astype(F64)[:, [0, Cin - 1]]
    y = xs * (1.0 - wd) + wet * wd
    return y, HALF * SLACK * (3.0 * np.abs(xs * (1.0 - wd)) + (2.0 + (Cin == 2)) * np.abs(wet * wd)) + TINY


def forms_sox(c):
    out = {"fx_sox_bank_kernel:Cin%d" % c["Cin"], "fx_sox_mix_kernel:Cin%d" % c["Cin"]} | forms_stream("fx_sox_mix_kernel", c["T"], 256, False)
    for dly, L in c["banks"]:
        blk = min(64, min(L))
        out.add("fx_sox_bank_kernel:blk_%s" % ("64" if blk == 64 else "1" if blk == 1 else "between"))
        out.add("fx_sox_bank_kernel:predelay_" + ("0" if dly == 0 else ">=T" if dly >= c["T"] else "inside"))
        out.add("fx_sox_bank_kernel:" + ("rings_wrapped" if c["T"] > max(L) else "rings_not_wrapped"))
        out.add("fx_sox_bank_kernel:" + ("partial_last_block" if c["T"] % blk else "full_last_block"))
    return out


# ---- biquad cascades: EQ and K-weighting -----------------------------------------------------------------------------------------------
def rbj(kind, gain_db, fc, q, rate):
    """RBJ cookbook biquad -> (b0 b1 b2 a1 a2) / a0"""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * fc / rate
    al, c, sA = math.sin(w0) / (2.0 * q), math.cos(w0), math.sqrt(A)
    if kind == "high_shelf":
        b = (A * ((A + 1) + (A - 1) * c + 2 * sA * al), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - 2 * sA * al))
        a = ((A + 1) - (A - 1) * c + 2 * sA * al, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - 2 * sA * al)
    elif kind == "low_shelf":
        b = (A * ((A + 1) - (A - 1) * c + 2 * sA * al), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - 2 * sA * al))
        a = ((A + 1) + (A - 1) * c + 2 * sA * al, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - 2 * sA * al)
    elif kind == "peaking":
        b, a = (1 + al * A, -2 * c, 1 - al * A), (1 + al / A, -2 * c, 1 - al / A)
    else:                                                               # high_pass
        b, a = ((1 + c) / 2, -(1 + c), (1 + c) / 2), (1 + al, -2 * c, 1 - al)
    return np.array([b[0], b[1], b[2], a[1], a[2]]) / a[0]


def k_weighting(rate):
    """pyloudnorm's K-weighting: high shelf (+4 dB, 1500 Hz, Q 1 / sqrt 2), then high pass (38 Hz, Q 0.5)"""
    return np.stack([rbj("high_shelf", 4.0, 1500.0, 1.0 / math.sqrt(2.0), rate), rbj("high_pass", 0.0, 38.0, 0.5, rate)])


def eq_sections(p, rate):
    """low shelf, the bands, high shelf: (NS, 5)"""
    s = [rbj("low_shelf", *p["low"], rate)] + [rbj("peaking", *b, rate) for b in p["bands"]] + [rbj("high_shelf", *p["high"], rate)]
    return np.stack(s)


def cascade_step(sec, v, s):
    """one sample through the sections (NS, 5) in transposed direct form II; s (..., 2 NS) is updated in place"""
    for k in range(sec.shape[-2]):
        c = sec[..., k, :]
        y = c[..., 0] * v + s[..., 2 * k]
        s[..., 2 * k] = c[..., 1] * v - c[..., 3] * y + s[..., 2 * k + 1]
        s[..., 2 * k + 1] = c[..., 2] * v - c[..., 4] * y
        v = y
    return v


def cascade(x, sec):
    """x (R, T), sec (R, NS, 5) -> y (R, T) fp64, the largest intermediate value or state per row"""
    R, T = x.shape
    s = np.zeros((R, 2 * sec.shape[1]))
    y, big = np.empty((R, T)), np.abs(x).max(axis=1).astype(F64)
    x64 = x.astype(F64)
    for n in range(T):
        y[:, n] = cascade_step(sec, x64[:, n], s)
        big = np.maximum(big, np.abs(s).max(axis=1))
    return y, np.maximum(big, np.abs(y).max(axis=1))


def transition(sec, steps):
    """the zero-input state transition of `steps` samples: the one-step matrix from the recurrence applied to every unit state, then
    its power by repeated multiplication"""
    D = 2 * sec.shape[0]
    A = np.zeros((D, D))
    for i in range(D):
        s = np.zeros(D)
        s[i] = 1.0
        cascade_step(sec, 0.0, s)
        A[:, i] = s
    M, P, k = np.eye(D), A.copy(), int(steps)
    while k:
        if k & 1:
            M = P @ M
        P, k = P @ P, k >> 1
    return A, M


def state_gain(A, T):
    """|| sum_{n < T} |A^n| ||_inf: what a perturbation of the state of unit size at every sample can add up to"""
    S, P = np.zeros_like(A), np.eye(A.shape[0])
    for _ in range(int(T)):
        S += np.abs(P)
        P = A @ P
    return float(np.abs(S).sum(axis=1).max())


def cascade_fp64_term(sec, T, big):
    """the fp64 evaluation's error per row (module docstring): 2^-53 x (16 NS (1 + max |coef|) + 64 (D + 1)) x state gain x largest value"""
    out = np.empty(sec.shape[0])
    for r in range(sec.shape[0]):
        A, _ = transition(sec[r], 1)
        out[r] = U64 * (16.0 * sec.shape[1] * (1.0 + np.abs(sec[r]).max()) + 64.0 * (2 * sec.shape[1] + 1)) * max(1.0, state_gain(A, T)) * big[r]
    return out


EQ_RATE = 8000.0
EQ_CASES = (dict(NS=2, B=2, T=128, chunk=2), dict(NS=3, B=3, T=100, chunk=7), dict(NS=4, B=1, T=70, chunk=2), dict(NS=5, B=2, T=333, chunk=6),
            dict(NS=6, B=1, T=64, chunk=1), dict(NS=7, B=2, T=95, chunk=3), dict(NS=8, B=3, T=257, chunk=5), dict(NS=5, B=1, T=9, chunk=40))


def eq_data(c, seed=12):
    g = np.random.default_rng(seed + c["T"])
    x = signal(c["B"], c["T"], seed + c["T"] + 1, 1.0)
    sec = []
    for _ in range(c["B"]):
        p = dict(low=(g.uniform(-6, 6), g.uniform(20, 200) / 6, g.uniform(0.1, 4)), high=(g.uniform(-6, 6), g.uniform(8000, 16000) / 6, g.uniform(0.1, 4)),
                 bands=[(g.uniform(-6, 6), g.uniform(1000, 10000) / 6, g.uniform(0.1, 4)) for _ in range(c["NS"] - 2)])
        sec.append(eq_sections(p, EQ_RATE))
    sec = np.stack(sec)
    coef = np.stack([np.concatenate([sec[r].reshape(-1), transition(sec[r], c["chunk"])[1].reshape(-1)]) for r in range(c["B"])])
    return x, sec, coef


def eq(x, sec):
    """-> y (fp64, before the float32 rounding), bound"""
    y, big = cascade(x, sec)
    return y, HALF * np.abs(y) + cascade_fp64_term(sec, x.shape[1], big)[:, None] + TINY


def forms_chunks(kernel, T, chunk):
    out = {kernel + (":full_last_chunk" if T % chunk == 0 else ":short_last_chunk")}
    if -(-T // chunk) < 64:
        out.add(kernel + ":empty_chunks")
    if chunk * 64 == T:
        out.add(kernel + ":chunk*64==T")
    if T <= chunk:
        out.add(kernel + ":one_chunk")
    return out


def forms_eq(c):
    return {"fx_eq_kernel<%d>" % c["NS"], "fx_eq_kernel:state_lanes", "fx_eq_kernel:shadow_lanes"} | forms_chunks("fx_eq_kernel", c["T"], c["chunk"])


# ---- loudness --------------------------------------------------------------------------------------------------------------------------
LOUD_RATE = 8000.0
LOUD_CASES = (
    dict(B=2, C=1, T=1000, chunk=16, hop=40, nhop=24, nblk=21, kind=("plain", "relative")),
    dict(B=2, C=1, T=1000, chunk=16, hop=10, nhop=90, nblk=87, kind=("relative", "quiet")),
    dict(B=1, C=1, T=1024, chunk=16, hop=64, nhop=16, nblk=13, kind=("plain",)),
    dict(B=2, C=1, T=200, chunk=50, hop=10, nhop=20, nblk=17, kind=("plain", "relative")),
    dict(B=2, C=2, T=1000, chunk=16, hop=40, nhop=25, nblk=22, kind=("plain", "relative")),
    dict(B=65, C=1, T=96, chunk=2, hop=8, nhop=12, nblk=9, kind=("plain", "relative", "quiet")),
    dict(B=130, C=1, T=96, chunk=2, hop=8, nhop=12, nblk=9, kind=("plain", "relative", "quiet")),
    dict(B=64, C=1, T=96, chunk=3, hop=8, nhop=12, nblk=9, kind=("relative", "plain")),
    dict(B=1, C=1, T=40, chunk=64, hop=8, nhop=5, nblk=2, kind=("plain",)),
)
LOUD_TARGET = -32.0


def loud_plan(T, rate):
    """the launch arguments of a T-sample clip at `rate`: 400 ms blocks at 75 % overlap over 100 ms hops, 64 chunks
    -> chunk, hop, nhop, nblk, inv_block, the 28 coefficients"""
    nblk = int(np.round((T / rate - 0.4) / 0.1) + 1)
    hop, chunk = int(round(0.1 * rate)), -(-T // 64)
    sec = k_weighting(rate)
    coef = np.concatenate([sec[0, :3], [1.0], sec[0, 3:], sec[1, :3], [1.0], sec[1, 3:], transition(sec, chunk)[1].reshape(-1)])
    return chunk, hop, nblk + 3, nblk, 1.0 / (0.4 * rate), coef


def loud_data(c, seed=13):
    """rows of kind plain (one level), relative (a stretch 25 dB down: removed by the relative gate), quiet (below -70 LUFS throughout)"""
    B, C, T = c["B"], c["C"], c["T"]
    x = signal(B * C, T, seed + T + B, 0.5, 0.5).reshape(B, C, T)
    for b in range(B):
        k = c["kind"][b % len(c["kind"])]
        if k == "relative":
            x[b, :, :T // 2] *= F32(10.0 ** (-25.0 / 20.0))
        elif k == "quiet":
            x[b] *= F32(1e-5)
    sec = k_weighting(LOUD_RATE)
    coef = np.concatenate([sec[0, :3], [1.0], sec[0, 3:], sec[1, :3], [1.0], sec[1, 3:], transition(sec, c["chunk"])[1].reshape(-1)])
    return x, sec, coef.astype(F64), 1.0 / (4.0 * c["hop"])


def loudness(x, sec, c, target=LOUD_TARGET):
    """x (B, C, T) -> dict(hop (B C, nhop), hop_bound, lufs (B,), lufs_bound, gain, gain_bound, l (B, nblk) block loudness, gamma_r, margin)"""
    B, C, T = x.shape
    R, nhop, hop, nblk = B * C, c["nhop"], c["hop"], c["nblk"]
    w, big = cascade(x.reshape(R, T), np.broadcast_to(sec, (R,) + sec.shape))
    dw = cascade_fp64_term(np.broadcast_to(sec, (R,) + sec.shape), T, big)
    hs, hb = np.zeros((R, nhop)), np.zeros((R, nhop))
    for h in range(nhop):
        seg = w[:, h * hop:min((h + 1) * hop, T)]
        hs[:, h] = (seg * seg).sum(axis=1)
        hb[:, h] = (2.0 * np.abs(seg) * dw[:, None] + dw[:, None] ** 2).sum(axis=1) + U64 * (seg.shape[1] + 64 + 2) * hs[:, h]
    hc, hcb = hs.reshape(B, C, nhop).sum(axis=1), hb.reshape(B, C, nhop).sum(axis=1)
    inv = 1.0 / (4.0 * hop)
    z = np.stack([hc[:, j:j + 4].sum(axis=1) for j in range(nblk)], 1) * inv
    zb = np.stack([hcb[:, j:j + 4].sum(axis=1) for j in range(nblk)], 1) * inv + U64 * (4 * C + 2) * z
    lufs, lb, gam, margin = np.empty(B), np.empty(B), np.full(B, -np.inf), np.zeros(B)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    db = 10.0 / math.log(10.0)
    for b in range(B):
        J = l[b] >= -70.0
        margin[b] = 4.0 * db * float((zb[b] / np.maximum(z[b], 1e-300)).max()) + 64.0 * U64 * 70.0
        if not J.any():
            lufs[b], lb[b] = -np.inf, 0.0
            continue
        gam[b] = -0.691 + 10.0 * math.log10(z[b][J].mean()) - 10.0
        K = (l[b] > gam[b]) & (l[b] > -70.0)
        lufs[b] = -0.691 + 10.0 * math.log10(z[b][K].mean())
        lb[b] = db * float(zb[b][K].sum() / z[b][K].sum()) * 2.0 + 64.0 * U64 * abs(lufs[b]) + HALF * abs(lufs[b])
    # gain = powf(10, clamp(target - (float) L, -120, 40) / 20): the difference and the quotient round once each
    d = np.clip(F64(F32(target)) - lufs, -120.0, 40.0)
    gain = 10.0 ** (d / 20.0)
    du = np.where((d > -120.0) & (d < 40.0), (lb + HALF * np.abs(d)) / 20.0 + HALF * np.abs(d / 20.0), HALF * np.abs(d / 20.0))
    return dict(hop=hs, hop_bound=hb + 1e-300, lufs=lufs, lufs_bound=lb, gain=gain, gain_bound=gain * (math.log(10.0) * du * SLACK + k_of("powf") * EPS32),
                l=l, gamma_r=gam, margin=margin)


def loud_margins(res):
    """per clip: the smallest distance of a block's loudness from -70 LUFS and from the relative gate, and the margin it has to exceed"""
    dist = np.minimum(np.abs(res["l"] + 70.0).min(axis=1), np.abs(res["l"] - res["gamma_r"][:, None]).min(axis=1))
    return dist, res["margin"]


def forms_loudness(c):
    x, sec, _, _ = loud_data(c)
    res = loudness(x, sec, c)
    T, ch, hop, nhop = c["T"], c["chunk"], c["hop"], c["nhop"]
    out = forms_chunks("fx_kweight_kernel", T, ch) | forms_lanes("fx_loud_gate_kernel", c["B"]) | {"fx_kweight_kernel:C%s" % ("1" if c["C"] == 1 else ">1")}
    borders = [h for h in range(hop, T, hop)]
    if any(h % ch for h in borders):
        out.add("fx_kweight_kernel:hop_border_inside_chunk")
    if any(h % ch == 0 for h in borders):
        out.add("fx_kweight_kernel:hop_border_on_chunk_border")
    if any(len([h for h in borders if k * ch < h < min((k + 1) * ch, T)]) > 1 for k in range(64)):
        out.add("fx_kweight_kernel:several_hops_per_chunk")
    if T > nhop * hop:
        out.add("fx_kweight_kernel:samples_past_the_hops")
    if -(-T // ch) <= 32:
        out.add("fx_kweight_kernel:most_chunks_empty")
    for b in range(c["B"]):
        J = res["l"][b] >= -70.0
        if not J.any():
            out.add("fx_loud_gate_kernel:no_block_above_absolute_gate")
        elif (res["l"][b][J] <= res["gamma_r"][b]).any():
            out.add("fx_loud_gate_kernel:relative_gate_removes")
        else:
            out.add("fx_loud_gate_kernel:all_blocks_kept")
    return out


NORM_CASES = (dict(B=3, C=1, T=200, chunk=50, hop=10, nhop=20, nblk=17, kind=("plain", "relative", "plain"), N=6, rows=(4, 0, 2)),
              dict(B=2, C=1, T=200, chunk=4, hop=10, nhop=20, nblk=17, kind=("plain", "relative"), N=2, rows=None, value="the dense form, in place of the state"))


# ---- phaser ----------------------------------------------------------------------------------------------------------------------------
PHASER_CASES = (dict(B=1, T=20), dict(B=3, T=77), dict(B=65, T=40), dict(B=130, T=100), dict(B=1, T=4 * 2048 * 256 + 50, prefix=4096),
                dict(B=64, T=64, mix0=True))
PHASER_SR = 8000.0


def phaser_ws_floats(B, T):
    return B * (((T + 3) // 4 + 7) // 8 * 8)


def phaser_data(c, seed=14):
    B = c["B"]
    mix = uniform(B, 0.1, 0.7, seed + 5)
    if c.get("mix0"):
        mix[:] = 0.0
    return (signal(B, c["T"], seed + c["T"], 1.0), uniform(B, 5.0, 100.0, seed + 1), uniform(B, 0.1, 0.6, seed + 2), uniform(B, 200.0, 600.0, seed + 3),
            uniform(B, 0.1, 0.6, seed + 4), mix)


def phaser_coef(T, sr, rate, depth, centre):
    """G[m] of every row, m = n / 4, fp64 (before the float32 rounding): G = g / (1 + g), g = tan(pi f / sr), f = 20 (fmax / 20)^v,
    v = clamp(sin(2 pi rate m / (sr / 4) - pi) depth / 2 + normCentre, 0, 1).  -> G (B, M), bound"""
    sr = float(F32(sr))
    M = (T + 3) // 4
    fhi = min(20000.0, 0.49 * sr)
    nc = (np.log10(centre.astype(F64)) - math.log10(20.0)) / (math.log10(fhi) - math.log10(20.0))
    m = np.arange(M, dtype=F64)[None, :]
    v = np.clip(np.sin(2.0 * math.pi * rate.astype(F64)[:, None] / (sr / 4.0) * m - math.pi) * (0.5 * depth.astype(F64)[:, None]) + nc[:, None], 0.0, 1.0)
    g = np.tan(math.pi * (20.0 * (fhi / 20.0) ** v) / sr)
    G = g / (1.0 + g)
    return G, k_of("phaser_coef") * EPS32 * G


def restate_phaser_coef(T, sr, rate, depth, centre):
    """the kernel's order: the phase reduced by its whole turns before the sine; rounded to float32 at the end"""
    sr = float(F32(sr))
    M, pi = (T + 3) // 4, 3.14159265358979323846
    fhi = min(20000.0, 0.49 * sr)
    lmin, lmax = math.log10(20.0), math.log10(fhi)
    nc = (np.log10(centre.astype(F64)) - lmin) / (lmax - lmin)
    ph = (2.0 * pi * rate.astype(F64)[:, None] / (sr / 4.0)) * np.arange(M, dtype=F64)[None, :]
    ph -= np.floor(ph * (0.5 / pi)) * (2.0 * pi)
    v = np.minimum(np.maximum(np.sin(ph - pi) * (0.5 * depth.astype(F64)[:, None]) + nc[:, None], 0.0), 1.0)
    g = np.tan(pi * (20.0 * np.power(fhi / 20.0, v)) / sr)
    return (g / (1.0 + g)).astype(F32)


def phaser(x, G, fb, mix):
    """given the float32 coefficient stream G (B, >= T / 4): u = x - fb out[n - 1]; six all-passes v = G (u - s), y = v + s, s = y + v,
    u = 2 y - u; y[n] = (1 - mix) x + mix u.  -> y, bound"""
    B, T = x.shape
    x64, f, m = x.astype(F64), fb.astype(F64), mix.astype(F64)
    s = np.zeros((6, B))
    last, big = np.zeros(B), np.zeros(B)
    y, bound = np.empty((B, T)), np.empty((B, T))
    for n in range(T):
        g = G[:, n // 4].astype(F64)
        u = x64[:, n] - last
        big = np.maximum(big, np.abs(x64[:, n]))
        for k in range(6):
            v = g * (u - s[k])
            yk = v + s[k]
            s[k] = yk + v
            u = 2.0 * yk - u
            big = np.maximum(big, np.maximum(np.abs(u), np.abs(s[k])))
        last = u * f
        y[:, n] = (1.0 - m) * x64[:, n] + m * u
        bound[:, n] = k_of("phaser") * EPS32 * (np.abs(1.0 - m) * np.abs(x64[:, n]) + np.abs(m) * big / (1.0 - np.abs(f))) + TINY
    if not mix.any():
        bound[:] = 0.0
    return y, bound


def restate_phaser(x, G, fb, mix):
    B, T = x.shape
    s = np.zeros((6, B), F32)
    last = np.zeros(B, F32)
    dry = (F32(1.0) - mix).astype(F32)
    y = np.empty((B, T), F32)
    for n in range(T):
        g = G[:, n // 4]
        u = (x[:, n] - last).astype(F32)
        for k in range(6):
            v = (g * (u - s[k]).astype(F32)).astype(F32)
            yk = (v + s[k]).astype(F32)
            s[k] = (yk + v).astype(F32)
            u = fma32(F32(2.0), yk, -u)
        last = (u * fb).astype(F32)
        y[:, n] = fma32(u, mix, (x[:, n] * dry).astype(F32))
    return y


def forms_phaser(c):
    M = (c["T"] + 3) // 4
    out = forms_lanes("fx_phaser_kernel", c["B"], c["T"]) | forms_stream("fx_phaser_coef_kernel", M, 256, False)
    out.add("fx_phaser_coef_kernel:" + ("row_padded" if M % 8 else "row_not_padded"))
    if c["T"] % 4:
        out.add("fx_phaser_kernel:last_coefficient_partly_used")
    if c.get("mix0"):
        out.add("fx_phaser_kernel:mix0")
    return out


# ---- every form ------------------------------------------------------------------------------------------------------------------------
# named, with the reason, in DESIGN.md 4.23
UNREACHABLE = {
    "fx_sox_mix_kernel:second_trip", "fx_sox_mix_kernel:grid_capped",      # T > 524288 through twelve fp64 rings per bank: no cheap reference
    "fx_grid:clamped_to_one_block",                                        # T <= 0 is refused before any grid is formed
    "fx_loud_gate_kernel:relative_gate_removes_all",                       # n2 == 0 with n1 > 0: the loudest block is above the mean - 10 LU
}


def _stream_forms(kernel, vec):
    out = {kernel + s for s in (":first_trip", ":second_trip", ":grid_capped")}
    return out | ({kernel + s for s in (":tail_only", ":body16", ":scalar_tail", ":rows_not_16B_aligned", ":payload_offset_1", ":payload_offset_2",
                                          ":payload_offset_3")} if vec else set())


def _lane_forms(kernel, T):
    out = {kernel + s for s in (":workgroups_1", ":workgroups_2", ":workgroups_3", ":partial_wave", ":full_wave")}
    return out | ({kernel + s for s in (":tail_only", ":prefetch32", ":scalar_tail")} if T else set())


def all_forms():
    out = set(UNREACHABLE)
    for k, vec in (("fx_distortion_kernel", True), ("fx_widener_kernel", True), ("fx_scale_kernel", False), ("fx_delay_kernel", False),
                   ("fx_volume_kernel", False), ("fx_comp_gain_kernel", False), ("fx_limit_out_kernel", False), ("fx_sox_mix_kernel", False),
                   ("fx_phaser_coef_kernel", False)):
        out |= _stream_forms(k, vec)
    out |= {"fx_scale_kernel:row_table", "fx_scale_kernel:dense", "fx_delay_kernel:D<=0", "fx_delay_kernel:0<D<T", "fx_delay_kernel:D>=T", "fx_delay_kernel:D==1"}
    out |= {"fx_volume_kernel:" + s for s in ("S_1", "S_64", "S_between", "table_ends_before_T", "table_ends_at_T", "table_ends_after_T",
                                              "zero_length_segment", "steps==1", "first_half", "second_half")}
    out |= _lane_forms("fx_comp_env_kernel", True) | _lane_forms("fx_phaser_kernel", True) | _lane_forms("fx_loud_gate_kernel", False)
    out |= {"fx_comp_env_kernel:attack", "fx_comp_env_kernel:release", "fx_comp_gain:above_threshold", "fx_comp_gain:below_threshold"}
    for st in ("limiter_stage1", "limiter_stage2"):
        out |= {st + s for s in (":attack", ":release", ":above_threshold", ":below_threshold")}
    out |= {"fx_limit_out_kernel:clip_active", "fx_limit_out_kernel:clip_idle"}
    out |= {"fx_chorus_kernel:" + s for s in ("blk_2", "blk_46", "blk_64", "blk_64_capped", "ring_wrapped", "ring_not_wrapped", "taps_before_the_clip",
                                              "partial_last_block", "full_last_block", "idle_lanes", "delay_floor_1ms", "mix0", "delay_beyond_half_ring")}
    out |= {"fx_reverb_kernel:" + s for s in ("rate_lowest", "rate_48000", "partial_last_block", "full_last_block")}
    out |= {"fx_reverb_kernel:ring%d_%s" % (j, s) for j in range(12) for s in ("wrapped", "not_wrapped")}
    out |= {"fx_sox_bank_kernel:" + s for s in ("Cin1", "Cin2", "blk_64", "blk_between", "blk_1", "predelay_0", "predelay_inside", "predelay_>=T",
                                                "rings_wrapped", "rings_not_wrapped", "partial_last_block", "full_last_block", "nan_plan_length_0",
                                                "nan_plan_beyond_lds")}
    out |= {"fx_sox_mix_kernel:Cin1", "fx_sox_mix_kernel:Cin2", "fx_sox_mix_kernel:nan_stays_nan"}
    out |= {"fx_eq_kernel<%d>" % n for n in range(2, 9)} | {"fx_eq_kernel:state_lanes", "fx_eq_kernel:shadow_lanes"}
    for k in ("fx_eq_kernel", "fx_kweight_kernel"):
        out |= {k + s for s in (":full_last_chunk", ":short_last_chunk", ":empty_chunks", ":chunk*64==T", ":one_chunk")}
    out |= {"fx_kweight_kernel:" + s for s in ("C1", "C>1", "hop_border_inside_chunk", "hop_border_on_chunk_border", "several_hops_per_chunk",
                                               "samples_past_the_hops", "most_chunks_empty")}
    out |= {"fx_loud_gate_kernel:" + s for s in ("no_block_above_absolute_gate", "relative_gate_removes", "all_blocks_kept")}
    out |= {"fx_phaser_coef_kernel:row_padded", "fx_phaser_coef_kernel:row_not_padded", "fx_phaser_kernel:last_coefficient_partly_used", "fx_phaser_kernel:mix0"}
    return out


NAN_PLAN_FORMS = {"fx_sox_bank_kernel:nan_plan_length_0", "fx_sox_bank_kernel:nan_plan_beyond_lds", "fx_sox_mix_kernel:nan_stays_nan"}


def case_tables():
    """(entry point, case, forms function) of every case both tests walk, in table order"""
    out = []
    for name, cases, fn in (("distortion", DIST_CASES, forms_distortion), ("widener", WIDE_CASES, forms_widener), ("scale", SCALE_CASES, forms_scale),
                            ("delay", DELAY_CASES, forms_delay), ("volume", VOL_CASES, forms_volume), ("compressor", COMP_CASES, forms_compressor),
                            ("limiter", LIMIT_CASES, forms_limiter), ("chorus", CHORUS_CASES, forms_chorus), ("reverb", REVERB_CASES, forms_reverb),
                            ("sox_reverb", SOX_CASES, forms_sox), ("eq", EQ_CASES, forms_eq), ("loudness", LOUD_CASES, forms_loudness),
                            ("phaser", PHASER_CASES, forms_phaser)):
        out += [(name, c, fn) for c in cases]
    out += [("normalize_rows", c, lambda c: forms_loudness(c) | forms_scale(c, c["rows"] is not None)) for c in NORM_CASES]
    return out


def walk_all_cases():
    """-> (the union of reached forms, [(entry, case, new forms)]); the NaN-plan test's forms are added by name (its geometry is no case)"""
    seen, per = set(NAN_PLAN_FORMS), []
    for name, c, fn in case_tables():
        f = fn(c)
        per.append((name, c, f - seen))
        seen |= f
    return seen, per
