"""tests/fft_ref.py against independent statements of the same operations (no GPU): torch.stft / torch.istft in float64, float64 autograd
for the two adjoint pairs, oracle/ref_losses.stft_loss through autograd, oracle/ref_hdemucs' _spec / _ispec; the case tables reach every
launch form the forms_*() mirrors can name (or the form is listed with its reason); the floor table is the measurement; every bound has
power."""
import functools
import math
import types

import pytest
import torch

from tests import fft_ref as F

GEOMS = ((512, 50, 240), (1024, 256, 1024), (4096, 1000, 4095), (64, 16, 64), (128, 50, 100), (8192, 2048, 8192))


def _close(a, b, rel=1e-10):
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= rel * scale, (float((a - b).abs().max()), scale)


@pytest.mark.parametrize("geom", GEOMS)
def test_analysis_is_torch_stft(geom):
    """every stored layout of analysis() is torch.stft(center=True, pad_mode='reflect') in float64, normalized or not; bins, frame0 and
    frames_out are slices of it; mag / pow / magpow are the functions of its modulus the header names"""
    n, hop, win = geom
    L = 3 * n + 7
    x, w = F.signal(2, L, 3), F.hann(win)
    for normalized in (False, True):
        ref = torch.stft(x.double(), n, hop, win, w.double(), return_complex=True, normalized=normalized).permute(0, 2, 1)       # (R, F, bins)
        sc = 1.0 / math.sqrt(n) if normalized else 1.0
        for kw in (dict(), dict(bins=n // 2, frame0=1, frames_out=2), dict(bins=8)):
            d = F.desc(2, L, n, hop, win, scale=sc, eps=F.EPS, alpha=F.ALPHA, **kw)
            X, mag = F.spectrum(d, x, w)
            r = ref[:, d.frame0:d.frame0 + d.frames_out, :d.bins]
            _close(X, r, 1e-6 if normalized else 1e-10)                                          # the descriptor's scale is a float32
            assert torch.equal(F.to_layout(F.with_(d, mode=F.COMPLEX), X), torch.view_as_real(X.permute(0, 2, 1).contiguous()))
            assert torch.equal(F.from_layout(F.with_(d, mode=F.CAC), F.to_layout(F.with_(d, mode=F.CAC), X)), X)
            assert torch.equal(F.from_layout(F.with_(d, mode=F.FM), F.to_layout(F.with_(d, mode=F.FM), X)), X)
            m = X.abs().permute(0, 2, 1)
            assert torch.equal(F.to_layout(F.with_(d, mode=F.MAG), X), torch.sqrt(torch.clamp(m * m, min=F.f32(F.EPS))))
            assert torch.equal(F.to_layout(F.with_(d, mode=F.POW), X), m * m)
            assert torch.equal(F.to_layout(F.with_(d, mode=F.MAGPOW), X), (m + F.f32(F.EPS)) ** F.f32(F.ALPHA))
            # the magnitude is the l2 norm of the frame's windowed samples: Parseval on the full spectrum
            if d.bins == n // 2 + 1:
                wts = torch.where((torch.arange(d.bins) == 0) | (torch.arange(d.bins) == n // 2), 1.0, 2.0).double()
                _close(((X.abs() ** 2 * wts).sum(-1) / n).sqrt(), mag[..., 0], 1e-6)


@pytest.mark.parametrize("geom", GEOMS)
def test_synthesis_is_torch_istft(geom):
    """synthesis(in_mode 1, herm 1, mul = 1 / envelope, scale = 1 / n_fft) is torch.istft(center=True, length=...) in float64; the
    imaginary parts of DC and Nyquist are ignored; frame0 / a missing Nyquist bin are zero frames / a zero bin"""
    n, hop, win = geom
    frames = 9
    d = F._istft_desc(n, hop, win, 2, frames, F.COMPLEX, cut=3)
    w = F.hann(win)
    S = F.spec_data(d, 5).to(torch.complex128)
    mul = F.inv_envelope(d, w, frames, torch.float64)
    out, _ = F.synthesis(d, S, w, mul)
    clean = S.clone()
    clean[..., 0] = clean[..., 0].real + 0j
    clean[..., -1] = clean[..., -1].real + 0j
    ref = torch.istft(clean.permute(0, 2, 1), n, hop, win, w.double(), length=d.T)
    _close(out, ref, 1e-6)                                                                 # scale = 1 / n_fft is exact; 1e-10 but for the fp32 window
    d2 = F._istft_desc(n, hop, win, 2, frames, F.COMPLEX, frame0=2, frames_in=4, bins=n // 2)
    S2 = torch.zeros_like(S)
    S2[:, 2:6, :n // 2] = S[:, 2:6, :n // 2]
    S2[..., 0] = S2[..., 0].real + 0j
    ref2 = torch.istft(S2.permute(0, 2, 1), n, hop, win, w.double(), length=d2.T)
    out2, b2 = F.synthesis(d2, S[:, 2:6, :n // 2], w, mul)
    _close(out2, ref2, 1e-6)
    assert bool((out2[b2 == 0] == 0).all())                                                # samples no stored frame covers


@pytest.mark.parametrize("geom", GEOMS)
def test_adjoint_pairs(geom):
    """synthesis(herm 0) is the vector-Jacobian product of analysis (extra pads and frame0 included), and analysis(herm 1, in_mode 1,
    mul) that of synthesis(herm 1, in_mode 1, mul): float64 autograd through the reference's own (differentiable) operations"""
    n, hop, win = geom
    w = F.hann(win)
    for kw in (dict(), dict(pads=(hop // 2 * 3, hop + 5), frame0=2, bins=n // 2), dict(scale=0.25)):
        L = 3 * n + 7
        d = F.desc(2, L, n, hop, win, **kw)
        x = F.signal(2, L, 4).double().requires_grad_(True)
        fr = F.windowed_frames(d, x, w.double())
        X = F._dft(fr, d.bins)
        G = F.spec_data(d, 6).to(torch.complex128)
        (X.real * G.real + X.imag * G.imag).sum().backward()
        out, _ = F.synthesis(d, G, w)
        _close(out, x.grad)
    d = F._istft_desc(n, hop, win, 2, 9, F.COMPLEX, cut=3, frame0=1, frames_in=7)
    mul = F.inv_envelope(d, w, 9)
    Sr = torch.view_as_real(F.spec_data(d, 7).to(torch.complex128)).clone().requires_grad_(True)
    out, _ = F.synthesis(d, torch.view_as_complex(Sr), w, mul)
    g = F.signal(2, d.T, 8).double()
    (out * g).sum().backward()
    X, _ = F.spectrum(d, g, w, mul)
    _close(torch.view_as_real(X.contiguous()), Sr.grad)


def test_hdemucs_descriptors():
    """the _spec / _ispec descriptors are oracle/ref_hdemucs.HDemucs._spec / _ispec"""
    from oracle import ref_hdemucs
    for n in (1024, 4096):
        me = types.SimpleNamespace(nfft=n, hop_length=n // 4)
        length = 5 * n + 777
        x = F.signal(2, length, 9).double()
        ref = ref_hdemucs.HDemucs._spec(me, x[None])[0]                                       # (R, n / 2, le)
        d = F._hdemucs_spec_desc(n, 2, length, F.COMPLEX)
        X, _ = F.spectrum(d, x, F.hann(n))
        _close(X.permute(0, 2, 1), ref, 1e-6)
        di = F._hdemucs_ispec_desc(n, 2, length, F.COMPLEX)
        S = F.spec_data(di, 10).to(torch.complex128)
        mul = F.inv_envelope(di, F.hann(n), di.frames_out + 4, torch.float64)
        out, bound = F.synthesis(di, S, F.hann(n), mul)
        _close(out, ref_hdemucs.HDemucs._ispec(me, S.permute(0, 2, 1)[None], length)[0], 1e-6)
        assert bool((bound > 0).all())                                                        # _ispec covers every sample


@pytest.mark.parametrize("geom", ((512, 128, 512), (1024, 120, 600), (2048, 240, 1200)))
def test_loss_is_the_oracle(geom):
    """pair_loss's sums give oracle/ref_losses.stft_loss, and lossgrad_cells through synthesis gives its float64 autograd gradient (away
    from the bands: Gaussian signals, y != x)"""
    from oracle import ref_losses
    n, hop, win = geom
    R, L = 3, 4 * n + 11
    d = F.desc(R, L, n, hop, win, mode=F.FM)
    g = torch.Generator().manual_seed(n)
    x = (0.3 * torch.randn(R, L, generator=g)).double()
    y = x + 0.1 * torch.randn(R, L, generator=g).double()
    w = torch.hann_window(win, dtype=torch.float64)                                         # the oracle's window is float64
    xr = x.clone().requires_grad_(True)
    lref = ref_losses.stft_loss(xr[:, None], y[:, None], n, hop, win, True)
    lref.backward()
    p = F.pair_loss(d, x, y, w, F.EPS)
    s = p["sums"]
    cells = d.frames_out * d.bins
    loss = (s[:, 0].sqrt() / s[:, 1].sqrt()).mean() + s[:, 2].sum() / (R * cells)
    assert abs(float(loss) - float(lref.detach())) <= 1e-12 * abs(float(lref.detach()))
    assert not bool(F.band_cells(p["X"], p["ymag"], F.EPS).any())
    gx, _ = F.synthesis_lossgrad(d, p["X"], p["ymag"], s, 1.0 / R, 1.0 / (R * cells), F.EPS, None, w)
    _close(gx, xr.grad, 1e-6)                                                               # the weights are float32 in the ABI
    # the weighted form of tests/mrstft_scaled_ref.py (scale None, no linear term), value and autograd gradient
    from tests import mrstft_scaled_ref as mref
    xs = x.clone().requires_grad_(True)
    lw = mref.stft_loss(xs[:, None], y[:, None], n, hop, win, w_sc=0.5, w_log_mag=2.0, w_lin_mag=0.0, scale=None, per_example_sc=True, eps=F.EPS)
    lw.backward()
    assert abs(float(0.5 * (s[:, 0].sqrt() / s[:, 1].sqrt()).mean() + 2.0 * s[:, 2].sum() / (R * cells)) - float(lw.detach())) <= 1e-7 * float(lw.detach())
    gw, _ = F.synthesis_lossgrad(d, p["X"], p["ymag"], s, 0.5 / R, 2.0 / (R * cells), F.EPS, None, w)
    _close(gw, xs.grad, 1e-6)
    g2, _ = F.stft_loss_grad(p["X"], p["Y"], s, 1.0 / R, 1.0 / (R * cells), F.EPS)
    g1, _ = F.lossgrad_cells(p["X"], p["ymag"], s, 1.0 / R, 1.0 / (R * cells), F.EPS)
    assert torch.equal(g1, g2)
    # the sums' bound holds the float32 restatement of the spectra
    X32 = F.restate_analysis(d, x, w).to(torch.complex128)
    Y32 = F.restate_analysis(d, y, w).to(torch.complex128)
    assert bool(((F.loss_sums(X32, Y32, F.EPS) - s).abs() <= p["sums_bound"]).all())
    assert bool((p["sums_bound"] <= 1e-3 * s.abs()).all()), (p["sums_bound"] / s.abs()).max()


def test_lossgrad_cells_branches():
    """the discontinuities: no gradient at or below eps, an exactly zero log term where |X| == ymag, ksc = 0 unless A > 0 and B > 0, gup
    multiplies both weights"""
    X = torch.tensor([[0j, 3 + 4j, 6 + 8j, 1e-5 + 0j, 1e-4 + 0j]], dtype=torch.complex128)
    ym = torch.tensor([[1.0, 5.0, 5.0, 1.0, 1.0]])
    sums = torch.tensor([[2.0, 8.0, 0.0]])
    g, m = F.lossgrad_cells(X, ym, sums, 0.5, 0.25, 1e-8)
    assert g[0, 0] == 0 and g[0, 1] == 0 and g[0, 3] == 0 and m[0, 0] == 0 and m[0, 3] == 0        # |X|^2 = 1e-10 < eps; sign 0 and |X| - ymag = 0
    ksc = 0.5 / 4.0
    assert abs(g[0, 2] - (ksc * 5.0 + 0.25 / 10.0) / 10.0 * (6 + 8j)) < 1e-15
    g0, _ = F.lossgrad_cells(X, ym, torch.tensor([[0.0, 8.0, 0.0]]), 0.5, 0.25, 1e-8)
    assert abs(g0[0, 2] - (0.25 / 10.0) / 10.0 * (6 + 8j)) < 1e-15
    gu, _ = F.lossgrad_cells(X, ym, sums, 0.5, 0.25, 1e-8, gup=2.0)
    assert torch.allclose(gu, 2.0 * g, rtol=1e-12, atol=0)
    assert bool(F.band_cells(X[:, 1:2], ym[:, 1:2], 1e-8).all()) and not bool(F.band_cells(X[:, 2:3], ym[:, 2:3], 1e-8).any())


def test_every_form_is_reached():
    """the case tables reach every label the forms functions can return, or the label is listed in UNREACHED with its reason"""
    walk, every = F.walk_all_cases(), F.all_forms()
    stray = walk - every
    assert not stray, sorted(stray)
    assert not (set(F.UNREACHED) & walk), sorted(set(F.UNREACHED) & walk)
    missing = every - walk - set(F.UNREACHED)
    assert not missing, sorted(missing)
    assert all(F.UNREACHED.values())
    assert [F.pair_geometry(c["d"])[0] for c in F.PAIR_NB_CASES] == [2, 4]
    names = [c["name"] for c in F.ANALYSIS_CASES + F.SYNTHESIS_CASES + F.LOSSGRAD_CASES + F.PAIR_CASES + F.PAIR_NB_CASES]
    assert len(set(names)) == len(names)
    # per size: one walk, two walks, three or more with a remainder, in both in_modes
    for n in F.FFT_SIZES:
        for in_mode in (0, 1):
            seen = set()
            for c in F.SYNTHESIS_CASES:
                if c["d"].n_fft == n and c["d"].in_mode == in_mode:
                    seen |= F.forms_synthesis(c["d"], False, c["mul"])
            for lab in ("own_walks1", "own_walks2", "own_walks3_or_more", "own_last_walk_takes_remainder"):
                assert "fft_synthesis_kernel:" + lab in seen, (n, in_mode, lab)
    # the mirrors of the geometry: the issue's figures at 512 / 128 / 512
    assert [F.syn_own_geometry(F.desc(3, (f - 1) * 128 + 3, 512, 128, 512))[2] for f in (16, 32, 55)] == [1, 2, 3]
    assert F.syn_own_geometry(F.desc(3, 2 * 512 + 2, 512, 128, 512))[2] == 0 and F.syn_own_geometry(F.desc(3, 2 * 512 + 3, 512, 128, 512))[2] == 1
    assert F._nb(F.desc(64, 126 * 16 * 16, 512, 16, 512, frames_out=126 * 16, mode=F.FM), False) == 1
    assert F._nb(F.desc(64, 126 * 16 * 16, 512, 16, 512, frames_out=126 * 16 + 1, mode=F.FM), False) == 2
    assert F._nb(F.desc(64, 126 * 16 * 16, 512, 16, 512, frames_out=126 * 16 + 1, mode=F.COMPLEX), False) == 1


@functools.lru_cache(maxsize=None)
def _measured():
    stats = {}
    return F.measure_floors(stats), stats


def test_floors():
    """FLOOR is the measurement rounded up to the next quarter: not below it, and not a figure picked to pass.  The restatement is
    float32 arithmetic of fixed order (fft_ref.fft32), so the figures do not depend on the host."""
    fl, _ = _measured()
    print({k: round(v, 4) for k, v in sorted(fl.items())})
    assert set(fl) == set(F.FLOOR)
    for k, v in fl.items():
        assert v <= F.FLOOR[k], (k, v)
        assert F.FLOOR[k] == math.ceil(v * 4.0) / 4.0, (k, v, F.FLOOR[k])
    v = F.measure_cell_floor()
    print("lossgrad cell", round(v, 4))
    assert v <= F.FLOOR_CELL == math.ceil(v * 4.0) / 4.0, v
    v = F.measure_terms_floor()
    print("loss terms", round(v, 4))
    assert v <= F.FLOOR_TERMS == math.ceil(v * 4.0) / 4.0, v


def test_every_bound_has_power():
    """conditions on the reference alone: every spectrum-cell bound is at most 1e-4 of its frame's rms |X| (= the frame's l2 norm), every
    synthesis bound at most 1e-4 of its row's rms output; and a one-cell error of the size of the cell's own value breaks the bound:
    in every case at most one cell in a thousand has a value within its bound (a Gaussian cell falls within K eps32 ~ 8e-6 of its
    scale with probability ~1e-5, so "every cell" cannot be asserted of Gaussian data: the share is), and the cells the kernels treat
    specially are each checked by name in EVERY case, herm and R = 64 included: DC, n_fft / 4, Nyquist (the self-paired bin of the
    pair transform) and the last stored bin of the first and the last frame are 100 bounds away from 0.  The samples next to the first
    and the last covered one (where a hann window is ~1e-5 of its peak and value and bound shrink together) are non-zero with a bound
    below 5 % of the row's rms.  The interval bounds of mag / pow / magpow (and of the pair kernel's ymag, in test_no_cell_in_a_band):
    doubling |X| moves mag by |X|, pow by 3 |X|^2, magpow by 0.23 of its value -- at most one cell in a thousand has a bound above a
    fifth of its value, and none of the named cells"""
    _, stats = _measured()
    assert set(stats) == {c["name"] for c in F.ANALYSIS_CASES + F.SYNTHESIS_CASES}
    for name, s in stats.items():
        assert s["power"] <= 1e-4, (name, s)
        assert s["weak"] <= 1e-3, (name, s)
    for c in F.ANALYSIS_CASES:
        d = F.with_(c["d"], mode=F.FM, R=1)
        x, w, mul = F.analysis_inputs(c)
        X, mag = F.spectrum(d, x[:1], w, mul)
        b = F.k_of(F.klass("ana", d.n_fft)) * F.EPS32 * mag
        ks = [k for k in (0, d.n_fft // 4, d.n_fft // 2, d.bins - 1) if k < d.bins]
        for f in (0, d.frames_out - 1):
            for k in ks:
                assert float(X[0, f, k].abs()) > 100.0 * float(b[0, f, k]), (c["name"], f, k)
        for mode in c["modes"]:
            if mode in F.SPECTRUM_MODES:
                continue
            dm = F.with_(d, mode=mode)
            v, bm = F.to_layout(dm, X), F.analysis_bound(dm, X, mag)                           # (1, bins, frames)
            assert float((bm > 0.2 * v).double().mean()) <= 1e-3, (c["name"], F.MODE_NAMES[mode])
            for f in (0, d.frames_out - 1):
                for k in ks:
                    assert float(bm[0, k, f]) <= 0.2 * float(v[0, k, f]), (c["name"], F.MODE_NAMES[mode], f, k)
    for c in F.SYNTHESIS_CASES:
        d = F.with_(c["d"], R=1, accum=0)
        S, w, mul, _ = F.synthesis_inputs(c)
        out, bound = F.synthesis(d, S[:1], w, mul)
        cov = torch.nonzero(bound[0] > 0)[:, 0]
        for s_ in (int(cov[1]), int(cov[-2])):                                                # next to the first / last covered sample (a hann window's end is 0)
            assert float(out[0, s_].abs()) > 0.0 and float(bound[0, s_]) <= 0.05 * float(out[0].pow(2).mean().sqrt()), (c["name"], s_)


def test_no_cell_in_a_band():
    """no cell of a loss-gradient or pair-loss case lies within 4 ulp of a discontinuity (the sign of |X| - ymag, the clamp at eps), so the
    fp64 reference and the fp32 kernel take the same branch: by the reference's own values.  The rows of the pair cases with y == x are
    the designated exception (every cell has |X| == |Y|: both numerator sums are exactly 0, which the GPU test asserts)."""
    for c in F.LOSSGRAD_CASES:
        X, ymag, sums, _ = F.lossgrad_inputs(c)
        band = F.band_cells(X, ymag, F.LG_EPS)
        band[..., list(F.LG_DESIGNATED_BINS)] = False
        band[0, list(F.LG_LONE_FRAMES)] = False
        assert not bool(band.any()), c["name"]
        G, m = F.lossgrad_cells(X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS)
        assert bool((G[..., list(F.LG_DESIGNATED_BINS)] == 0).all()) and bool((m[..., [3, 4, 5]] == 0).all())         # bin 6: a zero gradient with a magnitude
        assert float((X[1, 0, 4].real.double() ** 2)) == F.LG_EPS == F.CELL_EPS and 0 < float(X[1, 0, 5].real.double() ** 2) < F.LG_EPS
        assert float(X[1, 0, 6].abs()) == 0.625 == float(ymag[1, 0, 6])
        # the lone band cells of row 0: every other cell of their frames is X = 0 (no gradient, no magnitude)
        b, (fa, fu, fd) = F.LG_LONE_BIN, F.LG_LONE_FRAMES
        other = torch.ones(c["d"].bins, dtype=torch.bool)
        other[b] = False
        for fr in F.LG_LONE_FRAMES:
            assert bool((X[0, fr, other] == 0).all()) and bool((m[0, fr, other] == 0).all()) and float(G[0, fr, b].abs()) > 0
        for px in (X[0, fa, b].to(torch.complex128).abs() ** 2, (X[0, fa, b].imag * X[0, fa, b].imag + X[0, fa, b].real * X[0, fa, b].real).double()):
            assert F.LG_EPS < float(px) <= F.LG_EPS + 2 * float(F.ulp32(torch.tensor(F.LG_EPS)))
        assert float(X[0, fu, b].abs()) == 0.625 == float(X[0, fd, b].abs()) and float(ymag[0, fu, b]) > 0.625 > float(ymag[0, fd, b])
        assert float(ymag[0, fu, b]) - 0.625 == float(F.ulp32(torch.tensor(0.625))) and float(G[0, fu, b].real) < 0 < float(G[0, fd, b].real)
        d0 = F.with_(c["d"], accum=0)
        w = F.hann(d0.win)
        out, bound = F.synthesis_lossgrad(d0, X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"], w)
        for dl in F.lossgrad_sign_deltas(d0, X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"], w):
            assert float((dl.abs() / bound.clamp_min(1e-300))[0].max()) > 1e3, c["name"]            # the two outcomes are thousands of bounds apart
            assert bool((dl[1:] == 0).all())
        assert float(sums[-1, 0]) == 0.0 and bool((sums[:-1, :2] > 0).all())
    for c in F.PAIR_CASES:
        d = c["d"]
        x, y, w = F.pair_inputs(c)
        p = F.pair_loss(d, x, y, w, F.EPS)
        lo = 1 if d.R > 1 else 0
        assert not bool(F.band_cells(p["X"][lo:], p["ymag"][lo:], F.EPS).any()), c["name"]
        assert float((p["ymag_bound"] > 0.2 * p["ymag"]).double().mean()) <= 1e-3, c["name"]     # the power of ymag's interval bound
        e = F.f32(F.EPS)
        for Z in (p["X"], p["Y"]):
            px = Z.real ** 2 + Z.imag ** 2
            assert not bool(((px - e).abs() <= 4 * float(F.ulp32(torch.tensor(e)))).any()), c["name"]
        if lo:
            assert torch.equal(p["X"][0], p["Y"][0]) and float(p["sums"][0, 0]) == 0.0 and float(p["sums"][0, 2]) == 0.0


def test_lossgrad_bound_has_power():
    """the loss-gradient synthesis: the bound is at most 1e-4 of the row's rms gradient in every case, as for every other synthesis
    (|X| spreads over 0.5 .. 2 only: over three decades the 1 / |X| weight of the small cells dominated the frames' magnitude), and
    the fp32 restatement of the cell formula through the fp32 synthesis stays inside it"""
    for c in F.LOSSGRAD_CASES:
        d = F.with_(c["d"], accum=0)
        X, ymag, sums, w = F.lossgrad_inputs(c)
        out, bound = F.synthesis_lossgrad(d, X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"], w)
        assert float((bound / out.pow(2).mean(1, keepdim=True).sqrt()).max()) <= 1e-4, c["name"]
        G, _ = F.lossgrad_cells(X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.LG_EPS, c["gup"])
        o32 = F.restate_synthesis(d, G.to(torch.complex64), w)
        assert bool(((o32.double() - out).abs() <= bound).all()), c["name"]


def test_cell_kernel_inputs():
    """the inputs of the three cell kernels: only the designated cells lie in a band, each designated cell is what its name says in
    float32 and in fp64 alike (so the reference and the kernel take the same branch and the exact outcomes are exact), and the sums'
    bound is at most 1e-4 of each sum (a single cell's squared difference carries (|X| + |Y|) / ||X| - |Y|| roundings)"""
    e = F.f32(F.CELL_EPS)
    for R in F.CELL_R:
        for n in F.CELL_N:
            X, Y, ymag, sums = F.cell_inputs(R, n, 100 * R + n)
            des = F.designated_mask(n)
            assert not bool(F.band_cells(X, ymag, F.CELL_EPS)[:, ~des].any()), (R, n)
            assert not bool(F.band_cells(X, F.clamped_mag(Y.to(torch.complex128), F.CELL_EPS), F.CELL_EPS)[:, ~des].any()), (R, n)
            s = F.loss_sums(X, Y, F.CELL_EPS)
            z = torch.zeros(R, n, dtype=torch.float64)
            b = F.loss_sums_bound(X.to(torch.complex128), Y.to(torch.complex128), z, z, F.CELL_EPS, group=8)
            assert bool((b <= 1e-4 * s.abs()).all()), (R, n, (b / s.abs()).max())
            if n < 255:
                continue
            c = F.DESIGNATED_COL
            x64, x32 = X.to(torch.complex128), X
            p64 = (x64.real ** 2 + x64.imag ** 2)[0, c:c + 7]
            p32 = (x32.imag * x32.imag + x32.real * x32.real)[0, c:c + 7].double()
            for p in (p64, p32):
                assert float(p[0]) == 0.0 and float(p[1]) < e and float(p[2]) == e and float(p[3]) > e
                assert float((p[1] - e).abs()) <= 4 * float(F.ulp32(torch.tensor(e))) and float((p[3] - e).abs()) <= 4 * float(F.ulp32(torch.tensor(e)))
                assert bool((p[4:7].sqrt() == 0.625).all())
            assert float(ymag[0, c + 4]) == 0.625 and float(ymag[0, c + 5]) > 0.625 > float(ymag[0, c + 6])
            G, mag = F.lossgrad_cells(X, ymag, sums, F.LG_W_SC, F.LG_W_LM, F.CELL_EPS)
            assert bool((G[:, c:c + 3] == 0).all()) and bool((G[:, c + 4] == 0).all()) and bool((G[:, c + 3].abs() > 0).all())
            assert bool((G[:, c + 5].real < 0).all()) and bool((G[:, c + 6].real > 0).all())            # the log term's sign follows |X| - ymag
            # a wrong branch at a designated cell is far outside the bound
            b = F.k_cell() * F.EPS32 * mag
            assert bool((b[:, c + 3] < 1e-4 * G[:, c + 3].abs()).all()) and bool((b[:, c + 4:c + 7] < 1e-4 * G[:, c + 5].abs().min()).all())
