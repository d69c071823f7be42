"""CPU: the Wiener / expectation-maximisation restatements of tests/wiener_ref.py checked against what the algorithm must satisfy
 -- they are the reference tests/test_gpu_wiener_kernel.py judges the kernel by, and upstream's source is not here."""
import numpy as np
import pytest

from tests import wiener_ref as wr


def test_niter0_is_magnitude_times_phase():
    X, S = wr.make_case(1, 2, 2, 3, 5, 7)
    Y = wr.wiener64(X, S, 2, 2, 3)
    Xr = X.astype(np.complex128).reshape(2, 2, 5, 7)
    ph = np.where(np.abs(Xr) > 0, Xr / np.where(np.abs(Xr) > 0, np.abs(Xr), 1), 1)
    want = S.astype(np.float64).reshape(3, 2, 2, 5, 7).transpose(1, 0, 2, 3, 4) * ph[:, None]
    assert Y.shape == (2, 3, 2, 5, 7) and np.array_equal(Y, want)
    assert Y[-1, :, -1, -1, 0].imag.max() == 0 and np.array_equal(Y[-1, :, -1, -1, 0].real, S[:, -1, -1, 0])    # X = 0: phase 1
    Y32 = wr.wiener32(X, S, 2, 2, 3)
    assert Y32.dtype == np.complex64 and np.abs(Y32 - Y).max() < 1e-6 * np.abs(X).max()


def test_mono_em_step_is_the_scalar_wiener_gain():
    X, S = wr.make_case(2, 1, 1, 3, 4, 9)
    x = X.astype(np.complex128).reshape(1, 4, 9)
    y = wr.initial(x, S.astype(np.float64).reshape(3, 1, 4, 9), False, False)
    got = wr.em_step(x, y)
    v = np.abs(y[:, 0]) ** 2                                                # (J, bins, n)
    R = v.sum(-1) / (wr.EPS + v.sum(-1))                                    # (J, bins)
    gain = v * R[..., None] / (np.sqrt(wr.EPS) + (v * R[..., None]).sum(0))
    assert np.abs(got[:, 0] - x[0] * gain).max() < 1e-13 * np.abs(x).max()


@pytest.mark.parametrize("softmask", [False, True])
def test_residual_completes_the_mixture(softmask):
    X, S = wr.make_case(3, 2, 2, 2, 5, 8)
    Y = wr.wiener64(X, S, 2, 2, 8, softmask=softmask, residual=True)
    assert Y.shape[1] == 3
    assert np.abs(Y.sum(1) - X.astype(np.complex128).reshape(2, 2, 5, 8)).max() < 1e-14 * np.abs(X).max()


def test_windows_are_independent():
    X, S = wr.make_case(4, 1, 2, 2, 3, 10)
    Y = wr.wiener64(X, S, 1, 2, 4, niter=2, residual=True)
    for t0, n in ((0, 4), (4, 4), (8, 2)):
        alone = wr.wiener64(X[..., t0:t0 + n], S[..., t0:t0 + n], 1, 2, 4, niter=2, residual=True)
        assert np.array_equal(Y[..., t0:t0 + n], alone), t0
    X2 = X.copy()
    X2[..., 8:] *= 3                                                        # another window's mixture: the first two do not move
    Y2 = wr.wiener64(X2, S, 1, 2, 4, niter=2, residual=True)
    assert np.array_equal(Y2[..., :8], Y[..., :8]) and not np.array_equal(Y2[..., 8:], Y[..., 8:])


def test_scale_step_makes_the_filter_homogeneous():
    """X and S times 100 -> Y times 100: step B divides both by m, and eps is negligible against unit-scale data"""
    X, S = wr.make_case(5, 1, 2, 3, 4, 12, amp=30.0)                        # max |X| / 10 > 1 before and after
    Y = wr.wiener64(X, S, 1, 2, 12, niter=2)
    Yk = wr.wiener64(X.astype(np.complex128) * 100, S.astype(np.float64) * 100, 1, 2, 12, niter=2)
    assert np.abs(Yk - 100 * Y).max() < 1e-9 * 100 * np.abs(X).max()
    assert wr.window_scales(X, 1, 2, 12).max() > 10


def test_fp32_restatement_follows_the_fp64_one():
    """the figure the kernel's bound is made of: on inputs of this kind it is a few fp32 roundings of the window's scale"""
    for seed, (C, J0, res, soft, niter, amp) in enumerate([(1, 2, True, False, 2, 1.0), (2, 4, True, False, 1, 300.0),
                                                             (2, 8, False, True, 2, 0.1), (2, 2, False, False, 3, 30.0)]):
        X, S = wr.make_case(10 + seed, 2, C, J0, 5, 134, amp)
        a, b = wr.wiener64(X, S, 2, C, 64, niter, soft, res), wr.wiener32(X, S, 2, C, 64, niter, soft, res)
        s = wr.window_scales(X, 2, C, 64)[:, None, None, None, :]
        e32 = float((np.abs(b - a) / s).max())
        assert b.dtype == np.complex64 and e32 <= 1e-5, (seed, e32)


def test_single_source_cannot_iterate():
    X, S = wr.make_case(6, 1, 1, 1, 2, 4)
    with pytest.raises(ValueError):
        wr.wiener64(X, S, 1, 1, 4, niter=1)
