"""CPU: the host side of the generic framed FFT (every power-of-two n_fft from 16 to 32768): the descriptor's range check, the
synthesis scratch size, the mel limit of the MR-STFT loss, and that the references and bounds tests/test_gpu_fft_any.py holds the
kernels to are met, with margin, by torch's own fp32 transform."""
import ctypes as C

import pytest
import torch

from tests import fft_any_ref as ref


def _d(n_fft, hop=None, win=None, R=3, T=None, mode=0):
    from remfx_amd import stft
    hop, win = hop or n_fft // 4, win or n_fft
    T = T or 3 * n_fft + 7
    return stft._desc(R, T, n_fft, hop, win, n_fft // 2 + 1, 0, 1 + T // hop, mode)


def test_desc_accepts_every_power_of_two():
    for k in range(4, 16):
        d = _d(1 << k)
        assert d.n_fft == 1 << k


@pytest.mark.parametrize("n_fft", [8, 48, 1000, 65536])
def test_desc_rejects_other_lengths(n_fft):
    with pytest.raises(ValueError, match="16 to 32768"):
        _d(n_fft)


@pytest.mark.parametrize("geom", ref.GEOMS)
def test_synthesis_scratch_holds_the_frames(geom):
    from remfx_amd import _lib
    _lib.build()                                                     # hipcc cross-compiles without a GPU
    n_fft, hop, win = geom
    for L in ref.lengths(n_fft, hop):
        d = _d(n_fft, hop, win, R=ref.R, T=L)
        frames = 1 + L // hop
        ws = int(_lib.lib().rfx_fft_synthesis_ws(C.byref(d)))
        assert ws > 0 and ws >= ref.R * frames * n_fft, (ws, ref.R * frames * n_fft)
        d2 = _d(n_fft, hop, win, R=ref.R, T=L)                      # a stored sub-range of frames (HDemucs _ispec) needs only those
        d2.frame0, d2.frames_out = 1, frames - 2
        assert int(_lib.lib().rfx_fft_synthesis_ws(C.byref(d2))) >= ref.R * (frames - 2) * n_fft


def test_mel_above_4096_raises_at_construction():
    from remfx_amd import losses
    kw = dict(scale="mel", n_bins=64, sample_rate=48000)
    with pytest.raises(NotImplementedError, match=r"resolution 0 \(n_fft=8192\)"):
        losses.MultiResolutionSTFTLoss(fft_sizes=(8192,), hop_sizes=(2048,), win_lengths=(8192,), **kw)
    with pytest.raises(NotImplementedError, match=r"resolution 1 \(n_fft=16384\)"):
        losses.MultiResolutionSTFTLoss(fft_sizes=(2048, 16384), hop_sizes=(512, 4096), win_lengths=(2048, 16384), **kw)
    with pytest.raises(NotImplementedError, match="resolution 0"):
        losses.STFTLoss(8192, 2048, 8192, **kw)
    m = losses.MultiResolutionSTFTLoss(fft_sizes=(2048,), hop_sizes=(512,), win_lengths=(2048,), **kw)
    assert len(m.filterbanks) == 1
    losses.MultiResolutionSTFTLoss(fft_sizes=(8192,), hop_sizes=(2048,), win_lengths=(8192,), w_lin_mag=1.0)   # linear scale: no limit


@pytest.mark.parametrize("case", ref.CASES)
def test_fp32_torch_meets_half_of_every_forward_bound(case):
    """The fp64 reference and the bounds are sound: torch.stft in fp32, which rounds like any fp32 FFT, stays below HALF of each bound
    the device kernels are held to on the same inputs."""
    n_fft, hop, win, L = case
    r64, r32, scale = ref.forward_refs(n_fft, hop, win, L)
    for m in ref.MODES:
        err, bound = ref.rms(r32[m], r64[m]), ref.fwd_bound(m, n_fft, scale)
        print(f"n_fft={n_fft} hop={hop} win={win} L={L} {m}: fp32 torch error {err:.3e}, bound {bound:.3e}")
        assert err < 0.5 * bound, (m, err, bound)


@pytest.mark.parametrize("variant", sorted(ref.MR_VARIANTS))
def test_fp32_torch_meets_half_of_the_loss_gradient_bound(variant):
    """The MR-STFT loss inputs (tests/fft_any_ref.py: how the seed was chosen) are ones on which fp32 arithmetic CAN meet the bound
    the device is held to: torch's fp32 autograd against fp64."""
    l64, g64 = ref.loss_ref(variant)
    l32, g32 = ref.loss_ref(variant, torch.float32)
    err, bound = ref.rms(g32, g64), 1e-4 * float(g64.abs().max())
    print(f"{variant}: fp32 torch loss {l32:.7f} vs {l64:.7f}, gradient error {err:.3e}, bound {bound:.3e}")
    assert abs(l32 - l64) < 0.5 * 1e-4 * abs(l64)
    assert err < 0.5 * bound
