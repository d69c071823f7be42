"""Open-Unmix (sigsep/open-unmix-pytorch `OpenUnmix` + `Separator` as RemFX configures them:
reference remfx/models.py:259-304, cfg/model/umx.yaml:11-16) on the HIP kernels.

Same parameter names as upstream (fc1/bn1/lstm/fc2/bn2/fc3/bn3, input_mean, input_scale,
output_scale, output_mean).  Layout: the network runs channel-major, (1, features, frames*batch), so
every Linear is a 1x1 gather-GEMM with the position axis contiguous and BatchNorm1d is the same
per-channel reduction kernel the classifier uses; with two channels the features are channel-major, c * bins + k, as
upstream's reshape(-1, nb_channels * nb_bins).  STFT / magnitude, the magnitude x mixture-phase
product and the iSTFT are HIP kernels; the 3-layer BiLSTM is the persistent HIP recurrence of remfx_amd/lstm.py.

Separator covers upstream's interface: any number of targets (at most 8 sources with the residual), niter >= 0, softmask,
residual, one or two channels, wiener_win_len.  The default mode (niter = 0, no softmask, no residual) is magnitude x
mixture phase per target through rfx_phase_mask_fwd / _bwd and stays differentiable; every other mode is the multichannel
Wiener filter with expectation-maximisation of csrc/wiener.hip: one fused launch over all samples,
windows and bins, forward only.  Not built: unidirectional=True, max_bin, input_mean= / input_scale=, more than two
channels, windows longer than rfx_wiener_max_window() frames.
"""
import torch
import torch.nn as nn

from . import lstm, nnops, ops, stft
from .ops import launch, query


class OpenUnmix(nn.Module):
    def __init__(self, nb_bins=4096, nb_channels=2, hidden_size=512, nb_layers=3, unidirectional=False,
                 input_mean=None, input_scale=None, max_bin=None):
        super().__init__()
        if max_bin is not None or input_mean is not None or input_scale is not None:
            raise NotImplementedError("RemFX constructs OpenUnmix(nb_channels, nb_bins) only (models.py:278-281)")
        self.nb_output_bins = self.nb_bins = nb_bins
        self.hidden_size = hidden_size
        self.fc1 = nn.Linear(nb_bins * nb_channels, hidden_size, bias=False)
        self.bn1 = nn.BatchNorm1d(hidden_size)
        lstm_hidden = hidden_size if unidirectional else hidden_size // 2
        self.lstm = nn.LSTM(hidden_size, lstm_hidden, num_layers=nb_layers, bidirectional=not unidirectional,
                            batch_first=False, dropout=0.4 if nb_layers > 1 else 0)
        self.fc2 = nn.Linear(hidden_size * 2, hidden_size, bias=False)
        self.bn2 = nn.BatchNorm1d(hidden_size)
        self.fc3 = nn.Linear(hidden_size, nb_bins * nb_channels, bias=False)
        self.bn3 = nn.BatchNorm1d(nb_bins * nb_channels)
        self.input_mean = nn.Parameter(torch.zeros(nb_bins))
        self.input_scale = nn.Parameter(torch.ones(nb_bins))
        self.output_scale = nn.Parameter(torch.ones(nb_bins))
        self.output_mean = nn.Parameter(torch.ones(nb_bins))

    def forward(self, x):
        """x: (B, C, bins, frames) magnitude, C in {1, 2} -> same shape."""
        ops._req(x, "x")
        B, Cc, nb, nf = x.shape
        if Cc not in (1, 2):
            raise NotImplementedError("one or two channels (got %d)" % Cc)
        P = nf * B
        # the per-bin parameters broadcast over the channels
        per = (lambda p: p.view(1, -1, 1)) if Cc == 1 else (lambda p: p.repeat(Cc).view(1, -1, 1))
        # channel-major: (1, C*bins, frames*batch), feature c*bins + k, position p = f*B + b  (== upstream's (F, B, C, bins) rows)
        mix = x.detach().reshape(B, Cc * nb, nf).permute(1, 2, 0).reshape(1, Cc * nb, P).contiguous()
        h = (mix + per(self.input_mean)) * per(self.input_scale)
        h = ops.conv1d(h, self.fc1.weight.unsqueeze(-1))
        h = ops.activation(nnops.batch_norm(h, self.bn1, self.bn1.training), "tanh")            # (1, 512, P)
        lo = lstm.blstm(self.lstm, h, nf, B)                                                         # (1, 512, P)
        cat = torch.cat([h, lo], 1)
        h = nnops.batch_norm(ops.conv1d(cat, self.fc2.weight.unsqueeze(-1)), self.bn2, self.bn2.training, relu=True)
        h = nnops.batch_norm(ops.conv1d(h, self.fc3.weight.unsqueeze(-1)), self.bn3, self.bn3.training)
        h = h * per(self.output_scale) + per(self.output_mean)
        y = ops.activation(h, "relu") * mix                                                          # (1, C*bins, P)
        return y.view(Cc * nb, nf, B).permute(2, 0, 1).reshape(B, Cc, nb, nf)


class _PhaseMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mag, xc):
        mag = mag.contiguous()
        out = torch.empty_like(xc)
        launch("rfx_phase_mask_fwd", mag, xc, out, mag.numel())
        ctx.save_for_backward(xc)
        return out

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        gm = torch.empty(xc.shape[:-1], device=xc.device, dtype=torch.float32)
        launch("rfx_phase_mask_bwd", xc, g.contiguous(), gm, gm.numel())
        return gm, None


MAX_SOURCES = 8                                   # rfx_wiener: J0 + residual


class Separator(nn.Module):
    """umx Separator(target_models, niter, softmask, residual, ..., nb_channels, wiener_win_len): (B, C, T) -> (B, J, C, T), the
    targets in dict order, then the residual.  niter = 0 without softmask and residual: magnitude x mixture phase per target,
    differentiable; every other mode: rfx_wiener, forward only."""

    def __init__(self, target_models, niter=0, softmask=False, residual=False, sample_rate=44100.0, n_fft=4096,
                 n_hop=1024, nb_channels=2, wiener_win_len=300, filterbank="torch"):
        super().__init__()
        niter, softmask, residual = int(niter), bool(softmask), bool(residual)
        nb_sources = len(target_models) + residual
        if niter < 0 or len(target_models) < 1 or nb_channels < 1:
            raise ValueError("Separator needs niter >= 0, at least one target model and at least one channel")
        if niter > 0 and nb_sources == 1:
            raise ValueError("Cannot use EM if only one target is estimated. Provide two targets or create an additional "
                             "one with `residual=True`")
        if nb_channels > 2:
            raise NotImplementedError("the Wiener filter inverts the spatial covariance in closed form: at most 2 channels (got %d)"
                                      % nb_channels)
        if nb_sources > MAX_SOURCES:
            raise NotImplementedError("at most %d sources, the residual included (got %d)" % (MAX_SOURCES, nb_sources))
        self.plain = niter == 0 and not softmask and not residual
        if wiener_win_len is not None:
            wiener_win_len = int(wiener_win_len)
            if wiener_win_len < 1:
                raise ValueError("wiener_win_len must be positive or None")
            if not self.plain and wiener_win_len > query("rfx_wiener_max_window"):
                raise NotImplementedError("wiener_win_len %d is above the %d frames one workgroup keeps on chip "
                                          "(rfx_wiener_max_window)" % (wiener_win_len, query("rfx_wiener_max_window")))
        self.target_models = nn.ModuleDict(target_models)
        self.nb_targets = len(self.target_models)
        self.niter, self.softmask, self.residual, self.wiener_win_len = niter, softmask, residual, wiener_win_len
        self.n_fft, self.n_hop, self.nb_channels = n_fft, n_hop, nb_channels
        self.register_buffer("sample_rate", torch.as_tensor(sample_rate), persistent=False)

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def forward(self, audio):
        ops._req(audio, "audio")
        B, Cc, T = audio.shape
        xc = stft.stft(audio.reshape(B * Cc, T), self.n_fft, self.n_hop, mode="complex").detach()   # (B*C, bins, F, 2)
        X = stft.stft(audio.reshape(B * Cc, T), self.n_fft, self.n_hop, mode="mag", eps=0.0)        # |X|
        X = X.view(B, Cc, X.shape[-2], X.shape[-1])
        if self.plain:
            ys = []
            for model in self.target_models.values():
                mag = model(X)
                Y = _PhaseMaskFn.apply(mag.reshape(B * Cc, mag.shape[-2], mag.shape[-1]), xc)
                ys.append(stft.istft(Y, self.n_fft, self.n_hop, mode="complex", length=T).view(B, Cc, T))
            return ys[0].view(B, 1, Cc, T) if len(ys) == 1 else torch.stack(ys, 1)
        if Cc > 2:
            raise NotImplementedError("the Wiener filter takes at most 2 channels (got %d)" % Cc)
        bins, frames = X.shape[-2:]
        W = frames if self.wiener_win_len is None else self.wiener_win_len
        if W > query("rfx_wiener_max_window"):
            raise NotImplementedError("wiener_win_len=None on %d frames: one window above the %d frames one workgroup keeps on chip "
                                      "(rfx_wiener_max_window)" % (frames, query("rfx_wiener_max_window")))
        J0, J = self.nb_targets, self.nb_targets + self.residual
        S = torch.empty((J0, B * Cc, bins, frames), device=audio.device, dtype=torch.float32)     # the models' magnitudes, written once
        for j, model in enumerate(self.target_models.values()):
            mag = model(X)
            if torch.is_grad_enabled() and mag.requires_grad:
                raise RuntimeError("Separator with niter > 0, softmask or residual is forward only: there is no gradient through the "
                                   "Wiener filter.  Call it under torch.no_grad() or freeze() it")
            S[j].copy_(mag.detach().reshape(B * Cc, bins, frames))
        ws = torch.empty((max(1, query("rfx_wiener_ws_floats", B, Cc, bins, frames, W)),), device=audio.device, dtype=torch.float32)
        Y = torch.empty((B, J, Cc, bins, frames, 2), device=audio.device, dtype=torch.float32)
        launch("rfx_wiener", xc, S, Y, B, Cc, J0, int(self.residual), bins, frames, W, self.niter, int(self.softmask), ws)
        y = stft.istft(Y.view(B * J * Cc, bins, frames, 2), self.n_fft, self.n_hop, mode="complex", length=T)
        return y.view(B, J, Cc, T)

    def to_dict(self, estimates, aggregate_dict=None):
        """(B, J, C, T) -> {target name: (B, C, T)}, the residual under "residual"; aggregate_dict {name: [targets]} sums groups"""
        out = {name: estimates[:, k] for k, name in enumerate(self.target_models)}
        if self.residual:
            out["residual"] = estimates[:, -1]
        if aggregate_dict is not None:
            out = {key: sum(out[t] for t in targets) for key, targets in aggregate_dict.items()}
        return out
