"""The seeded (oracle, HIP) pair of small Hybrid Demucs models that test_gpu_hdemucs.py and test_gpu_bf16x3.py compare."""
import torch


def pair(channels, seed=0, dev="cuda:0"):
    from oracle import ref_hdemucs
    from remfx_amd.hdemucs import HDemucs
    torch.manual_seed(seed)
    ref = ref_hdemucs.HDemucs(sources=["mixture"], audio_channels=1, nfft=4096, channels=channels)
    # make LayerScale / freq-emb paths numerically visible
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith(".scale"):
                p.fill_(0.3)
    net = HDemucs(sources=["mixture"], audio_channels=1, nfft=4096, channels=channels)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.to(dev)
