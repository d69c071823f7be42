"""Every torch.autograd.Function subclass under remfx_amd/ -> the tests/test_gpu_*.py module that runs its forward AND backward against a
reference.  tests/test_host_cpu.py::test_every_autograd_node_is_pinned keeps the keys equal to the code (found with
ast) and checks that the module exists and names the node, a wrapper that applies it, or a case table that does.

The layer ops of ops.py / nnops.py are pinned at their seams by test_gpu_nodes.py (case table: tests/node_ref.py); the entries were
filled by reading the modules, not by searching for names."""

NODES = "test_gpu_nodes.py"

PINNED_BY = {
    # ops.py
    "ops.Conv2dFn": NODES, "ops.ConvFork2dFn": NODES, "ops.ConvGlu2dFn": NODES, "ops.ConvT2dFn": NODES,
    "ops.ActFn": NODES, "ops.ActAddFn": NODES, "ops.ActToFn": NODES,
    # nnops.py
    "nnops._GroupNormFn": NODES, "nnops._BatchNormFn": NODES, "nnops._AvgPoolFn": NODES, "nnops._GluFn": NODES, "nnops._AddFn": NODES,
    "nnops._MulFn": NODES, "nnops._RowAffineFn": NODES, "nnops._CmToFmAffineFn": NODES, "nnops._RowAffineAddFn": NODES,
    "nnops._LocalStateFn": NODES, "nnops._BlstmFrameFn": NODES, "nnops._BlstmUnframeFn": NODES, "nnops._DropoutFn": NODES,
    "nnops._DConvLayerFn": NODES,                     # node_ref.dconv_cases(): test_dconv_node
    # the fused blocks of the networks: forward and backward against the oracle / an fp64 restatement in their own modules
    "clchain.EncMidFn": "test_gpu_clchain.py", "clchain.EncTailFn": "test_gpu_clchain.py", "clchain.FreqDecoderFn": "test_gpu_clchain.py",
    "clchain.HeadGeluFn": "test_gpu_clchain.py", "clchain.HeadConvFn": "test_gpu_clchain.py",
    "cldconv.ClDconvLayerFn": "test_gpu_cldconv.py",
    "dcunet._CplxNormActFn": "test_gpu_dcunet.py", "dcunet._JoinFn": "test_gpu_dcunet.py", "dcunet._BoundMaskFn": "test_gpu_dcunet.py",
    "dptnet._MhaFn": "test_gpu_dptnet.py", "dptnet._PReLUFn": "test_gpu_dptnet.py",
    "losses._MRSTFTFn": "test_gpu_mrstft_scaled.py", "losses._L1Fn": "test_gpu_stft.py", "losses._TimeLossFn": "test_gpu_time_loss.py",
    "losses._FIRFn": "test_gpu_fir.py", "losses._SumDiffFn": "test_gpu_fir.py",
    "lstm._LSTMLayerFn": "test_gpu_lstm.py",
    "stft.STFTFn": "test_gpu_stft.py", "stft.ISTFTFn": "test_gpu_stft.py",
    "tcn.TCNBlockFn": "test_gpu_conv.py",
    "umx._PhaseMaskFn": "test_gpu_umx.py",
}

# what the pinning module names where it does not name the class: the public wrapper or module class that applies the node
VIA = {
    "clchain.EncMidFn": "clchain", "clchain.EncTailFn": "clchain", "clchain.FreqDecoderFn": "clchain", "clchain.HeadGeluFn": "clchain",
    "clchain.HeadConvFn": "clchain", "cldconv.ClDconvLayerFn": "cldconv", "dcunet._CplxNormActFn": "dcunet", "dcunet._JoinFn": "dcunet",
    "dcunet._BoundMaskFn": "dcunet", "dptnet._MhaFn": "dptnet", "dptnet._PReLUFn": "dptnet", "losses._MRSTFTFn": "MultiResolutionSTFTLoss",
    "losses._L1Fn": "L1Loss", "losses._TimeLossFn": "losses", "losses._FIRFn": "FIRFilter", "losses._SumDiffFn": "SumAndDifference",
    "lstm._LSTMLayerFn": "lstm", "stft.STFTFn": "stft", "stft.ISTFTFn": "istft", "tcn.TCNBlockFn": "TCN", "umx._PhaseMaskFn": "umx",
}
