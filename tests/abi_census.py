"""Which test module pins each entry point of include/remfx_hip.h: every key of remfx_amd._lib.SIGNATURES against the
tests/test_gpu_*.py module that calls it through the C ABI and judges what it wrote per element -- or tests/test_host_cpu.py for the
queries that never touch a device.  tests/test_host_cpu.py::test_every_entry_point_is_pinned keeps it true: the keys are the ABI, every
module exists, and the entry's name stands in that module, in a tests/*_ref.py it imports (the launch helpers of gemm_ref, clast_ref,
cldconv_ref ...) or in the remfx_amd wrapper it imports and calls (VIA says which, for the entries no test names).

There is no "unpinned" value.  Filled by reading each module, not by searching for names."""
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))
HOST_ONLY = "test_host_cpu.py"

# entries reached through a wrapper: the wrapper, and the per-element check behind it
VIA = {
    "rfx_cl_pack": ("remfx_amd/clast.py", "clast.pack: test_pack_with_structural_zeros, every packed bf16 equal to the rounded source element (0 at the structural zeros)"),
    "rfx_cl_to_cm": ("remfx_amd/clast.py", "clast.to_cm: test_to_cm judges every element of the channel-major copy (fp32 and bf16 targets)"),
    "rfx_cl_dgelu": ("remfx_amd/clast.py", "clast.dgelu: test_dgelu_dglu, clast_ref.from_cm_judge per element"),
    "rfx_cl_dglu": ("remfx_amd/clast.py", "clast.dglu: the same test"),
    "rfx_pack_a": ("remfx_amd/ops.py", "ops.pack_cached in gemm_ref.launch: every forward case's output is judged per element from the packed weights"),
    "rfx_unpack_set": ("remfx_amd/ops.py", "ops.unpack_set in gemm_ref.launch (weight-gradient cases, unpack 'set'): dw in a guarded buffer, judged per element"),
    "rfx_unpack_add": ("remfx_amd/ops.py", "ops.unpack_add in gemm_ref.launch (unpack 'add'): dw accumulated onto dw0, judged per element"),
}

PINNED_BY = {
    # test_gpu_attention_kernel.py
    "rfx_localstate_bwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_fwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_gen_bwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_gen_fwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_mfma_bwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_mfma_fwd": "test_gpu_attention_kernel.py",
    "rfx_localstate_mfma_ok": "test_gpu_attention_kernel.py",
    "rfx_mha_bwd": "test_gpu_attention_kernel.py",
    "rfx_mha_fwd": "test_gpu_attention_kernel.py",
    # test_gpu_clast_kernel.py
    "rfx_cl_conv": "test_gpu_clast_kernel.py",
    "rfx_cl_conv_variant": "test_gpu_clast_kernel.py",
    "rfx_cl_dgelu": "test_gpu_clast_kernel.py",
    "rfx_cl_dglu": "test_gpu_clast_kernel.py",
    "rfx_cl_from_cm": "test_gpu_clast_kernel.py",
    "rfx_cl_im2col_fm": "test_gpu_clast_kernel.py",
    "rfx_cl_im2col_s4": "test_gpu_clast_kernel.py",
    "rfx_cl_pack": "test_gpu_clast_kernel.py",
    "rfx_cl_rowsum": "test_gpu_clast_kernel.py",
    "rfx_cl_rowsum_ws": "test_gpu_clast_kernel.py",
    "rfx_cl_to_cm": "test_gpu_clast_kernel.py",
    "rfx_cl_wgrad": "test_gpu_clast_kernel.py",
    "rfx_cl_wgrad_reduce": "test_gpu_clast_kernel.py",
    "rfx_cl_wgrad_variant": "test_gpu_clast_kernel.py",
    "rfx_cl_wgrad_ws_floats": "test_gpu_clast_kernel.py",
    # test_gpu_cldconv_kernel.py
    "rfx_cl_dconv_bwd": "test_gpu_cldconv_kernel.py",
    "rfx_cl_dconv_bwd_ws_partial": "test_gpu_cldconv_kernel.py",
    "rfx_cl_dconv_bwd_ws_sums": "test_gpu_cldconv_kernel.py",
    "rfx_cl_dconv_bwd_ws_tsum": "test_gpu_cldconv_kernel.py",
    "rfx_cl_dconv_fwd": "test_gpu_cldconv_kernel.py",
    "rfx_cl_dconv_fwd_ws_partial": "test_gpu_cldconv_kernel.py",
    # test_gpu_cplx_kernel.py
    "rfx_bound_mask_bwd": "test_gpu_cplx_kernel.py",
    "rfx_bound_mask_fwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_affine_act_bwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_affine_act_bwd_ws": "test_gpu_cplx_kernel.py",
    "rfx_cplx_affine_act_fwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_coef_bwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_coef_fwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_moments": "test_gpu_cplx_kernel.py",
    "rfx_cplx_moments_bwd": "test_gpu_cplx_kernel.py",
    "rfx_cplx_moments_ws": "test_gpu_cplx_kernel.py",
    "rfx_phase_mask_bwd": "test_gpu_cplx_kernel.py",
    "rfx_phase_mask_fwd": "test_gpu_cplx_kernel.py",
    # test_gpu_dconv_kernel.py
    "rfx_dconv_layer_bwd": "test_gpu_dconv_kernel.py",
    "rfx_dconv_layer_bwd_ws": "test_gpu_dconv_kernel.py",
    "rfx_dconv_layer_fwd": "test_gpu_dconv_kernel.py",
    "rfx_dconv_layer_ok": "test_gpu_dconv_kernel.py",
    # test_gpu_elem_kernel.py
    "rfx_act_add_fwd": "test_gpu_elem_kernel.py",
    "rfx_act_bwd": "test_gpu_elem_kernel.py",
    "rfx_act_fwd": "test_gpu_elem_kernel.py",
    "rfx_act_rows": "test_gpu_elem_kernel.py",
    "rfx_act_rows16": "test_gpu_elem_kernel.py",
    "rfx_add_bcast": "test_gpu_elem_kernel.py",
    "rfx_blstm_frames": "test_gpu_elem_kernel.py",
    "rfx_channel_sum": "test_gpu_elem_kernel.py",
    "rfx_channel_sum_ws": "test_gpu_elem_kernel.py",
    "rfx_dropout": "test_gpu_elem_kernel.py",
    "rfx_fm_cm_affine_g": "test_gpu_elem_kernel.py",
    "rfx_l1_grad": "test_gpu_elem_kernel.py",
    "rfx_l1_sum": "test_gpu_elem_kernel.py",
    "rfx_l1_sum_ws": "test_gpu_elem_kernel.py",
    "rfx_mul": "test_gpu_elem_kernel.py",
    "rfx_prelu_bwd": "test_gpu_elem_kernel.py",
    "rfx_prelu_bwd_ws": "test_gpu_elem_kernel.py",
    "rfx_prelu_fwd": "test_gpu_elem_kernel.py",
    "rfx_row_affine": "test_gpu_elem_kernel.py",
    "rfx_row_affine_add": "test_gpu_elem_kernel.py",
    "rfx_row_moments": "test_gpu_elem_kernel.py",
    "rfx_row_moments_ws": "test_gpu_elem_kernel.py",
    "rfx_span_mask": "test_gpu_elem_kernel.py",
    "rfx_zero": "test_gpu_elem_kernel.py",
    # test_gpu_fft_kernel.py
    "rfx_fft_analysis": "test_gpu_fft_kernel.py",
    "rfx_fft_synthesis": "test_gpu_fft_kernel.py",
    "rfx_fft_synthesis_lossgrad": "test_gpu_fft_kernel.py",
    "rfx_fft_synthesis_ws": "test_gpu_fft_kernel.py",
    "rfx_stft_loss_grad": "test_gpu_fft_kernel.py",
    "rfx_stft_loss_grad_m": "test_gpu_fft_kernel.py",
    "rfx_stft_loss_reduce": "test_gpu_fft_kernel.py",
    "rfx_stft_loss_reduce_ws": "test_gpu_fft_kernel.py",
    "rfx_stft_pair_loss": "test_gpu_fft_kernel.py",
    "rfx_stft_pair_loss_ws": "test_gpu_fft_kernel.py",
    # test_gpu_fir.py
    "rfx_fir_same": "test_gpu_fir.py",
    "rfx_sum_diff": "test_gpu_fir.py",
    "rfx_sum_diff_adj": "test_gpu_fir.py",
    # test_gpu_fx_kernel.py
    "rfx_fx_chorus": "test_gpu_fx_kernel.py",
    "rfx_fx_compressor": "test_gpu_fx_kernel.py",
    "rfx_fx_compressor_ws": "test_gpu_fx_kernel.py",
    "rfx_fx_delay": "test_gpu_fx_kernel.py",
    "rfx_fx_distortion": "test_gpu_fx_kernel.py",
    "rfx_fx_eq": "test_gpu_fx_kernel.py",
    "rfx_fx_limiter": "test_gpu_fx_kernel.py",
    "rfx_fx_limiter_ws": "test_gpu_fx_kernel.py",
    "rfx_fx_loudness": "test_gpu_fx_kernel.py",
    "rfx_fx_loudness_joint": "test_gpu_fx_kernel.py",
    "rfx_fx_loudness_joint_ws": "test_gpu_fx_kernel.py",
    "rfx_fx_loudness_ws": "test_gpu_fx_kernel.py",
    "rfx_fx_normalize_rows": "test_gpu_fx_kernel.py",
    "rfx_fx_normalize_ws_bytes": "test_gpu_fx_kernel.py",
    "rfx_fx_phaser": "test_gpu_fx_kernel.py",
    "rfx_fx_phaser_ws_floats": "test_gpu_fx_kernel.py",
    "rfx_fx_reverb": "test_gpu_fx_kernel.py",
    "rfx_fx_scale": "test_gpu_fx_kernel.py",
    "rfx_fx_sox_reverb": "test_gpu_fx_kernel.py",
    "rfx_fx_sox_reverb_ws_floats": "test_gpu_fx_kernel.py",
    "rfx_fx_volume": "test_gpu_fx_kernel.py",
    "rfx_fx_widener": "test_gpu_fx_kernel.py",
    # test_gpu_gemm_kernel.py
    "rfx_gemm_fwd": "test_gpu_gemm_kernel.py",
    "rfx_gemm_fwd_variant": "test_gpu_gemm_kernel.py",
    "rfx_gemm_wgrad": "test_gpu_gemm_kernel.py",
    "rfx_gemm_wgrad_variant": "test_gpu_gemm_kernel.py",
    "rfx_pack_a": "test_gpu_gemm_kernel.py",
    "rfx_unpack_add": "test_gpu_gemm_kernel.py",
    "rfx_unpack_add_bias": "test_gpu_gemm_kernel.py",
    "rfx_unpack_col": "test_gpu_gemm_kernel.py",
    "rfx_unpack_set": "test_gpu_gemm_kernel.py",
    # test_gpu_hdemucs_route.py
    "rfx_cl_dconv_ok": "test_gpu_hdemucs_route.py",
    # test_gpu_loss_kernel.py
    "rfx_logcosh_grad": "test_gpu_loss_kernel.py",
    "rfx_logcosh_rows": "test_gpu_loss_kernel.py",
    "rfx_logcosh_ws": "test_gpu_loss_kernel.py",
    "rfx_mrstft_combine": "test_gpu_loss_kernel.py",
    "rfx_mrstft_combine_w": "test_gpu_loss_kernel.py",
    "rfx_sisdr_finish": "test_gpu_loss_kernel.py",
    "rfx_sisdr_sums": "test_gpu_loss_kernel.py",
    "rfx_sisdr_sums_ws": "test_gpu_loss_kernel.py",
    "rfx_stft_scaled_loss": "test_gpu_loss_kernel.py",
    "rfx_stft_scaled_loss_grad": "test_gpu_loss_kernel.py",
    "rfx_stft_scaled_loss_ws": "test_gpu_loss_kernel.py",
    "rfx_time_loss_grad": "test_gpu_loss_kernel.py",
    "rfx_time_loss_rows": "test_gpu_loss_kernel.py",
    "rfx_time_sums": "test_gpu_loss_kernel.py",
    "rfx_time_sums_ws": "test_gpu_loss_kernel.py",
    # test_gpu_lstm_kernel.py
    "rfx_lstm_bwd": "test_gpu_lstm_kernel.py",
    "rfx_lstm_cat_params": "test_gpu_lstm_kernel.py",
    "rfx_lstm_fwd": "test_gpu_lstm_kernel.py",
    "rfx_lstm_grad_scatter": "test_gpu_lstm_kernel.py",
    "rfx_lstm_local": "test_gpu_lstm_kernel.py",
    "rfx_lstm_pack": "test_gpu_lstm_kernel.py",
    "rfx_lstm_pack_bytes": "test_gpu_lstm_kernel.py",
    "rfx_lstm_pack_local": "test_gpu_lstm_kernel.py",
    "rfx_lstm_set_local": "test_gpu_lstm_kernel.py",
    # test_gpu_multisource.py
    "rfx_fm_cm_affine": "test_gpu_multisource.py",
    # test_gpu_norm_kernel.py
    "rfx_avgpool2d_bwd": "test_gpu_norm_kernel.py",
    "rfx_avgpool2d_fwd": "test_gpu_norm_kernel.py",
    "rfx_batchnorm_bwd": "test_gpu_norm_kernel.py",
    "rfx_batchnorm_fwd": "test_gpu_norm_kernel.py",
    "rfx_batchnorm_fwd_ws": "test_gpu_norm_kernel.py",
    "rfx_glu_bwd": "test_gpu_norm_kernel.py",
    "rfx_glu_bwd_bf16": "test_gpu_norm_kernel.py",
    "rfx_glu_fwd": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_bwd": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_bwd_x16": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_fwd": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_fwd_ws": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_fwd_x16": "test_gpu_norm_kernel.py",
    "rfx_groupnorm_stat_chunks": "test_gpu_norm_kernel.py",
    "rfx_norm_bwd_work_floats": "test_gpu_norm_kernel.py",
    # test_gpu_optim_kernel.py
    "rfx_sumsq": "test_gpu_optim_kernel.py",
    "rfx_sumsq_ws": "test_gpu_optim_kernel.py",
    "rfx_adamw_step": "test_gpu_optim_kernel.py",
    "rfx_clip_coef": "test_gpu_optim_kernel.py",
    # test_gpu_segment_kernel.py
    "rfx_segment_merge": "test_gpu_segment_kernel.py",
    "rfx_segment_merge_c": "test_gpu_segment_kernel.py",
    "rfx_segment_split": "test_gpu_segment_kernel.py",
    "rfx_segment_split_c": "test_gpu_segment_kernel.py",
    # test_gpu_wiener_kernel.py
    "rfx_wiener": "test_gpu_wiener_kernel.py",
    "rfx_wiener_max_window": "test_gpu_wiener_kernel.py",
    "rfx_wiener_ws_floats": "test_gpu_wiener_kernel.py",
    # test_host_cpu.py
    "rfx_abi_version": "test_host_cpu.py",
    "rfx_gemm_pick_r": "test_host_cpu.py",
    "rfx_lstm_ws_bytes": "test_host_cpu.py",
}


def _imports(text):
    """(tests/*_ref.py modules, remfx_amd modules but _lib) a module's text imports"""
    refs, wraps = set(), set()
    for m in re.finditer(r"from tests import ([^\n#]+)", text):
        refs |= {n.strip().split(" as ")[0].strip("() ") for n in m.group(1).split(",")}
    refs |= set(re.findall(r"(?:from|import) tests\.(\w+)", text))
    for m in re.finditer(r"from remfx_amd import ([^\n#]+)", text):
        wraps |= {n.strip().split(" as ")[0].strip("() ") for n in m.group(1).split(",")}
    wraps |= set(re.findall(r"(?:from|import) remfx_amd\.(\w+)", text))
    return {r for r in refs if r.endswith("_ref")}, {w for w in wraps if w and w != "_lib"}


def reach(module):
    """{file: text} of a test module, the tests/*_ref.py it imports (transitively) and the remfx_amd wrappers those import; never
    remfx_amd/_lib.py, which names every entry"""
    texts = {module: open(os.path.join(TESTS, module)).read()}
    todo, wraps = [texts[module]], set()
    while todo:
        refs, w = _imports(todo.pop())
        wraps |= w
        for r in refs:
            path = os.path.join(TESTS, r + ".py")
            if r + ".py" not in texts and os.path.exists(path):
                texts[r + ".py"] = open(path).read()
                todo.append(texts[r + ".py"])
    for w in wraps:
        path = os.path.join(os.path.dirname(TESTS), "remfx_amd", w + ".py")
        if os.path.exists(path):
            texts["remfx_amd/" + w + ".py"] = open(path).read()
    return texts


def names(entry, module):
    """the files of reach(module) whose text holds the entry's name as a word"""
    pat = re.compile(r"\b" + re.escape(entry) + r"\b")
    return sorted(f for f, t in reach(module).items() if pat.search(t))
