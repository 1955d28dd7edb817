"""Coverage guard: every __global__ kernel of csrc/ has an entry below naming the test file that reaches it and the hook (or, for a kernel that
only runs inside the engine, the entry point or test) through which it does; the test file must name that hook.  A new kernel without an entry
fails here -- give it a test of its own first."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "streamvoiceanon_amd", "csrc")

STEP, TAIL, KERN, PAR, CONV = "test_gpu_step_ops.py", "test_gpu_decode_tail.py", "test_gpu_kernels.py", "test_gpu_parity.py", "test_gpu_conv_gemm.py"
VOC = "test_gpu_voc_conv.py"
ROW_MAJOR_ARM = (VOC, "test_to_planes_act_row_major_arm")          # to_planes_act_kernel with blocked = 0, the layout voc_conv_kernel reads
IN_SITU = "in situ"         # reached only inside the engine's own step: the named test runs it and checks what it computes

# kernel -> (test file, hook or entry point named in that file[, IN_SITU])
MANIFEST = {
    # csrc/engine_kernels.hip: one launcher each, all through sva_test_step_ops
    **{k + "_kernel": (STEP, "test_step_op") for k in (
        "ar_prepare_step", "apply_forced", "ar_finish_frame", "append_content", "put_codes", "build_prompt", "build_delayfill", "build_reprefill",
        "finish_reprefill", "copy_rows", "copy_rows2", "broadcast_row", "fill_rows", "inc", "add_list", "add_vec", "set_slot_i32", "history_rows_copy",
        "history_rows_move", "put_row", "mean3", "copy_tokens")},
    "voc_level_kernel": (STEP, "test_voc_level"),
    # the persistent decode kernels: whole frames inside the engine, every output against the float64 frame of ar_frame_ref.py
    "ar_decode_kernel": ("test_gpu_ar_frame.py", "test_decode_frames_match_fp64", IN_SITU),
    "ar_batch_kernel": ("test_gpu_ar_frame.py", "test_decode_frames_match_fp64", IN_SITU),
    # csrc/kernels.hip
    "ring_write_kernel": (TAIL, "test_ring_write"),
    "fill_i32_kernel": (PAR, "host_launch_cost", IN_SITU),
    "add_i32_kernel": (TAIL, "test_shift_history"),
    "shift_history_kernel": (TAIL, "test_shift_history"),
    "stft_mag_kernel": (KERN, "test_stft_ring"),
    "dwconv7_ln_kernel": (KERN, "test_rowop"),
    "norm_rows_kernel": (KERN, "test_rowop"),
    "enc_attention_kernel": (KERN, "test_enc_attention"),
    "enc_attention_mfma_kernel": (KERN, "test_enc_attention"),
    "enc_attention_flash_kernel": (KERN, "test_enc_attention"),
    "bsq_kernel": (KERN, "test_bsq"),
    "rope_kvwrite_kernel": (KERN, "test_decode_attention"),
    "ar_attention_kernel": (KERN, "test_decode_attention"),
    "ar_attention_pair_kernel": (KERN, "test_decode_attention"),
    "ar_fast_attention_kernel": (KERN, "test_decode_attention"),
    "ar_prefill_attention_kernel": (PAR, "test_prefill_attention"),
    "sampler_kernel": (TAIL, "test_sampler_launch"),
    "sampler_reg_kernel": (TAIL, "test_sampler_launch"),
    "sampler_bisect_kernel": (TAIL, "test_sampler_launch"),
    "sampler_small_kernel": (TAIL, "test_sampler_launch"),
    "logit_edit_kernel": (TAIL, "test_logit_edits"),
    "gather_rows_kernel": (TAIL, "test_gather_rows"),
    "audio_embed_kernel": (TAIL, "test_audio_embed"),
    "gemv_kernel": (TAIL, "test_gemv"),
    "fsq_encode_kernel": (KERN, "test_fsq"),
    "fsq_decode_kernel": (KERN, "test_fsq"),
    "conv_post_tanh_kernel": (KERN, "test_conv_post"),
    # the conv-GEMM families
    "conv_gemm_kernel": (CONV, "test_conv_gemm"),
    "skinny_gemm_kernel": (CONV, "test_conv_gemm"),
    "pipe_gemm_kernel": (CONV, "test_conv_gemm"),
    "split_gemm_kernel": (CONV, "test_conv_gemm"),
    "split_ws_kernel": (CONV, "test_conv_gemm"),
    "stream_gemm_kernel": (CONV, "test_conv_gemm"),
    "planes_gemm_kernel": (CONV, "test_conv_gemm"),
    "planes_dma_kernel": (CONV, "test_conv_gemm"),
    "to_planes_kernel": (PAR, "test_gemm_planes"),
    "to_planes_act_kernel": (CONV, "test_conv_gemm"),            # (its row-major arm: ROW_MAJOR_ARM below)
    "voc_conv_kernel": (VOC, "test_voc_conv"),
    "f16w_gemm_kernel": (PAR, "test_gemm_f16w"),
    "stream_h_gemm_kernel": ("test_gpu_enc_fp16.py", "test_gemm_h16"),
    # csrc/prompt_ops.hip: the sva_op_* entry points
    "affine_kernel": (KERN, "test_op_affine"),
    "unary_kernel": (KERN, "test_op_unary"),
    "colstats_kernel": (KERN, "test_op_colstats"),
    "cam_context_kernel": (KERN, "test_op_cam_context"),
    "mul_kernel": (KERN, "test_op_mul_and_add"),
    "add_kernel": (KERN, "test_op_mul_and_add"),
    "conv_naive_kernel": (KERN, "test_op_conv"),
    "conv2d_kernel": (KERN, "test_op_conv2d"),
    "cf_to_rows_kernel": (KERN, "test_op_cf_to_rows"),
    "fbank_frames_kernel": (KERN, "test_op_fbank_power"),
    "stft_frames_kernel": (KERN, "test_op_stft_mag"),
    "dft_kernel": (KERN, "test_op_stft_mag"),
    "attention_kernel": (KERN, "test_op_attention"),
    "geglu_kernel": (KERN, "test_op_geglu"),
    "l2norm_kernel": (KERN, "test_op_l2norm"),
    # test-only kernels: wrappers that instantiate device functions of the persistent kernels, and the queue probe
    "test_nucleus_kernel": (TAIL, "test_ar_nucleus"),
    "test_ardev_gemv_kernel": (TAIL, "test_ar_gemv"),
    "waiter_kernel": ("_stream_queues_worker.py", "stream_overlap", IN_SITU),
    "setter_kernel": ("_stream_queues_worker.py", "stream_overlap", IN_SITU),
}


def kernels_in_source():
    """name -> file of every `__global__ ... void name(` in csrc/*.hip and csrc/*.h (templates and __launch_bounds__ in between allowed)"""
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        names = re.findall(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", src)
        assert len(names) == len(re.findall(r"\b__global__\b", src)), (fn, "a __global__ this test cannot name")
        for n in names:
            found[n] = fn
    return found


def test_every_kernel_has_a_test_that_names_its_hook():
    found = kernels_in_source()
    assert len(found) > 80
    missing = sorted(set(found) - set(MANIFEST))
    assert not missing, "kernels without a manifest entry (and, presumably, without a test): %s" % missing
    stale = sorted(set(MANIFEST) - set(found))
    assert not stale, "manifest entries whose kernel is gone: %s" % stale
    for k, entry in MANIFEST.items():
        path = os.path.join(ROOT, "tests", entry[0])
        assert os.path.isfile(path), (k, entry[0])
        with open(path) as f:
            assert entry[1] in f.read(), "%s: %s does not name %s" % (k, entry[0], entry[1])
        assert len(entry) == 2 or entry[2] == IN_SITU
    # to_planes_act_kernel has two arms: the conv-GEMM hook reaches only the K-blocked one, the row-major one has its own case
    for fn in (ROW_MAJOR_ARM[0], MANIFEST["to_planes_act_kernel"][0]):
        with open(os.path.join(ROOT, "tests", fn)) as f:
            assert ROW_MAJOR_ARM[1] in f.read(), "%s does not name the row-major case of to_planes_act_kernel" % fn


def test_step_ops_hook_covers_every_kernel_of_engine_kernels():
    """the 22 kernels of engine_kernels.hip are the kinds of sva_test_step_ops, one launcher each, and no other file launches them"""
    from streamvoiceanon_amd import engine as E
    found = kernels_in_source()
    mine = sorted(k[:-len("_kernel")] for k, fn in found.items() if fn == "engine_kernels.hip")
    assert mine == sorted(E.STEP_OPS) and sorted(E.STEP_OPS.values()) == list(range(len(mine)))
    with open(os.path.join(CSRC, "engine_kernels.h")) as f:
        header = f.read()
    for k in mine:
        assert re.search(r"\bint launch_%s\(" % k, header), k
    for fn in os.listdir(CSRC):
        if fn.endswith((".hip", ".h")) and fn != "engine_kernels.hip":
            with open(os.path.join(CSRC, fn)) as f:
                src = f.read()
            for k in mine:
                assert not re.search(r"(hipLaunchKernelGGL\s*\(\s*\(?\s*|__global__[^;{]*\b)%s_kernel\b|\b%s_kernel\s*<<<" % (k, k), src), (fn, k)
