"""ctypes binding of the C ABI in include/sva.h (libsva_hip.so, built by csrc/Makefile).

This is the ONLY compute path of the package: if the HIP library is missing or no MI355X is
visible the constructors raise -- there is no CPU fallback (the CPU oracle under oracle/ is
test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The engine overlaps its stages on four HIP streams (plus the process's default stream).  The runtime multiplexes streams
# onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share a queue serialise; the library gives its four
# streams a hardware queue each by construction (two stream-priority levels: csrc/engine.hip get_streams), at any pool size:
# 630 -> 1070 frames/s single-stream at the default pool of 4 (profiles/hw_queues_report.txt).  Exporting GPU_MAX_HW_QUEUES=8
# BEFORE the HIP runtime starts (bench.py asks for it where the variable is unset) is harmless and no longer
# needed; the name stays for callers that read it.  This module does not touch the process environment.
RECOMMENDED_ENV = {"GPU_MAX_HW_QUEUES": "8"}

LIB_PATH = os.environ.get("SVA_LIB_PATH") or os.path.join(_HERE, "libsva_hip.so")      # override: A/B builds of the kernels


class SvaConfig(C.Structure):
    _fields_ = [
        ("n_mels", C.c_int), ("enc_depths", C.c_int * 4), ("enc_dims", C.c_int * 4),
        ("tr_layers", C.c_int), ("tr_heads", C.c_int), ("tr_dim", C.c_int), ("tr_inter", C.c_int), ("bsq_bits", C.c_int),
        ("ar_dim", C.c_int), ("ar_heads", C.c_int), ("ar_layers", C.c_int), ("ar_fast_layers", C.c_int), ("ar_inter", C.c_int),
        ("ar_vocab", C.c_int), ("codebook_size", C.c_int), ("num_codebooks", C.c_int), ("max_delay", C.c_int),
        ("max_seq_len", C.c_int), ("timbre_dim", C.c_int), ("timbre_tokens", C.c_int), ("style_dim", C.c_int),
        ("voc_dim", C.c_int), ("ar_dtype", C.c_int), ("mm_mode", C.c_int), ("voc_dtype", C.c_int), ("enc_dtype", C.c_int),
    ]


class SvaStreamParams(C.Structure):
    _fields_ = [
        ("n_streams", C.c_int), ("encode_window_frames", C.c_int), ("decode_window_frames", C.c_int),
        ("chunk_frames", C.c_int), ("delay", C.c_int), ("max_seq_frames", C.c_int), ("buffer_frames", C.c_int),
        ("max_prompt_frames", C.c_int), ("temperature", C.c_float), ("top_p", C.c_float),
        ("voc_max_frames", C.c_int), ("use_graph", C.c_int), ("skip_semantic", C.c_int), ("pipeline", C.c_int),
        ("slot_priming", C.c_int),
    ]


_lib = None


def load_library():
    """dlopen libsva_hip.so; raises RuntimeError (never falls back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The engine has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, f32p = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    lib.sva_last_error.restype = C.c_char_p
    lib.sva_config_default.argtypes = [C.POINTER(SvaConfig)]
    lib.sva_stream_params_default.argtypes = [C.POINTER(SvaStreamParams)]
    lib.sva_engine_create.argtypes = [C.POINTER(SvaConfig), i32, C.POINTER(vp)]
    lib.sva_engine_load_weight.argtypes = [vp, C.c_char_p, i32, C.POINTER(C.c_int64), vp]
    lib.sva_engine_finalize.argtypes = [vp]
    lib.sva_engine_destroy.argtypes = [vp]
    lib.sva_engine_destroy.restype = None
    lib.sva_batch_create.argtypes = [vp, C.POINTER(SvaStreamParams), C.POINTER(vp)]
    lib.sva_batch_destroy.argtypes = [vp]
    lib.sva_batch_destroy.restype = None
    lib.sva_prefill_prompt.argtypes = [vp, i32, vp, vp, i32, vp, vp, C.c_uint64]
    lib.sva_streams_begin.argtypes = [vp]
    lib.sva_stream_restart.argtypes = [vp, i32, vp, vp, i32, vp, vp, C.c_uint64]
    lib.sva_stream_retire.argtypes = [vp, i32]
    lib.sva_stream_state.argtypes = [vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    lib.sva_stream_set_sampling.argtypes = [vp, i32, C.c_float, C.c_float]
    lib.sva_stream_get_sampling.argtypes = [vp, i32, f32p, f32p]
    lib.sva_stream_activations.argtypes = [vp, C.POINTER(C.c_long), f32p]
    lib.sva_stream_save_size.argtypes = [vp, i32]
    lib.sva_stream_save_size.restype = C.c_long
    lib.sva_stream_save.argtypes = [vp, i32, vp, C.c_long, C.POINTER(C.c_long)]
    lib.sva_stream_load.argtypes = [vp, i32, vp, C.c_long]
    lib.sva_stream_blob_info.argtypes = [vp, C.c_long, C.POINTER(C.c_long)]
    lib.sva_test_slot_pack.argtypes = [i32, vp, i32, vp, C.c_long, vp, C.c_long, i32, i32, i32, i32, vp, C.c_long, i32]
    lib.sva_test_snapshot_timings.argtypes = [vp, i32, f32p, C.POINTER(C.c_long)]
    lib.sva_test_snapshot_header.argtypes = [i32, vp, vp, vp, C.c_long, vp, C.c_long, vp]
    lib.sva_step.argtypes = [vp, vp, vp, vp, vp]
    lib.sva_step_device.argtypes = [vp, vp, vp]
    lib.sva_step_device_on.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.sva_join_stream.argtypes = [vp, vp]
    lib.sva_io_open.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.sva_io_close.argtypes = [vp]
    lib.sva_io_close.restype = None
    lib.sva_io_process.argtypes = [vp, vp, vp, i32, C.POINTER(C.c_int)]
    lib.sva_io_process_device.argtypes = [vp, vp, vp, i32, vp, i32]
    lib.sva_io_latency.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.sva_test_io_plan.argtypes = [i32, i32, vp, i32, vp, i32]
    lib.sva_test_resample.argtypes = [i32, i32, i32, i32, i32, i32, vp, C.c_long, vp, i32, vp, C.c_long, C.POINTER(C.c_long)]
    lib.sva_batch_uses_persistent_decode.argtypes = [vp]
    lib.sva_test_force_ar_timeout.argtypes = [vp]
    lib.sva_test_kv_rows.argtypes = [vp, i32, i32, i32, vp]
    lib.sva_test_fast_qkv0.argtypes = [vp, i32, i32, vp]
    lib.sva_test_stream_overlap.argtypes = [vp, C.POINTER(C.c_int)]
    lib.sva_debug_configure.argtypes = [C.c_char_p]
    lib.sva_sync.argtypes = [vp]
    lib.sva_encode_window.argtypes = [vp, vp, vp, vp]
    lib.sva_vocode_window.argtypes = [vp, vp, i32, vp]
    lib.sva_vocode_stream.argtypes = [vp, vp, i32, vp]
    lib.sva_quantizer_decode.argtypes = [vp, vp, i32, vp]
    lib.sva_vocoder_head.argtypes = [vp, vp, i32, vp]
    lib.sva_vocode_reset.argtypes = [vp]
    lib.sva_ar_delay_fill.argtypes = [vp, vp]
    lib.sva_ar_decode_one.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.sva_firefly_encode.argtypes = [vp, vp, vp]
    lib.sva_stream_chunks.argtypes = [vp, vp, vp, i32]
    lib.sva_generate.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, C.c_uint64, vp, vp]
    lib.sva_generate_many.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.sva_test_prefill_attention_runs.argtypes = [i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.sva_test_prefill_pack.argtypes = [vp, i32, i32, vp, i32]
    lib.sva_get_tap.argtypes = [vp, C.c_char_p, vp, C.c_long]
    lib.sva_get_tap.restype = C.c_long
    lib.sva_get_timings.argtypes = [vp, f32p]
    lib.sva_get_gemm_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    lib.sva_get_gemm_bytes.argtypes = [vp, C.POINTER(C.c_double)]
    lib.sva_stream_codes.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(C.c_long)]
    lib.sva_profile_gemm.argtypes = [vp, i32]
    lib.sva_get_gemm_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    lib.sva_get_gemm_profile_table.argtypes = [vp, vp, C.c_long]
    lib.sva_get_gemm_profile_table.restype = C.c_long
    lib.sva_bench_gemm.argtypes = [i32] * 9 + [f32p]
    lib.sva_bench_gemm_choice.argtypes = [i32] * 14 + [f32p]
    lib.sva_test_gemm.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp]
    lib.sva_test_gemm_plan.argtypes = [C.POINTER(C.c_int), i32, C.POINTER(C.c_int)]
    lib.sva_test_conv_gemm.argtypes = [i32, i32, vp, vp, vp, C.POINTER(C.c_int), i32, C.POINTER(C.c_int)]
    lib.sva_test_slot_book.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), i32, C.POINTER(C.c_int)]
    lib.sva_test_slot_prompt_tail.argtypes = [i32] * 6 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.sva_test_gemm_choice.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32]
    lib.sva_set_sampler_edits.argtypes = [vp, vp, i32, C.c_float, vp, i32]
    lib.sva_test_prefill_attention.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp]
    lib.sva_test_pair_attention.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp]
    i64 = C.c_long
    lib.sva_test_decode_attention.argtypes = [i32] * 6 + [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.sva_test_enc_attention.argtypes = [i32] * 5 + [vp, vp, i32, i32, vp, vp]
    lib.sva_test_rowop.argtypes = [i32] * 5 + [vp, i64, i64, i64, i32, vp, vp, vp, vp, C.c_float, vp, i64, i64, i64, i32, i32, i32, i32, i32, vp, i64]
    lib.sva_test_bsq.argtypes = [i32] * 4 + [vp, i64, i64, i64, i32, vp, C.c_float, vp, vp, vp, i32, vp, i64, i32, i32, vp]
    lib.sva_test_stft_ring.argtypes = [i32] * 3 + [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32]
    lib.sva_test_fsq.argtypes = [i32] * 6 + [vp, i64, i64, i64, i32, vp, vp, vp, i64, i64, i64]
    lib.sva_test_conv_post.argtypes = [i32] * 5 + [vp, i64, i64, i64, vp, vp, vp, i64, i64, i64, vp]
    lib.sva_test_sampler_launch.argtypes = [i32, vp, vp, vp]
    lib.sva_test_sampler_rows.argtypes = [i32, vp, vp, vp, vp, i32, vp]
    lib.sva_test_ar_device.argtypes = [i32, i32, vp, vp, vp]
    lib.sva_test_gemv.argtypes = [i32, vp, vp, vp]
    lib.sva_test_token_ops.argtypes = [i32, i32, vp, vp, vp]
    lib.sva_test_step_ops.argtypes = [i32, i32, vp, vp, vp]
    lib.sva_test_voc_level.argtypes = [i32, vp, vp, vp]
    lib.sva_test_voc_conv.argtypes = [i32, vp, vp, vp]
    lib.sva_test_gemm_f16w.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp]
    lib.sva_test_gemm_planes.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.sva_test_gemm_h16.argtypes = [i32] * 8 + [vp] * 5 + [i32] * 4 + [vp, i32, vp]
    lib.sva_host_launch_cost.argtypes = [i32, i32, f32p]
    lib.sva_test_sampler.argtypes = [i32, i32, i32, i32, vp, vp, C.c_float, C.c_float, vp, i32, f32p]
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "sva_last_error", "sva_config_default", "sva_stream_params_default", "sva_engine_create",
    "sva_engine_load_weight", "sva_engine_finalize", "sva_engine_destroy", "sva_batch_create", "sva_batch_destroy",
    "sva_prefill_prompt", "sva_streams_begin", "sva_stream_restart", "sva_stream_retire", "sva_stream_state", "sva_stream_set_sampling", "sva_stream_get_sampling", "sva_stream_activations", "sva_step", "sva_step_device", "sva_step_device_on", "sva_join_stream", "sva_batch_uses_persistent_decode", "sva_test_force_ar_timeout", "sva_test_kv_rows", "sva_test_fast_qkv0", "sva_test_stream_overlap", "sva_debug_configure", "sva_sync", "sva_stream_chunks", "sva_encode_window", "sva_firefly_encode",
    "sva_vocode_window", "sva_vocode_stream", "sva_vocode_reset", "sva_quantizer_decode", "sva_vocoder_head", "sva_ar_delay_fill", "sva_ar_decode_one", "sva_generate", "sva_generate_many", "sva_get_tap", "sva_get_timings",
    "sva_dev_alloc", "sva_dev_free", "sva_dev_upload", "sva_dev_download", "sva_op_conv", "sva_op_affine", "sva_op_unary", "sva_op_colstats",
    "sva_op_cam_context", "sva_op_mul", "sva_op_add", "sva_op_conv2d", "sva_op_cf_to_rows", "sva_op_fbank_power", "sva_op_stft_mag", "sva_op_attention",
    "sva_op_geglu", "sva_op_l2norm", "sva_ops_capture_begin", "sva_ops_capture_end", "sva_ops_graph_launch", "sva_ops_graph_free",
    "sva_get_gemm_stats", "sva_get_gemm_bytes", "sva_stream_codes", "sva_profile_gemm", "sva_get_gemm_profile", "sva_get_gemm_profile_table", "sva_test_gemm", "sva_test_gemm_choice", "sva_test_gemm_plan", "sva_test_conv_gemm", "sva_test_slot_book", "sva_test_slot_prompt_tail", "sva_test_gemm_f16w", "sva_test_gemm_planes", "sva_test_gemm_h16", "sva_test_prefill_attention", "sva_test_pair_attention", "sva_test_prefill_attention_runs", "sva_test_prefill_pack", "sva_test_decode_attention", "sva_test_enc_attention", "sva_test_rowop", "sva_test_bsq", "sva_test_stft_ring", "sva_test_fsq", "sva_test_conv_post", "sva_test_sampler_launch", "sva_test_sampler_rows", "sva_test_ar_device", "sva_test_gemv", "sva_test_token_ops", "sva_test_step_ops", "sva_test_voc_level", "sva_test_voc_conv", "sva_set_sampler_edits", "sva_bench_gemm", "sva_bench_gemm_choice", "sva_test_sampler", "sva_host_launch_cost",
    "sva_io_open", "sva_io_close", "sva_io_process", "sva_io_process_device", "sva_io_latency", "sva_test_io_plan", "sva_test_resample",
    "sva_stream_save_size", "sva_stream_save", "sva_stream_load", "sva_stream_blob_info", "sva_test_slot_pack", "sva_test_snapshot_header", "sva_test_snapshot_timings",
]


def _check(rc, what):
    if rc != 0:
        msg = load_library().sva_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# --------------------------------------------------------------------------------------------
# derived (non-persistent) buffers of the reference modules, computed exactly as the reference does
# --------------------------------------------------------------------------------------------
def slaney_mel_fb(n_freqs=1025, f_min=0.0, f_max=22050.0, n_mels=160, sample_rate=44100) -> np.ndarray:
    """LogMelSpectrogram.fb (modules/vqgan/spectrogram.py:93-101) = torchaudio.functional.
    melscale_fbanks(norm="slaney", mel_scale="slaney") of torchaudio==2.4.0, restated with torch fp32
    ops in the same order (torchaudio is not a dependency of this package).  [n_freqs, n_mels]."""
    import torch

    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0

    def hz2mel(f):
        return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(hz2mel(f_min), hz2mel(f_max), n_mels + 2)
    f_pts = f_sp * m_pts
    is_log = m_pts >= min_log_mel
    f_pts[is_log] = min_log_hz * torch.exp(logstep * (m_pts[is_log] - min_log_mel))
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.min(down, up), min=0.0)
    fb = fb * (2.0 / (f_pts[2: n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb.numpy().astype(np.float32)


def rope_table(seq_len: int, n_elem: int = 64, base: float = 10000.0) -> np.ndarray:
    """precompute_freqs_cis (modules/dual_ar_stream.py:993-1001): cos/sin rounded to bf16, returned as
    float32 [seq_len, n_elem/2, 2].  Computed with torch so the bf16 rounding matches the reference bit
    for bit on the same host."""
    import torch

    freqs = 1.0 / (base ** (torch.arange(0, n_elem, 2)[: n_elem // 2].float() / n_elem))
    ang = torch.outer(torch.arange(seq_len).float(), freqs)
    tab = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
    return tab.to(torch.bfloat16).float().numpy()


def derived_buffers(cfg: SvaConfig | None = None) -> dict:
    import torch

    out = {
        "tok.spec_transform.fb": slaney_mel_fb(),
        "tok.spec_transform.spectrogram.window": torch.hann_window(2048).numpy(),
        "tok.quantizer.pre_module.freqs_cis": rope_table(2048),
        "arvc.decoder.model.freqs_cis": rope_table(2048 if cfg is None else cfg.max_seq_len),
        "arvc.decoder.model.fast_freqs_cis": rope_table(8 if cfg is None else cfg.num_codebooks),
    }
    return out


class Engine:
    """Weights on one MI355X.  `weights`: dict name -> array-like (numpy / torch CPU tensor) keyed by the
    reference state-dict names prefixed with 'arvc.' / 'tok.' / 'voc.'."""

    def __init__(self, weights: dict, device: int = 0, ar_dtype: int = 0, mm_mode: int = None, voc_dtype: int = None, enc_dtype: int = None):
        """mm_mode / voc_dtype: sva_config fields of the same names (None = the library's default): precision format of the batch-scale
        encoder / vocoder GEMMs (csrc/gemm_planes.hip) and the reference-precision (fp16 operand) vocoder.  enc_dtype = 1: the tokenizer's
        content encoder on fp16 operands with fp32 accumulation (include/sva.h; content codes are no longer bit-equal to the fp32 oracle)."""
        self.lib = load_library()
        self.cfg = SvaConfig()
        _check(self.lib.sva_config_default(C.byref(self.cfg)), "sva_config_default")
        self.cfg.ar_dtype = ar_dtype
        if mm_mode is not None:
            self.cfg.mm_mode = mm_mode
        if voc_dtype is not None:
            self.cfg.voc_dtype = voc_dtype
        if enc_dtype is not None:
            self.cfg.enc_dtype = enc_dtype
        self.h = C.c_void_p()
        _check(self.lib.sva_engine_create(C.byref(self.cfg), device, C.byref(self.h)), "sva_engine_create")
        self.device = device
        allw = dict(derived_buffers(self.cfg))
        allw.update(weights)
        for name, arr in allw.items():
            a = np.ascontiguousarray(arr.detach().cpu().numpy() if hasattr(arr, "detach") else arr, dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            _check(self.lib.sva_engine_load_weight(self.h, name.encode(), max(a.ndim, 1), shape, _ptr(a)),
                   f"sva_engine_load_weight({name})")
        _check(self.lib.sva_engine_finalize(self.h), "sva_engine_finalize")
        self._batches = weakref.WeakSet()
        self.ops_lock = threading.RLock()      # serialises users of the engine's ops stream (prompt_encoders.py: recording / capture / replay)

    def fast_qkv0_rows(self, row0, n=1):
        """sva_test_fast_qkv0: rows row0 .. row0 + n - 1 of the table of fast layer 0 (RMSNorm + wqkv of fast_embeddings rows, before RoPE)
        -> float32 [n, 3 * ar_dim].  Read-only."""
        out = np.empty((int(n), 3 * self.cfg.ar_dim), dtype=np.float32)
        _check(self.lib.sva_test_fast_qkv0(self.h, int(row0), int(n), _ptr(out)), "sva_test_fast_qkv0")
        return out

    def close(self):
        if self.h:
            for b in list(getattr(self, "_batches", ())):      # a batch must not outlive its engine (its destroy touches the engine)
                b.close()
            self.lib.sva_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """B lock-step streams on one engine (InferenceWrapper.setup_stream_caches for B streams)."""

    def __init__(self, engine: Engine, n_streams=1, encode_window_frames=128, decode_window_frames=64, chunk_frames=1,
                 delay=2, max_seq_frames=768, buffer_frames=32, max_prompt_frames=256, temperature=0.7, top_p=0.7,
                 voc_max_frames=None, use_graph=False, skip_semantic=False, pipeline=False, slot_priming=False):
        self.engine = engine
        self.lib = engine.lib
        p = SvaStreamParams()
        _check(self.lib.sva_stream_params_default(C.byref(p)), "sva_stream_params_default")
        p.n_streams, p.encode_window_frames, p.decode_window_frames = n_streams, encode_window_frames, decode_window_frames
        p.chunk_frames, p.delay, p.max_seq_frames, p.buffer_frames = chunk_frames, delay, max_seq_frames, buffer_frames
        p.max_prompt_frames, p.temperature, p.top_p = max_prompt_frames, temperature, top_p
        p.voc_max_frames = voc_max_frames or chunk_frames
        p.use_graph, p.skip_semantic = int(use_graph), int(skip_semantic)
        p.pipeline = int(pipeline)
        p.slot_priming = int(slot_priming)
        self.p = p
        self.B, self.chunk = n_streams, chunk_frames
        self.io = None                             # the I/O adaptor, once open_io() has opened one
        self.h = C.c_void_p()
        _check(self.lib.sva_batch_create(engine.h, C.byref(p), C.byref(self.h)), "sva_batch_create")
        engine._batches.add(self)
        cfg = engine.cfg
        self.noise_stride = cfg.ar_vocab + cfg.num_codebooks * cfg.codebook_size

    def close(self):
        if self.h:
            if self.io is not None:
                self.io.h = None                   # (sva_batch_destroy closes a forgotten adaptor)
                self.io = None
            self.lib.sva_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def open_io(self, io_rate, fmt="f32", max_block=4096):
        """sva_io_open: feed and read this (begun) batch at `io_rate` in blocks of any length up to max_block, as float32 ("f32") or int16
        ("i16") -> BatchIO.  While it is open the batch is stepped through it alone; BatchIO.close() gives step() back."""
        assert self.io is None, "one adaptor per batch"
        self.io = BatchIO(self, io_rate, fmt, max_block)
        return self.io

    def prefill_prompt(self, slot, ref_content_codes, ref_audio_codes, style, timbre, noise_seed=0):
        cc = np.ascontiguousarray(ref_content_codes, dtype=np.int64).reshape(-1)
        ac = np.ascontiguousarray(ref_audio_codes, dtype=np.int32).reshape(8, -1)
        assert ac.shape[1] == cc.shape[0]
        st = np.ascontiguousarray(style, dtype=np.float32).reshape(-1)
        tm = np.ascontiguousarray(timbre, dtype=np.float32)
        _check(self.lib.sva_prefill_prompt(self.h, slot, _ptr(cc), _ptr(ac), cc.shape[0], _ptr(st), _ptr(tm), int(noise_seed)),
               "sva_prefill_prompt")

    def begin(self):
        _check(self.lib.sva_streams_begin(self.h), "sva_streams_begin")

    def restart(self, slot, ref_content_codes, ref_audio_codes, style, timbre, noise_seed=0, temperature=None, top_p=None):
        """sva_stream_restart: a new utterance in `slot` of a begun batch (operands as prefill_prompt).  From the next step on the slot
        behaves like a slot of a fresh batch -- `delay` chunks of zeros, then frame 0 -- and every other slot is unaffected.  The slot's
        sampling pair goes back to the batch's; temperature / top_p set it for the new utterance right after the restart."""
        cc = np.ascontiguousarray(ref_content_codes, dtype=np.int64).reshape(-1)
        ac = np.ascontiguousarray(ref_audio_codes, dtype=np.int32).reshape(8, -1)
        assert ac.shape[1] == cc.shape[0]
        st = np.ascontiguousarray(style, dtype=np.float32).reshape(-1)
        tm = np.ascontiguousarray(timbre, dtype=np.float32)
        _check(self.lib.sva_stream_restart(self.h, int(slot), _ptr(cc), _ptr(ac), cc.shape[0], _ptr(st), _ptr(tm), int(noise_seed)),
               "sva_stream_restart")
        if temperature is not None or top_p is not None:
            self.set_sampling(slot, temperature, top_p)

    def set_sampling(self, slot, temperature=None, top_p=None):
        """sva_stream_set_sampling: the slot's sampler settings from its next decoded frame on (None = the batch's value).  The slot keeps
        them until they are set again or the slot is restarted; the other slots are unaffected."""
        t = self.p.temperature if temperature is None else temperature
        tp = self.p.top_p if top_p is None else top_p
        _check(self.lib.sva_stream_set_sampling(self.h, int(slot), float(t), float(tp)), "sva_stream_set_sampling")

    def sampling(self, slot):
        """sva_stream_get_sampling -> (temperature, top_p) of the slot"""
        t, tp = C.c_float(), C.c_float()
        _check(self.lib.sva_stream_get_sampling(self.h, int(slot), C.byref(t), C.byref(tp)), "sva_stream_get_sampling")
        return float(t.value), float(tp.value)

    def retire(self, slot):
        """sva_stream_retire: the slot's input is no longer read and its output is zeros until restart()."""
        _check(self.lib.sva_stream_retire(self.h, int(slot)), "sva_stream_retire")

    def stream_state(self, slot):
        """-> (phase, frames): phase 0 retired, 1 delay filling, 2 decoding; frames decoded since the slot's stream began."""
        ph, fr = C.c_int(), C.c_long()
        _check(self.lib.sva_stream_state(self.h, int(slot), C.byref(ph), C.byref(fr)), "sva_stream_state")
        return int(ph.value), int(fr.value)

    def activations(self):
        """sva_stream_activations -> (n_local, n_whole, last_ms): restarted slots activated through the one-stream priming workspace
        (slot_priming=True) / through a whole-batch priming run, and the host wall time of the last activation."""
        counts, ms = (C.c_long * 2)(), C.c_float()
        _check(self.lib.sva_stream_activations(self.h, counts, C.byref(ms)), "sva_stream_activations")
        return int(counts[0]), int(counts[1]), float(ms.value)

    def save_size(self, slot):
        """sva_stream_save_size: bytes save_stream(slot) would return now"""
        n = self.lib.sva_stream_save_size(self.h, int(slot))
        if n < 0:
            _check(int(n), "sva_stream_save_size")
        return int(n)

    def save_stream(self, slot) -> bytes:
        """sva_stream_save: the decoding stream in `slot` as a snapshot (include/sva.h, "save and resume single streams").  Read-only."""
        n = self.save_size(slot)
        buf = np.empty(n, dtype=np.uint8)
        wr = C.c_long()
        _check(self.lib.sva_stream_save(self.h, int(slot), _ptr(buf), n, C.byref(wr)), "sva_stream_save")
        return buf[:int(wr.value)].tobytes()

    def load_stream(self, slot, blob):
        """sva_stream_load: `slot` continues the stream of the snapshot from the next step on, bit-identically in a batch of the same
        configuration; every other slot is unaffected.  A refusal (RuntimeError) changes nothing."""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        _check(self.lib.sva_stream_load(self.h, int(slot), _ptr(buf) if buf.size else (C.c_char * 1)(), buf.size), "sva_stream_load")

    def move_stream(self, slot, dst_batch, dst_slot):
        """save_stream(slot), dst_batch.load_stream(dst_slot), then retire the source slot (only once the load has succeeded)"""
        dst_batch.load_stream(dst_slot, self.save_stream(slot))
        self.retire(slot)

    def snapshot_timings(self, measure_d2d=False):
        """sva_test_snapshot_timings -> dict(kernel_ms, copy_ms, host_ms, d2d_ms (None unless measured), bytes, pipelined_steps) of the last save / load"""
        ms, cnt = (C.c_float * 4)(), (C.c_long * 2)()
        _check(self.lib.sva_test_snapshot_timings(self.h, int(bool(measure_d2d)), ms, cnt), "sva_test_snapshot_timings")
        return dict(kernel_ms=float(ms[0]), copy_ms=float(ms[1]), host_ms=float(ms[2]), d2d_ms=float(ms[3]) if measure_d2d else None,
                    bytes=int(cnt[0]), pipelined_steps=int(cnt[1]))

    def step(self, pcm_in, noise=None, forced_codes=None):
        x = np.ascontiguousarray(pcm_in, dtype=np.float32).reshape(self.B, 2048 * self.chunk)
        out = np.empty_like(x)
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).reshape(self.B, self.chunk, self.noise_stride)
        fc = None if forced_codes is None else np.ascontiguousarray(forced_codes, dtype=np.int32).reshape(self.B, 8, self.chunk)
        _check(self.lib.sva_step(self.h, _ptr(x), _ptr(out), _ptr(nz), _ptr(fc)), "sva_step")
        return out

    def encode_window(self, audio, return_u=False):
        a = np.ascontiguousarray(audio, dtype=np.float32).reshape(self.B, -1)
        W = self.p.encode_window_frames
        assert a.shape[1] == W * 2048
        codes = np.empty((self.B, W), dtype=np.int64)
        u = np.empty((self.B, W, self.engine.cfg.bsq_bits), dtype=np.float32) if return_u else None
        _check(self.lib.sva_encode_window(self.h, _ptr(a), _ptr(codes), _ptr(u)), "sva_encode_window")
        return (codes, u) if return_u else codes

    def firefly_encode(self, audio):
        """wav2target_fn (evaluations/infer_arvc.py:168-171): audio [B, W*2048] -> acoustic codes int32 [B, 8, W]."""
        a = np.ascontiguousarray(audio, dtype=np.float32).reshape(self.B, -1)
        W = self.p.encode_window_frames
        assert a.shape[1] == W * 2048
        codes = np.empty((self.B, 8, W), dtype=np.int32)
        _check(self.lib.sva_firefly_encode(self.h, _ptr(a), _ptr(codes)), "sva_firefly_encode")
        return codes

    def vocode_window(self, codes):
        c = np.ascontiguousarray(codes, dtype=np.int32).reshape(self.B, 8, -1)
        T = c.shape[2]
        out = np.empty((self.B, 2048 * T), dtype=np.float32)
        _check(self.lib.sva_vocode_window(self.h, _ptr(c), T, _ptr(out)), "sva_vocode_window")
        return out

    def quantizer_decode(self, codes):
        """firefly.quantizer.decode: codes [B, 8, T] -> z float32 [B, 512, 4T] (the reference's channel-first layout)."""
        c = np.ascontiguousarray(codes, dtype=np.int32).reshape(self.B, 8, -1)
        T = c.shape[2]
        z = np.empty((self.B, 4 * T, self.engine.cfg.voc_dim), dtype=np.float32)
        _check(self.lib.sva_quantizer_decode(self.h, _ptr(c), T, _ptr(z)), "sva_quantizer_decode")
        return np.ascontiguousarray(z.transpose(0, 2, 1))

    def vocoder_head(self, z):
        """firefly.head: z [B, 512, 4T] -> pcm float32 [B, 1, 2048 T]."""
        zz = np.ascontiguousarray(np.asarray(z, dtype=np.float32).reshape(self.B, self.engine.cfg.voc_dim, -1).transpose(0, 2, 1))
        T = zz.shape[1] // 4
        out = np.empty((self.B, 2048 * T), dtype=np.float32)
        _check(self.lib.sva_vocoder_head(self.h, _ptr(zz), T, _ptr(out)), "sva_vocoder_head")
        return out[:, None, :]

    def vocode_stream(self, codes):
        c = np.ascontiguousarray(codes, dtype=np.int32).reshape(self.B, 8, -1)
        T = c.shape[2]
        out = np.empty((self.B, 2048 * T), dtype=np.float32)
        _check(self.lib.sva_vocode_stream(self.h, _ptr(c), T, _ptr(out)), "sva_vocode_stream")
        return out

    def ar_delay_fill(self, codes):
        c = np.ascontiguousarray(codes, dtype=np.int64).reshape(self.B, self.p.delay)
        _check(self.lib.sva_ar_delay_fill(self.h, _ptr(c)), "sva_ar_delay_fill")

    def set_sampler_edits(self, previous_tokens=None, repetition_penalty=1.5, suppress_tokens=None):
        """decode_one_token_ar's previous_tokens [1 + num_codebooks, W] / repetition_penalty / suppress_tokens
        (modules/dual_ar_stream.py:1099-1117, 1175-1213); no arguments = no edits."""
        pt = None if previous_tokens is None else np.ascontiguousarray(_as_np(previous_tokens), dtype=np.int32)
        if pt is not None:
            assert pt.ndim == 2 and pt.shape[0] == 1 + self.engine.cfg.num_codebooks, "previous_tokens must be [1 + num_codebooks, W]"
        sp = None if suppress_tokens is None else np.ascontiguousarray(np.asarray(list(suppress_tokens)), dtype=np.int32).reshape(-1)
        W = 0 if pt is None else int(pt.shape[1])
        ns = 0 if sp is None else int(sp.size)
        _check(self.lib.sva_set_sampler_edits(self.h, _ptr(pt) if W else None, W, float(repetition_penalty), _ptr(sp) if ns else None, ns),
               "sva_set_sampler_edits")

    def ar_decode_one(self, code, noise=None, forced=None):
        c = np.ascontiguousarray(code, dtype=np.int64).reshape(self.B)
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).reshape(self.B, self.noise_stride)
        fc = None if forced is None else np.ascontiguousarray(forced, dtype=np.int32).reshape(self.B, 8)
        out = np.empty((self.B, 8), dtype=np.int32)
        pos = np.empty((self.B,), dtype=np.int32)
        _check(self.lib.sva_ar_decode_one(self.h, _ptr(c), _ptr(nz), _ptr(fc), _ptr(out), _ptr(pos)), "sva_ar_decode_one")
        return out, pos

    def generate(self, ref_content_codes, ref_audio_codes, src_content_codes, style, timbre, noise_seed=0, noise=None):
        """offline ARVCWrapper.generate -> codes int32 [8, S]"""
        cc = np.ascontiguousarray(ref_content_codes, dtype=np.int64).reshape(-1)
        ac = np.ascontiguousarray(ref_audio_codes, dtype=np.int32).reshape(8, -1)
        src = np.ascontiguousarray(src_content_codes, dtype=np.int64).reshape(-1)
        st = np.ascontiguousarray(style, dtype=np.float32).reshape(-1)
        tm = np.ascontiguousarray(timbre, dtype=np.float32)
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).reshape(src.shape[0], self.noise_stride)
        out = np.empty((8, src.shape[0]), dtype=np.int32)
        _check(self.lib.sva_generate(self.h, _ptr(cc), _ptr(ac), cc.shape[0], _ptr(src), src.shape[0], _ptr(st), _ptr(tm), int(noise_seed),
                                     _ptr(nz), _ptr(out)), "sva_generate")
        return out

    def generate_many(self, prompts, sources, noise_seeds=None, noise=None):
        """offline ARVCWrapper.generate for every slot of the batch at once (sva_generate_many): utterance i in slot i, len(prompts) ==
        len(sources) == n_streams.  prompts: (ref_content_codes, ref_audio_codes, style, timbre) per utterance; sources: content codes [S_i];
        noise: [S_max, n, vocab + 8 * codebook_size] frame-major or None (device RNG keyed by noise_seeds[i]) -> list of int32 [8, S_i]"""
        n = len(sources)
        assert len(prompts) == n, "one prompt per source"
        ccs = [np.ascontiguousarray(p[0], dtype=np.int64).reshape(-1) for p in prompts]
        acs = [np.ascontiguousarray(p[1], dtype=np.int32).reshape(8, -1) for p in prompts]
        for cc, ac in zip(ccs, acs):
            assert ac.shape[1] == cc.shape[0], "ref_audio_codes must be [8, R] for ref_content_codes [R]"
        srcs = [np.ascontiguousarray(s, dtype=np.int64).reshape(-1) for s in sources]
        st = np.ascontiguousarray(np.stack([np.asarray(_as_np(p[2]), dtype=np.float32).reshape(-1) for p in prompts]) if n else np.zeros((0, 192), np.float32))
        tm = np.ascontiguousarray(np.stack([np.asarray(_as_np(p[3]), dtype=np.float32).reshape(32, 128) for p in prompts]) if n else np.zeros((0, 32, 128), np.float32))
        R = np.array([c.shape[0] for c in ccs], dtype=np.int32)
        S = np.array([s.shape[0] for s in srcs], dtype=np.int32)
        seeds = np.ascontiguousarray(np.zeros(n) if noise_seeds is None else noise_seeds, dtype=np.uint64).reshape(n)
        s_max = int(S.max()) if n else 0
        nz = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32).reshape(s_max, n, self.noise_stride)
        outs = [np.empty((8, int(s)), dtype=np.int32) for s in S]
        ptrs = lambda arrs: (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        _check(self.lib.sva_generate_many(self.h, n, ptrs(ccs), ptrs(acs), _ptr(R), ptrs(srcs), _ptr(S), _ptr(st), _ptr(tm), _ptr(seeds), _ptr(nz), ptrs(outs)),
               "sva_generate_many")
        return outs

    def vocode_reset(self):
        _check(self.lib.sva_vocode_reset(self.h), "sva_vocode_reset")

    def tap(self, what, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        n = self.lib.sva_get_tap(self.h, what.encode(), _ptr(out), out.nbytes)
        if n < 0:
            raise RuntimeError(f"sva_get_tap({what}): " + self.lib.sva_last_error().decode())
        assert n == out.nbytes, (what, n, out.nbytes)
        return out

    def kv_rows(self, slot, pos0, n):
        """sva_test_kv_rows: rows pos0 .. pos0 + n - 1 of the slot's slow KV cache -> float32 [layers, 2 (k, v), heads, n, 64] (an fp16 cache
        widened exactly).  Read-only; drains the batch first."""
        cfg = self.engine.cfg
        out = np.empty((cfg.ar_layers, 2, cfg.ar_heads, int(n), 64), dtype=np.float32)
        _check(self.lib.sva_test_kv_rows(self.h, int(slot), int(pos0), int(n), _ptr(out)), "sva_test_kv_rows")
        return out

    def timings(self):
        ms = (C.c_float * 4)()
        _check(self.lib.sva_get_timings(self.h, ms), "sva_get_timings")
        return dict(encoder=ms[0], ar=ms[1], vocoder=ms[2], total=ms[3])

    def profile_gemm(self, enable=True):
        _check(self.lib.sva_profile_gemm(self.h, int(enable)), "sva_profile_gemm")

    def gemm_profile(self):
        t, n = C.c_double(), C.c_long()
        _check(self.lib.sva_get_gemm_profile(self.h, C.byref(t), C.byref(n)), "sva_get_gemm_profile")
        return t.value, n.value

    def gemm_profile_table(self, max_rows=4096):
        out = np.zeros((max_rows, 6), dtype=np.float64)
        n = self.lib.sva_get_gemm_profile_table(self.h, _ptr(out), max_rows)
        return out[:max(n, 0)]

    def step_device(self, d_in_ptr, d_out_ptr):
        """sva_step_device: asynchronous chunk-step on device buffers.  The engine runs on streams of its own: the producer of d_in (a
        torch op on torch's stream, say) must have completed before the call, and d_out is valid after sync()."""
        _check(self.lib.sva_step_device(self.h, C.c_void_p(d_in_ptr), C.c_void_p(d_out_ptr)), "sva_step_device")

    def step_device_on(self, d_in_ptr, d_out_ptr, stream=None, join_output=True):
        """sva_step_device_on: the stream-ordered chunk-step.  `stream` = a hipStream_t handle as int (default: torch's current
        stream); no host synchronisation anywhere: the engine waits on the device for the stream's earlier work, and (join_output) the
        stream waits for the step's output."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        _check(self.lib.sva_step_device_on(self.h, C.c_void_p(d_in_ptr), C.c_void_p(d_out_ptr), C.c_void_p(stream), int(bool(join_output))),
               "sva_step_device_on")

    def decode_path(self):
        """0 = multi-launch decode, 1 = persistent kernel (ar_decode.hip, small batches), 2 = batched persistent kernel (ar_batch.hip)."""
        return int(self.lib.sva_batch_uses_persistent_decode(self.h))

    def uses_persistent_decode(self):
        return self.decode_path() != 0

    STREAM_PAIRS = ("main|aux0", "main|sa", "main|sv", "aux0|sa", "aux0|sv", "sa|sv")

    def stream_overlap(self):
        """{pair: bool} for the six pairs of the pipelined batch's chain streams: True = the two run concurrently (a hardware queue each)."""
        ok = (C.c_int * 6)()
        _check(self.lib.sva_test_stream_overlap(self.h, ok), "sva_test_stream_overlap")
        return {n: bool(v) for n, v in zip(self.STREAM_PAIRS, ok)}

    def join_stream(self, stream=None):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        _check(self.lib.sva_join_stream(self.h, C.c_void_p(stream)), "sva_join_stream")

    def stream_chunks(self, pcm_in):
        """n consecutive chunk-steps over a host array [B, n_chunks * 2048 * chunk] in one call (device RNG; stages pipelined
        when the batch was created with pipeline=True) -> converted audio of the same shape."""
        x = np.ascontiguousarray(pcm_in, dtype=np.float32).reshape(self.B, -1)
        n = 2048 * self.chunk
        assert x.shape[1] % n == 0 and x.shape[1] >= n
        out = np.empty_like(x)
        _check(self.lib.sva_stream_chunks(self.h, _ptr(x), _ptr(out), x.shape[1] // n), "sva_stream_chunks")
        return out

    def sync(self):
        _check(self.lib.sva_sync(self.h), "sva_sync")

    def frames_decoded(self, slot=0):
        n = C.c_long()
        _check(self.lib.sva_stream_codes(self.h, slot, 0, None, C.byref(n)), "sva_stream_codes")
        return int(n.value)

    def pred_codes(self, slot=0, n=None):
        """`pred_codes[..., -n:]` of the slot's stream state (evaluations/infer_arvc.py:520-523): int32 [8, n]; n=None -> every
        frame decoded since begin() (at most the 4096-frame device ring)."""
        if n is None:
            n = min(self.frames_decoded(slot), 4096)
        out = np.empty((8, n), np.int32)
        _check(self.lib.sva_stream_codes(self.h, slot, n, _ptr(out) if n else None, None), "sva_stream_codes")
        return out

    def gemm_bytes(self):
        v = C.c_double()
        _check(self.lib.sva_get_gemm_bytes(self.h, C.byref(v)), "sva_get_gemm_bytes")
        return v.value

    def gemm_stats(self):
        f, n = C.c_double(), C.c_long()
        _check(self.lib.sva_get_gemm_stats(self.h, C.byref(f), C.byref(n)), "sva_get_gemm_stats")
        return f.value, n.value


IO_FORMATS = {"f32": (0, np.float32), "i16": (1, np.int16)}


def io_rate_supported(io_rate) -> bool:
    """the rule sva_io_open states: an integer in 8000 .. 96000 whose ratio to 44100, reduced by their gcd, has both terms <= 640"""
    r = int(io_rate)
    if r != io_rate or not 8000 <= r <= 96000:
        return False
    g = math.gcd(r, 44100)
    return r // g <= 640 and 44100 // g <= 640


class BatchIO:
    """The I/O adaptor of a batch (include/sva.h: sva_io_*): every call pushes n samples per slot at io_rate and pops n samples at io_rate, the
    output delayed by `latency` samples; resampling, format conversion and re-blocking run on the device."""

    def __init__(self, batch: Batch, io_rate, fmt="f32", max_block=4096):
        self.batch, self.lib = batch, batch.lib
        self.io_rate, self.max_block = int(io_rate), int(max_block)
        self.fmt, self.dtype = IO_FORMATS[fmt]
        self.h = C.c_void_p()
        _check(self.lib.sva_io_open(batch.h, self.io_rate, self.fmt, self.max_block, C.byref(self.h)), "sva_io_open")
        total, filt = C.c_int(), C.c_int()
        _check(self.lib.sva_io_latency(self.h, C.byref(total), C.byref(filt)), "sva_io_latency")
        self.latency, self.filter_latency = int(total.value), int(filt.value)
        self.steps_run = 0                         # engine steps of the last process() call

    def process(self, x):
        """[B, n] (or [n] for one stream) at io_rate -> the same shape and dtype; runs the engine steps that became due (0, 1 or several)"""
        a = np.ascontiguousarray(x, dtype=self.dtype)
        b = a.reshape(self.batch.B, -1)
        out = np.empty_like(b)
        steps = C.c_int()
        _check(self.lib.sva_io_process(self.h, _ptr(b), _ptr(out), b.shape[1], C.byref(steps)), "sva_io_process")
        self.steps_run = int(steps.value)
        return out.reshape(a.shape)

    def process_device(self, d_in_ptr, d_out_ptr, n, stream=None, join_output=True):
        """sva_io_process_device on device buffers [B, n]: asynchronous, stream-ordered like Batch.step_device_on"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        _check(self.lib.sva_io_process_device(self.h, C.c_void_p(d_in_ptr), C.c_void_p(d_out_ptr), int(n), C.c_void_p(stream), int(bool(join_output))),
               "sva_io_process_device")

    def close(self):
        if self.h:
            self.lib.sva_io_close(self.h)
            self.h = None
            self.batch.io = None

    def __del__(self):
        try:
            if self.batch.h:
                self.close()
        except Exception:
            pass


IO_PLAN_HEAD = ("L", "L_filter", "nbuf", "hist_in", "hist_out", "fifo_cap", "period", "orig", "new", "width_in", "width_out", "max_block")


def test_io_plan(io_rate, chunk_frames, blocks):
    """the adaptor's planner for a stream fed `blocks` (include/sva.h: sva_test_io_plan), no GPU needed -> (header dict, int32 [n_blocks, 5] rows
    of {model-rate samples made ready, steps, io-rate samples produced, staged model-rate samples, output FIFO fill})"""
    bl = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1)
    out = np.zeros(12 + 5 * bl.size, np.int32)
    n = load_library().sva_test_io_plan(int(io_rate), int(chunk_frames), _ptr(bl), bl.size, _ptr(out), out.size)
    if n < 0:
        _check(n, "sva_test_io_plan")
    return dict(zip(IO_PLAN_HEAD, (int(v) for v in out[:12]))), out[12:].reshape(-1, 5)


def test_resample(x, from_rate, to_rate, splits=(), fmt_in="f32", fmt_out="f32", device=0):
    """either kernel of the adaptor over a host array [B, n] cut into calls at `splits` (include/sva.h: sva_test_resample) -> [B, n_ready]"""
    fi, di = IO_FORMATS[fmt_in]
    fo, do = IO_FORMATS[fmt_out]
    a = np.ascontiguousarray(x, dtype=di)
    assert a.ndim == 2
    B, n = a.shape
    cap = int(math.ceil(n * to_rate / from_rate)) + 8
    y = np.zeros((B, cap), do)
    sp = np.ascontiguousarray(splits, dtype=np.int32).reshape(-1)
    n_out = C.c_long()
    _check(load_library().sva_test_resample(device, int(from_rate), int(to_rate), fi, fo, B, _ptr(a), n, _ptr(sp) if sp.size else None, sp.size, _ptr(y), cap,
                                            C.byref(n_out)), "sva_test_resample")
    return y[:, :n_out.value].copy()


def test_gemm(A, W, bias=None, device=0):
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), dtype=np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    _check(lib.sva_test_gemm(device, M, N, K, _ptr(A), _ptr(W), _ptr(b), _ptr(out)), "sva_test_gemm")
    return out


def _as_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def test_gemm_f16w(A, W, bias=None, rms_w=None, res=None, swiglu=False, iters=0, device=0):
    """The fp16-weight GEMM of the batched fp16 AR decode (csrc/gemm_f16w.hip): epi(norm(A) @ fp16(W).T).  Returns (C, us_per_launch)."""
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N // 2 if swiglu else N), dtype=np.float32)
    cv = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
    b, nw, r = cv(bias), cv(rms_w), cv(res)
    us = np.zeros(1, dtype=np.float32)
    mode = (1 if nw is not None else 0) | (2 if r is not None else 0) | (4 if swiglu else 0)
    _check(lib.sva_test_gemm_f16w(device, M, N, K, _ptr(A), _ptr(W), _ptr(b), _ptr(nw), _ptr(r), mode, _ptr(out), int(iters), _ptr(us)), "sva_test_gemm_f16w")
    return out, float(us[0])


def test_gemm_planes(A, W, bias=None, mode=1, variant=0, a_planes=False, c_planes=False, gelu=False, silu=False, iters=0, device=0, range_check=False,
                     swiglu=False, gamma_res=False, skip_rows=False):
    """The planes GEMM (csrc/gemm_planes.hip): epi(A @ W.T) with both operands as pre-split 16-bit planes.  Returns (C, us_per_launch).
    swiglu: W rows interleave w1 | w3 in groups of 16, C is [M, N / 2]; gamma_res: C = gamma * (.) + residual with gamma[i] = 0.5 + 0.001 ((37 i) % 101),
    residual.flat[i] = 0.01 ((13 i) % 257) - 1; skip_rows (M = 170 b): rows 56..61 of every 170-row item are left at the marker -77."""
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N // 2 if swiglu else N), dtype=np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    us = np.zeros(1, dtype=np.float32)
    flags = ((1 if a_planes else 0) | (2 if c_planes else 0) | (4 if gelu else 0) | (8 if silu else 0) | (16 if range_check else 0) | (32 if swiglu else 0) |
             (64 if gamma_res else 0) | (128 if skip_rows else 0))
    _check(lib.sva_test_gemm_planes(device, M, N, K, _ptr(A), _ptr(W), _ptr(b), _ptr(out), int(mode), int(variant), flags, int(iters), _ptr(us)),
           "sva_test_gemm_planes")
    return out, float(us[0])


def test_gemm_h16(A, W, B, T, taps=1, dil=1, stride=1, bias=None, gamma=None, res=None, gelu=False, swiglu=False, skip_rows=False, padded=False,
                  range_check=False, config=(0, 0, 0), out=None, iters=0, device=0):
    """The fp16-operand weight-streaming conv-GEMM (csrc/gemm_stream_h.hip) through its production launcher.  A [B, (T - 1) stride +
    (taps - 1) dil + 1, Cin], W [N, taps * Cin] fp32 (rounded to fp16 by the kernel / the packing); config = (mt, nt, kw), (0, 0, 0) = the
    heuristic's; `out` [B, T, N or N / 2] is uploaded first (skip_rows: rows [T / 4, T / 2) of every item keep it).  -> (C, us per launch)."""
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    Cin = A.shape[-1]
    N = W.shape[0]
    assert A.shape == (B, (T - 1) * stride + (taps - 1) * dil + 1, Cin) and W.shape == (N, taps * Cin)
    Nout = N // 2 if swiglu else N
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32).reshape(N)
    gm = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float32).reshape(N)
    r = None if res is None else np.ascontiguousarray(res, dtype=np.float32).reshape(B, T, N)
    assert (gm is None) == (r is None)
    Cout = np.zeros((B, T, Nout), dtype=np.float32) if out is None else np.ascontiguousarray(out, dtype=np.float32).reshape(B, T, Nout).copy()
    us = np.zeros(1, dtype=np.float32)
    mode = ((1 if gelu else 0) | (2 if gm is not None else 0) | (4 if skip_rows else 0) | (8 if swiglu else 0) | (16 if padded else 0) |
            (32 if range_check else 0))
    _check(lib.sva_test_gemm_h16(device, B, T, N, Cin, taps, dil, stride, _ptr(A), _ptr(W), _ptr(b), _ptr(gm), _ptr(r), mode, int(config[0]),
                                 int(config[1]), int(config[2]), _ptr(Cout), int(iters), _ptr(us)), "sva_test_gemm_h16")
    return Cout, float(us[0])


def test_prefill_attention(q, keys, vals, pos0=0, S=2048, half_kv=False, iters=0, device=0):
    """q [M, H*64], keys / vals [pos0 + M, H*64] -> (per-row kernel output, MFMA flash kernel output, (us_ref, us_mfma))."""
    lib = load_library()
    q = np.ascontiguousarray(q, dtype=np.float32)
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    M, D = q.shape
    assert keys.shape == (pos0 + M, D) and vals.shape == keys.shape and D % 64 == 0
    o1, o2 = np.empty((M, D), np.float32), np.empty((M, D), np.float32)
    us = np.zeros(2, np.float32)
    _check(lib.sva_test_prefill_attention(device, M, D // 64, int(pos0), int(S), _ptr(q), _ptr(keys), _ptr(vals), int(bool(half_kv)), _ptr(o1), _ptr(o2),
                                          int(iters), _ptr(us)), "sva_test_prefill_attention")
    return o1, o2, (float(us[0]), float(us[1]))


def test_pair_attention(q, keys, vals, pos0=0, S=2048, half_kv=False, iters=0, device=0):
    """as test_prefill_attention, the second output from the decode frame's PAIRED kernel (rows 2 i, 2 i + 1 = consecutive positions; M even)"""
    lib = load_library()
    q = np.ascontiguousarray(q, dtype=np.float32)
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    M, D = q.shape
    assert M % 2 == 0 and keys.shape == (pos0 + M, D) and vals.shape == keys.shape and D % 64 == 0
    o1, o2 = np.empty((M, D), np.float32), np.empty((M, D), np.float32)
    us = np.zeros(2, np.float32)
    _check(lib.sva_test_pair_attention(device, M, D // 64, int(pos0), int(S), _ptr(q), _ptr(keys), _ptr(vals), int(bool(half_kv)), _ptr(o1), _ptr(o2),
                                       int(iters), _ptr(us)), "sva_test_pair_attention")
    return o1, o2, (float(us[0]), float(us[1]))


# ---- per-kernel hooks of the non-GEMM launchers (include/sva.h); tests/test_gpu_kernels.py compares them with fp64 references ----
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def test_decode_attention(variant, qkv, cache, slot, pos, rope=None, x=None, W=None, norm_w=None, half_kv=False, out_fill=0.0, device=0):
    """qkv [M, 3 H 64], cache [n_slots, 2, H, S, 64] -> (out [M, H 64], qkv after the launch, cache after the launch); variants in include/sva.h"""
    lib = load_library()
    qkv, cache = np.array(qkv, dtype=np.float32, order="C"), np.array(cache, dtype=np.float32, order="C")
    slot, pos = np.ascontiguousarray(slot, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
    n_slots, _, H, S, _ = cache.shape
    M = qkv.shape[0]
    assert qkv.shape == (M, 3 * H * 64) and cache.shape == (n_slots, 2, H, S, 64) and slot.shape == (M,) and pos.shape == (M,)
    rope, x, W, norm_w = _f32(rope), _f32(x), _f32(W), _f32(norm_w)
    assert x is None or x.shape == (M, H * 64)
    assert W is None or W.shape == ((3 if variant == 6 else 1) * H * 64, H * 64)
    out = np.full((M, H * 64), out_fill, np.float32)
    _check(lib.sva_test_decode_attention(device, int(variant), M, H, S, n_slots, _ptr(slot), _ptr(pos), int(bool(half_kv)), _ptr(qkv), _ptr(cache), _ptr(rope),
                                         0 if rope is None else rope.shape[0], _ptr(x), _ptr(W), _ptr(norm_w), _ptr(out)), "sva_test_decode_attention")
    return out, qkv, cache


def test_enc_attention(qkv, rope, H, row0=0, n_planes=0, blocked=False, fill=0.0, device=0):
    """qkv [B, T, 3 H 64] -> (out [B, T, H 64] pre-filled with `fill`, planes uint16 [2, B T H 64] pre-filled with 0xFFFF or None)"""
    lib = load_library()
    qkv, rope = _f32(qkv), _f32(rope)
    B, T, _ = qkv.shape
    assert qkv.shape == (B, T, 3 * H * 64) and rope.shape == (T, 32, 2)
    out = np.full((B, T, H * 64), fill, np.float32)
    planes = np.full((2, B * T * H * 64), 0xFFFF, np.uint16) if n_planes else None
    _check(lib.sva_test_enc_attention(device, B, T, H, int(row0), _ptr(qkv), _ptr(rope), int(n_planes), int(bool(blocked)), _ptr(out), _ptr(planes)),
           "sva_test_enc_attention")
    return out, planes


def test_rowop(kind, x, B, T, C, params, eps, out, x_bstride, x_off=0, ldx=None, o_bstride=None, o_off=0, ldo=None, skip=(0, 0), n_planes=0, blocked=False,
               device=0):
    """kind 0 dwconv7 + LayerNorm, 1 LayerNorm rows, 2 RMSNorm rows over the flat arrays x / out (out is updated in place and returned with the
    planes uint16 [2, len(out)], pre-filled with 0xFFFF, or None)"""
    lib = load_library()
    x = _f32(x).reshape(-1)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 1
    p = [_f32(a) for a in params] + [None] * (4 - len(params))
    planes = np.full((2, out.size), 0xFFFF, np.uint16) if n_planes else None
    _check(lib.sva_test_rowop(device, int(kind), B, T, C, _ptr(x), x.size, int(x_bstride), int(x_off), int(C if ldx is None else ldx), _ptr(p[0]), _ptr(p[1]),
                              _ptr(p[2]), _ptr(p[3]), float(eps), _ptr(out), out.size, int(T * C if o_bstride is None else o_bstride), int(o_off),
                              int(C if ldo is None else ldo), int(skip[0]), int(skip[1]), int(n_planes), int(bool(blocked)), _ptr(planes), out.size),
           "sva_test_rowop")
    return out, planes


def test_bsq(z, B, T, W, bias, idx_out, z_bstride, z_off=0, ldz=None, norm_w=None, eps=1e-5, zn_out=None, idx_bstride=None, idx_off=0, u_out=None, device=0):
    """launch_bsq over the flat array z; idx_out int64 [n], zn_out (flat, like z) and u_out [n, nbits] are updated in place"""
    lib = load_library()
    z, W, bias, norm_w = _f32(z).reshape(-1), _f32(W), _f32(bias), _f32(norm_w)
    nbits, Cc = W.shape
    assert idx_out.dtype == np.int64 and idx_out.flags.c_contiguous
    assert zn_out is None or (zn_out.dtype == np.float32 and zn_out.size == z.size and zn_out.flags.c_contiguous)
    assert u_out is None or (u_out.dtype == np.float32 and u_out.shape == (idx_out.size, nbits) and u_out.flags.c_contiguous)
    _check(lib.sva_test_bsq(device, B, T, Cc, _ptr(z), z.size, int(z_bstride), int(z_off), int(Cc if ldz is None else ldz), _ptr(norm_w), float(eps), _ptr(zn_out),
                            _ptr(W), _ptr(bias), nbits, _ptr(idx_out), idx_out.size, int(T if idx_bstride is None else idx_bstride), int(idx_off), _ptr(u_out)),
           "sva_test_bsq")
    return idx_out, u_out, zn_out


def test_stft_ring(ring, mag, step=None, n_chunk=0, add=0, m0=0, nfr=1, second=None, device=0):
    """ring [B, N], mag [B, rows, ldm] (updated in place); second = (m0b, nfrb, row_b0) selects the two-range launch"""
    lib = load_library()
    ring = _f32(ring)
    B, N = ring.shape
    assert mag.dtype == np.float32 and mag.flags.c_contiguous and mag.shape[0] == B
    st = None if step is None else np.array([step], np.int32)
    m0b, nfrb, row_b0 = second if second is not None else (0, 0, 0)
    _check(lib.sva_test_stft_ring(device, B, N, _ptr(ring), _ptr(st), int(n_chunk), int(add), int(m0), int(nfr), int(second is not None), int(m0b), int(nfrb),
                                  int(row_b0), _ptr(mag), mag.shape[1], mag.shape[2]), "sva_test_stft_ring")
    return mag


def test_fsq(encode, lat, codes, B, T, G, gdim, Wt, bs, l_bstride, l_off, ld, c_bstride, c_gstride, device=0):
    """flat lat (float32) and codes (int32), updated in place: encode lat -> codes, else codes -> lat"""
    lib = load_library()
    assert lat.dtype == np.float32 and codes.dtype == np.int32 and lat.flags.c_contiguous and codes.flags.c_contiguous
    Wt, bs = _f32(Wt), _f32(bs)
    _check(lib.sva_test_fsq(device, int(bool(encode)), B, T, G, gdim, _ptr(lat), lat.size, int(l_bstride), int(l_off), int(ld), _ptr(Wt), _ptr(bs), _ptr(codes),
                            codes.size, int(c_bstride), int(c_gstride)), "sva_test_fsq")
    return lat, codes


def test_conv_post(x, pcm, B, T, Cc, k, w, bias, x_bstride, x_off, p_bstride, p_off, slot_flag=None, device=0):
    lib = load_library()
    x, w, bias = _f32(x).reshape(-1), _f32(w), _f32(bias)
    assert pcm.dtype == np.float32 and pcm.flags.c_contiguous
    flag = None if slot_flag is None else np.ascontiguousarray(slot_flag, dtype=np.int32)
    assert flag is None or flag.shape == (B,)
    _check(lib.sva_test_conv_post(device, B, T, Cc, k, _ptr(x), x.size, int(x_bstride), int(x_off), _ptr(w), _ptr(bias), _ptr(pcm), pcm.size, int(p_bstride),
                                  int(p_off), _ptr(flag)), "sva_test_conv_post")
    return pcm


# ---- the tail of the AR decode (include/sva.h; tests/test_gpu_decode_tail.py) ----
class Refused(RuntimeError):
    """a launcher's own check declined the problem before any launch"""


def _hook_call(fn, what, desc, fpar, arrays, *lead):
    """desc / fpar / ptrs convention of the decode-tail hooks; rc 1 (the launcher refused) raises Refused with the launcher's message"""
    d = np.array([int(v) for v in desc], np.int64)
    f = np.array([float(v) for v in fpar] + [0.0], np.float32)
    ptrs = (C.c_void_p * max(len(arrays), 1))()
    for i, a in enumerate(arrays):
        assert a is None or (isinstance(a, np.ndarray) and a.flags.c_contiguous), (what, i)
        ptrs[i] = None if a is None else a.ctypes.data
    rc = fn(*lead, _ptr(d), _ptr(f), ptrs)
    if rc == 1:
        raise Refused(load_library().sva_last_error().decode("utf-8", "replace"))
    _check(rc, what)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def test_sampler_launch(logits, rows, V, ldl, col_off=0, small=False, noise=None, ldn=0, noise_off=0, seed=None, frame=None, kind=0, noise_elem_off=0,
                        temperature=0.7, top_p=0.7, tok_raw=None, tok=None, tok_stride=1, tok_off=0, forced=None, forced_stride=0, forced_off=0,
                        use_forced=None, emb_table=None, emb_out=None, ldo=0, edits=None, device=0, _hook=None):
    """launch_sampler / launch_sampler_small (small) over the flat float32 array `logits` (rows at col_off + r ldl; edited in place when
    edits = dict(prev, prev_cap, W, suppress, penalty) is given: launch_logit_edits runs first on the same device rows).  noise: flat array or None
    (device RNG from seed [rows] uint64, frame [rows]).  tok_raw / tok (int32, flat) and emb_out (float32, flat) are updated in place."""
    lib = load_library()
    assert logits.dtype == np.float32 and logits.ndim == 1 and tok_raw.dtype == np.int32
    noise, emb_table = _f32(noise), _f32(emb_table)
    seed = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint64)
    frame, forced = _i32(frame), _i32(forced)
    assert tok is None or (tok.dtype == np.int32 and tok.size == tok_raw.size)
    assert emb_out is None or emb_out.dtype == np.float32
    e = edits or {}
    prev, sup = _i32(e.get("prev", [])), _i32(e.get("suppress", []))
    desc = [int(bool(small)), rows, V, ldl, col_off, logits.size, ldn, noise_off, 0 if noise is None else noise.size, kind, noise_elem_off, tok_stride, tok_off,
            tok_raw.size, forced_stride, forced_off, 0 if forced is None else forced.size, -1 if use_forced is None else int(use_forced),
            0 if emb_table is None else emb_table.shape[0], 0 if emb_table is None else emb_table.shape[1], ldo, 0 if emb_out is None else emb_out.size,
            int(edits is not None), e.get("W", prev.size), e.get("prev_cap", 4096), prev.size, e.get("n_suppress", sup.size), sup.size]
    _hook_call(_hook or lib.sva_test_sampler_launch, "sva_test_sampler_launch" if _hook is None else "sva_test_sampler_rows", desc,
               [temperature, top_p, e.get("penalty", 1.5)],
               [logits, noise, seed, frame, tok_raw, tok, forced, emb_table, emb_out, prev if prev.size else None, sup if sup.size else None], device)
    return tok_raw


def sampling_pairs(settings):
    """[(temperature, top_p)] -> float32 [n][2] = {inv_temp, top_p} as the samplers read them: the quotient in float, temperature clamped at 1e-5"""
    s = np.asarray(settings, np.float32).reshape(-1, 2)
    return np.ascontiguousarray(np.stack([np.float32(1.0) / np.maximum(s[:, 0], np.float32(1e-5)), s[:, 1]], axis=1), dtype=np.float32)


def test_sampler_rows(logits, rows, V, ldl, pairs=None, row_slot=None, **kw):
    """test_sampler_launch through sva_test_sampler_rows: row r samples with pairs[row_slot[r]] (row_slot None: pairs[r]), pairs = [(temperature,
    top_p)]; pairs None hands a null pointer over and the scalars temperature / top_p of `kw` apply"""
    lib = load_library()
    sp = None if pairs is None else sampling_pairs(pairs)
    rs = _i32(row_slot)

    def hook(device, d, f, ptrs):
        return lib.sva_test_sampler_rows(device, d, f, ptrs, _ptr(sp), 0 if sp is None else sp.shape[0], _ptr(rs))

    return test_sampler_launch(logits, rows, V, ldl, _hook=hook, **kw)


AR_NUCLEUS_INSTS = {0: (4, 4, 1024), 1: (4, 32, 8192), 2: (8, 16, 8192), 3: (1, 16, 1024)}        # inst -> (NW, PER, largest V)


def test_ar_nucleus(inst, logits, noise=None, seed=None, frame=None, kind=0, noise_elem_off=0, temperature=0.7, top_p=0.7, device=0):
    """ardev::nucleus_sample in one of its four instantiations over logits [rows, V] (noise [rows, V] or None: device RNG) ->
    (tokens [rows], every participating thread returned the token [rows] bool)"""
    lib = load_library()
    L, Q = _f32(logits), _f32(noise)
    rows, V = L.shape
    assert Q is None or Q.shape == L.shape
    seed = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint64)
    tok, same = np.full(rows, -1, np.int32), np.full(rows, -1, np.int32)
    _hook_call(lib.sva_test_ar_device, "sva_test_ar_device", [inst, rows, V, V, L.size, V, 0 if Q is None else Q.size, kind, noise_elem_off], [temperature, top_p],
               [L.reshape(-1), None if Q is None else Q.reshape(-1), seed, _i32(frame), tok, same], device, 0)
    return tok, same == 1


AR_GEMV_INSTS = [(768, 6, 2, True), (768, 2, 2, False), (768, 12, 2, True), (2304, 2, 2, False), (768, 11, 1, True),
                 (768, 6, 1, True), (768, 2, 1, False), (768, 12, 1, True), (2304, 2, 1, False), (768, 3, 1, True)]      # (K, ROWS, M, NORM)


def test_ar_gemv(inst, W, x, norm_w=None, eps=1e-5, half=False, row0=0, ldo=None, fill=0.0, device=0):
    """ardev::gemv<WT, K, ROWS, M, NORM> of instantiation `inst` over W [groups ROWS, K] (rounded to fp16 when half; placed at row `row0` of the device
    array), x [M, ldx] -> (out [M, ldo] pre-filled with `fill`, all 64 lanes agreed [groups] bool)"""
    lib = load_library()
    K, ROWS, M, norm = AR_GEMV_INSTS[inst]
    W, x, norm_w = _f32(W), _f32(x), _f32(norm_w)
    assert W.shape[1] == K and W.shape[0] % ROWS == 0 and x.shape[0] == M
    groups = W.shape[0] // ROWS
    ldo = W.shape[0] if ldo is None else ldo
    out, same = np.full((M, ldo), fill, np.float32), np.full(groups, -1, np.int32)
    _hook_call(lib.sva_test_ar_device, "sva_test_ar_device", [inst, int(bool(half)), groups, row0, x.shape[1], x.size, ldo, out.size], [eps],
               [W, x, norm_w, out, same], device, 1)
    return out, same == 1


def test_gemv(W, Y, M, N, K, X=None, ldx=None, ldy=None, y_off=0, norm_w=None, bias=None, res=None, ldr=0, alias=False, mode=0, eps=1e-5, S=0, H=0, device=0):
    """launch_gemv (modes 0, 1; 3 / 4 with zero operands) over W [rows, K], X flat / [M, ldx], Y flat float32 (updated in place); raises Refused when
    launch_gemv declines"""
    lib = load_library()
    W, X, norm_w, bias, res = _f32(W), _f32(X), _f32(norm_w), _f32(bias), _f32(res)
    assert Y.dtype == np.float32 and Y.flags.c_contiguous
    desc = [M, N, K, K if ldx is None else ldx, 0 if X is None else X.size, W.shape[0], N if ldy is None else ldy, y_off, Y.size, ldr, 0 if res is None else res.size,
            mode, int(bool(alias)), S, H]
    _hook_call(lib.sva_test_gemv, "sva_test_gemv", desc, [eps], [X, W, norm_w, bias, res, Y], device)
    return Y


STEP_OPS = {"ar_prepare_step": 0, "apply_forced": 1, "ar_finish_frame": 2, "append_content": 3, "put_codes": 4, "build_prompt": 5, "build_delayfill": 6,
            "build_reprefill": 7, "finish_reprefill": 8, "copy_rows": 9, "copy_rows2": 10, "broadcast_row": 11, "fill_rows": 12, "inc": 13, "add_list": 14,
            "add_vec": 15, "set_slot_i32": 16, "history_rows_copy": 17, "history_rows_move": 18, "put_row": 19, "mean3": 20, "copy_tokens": 21}          # kernel of csrc/engine_kernels.hip -> kind of sva_test_step_ops


def test_step_op(name, desc, arrays, device=0):
    """the launcher of one bookkeeping kernel (sva_test_step_ops, include/sva.h: descriptor and array order per kind); the "(io)" arrays are updated in
    place; raises Refused when the hook or the launcher declines the arguments"""
    _hook_call(load_library().sva_test_step_ops, "sva_test_step_ops", desc, [], arrays, device, STEP_OPS[name])


def test_voc_level(X, Y3, W, bias, C, B, Tl, xH, x_bstride, y_bstride, dil, rows_per_frame, frames_done, device=0):
    """launch_voc_level over flat float32 arrays: X, the three branch outputs Y3 (updated in place), the 18 weights W back to back, bias [18, C]
    -> the tile height the launcher chose"""
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in [X, W, bias] + list(Y3)) and len(Y3) == 3 and Y3[0].size == Y3[1].size == Y3[2].size
    tr = np.full(1, -1, np.int32)
    _hook_call(load_library().sva_test_voc_level, "sva_test_voc_level",
               [C, B, Tl, xH, x_bstride, X.size, y_bstride, Y3[0].size, dil[0], dil[1], dil[2], rows_per_frame, frames_done], [], [X, Y3[0], Y3[1], Y3[2], W, bias, tr], device)
    return int(tr[0])


_VOC_CONV_INTS = ("taps", "dil", "a_rows_b", "a_row0", "c_bstride", "c_off", "f_len", "r_bstride", "r_off", "r_len", "c_rows_b", "c_row0", "conv", "conv_row0",
                  "conv_T", "drop")
_VOC_CONV_PTRS = ("A", "Ap", "W", "Wp", "bias", "res", "Cf", "Cp")
_VOID_P = C.c_void_p          # (test_voc_conv names the channel count C)


def test_voc_conv(members, C, mode, B, T, cu_limit=0, repeat=False, ovf=None, n=None, device=0):
    """launch_voc_conv on one group of 1..3 members (include/sva.h: sva_test_voc_conv).  A member is a dict of the descriptor fields by name (taps, dil,
    a_rows_b, a_row0; c_bstride, c_off with Cf; r_bstride, r_off with res; c_rows_b, c_row0 with Cp; conv = 0 | 1 | 2 with conv_row0, conv_T and A;
    drop) and of its arrays: Ap uint16 (in and out), W float32 [C, taps C], Wp uint16 (out), optional A, bias, res, Cf (float32, flat) and Cp (uint16);
    res, Cf and Cp come back whole.  ovf: int32 [1] or None; n: the group's member count where it is not len(members).
    -> dict(refused, identical): refused = a row outside an array or the launcher's own refusal (no array was written), identical = the repeat verdict"""
    lib = load_library()
    nm = len(members)
    assert 1 <= nm <= 3
    desc = np.zeros(8 + 16 * nm, np.int64)
    desc[:7] = [C, mode, B, T, nm if n is None else n, cu_limit, int(bool(repeat))]
    same = np.full(1, -1, np.int32)
    ptrs = (_VOID_P * (2 + 8 * nm))()
    assert ovf is None or (ovf.dtype == np.int32 and ovf.size == 1)
    ptrs[0], ptrs[1] = None if ovf is None else ovf.ctypes.data, same.ctypes.data
    for i, m in enumerate(members):
        m = dict(m)
        for name, dt in (("A", np.float32), ("Ap", np.uint16), ("W", np.float32), ("Wp", np.uint16), ("bias", np.float32), ("res", np.float32), ("Cf", np.float32),
                         ("Cp", np.uint16)):
            a = m.get(name)
            assert a is None or (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous), name
            ptrs[2 + 8 * i + _VOC_CONV_PTRS.index(name)] = None if a is None else a.ctypes.data
        m["f_len"] = 0 if m.get("Cf") is None else m["Cf"].size
        m["r_len"] = 0 if m.get("res") is None else m["res"].size
        for j, name in enumerate(_VOC_CONV_INTS):
            desc[8 + 16 * i + j] = int(m.get(name, 0))
    fpar = np.zeros(1, np.float32)
    rc = lib.sva_test_voc_conv(device, _ptr(desc), _ptr(fpar), ptrs)
    if rc not in (0, 1):
        _check(rc, "sva_test_voc_conv")
    return dict(refused=rc == 1, identical=None if same[0] < 0 else bool(same[0]))


def test_logit_edits(logits, rows, V, ldl, prev, suppress, penalty, W=None, prev_cap=4096, device=0):
    """launch_logit_edits in place on the flat float32 array logits"""
    lib = load_library()
    assert logits.dtype == np.float32 and logits.ndim == 1
    prev, sup = _i32(prev), _i32(suppress)
    _hook_call(lib.sva_test_token_ops, "sva_test_token_ops", [rows, V, ldl, logits.size, prev.size if W is None else W, prev_cap, prev.size, sup.size, sup.size], [penalty],
               [logits, prev if prev.size else None, sup if sup.size else None], device, 0)
    return logits


def test_gather_rows(table, idx, idx_stride, idx_offset, rows, out, ldo, device=0):
    lib = load_library()
    table, idx = _f32(table), _i32(idx)
    assert out.dtype == np.float32 and out.ndim == 1
    _hook_call(lib.sva_test_token_ops, "sva_test_token_ops", [rows, table.shape[1], ldo, out.size, table.shape[0], idx.size, idx_stride, idx_offset], [],
               [table, idx, out], device, 1)
    return out


def test_audio_embed(table, codes, code_stride, cb_stride, rows, ncb, codebook_size, out, ldo, device=0):
    lib = load_library()
    table, codes = _f32(table), _i32(codes)
    assert out.dtype == np.float32 and out.ndim == 1
    _hook_call(lib.sva_test_token_ops, "sva_test_token_ops",
               [rows, table.shape[1], ldo, out.size, table.shape[0], codes.size, code_stride, cb_stride, ncb, codebook_size], [], [table, codes, out], device, 2)
    return out


def test_shift_history(buf, descs, B, col_slices=1, counter=None, counter_add=0, device=0):
    """launch_shift_history over the flat float32 array buf (in place); descs = [(offset, bstride, H, T, C), ...] -> the counter after the launch"""
    lib = load_library()
    assert buf.dtype == np.float32 and buf.ndim == 1
    cnt = None if counter is None else np.array([counter], np.int32)
    desc = [len(descs), B, col_slices, int(counter is not None), counter_add, buf.size] + [v for dsc in descs for v in dsc]
    _hook_call(lib.sva_test_token_ops, "sva_test_token_ops", desc, [], [buf, cnt], device, 3)
    return None if cnt is None else int(cnt[0])


def test_ring_write(ring, chunk, step=None, slot_flag=None, device=0):
    """launch_ring_write: chunk [B, n] into ring [B, N] (in place) at (step n) % N; step None -> the launcher's nullptr"""
    lib = load_library()
    chunk = np.ascontiguousarray(chunk, dtype=np.float32)
    assert ring.dtype == np.float32 and ring.flags.c_contiguous and ring.shape[0] == chunk.shape[0]
    _hook_call(lib.sva_test_token_ops, "sva_test_token_ops", [ring.shape[0], ring.shape[1], chunk.shape[1], int(step is not None), 0 if step is None else step], [],
               [ring, chunk, _i32(slot_flag)], device, 4)
    return ring


def test_gemm_choice(A, W, choice, bias=None, device=0):
    """C = A @ W.T (+bias) through ONE dispatch choice (kind, a, b, c) of the autotuned GEMM (see include/sva.h)."""
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), dtype=np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    _check(lib.sva_test_gemm_choice(device, M, N, K, _ptr(A), _ptr(W), _ptr(b), _ptr(out), *[int(x) for x in choice]), "sva_test_gemm_choice")
    return out


def test_gemm_plan(members):
    """the dispatcher's decision for 1..3 group members, each 12 ints (include/sva.h: sva_test_gemm_plan); no GPU needed.
    -> (family, a, b, c, z, report_kind); RuntimeError where the dispatcher refuses the problem"""
    desc = (C.c_int * (12 * len(members)))(*[int(x) for m in members for x in m])
    out = (C.c_int * 6)()
    _check(load_library().sva_test_gemm_plan(desc, len(members), out), "sva_test_gemm_plan")
    return tuple(out)


_CONV_GEMM_INTS = ("B", "T", "N", "Cin", "taps", "stride", "dil", "lda", "a_off", "a_bstride", "a_len", "ldc", "c_off", "c_bstride", "c_len", "ldr", "r_off",
                   "r_bstride", "r_len", "act", "accumulate", "a_silu", "w13", "skip_lo", "skip_hi", "use_wk", "pmode", "a_planes", "c_planes", "cp_silu")
_CONV_GEMM_PTRS = ("A", "W", "bias", "gamma", "res", "rms_w", "dw_wT", "dw_b", "ln_w", "ln_b", "C", "Cp", "Ap")
_CONV_GEMM_DEFAULTS = dict(stride=1, dil=1, taps=1, act=0, accumulate=0, a_silu=0, w13=0, skip_lo=0, skip_hi=0, use_wk=0, pmode=-1, a_planes=0, c_planes=0,
                           cp_silu=0, ldr=0, r_off=0, r_bstride=0, a_off=0, c_off=0)


def test_conv_gemm(members, plan=None, repeat=False, device=0):
    """1..3 conv-GEMM group members through the dispatcher (plan None) or one given plan (GemmFamily number, a, b, c, z) -- include/sva.h:
    sva_test_conv_gemm.  A member is a dict of the hook's descriptor fields by name (B, T, N, Cin, taps, stride, dil, lda, a_off, a_bstride, ldc,
    c_off, c_bstride, ldr, r_off, r_bstride, act, accumulate, a_silu, w13, skip_lo, skip_hi, use_wk, pmode, a_planes, c_planes, cp_silu, scale, ln_eps,
    rms_eps) and of its arrays: A, C and res the WHOLE flat float32 arrays (C, and the uint16 Cp, are written in place), W [N][taps Cin], the optional
    vectors, Ap an optional uint16 array that receives the A planes.  -> dict(refused, kind, identical): refused = the problem was declined before any
    launch (the arrays are as they went in), kind = the family number of the profiling tables, identical = the repeat verdict (None: not asked)."""
    lib = load_library()
    n = len(members)
    desc = np.zeros((n, 32), np.int64)
    fpar = np.zeros((n, 4), np.float32)
    ptrs = (C.c_void_p * (16 * n))()
    keep = []
    for i, m in enumerate(members):
        m = dict(_CONV_GEMM_DEFAULTS, **m)
        for name in ("A", "C", "W"):
            a = m[name]
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous, name
        m["a_len"], m["c_len"], m["r_len"] = m["A"].size, m["C"].size, 0
        if m.get("res") is not None:
            assert m["res"].dtype == np.float32 and m["res"].flags.c_contiguous
            m["r_len"] = m["res"].size
        for name in ("Cp", "Ap"):
            if m.get(name) is not None:
                assert m[name].dtype == np.uint16 and m[name].flags.c_contiguous, name
        for j, name in enumerate(_CONV_GEMM_INTS):
            desc[i, j] = int(m[name])
        fpar[i] = (m.get("scale", 1.0), m.get("ln_eps", 1e-6), m.get("rms_eps", 1e-5), 0.0)
        for j, name in enumerate(_CONV_GEMM_PTRS):
            a = m.get(name)
            if a is not None and name not in ("A", "C", "res", "Cp", "Ap"):
                a = _f32(a)
                keep.append(a)
            ptrs[16 * i + j] = None if a is None else a.ctypes.data
    pl = (C.c_int * 5)(*([-1, 0, 0, 0, 1] if plan is None else [int(x) for x in plan]))
    out = (C.c_int * 2)()
    rc = lib.sva_test_conv_gemm(device, n, _ptr(desc), _ptr(fpar), ptrs, pl, 1 if repeat else 0, out)
    if rc not in (0, 1):
        _check(rc, "sva_test_conv_gemm")
    return dict(refused=rc == 1, kind=int(out[0]), identical=None if out[1] < 0 else bool(out[1]))


def test_prefill_attention_runs(runs, total_rows, H, S, n_slots, half_kv, q, cache, out, single_out=None, device=0):
    """launch_ar_prefill_attention_runs on caller-chosen runs (include/sva.h: sva_test_prefill_attention_runs); out / single_out are written in
    place.  Returns True when the launcher refused."""
    r = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 4)
    assert q.dtype == np.float32 and q.shape == (total_rows, H * 64) and q.flags.c_contiguous
    assert cache.dtype == np.float32 and cache.size == n_slots * 2 * H * S * 64 and cache.flags.c_contiguous
    for o in (out, single_out):
        assert o is None or (o.dtype == np.float32 and o.shape == (total_rows, H * 64) and o.flags.c_contiguous)
    rc = load_library().sva_test_prefill_attention_runs(device, r.shape[0], _ptr(r), int(total_rows), int(H), int(S), int(n_slots), int(bool(half_kv)), _ptr(q),
                                                        _ptr(cache), _ptr(out), _ptr(single_out))
    if rc == 1:
        return True
    _check(rc, "sva_test_prefill_attention_runs")
    return False


def test_prefill_pack(M, Mmax):
    """the packing of sva_generate_many's prompt passes (include/sva.h: sva_test_prefill_pack), no GPU needed ->
    (pass_of [n], row0_of [n], tiles: per pass a list of (run inside the pass, q0))"""
    m = np.ascontiguousarray(M, dtype=np.int32).reshape(-1)
    n = m.shape[0]
    cap = 2 * n + n + 2 * (int(np.maximum(m, 0).sum()) // 16 + n) + 8
    out = np.zeros(cap, dtype=np.int32)
    n_pass = load_library().sva_test_prefill_pack(_ptr(m), n, int(Mmax), _ptr(out), cap)
    if n_pass < 0:
        _check(n_pass, "sva_test_prefill_pack")
    head = out[:2 * n].reshape(n, 2)
    tiles, k = [], 2 * n
    for _ in range(n_pass):
        nt = int(out[k])
        tiles.append([(int(a), int(b)) for a, b in out[k + 1:k + 1 + 2 * nt].reshape(nt, 2)])
        k += 1 + 2 * nt
    return head[:, 0].copy(), head[:, 1].copy(), tiles


def test_slot_book(cfg, ops):
    """the slot book's trace for a script of ops (include/sva.h: sva_test_slot_book); no GPU needed.  cfg = (B, chunk, delay, max_seq_frames,
    buffer_frames, window, nspk), ops = [(op, slot, R), ...] -> int32 array [len(ops)][8 B + 6]"""
    B = int(cfg[0])
    c = (C.c_int * 7)(*[int(x) for x in cfg])
    o = (C.c_int * (3 * max(len(ops), 1)))(*[int(x) for op in ops for x in op])
    out = (C.c_int * ((8 * B + 6) * max(len(ops), 1)))()
    _check(load_library().sva_test_slot_book(c, o, len(ops), out), "sva_test_slot_book")
    return np.frombuffer(out, dtype=np.int32).reshape(max(len(ops), 1), 8 * B + 6)[:len(ops)].copy()


def test_slot_prompt_tail(R, Rt, ncb, P, first, n):
    """include/sva.h: sva_test_slot_prompt_tail -> (codes int32 [ncb][n], (ref_len, content kept, audio kept, last content code)); no GPU needed"""
    out, stored = (C.c_int * max(ncb * n, 1))(), (C.c_int * 4)()
    _check(load_library().sva_test_slot_prompt_tail(R, Rt, ncb, P, first, n, out, stored), "sva_test_slot_prompt_tail")
    return np.array(out[:ncb * n], dtype=np.int32).reshape(ncb, n), tuple(stored)


SNAPSHOT_INFO = ("version", "frames", "last_pos", "ncontent", "ref_len", "ar_dtype", "chunk_frames", "payload_bytes")
SNAPSHOT_REFUSALS = {0: "ok", -10: "truncated", -11: "bad_magic", -12: "bad_version", -13: "bad_header", -14: "bad_checksum", -15: "config_mismatch",
                     -16: "layout_mismatch", -17: "size_mismatch"}
SEG_PLAIN, SEG_RING, SEG_KV_PREFIX, SEG_BLOCKED_PLANE = 0, 1, 2, 3


def stream_blob_info(blob) -> dict:
    """sva_stream_blob_info: the header of a snapshot, validated without a GPU (ValueError for a truncated, corrupt or foreign blob)"""
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    info = (C.c_long * 8)()
    lib = load_library()
    rc = lib.sva_stream_blob_info(_ptr(buf) if buf.size else (C.c_char * 1)(), buf.size, info)
    if rc != 0:
        raise ValueError(f"not a valid stream snapshot (rc={rc}): {lib.sva_last_error().decode('utf-8', 'replace')}")
    return dict(zip(SNAPSHOT_INFO, (int(v) for v in info)))


def idle_batch(engine, n_streams, prompt, **params):
    """A begun, steady batch with every slot retired: the landing batch of Batch.load_stream / move_stream ("beginning a batch with empty
    slots" is not supported: this prefills a throw-away prompt (ac, cc, style, timbre) everywhere, begins, steps ceil(delay / chunk) times on
    silence so that the lock-step delay is filled, and retires every slot)."""
    ac, cc, style, timbre = prompt
    b = Batch(engine, n_streams=n_streams, **params)
    for s in range(n_streams):
        b.prefill_prompt(s, cc, ac, style, timbre, noise_seed=0)
    b.begin()
    zeros = np.zeros((n_streams, 2048 * b.chunk), np.float32)
    for _ in range(-(-b.p.delay // b.chunk)):
        b.step(zeros)
    for s in range(n_streams):
        b.retire(s)
    return b


def test_slot_pack(table, arena_src, arena_dst, slot_src, slot_dst, step_src=0, step_dst=0, cus=8, device=0):
    """include/sva.h: sva_test_slot_pack.  table [n_seg][9] int64, arenas uint8 -> (image uint8, destination arena after the unpack)"""
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 9)
    src = np.ascontiguousarray(arena_src, dtype=np.uint8)
    dst = np.ascontiguousarray(arena_dst, dtype=np.uint8).copy()
    nbytes = int(sum((int(r[5]) * int(r[4]) + 15) // 16 * 16 for r in t))
    img = np.zeros(max(nbytes, 1), np.uint8)
    _check(load_library().sva_test_slot_pack(device, _ptr(t), t.shape[0], _ptr(src), src.size, _ptr(dst), dst.size, int(slot_src), int(slot_dst),
                                             int(step_src), int(step_dst), _ptr(img), nbytes, int(cus)), "sva_test_slot_pack")
    return img[:nbytes], dst


def test_snapshot_build(cfg, layout, fields, ref_content, ref_audio, payload=b""):
    """include/sva.h: sva_test_snapshot_header op 0 -> blob bytes.  fields = (frames, last_pos, ncontent, ar_dtype, chunk_frames); no GPU needed"""
    ra = np.asarray(ref_audio, dtype=np.int64)
    ncb, ref_len = (ra.shape if ra.ndim == 2 else (0, len(ref_content)))
    desc = np.array([len(cfg), len(layout), *fields, ncb, ref_len], dtype=np.int64)
    sig = np.array([*cfg, *layout, *ref_content, *ra.reshape(-1)], dtype=np.int64)
    pl = np.frombuffer(bytes(payload), dtype=np.uint8)
    out = np.zeros(4096 + 8 * sig.size + pl.size, np.uint8)
    res = np.full(12, -1, np.int64)
    _check(load_library().sva_test_snapshot_header(0, _ptr(desc), _ptr(sig) if sig.size else None, _ptr(pl) if pl.size else None, pl.size, _ptr(out),
                                                   out.size, _ptr(res)), "sva_test_snapshot_header")
    return out[:int(res[0])].tobytes()


def test_snapshot_check(data, cfg, layout, payload_bytes=-1):
    """include/sva.h: sva_test_snapshot_header op 1 -> (refusal code, first differing signature index, info dict); no GPU needed"""
    desc = np.array([len(cfg), len(layout), payload_bytes], dtype=np.int64)
    sig = np.array([*cfg, *layout], dtype=np.int64)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    res = np.full(12, -1, np.int64)
    keep = np.zeros(1, np.uint8)
    _check(load_library().sva_test_snapshot_header(1, _ptr(desc), _ptr(sig) if sig.size else None, _ptr(buf) if buf.size else _ptr(keep), buf.size, None, 0,
                                                   _ptr(res)), "sva_test_snapshot_header")
    info = dict(zip(SNAPSHOT_INFO + ("ncb", "header_bytes"), (int(v) for v in res[2:])))
    return int(res[0]), int(res[1]), info


def host_launch_cost(device=0, iters=300):
    """microseconds the calling thread spends enqueueing one kernel (idle stream)"""
    us = (C.c_float * 1)()
    _check(load_library().sva_host_launch_cost(device, int(iters), us), "sva_host_launch_cost")
    return float(us[0])


def pin_enqueue_thread(device=0, group=8, iters=120):
    """Place the calling (enqueueing) thread on the group of `group` consecutive CPUs from which kernel launches to `device`
    are cheapest, among the CPUs the thread may run on now.  One streaming step is ~430 kernel launches; at 1-8 streams the
    enqueue rate of this thread is as tight a bound as the GPU's dependent-kernel chains, and it varies by ~30 % between
    core groups of a two-socket host (distance to the GPU's PCIe root).  Only the calling thread moves (sched_setaffinity on
    its tid); runtime helper threads that already exist keep their placement, so call this after the first batch has run.
    Returns (chosen cpu list, {first cpu of group: us per launch})."""
    import os
    allowed = sorted(os.sched_getaffinity(0))
    groups = {}
    for c in allowed:
        groups.setdefault(c // group, []).append(c)
    if len(groups) <= 1:
        return allowed, {}
    table = {}
    try:
        for g, cpus in sorted(groups.items()):
            os.sched_setaffinity(0, {cpus[0]})
            table[cpus[0]] = host_launch_cost(device, iters)   # (the call itself starts with 32 untimed launches: the thread has settled)
        best = min(table, key=table.get)
        chosen = groups[best // group]
    except Exception:
        os.sched_setaffinity(0, set(allowed))
        raise
    os.sched_setaffinity(0, set(chosen))
    return chosen, table


def test_sampler(logits, noise, variant, temperature=0.7, top_p=0.7, iters=0, device=0):
    """tokens [rows] of the nucleus sampler through ONE implementation (see include/sva.h); with iters > 0 also the average
    microseconds per launch -> (tokens, us)."""
    lib = load_library()
    L = np.ascontiguousarray(logits, dtype=np.float32)
    Q = np.ascontiguousarray(noise, dtype=np.float32)
    rows, V = L.shape
    assert Q.shape == L.shape
    out = np.empty(rows, dtype=np.int32)
    us = (C.c_float * 1)()
    _check(lib.sva_test_sampler(device, int(variant), rows, V, _ptr(L), _ptr(Q), float(temperature), float(top_p), _ptr(out), int(iters),
                                us if iters > 0 else None), "sva_test_sampler")
    return (out, float(us[0])) if iters > 0 else out


def bench_gemm_choice(B, T, N, Cin, kind, a=0, b=0, c=0, taps=1, dil=1, mode=0, nrot=1, iters=50, device=0):
    """one dispatch choice (csrc/testhooks.hip: sva_bench_gemm_choice) -> (us eager, us as a graph, max |C - C_dispatcher|, max |C_dispatcher|)"""
    lib = load_library()
    out = (C.c_float * 4)()
    _check(lib.sva_bench_gemm_choice(device, B, T, N, Cin, taps, dil, mode, kind, a, b, c, nrot, iters, out), "sva_bench_gemm_choice")
    return float(out[0]), float(out[1]), float(out[2]), float(out[3])


def bench_gemm(B, T, N, Cin, taps=1, dil=1, mode=0, iters=50, device=0):
    """average microseconds per conv-GEMM launch (device-resident random data)"""
    lib = load_library()
    out = (C.c_float * 1)()
    _check(lib.sva_bench_gemm(device, B, T, N, Cin, taps, dil, mode, iters, out), "sva_bench_gemm")
    return float(out[0])
