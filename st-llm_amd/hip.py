"""ctypes binding of libstllm_hip.so (include/stllm_hip.h) for torch tensors.

This is plumbing only: torch owns device memory and streams; every function here hands raw
``data_ptr()``s and the current HIP stream to the C ABI.  There is NO fallback: if the shared
library is missing or a call fails, a RuntimeError is raised (a product path that silently ran
on eager PyTorch would void every parity claim).
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

import torch

BF16, F16, F32, BF16X3 = 0, 1, 2, 3   # BF16X3: stllm_gemm / the stack entry points only (fp32 activations, split bf16 weights)
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE, EPI_PATCH = 0, 1, 2, 3, 4
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2

_DT = {torch.bfloat16: BF16, torch.float16: F16, torch.float32: F32}
_NAMES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32,
          "bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}

EXPORTS = ["stllm_last_error", "stllm_abi_version", "stllm_last_kernel", "stllm_synth_normal_f32", "stllm_gemm", "stllm_layernorm", "stllm_rmsnorm",
           "stllm_attention", "stllm_gather_rows", "stllm_mean_t", "stllm_vit_cls_rows", "stllm_cosine_rows",
           "stllm_cross_entropy_rows", "stllm_cast_rows", "stllm_gemm_workspace_bytes", "stllm_gemm_workspace_status", "stllm_gemm_plan", "stllm_gemm_w4_plan", "stllm_set_option",
           "stllm_preprocess_workspace_bytes", "stllm_preprocess_frames", "stllm_attention_decode_workspace_bytes",
           "stllm_attention_decode", "stllm_gemm_profile", "stllm_gemm_profile_count", "stllm_gemm_profile_read",
           "stllm_vit_blocks_scratch_bytes", "stllm_vit_blocks", "stllm_llama_layers_scratch_bytes", "stllm_llama_layers", "stllm_llama_layer_sp_scratch_bytes", "stllm_llama_layer_sp",
           "stllm_qformer_layers_scratch_bytes", "stllm_qformer_layers", "stllm_split3_rows", "stllm_gemm_split_ws_bytes",
           "stllm_lora_down_workspace_bytes", "stllm_lora_down", "stllm_llama_layers_lora_scratch_bytes", "stllm_llama_layers_lora",
           "stllm_attention_offset_workspace_bytes", "stllm_attention_offset", "stllm_llama_layers_extend", "stllm_gemv_w8", "stllm_gemv_q4",
           "stllm_attention_decode_ragged_workspace_bytes", "stllm_attention_decode_ragged", "stllm_kv_append_rows",
           "stllm_attention_shared_workspace_bytes", "stllm_attention_shared", "stllm_select_tokens", "stllm_beam_candidates",
           "stllm_attention_offset_ragged_workspace_bytes", "stllm_attention_offset_ragged", "stllm_kv_append_spans",
           "stllm_attention_segments_workspace_bytes", "stllm_attention_segments", "stllm_kv_append_segments", "stllm_select_slots",
           "stllm_attention_segments_shared_workspace_bytes", "stllm_attention_segments_shared", "stllm_kv_reorder_rows", "stllm_beam_candidates_rows"]


def torch_dtype(d):
    return _NAMES[d] if isinstance(d, str) else d


def dtype_code(d):
    return _DT[torch_dtype(d)]


class GemmArgs(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("epilogue", c_int), ("act", c_int), ("out_is_f32", c_int),
                ("A", c_void_p), ("lda", c_int64), ("W", c_void_p), ("ldw", c_int64),
                ("bias", c_void_p), ("out", c_void_p), ("ldo", c_int64),
                ("resid", c_void_p), ("ldr", c_int64),
                ("aux0", c_void_p), ("aux1", c_void_p), ("frames", c_void_p),
                ("rope_seq", c_int), ("rope_cols", c_int), ("M", c_int), ("N", c_int), ("K", c_int),
                ("a_rows_per_batch", c_int), ("a_batch_stride", c_int64),
                ("o_rows_per_batch", c_int), ("o_batch_stride", c_int64),
                ("workspace", c_void_p), ("workspace_bytes", c_int64),
                ("a_norm_x", c_void_p), ("a_norm_ldx", c_int64), ("a_norm_gamma", c_void_p), ("a_norm_eps", ctypes.c_float),
                ("split_ws", c_void_p), ("split_ws_bytes", c_int64), ("split_flags", c_int), ("w_frag", c_void_p)]


class GemvW8Args(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("epilogue", c_int), ("out_is_f32", c_int), ("M", c_int), ("N", c_int), ("K", c_int),
                ("A", c_void_p), ("lda", c_int64), ("Wq", c_void_p), ("ldw", c_int64), ("scale", c_void_p), ("bias", c_void_p),
                ("out", c_void_p), ("ldo", c_int64), ("resid", c_void_p), ("ldr", c_int64),
                ("rope_cos", c_void_p), ("rope_sin", c_void_p), ("rope_seq", c_int), ("rope_cols", c_int),
                ("a_rows_per_batch", c_int), ("a_batch_stride", c_int64), ("o_rows_per_batch", c_int), ("o_batch_stride", c_int64),
                ("a_norm_x", c_void_p), ("a_norm_ldx", c_int64), ("a_norm_gamma", c_void_p), ("a_norm_eps", c_float)]


class GemvQ4Args(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("epilogue", c_int), ("out_is_f32", c_int), ("M", c_int), ("N", c_int), ("K", c_int),
                ("A", c_void_p), ("lda", c_int64), ("Wq", c_void_p), ("ldw", c_int64), ("scale", c_void_p), ("ld_scale", c_int64), ("bias", c_void_p),
                ("out", c_void_p), ("ldo", c_int64), ("resid", c_void_p), ("ldr", c_int64),
                ("rope_cos", c_void_p), ("rope_sin", c_void_p), ("rope_seq", c_int), ("rope_cols", c_int),
                ("a_rows_per_batch", c_int), ("a_batch_stride", c_int64), ("o_rows_per_batch", c_int), ("o_batch_stride", c_int64),
                ("a_norm_x", c_void_p), ("a_norm_ldx", c_int64), ("a_norm_gamma", c_void_p), ("a_norm_eps", c_float)]


class SelectArgs(ctypes.Structure):
    """stllm_select_args (include/stllm_hip.h)"""
    _fields_ = [("logits", c_void_p), ("ldl", c_int64), ("rows", c_int), ("V", c_int), ("prev", c_void_p), ("ld_prev", c_int64), ("n_prev", c_int),
                ("penalty", c_float), ("suppress_eos", c_int), ("eos_id", c_int), ("pad_id", c_int), ("sample", c_int), ("temperature", c_float),
                ("top_p", c_float), ("u", c_void_p), ("unfinished", c_void_p), ("out", c_void_p), ("out_stride", c_int64), ("aux", c_void_p)]


class SelectSlotsArgs(ctypes.Structure):
    """stllm_select_slots_args (include/stllm_hip.h)"""
    _fields_ = [("logits", c_void_p), ("ldl", c_int64), ("rows", c_int), ("V", c_int), ("n_slots", c_int), ("src", c_void_p), ("state", c_void_p),
                ("ids", c_void_p), ("ld_ids", c_int64), ("penalty", c_float), ("min_length", c_int), ("eos_id", c_int), ("pad_id", c_int), ("sample", c_int),
                ("temperature", c_float), ("top_p", c_float), ("u", c_void_p), ("stops", c_void_p), ("ld_stop", c_int64), ("stop_len", c_void_p),
                ("n_stop", c_int), ("aux", c_void_p)]


class BeamArgs(ctypes.Structure):
    """stllm_beam_args (include/stllm_hip.h)"""
    _fields_ = [("logits", c_void_p), ("ldl", c_int64), ("rows", c_int), ("V", c_int), ("prev", c_void_p), ("ld_prev", c_int64), ("n_prev", c_int),
                ("penalty", c_float), ("suppress_eos", c_int), ("eos_id", c_int), ("beam_score", c_void_p), ("k", c_int), ("cand_score", c_void_p),
                ("cand_token", c_void_p)]


class BeamRowsArgs(ctypes.Structure):
    """stllm_beam_rows_args (include/stllm_hip.h)"""
    _fields_ = [("logits", c_void_p), ("ldl", c_int64), ("n_logits_rows", c_int), ("V", c_int), ("rows", c_int), ("src", c_void_p), ("prev", c_void_p),
                ("ld_prev", c_int64), ("n_prev", c_void_p), ("penalty", c_float), ("min_length", c_int), ("eos_id", c_int), ("beam_score", c_void_p),
                ("k", c_int), ("cand_score", c_void_p), ("cand_token", c_void_p)]


class VitBlockWeights(ctypes.Structure):
    _fields_ = [("n1w", c_void_p), ("n1b", c_void_p), ("e1", c_float),
                ("wqkv", c_void_p), ("ld_qkv", c_int64), ("bqkv", c_void_p),
                ("wproj", c_void_p), ("ld_proj", c_int64), ("bproj", c_void_p),
                ("n2w", c_void_p), ("n2b", c_void_p), ("e2", c_float),
                ("wfc1", c_void_p), ("ld_fc1", c_int64), ("bfc1", c_void_p),
                ("wfc2", c_void_p), ("ld_fc2", c_int64), ("bfc2", c_void_p)]


class VitBlocksArgs(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("n_seq", c_int), ("seq_len", c_int), ("num_heads", c_int), ("dim", c_int), ("hidden", c_int),
                ("x", c_void_p), ("ldx", c_int64), ("scratch", c_void_p), ("scratch_bytes", c_int64),
                ("workspace", c_void_p), ("workspace_bytes", c_int64)]


class LlamaLayerWeights(ctypes.Structure):
    _fields_ = [("ln1", c_void_p), ("wqkv", c_void_p), ("ld_qkv", c_int64), ("wo", c_void_p), ("ld_o", c_int64),
                ("ln2", c_void_p), ("wgu", c_void_p), ("ld_gu", c_int64), ("wdown", c_void_p), ("ld_down", c_int64),
                ("kv_cache", c_void_p), ("wqkv_frag", c_void_p), ("wgu_frag", c_void_p)]


class LlamaLayersArgs(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("B", c_int), ("S", c_int), ("n_heads", c_int), ("hidden", c_int), ("inter", c_int), ("eps", c_float),
                ("x", c_void_p), ("ldx", c_int64), ("rope_cos", c_void_p), ("rope_sin", c_void_p), ("kv_len", c_void_p),
                ("cache_max_len", c_int64), ("scratch", c_void_p), ("scratch_bytes", c_int64),
                ("workspace", c_void_p), ("workspace_bytes", c_int64)]


class LlamaLoraLayer(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("ld_a", c_int64), ("wqkv_ext", c_void_p), ("ld_ext", c_int64), ("r", c_int), ("P", c_int)]


class BertOutputWeights(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("ldw", c_int64), ("b", c_void_p), ("g", c_void_p), ("beta", c_void_p), ("eps", c_float)]


class QformerLayerWeights(ctypes.Structure):
    _fields_ = [("wqkv", c_void_p), ("ld_qkv", c_int64), ("bqkv", c_void_p), ("attn_out", BertOutputWeights),
                ("has_cross", c_int), ("ckv_index", c_int), ("cq_w", c_void_p), ("ld_cq", c_int64), ("cq_b", c_void_p),
                ("cross_out", BertOutputWeights),
                ("fq_w1", c_void_p), ("ld_fq1", c_int64), ("fq_b1", c_void_p), ("fq_out", BertOutputWeights),
                ("ft_w1", c_void_p), ("ld_ft1", c_int64), ("ft_b1", c_void_p), ("ft_out", BertOutputWeights)]


class QformerLayersArgs(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("n_seq", c_int), ("n_query", c_int), ("n_text", c_int), ("n_heads", c_int), ("hidden", c_int), ("inter", c_int),
                ("enc_len", c_int), ("enc_dim", c_int), ("n_cross", c_int),
                ("hq32", c_void_p), ("hq16", c_void_p), ("ht32", c_void_p), ("ht16", c_void_p),
                ("enc16", c_void_p), ("ld_enc", c_int64), ("ckv_w", c_void_p), ("ld_ckv", c_int64), ("ckv_b", c_void_p),
                ("kv_len", c_void_p), ("scratch", c_void_p), ("scratch_bytes", c_int64), ("workspace", c_void_p), ("workspace_bytes", c_int64)]


LIB_PATH = os.environ.get("STLLM_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libstllm_hip.so")   # STLLM_LIB: the trace build (tools only)
_lib = None


def _bind(L, strict=True):
    """argument / result types of the forward entry points on a loaded library.  strict=False skips symbols the library does not
    export (the host-emulated test build of a subset of the sources, tests/hipemu)."""
    def B(name, argtypes=None, restype=c_int):
        try:
            fn = getattr(L, name)
        except AttributeError:
            if strict:
                raise
            return
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = restype
    B("stllm_last_error", None, c_char_p)
    B("stllm_abi_version")
    B("stllm_last_kernel", None, c_char_p)
    B("stllm_synth_normal_f32", [c_void_p, c_int64, c_int64, ctypes.c_uint32, c_float, c_float])
    B("stllm_gemm", [ctypes.POINTER(GemmArgs), c_void_p])
    B("stllm_layernorm", [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p])
    B("stllm_rmsnorm", [c_int, c_void_p, c_int64, c_void_p, c_float, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p])
    B("stllm_attention", [c_int] + [c_void_p, c_int64, c_int64] * 4 + [c_int] * 5 + [c_float, c_int, c_void_p, c_void_p])
    B("stllm_gather_rows", [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int,
                            c_float, c_void_p])
    B("stllm_mean_t", [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p])
    B("stllm_vit_cls_rows", [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p])
    B("stllm_cosine_rows", [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p])
    B("stllm_cross_entropy_rows", [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p])
    B("stllm_cast_rows", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p])
    B("stllm_gemm_workspace_bytes", None, c_int64)
    B("stllm_set_option", [c_char_p, c_int])
    B("stllm_gemm_workspace_status", [c_void_p, c_void_p])
    B("stllm_preprocess_workspace_bytes", [c_int, c_int, c_int], c_int64)
    B("stllm_preprocess_frames", [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p])
    B("stllm_attention_decode_workspace_bytes", [c_int, c_int, c_int], c_int64)
    B("stllm_attention_decode", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int,
                                 c_int, c_int, c_int, c_float, c_void_p, c_int64, c_void_p])
    B("stllm_attention_decode_ragged_workspace_bytes", [c_int, c_int, c_int], c_int64)
    B("stllm_attention_decode_ragged", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int,
                                        c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_int64, c_void_p])
    B("stllm_kv_append_rows", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p])
    B("stllm_attention_shared_workspace_bytes", [c_int] * 6, c_int64)
    B("stllm_attention_shared", [c_int] + [c_void_p, c_int64, c_int64] * 3 + [c_int] + [c_void_p, c_int64, c_int64] * 2 + [c_void_p, c_int, c_int] +
      [c_void_p, c_int64, c_int64] + [c_int] * 5 + [c_float, c_int, c_void_p, c_int64, c_void_p])
    B("stllm_gemm_profile", [c_int, c_char_p])
    B("stllm_gemm_profile_count", [])
    B("stllm_gemm_profile_read", [c_int, c_char_p, c_int, ctypes.POINTER(c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)])
    B("stllm_split3_rows", [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_void_p])
    B("stllm_gemm_split_ws_bytes", [c_int] * 5, c_int64)
    B("stllm_vit_blocks_scratch_bytes", [c_int] * 5, c_int64)
    B("stllm_vit_blocks", [ctypes.POINTER(VitBlocksArgs), ctypes.POINTER(VitBlockWeights), c_int, c_void_p])
    B("stllm_llama_layers_scratch_bytes", [c_int] * 5, c_int64)
    B("stllm_llama_layers", [ctypes.POINTER(LlamaLayersArgs), ctypes.POINTER(LlamaLayerWeights), c_int, c_void_p])
    B("stllm_llama_layer_sp_scratch_bytes", [c_int] * 5, c_int64)
    B("stllm_llama_layer_sp", [ctypes.POINTER(LlamaLayersArgs), ctypes.POINTER(LlamaLayerWeights), c_void_p, c_int, c_int, c_int, c_void_p])
    B("stllm_qformer_layers_scratch_bytes", [c_int] * 9, c_int64)
    B("stllm_qformer_layers", [ctypes.POINTER(QformerLayersArgs), ctypes.POINTER(QformerLayerWeights), c_int, c_void_p])
    B("stllm_lora_down_workspace_bytes", [c_int] * 4, c_int64)
    B("stllm_lora_down", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p])
    B("stllm_llama_layers_lora_scratch_bytes", [c_int] * 6, c_int64)
    B("stllm_llama_layers_lora", [ctypes.POINTER(LlamaLayersArgs), ctypes.POINTER(LlamaLayerWeights), ctypes.POINTER(LlamaLoraLayer), c_int, c_void_p])
    B("stllm_attention_offset_workspace_bytes", [c_int] * 4, c_int64)
    B("stllm_attention_offset_ragged_workspace_bytes", [c_int] * 4, c_int64)
    B("stllm_attention_offset_ragged", [c_int] + [c_void_p, c_int64, c_int64] * 4 + [c_int] * 5 + [c_float, c_void_p, c_void_p, c_void_p, c_int64, c_void_p])
    B("stllm_kv_append_spans", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p])
    B("stllm_attention_segments_workspace_bytes", [c_int] * 4, c_int64)
    B("stllm_attention_segments", [c_int, c_void_p, c_int64] + [c_void_p, c_int64, c_int64] * 2 + [c_void_p, c_int64] + [c_int] * 7 + [c_float] + [c_void_p] * 5 +
      [c_int64, c_void_p])
    B("stllm_kv_append_segments", [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64] + [c_void_p] * 4 + [c_int] * 6 + [c_void_p])
    B("stllm_attention_segments_shared_workspace_bytes", [c_int] * 6, c_int64)
    B("stllm_attention_segments_shared", [c_int] + [c_void_p, c_int64] * 3 + [c_int] + [c_void_p, c_int64, c_int64] * 2 + [c_void_p, c_int64] + [c_int] * 7 +
      [c_float] + [c_void_p] * 5 + [c_int64, c_void_p])
    B("stllm_attention_offset", [c_int] + [c_void_p, c_int64, c_int64] * 4 + [c_int] * 5 + [c_float, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p])
    B("stllm_llama_layers_extend", [ctypes.POINTER(LlamaLayersArgs), ctypes.POINTER(LlamaLayerWeights), c_int, c_int, c_void_p, c_int64, c_void_p])
    B("stllm_gemv_w8", [ctypes.POINTER(GemvW8Args), c_void_p])
    B("stllm_gemv_q4", [ctypes.POINTER(GemvQ4Args), c_void_p])
    B("stllm_select_tokens", [ctypes.POINTER(SelectArgs), c_void_p])
    B("stllm_beam_candidates", [ctypes.POINTER(BeamArgs), c_void_p])
    B("stllm_select_slots", [ctypes.POINTER(SelectSlotsArgs), c_void_p])
    B("stllm_beam_candidates_rows", [ctypes.POINTER(BeamRowsArgs), c_void_p])
    B("stllm_kv_reorder_rows", [c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p])
    B("stllm_gemm_plan", [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)])
    B("stllm_gemm_w4_plan", [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)])
    return L


def lib():
    """Load libstllm_hip.so (built in-tree by stllm_amd.build / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found — run `python __graft_entry__.py` (build()) first; "
                               "there is no CPU/eager fallback for the HIP path")
        _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().stllm_last_error().decode()}")


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


class _PinnedRing:
    """Persistent pinned staging memory for the small host -> device copies of a step (index tables, lengths, labels).  `tensor.pin_memory()`
    per copy allocates pinned memory through the runtime, which SYNCHRONISES the device: the host then loses its whole lead over the GPU
    (measured: the first index table of the Q-Former stalled the host until the ViT had finished, and everything after it ran host-bound,
    profiles/r03_gaps.md).  Slots are reused round-robin; a slot's previous copy is awaited through its event before it is overwritten."""
    SLOTS, SLOT_BYTES = 128, 1 << 16

    def __init__(self):
        self.buf = torch.empty(self.SLOTS * self.SLOT_BYTES, dtype=torch.uint8).pin_memory()
        self.events = [None] * self.SLOTS
        self.i = 0

    def stage(self, t, dev):
        nbytes = t.numel() * t.element_size()
        if nbytes > self.SLOT_BYTES or nbytes == 0:
            return None
        k, self.i = self.i, (self.i + 1) % self.SLOTS
        if self.events[k] is not None:
            self.events[k].synchronize()
        view = self.buf[k * self.SLOT_BYTES: k * self.SLOT_BYTES + nbytes].view(t.dtype).view(t.shape)
        view.copy_(t)
        out = view.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.events[k] = ev
        return out


_pinned_ring = None


def h2d(t, device):
    """Host tensor -> device WITHOUT stalling the host: staged through the persistent pinned ring and enqueued on the current stream.
    A pageable `.to(device)` blocks the host until everything queued before the copy has run, and so does a fresh `pin_memory()`
    allocation — one pipeline bubble plus the host's lost lead per index table (profiles/r03_gaps.md)."""
    global _pinned_ring
    dev = torch.device(device)
    if dev.type != "cuda" or t.is_cuda:
        return t.to(dev)
    t = t.contiguous()
    # content-keyed cache of small tables (round 6): the index tables / labels / lengths of a step are functions of shapes and token
    # ids only — identical every step of a bench loop and every frame batch of a served prompt — so steady state issues NO host -> device copy at all.
    # The cached device tensors are shared between calls: READ-ONLY for every consumer (all of them are gather / label / length operands).
    key = None
    nbytes = t.numel() * t.element_size()
    if _H2D_CACHE_ON and 0 < nbytes <= _PinnedRing.SLOT_BYTES and t.dtype in (torch.int32, torch.int64, torch.bool, torch.uint8):
        raw = t.numpy().tobytes()
        key = (_dev_index(dev), int(torch.cuda.current_stream(dev).cuda_stream), t.dtype, tuple(t.shape), hash(raw), len(raw))
        hit = _h2d_cache.get(key)
        if hit is not None and hit[0] == raw:
            return hit[1]
    if _pinned_ring is None:
        _pinned_ring = _PinnedRing()
    out = _pinned_ring.stage(t, dev)
    out = out if out is not None else t.to(dev)
    if key is not None:
        if len(_h2d_cache) >= 512:
            _h2d_cache.clear()
        _h2d_cache[key] = (raw, out)
    return out


_H2D_CACHE_ON = os.environ.get("STLLM_H2D_CACHE", "1") != "0"
_h2d_cache = {}


_const_tables = {}


def arange_repeat(n_inner, n_outer, device):
    """int32 [n_outer * n_inner] = (0 .. n_inner-1) repeated n_outer times, resident on the device (a constant table, like the RoPE
    tables: built once per shape)"""
    key = (n_inner, n_outer, str(device))
    t = _const_tables.get(key)
    if t is None:
        t = torch.arange(n_inner, dtype=torch.int32).repeat(n_outer).to(device)
        if len(_const_tables) > 64:
            _const_tables.clear()
        _const_tables[key] = t
    return t


def host_mask(t):
    """the host copy that travels with a device-side attention mask (set by the code that built it on the host), else a D2H read"""
    h = getattr(t, "_stllm_host", None)
    return h if h is not None else t.to("cpu")


def with_host(t_host, device):
    """device copy of a host tensor that remembers where it came from (see host_mask)"""
    d = h2d(t_host, device)
    if d is not t_host:
        d._stllm_host = t_host
    return d


def _req(t, dtype=None, what="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise RuntimeError(f"{what}: last dim must be contiguous")
    return t


_workspaces = {}   # (device index, stream handle) -> workspace
_ws_streams = {}   # (device index, stream handle) -> the torch stream object the workspace belongs to
_ws_probe_host = {}   # (device index, stream handle) -> pinned int32[1], allocated once
_ws_probes = {}    # (device index, stream handle) -> (pinned int32[1], event): the error word as of the previous check
_ERR_WORD_BYTE = 1000 * 4   # kSkErrWord of csrc/gemm_common.h


def _dev_index(device):
    """device ordinal of `device` (None / torch.device("cuda") without an index -> the current device)"""
    if device is None:
        return torch.cuda.current_device()
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def gemm_workspace(device):
    """Scratch of the split-K GEMMs (flags + fp32 partial slabs, 64 MiB), zeroed once at allocation.  The kernels that use it
    assume the launches sharing a workspace are ordered (stllm_hip.h: "private to the launch stream"), so there is ONE PER
    (device, stream): a GEMM issued from a second torch stream — e.g. next to an RCCL collective — gets its own flags and slabs
    instead of racing the first stream's exchanges."""
    dev = _dev_index(device)
    key = (dev, int(torch.cuda.current_stream(dev).cuda_stream))
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.zeros(int(lib().stllm_gemm_workspace_bytes()), dtype=torch.uint8, device=f"cuda:{dev}")
        _workspaces[key] = ws
        _ws_streams[key] = torch.cuda.current_stream(dev)
    return ws


def preprocess_frames(frames_u8, out=None):
    """uint8 RGB frames [T, H, W, 3] on the GPU -> CLIP-normalised f32 [T, 3, 224, 224] (see stllm_hip.h)."""
    _req(frames_u8, torch.uint8, "frames")
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise RuntimeError(f"frames must be uint8 [T, H, W, 3], got {tuple(frames_u8.shape)}")
    f = frames_u8.contiguous()
    T_, H, W, _ = f.shape
    need = int(lib().stllm_preprocess_workspace_bytes(T_, H, W))
    if need < 0:
        raise RuntimeError(f"preprocess_frames: unsupported frame size {H}x{W}")
    ws = torch.empty(need, dtype=torch.uint8, device=f.device)
    if out is None:
        out = torch.empty((T_, 3, 224, 224), dtype=torch.float32, device=f.device)
    _check(lib().stllm_preprocess_frames(_p(f), f.stride(0), T_, H, W, _p(out), _p(ws), need, _stream()), "stllm_preprocess_frames")
    return out


def gemm_plan(M, N, K, heavy=0, tile_rows=192):
    """(q, r, s, cap, est_us) of the phased kernel's schedule (host-only, see stllm_hip.h)."""
    out = (c_int * 5)()
    _check(lib().stllm_gemm_plan(M, N, K, heavy, tile_rows, out), "stllm_gemm_plan")
    return tuple(out)


def gemm_w4_plan(M, N, K, heavy=0, shape=34):
    """(q, r, s, cap, est_us) of the one-wave-per-SIMD kernel's schedule (host-only, see stllm_hip.h)."""
    out = (c_int * 5)()
    _check(lib().stllm_gemm_w4_plan(M, N, K, heavy, shape, out), "stllm_gemm_w4_plan")
    return tuple(out)


def gemm_workspace_ok(device=None):
    """Synchronises and returns True when no split-K GEMM exchange on this device ever timed out (see stllm_hip.h)."""
    dev = _dev_index(device)
    torch.cuda.synchronize(dev)   # device-wide: the workspaces belong to different streams (one per (device, stream))
    ok = True
    for (d, _), ws in list(_workspaces.items()):
        if d == dev:
            ok = ok and int(lib().stllm_gemm_workspace_status(_p(ws), _stream())) == 0
    return ok


def gemm_workspace_check(device=None, wait=False):
    """Raise if a split-K exchange of an earlier GEMM on `device` gave up waiting for a peer workgroup (its output is invalid;
    the kernels poll with a bound instead of hanging the GPU, e.g. when another process keeps some CUs busy).

    wait=True synchronises (end of generate(), of an optimizer step: the host waits there anyway).  wait=False costs no
    synchronisation: it looks at the copy of the error word that the PREVIOUS call enqueued (if that copy has landed) and
    enqueues a fresh one behind the work submitted so far — a forward() that went wrong is reported by the next call."""
    if not torch.cuda.is_available():
        return
    dev = _dev_index(device)
    if wait:
        if not gemm_workspace_ok(dev):
            raise RuntimeError(lib().stllm_last_error().decode())
        return
    for key, ws in list(_workspaces.items()):
        if key[0] != dev:
            continue
        probe = _ws_probes.get(key)
        if probe is not None and probe[1].query():
            if int(probe[0][0]) != 0:
                raise RuntimeError(f"stllm_gemm: a split-K workgroup timed out waiting for a peer (flags {int(probe[0][0]):#x}): the results "
                                   "of that launch — and of everything computed from them — are invalid")
            probe = None
        if probe is None:
            host = _ws_probe_host.get(key)
            if host is None:      # ONE pinned word per workspace for the life of the process: a pin_memory() per check synchronises the device
                host = _ws_probe_host[key] = torch.zeros(1, dtype=torch.int32).pin_memory()
            with torch.cuda.stream(_ws_streams[key]):   # behind the GEMMs of THAT stream, not of whichever stream is current here
                host.copy_(ws[_ERR_WORD_BYTE: _ERR_WORD_BYTE + 4].view(torch.int32), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            _ws_probes[key] = (host, ev)


class GemmProfiler:
    """HIP-event timing of GEMM launches on the launch stream (bench.py roofline leg), kept on the C side (stllm_gemm_profile: the events
    sit inside stllm_gemm, so launches issued by the whole-stack entry points are timed like per-op launches).
    start_all(): time every launch (calibration); start_target(sym): only launches whose kernel symbol == sym; summary() reads the
    session's records (synchronising their events): {symbol: {launches, total_ms, flops}}."""

    def __init__(self):
        self.target = None

    def start_all(self):
        self.target = None
        _check(lib().stllm_gemm_profile(1, None), "stllm_gemm_profile")

    SAMPLE_EVERY = 7   # csrc/profile.cpp kSampleEvery

    def start_target(self, sym, sampled=False):
        """sampled: every 7th launch of `sym` only — an event pair around each of the 78 launches per step of the dominant GEMM symbol costs the
        step 0.5 ms of 23.6 (`bench.py` / `bench.py --no-roofline` alternating on one box: 23.69 / 23.12 / 23.57 / 23.12 / 23.70 / 23.25)"""
        self.target = sym
        _check(lib().stllm_gemm_profile(3 if sampled else 2, sym.encode()), "stllm_gemm_profile")

    def stop(self):
        _check(lib().stllm_gemm_profile(0, None), "stllm_gemm_profile")

    def summary(self):
        L = lib()
        out = {}
        buf = ctypes.create_string_buffer(160)
        ms, fl, mnk = c_float(), ctypes.c_double(), (c_int * 3)()
        for i in range(int(L.stllm_gemm_profile_count())):
            _check(L.stllm_gemm_profile_read(i, buf, 160, ctypes.byref(ms), ctypes.byref(fl), mnk), "stllm_gemm_profile_read")
            e = out.setdefault(buf.value.decode(), dict(launches=0, total_ms=0.0, flops=0.0, shapes={}))
            e["launches"] += 1
            e["total_ms"] += ms.value
            e["flops"] += fl.value
            sh = e["shapes"].setdefault(f"{mnk[0]}x{mnk[1]}x{mnk[2]}", dict(launches=0, total_ms=0.0, flops=0.0))
            sh["launches"] += 1
            sh["total_ms"] += ms.value
            sh["flops"] += fl.value
        return out


def set_profiler(p):
    """kept for callers of the round-1/2 surface: set_profiler(None) stops a session"""
    if p is None:
        GemmProfiler().stop()


# ----------------------------------------------------------------------------------------------
def gemm(a, w, *, dtype, epilogue=EPI_STORE, bias=None, out=None, out_f32=False, act=ACT_NONE, resid=None,
         rope=None, rope_seq=0, rope_cols=0, frames=None, pos_embed=None, n_frames=0, M=None,
         a_rows=None, o_rows=None, a_norm=None, a_presplit=False, out_split=False, w_frag=None):
    """out = epilogue(a @ w.T).  a [M,K] (compute dtype), w [N,K] (compute dtype, maybe padded).
    dtype fp32 with a bf16 weight of 3 K columns (pack.split3_weight: the runtime's "bf16x3" mode) selects STLLM_BF16X3: a and every output
    stay fp32, the product runs as three bf16 matrix-core passes (stllm_hip.h).  In that mode a_presplit = a is ALREADY the split image bf16 [M, 3 K]
    (layernorm / rmsnorm with dtype "bf16x3", split3, or a previous gemm with out_split), out_split (STORE / SWIGLU) = return the split image of the
    result, bf16 [M, 3 N'], instead of the fp32 tensor — what stllm_vit_blocks / stllm_llama_layers chain internally.
    a_norm=(x, gamma, eps) with a=None (decode regime, M <= 8, 16-bit dtypes): the A operand is RMSNorm(x) * gamma of the fp32
    rows x [M,K], computed inside the kernel (stllm_hip.h: a_norm_*)."""
    td = torch_dtype(dtype)
    args = GemmArgs()
    args.dtype, args.epilogue, args.act, args.out_is_f32 = dtype_code(td), epilogue, act, int(out_f32)
    split = td == torch.float32 and w.dtype == torch.bfloat16 and epilogue != EPI_PATCH and a_norm is None
    if split:
        _req(w, torch.bfloat16, "W (bf16x3)")
        args.dtype, out_f32 = BF16X3, True
    else:
        _req(w, td, "W")
    N = w.shape[0]
    if epilogue == EPI_PATCH:
        M, K = n_frames * 256, 588
        _req(frames, torch.float32, "frames"); _req(pos_embed, torch.float32, "pos_embed")
        args.frames, args.aux0 = _p(frames), _p(pos_embed)
        args.A, args.lda = None, 0
    elif a_norm is not None:
        xn, gamma, eps = a_norm
        _req(xn, torch.float32, "a_norm x"); _req(gamma, torch.float32, "a_norm gamma")
        K = xn.shape[-1]
        M = xn.shape[0] if M is None else M
        args.A, args.lda = None, 0
        args.a_norm_x, args.a_norm_ldx, args.a_norm_gamma, args.a_norm_eps = _p(xn), xn.stride(-2), _p(gamma), float(eps)
    else:
        if a_presplit:
            if not split:
                raise RuntimeError("gemm: a_presplit needs the bf16x3 mode (fp32 dtype, split bf16 weight)")
            _req(a, torch.bfloat16, "A (pre-split)")
            K = a.shape[-1] // 3
        else:
            _req(a, td, "A")
            K = a.shape[-1]
        if a_rows is not None:  # (rows_per_batch, batch_stride): 2-level rows inside a larger buffer
            args.a_rows_per_batch, args.a_batch_stride = a_rows
            if M is None:
                raise RuntimeError("gemm: M is required with a_rows")
        elif M is None:
            M = a.shape[0]
        args.A, args.lda = _p(a), a.stride(-2)
    args.W, args.ldw = _p(w), w.stride(0)
    if w_frag is not None:   # pack.frag32(w): the fragment-major copy (W-direct kernel)
        _req(w_frag, td, "w_frag")
        if w_frag.numel() != w.shape[0] * K:
            raise RuntimeError("gemm: w_frag must hold N x K elements (pack.frag32 of the un-padded weight)")
        args.w_frag = _p(w_frag)
    if bias is not None:
        _req(bias, torch.float32, "bias")
    args.bias = _p(bias)
    if epilogue == EPI_RESID:
        _req(resid, torch.float32, "resid")
        out = resid if out is None else out
        _req(out, torch.float32, "out")
        args.resid, args.ldr = _p(resid), resid.stride(-2)
    elif epilogue == EPI_PATCH:
        _req(out, torch.float32, "out")
    else:
        n_out = N // 2 if epilogue == EPI_SWIGLU else N
        if out_split:
            if not split or epilogue not in (EPI_STORE, EPI_SWIGLU):
                raise RuntimeError("gemm: out_split needs the bf16x3 mode and a STORE / SWIGLU epilogue")
            if out is None:
                out = torch.empty((M, 3 * n_out), device=w.device, dtype=torch.bfloat16)
            _req(out, torch.bfloat16, "out (split)")
        else:
            if out is None:
                out = torch.empty((M, n_out), device=w.device, dtype=torch.float32 if out_f32 else td)
            _req(out, torch.float32 if out_f32 else td, "out")
    if epilogue == EPI_ROPE:
        cos, sin = rope
        _req(cos, torch.float32, "rope cos"); _req(sin, torch.float32, "rope sin")
        args.aux0, args.aux1, args.rope_seq, args.rope_cols = _p(cos), _p(sin), rope_seq, rope_cols
    if o_rows is not None:
        args.o_rows_per_batch, args.o_batch_stride = o_rows
    args.out, args.ldo = _p(out), out.stride(-2)
    args.M, args.N, args.K = M, N, K
    if split:
        if w.shape[1] != 3 * K:
            raise RuntimeError(f"gemm(bf16x3): the split weight must have 3 K = {3 * K} columns, got {w.shape[1]}")
        args.split_flags = (1 if a_presplit else 0) | (2 if out_split else 0)
        need = int(lib().stllm_gemm_split_ws_bytes(M, N, K, epilogue, args.split_flags))
        sws = split_workspace(w.device, need)
        args.split_ws, args.split_ws_bytes = _p(sws), sws.numel()
    ws = gemm_workspace(w.device)
    args.workspace, args.workspace_bytes = _p(ws), ws.numel()
    _check(lib().stllm_gemm(ctypes.byref(args), _stream()), "stllm_gemm")
    return out


def _gemv_quant(name, args, wdtype, early, late, a, wq, scale, *, dtype, epilogue, bias, resid, rope, rope_seq, rope_cols, out, out_f32, a_norm, M, a_rows,
                o_rows):
    """what gemv_w8 and gemv_q4 share: the checks of the operands, `args` (a GemvW8Args / GemvQ4Args: same field names) filled in, the call of
    stllm_<name>.  The format's own checks of (wq, scale) run where they always did: early(N) in front of the A operand, late(N, K) behind it."""
    td = torch_dtype(dtype)
    if td not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{name}: 16-bit activations only, got {td}")
    if epilogue not in (EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE):
        raise RuntimeError(f"{name}: epilogue {epilogue} is not STORE / RESID / SWIGLU / ROPE")
    args.dtype, args.epilogue, args.out_is_f32 = dtype_code(td), epilogue, int(out_f32)
    _req(wq, wdtype, "Wq"); _req(scale, torch.float32, "scale")
    N = wq.shape[0]
    early(N)
    if a_norm is not None:
        xn, gamma, eps = a_norm
        _req(xn, torch.float32, "a_norm x"); _req(gamma, torch.float32, "a_norm gamma")
        K = xn.shape[-1]
        M = xn.shape[0] if M is None else M
        args.a_norm_x, args.a_norm_ldx, args.a_norm_gamma, args.a_norm_eps = _p(xn), xn.stride(-2), _p(gamma), float(eps)
    else:
        _req(a, td, "A")
        K = a.shape[-1]
        if a_rows is not None:
            args.a_rows_per_batch, args.a_batch_stride = a_rows
            if M is None:
                raise RuntimeError(f"{name}: M is required with a_rows")
        elif M is None:
            M = a.shape[0]
        args.A, args.lda = _p(a), a.stride(-2)
    late(N, K)
    args.Wq, args.ldw, args.scale = _p(wq), wq.stride(0), _p(scale)
    if bias is not None:
        _req(bias, torch.float32, "bias")
    args.bias = _p(bias)
    if epilogue == EPI_RESID:
        _req(resid, torch.float32, "resid")
        out = resid if out is None else out
        _req(out, torch.float32, "out")
        args.resid, args.ldr = _p(resid), resid.stride(-2)
    else:
        n_out = N // 2 if epilogue == EPI_SWIGLU else N
        odt = torch.float32 if (out_f32 and epilogue == EPI_STORE) else td
        if out is None:
            out = torch.empty((M, n_out), device=wq.device, dtype=odt)
        _req(out, odt, "out")
    if epilogue == EPI_ROPE:
        cos, sin = rope
        _req(cos, torch.float32, "rope cos"); _req(sin, torch.float32, "rope sin")
        args.rope_cos, args.rope_sin, args.rope_seq, args.rope_cols = _p(cos), _p(sin), rope_seq, rope_cols
    if o_rows is not None:
        args.o_rows_per_batch, args.o_batch_stride = o_rows
    args.out, args.ldo = _p(out), out.stride(-2)
    args.M, args.N, args.K = M, N, K
    _check(getattr(lib(), "stllm_" + name)(ctypes.byref(args), _stream()), "stllm_" + name)
    return out


def gemv_w8(a, wq, scale, *, dtype, epilogue=EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    """out = epilogue(scale * (a @ wq.T) + bias) for the decode regime (M <= 16): a [M,K] bf16 / fp16, wq int8 [N,K] (pack.quant8_rows of the
    packed 16-bit weight), scale f32 [N] — stllm_gemv_w8 (stllm_hip.h).  Epilogues STORE / RESID / SWIGLU / ROPE as in gemm; a_norm=(x, gamma, eps)
    with a=None: the fused RMSNorm operand (M <= 2).  A shape no int8 kernel covers raises (nothing else runs in its place)."""
    def early(N):
        if scale.numel() != N or not scale.is_contiguous():
            raise RuntimeError(f"gemv_w8: scale must be a contiguous f32 [{N}]")

    def late(N, K):
        if wq.shape[1] != K:
            raise RuntimeError(f"gemv_w8: Wq has {wq.shape[1]} columns, A has K = {K}")
    return _gemv_quant("gemv_w8", GemvW8Args(), torch.int8, early, late, a, wq, scale, dtype=dtype, epilogue=epilogue, bias=bias, resid=resid, rope=rope,
                       rope_seq=rope_seq, rope_cols=rope_cols, out=out, out_f32=out_f32, a_norm=a_norm, M=M, a_rows=a_rows, o_rows=o_rows)


def gemv_q4(a, qp, scale, *, dtype, epilogue=EPI_STORE, bias=None, resid=None, rope=None, rope_seq=0, rope_cols=0, out=None, out_f32=False,
            a_norm=None, M=None, a_rows=None, o_rows=None):
    """out = epilogue(sum_g scale[:, g] * (a[:, g] @ q[:, g].T) + bias) for the decode regime (M <= 16): a [M,K] bf16 / fp16, (qp uint8 [N,K/2],
    scale f32 [N,K/128]) = pack.quant4_groups of the packed 16-bit weight (q: pack.dequant4_groups) — stllm_gemv_q4 (stllm_hip.h).  The scale is applied
    per 128-element K group to the finished group sum, before bias / residual / SwiGLU / RoPE.  Epilogues, a_norm (M <= 2), a_rows / o_rows as in
    gemv_w8.  A shape no 4-bit kernel covers raises (nothing else runs in its place)."""
    args = GemvQ4Args()

    def late(N, K):
        if qp.shape[1] * 2 != K:
            raise RuntimeError(f"gemv_q4: Wq holds {qp.shape[1] * 2} weights per row, A has K = {K}")
        if scale.dim() != 2 or tuple(scale.shape) != (N, -(-K // 128)):
            raise RuntimeError(f"gemv_q4: scale must be f32 [{N}, {-(-K // 128)}]")
        args.ld_scale = scale.stride(0)
    return _gemv_quant("gemv_q4", args, torch.uint8, lambda N: None, late, a, qp, scale, dtype=dtype, epilogue=epilogue, bias=bias, resid=resid, rope=rope,
                       rope_seq=rope_seq, rope_cols=rope_cols, out=out, out_f32=out_f32, a_norm=a_norm, M=M, a_rows=a_rows, o_rows=o_rows)


def stack_dtype_code(td, w):
    """dtype code of a whole-stack entry point: fp32 activations over split bf16 weights = the bf16x3 mode"""
    return BF16X3 if (td == torch.float32 and w.dtype == torch.bfloat16) else dtype_code(td)


def split3(x, weight_side=False, out=None):
    """x f32 [M, K] -> bf16 [M, 3 K]: (hi | hi | lo) for the A operand, (hi | lo | hi) for a weight (stllm_split3_rows)."""
    _req(x, torch.float32, "x")
    M, K = x.shape
    if out is None:
        out = torch.empty((M, 3 * K), device=x.device, dtype=torch.bfloat16)
    _req(out, torch.bfloat16, "out")
    _check(lib().stllm_split3_rows(_p(x), x.stride(0), 0, 0, _p(out), out.stride(0), M, K, int(bool(weight_side)), _stream()), "stllm_split3_rows")
    return out


_split_ws = {}


def split_workspace(device, nbytes):
    """scratch of the bf16x3 GEMMs (the split A operand; SwiGLU: + the fp32 gate/up columns), one per (device, stream) like the GEMM
    workspace: grows, never shrinks (a replaced buffer stays alive until the launches that use it have run: torch's stream-ordered allocator)"""
    key = str(torch.device(device)) if torch.device(device).type != "cuda" else (_dev_index(device), int(torch.cuda.current_stream(_dev_index(device)).cuda_stream))
    buf = _split_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _split_ws[key] = buf
    return buf


def vit_block_array(blocks):
    """list of Block.pack() dicts -> (ctypes array of stllm_vit_block_weights, the tensors it points into)"""
    arr = (VitBlockWeights * len(blocks))()
    for i, pk in enumerate(blocks):
        w = arr[i]
        w.n1w, w.n1b, w.e1 = pk["n1w"].data_ptr(), pk["n1b"].data_ptr(), float(pk["e1"])
        w.wqkv, w.ld_qkv, w.bqkv = pk["wqkv"].data_ptr(), pk["wqkv"].stride(0), pk["bqkv"].data_ptr()
        w.wproj, w.ld_proj, w.bproj = pk["wproj"].data_ptr(), pk["wproj"].stride(0), pk["bproj"].data_ptr()
        w.n2w, w.n2b, w.e2 = pk["n2w"].data_ptr(), pk["n2b"].data_ptr(), float(pk["e2"])
        w.wfc1, w.ld_fc1, w.bfc1 = pk["wfc1"].data_ptr(), pk["wfc1"].stride(0), pk["bfc1"].data_ptr()
        w.wfc2, w.ld_fc2, w.bfc2 = pk["wfc2"].data_ptr(), pk["wfc2"].stride(0), pk["bfc2"].data_ptr()
    return arr


def vit_blocks(x, blocks, carr, *, n_seq, seq_len, num_heads, dtype):
    """All ViT blocks of `blocks` (Block.pack() dicts; carr = vit_block_array(blocks), cached by the caller next to them) on the flat
    fp32 stream x [n_seq * seq_len, dim], in place — ONE C call (stllm_vit_blocks)."""
    _req(x, torch.float32, "x")
    td = torch_dtype(dtype)
    dim, hidden = x.shape[1], blocks[0]["wfc1"].shape[0]
    L = lib()
    code = stack_dtype_code(td, blocks[0]["wfc1"])
    need = int(L.stllm_vit_blocks_scratch_bytes(code, n_seq, seq_len, dim, hidden))
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    ws = gemm_workspace(x.device)
    a = VitBlocksArgs(code, n_seq, seq_len, num_heads, dim, hidden, x.data_ptr(), x.stride(0), scratch.data_ptr(), need,
                      ws.data_ptr(), ws.numel())
    _check(L.stllm_vit_blocks(ctypes.byref(a), carr, len(blocks), _stream()), "stllm_vit_blocks")
    return x


def llama_layer_array(layers, cache=None):
    arr = (LlamaLayerWeights * len(layers))()
    for i, pk in enumerate(layers):
        w = arr[i]
        w.ln1, w.wqkv, w.ld_qkv = pk["ln1"].data_ptr(), pk["wqkv"].data_ptr(), pk["wqkv"].stride(0)
        w.wo, w.ld_o, w.ln2 = pk["wo"].data_ptr(), pk["wo"].stride(0), pk["ln2"].data_ptr()
        w.wgu, w.ld_gu = pk["wgu"].data_ptr(), pk["wgu"].stride(0)
        w.wdown, w.ld_down = pk["wdown"].data_ptr(), pk["wdown"].stride(0)
        w.kv_cache = cache.qkv[i].data_ptr() if cache is not None else None
        w.wqkv_frag = pk["wqkv_frag"].data_ptr() if pk.get("wqkv_frag") is not None else None   # pack.frag32 copies (W-direct GEMM, 16-bit dtypes)
        w.wgu_frag = pk["wgu_frag"].data_ptr() if pk.get("wgu_frag") is not None else None
    return arr


def lora_pad(r, dtype):
    """P: the 2 r adapter columns rounded up to the K granularity of the GEMMs (one 128-byte panel: 64 columns in 16 bits, 32 in fp32)"""
    panel = 32 if torch_dtype(dtype) == torch.float32 else 64
    return (2 * r + panel - 1) // panel * panel


def lora_down(x, A, *, dtype, out, M=None):
    """out[M, n_pad] = x[M, K] @ A[n, K].T in the compute dtype, columns [n, n_pad) zeroed (stllm_lora_down; deterministic split-K).  x and out are
    2-D views with unit column stride — in the model both are column ranges of one [M, K + n_pad] row buffer."""
    td = torch_dtype(dtype)
    _req(x, td, "x"); _req(A, td, "A"); _req(out, td, "out")
    M = x.shape[0] if M is None else M
    K, n, n_pad = x.shape[1], A.shape[0], out.shape[1]
    if A.shape[1] != K or x.stride(1) != 1 or out.stride(1) != 1 or A.stride(1) != 1 or out.shape[0] < M:
        raise RuntimeError(f"lora_down: x {tuple(x.shape)}, A {tuple(A.shape)}, out {tuple(out.shape)}")
    L = lib()
    code = dtype_code(td)
    need = int(L.stllm_lora_down_workspace_bytes(code, M, K, n_pad))
    if need < 0:
        raise RuntimeError(f"lora_down: unsupported shape (M={M}, K={K}, n_pad={n_pad})")
    ws = split_workspace(x.device, need) if need else None
    _check(L.stllm_lora_down(code, _p(x), x.stride(0), _p(A), A.stride(0), _p(out), out.stride(0), M, K, n, n_pad, _p(ws), need, _stream()), "stllm_lora_down")
    return out


def llama_lora_array(layers):
    """list of LlamaDecoderLayer.pack() dicts with active adapters -> ctypes array of stllm_llama_lora_layer (pk["wqkv"] IS the extended weight)"""
    arr = (LlamaLoraLayer * len(layers))()
    for i, pk in enumerate(layers):
        w = arr[i]
        w.A, w.ld_a = pk["lora_A"].data_ptr(), pk["lora_A"].stride(0)
        w.wqkv_ext, w.ld_ext = pk["wqkv"].data_ptr(), pk["wqkv"].stride(0)
        w.r, w.P = pk["lora_r"], pk["lora_P"]
    return arr


def llama_layers(x, layers, carr, *, B, S, n_heads, eps, rope, dtype, kv_len=None, cache=None, lora=None):
    """All decoder layers of the PREFILL on the flat fp32 stream x [B * S, hidden], in place — ONE C call (stllm_llama_layers).
    carr = llama_layer_array(layers, cache).  lora = llama_lora_array(layers): the stack with active adapters (stllm_llama_layers_lora)."""
    _req(x, torch.float32, "x")
    td = torch_dtype(dtype)
    hidden, inter = x.shape[1], layers[0]["wgu"].shape[0] // 2
    L = lib()
    code = stack_dtype_code(td, layers[0]["wdown"])
    if lora is not None:
        need = int(L.stllm_llama_layers_lora_scratch_bytes(code, B, S, hidden, inter, layers[0]["lora_P"]))
        if need < 0:
            raise RuntimeError("stllm_llama_layers_lora: bad shape / dtype (bf16x3 runs merged adapters only)")
    else:
        need = int(L.stllm_llama_layers_scratch_bytes(code, B, S, hidden, inter))
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    ws = gemm_workspace(x.device)
    cos, sin = rope
    _req(cos, torch.float32, "rope cos"); _req(sin, torch.float32, "rope sin")
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len")
    a = LlamaLayersArgs(code, B, S, n_heads, hidden, inter, float(eps), x.data_ptr(), x.stride(0), cos.data_ptr(), sin.data_ptr(),
                        _p(kv_len), cache.max_len if cache is not None else 0, scratch.data_ptr(), need, ws.data_ptr(), ws.numel())
    if lora is not None:
        _check(L.stllm_llama_layers_lora(ctypes.byref(a), carr, lora, len(layers), _stream()), "stllm_llama_layers_lora")
        return x
    _check(L.stllm_llama_layers(ctypes.byref(a), carr, len(layers), _stream()), "stllm_llama_layers")
    return x


def llama_layers_extend(x, layers, carr, *, B, S, pos0, n_heads, eps, rope, dtype, cache):
    """All decoder layers for S new positions behind the pos0 positions `cache` already holds, on the flat fp32 stream x [B * S, hidden], in place — ONE C call
    (stllm_llama_layers_extend).  carr = llama_layer_array(layers, cache); rope = (cos, sin) rows of the positions pos0 .. pos0 + S - 1."""
    _req(x, torch.float32, "x")
    td = torch_dtype(dtype)
    hidden, inter = x.shape[1], layers[0]["wgu"].shape[0] // 2
    L = lib()
    code = dtype_code(td)
    need = int(L.stllm_llama_layers_scratch_bytes(code, B, S, hidden, inter))
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    ws = gemm_workspace(x.device)
    cos, sin = rope
    _req(cos, torch.float32, "rope cos"); _req(sin, torch.float32, "rope sin")
    aws = attention_offset_workspace(B, n_heads, S, pos0 + S, x.device) if td != torch.float32 and hidden // n_heads == 128 else None
    a = LlamaLayersArgs(code, B, S, n_heads, hidden, inter, float(eps), x.data_ptr(), x.stride(0), cos.data_ptr(), sin.data_ptr(),
                        None, cache.max_len, scratch.data_ptr(), need, ws.data_ptr(), ws.numel())
    _check(L.stllm_llama_layers_extend(ctypes.byref(a), carr, len(layers), pos0, _p(aws), aws.numel() if aws is not None else 0, _stream()),
           "stllm_llama_layers_extend")
    return x


def llama_layer_sp(x, carr, li, qkv, *, s0, s1, part, n_heads, eps, rope, dtype, inter):
    """ONE decoder layer of the sequence-parallel prefill, part 0 (RMSNorm + QKV GEMM + RoPE into rows [s0, s1) of `qkv`) or part 1 (attention over the s1
    rows, o_proj, RMSNorm, gate/up, down) — one C call each (stllm_llama_layer_sp).  x f32 [s1 - s0, hidden] in place; carr = llama_layer_array(layers);
    rope = (cos, sin) rows of THIS rank's positions (the tables offset by s0)."""
    _req(x, torch.float32, "x")
    td = torch_dtype(dtype)
    _req(qkv, td, "qkv")
    hidden = x.shape[1]
    L = lib()
    code = dtype_code(td)
    need = int(L.stllm_llama_layer_sp_scratch_bytes(code, s0, s1, hidden, inter))
    if need < 0:
        raise RuntimeError("stllm_llama_layer_sp: bad shape / dtype")
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    ws = gemm_workspace(x.device)
    cos, sin = rope
    _req(cos, torch.float32, "rope cos"); _req(sin, torch.float32, "rope sin")
    a = LlamaLayersArgs(code, 1, s1 - s0, n_heads, hidden, inter, float(eps), x.data_ptr(), x.stride(0), cos.data_ptr(), sin.data_ptr(),
                        None, 0, scratch.data_ptr(), need, ws.data_ptr(), ws.numel())
    _check(L.stllm_llama_layer_sp(ctypes.byref(a), ctypes.byref(carr[li]), qkv.data_ptr(), s0, s1, part, _stream()), "stllm_llama_layer_sp")
    return x


def _bert_out(dst, o):
    dst.w, dst.ldw, dst.b = o["w"].data_ptr(), o["w"].stride(0), o["b"].data_ptr()
    dst.g, dst.beta, dst.eps = o["g"].data_ptr(), o["beta"].data_ptr(), float(o["eps"])


def qformer_layer_array(layers):
    """list of BertLayer.pack() dicts -> ctypes array of stllm_qformer_layer_weights (the caller keeps `layers` alive next to it)"""
    arr = (QformerLayerWeights * len(layers))()
    for i, pk in enumerate(layers):
        w = arr[i]
        w.wqkv, w.ld_qkv, w.bqkv = pk["wqkv"].data_ptr(), pk["wqkv"].stride(0), pk["bqkv"].data_ptr()
        _bert_out(w.attn_out, pk["attn_out"])
        w.has_cross = int("cq_w" in pk)
        if w.has_cross:
            w.ckv_index = pk["ckv_all"][2]
            w.cq_w, w.ld_cq, w.cq_b = pk["cq_w"].data_ptr(), pk["cq_w"].stride(0), pk["cq_b"].data_ptr()
            _bert_out(w.cross_out, pk["cross_out"])
        f = pk["ffn_q"]
        w.fq_w1, w.ld_fq1, w.fq_b1 = f["w1"].data_ptr(), f["w1"].stride(0), f["b1"].data_ptr()
        _bert_out(w.fq_out, f["out"])
        f = pk.get("ffn_t")
        if f is not None:
            w.ft_w1, w.ld_ft1, w.ft_b1 = f["w1"].data_ptr(), f["w1"].stride(0), f["b1"].data_ptr()
            _bert_out(w.ft_out, f["out"])
    return arr


def qformer_layers(hq32, hq16, ht32, ht16, enc16, layers, carr, *, n_seq, n_query, n_text, n_heads, dtype, kv_len=None):
    """All Q-Former layers of `layers` (BertLayer.pack() dicts; carr = qformer_layer_array(layers)) on the embedded query rows hq32 / hq16
    [n_seq * n_query, C] and text rows ht32 / ht16 [n_seq * n_text, C] (None without text), in place — ONE C call (stllm_qformer_layers).
    enc16: the ln_vision'd image tokens, compute dtype [n_seq * P, 1408]."""
    _req(hq32, torch.float32, "hq32")
    td = torch_dtype(dtype)
    C, inter = hq32.shape[1], layers[0]["ffn_q"]["w1"].shape[0]
    cross = [pk for pk in layers if "cq_w" in pk]
    w_all = b_all = None
    n_cross = P = enc_dim = 0
    if cross:
        w_all, b_all, _, n_cross = cross[0]["ckv_all"]
        P, enc_dim = enc16.shape[0] // n_seq, enc16.shape[1]
    L = lib()
    code = stack_dtype_code(td, layers[0]["ffn_q"]["w1"])
    _req(hq16, td, "hq16"); _req(enc16, td, "enc16") if cross else None
    if n_text:
        _req(ht32, torch.float32, "ht32"); _req(ht16, td, "ht16")
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len")
    need = int(L.stllm_qformer_layers_scratch_bytes(code, n_seq, n_query, n_text, C, inter, P, enc_dim, n_cross))
    if need < 0:
        raise RuntimeError("stllm_qformer_layers_scratch_bytes: bad shape")
    scratch = torch.empty(need, dtype=torch.uint8, device=hq32.device)
    ws = gemm_workspace(hq32.device)
    a = QformerLayersArgs(code, n_seq, n_query, n_text, n_heads, C, inter, P, enc_dim, n_cross, hq32.data_ptr(), hq16.data_ptr(),
                          _p(ht32) if n_text else None, _p(ht16) if n_text else None, _p(enc16) if cross else None,
                          enc16.stride(0) if cross else 0, _p(w_all), w_all.stride(0) if cross else 0, _p(b_all), _p(kv_len),
                          scratch.data_ptr(), need, ws.data_ptr(), ws.numel())
    _check(L.stllm_qformer_layers(ctypes.byref(a), carr, len(layers), _stream()), "stllm_qformer_layers")
    return hq32, hq16, ht32


def _norm_dtype(dtype, D):
    """(C dtype code, torch dtype of out_t, columns of out_t): dtype "bf16x3" = the split image bf16 [M, 3 D] (stllm_hip.h)"""
    if isinstance(dtype, str) and dtype in ("bf16x3", "split"):
        return BF16X3, torch.bfloat16, 3 * D
    td = torch_dtype(dtype)
    return dtype_code(td), td, D


def layernorm(x, gamma, beta, eps, *, dtype, out_t=None, out_f32=None, want_t=True, want_f32=False):
    """x f32 [M,D] -> (out_t compute-dtype [M,D] | None, out_f32 | None)."""
    _req(x, torch.float32, "x")
    M, D = x.shape
    code, td, wt = _norm_dtype(dtype, D)
    if want_t and out_t is None:
        out_t = torch.empty((M, wt), device=x.device, dtype=td)
    if want_f32 and out_f32 is None:
        out_f32 = torch.empty((M, D), device=x.device, dtype=torch.float32)
    _check(lib().stllm_layernorm(code, _p(x), x.stride(0), _p(gamma), _p(beta), eps,
                                 _p(out_t), out_t.stride(0) if out_t is not None else 0,
                                 _p(out_f32), out_f32.stride(0) if out_f32 is not None else 0, M, D, _stream()),
           "stllm_layernorm")
    return out_t, out_f32


def rmsnorm(x, gamma, eps, *, dtype, out_t=None, out_f32=None, want_t=True, want_f32=False):
    _req(x, torch.float32, "x")
    M, D = x.shape
    code, td, wt = _norm_dtype(dtype, D)
    if want_t and out_t is None:
        out_t = torch.empty((M, wt), device=x.device, dtype=td)
    if want_f32 and out_f32 is None:
        out_f32 = torch.empty((M, D), device=x.device, dtype=torch.float32)
    _check(lib().stllm_rmsnorm(code, _p(x), x.stride(0), _p(gamma), eps,
                               _p(out_t), out_t.stride(0) if out_t is not None else 0,
                               _p(out_f32), out_f32.stride(0) if out_f32 is not None else 0, M, D, _stream()),
           "stllm_rmsnorm")
    return out_t, out_f32


_decode_attn = True   # tests flip this to compare the split-KV decode kernel with the tile kernels


def attention_offset_workspace(B, H, Sq, Skv, device):
    """the partial-state buffer of stllm_attention_offset's key-split kernels (no initialisation needed)"""
    need = int(lib().stllm_attention_offset_workspace_bytes(B, H, Sq, Skv))
    if need < 0:
        raise RuntimeError(f"stllm_attention_offset_workspace_bytes: bad shape (B={B}, H={H}, Sq={Sq}, Skv={Skv})")
    return torch.empty(need, dtype=torch.uint8, device=device)


def attention(q, k, v, *, B, H, Sq, Skv, D, scale, causal=False, kv_len=None, out=None,
              q_strides=None, k_strides=None, v_strides=None, q_off=0):
    """q/k/v: 2-D views [B*S, >=H*D] of the compute dtype (may be column slices of a fused QKV buffer).
    *_strides = (batch_stride, row_stride) in elements; default: rows of one batch are consecutive.
    q_off > 0 (stllm_attention_offset): query row i sits at position q_off + i — with `causal`, key j is visible iff j <= q_off + i (q_off + Sq <= Skv);
    q_off = 0 is the call it always was.  Sq = 1 with a kv_len (a ragged KV cache: row b attends keys [0, kv_len[b]), Skv their upper bound) runs the ragged
    decode kernels in bf16 / fp16 at D = 128 (attention_decode_ragged); fp32 keeps stllm_attention's kv_len route."""
    td = q.dtype
    if q_off:
        qs = q_strides if q_strides is not None else (Sq * q.stride(0), q.stride(0))
        ks = k_strides if k_strides is not None else (Skv * k.stride(0), k.stride(0))
        vs = v_strides if v_strides is not None else (Skv * v.stride(0), v.stride(0))
        if out is None:
            out = torch.empty((B * Sq, H * D), device=q.device, dtype=td)
        if kv_len is not None:
            _req(kv_len, torch.int32, "kv_len")
        ws = attention_offset_workspace(B, H, Sq, Skv, q.device) if td != torch.float32 and D == 128 else None
        _check(lib().stllm_attention_offset(dtype_code(td), _p(q), qs[0], qs[1], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1],
                                            _p(out), Sq * out.stride(0), out.stride(0), B, H, Sq, Skv, D, scale, int(causal),
                                            _p(kv_len), int(q_off), _p(ws), ws.numel() if ws is not None else 0, _stream()), "stllm_attention_offset")
        return out

    def st(t, S, given):
        return given if given is not None else (S * t.stride(0), t.stride(0))
    qs, ks, vs = st(q, Sq, q_strides), st(k, Skv, k_strides), st(v, Skv, v_strides)
    if out is None:
        out = torch.empty((B * Sq, H * D), device=q.device, dtype=td)
    if Sq == 1 and D == 128 and kv_len is None and td in (torch.bfloat16, torch.float16) and _decode_attn:
        need = int(lib().stllm_attention_decode_workspace_bytes(B, H, Skv))   # one-token decode: keys split over workgroups
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        _check(lib().stllm_attention_decode(dtype_code(td), _p(q), qs[0], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1], _p(out),
                                            out.stride(0), B, H, Skv, D, scale, _p(ws), need, _stream()), "stllm_attention_decode")
        return out
    if Sq == 1 and D == 128 and kv_len is not None and td in (torch.bfloat16, torch.float16) and _decode_attn:
        return attention_decode_ragged(q, k, v, kv_len, B=B, H=H, max_kv=Skv, D=D, scale=scale, out=out, q_stride=qs[0], k_strides=ks, v_strides=vs)
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len")
    _check(lib().stllm_attention(dtype_code(td), _p(q), qs[0], qs[1], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1],
                                 _p(out), Sq * out.stride(0), out.stride(0), B, H, Sq, Skv, D, scale, int(causal),
                                 _p(kv_len), _stream()), "stllm_attention")
    return out


def attention_decode_ragged(q, k, v, kv_len, *, B, H, max_kv, D, scale, out=None, q_stride=None, k_strides=None, v_strides=None):
    """stllm_attention_decode_ragged: one query row per batch entry against a KV cache whose rows have their own lengths.  q: [B, >= H*D] (row stride
    q_stride), k / v: 2-D views with (batch_stride, row_stride) in elements, kv_len: int32 [B] on the device, max_kv: the host-known bound of the lengths.
    bf16 / fp16 at D = 128; anything else is an error (STLLM_ERR_UNSUPPORTED), not a fallback."""
    td = q.dtype
    _req(kv_len, torch.int32, "kv_len")
    if kv_len.numel() != B:
        raise RuntimeError(f"attention_decode_ragged: kv_len has {kv_len.numel()} entries for B = {B}")
    ks = k_strides if k_strides is not None else (max_kv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (max_kv * v.stride(0), v.stride(0))
    if out is None:
        out = torch.empty((B, H * D), device=q.device, dtype=td)
    need = int(lib().stllm_attention_decode_ragged_workspace_bytes(B, H, max_kv))
    if need < 0:
        raise RuntimeError(f"stllm_attention_decode_ragged_workspace_bytes: bad shape (B={B}, H={H}, max_kv={max_kv})")
    ws = torch.empty(need, dtype=torch.uint8, device=q.device)
    _check(lib().stllm_attention_decode_ragged(dtype_code(td), _p(q), q.stride(0) if q_stride is None else q_stride, _p(k), ks[0], ks[1], _p(v), vs[0], vs[1],
                                               _p(out), out.stride(0), B, H, _p(kv_len), max_kv, D, scale, _p(ws), need, _stream()),
           "stllm_attention_decode_ragged")
    return out


def ragged_extend_available(device):
    """attention_offset_ragged and kv_append_spans can serve tensors on `device`: a device check, nothing more — lib() binds strictly, so a library that
    loads has both entry points.  LlamaModel.extend asks before it takes its ragged path, so that tensors off the device get the NotImplementedError the
    call always raised, before anything is written; a stand-in for this module that states the two contracts answers for itself."""
    return torch.device(device).type == "cuda"


def attention_offset_ragged(q, k, v, q_off, kv_len, *, B, H, Sq, max_kv, D, scale, out=None, q_strides=None, k_strides=None, v_strides=None):
    """stllm_attention_offset_ragged: up to Sq new query rows per batch row, each batch row behind its own number of cached positions (always causal).
    q_off, kv_len: int32 [B] on the device — row b holds q_off[b] cached positions and n_b = kv_len[b] - q_off[b] (0 .. Sq) new ones, max_kv is the host-known
    bound of kv_len; query row i < n_b sees key j iff j <= q_off[b] + i, the pad rows i >= n_b come out as zeros, K / V at or behind kv_len[b] are never read.
    q / k / v: 2-D views with (batch, row) strides in elements, as for attention(q_off=), whose workspace pool this shares.  bf16 / fp16 / fp32 at D = 128
    (fp32: max_kv <= 2048); anything else is an error (STLLM_ERR_UNSUPPORTED), not a fallback."""
    td = q.dtype
    _req(q_off, torch.int32, "q_off"); _req(kv_len, torch.int32, "kv_len")
    if q_off.numel() != B or kv_len.numel() != B:
        raise RuntimeError(f"attention_offset_ragged: q_off / kv_len have {q_off.numel()} / {kv_len.numel()} entries for B = {B}")
    qs = q_strides if q_strides is not None else (Sq * q.stride(0), q.stride(0))
    ks = k_strides if k_strides is not None else (max_kv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (max_kv * v.stride(0), v.stride(0))
    if out is None:
        out = torch.empty((B * Sq, H * D), device=q.device, dtype=td)
    ws = attention_offset_workspace(B, H, Sq, max_kv, q.device) if td != torch.float32 and D == 128 else None
    _check(lib().stllm_attention_offset_ragged(dtype_code(td), _p(q), qs[0], qs[1], _p(k), ks[0], ks[1], _p(v), vs[0], vs[1],
                                               _p(out), Sq * out.stride(0), out.stride(0), B, H, Sq, max_kv, D, scale, _p(q_off), _p(kv_len),
                                               _p(ws), ws.numel() if ws is not None else 0, _stream()), "stllm_attention_offset_ragged")
    return out


def segments_available(device):
    """attention_segments and kv_append_segments can serve tensors on `device`: a device check, nothing more (as ragged_extend_available).
    LlamaModel.step_segments asks before anything is written; a stand-in for this module that states the two contracts answers for itself."""
    return torch.device(device).type == "cuda"


def attention_segments(q, k, v, slot, row0, q_off, kv_len, *, H, D, T, n_slots, max_n, max_kv, scale, out=None, k_strides=None, v_strides=None):
    """stllm_attention_segments: causal attention for R segments of a PACKED query buffer.  q: 2-D view of T packed rows (row stride q.stride(0)); k / v: 2-D
    views of a cache of n_slots rows with (cache row, position) strides in elements; slot, row0, q_off, kv_len: int32 [R] on the device — segment r reads
    cache row slot[r], owns the packed rows row0[r] .. row0[r] + n_r - 1 (n_r = kv_len[r] - q_off[r] <= max_n) and sits behind q_off[r] cached positions;
    max_kv is the host-known bound of kv_len.  Only the packed rows of the segments are written (out: [T, H * D]); a segment whose tables point outside
    the buffers does nothing.  bf16 / fp16 / fp32 at D = 128 (fp32: max_kv <= 2048); anything else is an error (STLLM_ERR_UNSUPPORTED), not a fallback."""
    td = q.dtype
    R = slot.numel()
    for t, what in ((slot, "slot"), (row0, "row0"), (q_off, "q_off"), (kv_len, "kv_len")):
        _req(t, torch.int32, what)
        if t.numel() != R:
            raise RuntimeError(f"attention_segments: {what} has {t.numel()} entries for R = {R}")
    if q.shape[0] < T or (out is not None and out.shape[0] < T):
        raise RuntimeError(f"attention_segments: q {tuple(q.shape)} / out {None if out is None else tuple(out.shape)} hold fewer than T = {T} rows")
    ks = k_strides if k_strides is not None else (max_kv * k.stride(0), k.stride(0))
    vs = v_strides if v_strides is not None else (max_kv * v.stride(0), v.stride(0))
    if out is None:
        out = torch.empty((T, H * D), device=q.device, dtype=td)
    ws = attention_offset_workspace(R, H, max_n, max_kv, q.device) if td != torch.float32 and D == 128 else None
    _check(lib().stllm_attention_segments(dtype_code(td), _p(q), q.stride(0), _p(k), ks[0], ks[1], _p(v), vs[0], vs[1], _p(out), out.stride(0),
                                          R, H, D, T, n_slots, max_n, max_kv, scale, _p(slot), _p(row0), _p(q_off), _p(kv_len),
                                          _p(ws), ws.numel() if ws is not None else 0, _stream()), "stllm_attention_segments")
    return out


def segments_shared_available(device):
    """attention_segments_shared (and kv_append_segments) can serve tensors on `device`: a device check, nothing more (as segments_available).
    LlamaModel.step_segments asks before anything is written on a cache with a base; a stand-in for this module that states the contract answers for itself."""
    return torch.device(device).type == "cuda"


def attention_segments_shared(q, kp, vp, ks, vs, slot, row0, sfx_off, sfx_len, *, H, D, T, P, n_slots, max_n, max_sfx, scale, out=None, kp_strides=None,
                              ks_strides=None):
    """stllm_attention_segments_shared: attention_segments for segments that all sit behind the same P prefix keys.  q: 2-D view of T packed rows; kp / vp: 2-D
    views of the ONE base row (kp_strides: its (batch, row) strides, of which only the row stride is used; never written); ks / vs: 2-D views of the slot
    buffers, ks_strides their (slot, row) strides; slot, row0, sfx_off, sfx_len: int32 [R] on the device in SUFFIX-LOCAL positions — segment r holds
    sfx_off[r] suffix positions and n_r = sfx_len[r] - sfx_off[r] (<= max_n) new ones; its row i sees the P prefix keys and the suffix keys
    j <= sfx_off[r] + i.  Only the packed rows of live segments are written (out: [T, H * D]).  bf16 / fp16 / fp32 at D = 128; anything else is an error
    (STLLM_ERR_UNSUPPORTED), not a fallback.  The record workspace comes from the per-(device, stream) scratch cache (split_workspace)."""
    td = q.dtype
    R = slot.numel()
    for t, what in ((slot, "slot"), (row0, "row0"), (sfx_off, "sfx_off"), (sfx_len, "sfx_len")):
        _req(t, torch.int32, what)
        if t.numel() != R:
            raise RuntimeError(f"attention_segments_shared: {what} has {t.numel()} entries for R = {R}")
    if q.shape[0] < T or (out is not None and out.shape[0] < T):
        raise RuntimeError(f"attention_segments_shared: q {tuple(q.shape)} / out {None if out is None else tuple(out.shape)} hold fewer than T = {T} rows")
    kps = kp_strides if kp_strides is not None else (P * kp.stride(0), kp.stride(0))
    kss = ks_strides if ks_strides is not None else (max_sfx * ks.stride(0), ks.stride(0))
    if out is None:
        out = torch.empty((T, H * D), device=q.device, dtype=td)
    need = int(lib().stllm_attention_segments_shared_workspace_bytes(R, H, T, P, max_n, max_sfx))
    if need < 0:
        raise RuntimeError(f"stllm_attention_segments_shared_workspace_bytes: bad shape (R={R}, H={H}, T={T}, P={P}, max_n={max_n}, max_sfx={max_sfx})")
    ws = split_workspace(q.device, need) if td != torch.float32 else None
    _check(lib().stllm_attention_segments_shared(dtype_code(td), _p(q), q.stride(0), _p(kp), kps[1], _p(vp), kps[1], P, _p(ks), kss[0], kss[1],
                                                 _p(vs), kss[0], kss[1], _p(out), out.stride(0), R, H, D, T, n_slots, max_n, max_sfx, scale,
                                                 _p(slot), _p(row0), _p(sfx_off), _p(sfx_len), _p(ws), ws.numel() if ws is not None else 0, _stream()),
           "stllm_attention_segments_shared")
    return out


def attention_shared(q, kp, vp, ks, vs, *, B, G, H, Sq, P, D, scale, max_sfx, sfx_len=None, sfx_q_off=0, causal=False, out=None,
                     q_strides=None, kp_strides=None, ks_strides=None):
    """stllm_attention_shared: B = G * R query rows, the R rows of group g read the P keys of prefix row g ONCE (kp / vp: 2-D views of the prefix buffer,
    (batch, row) strides kp_strides, never written) and each row b its own suffix keys [0, min(sfx_len[b], max_sfx)) (ks / vs, strides ks_strides);
    with `causal` suffix key j is visible to query row i iff j <= sfx_q_off + i.  sfx_len: int32 [B] on the device or None (max_sfx keys in every row).
    q: 2-D view, (batch, row) strides q_strides (default: Sq consecutive rows per batch entry).  bf16 / fp16 / fp32 at D = 128; anything else is an
    error (STLLM_ERR_UNSUPPORTED), not a fallback.  The partial-state workspace comes from the per-(device, stream) scratch cache (split_workspace)."""
    td = q.dtype
    if sfx_len is not None:
        _req(sfx_len, torch.int32, "sfx_len")
        if sfx_len.numel() != B:
            raise RuntimeError(f"attention_shared: sfx_len has {sfx_len.numel()} entries for B = {B}")
    qs = q_strides if q_strides is not None else (Sq * q.stride(0), q.stride(0))
    kps = kp_strides if kp_strides is not None else (P * kp.stride(0), kp.stride(0))
    kss = ks_strides if ks_strides is not None else (max_sfx * ks.stride(0), ks.stride(0))
    if out is None:
        out = torch.empty((B * Sq, H * D), device=q.device, dtype=td)
    need = int(lib().stllm_attention_shared_workspace_bytes(B, G, H, Sq, P, max_sfx))
    if need < 0:
        raise RuntimeError(f"stllm_attention_shared_workspace_bytes: bad shape (B={B}, G={G}, H={H}, Sq={Sq}, P={P}, max_sfx={max_sfx})")
    ws = split_workspace(q.device, need) if td != torch.float32 else None
    _check(lib().stllm_attention_shared(dtype_code(td), _p(q), qs[0], qs[1], _p(kp), kps[0], kps[1], _p(vp), kps[0], kps[1], P,
                                        _p(ks), kss[0], kss[1], _p(vs), kss[0], kss[1], _p(sfx_len), max_sfx, int(sfx_q_off),
                                        _p(out), Sq * out.stride(0), out.stride(0), B, G, H, Sq, D, scale, int(causal),
                                        _p(ws), ws.numel() if ws is not None else 0, _stream()), "stllm_attention_shared")
    return out


def kv_append_rows(src, cache, pos, *, with_q=False):
    """stllm_kv_append_rows: cache[b, pos[b], cols] = src[b, cols] for the [k | v] columns (with_q: all of [q | k | v]) of the dense fused rows src [B, 3*hidden];
    cache: [B, max_len, 3*hidden], pos: int32 [B] on the device (outside [0, max_len): a free slot, nothing written).  All compute dtypes."""
    _req(src, cache.dtype, "src"); _req(pos, torch.int32, "pos")
    B, max_len, D3 = cache.shape
    if src.shape != (B, D3) or pos.numel() != B or cache.stride(2) != 1:
        raise RuntimeError(f"kv_append_rows: src {tuple(src.shape)}, cache {tuple(cache.shape)}, pos {tuple(pos.shape)}")
    _check(lib().stllm_kv_append_rows(dtype_code(cache.dtype), _p(src), src.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos), B, D3 // 3, max_len,
                                      int(with_q), _stream()), "stllm_kv_append_rows")
    return cache


def kv_append_spans(src, cache, pos0, n, *, S):
    """stllm_kv_append_spans: cache[b, pos0[b] + i, cols] = src[b * S + i, cols] for i < min(n[b], S) and the [k | v] columns of the dense fused rows
    src [B * S, 3*hidden]; cache: [B, max_len, 3*hidden], pos0 / n: int32 [B] on the device.  Pad rows, rows with n[b] = 0 and positions outside
    [0, max_len) write nothing.  All compute dtypes."""
    _req(src, cache.dtype, "src"); _req(pos0, torch.int32, "pos0"); _req(n, torch.int32, "n")
    B, max_len, D3 = cache.shape
    if src.shape != (B * S, D3) or pos0.numel() != B or n.numel() != B or cache.stride(2) != 1:
        raise RuntimeError(f"kv_append_spans: src {tuple(src.shape)}, cache {tuple(cache.shape)}, pos0 {tuple(pos0.shape)}, n {tuple(n.shape)}, S {S}")
    _check(lib().stllm_kv_append_spans(dtype_code(cache.dtype), _p(src), src.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(pos0), _p(n), B, S,
                                       D3 // 3, max_len, _stream()), "stllm_kv_append_spans")
    return cache


def kv_append_segments(src, cache, slot, row0, pos0, n, *, T, max_n):
    """stllm_kv_append_segments: cache[slot[r], pos0[r] + i, cols] = src[row0[r] + i, cols] for i < n[r] (<= max_n) and the [k | v] columns of the packed
    fused rows src [>= T, 3*hidden]; cache: [n_slots, max_len, 3*hidden]; slot, row0, pos0, n: int32 [R] on the device.  Segments whose tables point outside
    the buffers and positions outside [0, max_len) write nothing.  All compute dtypes."""
    _req(src, cache.dtype, "src")
    R = slot.numel()
    for t, what in ((slot, "slot"), (row0, "row0"), (pos0, "pos0"), (n, "n")):
        _req(t, torch.int32, what)
        if t.numel() != R:
            raise RuntimeError(f"kv_append_segments: {what} has {t.numel()} entries for R = {R}")
    n_slots, max_len, D3 = cache.shape
    if src.dim() != 2 or src.shape[0] < T or src.shape[1] != D3 or cache.stride(2) != 1 or src.stride(1) != 1:
        raise RuntimeError(f"kv_append_segments: src {tuple(src.shape)}, cache {tuple(cache.shape)}, T {T}")
    _check(lib().stllm_kv_append_segments(dtype_code(cache.dtype), _p(src), src.stride(0), _p(cache), cache.stride(0), cache.stride(1), _p(slot), _p(row0),
                                          _p(pos0), _p(n), R, T, n_slots, max_n, D3 // 3, max_len, _stream()), "stllm_kv_append_segments")
    return cache


def beam_rows_available(device):
    """kv_reorder_rows and beam_candidates_rows can serve tensors on `device`: a device check, nothing more (as segments_available).
    serving.Engine(num_beams > 1) asks before it allocates anything; a stand-in for this module that states the two contracts answers for itself."""
    return torch.device(device).type == "cuda"


def kv_reorder_rows(cache, src, lo, hi, *, nb, max_span):
    """stllm_kv_reorder_rows: the rows of cache [rows, capacity, 3*hidden] (one layer buffer) come in groups of nb; row r takes the [k | v] bytes of row
    src[r] (int32 [rows] on the device, any mapping inside a group; outside it: identity) at the positions [lo[g], hi[g]) of its group (int32 [rows / nb],
    clamped to [0, capacity); hi - lo <= max_span), in place, in ONE launch without scratch.  nb <= 16.  All compute dtypes."""
    _req(src, torch.int32, "src"); _req(lo, torch.int32, "lo"); _req(hi, torch.int32, "hi")
    if cache.dim() != 3 or cache.stride(2) != 1 or cache.shape[2] % 3:
        raise RuntimeError(f"kv_reorder_rows: cache must be [rows, capacity, 3*hidden] with unit column stride, got {tuple(cache.shape)}")
    rows, capacity, D3 = cache.shape
    if nb < 1 or rows % nb or src.numel() != rows or lo.numel() != rows // nb or hi.numel() != rows // nb or not (src.is_contiguous() and lo.is_contiguous() and
                                                                                                         hi.is_contiguous()):
        raise RuntimeError(f"kv_reorder_rows: {rows} rows in groups of {nb}: src {tuple(src.shape)}, lo {tuple(lo.shape)}, hi {tuple(hi.shape)}")
    _check(lib().stllm_kv_reorder_rows(dtype_code(cache.dtype), _p(cache), cache.stride(0), cache.stride(1), _p(src), _p(lo), _p(hi), rows, int(nb), D3 // 3,
                                       capacity, int(max_span), _stream()), "stllm_kv_reorder_rows")
    return cache


def gather_rows(src_a, idx_a, *, src_b=None, add=None, idx_add=None, out=None, scale=1.0):
    """out[i] = scale * ((idx_a[i] >= 0 ? src_a[idx_a[i]] : src_b[-idx_a[i]-1]) (+ add[idx_add[i]]))."""
    _req(src_a, torch.float32, "src_a"); _req(idx_a, torch.int32, "idx_a")
    n, D = idx_a.numel(), src_a.shape[-1]
    if out is None:
        out = torch.empty((n, D), device=src_a.device, dtype=torch.float32)
    _check(lib().stllm_gather_rows(_p(src_a), src_a.stride(0), _p(src_b), src_b.stride(0) if src_b is not None else 0,
                                   _p(idx_a), _p(add), add.stride(0) if add is not None else 0, _p(idx_add),
                                   _p(out), out.stride(0), n, D, scale, _stream()), "stllm_gather_rows")
    return out


def _sel_rows(logits, prev, n_prev, what):
    """common operands of the two selection entry points: fp32 logits rows (any row stride: `logits_from` returns a view of the padded rows) and the
    int32 ids generated so far, of which the first n_prev columns count"""
    _req(logits, torch.float32, "logits")
    if logits.dim() != 2:
        raise RuntimeError(f"{what}: logits must be [rows, V], got {tuple(logits.shape)}")
    rows = logits.shape[0]
    if n_prev:
        _req(prev, torch.int32, "prev")
        if prev.dim() != 2 or prev.shape[0] != rows or prev.shape[1] < n_prev:
            raise RuntimeError(f"{what}: prev {tuple(prev.shape)} does not hold {n_prev} ids for each of {rows} rows")
    return rows, logits.shape[1], (logits.stride(0) if rows > 1 else max(logits.stride(0), logits.shape[1]))


def select_tokens(logits, out, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, pad_id=0, sample=False, temperature=1.0, top_p=1.0,
                  u=None, unfinished=None, aux=None):
    """stllm_select_tokens: the next token of every row of `logits` f32 [rows, V] -> out (int32 [rows] view, any element stride: a column of the ids buffer).
    Repetition penalty over the distinct ids prev[r, :n_prev], EOS suppression, then argmax (lowest index) or temperature / top-p sampling driven by
    u f32 [rows] in [0, 1).  unfinished int32 [rows] (in / out): rows at 0 emit pad_id, rows that emit eos_id are set to 0.  aux f32 [rows, 4] (optional):
    max, log-sum-exp - max, threshold e-value, kept mass.  A vocabulary that does not fit the LDS raises (no other path runs)."""
    rows, V, ldl = _sel_rows(logits, prev, n_prev, "select_tokens")
    _req(out.unsqueeze(-1), torch.int32, "out")   # device and dtype only: a strided column of the ids buffer is what this output is for
    if out.dim() != 1 or out.numel() != rows:
        raise RuntimeError(f"select_tokens: out must be int32 [{rows}], got {tuple(out.shape)}")
    if sample:
        _req(u, torch.float32, "u")
        if u.numel() != rows or not u.is_contiguous():
            raise RuntimeError("select_tokens(sample): u must be contiguous f32 [rows]")
    if unfinished is not None:
        _req(unfinished, torch.int32, "unfinished")
        if unfinished.numel() != rows or not unfinished.is_contiguous():
            raise RuntimeError("select_tokens: unfinished must be contiguous int32 [rows]")
    if aux is not None:
        _req(aux, torch.float32, "aux")
        if tuple(aux.shape) != (rows, 4) or not aux.is_contiguous():
            raise RuntimeError("select_tokens: aux must be contiguous f32 [rows, 4]")
    a = SelectArgs(logits=logits.data_ptr(), ldl=ldl, rows=rows, V=V, prev=prev.data_ptr() if n_prev else None, ld_prev=prev.stride(0) if n_prev else 0,
                   n_prev=n_prev, penalty=penalty, suppress_eos=int(bool(suppress_eos)), eos_id=-1 if eos_id is None else int(eos_id), pad_id=int(pad_id),
                   sample=int(bool(sample)), temperature=temperature, top_p=top_p, u=u.data_ptr() if sample else None,
                   unfinished=unfinished.data_ptr() if unfinished is not None else None, out=out.data_ptr(), out_stride=out.stride(0) if rows > 1 else 1,
                   aux=aux.data_ptr() if aux is not None else None)
    _check(lib().stllm_select_tokens(ctypes.byref(a), _stream()), "stllm_select_tokens")
    return out


def select_slots(logits, src, state, ids, *, penalty=1.0, min_length=0, eos_id=None, pad_id=0, sample=False, temperature=1.0, top_p=1.0, u=None, stops=None,
                 stop_len=None, aux=None):
    """stllm_select_slots: one launch selects the next token of every SERVED slot of a continuous batch.  logits f32 [rows, V]; src int32 [n_slots]: slot s
    reads row src[s] (outside [0, rows): not served, untouched); state int32 [n_slots, 4] = (live, n_gen, max_new, pending) and ids int32 [n_slots, ld_ids],
    both in / out: a live slot appends its token at ids[s, n_gen], counts it, leaves it in `pending` and drops `live` on EOS, at max_new or when its ids end
    in a row of stops int32 [n_stop, ld_stop] (stop_len int32 [n_stop]); a dead served slot gets pending = pad_id.  EOS is suppressed while n_gen <
    min_length; u f32 [n_slots] drives sampling; aux f32 [n_slots, 4] (optional) as select_tokens.  V + ld_ids floats that do not fit the LDS raise."""
    _req(logits, torch.float32, "logits")
    if logits.dim() != 2:
        raise RuntimeError(f"select_slots: logits must be [rows, V], got {tuple(logits.shape)}")
    rows, V = logits.shape
    ldl = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    _req(src, torch.int32, "src"); _req(state, torch.int32, "state"); _req(ids, torch.int32, "ids")
    n_slots = src.numel()
    if src.dim() != 1 or not src.is_contiguous() or tuple(state.shape) != (n_slots, 4) or not state.is_contiguous():
        raise RuntimeError(f"select_slots: src must be contiguous int32 [n_slots], state contiguous int32 [n_slots, 4]; got {tuple(src.shape)}, {tuple(state.shape)}")
    if ids.dim() != 2 or ids.shape[0] != n_slots or ids.shape[1] < 1 or not ids.is_contiguous():
        raise RuntimeError(f"select_slots: ids must be contiguous int32 [{n_slots}, ld_ids >= 1], got {tuple(ids.shape)}")
    if sample:
        _req(u, torch.float32, "u")
        if u.numel() != n_slots or not u.is_contiguous():
            raise RuntimeError("select_slots(sample): u must be contiguous f32 [n_slots]")
    n_stop = 0 if stops is None else stops.shape[0]
    if n_stop:
        _req(stops, torch.int32, "stops"); _req(stop_len, torch.int32, "stop_len")
        if stops.dim() != 2 or stops.shape[1] < 1 or not stops.is_contiguous() or stop_len.numel() != n_stop or not stop_len.is_contiguous():
            raise RuntimeError("select_slots: stops must be contiguous int32 [n_stop, ld_stop >= 1], stop_len contiguous int32 [n_stop]")
    if aux is not None:
        _req(aux, torch.float32, "aux")
        if tuple(aux.shape) != (n_slots, 4) or not aux.is_contiguous():
            raise RuntimeError("select_slots: aux must be contiguous f32 [n_slots, 4]")
    a = SelectSlotsArgs(logits=logits.data_ptr(), ldl=ldl, rows=rows, V=V, n_slots=n_slots, src=src.data_ptr(), state=state.data_ptr(), ids=ids.data_ptr(),
                        ld_ids=ids.shape[1], penalty=penalty, min_length=int(min_length),
                        eos_id=-1 if eos_id is None else int(eos_id), pad_id=int(pad_id), sample=int(bool(sample)), temperature=temperature, top_p=top_p,
                        u=u.data_ptr() if sample else None, stops=stops.data_ptr() if n_stop else None, ld_stop=stops.shape[1] if n_stop else 0,
                        stop_len=stop_len.data_ptr() if n_stop else None, n_stop=n_stop, aux=aux.data_ptr() if aux is not None else None)
    _check(lib().stllm_select_slots(ctypes.byref(a), _stream()), "stllm_select_slots")
    return state


def beam_candidates(logits, beam_score, k, *, prev=None, n_prev=0, penalty=1.0, suppress_eos=False, eos_id=None, cand_score=None, cand_token=None):
    """stllm_beam_candidates: per row the k best of log_softmax(logits) (penalised over prev[r, :n_prev], EOS suppressed) + beam_score[r], ordered by
    (score descending, token ascending) -> (cand_score f32 [rows, k], cand_token int32 [rows, k]).  1 <= k <= min(32, V)."""
    rows, V, ldl = _sel_rows(logits, prev, n_prev, "beam_candidates")
    _req(beam_score, torch.float32, "beam_score")
    if beam_score.numel() != rows or not beam_score.is_contiguous():
        raise RuntimeError("beam_candidates: beam_score must be contiguous f32 [rows]")
    if cand_score is None:
        cand_score = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    if cand_token is None:
        cand_token = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    _req(cand_score, torch.float32, "cand_score"); _req(cand_token, torch.int32, "cand_token")
    if tuple(cand_score.shape) != (rows, k) or tuple(cand_token.shape) != (rows, k) or not cand_score.is_contiguous() or not cand_token.is_contiguous():
        raise RuntimeError(f"beam_candidates: cand_score / cand_token must be contiguous [{rows}, {k}]")
    a = BeamArgs(logits=logits.data_ptr(), ldl=ldl, rows=rows, V=V, prev=prev.data_ptr() if n_prev else None, ld_prev=prev.stride(0) if n_prev else 0,
                 n_prev=n_prev, penalty=penalty, suppress_eos=int(bool(suppress_eos)), eos_id=-1 if eos_id is None else int(eos_id),
                 beam_score=beam_score.data_ptr(), k=int(k), cand_score=cand_score.data_ptr(), cand_token=cand_token.data_ptr())
    _check(lib().stllm_beam_candidates(ctypes.byref(a), _stream()), "stllm_beam_candidates")
    return cand_score, cand_token


SEL_LDS_BYTES = 160 * 1024 - 4096   # kSelLdsBytes of csrc/elementwise.hip: the dynamic LDS that a row of a selection launch may take


def beam_rows_fit(V, ld_prev):
    """whether stllm_beam_candidates_rows takes rows of V logits behind a history table of ld_prev columns: V + ld_prev floats in the LDS, whatever the
    rows hold.  serving.Engine(num_beams > 1, state="device") asks when a request is submitted, so that no launch in the middle of a run raises."""
    return (int(V) + int(ld_prev)) * 4 <= SEL_LDS_BYTES


def beam_candidates_rows(logits, src, beam_score, k, *, prev=None, n_prev, penalty=1.0, min_length=0, eos_id=None, cand_score=None, cand_token=None):
    """stllm_beam_candidates_rows: beam_candidates for the beam rows of a continuous batch.  logits f32 [n_logits_rows, V]; src int32 [rows]: candidate row
    r reads logits row src[r] (outside [0, n_logits_rows): not served, its outputs untouched; several rows may name one logits row); prev int32
    [rows, ld_prev] and n_prev int32 [rows]: row r's history is prev[r, :n_prev[r]]; EOS is suppressed while n_prev[r] < min_length; beam_score f32 [rows].
    -> (cand_score f32 [rows, k], cand_token int32 [rows, k]), a served row bit-equal to beam_candidates of that row alone.  V + ld_prev floats that do not
    fit the LDS raise."""
    _req(logits, torch.float32, "logits")
    if logits.dim() != 2:
        raise RuntimeError(f"beam_candidates_rows: logits must be [n_logits_rows, V], got {tuple(logits.shape)}")
    n_rows, V = logits.shape
    ldl = logits.stride(0) if n_rows > 1 else max(logits.stride(0), V)
    _req(src, torch.int32, "src"); _req(n_prev, torch.int32, "n_prev"); _req(beam_score, torch.float32, "beam_score")
    rows = src.numel()
    if src.dim() != 1 or n_prev.numel() != rows or beam_score.numel() != rows or not (src.is_contiguous() and n_prev.is_contiguous() and beam_score.is_contiguous()):
        raise RuntimeError(f"beam_candidates_rows: src, n_prev and beam_score must be contiguous [{rows}]")
    ld_prev = 0
    if prev is not None:
        _req(prev, torch.int32, "prev")
        if prev.dim() != 2 or prev.shape[0] != rows or not prev.is_contiguous():
            raise RuntimeError(f"beam_candidates_rows: prev must be contiguous int32 [{rows}, ld_prev], got {tuple(prev.shape)}")
        ld_prev = prev.shape[1]
    if cand_score is None:
        cand_score = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    if cand_token is None:
        cand_token = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    _req(cand_score, torch.float32, "cand_score"); _req(cand_token, torch.int32, "cand_token")
    if tuple(cand_score.shape) != (rows, k) or tuple(cand_token.shape) != (rows, k) or not cand_score.is_contiguous() or not cand_token.is_contiguous():
        raise RuntimeError(f"beam_candidates_rows: cand_score / cand_token must be contiguous [{rows}, {k}]")
    a = BeamRowsArgs(logits=logits.data_ptr(), ldl=ldl, n_logits_rows=n_rows, V=V, rows=rows, src=src.data_ptr(), prev=prev.data_ptr() if ld_prev else None,
                     ld_prev=ld_prev, n_prev=n_prev.data_ptr(), penalty=penalty, min_length=int(min_length), eos_id=-1 if eos_id is None else int(eos_id),
                     beam_score=beam_score.data_ptr(), k=int(k), cand_score=cand_score.data_ptr(), cand_token=cand_token.data_ptr())
    _check(lib().stllm_beam_candidates_rows(ctypes.byref(a), _stream()), "stllm_beam_candidates_rows")
    return cand_score, cand_token


def mean_t(x):
    """x f32 [B,T,...] contiguous -> mean over dim 1."""
    _req(x, torch.float32, "x")
    x = x.contiguous()
    B, T = x.shape[0], x.shape[1]
    J = x[0, 0].numel()
    out = torch.empty((B,) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    _check(lib().stllm_mean_t(_p(x), _p(out), B, T, J, _stream()), "stllm_mean_t")
    return out


def vit_cls_rows(cls, pos, x, n_frames):
    _check(lib().stllm_vit_cls_rows(_p(cls), _p(pos), _p(x), x.stride(0), n_frames, x.shape[-1], _stream()),
           "stllm_vit_cls_rows")


def cosine_rows(a, b, idx_a=None, idx_b=None, n_rows=None):
    n = n_rows if n_rows is not None else (idx_a.numel() if idx_a is not None else a.shape[0])
    out = torch.empty((n,), device=a.device, dtype=torch.float32)
    _check(lib().stllm_cosine_rows(_p(a), a.stride(0), _p(idx_a), _p(b), b.stride(0), _p(idx_b), _p(out), n,
                                   a.shape[-1], _stream()), "stllm_cosine_rows")
    return out


def cross_entropy_rows(logits, labels):
    """logits f32 [n,V], labels int32 [n] (already shifted; <0 = ignore) -> per-row loss f32 [n]."""
    _req(logits, torch.float32, "logits"); _req(labels, torch.int32, "labels")
    n, V = logits.shape
    out = torch.empty((n,), device=logits.device, dtype=torch.float32)
    _check(lib().stllm_cross_entropy_rows(_p(logits), logits.stride(0), _p(labels), _p(out), n, V, _stream()),
           "stllm_cross_entropy_rows")
    return out


def cast_rows(x, dtype, out=None):
    """x f32 [M,D] (row-strided ok) -> compute dtype [M,D]."""
    _req(x, torch.float32, "x")
    td = torch_dtype(dtype)
    M, D = x.shape
    if out is None:
        out = torch.empty((M, D), device=x.device, dtype=td)
    _check(lib().stllm_cast_rows(dtype_code(td), _p(x), x.stride(0), _p(out), out.stride(0), M, D, _stream()),
           "stllm_cast_rows")
    return out


def set_option(key, value):
    _check(lib().stllm_set_option(key.encode(), int(value)), "stllm_set_option")


# ----------------------------------------------------------------------------------------------
# Training entry points (include/stllm_hip.h "backward / optimizer").  Same rules: device pointers,
# current stream, no fallback.
TRAIN_EXPORTS = ["stllm_transpose", "stllm_norm_bwd_workspace_bytes", "stllm_rmsnorm_bwd", "stllm_layernorm_bwd", "stllm_swiglu",
                 "stllm_swiglu_bwd", "stllm_rope_bwd", "stllm_attention_bwd_workspace_bytes", "stllm_attention_bwd", "stllm_cross_entropy_bwd", "stllm_scatter_add_rows",
                 "stllm_cosine_rows_bwd", "stllm_colsum", "stllm_relu_bwd", "stllm_gelu", "stllm_gelu_bwd", "stllm_scale_rows", "stllm_bcast_add_t", "stllm_adamw", "stllm_sumsq"]
EXPORTS += TRAIN_EXPORTS
_train_bound = False


def _tlib():
    global _train_bound
    L = lib()
    if not _train_bound:
        i64, i, f, p = c_int64, c_int, c_float, c_void_p
        L.stllm_transpose.argtypes = [i, p, i64, p, i64, i, i, i, p]
        L.stllm_norm_bwd_workspace_bytes.restype = c_int64
        L.stllm_norm_bwd_workspace_bytes.argtypes = [i, i]
        L.stllm_rmsnorm_bwd.argtypes = [i, p, i64, p, f, p, i64, p, i64, i, p, p, i64, i, i, p]
        L.stllm_layernorm_bwd.argtypes = [i, p, i64, p, f, p, i64, p, i64, i, p, p, p, i64, i, i, p]
        L.stllm_swiglu.argtypes = [i, p, i64, p, i64, i, i, p]
        L.stllm_swiglu_bwd.argtypes = [i, p, i64, p, i64, p, i64, i, i, p]
        L.stllm_rope_bwd.argtypes = [i, p, i64, p, p, i, i, i, i, p]
        L.stllm_attention_bwd_workspace_bytes.restype = c_int64
        L.stllm_attention_bwd_workspace_bytes.argtypes = [i, i, i]
        L.stllm_attention_bwd.argtypes = [i] + [p, i64, i64] * 8 + [i, i, i, i, i, f, i, p, p, i64, p]
        L.stllm_cross_entropy_bwd.argtypes = [i, p, i64, p, f, p, i64, i, i, i, p]
        L.stllm_scatter_add_rows.argtypes = [p, i64, p, p, i64, p, i64, i, i, f, p]
        L.stllm_cosine_rows_bwd.argtypes = [p, i64, p, p, i64, p, f, p, i64, i, i, p]
        L.stllm_colsum.argtypes = [i, p, i64, p, i, i, p, i64, p]
        L.stllm_relu_bwd.argtypes = [i, p, i64, p, i64, p, i64, i, i, p]
        L.stllm_gelu.argtypes = [i, p, i64, p, i64, i, i, p]
        L.stllm_scale_rows.argtypes = [i, p, i64, p, p, i, i, i, p]
        L.stllm_gelu_bwd.argtypes = [i, p, i64, p, i64, p, i64, i, i, p]
        L.stllm_bcast_add_t.argtypes = [p, p, i, i, i64, f, p]
        L.stllm_adamw.argtypes = [p, p, p, p, p, i, i64, f, f, f, f, f, i, f, p]
        L.stllm_sumsq.argtypes = [p, i64, p, p]
        for n in TRAIN_EXPORTS:
            if not n.endswith("_workspace_bytes"):
                getattr(L, n).restype = c_int
        _train_bound = True
    return L


def _colws(rows, cols, device):
    need = int(_tlib().stllm_norm_bwd_workspace_bytes(rows, cols))
    return torch.empty(need, dtype=torch.uint8, device=device), need


def transpose(x, *, pad=64, out=None):
    """x [R, C] (bf16 / f16 / f32, row-strided) -> out [C, Rp], Rp = R rounded up to `pad`; out[c, r] = x[r, c], 0 for r >= R.
    (Operand re-layout for the dgrad / wgrad GEMMs: stllm_gemm contracts over the contiguous dim of both operands.)"""
    _req(x, None, "x")
    R, C = x.shape
    Rp = (R + pad - 1) // pad * pad
    if out is None:
        out = torch.empty((C, Rp), device=x.device, dtype=x.dtype)
    _check(_tlib().stllm_transpose(dtype_code(x.dtype), _p(x), x.stride(0), _p(out), out.stride(0), R, C, Rp, _stream()), "stllm_transpose")
    return out


def rmsnorm_bwd(x, gamma, eps, dy, dx, *, accumulate=True):
    """y = gamma * x * rsqrt(mean(x^2) + eps).  x f32 [M,D]; dy [M,D] (compute dtype or f32); dx f32 [M,D] (+= if accumulate).
    Returns dgamma f32 [D] (deterministic two-stage column reduction)."""
    _req(x, torch.float32, "x"); _req(dx, torch.float32, "dx"); _req(dy, None, "dy")
    M, D = x.shape
    dgamma = torch.empty((D,), device=x.device, dtype=torch.float32)
    ws, need = _colws(M, D, x.device)
    _check(_tlib().stllm_rmsnorm_bwd(dtype_code(dy.dtype), _p(x), x.stride(0), _p(gamma), eps, _p(dy), dy.stride(0), _p(dx), dx.stride(0),
                                     int(accumulate), _p(dgamma), _p(ws), need, M, D, _stream()), "stllm_rmsnorm_bwd")
    return dgamma


def layernorm_bwd(x, gamma, eps, dy, dx=None, *, accumulate=False):
    """LayerNorm backward (fp32 statistics).  x f32 [M,D], dy [M,D] -> (dx f32 [M,D], dgamma [D], dbeta [D])."""
    _req(x, torch.float32, "x"); _req(dy, None, "dy")
    M, D = x.shape
    if dx is None:
        dx = torch.empty((M, D), device=x.device, dtype=torch.float32)
        accumulate = False
    dgamma = torch.empty((D,), device=x.device, dtype=torch.float32)
    dbeta = torch.empty((D,), device=x.device, dtype=torch.float32)
    ws, need = _colws(M, D, x.device)
    _check(_tlib().stllm_layernorm_bwd(dtype_code(dy.dtype), _p(x), x.stride(0), _p(gamma), eps, _p(dy), dy.stride(0), _p(dx), dx.stride(0),
                                       int(accumulate), _p(dgamma), _p(dbeta), _p(ws), need, M, D, _stream()), "stllm_layernorm_bwd")
    return dx, dgamma, dbeta


def swiglu(gu, out=None):
    """gu [M, 2I] in the packed [32 gate | 32 up] groups of pack.llama_gate_up -> silu(gate) * up [M, I] (compute dtype)."""
    _req(gu, None, "gu")
    M, N2 = gu.shape
    if out is None:
        out = torch.empty((M, N2 // 2), device=gu.device, dtype=gu.dtype)
    _check(_tlib().stllm_swiglu(dtype_code(gu.dtype), _p(gu), gu.stride(0), _p(out), out.stride(0), M, N2 // 2, _stream()), "stllm_swiglu")
    return out


def swiglu_bwd(gu, dg, out=None):
    """d(silu(gate) * up) -> d[gate | up] in the packed layout of `gu`.  gu [M,2I], dg [M,I] -> [M,2I] (compute dtype)."""
    _req(gu, None, "gu"); _req(dg, gu.dtype, "dg")
    M, N2 = gu.shape
    if out is None:
        out = torch.empty((M, N2), device=gu.device, dtype=gu.dtype)
    _check(_tlib().stllm_swiglu_bwd(dtype_code(gu.dtype), _p(gu), gu.stride(0), _p(dg), dg.stride(0), _p(out), out.stride(0), M, N2 // 2,
                                    _stream()), "stllm_swiglu_bwd")
    return out


def rope_bwd(dqkv, cos, sin, *, rope_seq, rope_cols):
    """Transpose of the ROPE epilogue's rotation, in place on the first `rope_cols` columns of dqkv [M, N] (packed head layout)."""
    _req(dqkv, None, "dqkv"); _req(cos, torch.float32, "cos"); _req(sin, torch.float32, "sin")
    M, N = dqkv.shape
    _check(_tlib().stllm_rope_bwd(dtype_code(dqkv.dtype), _p(dqkv), dqkv.stride(0), _p(cos), _p(sin), M, N, rope_seq, rope_cols, _stream()),
           "stllm_rope_bwd")
    return dqkv


def attention_bwd(q, k, v, o, do, dq, dk, dv, *, B, H, S=None, D, scale, causal=True, kv_len=None, Sq=None, Skv=None, strides=None,
                  kv_strides=None, do_strides=None, d_strides=None, dkv_strides=None):
    """Gradients of o = softmax(scale * q k^T + masks) v.  q/k/v/dq/dk/dv: 2-D views of the compute dtype as in `attention`
    (strides = (batch_stride, row_stride) in elements of q; kv_strides of k and v (default: strides); d_strides of dq; dkv_strides of
    dk and dv (default: d_strides)); o, do [B*Sq, H*D].  S = Sq = Skv for self-attention."""
    td = q.dtype
    Sq = S if Sq is None else Sq
    Skv = S if Skv is None else Skv

    def st(t, n, given):
        return given if given is not None else (n * t.stride(0), t.stride(0))
    qs = st(q, Sq, strides)
    ks = st(k, Skv, kv_strides if kv_strides is not None else (strides if Sq == Skv else None))
    dqs = st(dq, Sq, d_strides)
    dks = st(dk, Skv, dkv_strides if dkv_strides is not None else (d_strides if Sq == Skv else None))
    os_ = st(do, Sq, do_strides)
    if kv_len is not None:
        _req(kv_len, torch.int32, "kv_len")
    a = [dtype_code(td)]
    for t, ss in ((q, qs), (k, ks), (v, ks), (o, os_), (do, os_), (dq, dqs), (dk, dks), (dv, dks)):
        a += [_p(t), ss[0], ss[1]]
    need = int(_tlib().stllm_attention_bwd_workspace_bytes(B, H, Sq))
    ws = torch.empty(need, dtype=torch.uint8, device=q.device)
    _check(_tlib().stllm_attention_bwd(*a, B, H, Sq, Skv, D, scale, int(causal), _p(kv_len), _p(ws), need, _stream()), "stllm_attention_bwd")
    return dq, dk, dv


def cross_entropy_bwd(logits, labels, scale, *, dtype, vocab=None):
    """d(sum of per-row CE) * scale w.r.t. logits: (softmax - onehot) * scale for rows with label >= 0, 0 otherwise.
    logits f32 [n, Vp] (columns >= vocab are padding), labels int32 [n] -> [n, Vp] in `dtype`, padding columns 0."""
    _req(logits, torch.float32, "logits"); _req(labels, torch.int32, "labels")
    n, Vp = logits.shape
    V = Vp if vocab is None else vocab
    out = torch.empty((n, Vp), device=logits.device, dtype=torch_dtype(dtype))
    _check(_tlib().stllm_cross_entropy_bwd(dtype_code(out.dtype), _p(logits), logits.stride(0), _p(labels), scale, _p(out), out.stride(0),
                                           n, V, Vp, _stream()), "stllm_cross_entropy_bwd")
    return out


def scatter_add_rows(src, idx, dst_a, dst_b=None, scale=1.0):
    """Transpose of gather_rows: dst_a[idx[i]] += scale * src[i] (idx >= 0) or dst_b[-idx[i]-1] += scale * src[i] (fp32 atomics)."""
    _req(src, torch.float32, "src"); _req(idx, torch.int32, "idx"); _req(dst_a, torch.float32, "dst_a")
    n, D = idx.numel(), src.shape[-1]
    _check(_tlib().stllm_scatter_add_rows(_p(src), src.stride(0), _p(idx), _p(dst_a), dst_a.stride(0), _p(dst_b),
                                          dst_b.stride(0) if dst_b is not None else 0, n, D, scale, _stream()), "stllm_scatter_add_rows")


def cosine_rows_bwd(a, b, idx_a=None, idx_b=None, n_rows=None, scale=1.0):
    """Gradient of sum_i scale * (2 - 2 cos(a_i, b_i)) w.r.t. the (gathered) a rows -> f32 [n, D]; b is a constant target."""
    n = n_rows if n_rows is not None else (idx_a.numel() if idx_a is not None else a.shape[0])
    out = torch.empty((n, a.shape[-1]), device=a.device, dtype=torch.float32)
    _check(_tlib().stllm_cosine_rows_bwd(_p(a), a.stride(0), _p(idx_a), _p(b), b.stride(0), _p(idx_b), scale, _p(out), out.stride(0), n,
                                         a.shape[-1], _stream()), "stllm_cosine_rows_bwd")
    return out


def colsum(x):
    """sum over rows of x [M, N] (any dtype) -> f32 [N] (bias gradients)."""
    _req(x, None, "x")
    M, N = x.shape
    out = torch.empty((N,), device=x.device, dtype=torch.float32)
    ws, need = _colws(M, N, x.device)
    _check(_tlib().stllm_colsum(dtype_code(x.dtype), _p(x), x.stride(0), _p(out), M, N, _p(ws), need, _stream()), "stllm_colsum")
    return out


def relu_bwd(dy, y):
    """dy * (y > 0), same dtype as dy."""
    _req(dy, None, "dy"); _req(y, dy.dtype, "y")
    out = torch.empty_like(dy)
    M, N = dy.shape
    _check(_tlib().stllm_relu_bwd(dtype_code(dy.dtype), _p(dy), dy.stride(0), _p(y), y.stride(0), _p(out), out.stride(0), M, N, _stream()),
           "stllm_relu_bwd")
    return out


def gelu(x):
    """exact-erf GELU of raw pre-activations x [M,N] (compute dtype) -> same dtype"""
    _req(x, None, "x")
    out = torch.empty_like(x)
    M, N = x.shape
    _check(_tlib().stllm_gelu(dtype_code(x.dtype), _p(x), x.stride(0), _p(out), out.stride(0), M, N, _stream()), "stllm_gelu")
    return out


def gelu_bwd(x, dy):
    """dy * gelu'(x) with x the raw pre-activations"""
    _req(x, None, "x"); _req(dy, x.dtype, "dy")
    out = torch.empty_like(x)
    M, N = x.shape
    _check(_tlib().stllm_gelu_bwd(dtype_code(x.dtype), _p(x), x.stride(0), _p(dy), dy.stride(0), _p(out), out.stride(0), M, N, _stream()),
           "stllm_gelu_bwd")
    return out


def scale_rows(x, scale, *, rows_per_group=0, idx=None):
    """x[r] *= scale[idx[r]] (or scale[r // rows_per_group]) in place; x [M,N] any dtype, scale f32 — stochastic depth and its backward"""
    _req(x, None, "x"); _req(scale, torch.float32, "scale")
    if idx is not None:
        _req(idx, torch.int32, "idx")
    M, N = x.shape
    _check(_tlib().stllm_scale_rows(dtype_code(x.dtype), _p(x), x.stride(0), _p(scale), _p(idx), rows_per_group, M, N, _stream()),
           "stllm_scale_rows")
    return x


def bcast_add_t(dst, src, scale):
    """Transpose of mean_t: dst f32 [B,T,...] += scale * src f32 [B,...] for every t."""
    _req(dst, torch.float32, "dst"); _req(src, torch.float32, "src")
    assert dst.is_contiguous() and src.is_contiguous()
    B, T = dst.shape[0], dst.shape[1]
    _check(_tlib().stllm_bcast_add_t(_p(dst), _p(src), B, T, dst[0, 0].numel(), scale, _stream()), "stllm_bcast_add_t")


def adamw(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, p16=None):
    """torch.optim.AdamW's update on flat fp32 state, in place; optionally also writes the compute-dtype copy p16."""
    for t, w in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, torch.float32, w)
        assert t.is_contiguous()
    _check(_tlib().stllm_adamw(_p(p), _p(g), _p(m), _p(v), _p(p16), dtype_code(p16.dtype) if p16 is not None else 0, p.numel(), lr, beta1,
                               beta2, eps, weight_decay, step, grad_scale, _stream()), "stllm_adamw")


def sumsq(x, out=None):
    """out[0] += sum(x^2) (fp32; gradient-norm clipping)."""
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    if out is None:
        out = torch.zeros((1,), device=x.device, dtype=torch.float32)
    _check(_tlib().stllm_sumsq(_p(x), x.numel(), _p(out), _stream()), "stllm_sumsq")
    return out
