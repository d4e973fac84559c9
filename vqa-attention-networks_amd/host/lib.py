"""ctypes binding of libvqa_fusion.so (C ABI declared in include/vqa_fusion.h).

The product path has NO CPU fallback: if the shared library is missing or an
op is handed a non-GPU tensor, it raises.  `build()` compiles the library
in-tree with hipcc for gfx950 (cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libvqa_fusion.so")
if os.environ.get("VQF_LIB"):          # A/B builds (tools/build_variant.sh); never a different implementation
    LIB_PATH = os.path.abspath(os.environ["VQF_LIB"])
HEADER_PATH = os.path.join(os.path.dirname(PKG_DIR), "include", "vqa_fusion.h")

# The one place the expected ABI number lives (csrc/prof.hip returns it from vqf_abi_version()).
ABI_VERSION = 7

_lock = threading.Lock()
_lib = None

c_f = ctypes.c_void_p          # device float* (raw pointer)
c_i = ctypes.c_int
c_sz = ctypes.c_size_t
c_u64 = ctypes.c_uint64
c_p = ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol of include/vqa_fusion.h
SIGNATURES = {
    "vqf_abi_version": (c_i, []),
    "vqf_build_info": (ctypes.c_char_p, []),
    "vqf_set_option": (c_i, [c_i, c_i, ctypes.POINTER(c_i)]),
    "vqf_get_option": (c_i, [c_i, ctypes.POINTER(c_i)]),
    "vqf_option_env_name": (ctypes.c_char_p, [c_i]),
    "vqf_stat_get": (c_i, [c_i, ctypes.POINTER(ctypes.c_longlong)]),
    "vqf_gemm_f32_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_gemm_f32": (c_i, [c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_gemm_f32_big_rows": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_gemm_f32_sample_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "vqf_gemm_f32_sample": (c_i, [c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_gemm_f32_rowscale": (c_i, [c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_gemm_f32_batched": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, ctypes.c_longlong,
                                   c_f, c_i, ctypes.c_longlong, c_f, c_i, ctypes.c_longlong, c_i, c_p]),
    "vqf_gemm_bf16_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_gemm_bf16": (c_i, [c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_f, c_i, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_gemm_bf16_rowscale": (c_i, [c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_cast_f32_bf16": (c_i, [c_f, c_i, c_i, c_i, c_p, c_i, c_p]),
    "vqf_colsum_ws_bytes": (c_sz, [c_i, c_i]),
    "vqf_colsum_f32": (c_i, [c_f, c_i, c_i, c_i, c_f, c_p, c_sz, c_p]),
    "vqf_group_reduce_f32": (c_i, [c_f, c_i, c_i, c_i, c_f, c_p]),
    "vqf_relu_bwd_f32": (c_i, [c_f, c_f, c_i, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_att_logits_fwd": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_p]),
    "vqf_att_logits_fwd_lin": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_att_logits_bwd_ws_bytes": (c_sz, [c_i, c_i]),
    "vqf_att_logits_bwd_rowscale": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_att_logits_bwd_rowscale_obf16": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_p, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_att_logits_bwd": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_glimpse_pool_fwd": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_fwd_bf16": (c_i, [c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_bf16": (c_i, [c_f, c_f, c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_dropout_f32": (c_i, [c_f, c_p, c_u64, ctypes.c_float, ctypes.c_longlong, c_f, c_p]),
    "vqf_dropout_bt": (c_i, [c_f, ctypes.c_longlong, ctypes.c_longlong, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f,
                             ctypes.c_longlong, ctypes.c_longlong, c_p]),
    "vqf_gate_tanh_sigmoid_fwd": (c_i, [c_f, c_f, ctypes.c_longlong, c_f, c_p]),
    "vqf_gate_tanh_sigmoid_bwd": (c_i, [c_f, c_f, c_f, ctypes.c_longlong, c_f, c_f, c_p]),
    "vqf_tanh_dropout_fwd": (c_i, [c_f, c_f, c_p, c_u64, ctypes.c_float, ctypes.c_longlong, c_f, c_p]),
    "vqf_tanh_dropout_bwd": (c_i, [c_f, c_f, c_p, c_u64, ctypes.c_float, ctypes.c_longlong, c_f, c_p]),
    "vqf_tanh_dropout_fwd2d": (c_i, [c_f, c_i, c_f, c_i, c_p, c_u64, ctypes.c_float, c_i, c_i, c_f, c_i, c_p]),
    "vqf_tanh_dropout_bwd2d": (c_i, [c_f, c_i, c_f, c_i, c_p, c_u64, ctypes.c_float, c_i, c_i, c_f, c_i, c_p]),
    "vqf_relu_bwd_rank1_f32": (c_i, [c_f, c_f, c_f, c_f, c_i, ctypes.c_float, c_i, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_multi_add_f32": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p]),
    "vqf_multi_copy_f32": (c_i, [c_p, c_p, c_p, c_i, c_p]),
    "vqf_hie_stream_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "vqf_hie_chunks": (c_i, [c_i, c_i]),
    "vqf_hie_hv_fwd": (c_i, [c_f, c_i, c_f, c_f, c_i, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_hie_head_bwd": (c_i, [c_f, c_i, c_f, c_f, c_f, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i,
                               c_f, c_i, c_p]),
    "vqf_hie_rank_add": (c_i, [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_hie_rank_left": (c_i, [c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_hie_slab_sum": (c_i, [c_f, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_hie_affinity_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_hie_affinity": (c_i, [c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_i, c_f, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_phrase_ngram_supported": (c_i, [c_i, c_i]),
    "vqf_phrase_ngram_fwd": (c_i, [c_f, c_i, c_f, c_i, c_i, c_i, c_f, c_i, c_p, c_p]),
    "vqf_phrase_ngram_bwd": (c_i, [c_f, c_i, c_f, c_i, c_p, c_i, c_i, c_i, c_f, c_i, c_p]),
    "vqf_hie_affinity_levels_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "vqf_hie_affinity_levels": (c_i, [c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i,
                                      c_f, c_p]),
    # the question-length forms of HieCoAttenLadder (lens: device int32 pointer, c_p)
    "vqf_embed_tanh_fwd_len": (c_i, [c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_tanh_bwd_len": (c_i, [c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_phrase_ngram_fwd_len": (c_i, [c_f, c_i, c_f, c_p, c_i, c_i, c_i, c_f, c_i, c_p, c_p]),
    "vqf_phrase_ngram_bwd_len": (c_i, [c_f, c_i, c_f, c_i, c_p, c_p, c_i, c_i, c_i, c_f, c_i, c_p]),
    "vqf_dropout_bt_len": (c_i, [c_f, ctypes.c_longlong, ctypes.c_longlong, c_p, c_u64, ctypes.c_float, c_p, c_i, c_i, c_i, c_f,
                                 ctypes.c_longlong, ctypes.c_longlong, c_p]),
    "vqf_glimpse_pool_fwd_len": (c_i, [c_f, c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_len": (c_i, [c_f, c_f, c_f, c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_hie_affinity_len": (c_i, [c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_i, c_f, c_p, c_u64, ctypes.c_float, c_p, c_i, c_i, c_i,
                                   c_i, c_f, c_p]),
    "vqf_hie_affinity_levels_len": (c_i, [c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_p, c_i, c_i,
                                          c_i, c_i, c_f, c_p]),
    "vqf_tanh_bwd_rows_len": (c_i, [c_f, c_f, c_p, c_i, c_i, c_i, c_f, c_p]),
    # the region-count forms of HieCoAttenLadder's image-side passes (lens / rlens: device int32 pointers, c_p)
    "vqf_hie_affinity_regions": (c_i, [c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_i, c_f, c_p, c_u64, ctypes.c_float, c_p, c_p, c_i,
                                       c_i, c_i, c_i, c_f, c_p]),
    "vqf_hie_affinity_levels_regions": (c_i, [c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_f, c_p, c_p,
                                              c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_hie_hv_fwd_regions": (c_i, [c_f, c_i, c_f, c_f, c_i, c_p, c_u64, ctypes.c_float, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i,
                                     c_f, c_i, c_p]),
    "vqf_hie_rank_add_regions": (c_i, [c_f, c_i, c_f, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_p]),
    "vqf_hie_rank_left_regions": (c_i, [c_f, c_f, c_i, c_f, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_f, c_i, c_f, c_i,
                                        c_p]),
    "vqf_zero_cols_len": (c_i, [c_f, c_p, ctypes.c_longlong, c_i, c_i, c_i, c_p]),
    # the guided attention logits of HieCoAttenLadder's alternating co-attention (csrc/hie_ladder_alt.hip)
    "vqf_guided_logits_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_fwd": (c_i, [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_guided_logits_bwd_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_bwd": (c_i, [c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_f, c_p, c_sz, c_p]),
    # the grouped forms: N questions over U shared images (idx / order / grp_off: device int32 pointers, c_p)
    "vqf_guided_logits_grouped_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_fwd_grouped": (c_i, [c_f, c_i, c_f, c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_guided_logits_bwd_grouped_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_bwd_grouped": (c_i, [c_f, c_f, c_i, c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_f, c_p, c_sz,
                                            c_p]),
    "vqf_glimpse_pool_grouped_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_glimpse_pool_fwd_grouped": (c_i, [c_f, c_f, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_grouped": (c_i, [c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_row_block_supported": (c_i, [c_i, c_i, ctypes.c_longlong]),
    "vqf_row_block_gather": (c_i, [c_f, c_p, c_i, c_i, ctypes.c_longlong, c_f, c_p]),
    "vqf_row_block_group_sum": (c_i, [c_f, c_p, c_p, c_i, c_i, ctypes.c_longlong, c_f, c_p]),
    "vqf_softmax_rows_fwd": (c_i, [c_f, c_i, c_i, c_f, c_p]),
    "vqf_softmax_rows_bwd": (c_i, [c_f, c_f, c_i, c_i, c_f, c_p]),
    "vqf_log_softmax_rows_fwd": (c_i, [c_f, c_i, c_i, c_f, c_p]),
    "vqf_log_softmax_rows_bwd": (c_i, [c_f, c_f, c_i, c_i, c_f, c_p]),
    "vqf_mfb_fuse_fwd": (c_i, [c_f, c_f, c_f, c_f, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_f, c_f, c_p]),
    "vqf_l2_group_norm": (c_i, [c_f, c_i, c_i, c_f, c_f, c_p]),
    "vqf_scale_rows": (c_i, [c_f, c_f, c_i, c_i, c_i, c_f, c_p]),
    "vqf_rowdot": (c_i, [c_f, c_f, c_i, c_i, c_f, c_p]),
    "vqf_l2_norm_bwd_coef": (c_i, [c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_p]),
    "vqf_l2_norm_bwd_coef_lin": (c_i, [c_f, c_f, c_i, c_f, c_f, c_i, c_i, c_f, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_ws_bytes": (c_sz, [c_i, c_i, c_i]),
    "vqf_mfb_fuse_bwd": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_u64, ctypes.c_float,
                               c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_fwd_pbf16": (c_i, [c_p, c_f, c_f, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_fwd_pbf16_rb": (c_i, [c_p, c_f, c_f, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_p, c_i, c_f, c_p]),
    "vqf_mfb_fuse_bwd_pbf16": (c_i, [c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_p, c_u64, ctypes.c_float,
                                     c_i, c_i, c_i, c_p, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_bf16dp": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_u64, ctypes.c_float,
                                      c_i, c_i, c_i, c_p, c_f, c_f, c_p, c_sz, c_p]),
    # the grouped image fusion: N questions over U shared images (MFB / MHBCoAtt forward(..., img_index))
    "vqf_mfb_fuse_grouped_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "vqf_mfb_fuse_fwd_grouped": (c_i, [c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_grouped_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "vqf_mfb_fuse_bwd_grouped": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_u64, ctypes.c_float,
                                       c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    # the region-count forms of the image fusion (MFB / MHBCoAtt forward((img, img_length), ...)): lens device int32 pointers (c_p)
    "vqf_mfb_fuse_fwd_len": (c_i, [c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_len": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                   c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_fwd_grouped_len": (c_i, [c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f,
                                           c_p]),
    "vqf_mfb_fuse_bwd_grouped_len": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_u64, ctypes.c_float,
                                           c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_glimpse_pool_fwd_grouped_len": (c_i, [c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_grouped_len": (c_i, [c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    # the packed forms (forward(PackedRegions, ...)): P / dP / feat hold the real rows only, roff device int32 row offsets (c_p)
    "vqf_mfb_fuse_packed_supported": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_mfb_fuse_fwd_packed": (c_i, [c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_packed": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                      c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_fwd_grouped_packed": (c_i, [c_f, c_f, c_f, c_p, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_i, c_f, c_f,
                                              c_p]),
    "vqf_mfb_fuse_bwd_grouped_packed": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_u64, ctypes.c_float,
                                              c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_glimpse_pool_fwd_packed": (c_i, [c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_packed": (c_i, [c_f, c_f, c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    # the co-attention head on the packed rows (MFB / MHBCoAtt packed_coatt): R / Y / dY / rowssq / logits / dlogits hold the real rows
    "vqf_mfb_fuse_fwd_packed_rows": (c_i, [c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_packed_rows": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                           c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_sz, c_p]),
    # the bf16 image projection on counted / packed regions (MFB / MHBCoAtt regions_bf16; csrc/fusion_regions_bf16.hip): a bf16 P and /
    # or a bf16 dP of dP_rows rows (the int behind dP), zero behind the real ones
    "vqf_mfb_fuse_fwd_len_pbf16": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_fwd_packed_pbf16": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_fwd_packed_rows_pbf16": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_mfb_fuse_bwd_len_pbf16": (c_i, [c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                         c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_len_bf16dp": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                          c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_packed_pbf16": (c_i, [c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                            c_i, c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_packed_bf16dp": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                             c_i, c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_packed_rows_pbf16": (c_i, [c_f, c_f, c_f, c_f, c_f, c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                                 c_i, c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_mfb_fuse_bwd_packed_rows_bf16dp": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float,
                                                  c_i, c_i, c_i, c_i, c_p, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_cast_f32_bf16_rows": (c_i, [c_f, c_i, c_i, c_i, c_p, c_i, c_i, c_p]),
    # ... with the bf16 copy of R (regions_bf16_coatt): R_bf16, its pitch and its allocated rows behind R
    "vqf_mfb_fuse_fwd_len_pbf16_rb": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_f, c_p, c_i, c_i, c_f,
                                            c_p]),
    "vqf_mfb_fuse_fwd_packed_pbf16_rb": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p, c_i, c_i,
                                               c_f, c_p]),
    "vqf_mfb_fuse_fwd_packed_rows_pbf16_rb": (c_i, [c_p, c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p, c_i,
                                                    c_i, c_f, c_p]),
    "vqf_l2_group_norm_packed": (c_i, [c_f, c_p, c_i, c_i, c_i, c_f, c_f, c_f, c_p]),
    "vqf_l2_norm_bwd_coef_packed": (c_i, [c_f, c_p, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_l2_norm_bwd_coef_lin_packed": (c_i, [c_f, c_f, c_i, c_p, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_p]),
    "vqf_glimpse_pool_fwd_packed_rows": (c_i, [c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_glimpse_pool_bwd_packed_rows": (c_i, [c_f, c_f, c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    # the tanh / dropout pass as the packed <-> padded change of layout (HieCoAttenLadder.forward(PackedRegions, ...)): roff c_p
    "vqf_tanh_dropout_unpack_supported": (c_i, [c_i, c_i, c_i, c_i]),
    "vqf_tanh_dropout_unpack_fwd": (c_i, [c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_tanh_dropout_pack_bwd": (c_i, [c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_tanh_dropout_packed_fwd": (c_i, [c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_tanh_dropout_packed_bwd": (c_i, [c_f, c_f, c_p, c_p, c_u64, ctypes.c_float, c_i, c_i, c_i, c_i, c_f, c_p]),
    # the packed forms of the alternating image side (HieCoAttenLadder(packed_coatt=True)): Xh / dXh / feat / dfeat (R, .), roff c_p
    "vqf_guided_logits_packed_supported": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_fwd_packed": (c_i, [c_f, c_i, c_f, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_guided_logits_bwd_packed_ws_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "vqf_guided_logits_bwd_packed": (c_i, [c_f, c_f, c_i, c_f, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_i, c_f, c_f,
                                           c_p, c_sz, c_p]),
    "vqf_glimpse_pool_bwd_packed_dfeat": (c_i, [c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_f,
                                                c_p]),
    "vqf_lstm_seq_supported": (c_i, [c_i, c_i]),
    "vqf_lstm_seq_ws_bytes": (c_sz, [c_i, c_i]),
    "vqf_lstm_seq_fwd": (c_i, [c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_lstm_seq_bwd": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_lstm_cell_fwd": (c_i, [c_f, c_f, c_i, c_i, c_f, c_f, c_p]),
    "vqf_lstm_step_supported": (c_i, [c_i, c_i]),
    "vqf_lstm_step_fwd": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_f, c_f, c_p]),
    "vqf_lstm_cell_bwd": (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_f, c_f, c_p]),
    "vqf_embed_tanh_fwd": (c_i, [c_f, c_p, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_tanh_bwd": (c_i, [c_f, c_f, c_p, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_fwd": (c_i, [c_f, c_p, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_bwd": (c_i, [c_f, c_p, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_dropout_fwd": (c_i, [c_f, c_p, c_i, c_i, c_i, c_p, c_u64, ctypes.c_float, c_f, c_p]),
    "vqf_embed_dropout_bwd": (c_i, [c_f, c_p, c_i, c_i, c_i, c_p, c_u64, ctypes.c_float, c_f, c_p]),
    "vqf_embed_tanh_fwd_tm": (c_i, [c_f, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_embed_tanh_bwd_tm": (c_i, [c_f, c_f, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_feat_transpose": (c_i, [c_f, c_i, c_i, c_i, c_i, c_p, c_p]),
    "vqf_region_rows_stage": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "vqf_loss_ws_bytes": (c_sz, [c_i, c_i]),
    "vqf_ce_loss": (c_i, [c_f, c_p, c_i, c_i, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_kldiv_loss": (c_i, [c_f, c_f, c_i, c_i, c_f, c_f, c_p, c_sz, c_p]),
    # the evaluation tail (csrc/train.hip, csrc/eval.hip): counts int64 x 2, sums double, all device pointers
    "vqf_ce_loss_pred": (c_i, [c_f, c_p, c_i, c_i, c_f, c_f, c_p, c_p, c_p, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_answer_match_rows": (c_i, [c_f, c_f, c_i, c_i, c_p, c_p, c_f, c_p, c_p, c_f, c_p, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_topk_rows_supported": (c_i, [c_i, c_i]),
    "vqf_topk_rows": (c_i, [c_f, c_i, c_i, c_i, c_i, c_i, c_p, c_f, c_p]),
    # BCE with logits on soft answers (csrc/train.hip): scale a double, rows int64, sums double, all device pointers
    "vqf_bce_loss_ws_bytes": (c_sz, [c_i]),
    "vqf_bce_loss": (c_i, [c_f, c_f, c_i, c_i, ctypes.c_double, c_f, c_f, c_p, c_f, c_p, c_p, c_p, c_f, c_i, c_p, c_sz, c_p]),
    "vqf_bce_loss_sparse": (c_i, [c_f, c_p, c_i, c_f, c_i, c_i, c_i, ctypes.c_double, c_f, c_f, c_p, c_f, c_p, c_p, c_p, c_f,
                                  c_i, c_p, c_sz, c_p]),
    "vqf_adam_step": (c_i, [c_p, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                            ctypes.c_double, ctypes.c_longlong, c_p]),
    # gradient-norm clipping and the steps that read its coefficient (csrc/train.hip): tensors a host AdamTensor array,
    # max_norm a double, norm / coef / scale device fp32 pointers
    "vqf_grad_norm_ws_bytes": (c_sz, [c_p, c_i]),
    "vqf_grad_norm_clip": (c_i, [c_p, c_i, ctypes.c_double, c_f, c_f, c_p, c_sz, c_p]),
    "vqf_grad_scale": (c_i, [c_p, c_i, c_f, c_p]),
    "vqf_adam_step_scaled": (c_i, [c_p, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_longlong, c_f, c_p]),
    "vqf_adamax_step": (c_i, [c_p, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, ctypes.c_longlong, c_f, c_p]),
    "vqf_hbm_copy": (c_i, [c_p, c_p, ctypes.c_longlong, c_i, c_p]),
    "vqf_hbm_read_sweep_blocks": (c_i, [ctypes.c_longlong]),
    "vqf_hbm_read_sweep": (c_i, [c_p, ctypes.c_longlong, c_i, c_f, c_p]),
    "vqf_prof_enable": (None, [c_i]),
    "vqf_prof_filter": (None, [ctypes.c_longlong]),
    "vqf_prof_reset": (None, []),
    "vqf_prof_num_kernels": (c_i, []),
    "vqf_prof_kernel_name": (ctypes.c_char_p, [c_i]),
    "vqf_prof_get": (c_i, [c_i, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double)]),
    "vqf_prof_get_shape": (c_i, [c_i, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_longlong),
                                 ctypes.POINTER(ctypes.c_double)]),
}

class AdamTensor(ctypes.Structure):
    """VqfAdamTensor of include/vqa_fusion.h."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_longlong)]


_ERR = {-1: "VQF_E_BADARG", -2: "VQF_E_ALIGN", -3: "VQF_E_UNSUPPORTED", -4: "VQF_E_WORKSPACE", -5: "VQF_E_TIMEOUT"}


class VqfError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile csrc/*.hip into libvqa_fusion.so for gfx950 (make -C csrc)."""
    srcs = [os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith((".hip", ".h"))]
    srcs.append(HEADER_PATH)
    stale = force or not os.path.exists(LIB_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if not stale:
        return LIB_PATH
    cmd = ["make", "-C", CSRC_DIR, "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        subprocess.run(["make", "-C", CSRC_DIR, "clean"], check=True, capture_output=not verbose)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout)
        print(r.stderr)
    if r.returncode:
        raise VqfError("hipcc build of libvqa_fusion.so failed (see output above)")
    return LIB_PATH


def load():
    """Return the loaded library; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise VqfError(
                "libvqa_fusion.so is missing (%s).  The HIP extension is the product path and "
                "there is no CPU fallback: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C %s`." % (LIB_PATH, CSRC_DIR))
        # torch first: PyTorch-ROCm bundles its own libamdhip64 (same SONAME); loading ours
        # before it would put two HIP runtimes in the process (kernels would then be launched
        # on a runtime that has not opened torch's device/streams -> hipErrorNoDevice).
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)        # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.vqf_abi_version() != ABI_VERSION:
            raise VqfError("libvqa_fusion.so ABI version %d, host expects %d: rebuild with `make -C %s`"
                           % (lib.vqf_abi_version(), ABI_VERSION, CSRC_DIR))
        _lib = lib
        return _lib


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise VqfError("%s: %s" % (what, _ERR.get(rc, "error %d" % rc)))
    raise VqfError("%s: HIP error %d" % (what, rc))
