"""fastllm_amd -- MI355X (gfx950) forward-pass backend for FastLLM behind a C ABI.

The product is fastllm_amd/lib/libfastllm_mi355x.so (sources: fastllm_amd/csrc, ABI:
include/fastllm_mi355x.h).  This Python package is the thin ctypes harness the tests and
bench.py drive it with; it contains no arithmetic and no CPU fallback.
"""
from .binding import (Batch, Cache, FastLLMError, Model, abi_version, comm_unique_id, device_count, lib, op_attention, op_linear, op_sample,  # noqa: F401
                      tp_slice, tune, reload_env, library_loaded, op_quantize_rows, op_gemv_w8, lookup_draft, op_verify_select, op_verify_sample, op_verify_sample_time, op_verify_packed, op_kv_copy,
                      Encoder, FlEncoderConfig, make_encoder_config, op_encoder_attention, op_attention_plain, op_attention_batch, op_attention_packed, op_logprobs, FlLogprobs, LOGPROBS_MAX_TOP,
                      op_score, op_score_time, FlScore, SCORE_NO_TARGET, ScoreResult, op_pool_rows, FlEmbed, make_embed, POOLING, ATTN_MASK,
                      op_logit_rules, FlLogitRules, make_logit_rules, Guide, op_guide_mask, FlGuideDesc, make_guide_desc, op_verify_adjust, op_verify_adjust_time, op_rules_count,
                      op_rmsnorm_add, op_norm_linear, op_linear_resid, op_gemv_resid, FlNormLinearArgs, FlLinearResidArgs, FlGemvResidArgs, LK_NAMES,
                      op_rope_kv, op_qkv_rope, FlRopeSeqs, FlRopeKvArgs, FlQkvRopeArgs, ROPE_KV_NAMES,
                      op_attn_oproj_rep, op_attn_oproj_rep_info, FlAttnOprojRepArgs,
                      op_encoder_embed_ln, op_encoder_add_ln, op_encoder_bias_act, op_encoder_pool_l2, FlEncoderRowsArgs, ENC_ACT,
                      op_convert_slice, FlConvertSliceArgs, MODEL_TENSORS, ELEM_E4M3)
from .configs import MODEL_CONFIGS  # noqa: F401
