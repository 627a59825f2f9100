// Private interface of attention_long.hip: the T > 32 routes of tecm_attention_fwd / tecm_attention_bwd (attention.hip).
// The callers have checked the pointers, alignment, head_dim == 64, 1 <= T <= 1024 and the io_bf16 masks.
#pragma once
#include "common.h"

int att_long_fwd(const float* qkv, float* ctx, int32_t io_bf16, int32_t B, int32_t T, int32_t N, int32_t heads,
                 const TecmDrop* prob_drop, hipStream_t stream);
int att_long_bwd(const float* qkv, const float* dctx, float* dqkv, int32_t io_bf16, int32_t B, int32_t T, int32_t N,
                 int32_t heads, const TecmDrop* prob_drop, hipStream_t stream);
