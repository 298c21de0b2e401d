// attn_maps.hip: attention rollout over a whole encoder stack (declared for model.hip).
#pragma once
#include <hip/hip_runtime.h>

// Layer l's packed qkv [B*S, 3*H*dh] bf16 starts at qkv0 + l * qkv_lstride bytes, its lse [B, H, S] fp32 at lse0 + l * lse_lstride
// bytes.  out fp32 [B, S]: r <- start (e_0 when cls, else 1/S); for l = L-1 .. 0: r <- r (alpha * mean_h P_l + (1 - alpha) I).
int attn_rollout_launch(const unsigned char* qkv0, long qkv_lstride, const unsigned char* lse0, long lse_lstride, int L,
                        float* out, int B, int S, int H, int dh, int cls, float alpha, hipStream_t st);
