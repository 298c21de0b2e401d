// attn_maps.hip: attention rollout over a whole encoder stack and the relevance step (declared for model.hip).
#pragma once
#include <hip/hip_runtime.h>

// Layer l's packed qkv [B*S, 3*H*dh] bf16 starts at qkv0 + l * qkv_lstride bytes, its lse [B, H, S] fp32 at lse0 + l * lse_lstride
// bytes.  out fp32 [B, S]: r <- start (e_0 when cls, else 1/S); for l = L-1 .. 0: r <- r (alpha * mean_h P_l + (1 - alpha) I).
int attn_rollout_launch(const unsigned char* qkv0, long qkv_lstride, const unsigned char* lse0, long lse_lstride, int L,
                        float* out, int B, int S, int H, int dh, int cls, float alpha, hipStream_t st);

// One relevance step r_out[b, k] = r_in[b, k] + (1/H) sum_h sum_q r_in[b, q] max(P_h[q, k] dP_h[q, k], 0) (iq_attn_relevance_step);
// start 1: r_in is e_0, 2: r_in is 1/S (r_in not read), 0: r_in as given.
int attn_relevance_step_launch(const void* qkv, const float* lse, const void* dout, const float* r_in, float* r_out, int B, int S,
                               int H, int dh, int start, hipStream_t st);
