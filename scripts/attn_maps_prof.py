"""Workload for `rocprofv3 --kernel-trace --stats` of the attention read-back ("Attention maps"): cfg B (ViT-Tiny/16
224x224, 12 layers, 3 heads, S = 197) at batch 256, seeded init.  Per repetition: one eval forward of the plan, then
iq_attn_probs of one layer in rows=1 (CLS row) and rows=0 (every row) mode, then one iq_model_attention_rollout.
Prints the host-clock time of each call after a device synchronise, and the bytes the rows=0 call writes."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
import vit_vs_raw_iq_amd._native as N  # noqa: E402


def main(reps=10, B=256, layer=11):
    torch.manual_seed(0)
    d = torch.device("cuda:0")
    m = P.AMCTransformerViT(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192,
                            n_head=3, n_layers=12, ffn_hidden=768, drop_prob=0.1, device="cuda").to(d).eval()
    x = torch.randn(B, 1, 224, 224, device=d)
    plan = m.native_plan()
    S, H = plan.S, 3
    full = torch.empty(B, H, S, S, device=d)
    cls = torch.empty(B, H, S, device=d)
    roll = torch.empty(B, S, device=d)
    st = N.stream_handle()
    t = {"forward": 0.0, "rows1": 0.0, "rows0": 0.0, "rollout": 0.0}

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t[key] += time.perf_counter() - t0

    for i in range(reps + 2):
        if i == 2:
            t = dict.fromkeys(t, 0.0)
        with torch.no_grad():
            timed("forward", lambda: plan.forward(x, False, False, False))
        ws = plan.ws
        timed("rows1", lambda: N.check(plan.L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), B, layer, 1, 0,
                                                                 cls.data_ptr(), H * S, st), "attention", plan.h))
        timed("rows0", lambda: N.check(plan.L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), B, layer, 0, 0,
                                                                 full.data_ptr(), H * S * S, st), "attention", plan.h))
        timed("rollout", lambda: N.check(plan.L.iq_model_attention_rollout(plan.h, ws.data_ptr(), ws.numel(), B, 0.5,
                                                                           roll.data_ptr(), st), "rollout", plan.h))
    for k, v in t.items():
        print(f"{k}: {1e6 * v / reps:.1f} us per call (host clock around a synchronise)")
    print(f"rows=0 writes {full.numel() * 4 / 1e6:.1f} MB; rollout rows sum to 1 within {(roll.sum(1) - 1).abs().max().item():.2e}")


if __name__ == "__main__":
    main()
