"""Workload for `rocprofv3 --kernel-trace --stats` of the class-specific relevance ("Attention relevance"), seeded
init, eval mode, 256 frames of cfg B (ViT-Tiny/16 224x224, 12 layers, S 197) and cfg C (raw IQ 2 x 1024, segments of 16,
6 layers, S 65):
1. eval forward alone, and forward + the data-only backward (iq_model_backward_input without IQ_BWD_PARAM_GRADS);
2. forward + iq_model_attention_relevance with the relevance only (L relevance steps), with the CLS-row maps of every layer
   only (L iq_attn_grad_probs rows=1), and with the all-rows maps of every layer only;
3. attention_rollout for comparison.
Prints host-clock times around a device synchronise (launch overhead included)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
import vit_vs_raw_iq_amd._native as N  # noqa: E402
from vit_vs_raw_iq_amd import attention_relevance, attention_rollout  # noqa: E402

CFG = {
    "B": (P.AMCTransformerViT, dict(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192,
                                    n_head=3, n_layers=12, ffn_hidden=768), (1, 224, 224)),
    "C": (P.AMCTransformerRawIQ, dict(in_channels=2, seq_length=1024, num_classes=19, d_model=128, n_head=8, n_layers=6,
                                      ffn_hidden=1024, use_cls_token=True, embedding_type="segment", segment_size=16), (2, 1024)),
}


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def main(reps=10, B=256):
    torch.manual_seed(0)
    d = torch.device("cuda:0")
    st = N.stream_handle()
    for cid, (cls, kw, shape) in CFG.items():
        m = cls(drop_prob=0.1, device="cuda", **kw).to(d).eval()
        plan = m.native_plan()
        plan.ensure(d)
        Lr, H, S = kw["n_layers"], kw["n_head"], plan.S
        x = torch.randn(B, *shape, device=d)
        dl = torch.nn.functional.one_hot(torch.arange(B, device=d) % 19, 19).float()
        dsrc = torch.empty_like(x)
        rel = torch.empty(B, S, device=d)
        cls_maps = torch.empty(B, Lr, S, device=d)
        all_maps = torch.empty(B, Lr, S, S, device=d)
        fwd = lambda: plan.forward(x, False, True, False)  # noqa: E731

        def relevance(out, maps, rows, per_layer):
            ptrs = (ctypes.c_void_p * Lr)()
            for l in range(Lr):
                ptrs[l] = None if maps is None else maps.data_ptr() + 4 * l * per_layer
            fwd()
            N.check(plan.L.iq_model_attention_relevance(plan.h, dl.data_ptr(), B, plan.ws.data_ptr(), plan.ws.numel(),
                                                        None if out is None else out.data_ptr(), ptrs, rows, 1, 1,
                                                        Lr * per_layer, st), "iq_model_attention_relevance", plan.h)

        t_f = timed(fwd, reps)
        t_data = timed(lambda: (fwd(), plan.backward_input(B, dl, None, dsrc)), reps)
        t_rel = timed(lambda: relevance(rel, None, 0, 0), reps)
        t_cls = timed(lambda: relevance(None, cls_maps, 1, S), reps)
        t_all = timed(lambda: relevance(None, all_maps, 0, S * S), reps)
        t_api = timed(lambda: attention_relevance(m, x), reps)
        t_roll = timed(lambda: attention_rollout(m, x), reps)
        print(f"cfg {cid} @ {B} (S {S}, {Lr} layers, {H} heads): eval forward {t_f:.0f} us; forward + data-only backward "
              f"{t_data:.0f} us; forward + relevance ({Lr} steps) {t_rel:.0f} us; forward + CLS-row maps {t_cls:.0f} us; "
              f"forward + all-rows maps {t_all:.0f} us; attention_relevance() {t_api:.0f} us; attention_rollout() {t_roll:.0f} us")
        r0 = attention_relevance(m, x)
        print(f"cfg {cid}: relevance finite {bool(torch.isfinite(r0).all())}, mean excess over the start "
              f"{(r0.sum(1) - 1).mean().item():.4f}")


if __name__ == "__main__":
    main()
