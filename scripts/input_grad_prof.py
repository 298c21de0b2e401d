"""Workload for `rocprofv3 --kernel-trace --stats` of the input gradient ("Input gradients"), seeded init, eval mode:
1. iq_embed_dgrad alone at 256 frames on the embedding geometries of cfg B (ViT-Tiny/16 224x224, D 192), cfg C (raw IQ 2 x 1024,
   segments of 16, D 128) and cfg D (ViT-Base/16 224x224, D 768);
2. cfg B and cfg C at 256 frames: forward + the full backward (iq_model_backward) against forward + the data-only backward
   (iq_model_backward_input without IQ_BWD_PARAM_GRADS) and with it;
3. one PGD step (forward, iq_ce_fwd_bwd, data-only backward, iq_linf_step) per frame at cfg B and cfg C.
Prints host-clock times around a device synchronise (launch overhead included) and the bytes iq_embed_dgrad moves."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vit_vs_raw_iq_amd as P  # noqa: E402
import vit_vs_raw_iq_amd._native as N  # noqa: E402
from vit_vs_raw_iq_amd.adversarial import pgd  # noqa: E402

CFG = {
    "B": (P.AMCTransformerViT, dict(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192,
                                    n_head=3, n_layers=12, ffn_hidden=768)),
    "C": (P.AMCTransformerRawIQ, dict(in_channels=2, seq_length=1024, num_classes=19, d_model=128, n_head=8, n_layers=6,
                                      ffn_hidden=1024, use_cls_token=True, embedding_type="segment", segment_size=16)),
}
EMB = {"B": (0, 1, 224, 224, 16, 192), "C": (1, 2, 1024, 0, 16, 128), "D": (0, 1, 224, 224, 16, 768)}


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
    L = N.lib()
    st = N.stream_handle()
    for cid, (kind, C, H, W, p, D) in EMB.items():
        Pn = C * p * p if kind == 0 else C * p
        Kpad = (Pn + 31) // 32 * 32
        tok = (H // p) * (W // p) if kind == 0 else H // p
        demb = torch.randn(B * tok, D, device=d).to(torch.bfloat16)
        w = torch.randn(D, Kpad, device=d).to(torch.bfloat16)
        out = torch.empty((B, C, H, W) if kind == 0 else (B, C, H), device=d)
        us = timed(lambda: N.check(L.iq_embed_dgrad(demb.data_ptr(), w.data_ptr(), Kpad, out.data_ptr(), kind, B, C, H, W, p, D,
                                                    st), "iq_embed_dgrad"), reps)
        mb = (demb.numel() * 2 + w.numel() * 2 + out.numel() * 4) / 1e6
        print(f"embed_dgrad cfg {cid}: {us:.1f} us per call (host clock), moves {mb:.1f} MB "
              f"(reads {demb.numel() * 2 / 1e6:.1f} MB demb + {w.numel() * 2 / 1e3:.0f} KB W, writes {out.numel() * 4 / 1e6:.1f} MB)")
    for cid, (cls, kw) in CFG.items():
        m = cls(drop_prob=0.1, device="cuda", **kw).to(d).eval()
        plan = m.native_plan()
        plan.ensure(d)
        shape = (B, 1, 224, 224) if cid == "B" else (B, 2, 1024)
        x = torch.randn(*shape, device=d)
        y = torch.randint(0, 19, (B,), device=d)
        dl = torch.randn(B, 19, device=d)
        gflat = torch.zeros_like(plan.flat)
        dsrc = torch.empty_like(x)
        fwd = lambda: plan.forward(x, False, True, False)  # noqa: E731
        t_f = timed(fwd, reps)
        t_full = timed(lambda: (fwd(), plan.backward(B, dl, None, gflat)), reps)
        t_data = timed(lambda: (fwd(), plan.backward_input(B, dl, None, dsrc)), reps)
        t_both = timed(lambda: (fwd(), plan.backward_input(B, dl, None, dsrc, gflat)), reps)
        print(f"cfg {cid} @ {B}: forward {t_f:.0f} us; forward + backward: full (iq_model_backward) {t_full:.0f} us, "
              f"data-only (iq_model_backward_input, flags 0) {t_data:.0f} us, with IQ_BWD_PARAM_GRADS {t_both:.0f} us")
        t_pgd = timed(lambda: pgd(m, x, y, 0.05, 0.0125, 10), max(2, reps // 4))
        print(f"cfg {cid} @ {B}: PGD 10 steps {t_pgd:.0f} us = {t_pgd / 10 / B:.2f} us per step per frame")


if __name__ == "__main__":
    main()
