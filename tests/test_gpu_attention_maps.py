"""GPU (MI355X): attention probabilities and attention rollout read back from the fused forward
(csrc/attn_maps.hip, vit_vs_raw_iq_amd.attention_maps).

1. Kernel level, identical inputs: iq_attn_probs after iq_attn_fwd against an fp64 softmax of the same bf16 q, k, and P @ V
   against the forward's own output (the lse and q, k belong together).
2. Model level against the oracle: fp64 probabilities from the oracle's per-layer inputs (O.embed, CLS, PE, O.encoder_layer).
   The loaded state dict's w_q and w_k weights are scaled by W_SCALE in model and oracle alike, so the seeded-init maps are
   peaked enough to tell two frames apart.  Metric: total-variation distance per query row, 0.5 * sum_key |P - P_ref|.
   The error is that of the bf16 plan (activations, q, k), not of the read-back (item 1 checks that to ~1e-6); it is
   concentrated in rows where two keys nearly tie, and it grows with depth.  Measured worst row / median row / median TV
   between the oracle maps of the batch's first two frames, on one MI355X:
     vit_A 0.0196 / 0.0021 / 0.754     vit_ref_L2 0.0323 / 0.0063 / 0.939     vit_tiny224_L2 0.0327 / 0.0065 / 0.964
     rawiq_R 0.0340 / 0.0042 / 0.915   rawiq_nocls 0.0130 / 0.0034 / 0.825    rawiq_conv1d 0.0391 / 0.0069 / 0.944
     rawiq_C_L6 0.0800 / 0.0102 / 0.945
   TV_BOUND holds each fixture's worst row with room (the computation is deterministic), and the test asserts that it is at
   most 1/10 of the frame-to-frame median, so a map of the wrong frame cannot pass.
3. Rollout against an fp64 rollout of the returned maps, and against the oracle's.
4. No interference with training: graph-captured steps around a read-back follow the trajectory without it.
"""
import math

import numpy as np
import pytest
import torch

import iq_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

W_SCALE = 4.0
TV_BOUND = {"vit_A": 0.04, "vit_ref_L2": 0.06, "vit_tiny224_L2": 0.06, "rawiq_R": 0.06, "rawiq_nocls": 0.03,
            "rawiq_conv1d": 0.07, "rawiq_C_L6": 0.09}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(kind, kw, drop=0.0):
    import vit_vs_raw_iq_amd as P
    return (P.AMCTransformerViT if kind == "vit" else P.AMCTransformerRawIQ)(drop_prob=drop, device="cuda", **kw)


# ------------------------------------------------------------------------------------------------------------------------
# 1. kernel level
# ------------------------------------------------------------------------------------------------------------------------
def probs(qkv, lse, B, S, H, dh, rows, heads):
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    hn = 1 if heads else H
    shape = (B, hn, S, S) if rows == 0 else (B, hn, S)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=qkv.device)
    per = out[0].numel()
    N.check(L.iq_attn_probs(qkv.data_ptr(), lse.data_ptr(), out.data_ptr(), per, B, S, H, dh, rows, heads,
                            N.stream_handle()), "iq_attn_probs")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dh", [16, 32, 64])
@pytest.mark.parametrize("S", [1, 5, 65, 128, 129, 197, 1025])
def test_probs_kernel_against_fp64_softmax_of_the_same_inputs(dh, S):
    import vit_vs_raw_iq_amd._native as N
    d = dev()
    L = N.lib()
    B, H = 2, 3
    D = H * dh
    g = torch.Generator().manual_seed(S * 100 + dh)
    qkv = torch.randn(B * S, 3 * D, generator=g).to(torch.bfloat16).to(d)
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=d)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=d)
    N.check(L.iq_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, dh, N.stream_handle()), "iq_attn_fwd")
    P = probs(qkv, lse, B, S, H, dh, 0, 0)
    x = qkv.double().cpu().view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)        # (3, B, H, S, dh)
    q, k, v = x[0], x[1], x[2]
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    Pd = P.double().cpu()
    assert torch.isfinite(Pd).all()
    err = (Pd - ref).abs().max().item()
    assert err <= 1e-4, err
    assert (Pd.sum(-1) - 1).abs().max().item() <= 1e-4
    # P @ V reproduces the forward's output to its bf16 rounding: the lse and q, k belong together
    o = (Pd @ v).permute(0, 2, 1, 3).reshape(B * S, D)
    fo = out.double().cpu()
    assert ((fo - o).abs() <= 2 ** -7 * o.abs() + 4e-3).all(), (fo - o).abs().max().item()
    # the reduced modes are slices / means of the full matrices
    tol = 1e-6
    assert (probs(qkv, lse, B, S, H, dh, 1, 0) - P[:, :, 0, :]).abs().max().item() <= tol
    assert (probs(qkv, lse, B, S, H, dh, 2, 0) - P.mean(2)).abs().max().item() <= tol
    assert (probs(qkv, lse, B, S, H, dh, 0, 1) - P.mean(1, keepdim=True)).abs().max().item() <= tol
    assert (probs(qkv, lse, B, S, H, dh, 1, 1) - P[:, :, 0, :].mean(1, keepdim=True)).abs().max().item() <= tol
    assert (probs(qkv, lse, B, S, H, dh, 2, 1) - P.mean(2).mean(1, keepdim=True)).abs().max().item() <= tol
    assert torch.equal(probs(qkv, lse, B, S, H, dh, 0, 0), P)                 # no atomics: same bits twice
    assert torch.equal(probs(qkv, lse, B, S, H, dh, 2, 1), probs(qkv, lse, B, S, H, dh, 2, 1))


# ------------------------------------------------------------------------------------------------------------------------
# 2. model level against the oracle
# ------------------------------------------------------------------------------------------------------------------------
FIXTURES = ["vit_A", "vit_ref_L2", "vit_tiny224_L2", "rawiq_R", "rawiq_nocls", "rawiq_conv1d", "rawiq_C_L6"]


def scaled_state(kind, kw, z):
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, int(z["seed"]))
    for k in sd:
        if k.endswith(("attention.w_q.weight", "attention.w_k.weight")):
            sd[k] = sd[k] * W_SCALE
    return cfg, sd


def oracle_maps(cfg, sd, x):
    """(B, L, H, S, S) fp64 probabilities from the oracle's per-layer inputs (q, k projected as O.multi_head_attention)."""
    sd = {k: v.double() for k, v in sd.items()}
    h = O.embed(cfg, sd, x.double())
    B, D, H = h.shape[0], cfg.d_model, cfg.n_head
    if cfg.has_cls():
        h = torch.cat([sd["encoder.cls_token"].expand(B, 1, D), h], dim=1)
    S = h.shape[1]
    h = h + sd["encoder.positional_encoding.encoding"][:S].unsqueeze(0)
    out = []
    for i in range(cfg.n_layers):
        pre = f"encoder.layers.{i}."
        a = pre + "attention."
        q = (h @ sd[a + "w_q.weight"].t() + sd[a + "w_q.bias"]).view(B, S, H, D // H).transpose(1, 2)
        k = (h @ sd[a + "w_k.weight"].t() + sd[a + "w_k.bias"]).view(B, S, H, D // H).transpose(1, 2)
        out.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), dim=-1))
        h = O.encoder_layer(sd, pre, h, H)
    return torch.stack(out, 1)


def tv(a, b):
    return 0.5 * (a - b).abs().sum(-1)


def rollout_np(maps_mean, alpha, cls):
    """fp64 rollout of (B, L, 1, S, S) head-mean maps."""
    m = np.asarray(maps_mean, np.float64)[:, :, 0]
    B, L, S, _ = m.shape
    r = np.zeros((B, S)) + (0.0 if cls else 1.0 / S)
    if cls:
        r[:, 0] = 1.0
    eye = np.eye(S)
    for l in range(L - 1, -1, -1):
        r = np.einsum("bq,bqk->bk", r, alpha * m[:, l] + (1 - alpha) * eye)
    return r


def model_and_input(name):
    d = dev()
    kind, kw, z = load_golden(name)
    cfg, sd = scaled_state(kind, kw, z)
    m = build(kind, kw)
    m.load_state_dict(sd)
    m.to(d).eval()
    x = torch.from_numpy(z["x"]).float()
    return m, cfg, sd, x


@pytest.mark.parametrize("name", FIXTURES)
def test_model_maps_match_the_oracle(name):
    from vit_vs_raw_iq_amd import attention_maps, attention_rollout
    m, cfg, sd, x = model_and_input(name)
    d = dev()
    xd = x.to(d)
    full = attention_maps(m, xd, query="all", heads="all")
    B, L, H, S = x.shape[0], cfg.n_layers, cfg.n_head, cfg.seq()
    assert full.shape == (B, L, H, S, S)
    ref = oracle_maps(cfg, sd, x)
    err = tv(full.double().cpu(), ref)
    sep = tv(ref[0], ref[1]).median().item()           # two different frames of the batch
    bound = TV_BOUND[name]
    print(f"{name}: worst row TV {err.max().item():.4f}, median {err.median().item():.4f}, frame-to-frame median {sep:.4f}")
    assert bound <= sep / 10, (bound, sep)
    assert err.max().item() <= bound
    # the reduced modes and a layer subset are slices / means of the full output
    tol = 1e-6
    mean_h = attention_maps(m, xd, query="all", heads="mean")
    assert (mean_h - full.mean(2, keepdim=True)).abs().max().item() <= tol
    assert (attention_maps(m, xd, query="mean", heads="all") - full.mean(3)).abs().max().item() <= tol
    assert (attention_maps(m, xd, query="mean") - full.mean(3).mean(2, keepdim=True)).abs().max().item() <= tol
    if cfg.has_cls():
        assert (attention_maps(m, xd, query="cls", heads="all") - full[:, :, :, 0]).abs().max().item() <= tol
        assert (attention_maps(m, xd) - full[:, :, :, 0].mean(2, keepdim=True)).abs().max().item() <= tol
    sub = [L - 1, 0] if L > 1 else [0]
    assert torch.equal(attention_maps(m, xd, layers=sub, query="all", heads="all"), full[:, sub])
    # chunks of the batch give the frames' own maps (a forward of another batch may pick other GEMM tilings: not bitwise)
    assert tv(attention_maps(m, xd, query="all", heads="all", batch=1), full).max().item() <= bound
    # rollout
    for alpha in (0.5, 1.0):
        roll = attention_rollout(m, xd, alpha=alpha)
        assert roll.shape == (B, S)
        r = roll.double().cpu().numpy()
        exp = rollout_np(mean_h.cpu().numpy(), alpha, cfg.has_cls())
        assert np.abs(r - exp).max() <= 1e-5 * np.abs(exp).max(axis=1).max(), np.abs(r - exp).max()
        assert np.abs(r.sum(1) - 1).max() <= 1e-5
        oref = rollout_np(ref.mean(2, keepdim=True).numpy(), alpha, cfg.has_cls())
        print(f"{name}: rollout alpha {alpha} TV to the oracle's {0.5 * np.abs(r - oref).sum(1).max():.4f}")
        assert 0.5 * np.abs(r - oref).sum(1).max() <= bound
        assert torch.equal(attention_rollout(m, xd, alpha=alpha), roll)
        assert 0.5 * (attention_rollout(m, xd, alpha=alpha, batch=1) - roll).abs().sum(1).max().item() <= bound


def test_encoders_read_back_through_the_plan_their_forward_runs():
    from vit_vs_raw_iq_amd import attention_maps, attention_rollout
    m, cfg, sd, x = model_and_input("rawiq_R")
    xd = x.to(dev())
    full = attention_maps(m, xd, query="all", heads="all")
    assert torch.equal(attention_maps(m.encoder, xd, query="all", heads="all"), full)
    assert m.encoder._plan is None                      # the owner's plan, not a second one
    import vit_vs_raw_iq_amd as P
    kind, kw, z = load_golden("rawiq_R")
    g = {k: v for k, v in kw.items() if k != "num_classes"}
    enc = P.EncoderRawIQ(drop_prob=0.0, device="cuda", **g)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
    enc.to(dev()).eval()
    assert torch.equal(attention_maps(enc, xd, query="all", heads="all"), full)
    assert torch.equal(attention_rollout(enc, xd), attention_rollout(m, xd))


def test_native_entry_points_refuse_a_mismatched_workspace():
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import attention_maps
    m, cfg, sd, x = model_and_input("vit_A")
    plan = m.native_plan()
    L = plan.L
    out = torch.empty(64 * plan.S * plan.S * cfg.n_head, dtype=torch.float32, device=dev())
    st = N.stream_handle()
    plan.ensure(dev())
    ws = plan.workspace(4, dev())
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 4, 0, 0, 0, out.data_ptr(), out.numel(), st) != 0
    assert b"no forward" in L.iq_model_last_error(plan.h)
    attention_maps(m, x[:2].to(dev()))                 # last forward: batch 2
    ws = plan.ws
    bs = cfg.n_head * plan.S * plan.S
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 3, 0, 0, 0, out.data_ptr(), bs, st) != 0
    assert b"batch 2" in L.iq_model_last_error(plan.h)
    assert L.iq_model_attention_rollout(plan.h, ws.data_ptr(), ws.numel(), 3, 0.5, out.data_ptr(), st) != 0
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 2, cfg.n_layers, 0, 0, out.data_ptr(), bs, st) != 0
    assert b"layer" in L.iq_model_last_error(plan.h)
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 2, 0, 3, 0, out.data_ptr(), bs, st) != 0
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 2, 0, 0, 0, out.data_ptr(), bs - 1, st) != 0
    assert L.iq_model_attention(plan.h, ws.data_ptr(), 1024, 2, 0, 0, 0, out.data_ptr(), bs, st) != 0
    assert L.iq_model_attention(plan.h, ws.data_ptr(), ws.numel(), 2, 0, 0, 0, out.data_ptr(), bs, st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# 4. no interference with training
# ------------------------------------------------------------------------------------------------------------------------
def test_read_back_between_graph_steps_leaves_the_training_trajectory_alone():
    from vit_vs_raw_iq_amd import attention_maps
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    d = dev()
    kind, kw, z = load_golden("rawiq_C_L2")              # cfg C geometry at reduced depth
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, 5)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(8, 2, 1024, generator=g).to(d)
    y = torch.randint(0, 19, (8,), generator=g).to(d)
    xe = torch.randn(40, 2, 1024, generator=g).to(d)
    res = []
    for read_back in (False, True):
        m = build(kind, kw, drop=0.2)
        m.load_state_dict(sd)
        m.to(d).train()
        tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3, use_graph=True, dropout_seed=77)
        for _ in range(3):
            tr.step(x, y)
        if read_back:
            small = tr.plan.ws.numel()
            maps = attention_maps(m, xe, query="all", heads="all")     # 40 > 8 frames: the workspace is regrown
            assert tr.plan.ws.numel() > small
            assert torch.isfinite(maps).all()
            assert m.training
        for _ in range(3):
            tr.step(x, y)
        res.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


def test_pending_backward_raises_after_a_read_back():
    from vit_vs_raw_iq_amd import attention_maps
    d = dev()
    kind, kw, z = load_golden("vit_A")
    m = build(kind, kw)
    m.load_state_dict(O.init_state(O.OracleConfig(kind=kind, drop_prob=0.0, **kw), 0))
    m.to(d).train()
    x = torch.from_numpy(z["x"]).float().to(d)
    out = m(x)
    attention_maps(m, x)
    assert m.training
    with pytest.raises(RuntimeError, match="overwritten"):
        out.sum().backward()
