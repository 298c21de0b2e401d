"""GPU (MI355X): class-specific attention relevance and gradient-weighted attention maps (Chefer, Gur & Wolf 2021, eqs. 5-6;
csrc/attn_maps.hip, iq_model_attention_relevance, vit_vs_raw_iq_amd.relevance).

1. Kernel level, identical inputs: iq_attn_grad_probs and iq_attn_relevance_step on the q|k|v and lse iq_attn_fwd used and
   produced, against fp64 torch (softmax(q k^T / sqrt(dh)) * (dO v^T)) of the same bf16 values.
2. Model level against an fp64 restatement of the oracle (O.embed, CLS, PE, the layers of O.encoder_layer with each layer's
   softmax A_l kept through retain_grad, the head of O.model_forward; logit[target].backward()).  The state dict's w_q and w_k
   weights are scaled by W_SCALE as in test_gpu_attention_maps, so attention is not uniform.  Metrics per frame: relative L1
   of the (L, H, S, S) signed maps, and of the relevance beyond its start vector, |r - r_ref|_1 / |r_ref - r_0|_1 (the
   identity part of R is exact and common to every frame and class).  The error is that of the bf16 plan (activations, q, k,
   dO): item 1 checks the read-back itself.  Each bound is at most 1/10 of the frame-to-frame separation of the same metric,
   and two targets' results differ by more than 10 x the bound, so a map of another frame or class cannot pass.
3. Consistency of the modes, the layer subset, chunking, repeated calls; the relevance against an fp64 row rollout of the
   GPU's own all-rows head-mean maps.
4. No side effects: p.grad, training, pending backward, graph-replayed training steps; refusals of the native entry point.
"""
import math

import numpy as np
import pytest
import torch

import iq_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

W_SCALE = 4.0
# relative-L1 bounds per frame (maps, relevance).  Measured worst frame over both targets on one MI355X (maps / relevance):
#   vit_A 0.043 / 0.017   vit_ref_L2 0.033 / 0.031   vit_tiny224_L2 0.050 / 0.044   rawiq_R 0.034 / 0.036
#   rawiq_nocls 0.019 / 0.017   rawiq_conv1d 0.031 / 0.026   rawiq_C_L6 0.064 / 0.037   vit_tiny224_L12 0.145 / 0.088
# The smallest frame-to-frame separations are 1.5 (maps) and 0.44 (relevance, vit_A); the errors grow with depth.
BOUND = {"vit_A": (0.06, 0.03), "vit_ref_L2": (0.05, 0.045), "vit_tiny224_L2": (0.09, 0.08), "rawiq_R": (0.06, 0.06),
         "rawiq_nocls": (0.03, 0.03), "rawiq_conv1d": (0.05, 0.045), "rawiq_C_L6": (0.09, 0.06), "vit_tiny224_L12": (0.18, 0.13)}


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
def grad_probs(qkv, lse, dout, B, S, H, dh, rows, heads, positive):
    import vit_vs_raw_iq_amd._native as N
    hn = 1 if heads else H
    shape = (B, hn, S, S) if rows == 0 else (B, hn, S)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=qkv.device)
    N.check(N.lib().iq_attn_grad_probs(qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), out.data_ptr(), out[0].numel(), B, S, H,
                                       dh, rows, heads, positive, N.stream_handle()), "iq_attn_grad_probs")
    torch.cuda.synchronize()
    return out


def step(qkv, lse, dout, rin, B, S, H, dh):
    import vit_vs_raw_iq_amd._native as N
    out = torch.full_like(rin, float("nan"))
    N.check(N.lib().iq_attn_relevance_step(qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), rin.data_ptr(), out.data_ptr(), B, S,
                                           H, dh, N.stream_handle()), "iq_attn_relevance_step")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dh", [16, 32, 64])
@pytest.mark.parametrize("S", [5, 17, 65, 197, 1025])
def test_kernels_against_fp64_of_the_same_inputs(dh, S):
    import vit_vs_raw_iq_amd._native as N
    d = dev()
    L = N.lib()
    B, H = 2, 3
    D = H * dh
    g = torch.Generator().manual_seed(S * 100 + dh)
    qkv = torch.randn(B * S, 3 * D, generator=g).to(torch.bfloat16).to(d)
    dout = torch.randn(B * S, D, generator=g).to(torch.bfloat16).to(d)
    att = torch.empty(B * S, D, dtype=torch.bfloat16, device=d)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=d)
    N.check(L.iq_attn_fwd(qkv.data_ptr(), att.data_ptr(), lse.data_ptr(), B, S, H, dh, N.stream_handle()), "iq_attn_fwd")
    x = qkv.double().cpu().view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)        # (3, B, H, S, dh)
    q, k, v = x[0], x[1], x[2]
    do = dout.double().cpu().view(B, S, H, dh).transpose(1, 2)
    Pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    dP = do @ v.transpose(-1, -2)
    G = Pr * dP                                                                 # (B, H, S, S)
    tol = 2e-4 * dP.abs().max().item()
    full = {}
    for positive in (0, 1):
        ref = G.clamp_min(0) if positive else G
        full[positive] = grad_probs(qkv, lse, dout, B, S, H, dh, 0, 0, positive)
        got = full[positive].double().cpu()
        assert torch.isfinite(got).all()
        err = (got - ref).abs().max().item()
        assert err <= tol, (positive, err, tol)
        derived = {(1, 0): ref[:, :, 0], (2, 0): ref.mean(2), (0, 1): ref.mean(1, keepdim=True),
                   (1, 1): ref[:, :, 0].mean(1, keepdim=True), (2, 1): ref.mean(2).mean(1, keepdim=True)}
        for (rows, heads), r in derived.items():
            got = grad_probs(qkv, lse, dout, B, S, H, dh, rows, heads, positive).double().cpu()
            assert (got - r).abs().max().item() <= tol, (rows, heads, positive)
        assert torch.equal(grad_probs(qkv, lse, dout, B, S, H, dh, 0, 0, positive), full[positive])    # same bits twice
        assert torch.equal(grad_probs(qkv, lse, dout, B, S, H, dh, 2, 1, positive),
                           grad_probs(qkv, lse, dout, B, S, H, dh, 2, 1, positive))
    assert torch.equal(full[1], full[0].clamp_min(0))
    # the relevance step
    rin = torch.rand(B, S, generator=g, dtype=torch.float64)
    rin[:, 0] += 1.0
    exp = rin + torch.einsum("bq,bhqk->bk", rin, G.clamp_min(0)) / H
    rd = rin.float().to(d)
    r = step(qkv, lse, dout, rd, B, S, H, dh)
    got = r.double().cpu()
    assert torch.isfinite(got).all()
    assert (got - exp).abs().max().item() <= tol * rin.sum(1).max().item()
    own = rin + torch.einsum("bq,bhqk->bk", rd.double().cpu(), full[1].double().cpu()) / H     # the kernel's own maps
    assert (got - own).abs().max().item() <= 1e-5 * own.abs().max().item()
    assert torch.equal(step(qkv, lse, dout, rd, B, S, H, dh), r)
    # overlapping r_in / r_out are refused
    assert L.iq_attn_relevance_step(qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), rd.data_ptr(), rd.data_ptr() + 4, B, S, H,
                                    dh, N.stream_handle()) != 0


# ------------------------------------------------------------------------------------------------------------------------
# 2. model level against the oracle
# ------------------------------------------------------------------------------------------------------------------------
def scaled_state(kind, kw, seed):
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, seed)
    for k in sd:
        if k.endswith(("attention.w_q.weight", "attention.w_k.weight")):
            sd[k] = sd[k] * W_SCALE
    return cfg, sd


def oracle_grad_maps(cfg, sd, x, target):
    """(B, L, H, S, S) fp64 dy/dA_l * A_l, y = logit[target] of each frame, A_l kept with retain_grad."""
    sd = {k: v.double() for k, v in sd.items()}
    h = O.embed(cfg, sd, x.double())
    B, D, H = h.shape[0], cfg.d_model, cfg.n_head
    dh = D // H
    if cfg.has_cls():
        h = torch.cat([sd["encoder.cls_token"].expand(B, 1, D), h], dim=1)
    S = h.shape[1]
    h = (h + sd["encoder.positional_encoding.encoding"][:S].unsqueeze(0)).detach().requires_grad_(True)
    x0, A = h, []
    for i in range(cfg.n_layers):
        pre = f"encoder.layers.{i}."
        a = pre + "attention."

        def lin(t, name):
            return t @ sd[a + name + ".weight"].t() + sd[a + name + ".bias"]
        q, k, v = (lin(h, n).view(B, S, H, dh).transpose(1, 2) for n in ("w_q", "w_k", "w_v"))
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
        p.retain_grad()
        A.append(p)
        o = lin((p @ v).transpose(1, 2).reshape(B, S, D), "w_concat")
        h1 = O.custom_layer_norm(o + h, sd[pre + "norm1.gamma"], sd[pre + "norm1.beta"])
        h = O.custom_layer_norm(O.feed_forward(sd, pre + "ffn.", h1) + h1, sd[pre + "norm2.gamma"], sd[pre + "norm2.beta"])
    feat = h[:, 0] if cfg.has_cls() else h.mean(dim=1)
    if cfg.kind == "vit":
        logits = feat @ sd["mlp_head.weight"].t() + sd["mlp_head.bias"]
    else:
        mean = feat.mean(-1, keepdim=True)
        var = ((feat - mean) ** 2).mean(-1, keepdim=True)
        feat = (feat - mean) / torch.sqrt(var + 1e-5) * sd["mlp_head.0.weight"] + sd["mlp_head.0.bias"]
        logits = feat @ sd["mlp_head.1.weight"].t() + sd["mlp_head.1.bias"]
    logits.gather(1, target.view(-1, 1)).sum().backward()
    assert x0.grad is not None
    return torch.stack([p.grad * p for p in A], 1).detach()


def start(B, S, cls):
    r = np.zeros((B, S)) + (0.0 if cls else 1.0 / S)
    if cls:
        r[:, 0] = 1.0
    return r


def row_rollout(maps_mean, cls):
    """fp64 r <- r (I + A_l), l = L-1 .. 0, of (B, L, 1, S, S) head-mean maps."""
    m = np.asarray(maps_mean, np.float64)[:, :, 0]
    B, L, S, _ = m.shape
    r = start(B, S, cls)
    for l in range(L - 1, -1, -1):
        r = r + np.einsum("bq,bqk->bk", r, m[:, l])
    return r


def rel_l1(a, b, axes):
    return (a - b).abs().sum(axes) / b.abs().sum(axes)


def model_and_input(name):
    d = dev()
    kind, kw, z = load_golden(name)
    cfg, sd = scaled_state(kind, kw, int(z["seed"]))
    m = build(kind, kw)
    m.load_state_dict(sd)
    m.to(d).eval()
    return m, cfg, sd, torch.from_numpy(z["x"]).float()


def check_against_oracle(name, m, cfg, sd, x, target):
    """-> (signed all-rows maps, relevance) of `target`, both checked against the oracle's (and their bounds)"""
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps
    xd = x.to(dev())
    B, S = x.shape[0], cfg.seq()
    full = grad_attention_maps(m, xd, target=target, query="all", heads="all", positive=False)
    assert full.shape == (B, cfg.n_layers, cfg.n_head, S, S)
    rel = attention_relevance(m, xd, target=target)
    assert rel.shape == (B, S)
    ref = oracle_grad_maps(cfg, sd, x, target)
    rref = row_rollout(ref.clamp_min(0).mean(2, keepdim=True).numpy(), cfg.has_cls())
    r0 = start(B, S, cfg.has_cls())
    err_m = rel_l1(full.double().cpu(), ref, (1, 2, 3, 4))
    err_r = np.abs(rel.double().cpu().numpy() - rref).sum(1) / np.abs(rref - r0).sum(1)
    sep_m = rel_l1(ref[1], ref[0], (0, 1, 2, 3)).item()
    sep_r = np.abs(rref[1] - rref[0]).sum() / np.abs(rref[0] - r0[0]).sum()
    bm, br = BOUND[name]
    print(f"{name} target {target.tolist()}: maps worst {err_m.max().item():.4f} frame sep {sep_m:.3f}; "
          f"relevance worst {err_r.max():.4f} frame sep {sep_r:.3f}")
    assert bm <= sep_m / 10 and br <= sep_r / 10, (bm, sep_m, br, sep_r)
    assert err_m.max().item() <= bm
    assert err_r.max() <= br
    return full, rel, ref, rref


FIXTURES = ["vit_A", "vit_ref_L2", "vit_tiny224_L2", "rawiq_R", "rawiq_nocls", "rawiq_conv1d", "rawiq_C_L6"]


@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_the_oracle_and_depends_on_the_class(name):
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps
    m, cfg, sd, x = model_and_input(name)
    B, K = x.shape[0], cfg.num_classes
    ta = torch.arange(B) % K
    tb = (ta + 1 + K // 2) % K
    fa, ra, _, rrefa = check_against_oracle(name, m, cfg, sd, x, ta)
    fb, rb, _, rrefb = check_against_oracle(name, m, cfg, sd, x, tb)
    # class specificity: the two classes' results differ by far more than the bound
    bm, br = BOUND[name]
    r0 = start(B, cfg.seq(), cfg.has_cls())
    assert rel_l1(fa.double(), fb.double(), (1, 2, 3, 4)).min().item() > 10 * bm
    assert (np.abs(ra.double().cpu().numpy() - rb.double().cpu().numpy()).sum(1) / np.abs(rrefb - r0).sum(1)).min() > 10 * br
    # target None: the predicted class of the same forward
    xd = x.to(dev())
    pred = m(xd).argmax(1).cpu()
    assert torch.equal(attention_relevance(m, xd), attention_relevance(m, xd, target=pred))
    assert torch.equal(attention_relevance(m, xd, target=int(ta[0])), attention_relevance(m, xd, target=torch.full((B,), int(ta[0]))))


@pytest.mark.parametrize("name", ["vit_ref_L2", "rawiq_nocls", "rawiq_C_L6"])
def test_modes_subsets_chunks_and_the_relevance_are_consistent(name):
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps, rollout_to_input
    m, cfg, sd, x = model_and_input(name)
    xd = x.to(dev())
    L = cfg.n_layers
    t = torch.arange(x.shape[0]) % cfg.num_classes
    full = grad_attention_maps(m, xd, target=t, query="all", heads="all", positive=False)
    pos = grad_attention_maps(m, xd, target=t, query="all", heads="all")
    assert torch.equal(pos, full.clamp_min(0))
    tol = 1e-6 * max(1.0, full.abs().max().item())
    for positive, f in ((False, full), (True, pos)):
        kw = dict(target=t, positive=positive)
        assert (grad_attention_maps(m, xd, query="all", heads="mean", **kw) - f.mean(2, keepdim=True)).abs().max().item() <= tol
        assert (grad_attention_maps(m, xd, query="mean", heads="all", **kw) - f.mean(3)).abs().max().item() <= tol
        assert (grad_attention_maps(m, xd, query="mean", **kw) - f.mean(3).mean(2, keepdim=True)).abs().max().item() <= tol
        if cfg.has_cls():
            assert (grad_attention_maps(m, xd, query="cls", heads="all", **kw) - f[:, :, :, 0]).abs().max().item() <= tol
            assert (grad_attention_maps(m, xd, **kw) - f[:, :, :, 0].mean(2, keepdim=True)).abs().max().item() <= tol
    sub = [L - 1, 0] if L > 1 else [0]
    assert torch.equal(grad_attention_maps(m, xd, target=t, layers=sub, query="all", heads="all", positive=False), full[:, sub])
    # the relevance is the row rollout of the GPU's own all-rows head-mean positive maps
    rel = attention_relevance(m, xd, target=t)
    own = row_rollout(grad_attention_maps(m, xd, target=t, query="all").cpu().numpy(), cfg.has_cls())
    r = rel.double().cpu().numpy()
    assert np.abs(r - own).max() <= 1e-5 * np.abs(own).max(), np.abs(r - own).max()
    assert torch.equal(attention_relevance(m, xd, target=t), rel)                   # same bits twice
    assert torch.equal(grad_attention_maps(m, xd, target=t, query="all", heads="all", positive=False), full)
    # chunks of the batch stay within the oracle bound (another batch may pick other GEMM tilings: not bitwise)
    bm, br = BOUND[name]
    assert rel_l1(grad_attention_maps(m, xd, target=t, query="all", heads="all", positive=False, batch=1).double(),
                  full.double(), (1, 2, 3, 4)).max().item() <= bm
    r0 = start(x.shape[0], cfg.seq(), cfg.has_cls())
    r1 = attention_relevance(m, xd, target=t, batch=1).double().cpu().numpy()
    assert (np.abs(r1 - r).sum(1) / np.abs(r - r0).sum(1)).max() <= br
    assert rollout_to_input(m, rel).shape[0] == x.shape[0]


@pytest.mark.parametrize("name", ["vit_tiny224_L12", "rawiq_C_L6"])
def test_full_depth_against_the_oracle(name):
    """cfg B (12 layers, S 197) and cfg C (6 layers, S 65)."""
    m, cfg, sd, x = model_and_input(name)
    check_against_oracle(name, m, cfg, sd, x, torch.arange(x.shape[0]) % cfg.num_classes)


# ------------------------------------------------------------------------------------------------------------------------
# 4. side effects and refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_grads_training_and_pending_backward():
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps
    m, cfg, sd, x = model_and_input("vit_A")
    xd = x.to(dev())
    m.train()
    out = m(xd)
    out.sum().backward()
    before = {n: p.grad.clone() for n, p in m.named_parameters()}
    out = m(xd)
    attention_relevance(m, xd)
    grad_attention_maps(m, xd, target=1, query="all")
    assert m.training
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, before[n]), n
    with pytest.raises(RuntimeError, match="overwritten"):
        out.sum().backward()


def test_native_entry_point_refusals():
    import ctypes
    import vit_vs_raw_iq_amd._native as N
    from vit_vs_raw_iq_amd import attention_relevance
    m, cfg, sd, x = model_and_input("vit_A")
    d = dev()
    plan = m.native_plan()
    L = plan.L
    st = N.stream_handle()
    plan.ensure(d)
    ws = plan.workspace(4, d)
    rel = torch.empty(4 * plan.S, dtype=torch.float32, device=d)
    dl = torch.zeros(4, cfg.num_classes, dtype=torch.float32, device=d)
    no_maps = (ctypes.c_void_p * cfg.n_layers)()
    call = lambda ws_ptr, nbytes, b, rows=1, heads=1, maps=None: L.iq_model_attention_relevance(  # noqa: E731
        plan.h, dl.data_ptr(), b, ws_ptr, nbytes, rel.data_ptr(), maps, rows, heads, 1, plan.S, st)
    assert call(ws.data_ptr(), ws.numel(), 4) != 0
    assert b"no forward" in L.iq_model_last_error(plan.h)
    attention_relevance(m, x[:2].to(d))                 # last forward: batch 2
    ws = plan.ws
    assert call(ws.data_ptr(), ws.numel(), 3) != 0
    assert b"batch 2" in L.iq_model_last_error(plan.h)
    other = torch.empty_like(ws)
    assert call(other.data_ptr(), other.numel(), 2) != 0
    assert b"another workspace" in L.iq_model_last_error(plan.h)
    assert call(ws.data_ptr(), 1024, 2) != 0
    assert call(ws.data_ptr(), ws.numel(), 2, rows=3) != 0
    assert b"rows" in L.iq_model_last_error(plan.h)
    assert L.iq_model_attention_relevance(plan.h, dl.data_ptr(), 2, ws.data_ptr(), ws.numel(), None, no_maps, 1, 1, 1, plan.S,
                                          st) != 0
    assert b"NULL" in L.iq_model_last_error(plan.h)
    assert call(ws.data_ptr(), ws.numel(), 2, maps=no_maps) == 0
    torch.cuda.synchronize()


def test_read_back_between_graph_steps_leaves_the_training_trajectory_alone():
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps
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
            rel = attention_relevance(m, xe)                             # 40 > 8 frames: the workspace is regrown
            assert tr.plan.ws.numel() > small
            maps = grad_attention_maps(m, x, target=y, query="all", heads="all")
            assert torch.isfinite(rel).all() and torch.isfinite(maps).all()
            assert m.training
        for _ in range(3):
            tr.step(x, y)
        res.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
