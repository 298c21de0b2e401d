"""GPU (MI355X): gradients with respect to the model input (csrc/embed_dgrad.hip, iq_model_backward_input, iq_linf_step,
vit_vs_raw_iq_amd.saliency / adversarial, x.grad through the autograd surface).

1. iq_embed_dgrad alone against the fp64 autograd of conv2d / conv1d on the same bf16 operands: fp32-accumulation-level
   error, exact zeros where no patch covers the input, padding columns (filled with NaN here) never reach the output, every
   element written (the output starts as NaN), two calls give the same bits.
2. Model input gradients in eval mode against the CPU oracle's autograd (O.model_forward(cfg, sd, x.requires_grad_()), fp64 on
   the fixtures, fp32 at the benchmarked batch),
   loss = sum of each frame's logit of its fixture label.  Metric: relative L2 error ||g - g_ref|| / ||g_ref||, per frame
   (worst frame) and over the batch.  The error is that of the bf16 plan (activations and activation gradients in bf16);
   it grows with depth, and the worst of 256 frames lies further out than the worst of two.  REL_FRAME / REL_TOTAL hold about
   2x the errors measured on one MI355X (worst frame / total):
     vit_A 0.027 / 0.025          vit_ref_L2 0.014 / 0.012      vit_c2_dh32 0.006 / 0.006     vit_tiny224_L12 0.055 / 0.054
     vit_base_L2 0.017 / 0.016    rawiq_R 0.020 / 0.014         rawiq_nocls 0.008 / 0.007     rawiq_conv1d 0.012 / 0.011
     rawiq_C_L6 0.030 / 0.030     rawiq_Cp_L9 0.048 / 0.045
     cfg B @ 256 frames 0.079 / 0.050     cfg C @ 256 frames 0.068 / 0.035
   (The parameter gradients of the same plan are 1.5-3 % off the oracle, tests/test_gpu_model.py; the input gradient is the
   end of the longest chain of bf16 activation gradients.)
3. Bit identity: dsrc with and without IQ_BWD_PARAM_GRADS (also under training-mode dropout), the flat gradient with the flag
   against iq_model_backward(accumulate=0), two calls on one forward, p.grad with and without x.requires_grad.
4. The autograd contract (frozen / trainable models, torch.autograd.grad, the encoder's `enc`, the stand-alone embeddings,
   the src_mask path, create_graph, an unbound gradient buffer, stale workspaces).
5. Saliency and attacks: integrated-gradients completeness, iq_linf_step bit-exact against torch, PGD inside the eps ball,
   FGSM / PGD raise the loss of a trained model, robustness_curve at eps 0, no interference with graph-captured training.
"""
import copy
import math

import numpy as np
import pytest
import torch

import iq_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURES = ["vit_A", "vit_ref_L2", "vit_c2_dh32", "vit_tiny224_L12", "vit_base_L2", "rawiq_R", "rawiq_nocls", "rawiq_conv1d",
            "rawiq_C_L6", "rawiq_Cp_L9"]
REL_FRAME = {"vit_A": 0.055, "vit_ref_L2": 0.03, "vit_c2_dh32": 0.015, "vit_tiny224_L12": 0.11, "vit_base_L2": 0.035,
             "rawiq_R": 0.04, "rawiq_nocls": 0.016, "rawiq_conv1d": 0.025, "rawiq_C_L6": 0.06, "rawiq_Cp_L9": 0.095,
             "B": 0.16, "C": 0.135}
REL_TOTAL = {"vit_A": 0.05, "vit_ref_L2": 0.025, "vit_c2_dh32": 0.012, "vit_tiny224_L12": 0.11, "vit_base_L2": 0.033,
             "rawiq_R": 0.03, "rawiq_nocls": 0.014, "rawiq_conv1d": 0.023, "rawiq_C_L6": 0.06, "rawiq_Cp_L9": 0.09,
             "B": 0.10, "C": 0.07}
FULL = {
    "B": ("vit", dict(in_channels=1, img_size_h=224, img_size_w=224, patch_size=16, num_classes=19, d_model=192,
                      n_head=3, n_layers=12, ffn_hidden=768), 256),
    "C": ("rawiq", dict(in_channels=2, seq_length=1024, num_classes=19, d_model=128, n_head=8, n_layers=6,
                        ffn_hidden=1024, use_cls_token=True, embedding_type="segment", segment_size=16), 256),
}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(kind, kw, drop=0.0):
    import vit_vs_raw_iq_amd as P
    return (P.AMCTransformerViT if kind == "vit" else P.AMCTransformerRawIQ)(drop_prob=drop, device="cuda", **kw)


def model_and_state(name, seed=0, drop=0.0):
    kind, kw, z = load_golden(name)
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, seed)
    m = build(kind, kw, drop)
    m.load_state_dict(sd)
    return kind, kw, z, cfg, sd, m.to(dev())


def rel_errors(g, r):
    g, r = g.detach().cpu().double().flatten(1), r.detach().double().flatten(1)
    per = ((g - r).norm(dim=1) / r.norm(dim=1)).max().item()
    return per, ((g - r).norm() / r.norm()).item()


# ------------------------------------------------------------------------------------------------------------------------
# 1. kernel level
# ------------------------------------------------------------------------------------------------------------------------
EMB_CASES = [  # kind, B, C, H (L), W, p, D
    (0, 3, 1, 32, 32, 16, 128),      # vit_A geometry, P 256
    (0, 2, 2, 16, 48, 8, 64),        # C = 2, P 128
    (0, 2, 1, 224, 224, 16, 768),    # ViT-Base: D 768
    (0, 2, 3, 36, 40, 16, 192),      # uncovered tails in H and W, P 768 (three column chunks)
    (0, 2, 1, 35, 70, 4, 64),        # P 16 (VALU path) with tails
    (0, 2, 2, 32, 32, 4, 16),        # D 16 < one K step of 32
    (1, 3, 2, 1024, 0, 64, 128),     # raw-IQ segments, P 128
    (1, 2, 2, 1024, 0, 1, 128),      # raw-IQ conv1d, P 2
    (1, 2, 2, 1000, 0, 16, 256),     # L % p != 0
    (1, 300, 2, 1024, 0, 16, 128),   # cfg C geometry, 300 frames: ragged last row tile
]


def embed_dgrad(demb, w, Kpad, kind, B, C, H, W, p, D):
    import vit_vs_raw_iq_amd._native as N
    out = torch.full((B, C, H, W) if kind == 0 else (B, C, H), float("nan"), dtype=torch.float32, device=demb.device)
    N.check(N.lib().iq_embed_dgrad(demb.data_ptr(), w.data_ptr(), Kpad, out.data_ptr(), kind, B, C, H, W, p, D,
                                   N.stream_handle()), "iq_embed_dgrad")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", EMB_CASES, ids=lambda c: "k%d_B%d_C%d_%dx%d_p%d_D%d" % c)
def test_embed_dgrad_kernel_against_fp64_conv_autograd(case):
    kind, B, C, H, W, p, D = case
    d = dev()
    P = C * p * p if kind == 0 else C * p
    Kpad = (P + 31) // 32 * 32
    gh, gw = (H // p, W // p) if kind == 0 else (1, H // p)
    tok = gh * gw
    g = torch.Generator().manual_seed(sum(case))
    demb = torch.randn(B * tok, D, generator=g).to(torch.bfloat16)
    w = torch.randn(D, Kpad, generator=g).to(torch.bfloat16)
    w[:, P:] = float("nan")                                   # the padding columns must never reach the output
    got = embed_dgrad(demb.to(d), w.to(d), Kpad, kind, B, C, H, W, p, D)
    again = embed_dgrad(demb.to(d), w.to(d), Kpad, kind, B, C, H, W, p, D)
    assert torch.equal(got, again)
    wd = w[:, :P].double()
    gout = demb.double().view(B, gh, gw, D).permute(0, 3, 1, 2) if kind == 0 else demb.double().view(B, tok, D).permute(0, 2, 1)
    if kind == 0:
        x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(x, wd.view(D, C, p, p), stride=p).backward(gout)
    else:
        x = torch.zeros(B, C, H, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv1d(x, wd.view(D, C, p), stride=p).backward(gout)
    ref = x.grad
    gc = got.cpu().double()
    assert torch.isfinite(gc).all()
    err = (gc - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)                  # fp32 accumulation (bf16 rounding would be ~4e-3)
    if kind == 0:
        assert torch.equal(got[:, :, gh * p:, :].cpu(), torch.zeros_like(got[:, :, gh * p:, :].cpu()))
        assert torch.equal(got[:, :, :, gw * p:].cpu(), torch.zeros_like(got[:, :, :, gw * p:].cpu()))
    else:
        assert torch.equal(got[:, :, gw * p:].cpu(), torch.zeros_like(got[:, :, gw * p:].cpu()))


# ------------------------------------------------------------------------------------------------------------------------
# 2. model input gradients against the oracle
# ------------------------------------------------------------------------------------------------------------------------
def oracle_input_grad(cfg, sd, x, y):
    xr = x.clone().double().requires_grad_()
    sdd = {k: v.double() for k, v in sd.items()}
    O.model_forward(cfg, sdd, xr).gather(1, y[:, None]).sum().backward()
    return xr.grad


@pytest.mark.parametrize("name", FIXTURES)
def test_model_input_gradient_matches_oracle(name):
    kind, kw, z, cfg, sd, m = model_and_state(name)
    d = dev()
    m.eval().requires_grad_(False)
    x = torch.from_numpy(z["x"]).float()
    y = torch.from_numpy(z["y"]).long()
    xd = x.to(d).requires_grad_()
    m(xd).gather(1, y.to(d)[:, None]).sum().backward()
    assert all(p.grad is None for p in m.parameters())
    ref = oracle_input_grad(cfg, sd, x, y)
    per, tot = rel_errors(xd.grad, ref)
    print(f"{name}: input-gradient rel L2 err worst frame {per:.4f}, total {tot:.4f}")
    assert per <= REL_FRAME[name] and tot <= REL_TOTAL[name], (per, tot)
    from vit_vs_raw_iq_amd import input_gradient
    sal = input_gradient(m, x.to(d), target=y)
    assert torch.equal(sal, xd.grad)                     # the same native chain, whichever way it is reached


@pytest.mark.parametrize("cid", ["B", "C"])
def test_benchmarked_batch_input_gradient_matches_oracle(cid):
    """At 256 frames the one-launch chain backward and the deferred q,k,v data gradient lie on the tested path."""
    d = dev()
    kind, kw, B = FULL[cid]
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, 5)
    m = build(kind, kw)
    m.load_state_dict(sd)
    m.to(d).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(6)
    shape = (B, kw["in_channels"], kw["img_size_h"], kw["img_size_w"]) if kind == "vit" else (B, kw["in_channels"], kw["seq_length"])
    x = torch.randn(*shape, generator=g)
    y = torch.randint(0, kw["num_classes"], (B,), generator=g)
    xd = x.to(d).requires_grad_()
    m(xd).gather(1, y.to(d)[:, None]).sum().backward()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    xr = x.clone().requires_grad_()
    O.model_forward(cfg, sd, xr).gather(1, y[:, None]).sum().backward()
    per, tot = rel_errors(xd.grad, xr.grad)
    print(f"{cid}@{B}: input-gradient rel L2 err worst frame {per:.4f}, total {tot:.4f}")
    assert per <= REL_FRAME[cid] and tot <= REL_TOTAL[cid], (per, tot)


# ------------------------------------------------------------------------------------------------------------------------
# 3. bit identity
# ------------------------------------------------------------------------------------------------------------------------
def native_forward(plan, x, training, step):
    """iq_model_forward with a fixed dropout step (plan.forward advances it)."""
    import vit_vs_raw_iq_amd._native as N
    plan.ensure(x.device)
    B = x.shape[0]
    ws = plan.workspace(B, x.device)
    logits = torch.empty(B, plan.cfg.num_classes, dtype=torch.float32, device=x.device)
    plan.generation += 1
    N.check(plan.L.iq_model_forward(plan.h, N.ptr(x), B, N.ptr(ws), ws.numel(), 1 if training else 0, 1234, step, None,
                                    N.ptr(logits), N.stream_handle()), "iq_model_forward", plan.h)
    return logits


@pytest.mark.parametrize("name,training", [("vit_A", False), ("vit_A", True), ("rawiq_R", True), ("rawiq_C_L6", True)])
def test_input_gradient_bits_do_not_depend_on_the_parameter_gradients(name, training):
    kind, kw, z, cfg, sd, m = model_and_state(name, drop=0.2)
    d = dev()
    plan = m.native_plan()
    x = torch.from_numpy(z["x"]).float().to(d)
    B = x.shape[0]
    dl = torch.randn(B, kw["num_classes"], generator=torch.Generator().manual_seed(3)).to(d)
    res = []
    for flags in (0, 1, 0, 1, "full"):
        native_forward(plan, x, training, 7)
        gflat = torch.zeros_like(plan.flat)
        ds = torch.full_like(x, float("nan"))
        if flags == "full":
            plan.backward(B, dl, None, gflat)
        else:
            plan.backward_input(B, dl, None, ds, gflat if flags else None)
        torch.cuda.synchronize()
        res.append((ds, gflat))
    assert torch.isfinite(res[0][0]).all()
    for i in (1, 2, 3):
        assert torch.equal(res[i][0], res[0][0]), i             # dsrc: with / without the flag, and on a second call
    assert torch.equal(res[1][1], res[4][1]) and torch.equal(res[3][1], res[4][1])   # the flat gradient of iq_model_backward
    assert not res[0][1].any() and not res[2][1].any()         # without the flag nothing was written


def test_parameter_gradients_do_not_depend_on_x_requires_grad():
    kind, kw, z, cfg, sd, m = model_and_state("rawiq_R")
    d = dev()
    x = torch.from_numpy(z["x"]).float().to(d)
    y = torch.from_numpy(z["y"]).long().to(d)
    m.eval()
    grads = []
    for need_x in (False, True):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(need_x)
        torch.nn.functional.cross_entropy(m(xi), y).backward()
        assert (xi.grad is not None) == need_x
        grads.append([p.grad.clone() for p in m.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------
# 4. autograd contract
# ------------------------------------------------------------------------------------------------------------------------
def test_frozen_and_trainable_models_and_autograd_grad():
    kind, kw, z, cfg, sd, m = model_and_state("vit_A")
    d = dev()
    x = torch.from_numpy(z["x"]).float().to(d)
    y = torch.from_numpy(z["y"]).long().to(d)
    m.eval().requires_grad_(False)
    xf = x.clone().requires_grad_()
    torch.nn.functional.cross_entropy(m(xf), y).backward()
    assert xf.grad is not None and all(p.grad is None for p in m.parameters())
    assert m._plan.gflat is None                               # no gradient buffer was ever bound
    m.requires_grad_(True)
    xt = x.clone().requires_grad_()
    torch.nn.functional.cross_entropy(m(xt), y).backward()
    assert torch.equal(xt.grad, xf.grad)
    assert all(p.grad is not None for p in m.parameters())
    xa = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(torch.nn.functional.cross_entropy(m(xa), y), xa)
    assert torch.equal(gx, xf.grad)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(torch.nn.functional.cross_entropy(m(xa), y), xa, create_graph=True)
    out = m(xa)
    m(x)
    with pytest.raises(RuntimeError, match="overwritten"):
        out.sum().backward()


@pytest.mark.parametrize("name", ["vit_c2_dh32", "rawiq_nocls"])
def test_encoder_output_gradient_matches_oracle(name):
    kind, kw, z, cfg, sd, m = model_and_state(name)
    d = dev()
    m.eval().requires_grad_(False)
    x = torch.from_numpy(z["x"]).float()
    S = m.native_plan().S
    w = torch.randn(x.shape[0], S, kw["d_model"], generator=torch.Generator().manual_seed(4))
    xr = x.clone().double().requires_grad_()
    (O.encoder_forward(cfg, {k: v.double() for k, v in sd.items()}, xr) * w.double()).sum().backward()
    alone = copy.deepcopy(m.encoder)                           # a stand-alone encoder with its own plan
    for enc in (m.encoder, alone):
        xd = x.to(d).requires_grad_()
        (enc(xd) * w.to(d)).sum().backward()
        per, tot = rel_errors(xd.grad, xr.grad)
        assert per <= 0.03 and tot <= 0.03, (per, tot)
    assert alone._plan is not None


@pytest.mark.parametrize("name", ["vit_ref_L2", "vit_c2_dh32", "rawiq_R", "rawiq_conv1d"])
def test_standalone_embedding_input_gradient(name):
    kind, kw, z, cfg, sd, m = model_and_state(name)
    d = dev()
    emb = m.encoder.patch_embedding if kind == "vit" else m.encoder.sequence_embedding
    x = torch.from_numpy(z["x"]).float().to(d)
    conv = torch.nn.functional.conv2d if kind == "vit" else torch.nn.functional.conv1d
    wt, bt = emb.projection.weight, emb.projection.bias
    k = wt.shape[-1]
    wg = []
    for need_x in (False, True):
        emb.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(need_x)
        out = emb(xi)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(d)
        (out * gout).sum().backward()
        wg.append((wt.grad.clone(), bt.grad.clone()))
    assert torch.equal(wg[0][0], wg[1][0]) and torch.equal(wg[0][1], wg[1][1])     # weight / bias gradients as before
    xr = x.clone().requires_grad_()
    ref = conv(xr, wt.detach(), bt.detach(), stride=k)
    ref = ref.flatten(2).transpose(1, 2)
    (ref * gout).sum().backward()
    per, tot = rel_errors(xi.grad, xr.grad.cpu())
    assert per <= 1.5e-2 and tot <= 1.5e-2, (per, tot)        # bf16 operands (gradient and weight), fp32 accumulation


@pytest.mark.parametrize("name", ["vit_A", "rawiq_R"])
def test_src_mask_path_input_gradient_matches_oracle_layers(name):
    kind, kw, z, cfg, sd, m = model_and_state(name)
    d = dev()
    m.eval().requires_grad_(False)
    x = torch.from_numpy(z["x"]).float()
    S = m.native_plan().S
    mask = torch.ones(1, 1, S, S)
    mask[..., S - 1] = 0                                       # every query ignores the last key
    w = torch.randn(x.shape[0], S, kw["d_model"], generator=torch.Generator().manual_seed(5))
    xd = x.to(d).requires_grad_()
    (m.encoder(xd, src_mask=mask.to(d)) * w.to(d)).sum().backward()
    xr = x.clone().requires_grad_()
    h = O.embed(cfg, sd, xr)
    if cfg.has_cls():
        h = torch.cat([sd["encoder.cls_token"].expand(h.shape[0], 1, cfg.d_model), h], dim=1)
    h = h + sd["encoder.positional_encoding.encoding"][:S].unsqueeze(0)
    for i in range(cfg.n_layers):
        h = O.encoder_layer(sd, f"encoder.layers.{i}.", h, cfg.n_head, mask=mask)
    (h * w).sum().backward()
    per, tot = rel_errors(xd.grad, xr.grad)
    assert per <= 0.04 and tot <= 0.04, (per, tot)


def test_stale_workspace_and_batch_are_refused():
    import vit_vs_raw_iq_amd as P
    import vit_vs_raw_iq_amd._native as N
    kind, kw, z, cfg, sd, m = model_and_state("vit_A")
    d = dev()
    plan = m.native_plan()
    x = torch.from_numpy(z["x"]).float().to(d)
    B = x.shape[0]
    plan.forward(x, False, True, False)
    dl = torch.ones(B, kw["num_classes"], device=d)
    ds = torch.empty_like(x)
    with pytest.raises(P.IqError, match="batch"):
        plan.backward_input(B - 1, dl[:B - 1], None, ds[:B - 1])
    other = torch.empty_like(plan.ws)
    with pytest.raises(P.IqError, match="another workspace"):
        N.check(plan.L.iq_model_backward_input(plan.h, N.ptr(dl), None, B, N.ptr(other), other.numel(), N.ptr(ds), 0,
                                               N.stream_handle()), "iq_model_backward_input", plan.h)
    assert plan.gflat is None
    with pytest.raises(P.IqError, match="gradient buffer"):            # IQ_BWD_PARAM_GRADS on a plan bound without one
        N.check(plan.L.iq_model_backward_input(plan.h, N.ptr(dl), None, B, N.ptr(plan.ws), plan.ws.numel(), N.ptr(ds), 1,
                                               N.stream_handle()), "iq_model_backward_input", plan.h)
    plan.backward_input(B, dl, None, ds)                       # the right workspace and batch still work
    torch.cuda.synchronize()
    assert torch.isfinite(ds).all()


# ------------------------------------------------------------------------------------------------------------------------
# 5. saliency and attacks
# ------------------------------------------------------------------------------------------------------------------------
IG_TOL = 0.012     # |sum(attr) - (logit(x) - logit(baseline))| / max(|logit(x) - logit(baseline)|, 1); measured 0.0056 / 0.0049
                   # (vit_A / rawiq_R, 64 steps)


@pytest.mark.parametrize("name", ["vit_A", "rawiq_R"])
def test_integrated_gradients_completeness(name):
    from vit_vs_raw_iq_amd import integrated_gradients
    kind, kw, z, cfg, sd, m = model_and_state(name)
    d = dev()
    m.train()
    x = torch.from_numpy(z["x"]).float().to(d)
    base = torch.zeros_like(x[0])
    attr = integrated_gradients(m, x, baseline=base, steps=64, batch=48)
    assert m.training and attr.shape == x.shape
    m.eval()
    with torch.no_grad():
        lx, lb = m(x), m(base.expand_as(x).contiguous())
    t = lx.argmax(1)
    diff = (lx - lb).gather(1, t[:, None])[:, 0]
    err = ((attr.flatten(1).sum(1) - diff).abs() / diff.abs().clamp(min=1.0)).max().item()
    print(f"{name}: integrated-gradients completeness error {err:.4g}")
    assert err <= IG_TOL


def test_linf_step_is_bit_exact_against_torch():
    import vit_vs_raw_iq_amd._native as N
    d = dev()
    g = torch.Generator().manual_seed(11)
    n = 100003
    x0 = torch.randn(n, generator=g).to(d)
    grad = torch.randn(n, generator=g).to(d)
    grad[::7] = 0.0
    x = (x0 + 0.01 * torch.randn(n, generator=g).to(d)).contiguous()
    alpha, eps = float(np.float32(0.0123)), float(np.float32(0.05))
    for lo, hi in ((math.nan, math.nan), (-0.5, 0.75), (math.nan, 0.2), (-0.1, math.nan)):
        xa = x.clone()
        N.check(N.lib().iq_linf_step(xa.data_ptr(), grad.data_ptr(), x0.data_ptr(), alpha, eps, lo, hi, n, N.stream_handle()),
                "iq_linf_step")
        ref = torch.minimum(torch.maximum(x + alpha * grad.sign(), x0 - eps), x0 + eps)
        if lo == lo:
            ref = ref.clamp(min=lo)
        if hi == hi:
            ref = ref.clamp(max=hi)
        assert torch.equal(xa, ref), (lo, hi)


def trained_rawiq():
    """A small raw-IQ classifier trained on four classes of the synthetic task (data.py) at 8 dB."""
    from vit_vs_raw_iq_amd import data as D
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    d = dev()
    X, Y, _ = D.make_dataset(640, seed=3, classes=["BPSK", "QPSK", "16QAM", "OOK"], snrs_db=(8.0,), n_symbols=1024)
    mean, std = D.zscore_stats(X)
    x = torch.from_numpy(D.to_rawiq(X, mean, std)).float().to(d)
    y = torch.from_numpy(Y).long().to(d)
    torch.manual_seed(0)
    m = build("rawiq", dict(in_channels=2, seq_length=1024, num_classes=4, d_model=64, n_head=4, n_layers=2, ffn_hidden=128,
                            use_cls_token=True, embedding_type="segment", segment_size=64)).to(d)
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3)
    for epoch in range(6):
        for i in range(0, 512, 64):
            tr.step(x[i:i + 64], y[i:i + 64])
    return m.eval(), x[512:], y[512:]


def test_attacks_raise_the_loss_of_a_trained_model_and_the_curve_starts_at_the_clean_accuracy():
    from vit_vs_raw_iq_amd import fgsm, pgd, robustness_curve
    m, x, y = trained_rawiq()
    F = torch.nn.functional

    def ce(xs):
        with torch.no_grad():
            return F.cross_entropy(m(xs), y).item()
    eps = 0.05
    clean = ce(x)
    xf = fgsm(m, x, y, eps)
    xp = pgd(m, x, y, eps, alpha=eps / 4, steps=10)
    xr = pgd(m, x, y, eps, alpha=eps / 4, steps=10, random_start=True, seed=3)
    for xa in (xf, xp, xr):
        assert ((xa >= x - eps) & (xa <= x + eps)).all()      # inside the eps ball, exactly (the step's own fp32 bounds)
    lf, lp = ce(xf), ce(xp)
    print(f"trained raw-IQ: CE clean {clean:.4f}, FGSM {lf:.4f}, PGD-10 {lp:.4f} at eps {eps}")
    assert lf >= clean and lp >= clean
    assert lp >= lf - 0.02 * lf                                 # PGD (10 steps of eps/4) at least FGSM, 2 % slack
                                                                # (measured: CE clean 0.852, FGSM 1.442, PGD-10 1.491 at eps 0.05)
    with torch.no_grad():
        acc = (m(x).argmax(1) == y).float().mean().item()
    assert robustness_curve(m, x, y, [0.0]) == [acc]
    curve = robustness_curve(m, x, y, [0.0, eps, 4 * eps], attack="pgd", steps=5)
    assert curve[0] == acc and curve[2] <= curve[0]
    assert not m.training


def test_saliency_and_attack_between_graph_steps_leave_the_training_trajectory_alone():
    from vit_vs_raw_iq_amd import input_gradient, pgd
    from vit_vs_raw_iq_amd.trainer import FusedTrainer
    d = dev()
    kind, kw, z = load_golden("rawiq_C_L2")
    cfg = O.OracleConfig(kind=kind, drop_prob=0.0, **kw)
    sd = O.init_state(cfg, 5)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(8, 2, 1024, generator=g).to(d)
    y = torch.randint(0, 19, (8,), generator=g).to(d)
    xe = torch.randn(40, 2, 1024, generator=g).to(d)
    ye = torch.randint(0, 19, (40,), generator=g).to(d)
    res = []
    for probe in (False, True):
        m = build(kind, kw, drop=0.2)
        m.load_state_dict(sd)
        m.to(d).train()
        tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-3, use_graph=True, dropout_seed=77)
        for _ in range(3):
            tr.step(x, y)
        if probe:
            small = tr.plan.ws.numel()
            sal = input_gradient(m, xe)                          # 40 > 8 frames: the workspace is regrown
            adv = pgd(m, xe, ye, 0.1, 0.05, 3)
            assert tr.plan.ws.numel() > small
            assert torch.isfinite(sal).all() and torch.isfinite(adv).all()
            assert m.training
        for _ in range(3):
            tr.step(x, y)
        res.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
