"""CPU: tests/chain_ref.py is what it says it is.

  * its LayerNorm backward formula equals torch.autograd of the LayerNorm, in fp64;
  * its stages, composed without rounding and with fixed masks, equal torch.autograd of the layer tail written directly
    (`norm2(drop(ffn(norm1(drop(proj(A)) + R))) + ...)`, encoder_layer.py:24-33, and the next layer's q,k,v projection) to
    1e-10 relative, forward and backward -- which is what entitles tests/test_gpu_chain_dropout_reference.py to use the
    stages as the definition of the kernels' outputs;
  * the mask-injected dropout of the oracle changes nothing but the masks: all-true masks and scale 1 give
    O.loss_and_grads(train=False) bit for bit, and the masks are asked for in the order of the plan's site ids with the
    plan's shapes.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import chain_ref as CR
import iq_oracle as O
from dropout_ref import dropout_scale, keep_mask

REL = 1e-10


def rel_err(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


@pytest.mark.parametrize("M,D", [(1, 8), (5, 128), (37, 192)])
def test_layer_norm_backward_formula_equals_autograd(M, D):
    g = torch.Generator().manual_seed(M * 1000 + D)
    z = (torch.randn(M, D, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(D, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(D, generator=g, dtype=torch.float64).requires_grad_(True)
    dx = torch.randn(M, D, generator=g, dtype=torch.float64)
    x_ref = Fn.layer_norm(z, (D,), gamma, beta, eps=CR.EPS)
    x_ref.backward(dx)
    x, mean, rstd = CR.layer_norm(z.detach(), gamma.detach(), beta.detach())
    assert rel_err(x, x_ref.detach()) <= REL
    assert rel_err(mean, z.detach().mean(-1)) <= REL
    assert rel_err(rstd, 1 / torch.sqrt(z.detach().var(-1, unbiased=False) + CR.EPS)) <= REL
    dz, dgamma, dbeta = CR.layer_norm_bwd(dx, z.detach(), mean, rstd, gamma.detach())
    assert rel_err(dz, z.grad) <= REL
    assert rel_err(dgamma, gamma.grad) <= REL
    assert rel_err(dbeta, beta.grad) <= REL


@pytest.mark.parametrize("M,D,F,p", [(7, 16, 24, 0.25), (33, 24, 40, 0.1), (2, 8, 8, 0.5)])
def test_stages_composed_equal_autograd_of_the_layer_tail(M, D, F, p):
    g = torch.Generator().manual_seed(M + D + F)
    rnd = lambda *shape, s=1.0: torch.randn(*shape, generator=g, dtype=torch.float64) * s
    names = ("Wo", "bo", "g1", "be1", "W1", "b1", "W2", "b2", "g2", "be2", "Wq", "bq")
    w = dict(Wo=rnd(D, D, s=D ** -0.5), bo=rnd(D), g1=torch.rand(D, generator=g, dtype=torch.float64) + 0.5, be1=rnd(D),
             W1=rnd(F, D, s=D ** -0.5), b1=rnd(F), W2=rnd(D, F, s=F ** -0.5), b2=rnd(D),
             g2=torch.rand(D, generator=g, dtype=torch.float64) + 0.5, be2=rnd(D), Wq=rnd(3 * D, D, s=D ** -0.5), bq=rnd(3 * D))
    A, R = rnd(M, D), rnd(M, D)
    gQKV, residual0 = rnd(M, 3 * D), rnd(M, D)
    masks = tuple(torch.rand(M, n, generator=g) >= p for n in (D, F, D))          # fixed masks: any will do
    s = 1.0 / (1.0 - p)
    # the tail written directly, differentiated by autograd
    lw = {k: w[k].clone().requires_grad_(True) for k in names}
    Ar = A.clone().requires_grad_(True)
    drop = lambda t, m: t * m * s
    z1 = drop(Ar @ lw["Wo"].t() + lw["bo"], masks[0]) + R
    x1 = Fn.layer_norm(z1, (D,), lw["g1"], lw["be1"], eps=CR.EPS)
    pre = x1 @ lw["W1"].t() + lw["b1"]
    h = drop(torch.relu(pre), masks[1])
    z2 = drop(h @ lw["W2"].t() + lw["b2"], masks[2]) + x1
    x = Fn.layer_norm(z2, (D,), lw["g2"], lw["be2"], eps=CR.EPS)
    yq = x @ lw["Wq"].t() + lw["bq"]
    loss = (yq * gQKV).sum() + (x * residual0).sum()
    gz2, gpre, gz1, gA, gg2, gb2, gg1, gb1 = torch.autograd.grad(
        loss, [z2, pre, z1, Ar, lw["g2"], lw["be2"], lw["g1"], lw["be1"]])
    # the stages
    fwd = CR.tail_forward(A, R, w, masks, s)
    for k, ref in (("Z1", z1), ("X1", x1), ("H", h), ("Z2", z2), ("X", x), ("Yq", yq)):
        assert rel_err(fwd[k], ref.detach()) <= REL, k
    bwd = CR.tail_backward(fwd, gQKV, residual0, w, masks, s)
    # dy2 / dy are the gradients at the two projections' outputs: mask * s * (gradient at Z2 / Z1)
    for k, ref in (("dz2", gz2), ("dy2", gz2 * masks[2] * s), ("gH", gpre), ("dz", gz1), ("dy", gz1 * masks[0] * s), ("dA", gA),
                   ("dgamma2", gg2), ("dbeta2", gb2), ("dgamma1", gg1), ("dbeta1", gb1)):
        assert rel_err(bwd[k], ref) <= REL, k
    # and the tail is not degenerate: every mask drops something, every gradient is non-zero
    assert all((~m).any() and m.any() for m in masks) and all(bwd[k].abs().max().item() > 0 for k in bwd)


def small_cfgs():
    return [O.OracleConfig(kind="vit", in_channels=1, img_size_h=32, img_size_w=48, patch_size=16, num_classes=5, d_model=16,
                           n_head=2, n_layers=2, ffn_hidden=40, drop_prob=0.2),
            O.OracleConfig(kind="rawiq", in_channels=2, seq_length=64, segment_size=16, num_classes=4, d_model=24, n_head=4,
                           n_layers=3, ffn_hidden=32, drop_prob=0.1)]


def frames(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, cfg.in_channels, cfg.img_size_h, cfg.img_size_w) if cfg.kind == "vit" else (B, cfg.in_channels, cfg.seq_length)
    return torch.randn(*shape, generator=g), torch.randint(0, cfg.num_classes, (B,), generator=g)


@pytest.mark.parametrize("cfg", small_cfgs(), ids=lambda c: c.kind)
def test_injected_dropout_with_all_true_masks_is_the_oracle_without_dropout(cfg, monkeypatch):
    sd = O.init_state(cfg, 3)
    x, y = frames(cfg, 3, 4)
    logits0, loss0, g0 = O.loss_and_grads(cfg, sd, x, y, 0.1, train=False)
    inj = CR.MaskInjector(lambda site, shape: torch.ones(shape, dtype=torch.bool), 1.0)
    monkeypatch.setattr(O, "_dropout", inj)
    logits1, loss1, g1 = O.loss_and_grads(cfg, sd, x, y, 0.1, train=True)
    assert torch.equal(logits0, logits1) and torch.equal(loss0, loss1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    # one mask per site, in the plan's order, with the plan's shapes
    BS, D, F = 3 * cfg.seq(), cfg.d_model, cfg.ffn_hidden
    want = [(0, (BS, D))]
    for l in range(cfg.n_layers):
        want += [(1 + 3 * l, (BS, D)), (2 + 3 * l, (BS, F)), (3 + 3 * l, (BS, D))]
    assert len(inj.calls) == 1 + 3 * cfg.n_layers
    assert inj.calls == want
    # train = False asks for nothing
    inj.calls.clear()
    O.loss_and_grads(cfg, sd, x, y, 0.1, train=False)
    assert inj.calls == []


def test_philox_injector_hands_out_the_host_masks_and_the_quantised_scale():
    seed, step, p = 0x1234_5678_9ABC_DEF0, 77, 0.2
    inj = CR.philox_injector(seed, step, p)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(2, 5, 24, generator=g), torch.randn(2, 5, 24, generator=g), torch.randn(2, 5, 40, generator=g)]
    for site, x in enumerate(xs):
        out = inj(x, p, True)
        keep = torch.from_numpy(np.ascontiguousarray(keep_mask(seed, step, site, p, x.numel()))).view(x.shape)
        assert torch.equal(out, torch.where(keep, x * float(dropout_scale(p)), torch.zeros_like(x)))
        assert 0.0 < keep.float().mean().item() < 1.0
    assert [c[0] for c in inj.calls] == [0, 1, 2]
    assert float(dropout_scale(p)) != 1.0 / (1.0 - p)                  # 13107 / 65536 is not 0.2
    # p = 0: every element kept, scale exactly 1 -- the dropout-off control runs the same code
    inj0 = CR.philox_injector(seed, step, 0.0)
    assert torch.equal(inj0(xs[0], 0.0, True), xs[0])


def test_chunked_mask_is_the_mask():
    seed, step, site, p = 0x9E3779B97F4A7C15, 1_000_003, 5, 0.2
    for n in (1, 13, 8 * CR._CHUNK, 8 * CR._CHUNK + 1, 8 * (2 * CR._CHUNK + 77) + 5):
        assert np.array_equal(CR.keep_mask_chunked(seed, step, site, p, n), keep_mask(seed, step, site, p, n)), n
    assert np.array_equal(CR.keep_mask_chunked(seed, step, site, 0.0, 1001), keep_mask(seed, step, site, 0.0, 1001))
    assert CR.keep_mask_chunked(seed, step, site, 0.0, 1001).all()


@pytest.mark.parametrize("cfg", small_cfgs(), ids=lambda c: c.kind)
def test_injected_masks_change_the_oracle_and_its_gradient_follows_them(cfg, monkeypatch):
    """With real masks the patched oracle is a different function of its weights, and autograd differentiates THAT function:
    a central difference of the loss along the gradient reproduces |g|^2 (fp64 copy of the state)."""
    sd = {k: v.double() for k, v in O.init_state(cfg, 5).items()}
    x, y = frames(cfg, 4, 6)
    x = x.double()
    _, loss_off, _ = O.loss_and_grads(cfg, sd, x, y, 0.1, train=False)
    monkeypatch.setattr(O, "_dropout", CR.philox_injector(9, 2, cfg.drop_prob))
    _, loss_on, grads = O.loss_and_grads(cfg, sd, x, y, 0.1, train=True)
    assert abs(float(loss_on) - float(loss_off)) > 1e-6
    g2 = sum(float(v.pow(2).sum()) for v in grads.values())
    eps = 1e-5 / g2 ** 0.5

    def loss_at(a):
        monkeypatch.setattr(O, "_dropout", CR.philox_injector(9, 2, cfg.drop_prob))
        moved = {k: (v + a * grads[k] if k in grads else v) for k, v in sd.items()}
        return float(O.smoothed_cross_entropy(O.model_forward(cfg, moved, x, True), y, 0.1))

    got = loss_at(eps) - loss_at(-eps)
    assert abs(got - 2 * eps * g2) <= 1e-5 * 2 * eps * g2
