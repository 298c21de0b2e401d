"""GPU (MI355X): the kernels of csrc/misc.hip at both ends of the model -- class-token rows, the embedding backward
gather, the classifier head, label-smoothed cross entropy, gradient norm, clip + AdamW, the casts and patchify -- at
every branch their launchers take, through the C ABI, against plain fp64 (or bit-exact) references.

Launch branches and the cases that reach them:
  ce_kernel<0> (K > 32) ................. test_head_fwd_ce_bwd_branches K = 33, 53, 64; test_ce_alone K = 33, 64
  ce_kernel<32> with B > 256 ............ test_head_fwd_ce_bwd_branches (300, 9, 192, 19); test_ce_alone (300, 5)
  head_bwd_w_kernel (K > 32) ............ test_head_fwd_ce_bwd_branches K = 33, 53, 64, with and without the head LayerNorm
  head_bwd_w2_kernel (K <= 32) .......... test_head_fwd_ce_bwd_branches K = 1, 3, 8, 19, 32
  head forward serial fallback .......... D = 1048
  head forward kpar = 1 / 2 / 4 / 8 ..... D = 256, 768 / 136, 192 / 64 / 32
  dcls_kernel frame loop (B > 256) ...... test_embed_bwd_gather (300, 3, 2, 192, 1)
  AdamW grid-stride loop ................ test_clip_adamw_against_fp64 n = 2,500,000
  gradient-norm n & 3 tail .............. test_gradnorm_sq n = 1, 7, 100003
  cast n & 3 tail ....................... test_cast_bf16 n = 1, 3, 1001, 1002, 1003, 2100001

Dropout-on cases use the host mask of tests/dropout_ref.py; test_device_mask_equals_host_mask is what entitles them to.

Tolerances are those tests/test_gpu_kernels.py states for the same kind of output (close_bf16, close_f32 and their
arguments are imported from there); the few it has no counterpart for are derived where they are used.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dropout_ref import dropout_scale, keep_groups, keep_mask
from test_gpu_kernels import L, _N, _drop, bf, close_bf16, close_f32, dev, run_gemm, stream  # noqa: F401  (L is a fixture)

pytestmark = pytest.mark.gpu

ERR_ARG = 1
SEED_HI = 0x9E3779B97F4A7C15            # non-zero high word: the key's second half


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def scale_t(p):
    """dropout_scale(p) as an fp32 device scalar, so `x.float() * scale_t(p)` is the kernel's one fp32 product."""
    return torch.tensor(float(dropout_scale(p)), dtype=torch.float32, device=dev())


# ------------------------------------------------------------------------------------------------
# 1. the device mask is the host mask
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(130, 192), (77, 64), (1, 128)])
@pytest.mark.parametrize("seed,step,site,p,step_on_device", [(123, 7, 4, 0.25, False), (SEED_HI, 1_000_003, 2, 0.1, False),
                                                             (SEED_HI, 41, 0, 0.5, True)])
def test_device_mask_equals_host_mask(L, M, D, seed, step, site, p, step_on_device):
    """Identity probe: ones x I through the GEMM epilogue leaves scale where an element is kept and 0 where it is dropped."""
    A = bf(torch.ones(M, D, device=dev()))
    I = bf(torch.eye(D, device=dev()))
    d = _drop(seed, step, site, p)
    if step_on_device:
        step_dev = torch.tensor([step], dtype=torch.int32, device=dev())
        d.step = step + 1000                              # the device word must win
        d.step_dev = step_dev.data_ptr()
    out = run_gemm(L, A, I, M, D, D, drop=d)
    keep = on_dev(keep_mask(seed, step, site, p, M * D)).view(M, D)
    assert torch.equal(out != 0, keep), f"{int(((out != 0) != keep).sum())} of {M * D} flags differ"
    assert torch.equal(out, torch.where(keep, scale_t(p), 0.0).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------
# 2. iq_cls_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 65])
@pytest.mark.parametrize("D", [32, 136, 192, 1048])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_cls_rows(L, B, D, S):
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(B * 10000 + D * 10 + S)
    cls = torch.randn(D, device=dev(), generator=g)
    pe = torch.randn(S, D, device=dev(), generator=g)
    plain = cls + pe[0]                                   # fp32, as the kernel adds them
    sentinel = -1.5

    def run(drop):
        x0 = torch.full((B, S, D), sentinel, dtype=torch.bfloat16, device=dev())
        N.check(L.iq_cls_rows(cls.data_ptr(), pe.data_ptr(), x0.data_ptr(), B, S, D, None if drop is None else C.byref(drop),
                              stream()), "cls_rows")
        torch.cuda.synchronize()
        assert torch.equal(x0[:, 1:], torch.full_like(x0[:, 1:], sentinel)), "rows other than the class row were written"
        return x0[:, 0]

    want = bf(plain).expand(B, D)
    assert torch.equal(run(None), want)
    assert torch.equal(run(_drop(5, 3, 0, 0.0)), want)
    p, seed, step, site = 0.3, SEED_HI + B, 11, 0
    groups = (np.arange(B, dtype=np.int64)[:, None] * S * D + np.arange(D // 8, dtype=np.int64)[None, :] * 8) >> 3
    keep = on_dev(keep_groups(seed, step, site, p, groups).reshape(B, D))
    want = torch.where(keep, plain * scale_t(p), 0.0).to(torch.bfloat16)
    assert torch.equal(run(_drop(seed, step, site, p)), want)


def test_cls_rows_refuses_a_width_that_is_no_multiple_of_8(L):
    B, S, D = 3, 4, 20
    cls, pe = torch.randn(D, device=dev()), torch.randn(S, D, device=dev())
    x0 = torch.full((B, S, D), 2.0, dtype=torch.bfloat16, device=dev())
    assert L.iq_cls_rows(cls.data_ptr(), pe.data_ptr(), x0.data_ptr(), B, S, D, None, stream()) == ERR_ARG
    assert L.iq_cls_rows(None, pe.data_ptr(), x0.data_ptr(), B, S, 24, None, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(x0, torch.full_like(x0, 2.0))


# ------------------------------------------------------------------------------------------------
# 3. iq_embed_bwd_gather
# ------------------------------------------------------------------------------------------------
GATHER_CASES = [(3, 5, 4, 64, 1), (2, 8, 8, 136, 0), (300, 3, 2, 192, 1), (1, 65, 64, 128, 1)]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,S,tok,D,has_cls", GATHER_CASES)
def test_embed_bwd_gather(L, B, S, tok, D, has_cls, p):
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(B + 7 * D)
    dx0 = bf(torch.randn(B, S, D, device=dev(), generator=g) + 0.25)
    seed, step, site = SEED_HI ^ D, 19, 0
    drop = _drop(seed, step, site, p) if p > 0 else None
    dref = C.byref(drop) if drop is not None else None
    if p > 0:
        keep = on_dev(keep_mask(seed, step, site, p, B * S * D)).view(B, S, D)
        masked32 = torch.where(keep, dx0.float() * scale_t(p), 0.0)                      # the kernel's fp32 product
        masked64 = torch.where(keep, dx0.double() * float(dropout_scale(p)), 0.0)
        want_demb = masked32[:, has_cls:has_cls + tok].to(torch.bfloat16)
    else:
        masked64 = dx0.double()
        want_demb = dx0[:, has_cls:has_cls + tok]
    want_dcls = masked64[:, 0].sum(0)
    demb = torch.full((B, tok, D), 3.0, dtype=torch.bfloat16, device=dev())
    start = torch.randn(D, device=dev(), generator=g) * 2
    dcls = start.clone()
    N.check(L.iq_embed_bwd_gather(dx0.data_ptr(), demb.data_ptr(), dcls.data_ptr(), B, S, tok, D, has_cls, dref, 0, stream()),
            "embed_bwd_gather")
    torch.cuda.synchronize()
    assert torch.equal(demb, want_demb)
    if has_cls:
        close_f32(dcls, want_dcls, "dcls", 1e-3)
        acc = start.clone()
        N.check(L.iq_embed_bwd_gather(dx0.data_ptr(), demb.data_ptr(), acc.data_ptr(), B, S, tok, D, 1, dref, 1, stream()),
                "embed_bwd_gather acc")
        close_f32(acc - start, want_dcls, "dcls accumulated, start taken off", 1e-3)
        close_f32(acc, start.double() + want_dcls, "dcls accumulated", 1e-3)
    else:
        assert torch.equal(dcls, start), "dcls written although there is no class token"
        demb.fill_(3.0)
        N.check(L.iq_embed_bwd_gather(dx0.data_ptr(), demb.data_ptr(), None, B, S, tok, D, 0, dref, 0, stream()), "no dcls")
        torch.cuda.synchronize()
        assert torch.equal(demb, want_demb)


def test_embed_bwd_gather_refusals(L):
    B, S, tok, D = 2, 3, 2, 24
    dx0 = bf(torch.randn(B, S, D, device=dev()))
    demb = torch.full((B, tok, D), 3.0, dtype=torch.bfloat16, device=dev())
    dcls = torch.full((D,), 4.0, device=dev())
    assert L.iq_embed_bwd_gather(dx0.data_ptr(), demb.data_ptr(), None, B, S, tok, D, 1, None, 0, stream()) == ERR_ARG
    assert L.iq_embed_bwd_gather(dx0.data_ptr(), demb.data_ptr(), dcls.data_ptr(), B, S, tok, 20, 1, None, 0, stream()) == ERR_ARG
    assert L.iq_embed_bwd_gather(None, demb.data_ptr(), dcls.data_ptr(), B, S, tok, D, 1, None, 0, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(demb, torch.full_like(demb, 3.0)) and torch.equal(dcls, torch.full_like(dcls, 4.0))


@pytest.mark.parametrize("B,S,tok,D,has_cls", GATHER_CASES)
def test_embed_bwd_gather_regenerates_the_forward_mask(L, B, S, tok, D, has_cls):
    """Forward: iq_cls_rows writes row 0 and the embedding GEMM (row remap, tok / seq / cls_off) rows cls_off + t of x0, each
    drawing its mask by OUTPUT element.  Backward of all-ones must keep exactly the elements the forward kept."""
    N = _N()
    p, seed, step, site = 0.35, SEED_HI + 3, 23, 0
    drop = _drop(seed, step, site, p)
    A = bf(torch.ones(B * tok, D, device=dev()))
    I = bf(torch.eye(D, device=dev()))
    pe = torch.zeros(S, D, device=dev())
    x0 = run_gemm(L, A, I, B * tok, D, D, rows_out=B * S, pe=pe, tok=tok, seq=S, cls_off=has_cls, drop=drop).view(B, S, D)
    if has_cls:
        one = torch.ones(D, device=dev())
        N.check(L.iq_cls_rows(one.data_ptr(), pe.data_ptr(), x0.data_ptr(), B, S, D, C.byref(drop), stream()), "cls_rows")
    torch.cuda.synchronize()
    kept = x0 != 0
    assert torch.equal(kept, on_dev(keep_mask(seed, step, site, p, B * S * D)).view(B, S, D))
    ones = bf(torch.ones(B, S, D, device=dev()))
    demb = torch.empty(B, tok, D, dtype=torch.bfloat16, device=dev())
    dcls = torch.zeros(D, device=dev())
    N.check(L.iq_embed_bwd_gather(ones.data_ptr(), demb.data_ptr(), dcls.data_ptr() if has_cls else None, B, S, tok, D, has_cls,
                                  C.byref(drop), 0, stream()), "embed_bwd_gather")
    torch.cuda.synchronize()
    assert torch.equal(demb != 0, kept[:, has_cls:has_cls + tok])
    assert torch.equal(demb, x0[:, has_cls:has_cls + tok])             # the same scale, rounded the same way
    if has_cls:
        # up to 300 copies of one fp32 value: two adds per thread, six shuffles, three through LDS = 11 roundings of 2^-24
        close_f32(dcls, kept[:, 0].double().sum(0) * float(dropout_scale(p)), "dcls of ones", 1e-6)


# ------------------------------------------------------------------------------------------------
# 4. head forward / backward and cross entropy
# ------------------------------------------------------------------------------------------------
# (B, S, D, K, pool, with_ln).  Head forward: D = 32 -> kpar 8, 64 -> 4, 136 and 192 -> 2, 256 and 768 -> 1, 1048 -> the
# serial fallback; one round is kpar * 4 classes.  K > 32 -> ce_kernel<0> and head_bwd_w_kernel.  B = 300 -> the CE thread loop.
HEAD_CASES = [
    (37, 9, 32, 8, 0, True),        # kpar 8, K below one round of 32
    (1, 1, 32, 64, 0, False),       # kpar 8, K = two whole rounds, one frame, one token, K > 32 without LayerNorm
    (37, 9, 64, 64, 1, False),      # kpar 4, K = four whole rounds
    (300, 1, 64, 53, 0, True),      # kpar 4, ce_kernel<0> with B > 256
    (1, 1, 136, 3, 1, True),        # D / 4 = 34 is no power of two (lpk 32), K below one round of 8
    (300, 9, 136, 33, 1, False),    # first K of the K > 32 kernels, ragged last round
    (300, 9, 192, 19, 0, True),     # the trained geometry with B > 256: ce_kernel<32> thread loop
    (37, 9, 192, 32, 1, True),      # last K of the K <= 32 kernels, whole rounds
    (37, 1, 256, 1, 0, False),      # kpar 1, K = 1
    (37, 9, 256, 8, 1, True),       # kpar 1, K = two whole rounds of 4
    (37, 9, 768, 33, 1, True),      # kpar 1, three passes over D per lane, K > 32 with the LayerNorm row
    (37, 9, 1048, 53, 0, True),     # serial fallback, K > 32
    (1, 9, 1048, 19, 1, False),     # serial fallback, mean pool, no LayerNorm
]


@pytest.mark.parametrize("B,S,D,K,pool,with_ln", HEAD_CASES)
def test_head_fwd_ce_bwd_branches(L, B, S, D, K, pool, with_ln):
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(B * 7 + S * 5 + D * 3 + K)
    x = bf(torch.randn(B * S, D, device=dev(), generator=g) + 0.3)
    W = torch.randn(K, D, device=dev(), generator=g) / math.sqrt(D)
    b = torch.randn(K, device=dev(), generator=g)
    lg = torch.randn(D, device=dev(), generator=g) if with_ln else None
    lb = torch.randn(D, device=dev(), generator=g) if with_ln else None
    y = torch.randint(0, K, (B,), device=dev(), generator=g)
    feat = torch.empty(B, D, device=dev())
    hstat = torch.empty(B, 2, device=dev())
    logits = torch.full((B, K), 1e9, device=dev())
    N.check(L.iq_head_fwd(x.data_ptr(), N.ptr(lg), N.ptr(lb), W.data_ptr(), b.data_ptr(), feat.data_ptr(),
                          hstat.data_ptr(), logits.data_ptr(), B, S, D, K, pool, stream()), "head_fwd")
    xr = x.double().view(B, S, D).requires_grad_(True)
    Wr, br = W.double().requires_grad_(True), b.double().requires_grad_(True)
    f = xr[:, 0] if pool == 0 else xr.mean(1)
    if with_ln:
        lgr, lbr = lg.double().requires_grad_(True), lb.double().requires_grad_(True)
        mu, var = f.detach().mean(-1), f.detach().var(-1, unbiased=False)
        close_f32(hstat[:, 0], mu, "head LayerNorm mean", 1e-5)
        close_f32(hstat[:, 1], 1 / torch.sqrt(var + 1e-5), "head LayerNorm rstd", 1e-4)
        f = torch.nn.functional.layer_norm(f, (D,), lgr, lbr, 1e-5)
    ref_logits = f @ Wr.t() + br
    close_f32(logits, ref_logits.detach(), "logits", 1e-4)
    loss_ref = torch.nn.functional.cross_entropy(ref_logits, y, label_smoothing=0.1)
    loss_sum = torch.zeros(1, device=dev())
    ncorr = torch.zeros(1, dtype=torch.int32, device=dev())
    dlogits = torch.empty(B, K, device=dev())
    N.check(L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, 0.1, float(B), loss_sum.data_ptr(),
                            ncorr.data_ptr(), dlogits.data_ptr(), stream()), "ce")
    assert abs(loss_sum.item() / B - loss_ref.item()) < 1e-4
    assert ncorr.item() == int((logits.argmax(1) == y).sum())
    if K > 1:
        loss_ref.backward()
    else:
        # one class: the loss is 0 whatever the logit, so its gradient says nothing; push a gradient of our own through the head
        assert dlogits.abs().max().item() < 1e-6 / B
        dlogits = torch.randn(B, K, device=dev(), generator=g) / B
        ref_logits.backward(dlogits.double())

    def grads(fill, accumulate):
        dW, db = torch.full_like(W, fill), torch.full_like(b, fill)
        dlg = torch.full((D,), fill, device=dev()) if with_ln else None
        dlb = torch.full((D,), fill, device=dev()) if with_ln else None
        dx = torch.full_like(x, 7.0)
        N.check(L.iq_head_bwd(dlogits.data_ptr(), feat.data_ptr(), hstat.data_ptr(), N.ptr(lg), N.ptr(lb), W.data_ptr(),
                              dW.data_ptr(), db.data_ptr(), N.ptr(dlg), N.ptr(dlb), dx.data_ptr(), B, S, D, K, pool, accumulate,
                              stream()), "head_bwd")
        return dW, db, dlg, dlb, dx

    dW, db, dlg, dlb, dx = grads(1e9, 0)                 # overwrites whatever was there
    close_f32(dW, Wr.grad, "dW", 1e-3)
    close_f32(db, br.grad, "db", 1e-3)
    close_bf16(dx.view(B, S, D), xr.grad, "dx")
    if with_ln:
        close_f32(dlg, lgr.grad, "dln_g", 1e-3)
        close_f32(dlb, lbr.grad, "dln_b", 1e-3)
    # accumulate = 1 adds onto what is there; the start is of the gradients' own size, so losing either term shows
    for fill in (Wr.grad.abs().max().item(), -br.grad.abs().max().item()):
        dW, db, dlg, dlb, dx = grads(fill, 1)
        close_f32(dW - fill, Wr.grad, "dW accumulated", 1e-3)
        close_f32(db - fill, br.grad, "db accumulated", 1e-3)
        close_bf16(dx.view(B, S, D), xr.grad, "dx is never accumulated")
        if with_ln:
            close_f32(dlg - fill, lgr.grad, "dln_g accumulated", 1e-3)
            close_f32(dlb - fill, lbr.grad, "dln_b accumulated", 1e-3)


def ce_ref(logits, y, smoothing, denom):
    """fp64 label-smoothed CE summed over frames, and the gradient of loss_sum / denom with respect to the logits."""
    z = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(z, y, label_smoothing=smoothing, reduction="sum")
    (loss / denom).backward()
    return loss.item(), z.grad


@pytest.mark.parametrize("shift", [0.0, 80.0, -80.0])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(37, 5), (300, 5), (37, 32), (37, 33), (300, 64)])
def test_ce_alone(L, B, K, smoothing, shift):
    """Loss at the file's 1e-4 of the mean loss.  dlogits at 2e-5 of the tensor's scale (which is about 1 / denom, the label's
    entry): with logits near 80 the log-sum-exp is rounded at ulp(80) / 2 = 3.8e-6, which is the relative error of every
    probability taken from it; logf, the subtraction and expf add about 1e-6, and the 32-term sum of the register path 2e-6."""
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(B + K)
    logits = torch.randn(B, K, device=dev(), generator=g) * 3 + shift
    y = torch.randint(0, K, (B,), device=dev(), generator=g)
    # ties for the maximum at classes 2 and 4: the first index counts, whichever of the two the label is
    top = logits.max(1).values + 1.0
    for row, label in ((0, 2), (1, 4), (B - 1, 4), (B // 2, 2)):
        logits[row, 2] = logits[row, 4] = top[row]
        y[row] = label
    denom = 2.5 * B
    loss, dref = ce_ref(logits, y, smoothing, denom)
    pred = logits.argmax(1)
    pred[[0, 1, B - 1, B // 2]] = 2                      # by construction: the first of the two maxima
    ncorrect = int((pred == y).sum())
    loss_sum = torch.full((1,), 5.0, device=dev())
    ncorr = torch.full((1,), 7, dtype=torch.int32, device=dev())
    dlogits = torch.full((B, K), 1e9, device=dev())
    N.check(L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, smoothing, denom, loss_sum.data_ptr(), ncorr.data_ptr(),
                            dlogits.data_ptr(), stream()), "ce")
    assert abs((loss_sum.item() - 5.0) / B - loss / B) < 1e-4, (loss_sum.item() - 5.0, loss)
    assert ncorr.item() == 7 + ncorrect
    close_f32(dlogits, dref, "dlogits", 2e-5)
    # dlogits = NULL: the loss alone, accumulated again
    N.check(L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, smoothing, denom, loss_sum.data_ptr(), None, None, stream()),
            "ce, loss only")
    assert abs((loss_sum.item() - 5.0) / B - 2 * loss / B) < 2e-4
    assert ncorr.item() == 7 + ncorrect
    # neither output asked for: still fine
    N.check(L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, smoothing, denom, None, ncorr.data_ptr(), None, stream()),
            "ce, count only")
    assert ncorr.item() == 7 + 2 * ncorrect


@pytest.mark.parametrize("B,K", [(37, 5), (300, 32), (37, 33), (300, 64)])
def test_ce_label_out_of_range_is_nan_for_that_frame_only(L, B, K):
    """Documented behaviour: no error, no out-of-bounds read; the frame's loss and gradient row are NaN, the rest is right."""
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(B * K)
    logits = torch.randn(B, K, device=dev(), generator=g) * 2
    y = torch.randint(0, K, (B,), device=dev(), generator=g)
    bad = [3, B - 2]
    good = torch.tensor([i for i in range(B) if i not in bad], device=dev())
    y_ok = y.clone()
    y[bad[0]], y[bad[1]] = -1, K
    denom = float(B)
    _, dref = ce_ref(logits, y_ok, 0.1, denom)
    loss_sum = torch.zeros(1, device=dev())
    ncorr = torch.zeros(1, dtype=torch.int32, device=dev())
    dlogits = torch.full((B, K), 1e9, device=dev())
    N.check(L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, 0.1, denom, loss_sum.data_ptr(), ncorr.data_ptr(),
                            dlogits.data_ptr(), stream()), "ce with bad labels")
    torch.cuda.synchronize()
    assert math.isnan(loss_sum.item())
    assert torch.isnan(dlogits[bad]).all()
    assert not torch.isnan(dlogits[good]).any()
    close_f32(dlogits[good], dref[good], "dlogits of the valid frames", 2e-5)
    assert ncorr.item() == int((logits.argmax(1) == y)[good].sum())
    # without the bad frames the same call gives their loss: the NaN came from those two frames alone
    lg, yg = logits[good].contiguous(), y[good].contiguous()
    loss_sum.zero_()
    N.check(L.iq_ce_fwd_bwd(lg.data_ptr(), yg.data_ptr(), B - 2, K, 0.1, denom, loss_sum.data_ptr(), None, None, stream()), "ce")
    want, _ = ce_ref(lg, yg, 0.1, denom)
    assert abs(loss_sum.item() - want) / (B - 2) < 1e-4


def test_ce_refusals(L):
    B, K = 4, 5
    logits = torch.randn(B, K, device=dev())
    y = torch.zeros(B, dtype=torch.int64, device=dev())
    loss_sum = torch.full((1,), 5.0, device=dev())
    ncorr = torch.full((1,), 7, dtype=torch.int32, device=dev())
    dlogits = torch.full((B, K), 2.0, device=dev())
    a = (loss_sum.data_ptr(), ncorr.data_ptr(), dlogits.data_ptr(), stream())
    assert L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, 0.1, 0.0, *a) == ERR_ARG
    assert L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, K, 0.1, -4.0, *a) == ERR_ARG
    assert L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, 0, 0.1, 4.0, *a) == ERR_ARG
    assert L.iq_ce_fwd_bwd(logits.data_ptr(), y.data_ptr(), B, -3, 0.1, 4.0, *a) == ERR_ARG
    assert L.iq_ce_fwd_bwd(None, y.data_ptr(), B, K, 0.1, 4.0, *a) == ERR_ARG
    assert L.iq_ce_fwd_bwd(logits.data_ptr(), None, B, K, 0.1, 4.0, *a) == ERR_ARG
    torch.cuda.synchronize()
    assert loss_sum.item() == 5.0 and ncorr.item() == 7 and torch.equal(dlogits, torch.full_like(dlogits, 2.0))


# ------------------------------------------------------------------------------------------------
# 5. gradient norm, clip, AdamW
# ------------------------------------------------------------------------------------------------
def f32(x):
    """The value a C float argument carries, as a Python double."""
    return float(np.float32(x))


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 4, 7, 1000, 100003, 4_200_004])
def test_gradnorm_sq(L, n, scale):
    """out = scale^2 * sum g^2.  n = 1, 7, 100003 end in the n & 3 tail (alone, after one vector, after many); 4,200,004 is
    more than 1024 blocks x 256 threads x 4 vectors of 4, so the grid-stride loop runs, with a tail of none.

    Bound 1e-5 on the norm (the existing test allows 1e-4): a thread adds at most 5 vectors of 4 squares, then 6 shuffles, 3 adds
    through LDS, and the same again over the 1024 partials: under 50 roundings of 2^-24 on a sum of positives, 3e-6 at worst."""
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(n)
    grad = torch.randn(n, device=dev(), generator=g) * 0.05
    ws = torch.full((L.iq_gradnorm_ws_bytes(n) // 4,), 1e9, device=dev())
    out = torch.full((1,), 1e9, device=dev())
    N.check(L.iq_gradnorm_sq(grad.data_ptr(), n, scale, ws.data_ptr(), out.data_ptr(), stream()), "gradnorm")
    want = scale * grad.double().norm().item()
    assert abs(math.sqrt(out.item()) - want) <= 1e-5 * want, (math.sqrt(out.item()), want)


def test_gradnorm_sq_refusals(L):
    n = 64
    buf = torch.randn(n + 4, device=dev())
    ws = torch.empty(L.iq_gradnorm_ws_bytes(n) // 4, device=dev())
    out = torch.full((1,), 3.0, device=dev())
    assert L.iq_gradnorm_sq(buf[1:].data_ptr(), n, 1.0, ws.data_ptr(), out.data_ptr(), stream()) == ERR_ARG
    assert L.iq_gradnorm_sq(None, n, 1.0, ws.data_ptr(), out.data_ptr(), stream()) == ERR_ARG
    assert L.iq_gradnorm_sq(buf.data_ptr(), n, 1.0, None, out.data_ptr(), stream()) == ERR_ARG
    assert L.iq_gradnorm_sq(buf.data_ptr(), n, 1.0, ws.data_ptr(), None, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert out.item() == 3.0


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, grad_scale, clip):
    """clip_grad_norm_(max_norm) on grad_scale * g, then decoupled AdamW, in fp64; every hyper-parameter is the fp32 value the C
    ABI carries.  Updates p, m, v in place."""
    lr, b1, b2, eps, wd, max_norm, grad_scale = (f32(t) for t in (lr, b1, b2, eps, wd, max_norm, grad_scale))
    coef = grad_scale
    if clip and max_norm > 0:
        total = grad_scale * g.norm().item()
        coef *= min(1.0, max_norm / (total + 1e-6))
    gg = g * coef
    p.mul_(1.0 - lr * wd)
    m.mul_(b1).add_(gg, alpha=1.0 - b1)
    v.mul_(b2).addcmul_(gg, gg, value=1.0 - b2)
    den = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    p.addcdiv_(m, den, value=-lr / (1.0 - b1 ** step))


# (n, grad norm after grad_scale, max_norm, clip, grad_scale, weight_decay, dyn, shadow)
ADAMW_CASES = [
    (100_000, 16.0, 1.0, True, 1.0, 1e-3, False, True),        # clip active: the existing test's setting
    (1000, 0.3, 1.0, True, 0.125, 1e-3, False, True),          # clip inactive, gradient scale 1 / world
    (4, 16.0, 0.0, True, 1.0, 0.0, False, False),              # one vector; max_norm 0 switches the clip off; no decay, no shadow
    (100_000, 5.0, 1.0, False, 0.125, 0.0, True, False),       # no norm given at all; device lr / step
    (2_500_000, 16.0, 1.0, True, 0.125, 1e-3, True, True),     # more than 2048 x 256 x 4 elements: the grid-stride loop
]


@pytest.mark.parametrize("n,gnorm,max_norm,clip,grad_scale,wd,use_dyn,use_shadow", ADAMW_CASES)
def test_clip_adamw_against_fp64(L, n, gnorm, max_norm, clip, grad_scale, wd, use_dyn, use_shadow):
    """Three steps (the bias corrections move) against clip_grad_norm_ + decoupled AdamW written out in fp64.
    p at the existing atol 2e-7 / rtol 1e-6; m and v at 1e-5 of their scale: per step they take four fp32 roundings of 2^-24
    plus the relative error of the clip coefficient (the fp32 norm, under 3e-6 by the count in test_gradnorm_sq)."""
    N = _N()
    lr, b1, b2, eps = 1e-4, 0.9, 0.99, 1e-8
    g = torch.Generator(device="cuda").manual_seed(n + int(gnorm * 10))
    p0 = torch.randn(n, device=dev(), generator=g)
    grad = torch.randn(n, device=dev(), generator=g)
    grad *= gnorm / grad_scale / grad.double().norm().item()
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64, device=dev()), torch.zeros(n, dtype=torch.float64, device=dev())
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev()) if use_shadow else None
    ws = torch.empty(L.iq_gradnorm_ws_bytes(n) // 4, device=dev())
    gn = torch.empty(1, device=dev())
    torch_ref = n == 100_000 and grad_scale == 1.0             # the fp32 torch.optim.AdamW comparison, kept where it applies
    if torch_ref:
        pt = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([pt], lr=lr, weight_decay=wd, betas=(b1, b2), eps=eps)
    for step in (1, 2, 3):
        gstep = grad * (1.0 if gnorm < 1 else step)            # (an inactive clip stays inactive)
        lr_s = lr * step                                       # a schedule: the step size changes too
        if clip:
            N.check(L.iq_gradnorm_sq(gstep.data_ptr(), n, grad_scale, ws.data_ptr(), gn.data_ptr(), stream()), "gradnorm")
        dyn = torch.tensor([lr_s, float(step)], device=dev()) if use_dyn else None
        N.check(L.iq_adamw_step(p.data_ptr(), gstep.data_ptr(), m.data_ptr(), v.data_ptr(), N.ptr(shadow), n,
                                0.0 if use_dyn else lr_s, b1, b2, eps, wd, 0 if use_dyn else step, gn.data_ptr() if clip else None,
                                max_norm, grad_scale, N.ptr(dyn), stream()), "adamw")
        adamw_ref(pr, gstep.double(), mr, vr, lr_s, b1, b2, eps, wd, step, max_norm, grad_scale, clip)
        err = (p.double() - pr).abs()
        assert (err <= 2e-7 + 1e-6 * pr.abs()).all(), f"step {step}: p off by {err.max().item():.3g}"
        close_f32(m, mr, f"m, step {step}", 1e-5)
        close_f32(v, vr, f"v, step {step}", 1e-5)
        if use_shadow:
            assert torch.equal(shadow, p.to(torch.bfloat16))
        if torch_ref:
            for grp in opt.param_groups:
                grp["lr"] = lr_s
            pt.grad = gstep.clone()
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
            opt.step()
            assert torch.allclose(p, pt.data, atol=2e-7, rtol=1e-6), (p - pt.data).abs().max()
    # the clip did what the case says it does
    total = grad_scale * (grad.double() * (1.0 if gnorm < 1 else 3)).norm().item()
    assert (total > max_norm) == (gnorm > 1)


def test_adamw_refusals_leave_the_state_untouched(L):
    n = 64
    buf = [torch.randn(n + 4, device=dev()) for _ in range(4)]
    p, g, m, v = (t[:n] for t in buf)
    before = [t.clone() for t in buf]
    shadow = torch.full((n,), 2.0, dtype=torch.bfloat16, device=dev())
    hyper = (1e-3, 0.9, 0.99, 1e-8, 1e-2)

    def call(p_, g_, m_, v_, n_, step, dyn=None):
        return L.iq_adamw_step(N_ptr(p_), N_ptr(g_), N_ptr(m_), N_ptr(v_), shadow.data_ptr(), n_, *hyper, step, None, 0.0, 1.0, dyn,
                               stream())

    def N_ptr(t):
        return None if t is None else t.data_ptr()

    assert call(p, g, m, v, 62, 1) == ERR_ARG                                   # n % 4
    for i in range(4):                                                          # each pointer in turn: off by one element, NULL
        args = [p, g, m, v]
        args[i] = buf[i][1:n + 1]
        assert call(*args, n, 1) == ERR_ARG
        args[i] = None
        assert call(*args, n, 1) == ERR_ARG
    assert call(p, g, m, v, n, 0) == ERR_ARG                                    # step < 1 and no device step
    assert call(p, g, m, v, n, -2) == ERR_ARG
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(buf, before))
    assert torch.equal(shadow, torch.full_like(shadow, 2.0))
    # the same call with a device step is accepted
    dyn = torch.tensor([1e-3, 1.0], device=dev())
    assert call(p, g, m, v, n, 0, dyn.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf[0], before[0]) and torch.equal(buf[1], before[1])
    assert torch.equal(buf[0][n:], before[0][n:])


# ------------------------------------------------------------------------------------------------
# 6. casts and patchify
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 1001, 1002, 1003, 2_100_001])
def test_cast_bf16(L, n):
    """n & 3 = 1, 2, 3 elements after the last whole vector; 2,100,001 is more than 2048 blocks x 256 threads x 4."""
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(n)
    src = torch.randn(n, device=dev(), generator=g)
    out = torch.full((n + 3,), 9.0, dtype=torch.bfloat16, device=dev())
    N.check(L.iq_cast_bf16(src.data_ptr(), out.data_ptr(), n, stream()), "cast")
    torch.cuda.synchronize()
    assert torch.equal(out[:n], bf(src))
    assert torch.equal(out[n:], torch.full_like(out[n:], 9.0)), "written past n"


def test_cast_bf16_empty_and_misaligned(L):
    assert L.iq_cast_bf16(None, None, 0, stream()) == 0
    src = torch.randn(68, device=dev())
    out = torch.full((68,), 9.0, dtype=torch.bfloat16, device=dev())
    assert L.iq_cast_bf16(src[1:].data_ptr(), out.data_ptr(), 64, stream()) == ERR_ARG
    assert L.iq_cast_bf16(src.data_ptr(), out[1:].data_ptr(), 64, stream()) == ERR_ARG
    assert L.iq_cast_bf16(None, out.data_ptr(), 64, stream()) == ERR_ARG
    assert L.iq_cast_bf16(src.data_ptr(), None, 64, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 9.0))


@pytest.mark.parametrize("rows,cols", [(1, 1), (33, 31), (64, 96)])
def test_transpose_cast_bf16(L, rows, cols):
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(rows * 100 + cols)
    src = torch.randn(rows, cols, device=dev(), generator=g)
    dst = torch.full((cols * rows + 8,), 9.0, dtype=torch.bfloat16, device=dev())
    N.check(L.iq_transpose_cast_bf16(src.data_ptr(), dst.data_ptr(), rows, cols, stream()), "transpose")
    torch.cuda.synchronize()
    assert torch.equal(dst[:cols * rows].view(cols, rows), bf(src.t().contiguous()))
    assert torch.equal(dst[cols * rows:], torch.full_like(dst[cols * rows:], 9.0))


@pytest.mark.parametrize("Cc,H,W,p,Kpad", [(1, 32, 32, 16, 256), (2, 16, 48, 8, 128), (2, 16, 48, 8, 136), (3, 8, 12, 4, 48)])
def test_patchify_2d(L, Cc, H, W, p, Kpad):
    """(1, 32, 32, 16) is the ViT geometry with Kpad == P: every chunk takes the 16-byte path; Kpad = 136 adds a zero chunk."""
    N = _N()
    Bf, P = 3, Cc * p * p
    x = torch.randn(Bf, Cc, H, W, device=dev(), generator=torch.Generator(device="cuda").manual_seed(H * W))
    out = torch.full((Bf * (H // p) * (W // p), Kpad), 9.0, dtype=torch.bfloat16, device=dev())
    N.check(L.iq_patchify(x.data_ptr(), out.data_ptr(), 0, Bf, Cc, H, W, p, Kpad, stream()), "patchify")
    ref = torch.nn.functional.unfold(x, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, P)
    assert torch.equal(out[:, :P], bf(ref))
    assert torch.count_nonzero(out[:, P:]) == 0


@pytest.mark.parametrize("k,Kpad", [(16, 32), (8, 32)])
def test_patchify_1d(L, k, Kpad):
    N = _N()
    Bf, Cc, Lq = 3, 2, 64
    x = torch.randn(Bf, Cc, Lq, device=dev(), generator=torch.Generator(device="cuda").manual_seed(k))
    out = torch.full((Bf * (Lq // k), Kpad), 9.0, dtype=torch.bfloat16, device=dev())
    N.check(L.iq_patchify(x.data_ptr(), out.data_ptr(), 1, Bf, Cc, Lq, 0, k, Kpad, stream()), "patchify1d")
    ref = torch.nn.functional.unfold(x.unsqueeze(2), kernel_size=(1, k), stride=(1, k)).transpose(1, 2).reshape(-1, Cc * k)
    assert torch.equal(out[:, :Cc * k], bf(ref))
    assert torch.count_nonzero(out[:, Cc * k:]) == 0


def test_patchify_refusals(L):
    x = torch.randn(2, 2, 16, 16, device=dev())
    out = torch.full((2 * 4, 136), 9.0, dtype=torch.bfloat16, device=dev())     # P = 2 * 8 * 8 = 128
    a = (x.data_ptr(), out.data_ptr())
    assert L.iq_patchify(*a, 0, 2, 2, 16, 16, 8, 120, stream()) == ERR_ARG      # Kpad < P
    assert L.iq_patchify(*a, 0, 2, 2, 16, 16, 8, 132, stream()) == ERR_ARG      # Kpad % 8
    assert L.iq_patchify(*a, 2, 2, 2, 16, 16, 8, 128, stream()) == ERR_ARG      # kind
    assert L.iq_patchify(*a, 1, 2, 2, 16, 0, 8, 8, stream()) == ERR_ARG         # 1-D: Kpad < P = 16
    assert L.iq_patchify(None, out.data_ptr(), 0, 2, 2, 16, 16, 8, 128, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 9.0))
