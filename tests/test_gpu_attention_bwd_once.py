"""GPU (MI355X): attn_bwd_once_kernel, the attention backward that forms the S x S terms once and hands dS to the dQ
product through an LDS image (csrc/attention.hip).  It takes dh = 64, no mask, padded length <= 224 rows, whenever the
per-frame kernel does not claim the shape; everything runs through the iq_attn_fwd / iq_attn_bwd entry points and the
kernel that ran is read back from the profiling records (iq_prof_kernels).

Accuracy bound: the project's attention-backward bound (test_gpu_kernels.py::test_attention_fwd_bwd),
max |err| <= 0.02 * max |grad| + 1e-6 against fp64 autograd of the same attention on the bf16-rounded inputs.
"""
import math

import pytest
import torch

from prof_names import kernels_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vit_vs_raw_iq_amd._native as N
    return N.lib()


def _N():
    import vit_vs_raw_iq_amd._native as N
    return N


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def attn_ref(qkv, Bf, S, H, dh):
    D = H * dh
    q, k, v = [t.view(Bf, S, H, dh).transpose(1, 2) for t in qkv.view(Bf, S, 3, D).unbind(2)]
    s = (q @ k.transpose(2, 3)) / math.sqrt(dh)
    p = torch.softmax(s, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(Bf * S, D)
    return o, torch.logsumexp(s, dim=-1)


def frame_claims(S, H, dh):
    """use_frame(S, frame_bwd_lds(S, H, dh)) of csrc/attention.hip, restated: S <= 128 and the frame's images fit 112 KiB."""
    spad = (S + 31) // 32 * 32
    lds = spad * (3 * H * dh + 16) * 2 + spad * (H * dh + 16) * 2 + 2 * H * spad * 4
    return S <= 128 and lds <= 112 * 1024


def once_claims(S, H, dh):
    return dh == 64 and (S + 31) // 32 * 32 <= 224 and not frame_claims(S, H, dh)


def frame_fwd_claims(S, H, dh):
    """use_frame(S, frame_fwd_lds(S, H, dh)), restated: the forward's frame holds q, k, v only."""
    spad = (S + 31) // 32 * 32
    return S <= 128 and spad * (3 * H * dh + 16) * 2 <= 112 * 1024


def forward(L, qkv, Bf, S, H, dh):
    out = torch.empty(Bf * S, H * dh, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(Bf, H, S, device=dev())
    _N().check(L.iq_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), Bf, S, H, dh, stream()), "attn_fwd")
    return out, lse


def backward(L, qkv, out, dout, lse, Bf, S, H, dh, fill=float("nan")):
    dqkv = torch.full_like(qkv, fill)          # every element must be written
    _N().check(L.iq_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), Bf, S, H,
                             dh, stream()), "attn_bwd")
    return dqkv


def backward_old(L, qkv, out, dout, lse, Bf, S, H, dh):
    """The two-phase kernel that recomputes dS: an all-ones mask still dispatches to attn_bwd_kernel<64, true>."""
    mk = torch.ones(Bf, 1, S, S, dtype=torch.uint8, device=dev())
    dqkv = torch.full_like(qkv, float("nan"))
    _N().check(L.iq_attn_bwd_masked(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                    mk.data_ptr(), 0, Bf, S, H, dh, stream()), "attn_bwd_masked")
    return dqkv


def check_against_fp64(qkv, dout, dqkv, Bf, S, H, dh, what):
    qr = qkv.double().requires_grad_(True)
    oref, _ = attn_ref(qr, Bf, S, H, dh)
    oref.backward(dout.double())
    gref = qr.grad
    scale = gref.abs().max().item()
    err = (dqkv.double() - gref).abs().max().item()
    print(f"{what}: max err {err:.4g}, scale {scale:.4g}, bound {0.02 * scale + 1e-6:.4g}")
    assert torch.isfinite(dqkv.float()).all(), what
    assert err <= 0.02 * scale + 1e-6, f"{what}: attn bwd max err {err:.4g} scale {scale:.4g}"


# S: the edges of the 16-key unit (16, 17, 208, 209), of the 32-row block (193, 224) and of the S = 197 image (207, 208)
SMALL = [(S, H, 64, 2) for S in (1, 16, 17, 193, 197, 207, 208, 209, 224) for H in (1, 3, 12)]
# The edges of the kernel choice, with the (forward, backward) kernel each side must run: S = 128 | 129 (the per-frame kernels
# end at 128 rows); S = 128 with H = 2 (the forward's frame is 102,400 B of LDS, the backward's 141,312 B > 112 KiB); S = 225
# (padded length 256 > 224: the two-phase kernel).
EDGES = {(128, 1, 64, 2): ("attn_frame_fwd_kernel<64>", "attn_frame_bwd_kernel<64>"),
         (129, 1, 64, 2): ("attn_fwd_kernel<64, false>", "attn_bwd_once_kernel<1024>"),
         (128, 2, 64, 2): ("attn_frame_fwd_kernel<64>", "attn_bwd_once_kernel<1024>"),
         (225, 1, 64, 2): ("attn_fwd_kernel<64, false>", "attn_bwd_kernel<64, false>")}


@pytest.mark.parametrize("S,H,dh,Bf", [(197, 3, 64, 256)] + SMALL + list(EDGES))
def test_bwd_once_matches_fp64_autograd(L, S, H, dh, Bf):
    D = H * dh
    g = torch.Generator(device="cuda").manual_seed(S * 131 + H)
    qkv = torch.randn(Bf * S, 3 * D, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    res = {}
    fwd = kernels_of(L, lambda: res.setdefault("fwd", forward(L, qkv, Bf, S, H, dh)))
    out, lse = res["fwd"]
    assert fwd == ["attn_frame_fwd_kernel<64>" if frame_fwd_claims(S, H, dh) else "attn_fwd_kernel<64, false>"], fwd
    names = kernels_of(L, lambda: res.setdefault("dqkv", backward(L, qkv, out, dout, lse, Bf, S, H, dh)))
    bwd = [n for n in names if "bwd" in n]
    if 193 <= S <= 224:
        assert once_claims(S, H, dh)          # the long shapes must reach the new kernel
    if once_claims(S, H, dh):
        assert len(bwd) == 1 and bwd[0].startswith("attn_bwd_once_kernel<"), names
    elif frame_claims(S, H, dh):
        assert len(bwd) == 1 and bwd[0].startswith("attn_frame_bwd_kernel<"), names
    else:
        assert len(bwd) == 1 and bwd[0].startswith("attn_bwd_kernel<"), names
    if (S, H, dh, Bf) in EDGES:
        assert (fwd[0], bwd[0]) == EDGES[(S, H, dh, Bf)], (fwd, names)
    check_against_fp64(qkv, dout, res["dqkv"], Bf, S, H, dh, f"S={S} H={H} frames={Bf} ({bwd[0]})")


def test_bwd_once_against_the_recomputing_kernel_at_the_benchmarked_shape(L):
    """Same inputs through attn_bwd_kernel<64, true> (all-ones mask): both kernels feed the same bf16 operands to the same
    products in the same order, so the difference is expected to be zero; the requirement is the accuracy bound."""
    S, H, dh, Bf = 197, 3, 64, 256
    D = H * dh
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(Bf * S, 3 * D, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    out, lse = forward(L, qkv, Bf, S, H, dh)
    new = backward(L, qkv, out, dout, lse, Bf, S, H, dh)
    names = kernels_of(L, lambda: backward_old(L, qkv, out, dout, lse, Bf, S, H, dh))
    assert any(n.startswith("attn_bwd_kernel<64, true>") for n in names), names
    old = backward_old(L, qkv, out, dout, lse, Bf, S, H, dh)
    scale = old.float().abs().max().item()
    diff = (new.float() - old.float()).abs().max().item()
    print(f"new vs recomputing kernel: max |diff| {diff:.4g}, scale {scale:.4g}, bit-identical {torch.equal(new, old)}")
    assert torch.isfinite(new.float()).all()
    assert diff <= 0.02 * scale + 1e-6


@pytest.mark.parametrize("S,H,Bf", [(197, 3, 256), (209, 12, 2), (17, 12, 2)])
def test_bwd_once_is_deterministic(L, S, H, Bf):
    dh, D = 64, H * 64
    g = torch.Generator(device="cuda").manual_seed(S + 5)
    qkv = torch.randn(Bf * S, 3 * D, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    out, lse = forward(L, qkv, Bf, S, H, dh)
    a = backward(L, qkv, out, dout, lse, Bf, S, H, dh, fill=1.0)
    b = backward(L, qkv, out, dout, lse, Bf, S, H, dh, fill=-1.0)
    assert torch.equal(a, b)


def test_bwd_once_all_scores_very_negative_stays_finite(L):
    """Rows whose scores are all << 0 have a very negative LSE: exp2(0 - lse) on a padding key overflows fp32.  Padding
    keys are masked in the partial unit, their image columns hold zeros and the key block's unwritten half is a constant
    zero, so nothing non-finite may reach dQ / dK / dV."""
    S, H, dh, Bf = 197, 3, 64, 2
    D = H * dh
    qkv = torch.empty(Bf * S, 3 * D, device=dev())
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv[:, :D] = 6.0 + 0.1 * torch.randn(Bf * S, D, device=dev(), generator=g)          # q . k = -64 * 36 / 8 = -288
    qkv[:, D:2 * D] = -6.0 + 0.1 * torch.randn(Bf * S, D, device=dev(), generator=g)
    qkv[:, 2 * D:] = torch.randn(Bf * S, D, device=dev(), generator=g)
    qkv = qkv.to(torch.bfloat16)
    out, lse = forward(L, qkv, Bf, S, H, dh)
    assert lse.max().item() < -150
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    res = {}
    names = kernels_of(L, lambda: res.setdefault("dqkv", backward(L, qkv, out, dout, lse, Bf, S, H, dh)))
    assert any(n.startswith("attn_bwd_once_kernel<") for n in names), names
    assert torch.isfinite(out.float()).all() and torch.isfinite(res["dqkv"].float()).all()
    check_against_fp64(qkv, dout, res["dqkv"], Bf, S, H, dh, "very negative scores")
