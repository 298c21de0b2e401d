"""GPU (MI355X): what a change to WHEN attn_bwd_once_kernel<1024> and attn_fwd_kernel<64, *> (csrc/attention.hip) load
their operands, or to which wave owns which 16-key unit, must leave alone: every bit of every result.

Written with the load-schedule experiments of profiles/attn_loads.txt (O staged into the LDS region that later holds the
dS image, phase B's K image written from the fragments phase A held with idle waves zeroing rows [16 nunit, spad), the
forward's Q fragments requested with the K / V stage); the shapes are the ones at which those go wrong, and at which
"one unit per wave" does: one unit, the unit edge, 13 and 14 units, image rows nobody writes.

1. test_once_equals_the_recomputing_kernel: iq_attn_bwd against iq_attn_bwd_masked with an all-ones mask
   (attn_bwd_kernel<64, true>), torch.equal on the whole NaN-prefilled dqkv.  S covers one unit (1, 16), the unit edge (17),
   a 64-row O image larger than (48: 8,192 B against 7,168 B) and smaller than (49) the dS region, 13 full units with 16
   padding rows (193 .. 208), 14 units (209, 224), and the benchmark's 197.  At H = 1, 3 the per-frame kernel claims
   S <= 128, so those S also run at H = 12, where the once kernel takes them; the kernel that ran is asserted.  All 27
   cases are equal on the commit before this file as well.
2. test_fenced_poisoned_budgeted: run() of test_gpu_attention_exact (fenced operands, NaN guard rows, whole-buffer
   prefill patterns, the fp64 budget), forward and backward; S = 225 is the multi-stage forward, which must behave as before.
3. Stale LDS: (a) 270 workgroups, more than one per CU, every frame against a one-frame launch; (b) a small problem
   before and after a large one with 8 x larger inputs in every image row the small one leaves unwritten.
"""
import pytest
import torch

from prof_names import kernels_of
from test_gpu_attention_bwd_once import backward, backward_old, forward, frame_claims, once_claims
from test_gpu_attention_exact import L, random_case, run  # noqa: F401  (L is a fixture)
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

EQ_S = (1, 16, 17, 48, 49, 193, 197, 207, 208, 209, 224)
EQUAL = [(S, H) for S in EQ_S for H in (1, 3)] + [(S, 12) for S in EQ_S if S <= 128]


@pytest.mark.parametrize("S,H", EQUAL)
def test_once_equals_the_recomputing_kernel(L, S, H):
    dh, Bf, D = 64, 2, H * 64
    g = torch.Generator(device="cuda").manual_seed(S * 257 + H)
    qkv = torch.randn(Bf * S, 3 * D, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    out, lse = forward(L, qkv, Bf, S, H, dh)
    res = {}
    names = kernels_of(L, lambda: res.setdefault("new", backward(L, qkv, out, dout, lse, Bf, S, H, dh)))
    if once_claims(S, H, dh):
        assert names == ["attn_bwd_once_kernel<1024>"], names
    else:
        assert frame_claims(S, H, dh) and names == ["attn_frame_bwd_kernel<64>"], names
    assert S > 128 or H != 12 or once_claims(S, H, dh)     # every S reaches the once kernel at some H
    old_names = kernels_of(L, lambda: res.setdefault("old", backward_old(L, qkv, out, dout, lse, Bf, S, H, dh)))
    assert old_names == ["attn_bwd_kernel<64, true>"], old_names
    new, old = res["new"], res["old"]
    assert not new.isnan().any() and not old.isnan().any()
    diff = (new.float() - old.float()).abs().max().item()
    print(f"S={S} H={H} {names[0]}: max |diff| against attn_bwd_kernel<64, true> {diff:.4g}")
    assert torch.equal(new, old), f"S={S} H={H} {names[0]}: dqkv differs from the recomputing kernel by {diff:.4g}"


BUDGET = ([(S, H, None) for S in (1, 31, 32, 33, 48, 49, 197, 208, 224) for H in (1, 3)] +
          [(S, 12, None) for S in (1, 31, 32, 33, 48, 49)] +         # the once kernel and attn_fwd_kernel at S <= 128
          [(225, 1, None), (33, 1, "shared"), (197, 1, "shared"), (33, 12, "shared")])


@pytest.mark.parametrize("S,H,kind", BUDGET)
def test_fenced_poisoned_budgeted(L, S, H, kind):
    run(L, 2, S, H, 64, kind)


def test_stale_lds_more_workgroups_than_cus(L):
    """Bf = 90, H = 3: 270 workgroups on 256 CUs, so some CUs run a second workgroup over what the first left in LDS."""
    Bf, S, H, dh = 90, 197, 3, 64
    c = random_case(L, Bf, S, H, dh)
    assert tuple(c.names[:2]) == ("attn_fwd_kernel<64, false>", "attn_bwd_once_kernel<1024>"), c.names
    out, lse = c.fwd(0)
    dqkv = c.bwd(out, lse, 0)
    out1, lse1 = c.fwd(1, frames=True)
    dqkv1 = c.bwd(out1, lse1, 1, frames=True)
    for a, b, name in ((out, out1, "out"), (lse, lse1, "lse"), (dqkv, dqkv1, "dqkv")):
        if not torch.equal(a.body, b.body):
            rows = (a.body.reshape(Bf, -1) != b.body.reshape(Bf, -1)).any(1).nonzero().flatten().tolist()
            raise AssertionError(f"{c.what} {c.names}: {name} of frames {rows[:8]} depends on the batch it was launched in")
        assert not a.body.isnan().any()


def test_stale_lds_small_problem_after_a_large_one(L):
    """X (S = 17, H = 3, two frames) before and after Y (S = 224, 256 frames, inputs 8 x larger: every image row and every
    dS cell of every CU written).  At H = 3 the per-frame kernels take X; the next test has X on the once kernel (one full
    unit + one key, 32 image rows, an O image of 4,096 B over a dS region of 2,560 B)."""
    dh, H = 64, 3
    D = H * dh

    def problem(Bf, S, seed, gain):
        g = torch.Generator(device="cuda").manual_seed(seed)
        qkv = (gain * torch.randn(Bf * S, 3 * D, device=dev(), generator=g)).to(torch.bfloat16)
        dout = (gain * torch.randn(Bf * S, D, device=dev(), generator=g)).to(torch.bfloat16)
        return qkv, dout

    def both(qkv, dout, Bf, S):
        res = {}
        fwd = kernels_of(L, lambda: res.setdefault("f", forward(L, qkv, Bf, S, H, dh)))
        out, lse = res["f"]
        bwd = kernels_of(L, lambda: res.setdefault("b", backward(L, qkv, out, dout, lse, Bf, S, H, dh)))
        return out, lse, res["b"], fwd, bwd

    xq, xd = problem(2, 17, 5, 1.0)
    yq, yd = problem(256, 224, 6, 8.0)
    first = both(xq, xd, 2, 17)
    big = both(yq, yd, 256, 224)
    assert big[3] == ["attn_fwd_kernel<64, false>"] and big[4] == ["attn_bwd_once_kernel<1024>"], big[3:]
    assert torch.isfinite(big[2].float()).all()
    again = both(xq, xd, 2, 17)
    for a, b, name in zip(first[:3], again[:3], ("out", "lse", "dqkv")):
        assert not a.isnan().any(), name
        assert torch.equal(a, b), f"X {name} changed after Y ran on the same CUs ({first[3]}, {first[4]})"


def test_stale_lds_small_problem_after_a_large_one_on_the_once_kernel(L):
    """The same at H = 12, where X itself runs attn_fwd_kernel<64, false> and attn_bwd_once_kernel<1024>."""
    dh = 64

    def problem(Bf, S, H, seed, gain):
        g = torch.Generator(device="cuda").manual_seed(seed)
        qkv = (gain * torch.randn(Bf * S, 3 * H * dh, device=dev(), generator=g)).to(torch.bfloat16)
        dout = (gain * torch.randn(Bf * S, H * dh, device=dev(), generator=g)).to(torch.bfloat16)
        return qkv, dout

    def both(qkv, dout, Bf, S, H):
        res = {}
        fwd = kernels_of(L, lambda: res.setdefault("f", forward(L, qkv, Bf, S, H, dh)))
        out, lse = res["f"]
        bwd = kernels_of(L, lambda: res.setdefault("b", backward(L, qkv, out, dout, lse, Bf, S, H, dh)))
        assert fwd == ["attn_fwd_kernel<64, false>"] and bwd == ["attn_bwd_once_kernel<1024>"], (fwd, bwd)
        return out, lse, res["b"]

    xq, xd = problem(2, 17, 12, 5, 1.0)
    yq, yd = problem(256, 224, 3, 6, 8.0)
    first = both(xq, xd, 2, 17, 12)
    big = both(yq, yd, 256, 224, 3)
    assert torch.isfinite(big[2].float()).all()
    again = both(xq, xd, 2, 17, 12)
    for a, b, name in zip(first, again, ("out", "lse", "dqkv")):
        assert not a.isnan().any(), name
        assert torch.equal(a, b), f"X {name} changed after Y ran on the same CUs"
