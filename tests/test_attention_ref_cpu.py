"""CPU: the attention references, restated launch rules and checks of tests/attention_ref.py.

The references are checked against torch autograd in fp64; attn_rounded against its documented distance; the launch rules
at the table the GPU suite asserts kernel names with; and every check of the GPU suite is shown to fail, on the CPU, for
the reason it exists: a hand-made error is applied to reference outputs and the failure message must name it.
"""
import math

import pytest
import torch

import attention_ref as A

SHAPES = [(2, 5, 2, 16), (2, 33, 3, 32), (1, 70, 2, 64)]      # (Bf, S, H, dh)


def inputs(Bf, S, H, dh, seed=0, masked=False):
    g = torch.Generator().manual_seed(seed + S)
    qkv = torch.randn(Bf * S, 3 * H * dh, generator=g).bfloat16()
    dout = torch.randn(Bf * S, H * dh, generator=g).bfloat16()
    mask = None
    if masked:
        mask = torch.rand(Bf, H, S, S, generator=g) > 0.3
        mask[:, :, S // 2, :] = False
        mask[:, :, 0, :] = False
        mask[:, :, 0, S - 1] = True
    return qkv, dout, mask


def autograd(qkv, dout, mask, Bf, S, H, dh):
    x = qkv.double().requires_grad_(True)
    q, k, v = A.parts_of(x, Bf, S, H, dh)
    s = A.scores(q, k, mask, dh)
    out = torch.softmax(s, -1) @ v
    out.backward(A.heads_of(dout, Bf, S, H, dh))
    return out.detach(), torch.logsumexp(s, -1).detach(), A.parts_of(x.grad, Bf, S, H, dh)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Bf,S,H,dh", SHAPES)
def test_fp64_reference_is_autograd(Bf, S, H, dh, masked):
    qkv, dout, mask = inputs(Bf, S, H, dh, masked=masked)
    r = A.attn_fp64(qkv, dout, mask, Bf, S, H, dh)
    out, lse, (dq, dk, dv) = autograd(qkv, dout, mask, Bf, S, H, dh)
    for name, got, ref in (("out", r.out, out), ("lse", r.lse, lse), ("dq", r.dq, dq), ("dk", r.dk, dk), ("dv", r.dv, dv)):
        assert (got - ref).abs().max().item() <= 1e-12 * (1 + ref.abs().max().item()), name


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Bf,S,H,dh", SHAPES)
def test_rounded_reference_is_within_its_documented_distance(Bf, S, H, dh, masked):
    """|rounded - fp64| <= 2^-7 mag (out, dV) and 2^-6 mag (dQ, dK), elementwise; lse is not rounded; and it agrees with
    autograd to bf16 accuracy (it is the same mathematics)."""
    qkv, dout, mask = inputs(Bf, S, H, dh, masked=masked)
    f, r = A.attn_fp64(qkv, dout, mask, Bf, S, H, dh), A.attn_rounded(qkv, dout, mask, Bf, S, H, dh)
    assert (f.lse - r.lse).abs().max().item() <= 1e-12 * (1 + f.lse.abs().max().item())
    for name, c in (("out", 2.0 ** -7), ("dv", 2.0 ** -7), ("dq", 2.0 ** -6), ("dk", 2.0 ** -6)):
        d = (getattr(r, name) - getattr(f, name)).abs()
        assert (d <= 1.01 * c * f.mag[name]).all(), (name, float((d / f.mag[name].clamp_min(1e-300)).max()))
        assert d.max().item() > 0, name                               # and it does round
    out, _, (dq, dk, dv) = autograd(qkv, dout, mask, Bf, S, H, dh)
    for got, ref in ((r.out, out), (r.dq, dq), (r.dk, dk), (r.dv, dv)):
        assert (A._blk(got - ref) <= 2.0 ** -6 * A._blk(ref)).all()
    assert A.check_all(r.out, r.lse, r.dq, r.dk, r.dv, f, r, "self") is not None        # the model passes its own check


# (S, H, dh, masked) -> (forward, backward, stages, chunks): the table of the GPU suite's route section, written out by hand
FF, FB = "attn_frame_fwd_kernel<%d>", "attn_frame_bwd_kernel<%d>"
KF, KB, ONCE = "attn_fwd_kernel<%d, %s>", "attn_bwd_kernel<%d, %s>", "attn_bwd_once_kernel<1024>"
TABLE = {
    # frame forward fit
    (128, 9, 16, False): (FF % 16, KB % (16, "false"), 1, 1), (128, 10, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 1),
    (65, 12, 16, False): (FF % 16, KB % (16, "false"), 1, 1), (65, 13, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 1),
    (128, 4, 32, False): (FF % 32, KB % (32, "false"), 1, 1), (128, 5, 32, False): (KF % (32, "false"), KB % (32, "false"), 1, 1),
    (128, 2, 64, False): (FF % 64, ONCE, 1, 1), (128, 3, 64, False): (KF % (64, "false"), ONCE, 1, 1),
    (128, 1, 16, False): (FF % 16, FB % 16, 1, 1), (129, 1, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 1),
    (128, 1, 32, False): (FF % 32, FB % 32, 1, 1), (129, 1, 32, False): (KF % (32, "false"), KB % (32, "false"), 1, 1),
    (128, 1, 64, False): (FF % 64, FB % 64, 1, 1), (129, 1, 64, False): (KF % (64, "false"), ONCE, 1, 1),
    # frame backward fit
    (65, 8, 16, False): (FF % 16, FB % 16, 1, 1), (65, 9, 16, False): (FF % 16, KB % (16, "false"), 1, 1),
    (128, 6, 16, False): (FF % 16, FB % 16, 1, 1), (128, 7, 16, False): (FF % 16, KB % (16, "false"), 1, 1),
    (128, 3, 32, False): (FF % 32, FB % 32, 1, 1),
    # once-kernel edge, forward stage edge, backward chunk edge
    (224, 1, 64, False): (KF % (64, "false"), ONCE, 1, 1), (225, 1, 64, False): (KF % (64, "false"), KB % (64, "false"), 2, 2),
    (384, 1, 32, False): (KF % (32, "false"), KB % (32, "false"), 1, 1), (385, 1, 32, False): (KF % (32, "false"), KB % (32, "false"), 2, 2),
    (416, 1, 32, False): (KF % (32, "false"), KB % (32, "false"), 2, 2), (417, 1, 32, False): (KF % (32, "false"), KB % (32, "false"), 2, 2),
    (1152, 1, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 2), (1153, 1, 16, False): (KF % (16, "false"), KB % (16, "false"), 2, 2),
    (1056, 1, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 1), (1057, 1, 16, False): (KF % (16, "false"), KB % (16, "false"), 1, 2),
    (449, 1, 64, False): (KF % (64, "false"), KB % (64, "false"), 3, 3),
    # masks never take the per-frame or the once kernel
    (17, 2, 16, True): (KF % (16, "true"), KB % (16, "true"), 1, 1), (225, 1, 64, True): (KF % (64, "true"), KB % (64, "true"), 2, 2),
    (197, 3, 64, True): (KF % (64, "true"), KB % (64, "true"), 1, 1), (385, 1, 32, True): (KF % (32, "true"), KB % (32, "true"), 2, 2),
}


@pytest.mark.parametrize("key", sorted(TABLE), ids=str)
def test_expected_kernels_table(key):
    assert A.expected_kernels(*key) == TABLE[key]


def test_restated_thresholds():
    assert A.frame_fwd_lds(128, 9, 16) == 112 * 1024                   # exactly the limit: fits
    assert [A.kchunk(4096, dh) for dh in (64, 32, 16)] == [224, 384, 1152]
    assert A.bwd_chunk_rows(225, 64) == 224 and A.bwd_chunk_rows(449, 64) == 224
    assert A.bwd_chunk_rows(384, 32) == 384 and A.bwd_chunk_rows(417, 32) == 384
    assert A.bwd_chunk_rows(1056, 16) == 1056 and A.bwd_chunk_rows(1057, 16) == 1056
    assert [A.heads_defeating_frame_fwd(S, 16) for S in (32, 64, 96, 128)] == [38, 19, 13, 10]
    assert [A.heads_defeating_frame_fwd(S, 32) for S in (32, 64, 96, 128)] == [19, 10, 7, 5]


# ------------------------------------------------------------------------------------------------
# exact case: the seeds keep the midpoint cells inside the cap
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bf,S,H,dh,seed", A.UNIFORM)
def test_uniform_reference_both_ways_within_the_midpoint_cap(Bf, S, H, dh, seed):
    for zero in "qk":
        qkv, _ = A.uniform_inputs(Bf, S, H, dh, zero, seed)
        mean = A.uniform_out_ref(qkv, Bf, S, H, dh)
        n = A.check_uniform_out(A.uniform_out_fp32_way(qkv, Bf, S, H, dh), mean, f"S={S} zero={zero}")
        assert n <= A.MID_SHARE * mean.numel()
        f = A.attn_fp64(qkv, torch.zeros(Bf * S, H * dh), None, Bf, S, H, dh)
        assert (f.out - mean).abs().max().item() < 1e-12                   # the scores are 0: attention IS the mean
        assert (f.lse - math.log(S)).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------
# self-checks: each check fails for the reason it exists
# ------------------------------------------------------------------------------------------------
def with_padding_key(qkv, dout, Bf, S, H, dh):
    """The same problem with one all-zero key / value row appended to every frame and counted: a padding key let in."""
    D = H * dh
    x = torch.zeros(Bf, S + 1, 3 * D, dtype=qkv.dtype)
    x[:, :S] = qkv.view(Bf, S, 3 * D)
    d = torch.zeros(Bf, S + 1, D, dtype=dout.dtype)
    d[:, :S] = dout.view(Bf, S, D)
    r = A.attn_rounded(x.view(-1, 3 * D), d.view(-1, D), None, Bf, S + 1, H, dh)
    return A.AttnRef(r.out[:, :, :S], r.lse[:, :, :S], r.dq[:, :, :S], r.dk[:, :, :S], r.dv[:, :, :S], None)


@pytest.mark.parametrize("Bf,S,H,dh", [(2, 33, 2, 16), (1, 225, 2, 64)])
def test_checks_catch_a_counted_padding_key(Bf, S, H, dh):
    qkv, dout, _ = inputs(Bf, S, H, dh)
    f, r = A.attn_fp64(qkv, dout, None, Bf, S, H, dh), A.attn_rounded(qkv, dout, None, Bf, S, H, dh)
    w = with_padding_key(qkv, dout, Bf, S, H, dh)
    with pytest.raises(AssertionError, match="a key counted that should not be"):
        A.check_lse(w.lse, f.lse, "extra key")
    if S == 33:         # 1 / 34 of every row: the block bound on out sees it too
        with pytest.raises(AssertionError, match="extra key out: frame"):
            A.check_part("out", w.out, f.out, r.out, f.mag["out"], "extra key")
    else:               # 1 / 226 is inside two bf16 budgets on out, and inside the older 2e-3 limit on lse: only the lse bound sees it
        assert (w.lse - f.lse).abs().max().item() < 2e-3 * (1 + f.lse.abs().max().item())


def test_checks_catch_a_dropped_key():
    Bf, S, H, dh = 2, 65, 2, 16
    qkv, dout, _ = inputs(Bf, S, H, dh)
    f, r = A.attn_fp64(qkv, dout, None, Bf, S, H, dh), A.attn_rounded(qkv, dout, None, Bf, S, H, dh)
    # dropped in ONE row of one block only: the global bounds of the older tests pass, the per-block / per-row ones do not
    mask = torch.ones(Bf, H, S, S, dtype=torch.bool)
    mask[1, 0, 7, S - 1] = False
    w = A.attn_rounded(qkv, dout, mask, Bf, S, H, dh)
    with pytest.raises(AssertionError, match="lse: 1 rows off, first frame 1 head 0 row 7.*live key dropped"):
        A.check_lse(w.lse, f.lse, "dropped key")
    with pytest.raises(AssertionError, match="dropped key out: .*frame 1 head 0"):
        A.check_part("out", w.out, f.out, r.out, f.mag["out"], "dropped key")
    packed = torch.cat([w.dq, w.dk, w.dv], -1) - torch.cat([f.dq, f.dk, f.dv], -1)
    scale = torch.cat([f.dq, f.dk, f.dv], -1).abs().max().item()
    assert packed.abs().max().item() <= 0.02 * scale                    # what test_attention_fwd_bwd asks: it passes
    with pytest.raises(AssertionError, match="dropped key dq: .*frame 1 head 0"):
        A.check_part("dq", w.dq, f.dq, r.dq, f.mag["dq"], "dropped key")


def test_checks_catch_blocks_swapped_between_heads():
    Bf, S, H, dh = 2, 33, 3, 32
    qkv, dout, _ = inputs(Bf, S, H, dh)
    f, r = A.attn_fp64(qkv, dout, None, Bf, S, H, dh), A.attn_rounded(qkv, dout, None, Bf, S, H, dh)
    for name in A.PARTS:
        got = getattr(r, name).clone()
        got[1, [0, 2]] = got[1, [2, 0]]
        with pytest.raises(AssertionError, match=f"swapped {name}: frame 1 head 0 block L2 error"):
            A.check_part(name, got, getattr(f, name), getattr(r, name), f.mag[name], "swapped")


def test_checks_catch_a_nan_inside_and_a_cell_outside():
    Bf, S, H, dh = 2, 17, 2, 16
    qkv, dout, _ = inputs(Bf, S, H, dh)
    f, r = A.attn_fp64(qkv, dout, None, Bf, S, H, dh), A.attn_rounded(qkv, dout, None, Bf, S, H, dh)
    got = r.dv.clone()
    got[0, 1, 16, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite cells inside the result, first at frame 0 head 1 row 16 col 3: a read outside"):
        A.check_part("dv", got, f.dv, r.dv, f.mag["dv"], "nan")
    lse = r.lse.clone()
    lse[1, 0, 2] = float("inf")
    with pytest.raises(AssertionError, match="lse: non-finite inside the result at frame 1 head 0 row 2"):
        A.check_lse(lse, f.lse, "nan")
    PAT = 0x7FC5
    raw = torch.full((4 + Bf * S + 4, H * dh), PAT, dtype=torch.int16)
    raw[4:4 + Bf * S] = 0x3F80
    A.check_surroundings(raw, 4, Bf * S, PAT, "fine")
    bad = raw.clone()
    bad[4 + Bf * S, 0] = 0
    with pytest.raises(AssertionError, match="1 cells written outside the result, first after it"):
        A.check_surroundings(bad, 4, Bf * S, PAT, "outside")
    bad = raw.clone()
    bad[3, 5] = 0
    with pytest.raises(AssertionError, match="written outside the result, first before it"):
        A.check_surroundings(bad, 4, Bf * S, PAT, "outside")
    bad = raw.clone()
    bad[4 + 16, 8:12] = PAT
    with pytest.raises(AssertionError, match="4 cells of the result never written, first at \\[16, 8\\]"):
        A.check_surroundings(bad, 4, Bf * S, PAT, "unwritten")


@pytest.mark.parametrize("S", [17, 225])
def test_uniform_check_catches_one_key_more_or_less(S):
    Bf, H, dh = 1, 1, 16
    qkv, _ = A.uniform_inputs(Bf, S, H, dh, "q", 1)
    mean = A.uniform_out_ref(qkv, Bf, S, H, dh)
    with pytest.raises(AssertionError, match="a padding key counted"):
        A.check_uniform_out(A.bf16r(mean * S / (S + 1)), mean, "extra")     # a zero padding row counted: l = S + 1
    v = A.parts_of(qkv, Bf, S, H, dh)[2]
    dropped = ((v.sum(2, keepdim=True) - v[:, :, S - 1:]) / (S - 1)).expand_as(mean)
    with pytest.raises(AssertionError, match="live key dropped"):
        A.check_uniform_out(A.bf16r(dropped), mean, "dropped")
