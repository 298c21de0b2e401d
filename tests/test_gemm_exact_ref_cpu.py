"""CPU: tests/gemm_exact_ref.py is what it says it is.

  * `expected` equals an independent plain-torch fp32 statement of the header's epilogue (+bias, relu, +pe with the row
    remap, dropout, *gate, +residual), one small shape per epilogue mode; the embedding remap and the dropout mask are
    written differently there (a view per frame; the flat keep_mask of the whole output tensor);
  * the integer bound holds for the largest K of the case tables, and random operands of that K stay inside it;
  * the operands of the LayerNorm-backward cases keep max|dX| < 128 for every (D, K) the GPU test uses;
  * `explain` names a skipped 32-deep K stage, and the variants it offers as causes differ from the true result.
"""
import pytest
import torch

import gemm_exact_ref as GR
from dropout_ref import keep_mask

MODES = {            # name: (residual, gate, pe)
    "plain": (False, False, False), "res": (True, False, False), "gate": (False, True, False),
    "res_gate": (True, True, False), "pe": (False, False, True)}


def operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    ints = lambda amp, *s: torch.randint(-amp, amp + 1, s, generator=g).to(torch.bfloat16)
    gate = torch.tensor([-1.0, -0.0, 0.0, 1.0])[torch.randint(0, 4, (M, N), generator=g)].to(torch.bfloat16)
    return ints(2, M, K), ints(2, N, K), ints(8, N).float(), ints(8, M, N), gate, g


def plain_fp32(A, B, bias, relu, pe, tok, seq, cls_off, drop, gate, residual):
    """The epilogue written directly, in fp32, on the [rows_out, N] output tensor -> (bf16 [rows_out, N], written rows)."""
    M, N = A.shape[0], B.shape[0]
    v = A.float() @ B.float().t()
    if bias is not None:
        v = v + bias
    if relu:
        v = torch.relu(v)
    if tok > 0:
        frames = M // tok
        out = torch.zeros(frames, seq, N)
        out[:, cls_off:cls_off + tok] = v.view(frames, tok, N) + pe[cls_off:cls_off + tok]
        written = torch.zeros(frames, seq, dtype=torch.bool)
        written[:, cls_off:cls_off + tok] = True
        v, written = out.view(-1, N), written.view(-1)
    else:
        written = torch.ones(M, dtype=torch.bool)
    if drop:
        keep = torch.from_numpy(keep_mask(GR.SEED, GR.STEP, GR.SITE, GR.P, v.numel())).view(-1, N)
        v = torch.where(keep, v * 2.0, torch.zeros(()))              # a dropped element is +0, whatever its sign was
    if gate is not None:
        v = torch.where(gate.float() > 0, v * 1.25, torch.zeros(()))
    if residual is not None:
        v = v + residual.float()
    return v.to(torch.bfloat16), written


@pytest.mark.parametrize("flags", [(0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0)], ids=lambda f: "b%dr%dd%d" % f)
@pytest.mark.parametrize("mode", list(MODES))
def test_expected_equals_a_plain_fp32_statement_of_the_epilogue(mode, flags):
    res, gt, emb = MODES[mode]
    with_bias, relu, drop = flags
    tok, seq, cls_off = (4, 5, 1) if emb else (0, 0, 0)
    M, N, K = (12 if emb else 13), 24, 40
    A, B, bias, R, G, g = operands(M, N, K, 11)
    pe = torch.randint(-8, 9, (seq, N), generator=g).float() if emb else None
    kw = dict(bias=bias if with_bias else None, relu=bool(relu), pe=pe, tok=tok, seq=seq, cls_off=cls_off, drop=bool(drop),
              gate=G if gt else None, residual=R if res else None)
    rows, got = GR.expected(A, B, **kw)
    ref, written = plain_fp32(A, B, **kw)
    assert torch.equal(rows, written.nonzero().flatten())
    assert torch.equal(got.view(torch.int16), ref[rows].view(torch.int16))
    if drop and not res:                                   # (a dropped element of a residual mode is the residual)
        assert 0.3 <(got.float() == 0).float().mean().item() < 0.95


def test_the_remap_moves_the_mask_with_the_output_row():
    A, B, bias, _, _, g = operands(12, 24, 40, 12)
    pe = torch.randint(-8, 9, (5, 24), generator=g).float()
    kw = dict(bias=bias, pe=pe, tok=4, seq=5, cls_off=1, drop=True)
    _, good = GR.expected(A, B, **kw)
    _, other = GR.expected(A, B, variant="mask_input_row", **kw)
    assert not torch.equal(good.view(torch.int16), other.view(torch.int16))


def test_integer_bound_holds_at_the_largest_k():
    GR.assert_exact(GR.K_MAX)
    assert GR.magnitude_bound(GR.K_MAX) == (GR.K_MAX * 4 + 16) * 2 * 1.25 + 8 < 2 ** 22
    A, B, bias, R, G, _ = operands(65, 72, GR.K_MAX, 13)
    pre = GR.epilogue(A.double() @ B.double().t(), bias=bias, keep=torch.ones(65, 72, dtype=torch.bool), gate=G, residual=R)
    assert pre.abs().max().item() <= GR.magnitude_bound(GR.K_MAX)
    assert torch.equal(pre * 4, (pre * 4).round())                        # multiples of 1/4
    assert torch.equal(pre.float().double(), pre)
    with pytest.raises(AssertionError):
        GR.assert_exact(2 ** 19)


def test_rounding_is_to_nearest_even_and_the_variants_differ():
    v = torch.tensor([257.0, 259.0, 258.5, -257.0, 1.25, 0.0], dtype=torch.float64)      # ties at 257 and 259 (ulp 2 above 256)
    assert GR.round_bf16(v).tolist() == [256.0, 260.0, 258.0, -256.0, 1.25, 0.0]
    assert GR.round_bf16(v, truncate=True).tolist() == [256.0, 258.0, 258.0, -256.0, 1.25, 0.0]
    acc = torch.tensor([[255.0, 3.0]], dtype=torch.float64)
    res = torch.tensor([[2.0, 1.0]]).to(torch.bfloat16)
    assert GR.stored(acc, residual=res).tolist() == [[256.0, 4.0]]                         # 257 -> 256
    assert GR.stored(acc * 1.0 + 1.0, residual=res).tolist() == [[258.0, 5.0]]
    acc = torch.tensor([[256.5, 3.0]], dtype=torch.float64)                                # 258.5 -> 258; rounded first: 256 + 2
    assert GR.stored(acc, residual=res).tolist() == [[258.0, 4.0]]
    assert GR.stored(acc, "res_after_round", residual=res).tolist() == [[258.0, 4.0]]
    acc = torch.tensor([[257.0]], dtype=torch.float64)                                     # 259 -> 260; rounded first: 256 + 2
    assert GR.stored(acc, residual=res[:, :1]).tolist() == [[260.0]]
    assert GR.stored(acc, "res_after_round", residual=res[:, :1]).tolist() == [[258.0]]
    gate = torch.tensor([[0.0, -0.0]]).to(torch.bfloat16)
    assert GR.stored(acc.expand(1, 2), gate=gate).tolist() == [[0.0, 0.0]]
    assert GR.stored(acc.expand(1, 2), "gate_ge", gate=gate).tolist() == [[322.0, 322.0]]  # 321.25 -> 322


@pytest.mark.parametrize("a,b,word", [(96, 128, "missing"), (64, 128, "missing"), (32, 64, "counted twice")])
def test_explain_names_the_k_range(a, b, word):
    A, B, bias, R, _, _ = operands(40, 24, 160, 14)
    epi = lambda rs, cs, acc: GR.stored(acc, bias=bias[cs], residual=R[rs, cs])
    _, want = GR.expected(A, B, bias=bias, residual=R)
    part = A[:, a:b].double() @ B[:, a:b].double().t()
    got = GR.stored(A.double() @ B.double().t() + (part if word == "counted twice" else -part), bias=bias, residual=R)
    assert f"k {a}..{b - 1} {word}" in GR.explain(A, B, got, want, epi)
    got = want.clone()
    got[3, 5] = float("nan")
    assert "read outside an operand" in GR.explain(A, B, got, want, epi)


@pytest.mark.parametrize("K", [64, 96, 384, 1024])
@pytest.mark.parametrize("D", [128, 192])
def test_lnbwd_operands_keep_dx_below_the_limit(D, K):
    A, Wt, R, z, gamma = GR.lnbwd_operands(D, K)
    assert A.shape == (GR.LNBWD_ROWS, K) and A.abs().max().item() == 1
    dX = GR.lnbwd_dx(A, Wt, R)
    assert torch.equal(dX, dX.round())
    peak = dX.abs().max().item()
    print(f"D={D} K={K}: max|dX| = {peak:.0f}, density {GR.lnbwd_density(K):.3f}")
    assert 16 < peak < GR.DX_LIMIT
    assert 0.5 <= gamma.min().item() and gamma.max().item() <= 1.5
    # a one-unit error in dX moves dz by about rstd * gamma: more than twice the bound at the typical cell
    zf = z[:1000].double()
    mean = zf.mean(-1).float()
    rstd = (1 / torch.sqrt(zf.var(-1, unbiased=False) + 1e-12)).float()
    dz, _, gmax, _ = GR.lnbwd_reference(dX[:1000], z[:1000], mean, rstd, gamma)
    bound = 2.0 ** -8 * dz.abs() + 2.0 ** -16 * gmax * rstd.double()[:, None]
    step = rstd.double()[:, None] * gamma.double() * (1 - 1 / D)         # d dz[m, n] / d dX[m, n], up to the xhat term's 1/D share
    assert (step / bound).median().item() > 2
