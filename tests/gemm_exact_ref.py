"""Host statement of what the forward / data-gradient GEMM family must store, for tests/test_gpu_gemm_exact.py.

The epilogue of include/iqvit.h, in its order: +bias, relu, +pe (row remap), dropout, *gate, +residual, evaluated in fp64 on
operands that hold small integers, so that every product, partial sum and epilogue step is an integer (or an integer times
1.25) far below 2^24: the fp32 value a kernel holds before its store is then exact in ANY summation order, and the stored
value is that number rounded once to bf16, to nearest even (fp64 -> fp32 -> bf16).  Nothing here depends on a device; the
keep mask is tests/dropout_ref.py's, indexed by OUTPUT element row_out * N + n.

The module also holds the operands of the LayerNorm-backward cases (`lnbwd_operands`): they are drawn on the host from seeds
that do not depend on M, so that tests/test_gemm_exact_ref_cpu.py can confirm the amplitude condition max|dX| < 128 for
exactly the numbers the GPU test uses.
"""
import numpy as np
import torch

import dropout_ref

SEED, STEP, SITE, P = 0x9E3779B97F4A7C15, 7, 11, 0.5        # four distinct counter / key words; thresh 32768, scale exactly 2
DROP_SCALE = float(dropout_ref.dropout_scale(P))
GATE_SCALE = 1.25
AMP_A, AMP_B, AMP_E = 2, 2, 8                                # |A|, |B| <= 2; |bias|, |pe|, |residual| <= 8
K_MAX = 4104                                                 # the largest contraction in the case tables
LNBWD_ROWS = 40961                                           # the most rows an lnbwd case uses
DX_LIMIT = 128                                               # max|dX| of the lnbwd cases stays below this

VARIANTS = {
    "res_after_round": "the residual was added after the rounding to bf16",
    "mask_input_row": "the dropout mask was indexed by the input row, not the output row",
    "truncate": "the store truncated to bf16 instead of rounding to nearest even",
    "gate_ge": "the gate kept its zeros (>= 0 instead of > 0)",
}


def magnitude_bound(K, bias=True, pe=True, drop=True, gate=True, residual=True, amp_a=AMP_A, amp_b=AMP_B):
    """Largest magnitude any intermediate of the epilogue can reach."""
    v = K * amp_a * amp_b + (AMP_E if bias else 0) + (AMP_E if pe else 0)
    v *= DROP_SCALE if drop else 1.0
    v *= GATE_SCALE if gate else 1.0
    return v + (AMP_E if residual else 0)


def assert_exact(K, **kw):
    """Every intermediate is a multiple of 1/4 (the gate scale is 5/4) below 2^22: exact in fp32, in any order."""
    assert DROP_SCALE == 2.0 and GATE_SCALE == 1.25
    assert magnitude_bound(K, **kw) < 2 ** 22, "partial sums and epilogue steps must stay exact in fp32"


def out_rows(M, tok=0, seq=0, cls_off=0, device="cpu"):
    """Output row of every input row: the identity, or the embedding remap (m / tok) * seq + m % tok + cls_off."""
    m = torch.arange(M, device=device)
    return m if tok <= 0 else (m // tok) * seq + m % tok + cls_off


def keep_rows(rows, N, seed=SEED, step=STEP, site=SITE, p=P):
    """Keep flags of the output rows `rows` (integer tensor) of a row-major [*, N] tensor -> bool [len(rows), N], same device."""
    assert N % 8 == 0
    r = rows.detach().cpu().numpy().astype(np.uint64)
    groups = r[:, None] * np.uint64(N // 8) + np.arange(N // 8, dtype=np.uint64)[None, :]       # (row * N + col) >> 3
    keep = dropout_ref.keep_groups(seed, step, site, p, groups).reshape(len(r), N)
    return torch.from_numpy(keep).to(rows.device)


def epilogue(acc, bias=None, relu=False, pe=None, keep=None, gate=None, residual=None, gate_ge=False):
    """The fp64 value before the store.  Operands broadcast against acc [..., rows, cols]; pe is already gathered per row."""
    v = acc.double()
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    if bias is not None:
        v = v + bias.double()
    if relu:
        v = torch.clamp_min(v, 0.0)
    if pe is not None:
        v = v + pe.double()
    if keep is not None:
        v = torch.where(keep, v * DROP_SCALE, zero)
    if gate is not None:
        v = torch.where((gate.double() >= 0) if gate_ge else (gate.double() > 0), v * GATE_SCALE, zero)
    if residual is not None:
        v = v + residual.double()
    return v


def round_bf16(v, truncate=False):
    """fp64 -> fp32 (exact here) -> bf16, round to nearest even."""
    f = v.float()
    assert torch.equal(f.double(), v), "the value before the store must be exact in fp32"
    if truncate:
        f = (f.view(torch.int32) & -65536).view(torch.float32)
    return f.to(torch.bfloat16)


def stored(acc, variant=None, keep_in=None, **epi):
    """bf16 result of the epilogue on an accumulator, as the header says -- or as one of VARIANTS would have stored it
    (keep_in: the mask taken at the INPUT rows, for "mask_input_row")."""
    if variant == "res_after_round" and epi.get("residual") is not None:
        res = epi.pop("residual")
        return (round_bf16(epilogue(acc, **epi)).float() + res.float()).to(torch.bfloat16)
    if variant == "mask_input_row" and epi.get("keep") is not None:
        epi["keep"] = keep_in
    return round_bf16(epilogue(acc, gate_ge=(variant == "gate_ge"), **epi), truncate=(variant == "truncate"))


def expected(A, B, bias=None, relu=False, pe=None, tok=0, seq=0, cls_off=0, drop=False, gate=None, residual=None,
             variant=None):
    """-> (output rows [M], bf16 [M, N] in input-row order) of iq_gemm_bf16_nt on value tensors A [M, K], B [N, K]."""
    M, N = A.shape[0], B.shape[0]
    rows = out_rows(M, tok, seq, cls_off, A.device)
    acc = A.double() @ B.double().t()
    pe_rows = pe[torch.arange(M, device=A.device) % tok + cls_off] if pe is not None else None
    keep = keep_rows(rows, N) if drop else None
    keep_in = keep_rows(torch.arange(M, device=A.device), N) if drop and variant == "mask_input_row" else None
    return rows, stored(acc, variant, keep_in, bias=bias, relu=relu, pe=pe_rows, keep=keep, gate=gate, residual=residual)


def explain(A, B, got, want, epi_box):
    """Where a wrong [M, N] result (input-row order) is wrong, and whether ONE contiguous range of k, aligned to 64 or 32,
    explains it.  epi_box(rows slice, cols slice, acc [..., r, c]) -> the bf16 the epilogue stores for those cells."""
    K = A.shape[1]
    bad = got.view(torch.int16) != want.view(torch.int16)
    idx = bad.nonzero()
    r0, r1, c0, c1 = (int(v) for v in (idx[:, 0].min(), idx[:, 0].max(), idx[:, 1].min(), idx[:, 1].max()))
    msg = f"{len(idx)} wrong cells ({int(got.isnan().sum())} NaN) within rows {r0}..{r1}, cols {c0}..{c1}"
    a0, b0 = int(idx[0, 0]), int(idx[0, 1])                  # a 16 x 16 box at the first wrong cell: one tile, one cause
    rs, cs = slice(a0, min(a0 + 16, r1 + 1)), slice(b0, min(b0 + 16, c1 + 1))
    box, gbox = bad[rs, cs], got[rs, cs]
    if gbox[box].isnan().any():
        return msg + "; NaN at the first wrong cell: a read outside an operand, or a cell nobody wrote"
    where = f"(cells rows {rs.start}..{rs.stop - 1}, cols {cs.start}..{cs.stop - 1})"
    Ab, Bb = A[rs].double(), B[cs].double()
    acc = Ab @ Bb.t()
    for unit in (64, 32):
        nb = (K + unit - 1) // unit
        Ap = torch.zeros(Ab.shape[0], nb * unit, dtype=torch.float64, device=A.device)
        Bp = torch.zeros(Bb.shape[0], nb * unit, dtype=torch.float64, device=A.device)
        Ap[:, :K], Bp[:, :K] = Ab, Bb
        contrib = torch.einsum("rbu,cbu->brc", Ap.view(-1, nb, unit), Bp.view(-1, nb, unit))
        Pre = torch.cat([torch.zeros_like(contrib[:1]), contrib.cumsum(0)])
        for a in range(nb):
            d = Pre[a + 1:] - Pre[a]                         # k a * unit .. (a + 1 + j) * unit
            for sign, word in ((-1.0, "missing"), (1.0, "counted twice")):
                cand = epi_box(rs, cs, acc + sign * d)
                hit = ((cand.view(torch.int16) == gbox.view(torch.int16)) | ~box).flatten(1).all(1).nonzero()
                if len(hit) and int(box.sum()) < 8:
                    return msg + f"; too few wrong cells at the first one to name a k range {where}"
                if len(hit):
                    b = a + 1 + int(hit[0])
                    return msg + f"; k {a * unit}..{min(b * unit, K) - 1} {word} {where}"
    return msg + f"; no single 32- or 64-aligned k range explains it {where}"


# ------------------------------------------------------------------------------------------------
# operands of the LayerNorm-backward cases
# ------------------------------------------------------------------------------------------------
def lnbwd_density(K):
    """Share of A that may be nonzero: var(dX) = K * density * (2/3) * var(Wt) + var(R) stays near 256 + 24 whatever K is,
    so max|dX| over 8 M cells (7.5 sigma would be 125) stays below DX_LIMIT."""
    return min(1.0, 192.0 / K)


def lnbwd_operands(D, K, rows=LNBWD_ROWS):
    """Host operands of iq_gemm_bf16_lnbwd for (D, K); a case with M rows uses the first M.  A in {-1, 0, 1} thinned to
    lnbwd_density(K), Wt in [-2, 2], R in [-8, 8] (integers), z random bf16, gamma in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(7919 * D + K)
    A = torch.randint(-1, 2, (rows, K), generator=g, dtype=torch.int8)
    A = A * (torch.rand(rows, K, generator=g) < lnbwd_density(K)).to(torch.int8)
    Wt = torch.randint(-AMP_B, AMP_B + 1, (D, K), generator=g, dtype=torch.int8)
    R = torch.randint(-AMP_E, AMP_E + 1, (rows, D), generator=g, dtype=torch.int8)
    z = (torch.randn(rows, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    gamma = torch.rand(D, generator=g) + 0.5
    return A, Wt, R, z, gamma


def lnbwd_dx(A, Wt, R):
    """dX = A Wt^T + R in fp32: integers below 2^24, exact on any device and in any order."""
    return A.float() @ Wt.float().t() + R.float()


def lnbwd_reference(dX, z, mean, rstd, gamma, keep=None):
    """fp64 LayerNorm backward on exact inputs (mean, rstd: the fp32 values the kernel is given) -> dz, dy, rowmax|g|."""
    dX, z, mean, rstd, gamma = dX.double(), z.double(), mean.double()[:, None], rstd.double()[:, None], gamma.double()
    g = dX * gamma
    xhat = (z - mean) * rstd
    dz = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    dy = torch.where(keep, dz * DROP_SCALE, torch.zeros_like(dz)) if keep is not None else None
    return dz, dy, g.abs().amax(-1, keepdim=True), xhat
