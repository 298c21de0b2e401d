"""Host statement of what the two one-launch chain kernels (csrc/ffn_chain.hip) must store, for tests/test_gpu_chain_exact.py.

include/iqvit.h and the two header comments of ffn_chain.hip, evaluated in fp64 on operands that hold small integers, so that
every fp32 value a kernel holds before a store is exact in ANY summation order (the kernels walk the k-slots of an MFMA step in
a permuted order) and the stored value is that number rounded once to bf16, to nearest even.  Dropout uses p = 0.5 with
gemm_exact_ref's SEED / STEP (scale exactly 2) at the three distinct sites SITE (attention output projection / norm1's
backward), SITE + 1 (hidden activation) and SITE + 2 (feed-forward output / norm2's backward); masks are indexed by output
element, row * F + col for H and row * D + col elsewhere.  Nothing here depends on a device.

  forward core   H = keep1 ? 2 relu(X1 W1^T + b1) : 0                  stored as bf16 AND consumed as a bf16 MFMA operand: it has to
                                                                       be representable, max relu(.) <= H_LIMIT = 128
                 Z = (keep2 ? 2 (H W2^T + b2) : 0) + X1                |H W2^T| < 2^22; hundreds to thousands: the ONE rounding shows
  PRE stage      Z1 = (keep0 ? 2 (A Wo^T + bo) : 0) + R
  POST stage     with gamma2 = 0 and an integer beta2 the norm's output is beta2 in every row: Yq = beta2 Wq^T + bq
  backward core  gH = (H > 0) ? 2 (dO W2t^T) : 0, |gH| <= 256;  dX1 = gH W1t^T + R, integers below DX_LIMIT (exact through the
                 kernel's rounding of dX1 to bf16); the dbeta half of `partial` = the column sums of dX1 over each workgroup's
                 NW * 16 RG rows (chain_shape)
  PREB stage     dX2 = gQKV Wqkv_t^T + R0 (gemm_exact_ref.lnbwd_operands(D, 3 D)), its dbeta partial rows likewise

Operands are drawn on the host from seeds that do not depend on M (a case with M rows uses the first M), so that
tests/test_chain_exact_ref_cpu.py confirms the amplitude conditions for exactly the numbers the GPU test uses.

The backward's dO.  dX1 is a product of a product: a dO thinned the way lnbwd_density thins A (independent cells) would leave
most rows of gH zero and put the whole variance of dX1 on the few rows that are not -- max|dX1| passes DX_LIMIT there while
nothing is tested elsewhere.  So the sparsity that keeps dX1 small has to sit in the hidden dimension of EVERY row: the
backward's first weight W2t is an operand of its own here (the entry point takes it as one; the gate bits depend on X1, W1
and b1 only) with exactly n = max(1, round(256 / F)) nonzero entries per hidden unit, and every row of dO holds exactly
D * BWD_TERMS / (F n) nonzero cells (at least one), so that every row of gH holds about BWD_TERMS * P(H > 0) nonzero cells at
hidden units that differ from row to row, and every row of dX1 has the same variance.
W1t is the forward's W1 transposed, dense.

The case table of the GPU test lives here too (SMALL_M, LARGE, cases()), so that the CPU test walks the same list.
"""
import functools

import numpy as np
import torch

import dropout_ref
import gemm_exact_ref as GR

SITE0, SITE1, SITE2 = GR.SITE, GR.SITE + 1, GR.SITE + 2
GATE_SCALE = 2.0
H_LIMIT = 128                     # max relu(X1 W1^T + b1): twice that is still an integer bf16 holds
GH_LIMIT = 256
ROWS = 32785                      # the most rows a case uses
AMP_X_VAR = 169.0                 # D * density * (2/3) * E[w^2 = 2] = 225: sigma 15, so that 128 - 8 is eight sigma
BWD_TERMS = 24.0                  # nonzero cells a row of dO W2t^T holds on average
F_LIMIT = {192: 2368, 128: 15232}                 # iq_ffn_chain_supported's last F: the b1 / vector region ends at 160 KB
WIDTHS = [64, 128, 192, 256, 832]                 # 1 to 4 ring chunks (fewer than, as many as, one more than the slots), 13

# Rows (chain_shape: 5 waves of 16 rows up to 20,480 rows, 8 of 16 up to 32,768, 7 of 32 above):
#   1, 15, 16, 17     around one 16-row wave          79, 80, 81     one full 5-wave workgroup and the next row
#   20,480 / 20,481   5 x 16 -> 8 x 16; the second has a last workgroup of ONE row and seven waves that only feed the ring
#   32,768 / 32,769   8 x 16 -> 7 x 32; the second has a wave whose second 16-row group is wholly past M and four trailing waves
#                     without rows           32,785   M mod 32 = 17: the second group is partly past M
# The full cross product is not run.  Every width meets M = 81 (two workgroups, the second ragged), a whole number of waves (16 or
# 80 rows: counted waits) and a ragged M at both D, the two F_LIMIT widths the small M only; every M meets both D.  Every large M
# meets both D, every width meets an 8 x 16 and a 7 x 32 launch, the 13-chunk width at both D (F small where M is large).
SMALL_M = [1, 15, 16, 17, 79, 80, 81]
SMALL = {128: {64: [1, 16, 81], 128: [15, 80, 81], 192: [17, 16, 81], 256: [79, 80, 81], 832: [17, 80, 81], 15232: [1, 16, 79, 81]},
         192: {64: [15, 80, 81], 128: [17, 16, 81], 192: [79, 80, 81], 256: [1, 16, 81], 832: [15, 16, 81], 2368: [1, 17, 80, 81]}}
LARGE = {20480: {128: [128], 192: [64]},
         20481: {128: [64, 832], 192: [128]},
         32768: {128: [192], 192: [256, 832]},
         32769: {128: [832], 192: [64, 192]},
         32785: {128: [128, 256], 192: [832]}}


def cases():
    """Every (M, D, F) of the GPU test."""
    out = [(M, D, F) for D, per_f in SMALL.items() for F, ms in per_f.items() for M in ms]
    out += [(M, D, F) for M, per_d in LARGE.items() for D, widths in per_d.items() for F in widths]
    return out


def max_rows(D, F):
    return max(m for m, d, f in cases() if (d, f) == (D, F))


VARIANTS = {
    "res_after_round": "the residual (X1 / R) was added after the rounding to bf16",
    "truncate": "the store truncated to bf16 instead of rounding to nearest even",
    "mask_stride_d": "the mask of H was indexed with row stride D instead of F",
    "gate_ge": "the gate kept the zeros of H (>= 0 instead of > 0)",
    "ragged_copies": "the rows of a ragged unit past M entered the dbeta sums as copies of row M - 1",
    "b1_mod_1024": "b1 was read modulo 1,024",
}


# ------------------------------------------------------------------------------------------------
# launch geometry (ffn_chain.hip::chain_shape)
# ------------------------------------------------------------------------------------------------
def chain_shape(M):
    """-> (waves per workgroup, 16-row groups per wave): 5 x 16 rows up to 20,480 rows, 8 x 16 up to 32,768, 7 x 32 above."""
    return (5, 1) if M <= 20480 else (8, 1) if M <= 32768 else (7, 2)


def units(M):
    return -(-M // (16 * chain_shape(M)[1]))


def partial_rows(M):
    return -(-units(M) // chain_shape(M)[0])


def gate_bytes(M, F):
    return units(M) * (F // 64) * 64 * 4


def amp_w(F):
    return 1 if F > 8192 else 2              # F = 15,232: F * 256 * 2 would pass 2^22


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def _ints(g, amp, *shape):
    return torch.randint(-amp, amp + 1, shape, generator=g, dtype=torch.int8)


def _thin(g, t, density):
    return t * (torch.rand(t.shape, generator=g) < density).to(t.dtype)


def _sparse(g, rows, cols, n, amp):
    """[rows, cols] int8 with exactly n nonzero cells per row, at random columns, drawn from +-1 .. +-amp."""
    at = torch.rand(rows, cols, generator=g).topk(n, dim=1).indices
    v = torch.randint(1, amp + 1, (rows, n), generator=g, dtype=torch.int8) * (torch.randint(0, 2, (rows, n), generator=g, dtype=torch.int8) * 2 - 1)
    return torch.zeros(rows, cols, dtype=torch.int8).scatter_(1, at, v)


def _comb(g, rows, cols, n):
    """[rows, cols] int8 with exactly n cells of +-1 per row: one in each of n stripes of cols // n columns, at a random place of
    its stripe, the stripes starting at a random column of the row (what _sparse gives, without a sort of rows * cols numbers)."""
    w = cols // n
    at = (torch.randint(0, cols, (rows, 1), generator=g) + torch.arange(n) * w + torch.randint(0, w, (rows, n), generator=g)) % cols
    v = torch.randint(0, 2, (rows, n), generator=g, dtype=torch.int8) * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.int8).scatter_(1, at, v)


def bwd_counts(D, F):
    """-> (nonzero entries per hidden unit of W2t, nonzero cells per row of dO): n_w n_o / D = BWD_TERMS / F."""
    n_w = max(1, round(256 / F))
    return n_w, max(1, round(D * BWD_TERMS / (F * n_w)))


@functools.lru_cache(maxsize=2)
def row_operands(D):
    """The [ROWS, D] operands, which do not depend on F: X1, A, R, the backward's residual and z1."""
    g = torch.Generator().manual_seed(104729 * D)
    o = {}
    o["X1"] = _thin(g, _ints(g, 1, ROWS, D), min(1.0, AMP_X_VAR / D))
    o["A"], o["R"], o["Rb"] = _ints(g, GR.AMP_A, ROWS, D), _ints(g, GR.AMP_E, ROWS, D), _ints(g, GR.AMP_E, ROWS, D)
    o["z1"] = (torch.randn(ROWS, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    return o


@functools.lru_cache(maxsize=2)
def operands(D, F):
    """Every host operand of the (D, F) cases (int8 / int16 integers; gamma / beta / z1 real), ROWS rows where rows there are."""
    g = torch.Generator().manual_seed(104729 * D + F)
    aw = amp_w(F)
    o = dict(row_operands(D))
    # forward core
    o["W1"], o["W2"] = _ints(g, aw, F, D), _ints(g, aw, D, F)
    o["b1"], o["b2"] = _ints(g, GR.AMP_E, F), _ints(g, GR.AMP_E, D)
    o["gamma"], o["beta"] = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    # PRE / POST
    o["Wo"], o["bo"] = _ints(g, GR.AMP_B, D, D), _ints(g, GR.AMP_E, D)
    o["gamma1"], o["beta1"] = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    # (bq in steps of 32 up to 256: beta2 Wq^T alone, sigma 80 to 100, would rarely pass 256, where the rounding shows)
    o["Wq"], o["bq"], o["beta_int"] = _ints(g, GR.AMP_B, 3 * D, D), _ints(g, GR.AMP_E, 3 * D).short() * 32, _ints(g, GR.AMP_E, D)
    # backward core: exactly n_w nonzero entries per hidden unit of W2t and n_o per row of dO, at random places, so that every
    # row of dO W2t^T holds about BWD_TERMS nonzero cells; with E[w^2 | w != 0] = 2.5, the scale 2, E[W1^2] = 2 and
    # P(H > 0) <= 1/2 the variance of dX1 - R is about BWD_TERMS / 2 * 4 * 2.5 * 2 = 240 in EVERY row: sigma 16 with R
    n_w, n_o = bwd_counts(D, F)
    o["W2t"] = _sparse(g, F, D, n_w, aw)
    o["dO"] = _comb(g, ROWS, D, n_o)
    o["W1t"] = o["W1"].t().contiguous()
    o["gamma_b"] = torch.rand(D, generator=g) + 0.5
    o["Wot"] = _ints(g, GR.AMP_B, D, D)
    return o


def preb_operands(D):
    """gQKV [*, 3 D], Wqkv_t [D, 3 D], R0, z2, gamma2: the LayerNorm-backward operands of gemm_exact_ref at K = 3 D."""
    return GR.lnbwd_operands(D, 3 * D, rows=ROWS)


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def keep(rows, ncols, site, stride=None):
    """Keep flags of columns 0 .. ncols - 1 of the rows `rows` of a row-major tensor whose rows are `stride` (= ncols) elements
    apart -> bool [len(rows), ncols] on rows' device."""
    if stride is None or stride == ncols:
        return GR.keep_rows(rows, ncols, site=site)
    assert stride % 8 == 0 and ncols % 8 == 0
    r = rows.detach().cpu().numpy().astype(np.uint64)
    groups = r[:, None] * np.uint64(stride // 8) + np.arange(ncols // 8, dtype=np.uint64)[None, :]
    k = dropout_ref.keep_groups(GR.SEED, GR.STEP, site, GR.P, groups).reshape(len(r), ncols)
    return torch.from_numpy(k).to(rows.device)


def _drop(v, k):
    return v if k is None else torch.where(k, v * GR.DROP_SCALE, torch.zeros((), dtype=torch.float64, device=v.device))


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def hidden_pre(X1, W1, b1, variant=None):
    """relu(X1 W1^T + b1) in fp64 (before dropout)."""
    b = b1.double()
    if variant == "b1_mod_1024":
        b = b[torch.arange(len(b), device=b.device) % 1024]
    return torch.clamp_min(X1.double() @ W1.double().t() + b, 0.0)


def hidden(X1, W1, b1, keep1=None, variant=None):
    """-> (H as the kernel stores it, bf16; its fp64 value).  keep1: bool [M, F] or None."""
    v = _drop(hidden_pre(X1, W1, b1, variant), keep1)
    return GR.round_bf16(v, truncate=(variant == "truncate")), v


def residual_store(v, res, variant=None):
    """(v + res) rounded once -- or as a VARIANT stores it."""
    if variant == "res_after_round":
        return (GR.round_bf16(v).float() + res.float()).to(torch.bfloat16)
    return GR.round_bf16(v + res.double(), truncate=(variant == "truncate"))


def z_acc(H, W2):
    """H W2^T in fp64 from the bf16 H the kernel holds."""
    return H.double() @ W2.double().t()


def z_store(acc, b2, X1, keep2=None, variant=None):
    """Z = (keep2 ? 2 (acc + b2) : 0) + X1, bf16."""
    return residual_store(_drop(acc + b2.double(), keep2), X1, variant)


def z1_store(A, Wo, bo, R, keep0=None, variant=None):
    return residual_store(_drop(A.double() @ Wo.double().t() + bo.double(), keep0), R, variant)


def yq_of_beta(beta_int, Wq, bq):
    """The row every row of Yq holds when gamma2 = 0: beta2 Wq^T + bq, bf16 [3 D]."""
    return GR.round_bf16(Wq.double() @ beta_int.double() + bq.double())


def assert_forward_exact(D, F, h_max):
    """|H W2^T + b2| doubled, plus X1, stays an integer below 2^23 whose partial sums stay below 2^22."""
    assert h_max <= H_LIMIT, f"max relu(X1 W1^T + b1) = {h_max} > {H_LIMIT}: H would not be representable"
    assert F * 2 * H_LIMIT * amp_w(F) + GR.AMP_E < 2 ** 22, "partial sums of H W2^T must stay exact in fp32"
    GR.assert_exact(D, pe=False, gate=False)                    # X1 W1^T + b1 and A Wo^T + bo


def layernorm(Z, gamma, beta, eps):
    """fp64 LayerNorm of the bf16 Z -> X, mean, rstd."""
    zb = Z.double()
    mu = zb.mean(-1, keepdim=True)
    var = zb.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    return gamma.double() * ((zb - mu) * rstd) + beta.double(), mu.squeeze(-1), rstd.squeeze(-1)


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
def gh_acc(dO, W2t):
    return dO.double() @ W2t.double().t()


def gh_store(acc, Hexp, variant=None):
    """gH = (H > 0) ? 2 acc : 0 -> (bf16, fp64).  Hexp: the forward statement's H (any float type)."""
    gate = (Hexp.double() >= 0) if variant == "gate_ge" else (Hexp.double() > 0)
    v = torch.where(gate, acc * GATE_SCALE, torch.zeros((), dtype=torch.float64, device=acc.device))
    return GR.round_bf16(v, truncate=(variant == "truncate")), v


def dx_of(gH, W1t, R):
    """dX1 = gH W1t^T + R in fp64: integers."""
    return gH.double() @ W1t.double().t() + R.double()


def dbeta_rows(dX, M, variant=None):
    """The dbeta half of `partial`: column sums of dX [M, D] over each workgroup's rows -> fp64 [partial_rows(M), D]."""
    nw, rg = chain_shape(M)
    per = nw * 16 * rg
    n = partial_rows(M)
    pad = torch.zeros(n * per, dX.shape[1], dtype=torch.float64, device=dX.device)
    pad[:M] = dX[:M].double()
    if variant == "ragged_copies":
        pad[M:units(M) * 16 * rg] = dX[M - 1].double()
    return pad.view(n, per, -1).sum(1)


def dgamma_rows(dX, xhat, M):
    nw, rg = chain_shape(M)
    per = nw * 16 * rg
    n = partial_rows(M)
    pad = torch.zeros(n * per, dX.shape[1], dtype=torch.float64, device=dX.device)
    pad[:M] = dX[:M].double() * xhat[:M]
    return pad.view(n, per, -1).sum(1)
