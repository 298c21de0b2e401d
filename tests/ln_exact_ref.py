"""Host statement of what the stand-alone LayerNorm kernels (csrc/layernorm.hip) must store, for tests/test_gpu_ln_exact.py.

Launch geometry.  `instance(D)` restates ln_shape, ln_dispatch and ln_masked_nv: a row is owned by LPR lanes of a wave that hold
NV 16-byte vectors each (D = LPR * NV * 8, the 20 pairs of TABLE), any other multiple of 8 up to 2048 by one whole wave whose lanes
past D / 8 vectors are masked off (NV = 1 .. 4).  A wave holds 64 / LPR rows, a workgroup of four waves RPB = 256 / LPR (masked: 4).
The forward launches at most 4096 workgroups, the backward at most 512, and walks the rest in a grid-stride loop: workgroup b owns
rows [b RPB + k nblk RPB, b RPB + k nblk RPB + RPB) for k = 0, 1, ..., and writes ONE partial row of 2 D floats (dgamma | dbeta).

Exact operands.  Everything is integer arithmetic on torch tensors, identical on any device (the patterns of a width come from a
seeded host generator, once):
  forward    z[r, c] = m_r + s_r sign[r, c]: sign holds as many +1 as -1, in an order rotated (and flipped) per row, s_r from
             {0.5, 1, 2, 4}, m_r a small integer that differs between neighbouring rows.  Row sum D m_r, squared deviations s_r^2
             and xhat = +-1 are exact in fp32 in any order; mean = m_r when fl(fl(D m) fl(1 / D)) == m, which `means(D)` keeps
             only the candidates for which it holds (zero always does); rstd = 1 / s_r.  gamma = c % 13 - 6, beta = c % 7 - 3:
             X = gamma sign + beta, an integer a bf16 holds.
  backward   gamma from {+-1, +-2, +-4}; g = dX gamma = 4 k1_r + sign (4 k2_r + u[r, c]) with u a multiple of 4 that is the same
             on the two columns of a (+1, -1) pair and sums to zero over the pairs (they come as +w, -w): sum g = 4 k1 D,
             sum g xhat = 4 k2 D, so c1 = 4 k1, c2 = 4 k2 and dZ = rstd (g - c1 - xhat c2) = sign u / s_r.  |g| <= 32, dX = g / gamma
             an integer; dbeta = sum_r dX and dgamma = sum_r dX sign stay below 2^24 for 131,073 rows.
  dropout    p = 0.5: scale exactly 2; dy = 2 dZ or +0 by the mask of tests/dropout_ref.py on group (row * D + col) >> 3.  `keep`
             restates dropout_ref.keep_groups in torch int64 arithmetic (products of two 32-bit words wrap in int64 without
             changing any of their 64 bits) so that it runs where the tensors are; tests/test_ln_exact_ref_cpu.py pins it.

Real operands.  `forward64` / `backward64`: the fp64 statement of the same bf16 inputs.  They also state the wrong kernels of
VARIANTS, each of which must change a stored value on the exact operands (the CPU test confirms it at every width it applies to).
"""
import functools

import torch

import dropout_ref
import gemm_exact_ref as GR

TABLE = [(64, 1), (64, 2), (64, 3), (64, 4), (32, 1), (32, 3), (32, 5), (16, 1), (16, 3), (16, 5), (8, 1), (8, 3), (8, 5),
         (4, 1), (4, 3), (4, 5), (2, 1), (2, 3), (1, 1), (1, 3)]
FWD_CAP, BWD_CAP = 4096, 512            # workgroups a launch has at most (LN_FWD_MAX_BLOCKS, LN_MAX_BLOCKS)
D_MAX = 2048
# one width per instance: the 20 of the table, then masked NV = 1 (56, 136), 2 (520, 1016), 3 (1048), 4 (1544, 2040)
WIDTHS = [8, 24, 16, 48, 32, 96, 160, 64, 192, 320, 128, 384, 640, 256, 768, 1280, 512, 1024, 1536, 2048,
          56, 136, 520, 1016, 1048, 1544, 2040]
SITE, SEED, STEP, P = GR.SITE, GR.SEED, GR.STEP, GR.P

CANDIDATE_MEANS = (0, 1, -2, 3, 5, -7, 16)
SCALES = (0.5, 1.0, 2.0, 4.0)
K1, K2 = (0, 1, -2, 4), (0, -1, 2)
E_ROW = (1, -1, 2)                       # per-row multiplier of u
GAMMA_B = (1, -2, 4, -1, 2, -4)
G_LIMIT = 32                             # max |dX gamma| of the recipe: 4 * 4 + 4 * 2 + 2 * 4

VARIANTS = {
    "var_dm1": "the variance was taken over D - 1",
    "wide_reduce": "the statistics were summed across the neighbouring row of the same wave (a reduction one step too wide)",
    "transposed_gamma": "gamma and beta were read with the lane-to-vector mapping transposed (j * NV + v instead of v * LPR + j)",
    "tail_in_var": "the masked tail columns were counted in the variance",
    "dgamma_times_gamma": "dgamma was summed from dX * gamma * xhat instead of dX * xhat",
    "padded_div": "c1 / c2 were divided by the padded width 64 * NV * 8 of the masked kernel",
    "mask_no_row": "the dropout group was taken without the row offset",
    "last_stripe_missing": "the last grid-stride stripe was missing from the partial rows",
    "accumulate_ignored": "the reduce ignored `accumulate`",
}


# ------------------------------------------------------------------------------------------------
# launch geometry
# ------------------------------------------------------------------------------------------------
def instance(D):
    """-> (LPR, NV, masked) of the kernel instance that runs width D, or None where iq_ln_supported(D) is 0."""
    if D <= 0 or D % 8:
        return None
    v, lpr = D // 8, 1
    while lpr < 64 and v % (lpr * 2) == 0:
        lpr *= 2
    if (lpr, v // lpr) in TABLE:
        return lpr, v // lpr, False
    return (64, (v + 63) // 64, True) if D <= D_MAX else None


def rpw(D):
    return 64 // instance(D)[0]


def rpb(D):
    return 4 * rpw(D)


def grid(M, D, cap):
    return min(max(-(-M // rpb(D)), 1), cap)


def partial_rows(M, D):
    return 0 if M <= 0 or instance(D) is None else grid(M, D, BWD_CAP)


def ws_bytes(D):
    return BWD_CAP * 2 * D * 4


def lds_bytes(D):
    """Dynamic LDS of the backward: red[RPB][2 D] floats."""
    return rpb(D) * 2 * D * 4


def fwd_name(D):
    lpr, nv, masked = instance(D)
    return "ln_fwd_kernel<%d, %d, %s>" % (lpr, nv, "true" if masked else "false")


def bwd_name(D, drop):
    lpr, nv, masked = instance(D)
    return "ln_bwd_kernel<%d, %d, %s, %s>" % (lpr, nv, "true" if drop else "false", "true" if masked else "false")


def row_edges(D):
    """The row counts every instance meets: one row, both sides of a wave and of a workgroup, two workgroups and a row, and both
    sides of the backward's grid-stride loop."""
    w, b = rpw(D), rpb(D)
    return sorted({m for m in (1, w - 1, w, b - 1, b, b + 1, 2 * b + 1, BWD_CAP * b, BWD_CAP * b + 1) if m > 0})


def fwd_cap_widths():
    """{rows per workgroup: the narrowest width of WIDTHS with that many} -- where the forward's grid-stride loop is met."""
    out = {}
    for D in sorted(WIDTHS):
        out.setdefault(rpb(D), D)
    return out


# ------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's scalar expressions (numpy.float32)
# ------------------------------------------------------------------------------------------------
def _f32_scaled(total, D):
    """fl(fl(total) * fl(1 / D)): what the kernel makes of an exact sum."""
    import numpy as np
    return np.float32(total) * (np.float32(1.0) / np.float32(D))


def mean_is_exact(m, D):
    return float(_f32_scaled(D * m, D)) == float(m)


@functools.lru_cache(maxsize=None)
def means(D):
    """The candidate means the kernel's fp32 expression returns exactly at width D."""
    return tuple(m for m in CANDIDATE_MEANS if mean_is_exact(m, D))


def stats_are_exact(D, eps=1e-12):
    """var = s^2 and rstd = 1 / s for every scale, c1 = 4 k1 and c2 = 4 k2 for every k, in the kernel's fp32 expressions."""
    import numpy as np
    for s in SCALES:
        var = _f32_scaled(D * s * s, D)
        rstd = np.float32(1.0) / np.sqrt(np.float32(var + np.float32(eps)), dtype=np.float32)
        if float(var) != s * s or float(rstd) != 1.0 / s:
            return False
    return all(float(_f32_scaled(4 * k * D, D)) == 4.0 * k for k in K1 + K2)


# ------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def patterns(D):
    """-> (base sign pattern [D] of +-1, D / 2 of each; ubase [D], multiples of 4 equal on the two columns of a pair, zero sum
    over the pairs; the same with +-4 where ubase is zero, for the centred recipe).  Host tensors, int64."""
    g = torch.Generator().manual_seed(48611 * D + 7)
    perm = torch.randperm(D, generator=g)
    base = torch.ones(D, dtype=torch.int64)
    base[perm[:D // 2]] = -1
    plus, minus = (base == 1).nonzero().flatten(), perm[:D // 2]           # pair t = (plus[t], minus[t])
    a = (torch.randint(-1, 2, (D // 4,), generator=g) * 4)
    a[0] = 4
    w = torch.stack([a, -a], 1).flatten()                                  # D / 2 values, +a and -a side by side
    ubase = torch.zeros(D, dtype=torch.int64)
    ubase[plus], ubase[minus] = w, w
    return base, ubase, torch.where(ubase == 0, 4 * _pair_sign(D, plus, minus), ubase)


def _pair_sign(D, plus, minus):
    """+1 on the columns of the even pairs, -1 on those of the odd ones: a zero-sum filler for the pairs whose u is zero."""
    t = torch.zeros(D, dtype=torch.int64)
    alt = 1 - 2 * (torch.arange(D // 2) % 2)
    t[plus], t[minus] = alt, alt
    return t


@functools.lru_cache(maxsize=None)
def _dev_patterns(D, device):
    return tuple(t.to(device) for t in patterns(D))


def _pick(values, idx, dtype=torch.float64):
    return torch.tensor(values, dtype=dtype, device=idx.device)[idx]


def row_params(rows, D, zero_rows=(), centred=False):
    """Per-row parameters of the rows `rows` (int64 tensor) -> dict of fp64 / int64 tensors [len(rows)].  centred: the recipe of
    the all-widths sweep, m = k1 = k2 = 0 in every row, so that mean, c1 and c2 are zero times 1 / D: exact at ANY width."""
    h = (rows * 2654435761 + 40503) & 0xFFFFFFFF
    ms = (0,) if centred else means(D)
    p = dict(m=_pick(ms, rows % len(ms)), s=_pick(SCALES, (h >> 5) & 3), flip=1 - 2 * ((h >> 11) & 1),
             e=_pick(E_ROW, (h >> 15) % 3, torch.int64), shift=((h >> 3) + rows) % D,
             k1=_pick((0,) if centred else K1, rows % (1 if centred else 4)), k2=_pick((0,) if centred else K2, rows % (1 if centred else 3)))
    for r in zero_rows:
        p["m"][rows == r] = 0.0
        p["s"][rows == r] = 0.0
    return p


def exact_case(rows, D, zero_rows=(), centred=False):
    """The exact operands and results of the rows `rows` at width D, fp64 tensors on rows' device:
    z, X, mean, rstd (forward with fwd_gamma / fwd_beta), dX, dZ, sign (= xhat), live (0 on an all-zero row).

    centred (the all-widths sweep): at 38 of the 256 widths fl(D s^2 fl(1 / D)) misses s^2 by an ulp, so rstd = (1 + d) / s with
    |d| <= 2^-22 and xhat = +-(1 + d).  With m = k1 = k2 = 0 the kernel holds X = gamma (+-(1 + d)) + beta and
    dZ = rstd (g - 0 - xhat 0) = (1 + d) sign u / s in fp32: within 2^-20 relative of an integer or half-integer of magnitude
    <= 16 that is NOT zero -- the sweep adds 1/2 to beta (allwidths_beta) and takes u from +-4, +-8 only, since c2 need not
    cancel to the last bit there either -- so the rounding to bf16 returns exactly that number."""
    base, ubase, ubase_nz = _dev_patterns(D, rows.device)
    if centred:
        ubase = ubase_nz
    p = row_params(rows, D, zero_rows, centred)
    at = (torch.arange(D, device=rows.device)[None, :] + p["shift"][:, None]) % D
    sign = (base[at] * p["flip"][:, None]).double()
    u = (ubase[at] * p["e"][:, None]).double()
    s, m = p["s"][:, None], p["m"][:, None]
    live = (s != 0).double()
    gamma, beta = fwd_gamma(D, rows.device).double(), (allwidths_beta if centred else fwd_beta)(D, rows.device).double()
    g = 4 * p["k1"][:, None] + sign * (4 * p["k2"][:, None] + u)
    return dict(z=m + s * sign, X=gamma * (sign * live) + beta, mean=p["m"], rstd=1 / p["s"], sign=sign, live=live,
                dX=g / bwd_gamma(D, rows.device).double(), dZ=sign * u / s + 0.0, g=g)


def fwd_gamma(D, device="cpu"):
    return (torch.arange(D, device=device) % 13 - 6).float()


def fwd_beta(D, device="cpu"):
    return (torch.arange(D, device=device) % 7 - 3).float()


def allwidths_beta(D, device="cpu"):
    """beta of the all-widths sweep: a half-integer, so that no X = gamma sign + beta is zero."""
    return fwd_beta(D, device) + 0.5


def bwd_gamma(D, device="cpu"):
    c = torch.arange(D, device=device)
    return _pick(GAMMA_B, (c * 5 + c // 8) % 6, torch.float32)


def to_bf16(v):
    """fp64 -> bf16 of a value a bf16 holds (asserted)."""
    b = v.float().to(torch.bfloat16)
    assert torch.equal(b.double(), v), "the operand / expected output must be representable in bf16"
    return b


# ------------------------------------------------------------------------------------------------
# dropout mask (dropout_ref.keep_groups in torch int64 arithmetic)
# ------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def keep(rows, D, p=P, site=SITE, seed=SEED, step=STEP, row_offset=True):
    """Keep flags of the rows `rows` of a row-major [*, D] tensor -> bool [len(rows), D] on rows' device."""
    assert D % 8 == 0
    g = torch.arange(D // 8, device=rows.device)[None, :] + (rows[:, None] * (D // 8) if row_offset else 0 * rows[:, None])
    c0, c1 = g & _M32, g >> 32
    c2, c3 = torch.full_like(g, site), torch.full_like(g, step)
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(dropout_ref.ROUNDS):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57                 # 32 x 32 bits: int64 wraps, every bit of the product stays
        c0, c1, c2, c3 = ((p1 >> 32) & _M32) ^ c1 ^ k0, p1 & _M32, ((p0 >> 32) & _M32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    w = torch.stack([c0, c1, c2, c3], -1)                                      # [rows, groups, word]
    u16 = torch.stack([w & 0xFFFF, w >> 16], -1)                               # element 2 * word + half
    return (u16 >= dropout_ref.dropout_thresh(p)).reshape(len(rows), D)


def dropped(dz, keep_, p=P):
    """dy of a dz (fp64): kept elements times the fp32 scale, dropped ones +0."""
    return torch.where(keep_, dz * float(dropout_ref.dropout_scale(p)), torch.zeros_like(dz))


# ------------------------------------------------------------------------------------------------
# the fp64 statement (and the wrong kernels of VARIANTS)
# ------------------------------------------------------------------------------------------------
def _padded(D):
    return 64 * instance(D)[1] * 8


def forward64(z, gamma, beta, eps, variant=None):
    """fp64 LayerNorm of z [M, D] -> X, mean [M], rstd [M]."""
    zb = z.double()
    M, D = zb.shape
    total, n = zb.sum(-1, keepdim=True), 1
    other = None
    if variant == "wide_reduce" and rpw(D) >= 2:
        other = torch.zeros_like(zb)
        idx = torch.arange(M, device=zb.device) ^ 1
        other[idx < M] = zb[idx[idx < M]]
        total = total + other.sum(-1, keepdim=True)
    mean = total / D
    q = ((zb - mean) ** 2).sum(-1, keepdim=True)
    if other is not None:
        q = q + ((other - mean) ** 2).sum(-1, keepdim=True)
    if variant == "tail_in_var" and instance(D)[2]:
        q = q + (_padded(D) - D) * mean ** 2
    var = q / (D - 1 if variant == "var_dm1" else D)
    rstd = 1 / torch.sqrt(var + eps)
    ga, be = gamma.double(), beta.double()
    lpr, nv, _ = instance(D)
    if variant == "transposed_gamma" and lpr > 1 and nv > 1:
        vec = torch.arange(D // 8, device=zb.device)                           # vector v * LPR + j reads vector j * NV + v
        src = ((vec % lpr) * nv + vec // lpr) % (D // 8)
        col = (src[:, None] * 8 + torch.arange(8, device=zb.device)).flatten()
        ga, be = ga[col], be[col]
    return ga * ((zb - mean) * rstd) + be, mean.squeeze(-1), rstd.squeeze(-1)


def backward64(dX, z, mean, rstd, gamma, variant=None):
    """fp64 LayerNorm backward of dX, z [M, D] with the fp32 mean / rstd the kernel is given
    -> dz, the rows of the dgamma sum (dX xhat), the rows of the dbeta sum (dX), rowmax|dX gamma|."""
    dX, z, mean, rstd, gamma = dX.double(), z.double(), mean.double()[:, None], rstd.double()[:, None], gamma.double()
    D = dX.shape[1]
    g = dX * gamma
    xhat = (z - mean) * rstd
    div = _padded(D) if variant == "padded_div" and instance(D)[2] else D
    c1, c2 = g.sum(-1, keepdim=True) / div, (g * xhat).sum(-1, keepdim=True) / div
    dz = rstd * (g - c1 - xhat * c2)
    return dz, (g if variant == "dgamma_times_gamma" else dX) * xhat, dX, g.abs().amax(-1, keepdim=True)


def owner(rows, M, D):
    """The workgroup (= partial row) that owns each of the rows `rows` of an M-row launch."""
    return (rows // rpb(D)) % partial_rows(M, D)


def partials(per_row_gamma, per_row_beta, M, D, variant=None):
    """The partial rows a backward launch leaves in ws: fp64 [partial_rows(M, D), 2 D], row b = the sums over the rows that
    workgroup b owns."""
    n, b = partial_rows(M, D), rpb(D)
    rows = torch.arange(M, device=per_row_gamma.device)
    vals = torch.cat([per_row_gamma.double(), per_row_beta.double()], 1)
    stripes = -(-(-(-M // b)) // n)
    if variant == "last_stripe_missing" and stripes > 1:
        vals = vals * (rows // (b * n) < stripes - 1).double()[:, None]
    return torch.zeros(n, 2 * D, dtype=torch.float64, device=vals.device).index_add_(0, owner(rows, M, D), vals)


def reduced(part, before, accumulate, variant=None):
    """dgamma | dbeta [2 D] after the reduce over `before` [2 D]."""
    t = part.sum(0)
    return t + before.double() if accumulate and variant != "accumulate_ignored" else t
