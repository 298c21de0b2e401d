"""fp64 references, restated launch rules and the checks of the attention kernels (csrc/attention.hip), importable on the
CPU.  Nothing here comes from the code under test: the mathematics is scale_dot_product_attention.py:23-39 of the
reference layer (softmax(q k^T / sqrt(dh) [masked_fill -10000]) v) and its closed-form backward, the launch rules are
copied by hand from the host code with the names they have there, and the checks compare tensors only.

Layout everywhere: qkv is the packed projection output [Bf * S, 3 D] (q | k | v, head h at columns h * dh), out / dout
are [Bf * S, D]; the references work on [Bf, H, S, dh] blocks ("parts") and `parts_of` / `heads_of` convert.

Two references
  attn_fp64      the exact mathematics in fp64.
  attn_rounded   the same in fp64 with a round-to-nearest-even to bf16 wherever the kernels' MFMA operands and stored
                 results pass through bf16 (csrc/attention.hip; pack_b and rebuild_p_ds are csrc/attn_common.h's):
                   forward   p = exp2(s c - rowmax), rounded by pack_b before V^T P^T (both forward kernels); the row sum
                             l adds the UNROUNDED p (`rs += pv`); out = bf16(o / l) (`o * inv`)
                   backward  P = exp2(s c - lse2), rounded by pack_b before dO^T P (phase A of the three backward kernels);
                             dS = P (dP - delta) scale uses the unrounded P and is rounded before Q^T dS and K^T dS
                             (phases A and B); delta = sum_d dO * out from the bf16
                             out (the `dl +=` loops); dQ, dK, dV stored as bf16 (the bf16x4 stores that end each phase)
                 The kernel's p is taken against the RUNNING maximum and rescaled by alpha in fp32; the model uses the row
                 maximum, which rounds the same number of values by the same relative step.  Rounding goes fp64 -> fp32 ->
                 bf16, as the kernels' values are fp32 when they are packed.
  Its distance from attn_fp64 is the error budget of the GPU tests.  Documented size (asserted in the CPU tests): with
  mag = the same sums over absolute values (AttnRef.mag), |rounded - fp64| <= 2^-7 mag for out and dV (one operand
  rounding, one result rounding, each at most 2^-8 relative) and <= 2^-6 mag for dQ and dK (delta from the rounded out
  adds 2^-7).

fp32 floor.  Beyond the bf16 roundings the kernels add fp32 accumulation order and v_exp_f32 / v_log_f32, about 2^-22
per value.  That is three orders below a bf16 step and is ignored by the budget -- but where the budget is exactly zero
(S = 1: P = 1, dS = dP - delta = 0 in exact arithmetic, while the kernel subtracts two fp32 sums taken in different
orders) a correct kernel is not: every bound therefore adds FLOOR = 2^-20 mag (four values at 2^-22), elementwise.
"""
import math
from collections import namedtuple

import torch

# ------------------------------------------------------------------------------------------------
# launch rules of csrc/attention.hip, restated (names of that file)
# ------------------------------------------------------------------------------------------------
FRAME_LDS_MAX = 112 * 1024        # ATT_FRAME_LDS_MAX
FRAME_MAX_S = 128                 # use_frame
FWD_BUDGET = 72 * 1024            # ATT_LDS_FWD_BUDGET
BWD_BUDGET = 76 * 1024            # ATT_LDS_BWD_BUDGET
MAX_S = 4096                      # ATT_MAX_S
ONCE_MAX_SPAD = 224               # ONCE_MAX_SPAD
WAVES = 8                         # ATT_WAVES = ATT_THREADS / 64


def spad_of(S):
    return (S + 31) // 32 * 32


def lds_ld(dh):
    """AttCfg<DH>::LD (csrc/attn_common.h): LDS row stride in elements."""
    return 16 if dh == 16 else dh + 16


def frame_fwd_lds(S, H, dh):
    """frame_fwd_lds: one [spad][3 D + 16] bf16 image."""
    return spad_of(S) * (3 * H * dh + 16) * 2


def frame_bwd_lds(S, H, dh):
    """frame_bwd_lds: the qkv image, a [spad][D + 16] dO image and lse / delta [H][spad] fp32 each."""
    sp = spad_of(S)
    return sp * (3 * H * dh + 16) * 2 + sp * (H * dh + 16) * 2 + 2 * H * sp * 4


def use_frame(S, lds):
    """use_frame."""
    return lds <= FRAME_LDS_MAX and S <= FRAME_MAX_S


def use_once(S, dh, masked):
    """use_once (and iq_attn_bwd_masked: only where the per-frame kernel does not claim the shape)."""
    return (not masked) and dh == 64 and spad_of(S) <= ONCE_MAX_SPAD


def kchunk(S, dh):
    """fwd_chunk_rows: key rows staged at a time."""
    return min(FWD_BUDGET // (2 * lds_ld(dh) * 2) // 32 * 32, spad_of(S))


def bwd_chunk_rows(S, dh):
    """bwd_chunk_rows: staged rows of the two-phase backward; lse / delta take 8 B per padded row out of the budget."""
    room = BWD_BUDGET - 2 * spad_of(S) * 4
    return min(room // (2 * lds_ld(dh) * 2) // 32 * 32, spad_of(S))


def expected_kernels(S, H, dh, masked):
    """-> (forward kernel, backward kernel, forward stages, backward chunks): iq_attn_fwd_masked and
    iq_attn_bwd_masked."""
    tf = "true" if masked else "false"
    if not masked and use_frame(S, frame_fwd_lds(S, H, dh)):
        fwd, stages = f"attn_frame_fwd_kernel<{dh}>", 1
    else:
        kc = kchunk(S, dh)
        fwd, stages = f"attn_fwd_kernel<{dh}, {tf}>", (S + kc - 1) // kc                # nstage
    if not masked and use_frame(S, frame_bwd_lds(S, H, dh)):
        bwd, chunks = f"attn_frame_bwd_kernel<{dh}>", 1
    elif use_once(S, dh, masked):
        bwd, chunks = "attn_bwd_once_kernel<1024>", 1
    else:
        ch = bwd_chunk_rows(S, dh)
        bwd, chunks = f"attn_bwd_kernel<{dh}, {tf}>", (spad_of(S) + ch - 1) // ch       # nchunk
    return fwd, bwd, stages, chunks


def heads_defeating_frame_fwd(S, dh):
    """Smallest H at which neither per-frame kernel takes (S, H, dh): the (frame, head) kernels run."""
    H = 1
    while use_frame(S, frame_fwd_lds(S, H, dh)):
        H += 1
    return H


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
AttnRef = namedtuple("AttnRef", "out lse dq dk dv mag")      # [Bf, H, S, dh] fp64 (lse [Bf, H, S]); mag: dict of the same
PARTS = ("out", "dq", "dk", "dv")


def bf16r(x):
    """Round-to-nearest-even to bf16 (through fp32, as the kernels' values are), back in fp64."""
    return x.float().bfloat16().double()


def heads_of(x, Bf, S, H, dh):
    """[Bf * S, H * dh] -> [Bf, H, S, dh] fp64."""
    return x.double().reshape(Bf, S, H, dh).transpose(1, 2)


def parts_of(qkv, Bf, S, H, dh):
    """[Bf * S, 3 D] -> three [Bf, H, S, dh] fp64."""
    return [t.reshape(Bf, S, H, dh).transpose(1, 2) for t in qkv.double().reshape(Bf, S, 3, H * dh).unbind(2)]


def scores(q, k, mask, dh):
    s = (q @ k.transpose(2, 3)) / math.sqrt(dh)
    if mask is not None:
        s = s.masked_fill(~mask.bool(), -10000.0)         # scale_dot_product_attention.py:30-31, after the scaling
    return s


def _attn(qkv, dout, mask, Bf, S, H, dh, rnd):
    q, k, v = parts_of(qkv, Bf, S, H, dh)
    do = heads_of(dout, Bf, S, H, dh)
    scale = 1.0 / math.sqrt(dh)
    s = scores(q, k, mask, dh)
    m = s.max(-1, keepdim=True).values
    p = (s - m).exp()
    l = p.sum(-1, keepdim=True)
    lse = (m + l.log()).squeeze(-1)
    out = rnd(rnd(p) @ v / l) if rnd else (p / l) @ v
    P = (s - lse.unsqueeze(-1)).exp()
    dP = do @ v.transpose(2, 3)
    delta = (do * out).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    if mask is not None:
        dS = dS.masked_fill(~mask.bool(), 0.0)            # masked_fill passes no gradient
    if rnd:
        Pb, dSb = rnd(P), rnd(dS)
        dv, dk, dq = rnd(Pb.transpose(2, 3) @ do), rnd(dSb.transpose(2, 3) @ q), rnd(dSb @ k)
    else:
        dv, dk, dq = P.transpose(2, 3) @ do, dS.transpose(2, 3) @ q, dS @ k
    # the same sums over absolute values: the size of what each result is made of
    mo = P @ v.abs()
    mdS = P * (do.abs() @ v.abs().transpose(2, 3) + (do.abs() * mo).sum(-1, keepdim=True)) * scale
    if mask is not None:
        mdS = mdS.masked_fill(~mask.bool(), 0.0)
    mag = {"out": mo, "dv": P.transpose(2, 3) @ do.abs(), "dk": mdS.transpose(2, 3) @ q.abs(), "dq": mdS @ k.abs()}
    return AttnRef(out, lse, dq, dk, dv, mag)


def attn_fp64(qkv, dout, mask, Bf, S, H, dh):
    """Closed-form forward and backward in fp64 (no autograd).  mask: bool / uint8 [Bf, 1 | H, S, S], 0 = masked, or None."""
    return _attn(qkv, dout, mask, Bf, S, H, dh, None)


def attn_rounded(qkv, dout, mask, Bf, S, H, dh):
    """attn_fp64 with bf16 roundings where the kernels' operands and results pass through bf16 (module docstring)."""
    return _attn(qkv, dout, mask, Bf, S, H, dh, bf16r)


# ------------------------------------------------------------------------------------------------
# checks (tensors in, AssertionError out)
# ------------------------------------------------------------------------------------------------
FLOOR = 2.0 ** -20          # fp32 term, times mag (module docstring)
SPEND = 2.0                 # the kernel may spend twice the modelled bf16 budget
LSE_TOL = 4e-6              # |lse - fp64| <= LSE_TOL (1 + |lse|): fp32 arithmetic on exact bf16 operands


def bf16_step(x):
    """One bf16 step at |x| (0 at 0)."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.where(x == 0, torch.zeros_like(a), torch.exp2(torch.floor(torch.log2(a)) - 7))


def _blk(t):
    return t.pow(2).sum((-1, -2)).sqrt()


def check_part(name, got, f64, rnd, mag, what):
    """One of out / dQ / dK / dV as [Bf, H, S, dh] fp64: per (frame, head) block, L2 and elementwise.  -> largest ratio of the
    kernel's block error to the block's budget (None where no block has a budget well above the fp32 floor)."""
    bad = ~torch.isfinite(got)
    if bad.any():
        b, h, r, c = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what} {name}: {int(bad.sum())} non-finite cells inside the result, first at frame {b} head {h} "
                             f"row {r} col {c}: a read outside an operand (NaN guard rows / columns), or 0 * NaN from padding")
    err, model, floor = got - f64, rnd - f64, FLOOR * mag
    e, bud, fl = _blk(err), _blk(model), _blk(floor)
    over = e > SPEND * bud + fl
    if over.any():
        b, h = (int(i) for i in over.nonzero()[0])
        rows = err[b, h].abs().amax(-1)
        raise AssertionError(f"{what} {name}: frame {b} head {h} block L2 error {e[b, h]:.4g} > {SPEND:g} x budget {bud[b, h]:.4g}"
                             f" + fp32 floor {fl[b, h]:.3g} (relative to the block: {e[b, h] / _blk(f64)[b, h].clamp_min(1e-300):.4g});"
                             f" worst row {int(rows.argmax())} ({int(over.sum())} of {over.numel()} blocks over)")
    lim = SPEND * model.abs().amax((-1, -2), keepdim=True) + bf16_step(f64) + floor
    cell = err.abs() > lim
    if cell.any():
        b, h, r, c = (int(i) for i in cell.nonzero()[0])
        raise AssertionError(f"{what} {name}: {int(cell.sum())} cells over the elementwise bound, first at frame {b} head {h} row {r}"
                             f" col {c}: got {got[b, h, r, c]:.6g}, fp64 {f64[b, h, r, c]:.6g}, bound {lim[b, h, r, c]:.4g}")
    big = bud > 10 * fl
    return float((e[big] / bud[big]).max()) if big.any() else None


def check_lse(got, ref, what):
    """[Bf, H, S] against fp64.  ln(S + 1) - ln(S) > 2.4e-4 for S <= 4096: one key counted or dropped is far outside."""
    got = got.double()
    bad = ~torch.isfinite(got)
    if bad.any():
        b, h, r = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what} lse: non-finite inside the result at frame {b} head {h} row {r}: a read outside an operand")
    over = (got - ref).abs() > LSE_TOL * (1 + ref.abs())
    if over.any():
        b, h, r = (int(i) for i in over.nonzero()[0])
        d = float(got[b, h, r] - ref[b, h, r])
        raise AssertionError(f"{what} lse: {int(over.sum())} rows off, first frame {b} head {h} row {r}: got - fp64 = {d:.4g} "
                             f"(exp = {math.exp(d):.6f} of the row sum: a key counted that should not be, or a live key dropped?)")


def check_all(got_out, got_lse, got_dq, got_dk, got_dv, f64, rnd, what):
    """Everything of one case; -> {part: ratio}."""
    check_lse(got_lse, f64.lse, what)
    ratios = {}
    for name, got in zip(PARTS, (got_out, got_dq, got_dk, got_dv)):
        ratios[name] = check_part(name, got, getattr(f64, name), getattr(rnd, name), f64.mag[name], what)
    return ratios


def check_surroundings(raw, first, rows, pattern, what):
    """raw: the whole integer view of a prefilled buffer whose result is rows [first, first + rows) (all columns).  The pattern
    must stand everywhere outside and nowhere inside."""
    outside = torch.cat([raw[:first].flatten(), raw[first + rows:].flatten()])
    w = (outside != pattern).nonzero()
    if len(w):
        i = int(w[0])
        where = "before" if i < raw[:first].numel() else "after"
        raise AssertionError(f"{what}: {len(w)} cells written outside the result, first {where} it (flat index {i} of the guards)")
    inside = raw[first:first + rows]
    w = (inside == pattern).nonzero()
    if len(w):
        raise AssertionError(f"{what}: {len(w)} cells of the result never written, first at {[int(i) for i in w[0]]}")


# ------------------------------------------------------------------------------------------------
# exact case: uniform attention
# ------------------------------------------------------------------------------------------------
MID_REL = 2.0 ** -20        # a cell this close (relatively) to a bf16 rounding midpoint may sit one step off
MID_SHARE = 0.01            # at most this share of the result


def uniform_inputs(Bf, S, H, dh, zero, seed):
    """CPU-generated (so the CPU test sees the GPU test's data): q = 0 (zero = 'q') or k = 0 (zero = 'k'), the other random,
    v integers from {-2, -1, 1, 2}, dout integers in [-2, 2].  -> qkv [Bf * S, 3 D], dout [Bf * S, D], bf16."""
    D = H * dh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(Bf * S, 3 * D, generator=g)
    v = torch.randint(0, 4, (Bf * S, D), generator=g)
    qkv[:, 2 * D:] = torch.tensor([-2.0, -1.0, 1.0, 2.0])[v]
    lo = 0 if zero == "q" else D
    qkv[:, lo:lo + D] = 0.0
    dout = torch.randint(-2, 3, (Bf * S, D), generator=g).float()
    return qkv.bfloat16(), dout.bfloat16()


def uniform_out_ref(qkv, Bf, S, H, dh):
    """fp64 mean of the S live value rows, [Bf, H, S, dh] (the same row for every query)."""
    v = parts_of(qkv, Bf, S, H, dh)[2]
    return (v.sum(2, keepdim=True) / S).expand(Bf, H, S, dh)


def check_uniform_out(got, mean, what):
    """got [Bf, H, S, dh] (bf16 values as fp64) must be bf16(mean) bit for bit, except cells within MID_REL of a rounding
    midpoint, which may sit one step off; those may be at most MID_SHARE of the result.  -> number of such cells."""
    want = bf16r(mean)
    off = got != want
    if not off.any():
        return 0
    step = bf16_step(mean)
    lo = torch.minimum(got, want)
    near = (mean - (lo + (got - want).abs() / 2)).abs() <= MID_REL * mean.abs()
    one = (got - want).abs() <= step * (1 + 2.0 ** -8)                   # one step (a step doubles at a power of two)
    wrong = off & ~(near & one)
    if wrong.any():
        b, h, r, c = (int(i) for i in wrong.nonzero()[0])
        S = mean.shape[2]
        ratio = float(got[b, h, r, c] / mean[b, h, r, c]) if float(mean[b, h, r, c]) else float("nan")
        raise AssertionError(f"{what}: {int(wrong.sum())} cells differ from bf16(mean of the {S} value rows), first frame {b} head {h} "
                             f"row {r} col {c}: got {float(got[b, h, r, c])!r}, mean {float(mean[b, h, r, c])!r} (got / mean = {ratio:.6f};"
                             f" S / (S + 1) = {S / (S + 1):.6f}, S / (S - 1) = {S / max(S - 1, 1):.6f}: a padding key counted, or a "
                             f"live key dropped, changes the integer sum and the row sum)")
    n = int(off.sum())
    assert n <= MID_SHARE * off.numel(), f"{what}: {n} of {off.numel()} cells one step off at a rounding midpoint, more than 1 %"
    return n


def uniform_out_fp32_way(qkv, Bf, S, H, dh):
    """What fp32 arithmetic gives for the same cell: bf16(fl32(sum v) * fl32(1 / S)), the kernels' o * (1 / l)."""
    v = parts_of(qkv, Bf, S, H, dh)[2]
    s = v.sum(2, keepdim=True).float()
    inv = (torch.ones((), dtype=torch.float32) / torch.tensor(float(S), dtype=torch.float32))
    return (s * inv).bfloat16().double().expand(Bf, H, S, dh)


# (Bf, S, H, dh, seed): every kernel family, S on each side of a 16-key edge and of a stage / chunk edge
UNIFORM = [(2, 16, 2, 16, 1), (2, 17, 2, 16, 1), (2, 32, 2, 32, 1), (2, 33, 2, 32, 1), (2, 64, 1, 64, 1), (2, 65, 1, 64, 1),
           (2, 17, 38, 16, 1), (2, 33, 10, 32, 1),
           (2, 208, 1, 64, 1), (2, 209, 1, 64, 1), (2, 224, 1, 64, 1), (2, 225, 1, 64, 1),
           (1, 384, 1, 32, 1), (1, 385, 1, 32, 1), (1, 1152, 1, 16, 1), (1, 1153, 1, 16, 1)]
