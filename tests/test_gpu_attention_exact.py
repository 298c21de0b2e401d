"""GPU (MI355X): the five attention kernel families of csrc/attention.hip -- attn_fwd_kernel<dh, masked>,
attn_frame_fwd_kernel<dh>, attn_bwd_kernel<dh, masked>, attn_frame_bwd_kernel<dh>, attn_bwd_once_kernel<1024> -- through
iq_attn_fwd[_masked] / iq_attn_bwd[_masked], at every launch route and at the edges of every tile, stage and chunk.

Method.  Every case names the kernels it expects from the launch rules RESTATED in tests/attention_ref.py and asserts
{kernel name: launches} as recorded by the launch sites (prof_names.kernel_launches).  The references are fp64 closed forms
(attention_ref.attn_fp64, checked against autograd on the CPU); nothing is compared with another kernel or with eager torch
in bf16.

Surroundings.  qkv, dout and the forward's out (the backward's input) live in NaN-filled bf16 buffers with GUARD rows before
and after; lse sits between sentinel words, as input and as output.  out, lse and dqkv are prefilled with a NaN payload no
kernel produces and compared WHOLE: the pattern everywhere outside [Bf*S, D], [Bf, H, S], [Bf*S, 3D] and nowhere inside.  A
NaN inside a result is a read outside an operand (or 0 * NaN from a padding row), and the message says so.  The operands
must be unchanged afterwards.

Budget rule.  For each of out, dQ, dK, dV and each (frame, head) block the kernel's error against attn_fp64 may be at most
TWICE the error of attention_ref.attn_rounded (fp64 with bf16 roundings exactly where the kernels' operands pass through
bf16) on the same block and inputs, computed on every run: in L2 over the block, and per cell within twice the block's
largest modelled error plus one bf16 step of the reference value.  Both add the fp32 floor 2^-20 * (the same sums over
absolute values), which matters only where the budget is exactly zero (S = 1); attention_ref's docstring derives it.  lse:
|lse - fp64| <= 4e-6 (1 + |lse|); ln(S + 1) - ln(S) >= 2.4e-4 for S <= 4096, so one key counted or dropped is outside at
every S.  No limit is taken from a kernel's output; the largest kernel-to-budget ratio per family is printed by
test_zz_report (profiles/attention_exact.txt has the measured values).  Two launches into differently prefilled outputs must
be torch.equal.

Exact cases (no accuracy tolerance).  Uniform attention (q = 0 or k = 0, integer v and dout): out is bf16(mean of the S value
rows) bit for bit, but for cells within relative 2^-20 of a rounding midpoint (at most 1 %; the CPU test asserts the seeds
keep the fp32 way of computing the same cell inside that cap), lse = ln S within 4e-6, dK (q = 0) or dQ (k = 0) is +-0
everywhere.  Poisoned neighbours: frame 1 and head 1 filled with NaN, then +Inf: every other (frame, head) block of out,
lse, dqkv keeps its bits.  Batch invariance: frame b of a Bf-frame launch equals a one-frame launch on its rows, also with
600 frames (more workgroups than the chip holds at once).  Refusals leave the prefilled outputs alone and record nothing.

Restated thresholds (attention_ref.py, with their names in csrc/attention.hip):
  per-frame kernels   S <= 128 and LDS <= 112 KiB (use_frame); forward spad (3 D + 16) 2 B (frame_fwd_lds); backward adds
                      spad (D + 16) 2 B + 2 H spad 4 B (frame_bwd_lds)
  once kernel         dh = 64, no mask, spad <= 224, where the per-frame backward does not claim the shape (use_once)
  forward stage       kchunk = 72 KiB / (2 images * LD * 2 B), down to 32 rows: 224 / 384 / 1152 rows at dh 64 / 32 / 16
                      (fwd_chunk_rows); LD = dh + 16, or 16 at dh = 16 (AttCfg)
  backward chunk      (76 KiB - 8 B * spad) / (2 * LD * 2 B), down to 32 rows (bwd_chunk_rows)
  refusals            S > 4096 or dh not in {16, 32, 64}: IQ_ERR_UNSUPPORTED before anything is recorded (iq_attn_supported)
The edge shapes below are derived from these rules at collection time, and both sides of each edge assert their kernel.

Self-checks (tests/test_attention_ref_cpu.py; each applies a hand-made error to reference outputs on the CPU and requires the
failure message to name it):
  test_checks_catch_a_counted_padding_key           one zero key row counted: lse (and out at S = 33) fails; at S = 225 the
                                                    older limits (2e-3, 2^-6) pass it
  test_checks_catch_a_dropped_key                   the last live key dropped in ONE row: lse, out and dQ of that block fail
                                                    while the older 0.02 * max|grad| bound over the packed gradient passes
  test_checks_catch_blocks_swapped_between_heads    out, dQ, dK, dV blocks of two heads exchanged
  test_checks_catch_a_nan_inside_and_a_cell_outside a NaN / Inf inside a result, a cell written before and after it, cells
                                                    never written
  test_uniform_check_catches_one_key_more_or_less   the exact case with l = S + 1, and with one live value row missing
"""
import math

import pytest
import torch

import attention_ref as A
from prof_names import kernel_launches
from test_gpu_kernels import L, _N, dev, stream  # noqa: F401  (L is a fixture)
from test_gpu_wgrad_exact import FENCE, GUARD, NAN, SENT, Fenced

pytestmark = pytest.mark.gpu

IQ_OK, IQ_ERR_ARG, IQ_ERR_UNSUPPORTED = 0, 1, 2
NANBITS = 0x7FC0                       # bf16 NaN of the operand guards
PAT = (0x7FC5, 0x7FA7)                 # bf16 prefill patterns: NaN payloads no kernel produces
LPAT = (SENT, 0x7FC5B6B6)              # the same for fp32 (lse)
RATIOS = {}                            # kernel family -> part -> largest block error / budget seen in this process


class Rows:
    """[rows, cols] bf16 between GUARD rows, the whole buffer filled with `bits`."""

    def __init__(self, rows, cols, bits, values=None):
        self.rows, self.bits = rows, bits
        self.raw = torch.full((GUARD + rows + GUARD, cols), bits, dtype=torch.int16, device=dev())
        self.body = self.raw.view(torch.bfloat16)[GUARD:GUARD + rows]
        if values is not None:
            self.body.copy_(values)

    def ptr(self, row=0):
        return self.body.data_ptr() + row * self.body.shape[1] * 2

    def whole(self, what):
        A.check_surroundings(self.raw, GUARD, self.rows, self.bits, what)

    def untouched(self):
        return bool((self.raw == self.bits).all())


class Lse:
    """Bf * H * S fp32 between sentinel words, prefilled with pattern i."""

    def __init__(self, n, i):
        self.f, self.n, self.bits = Fenced(n), n, LPAT[i]
        self.f.raw.fill_(self.bits)
        self.body = self.f.body

    def ptr(self, off=0):
        return self.f.ptr() + 4 * off

    def whole(self, what):
        A.check_surroundings(self.f.raw.view(-1, 1), FENCE, self.n, self.bits, what)

    def untouched(self):
        return bool((self.f.raw == self.bits).all())


class Case:
    """Operands of one problem in fenced buffers, and its launches.  mask: bool [Bf, 1 | H, S, S] or None."""

    def __init__(self, L, Bf, S, H, dh, qkv, dout, mask=None, per_head=False):
        self.L, self.Bf, self.S, self.H, self.dh, self.D = L, Bf, S, H, dh, H * dh
        self.qkv0, self.dout0 = qkv.to(dev()), dout.to(dev())
        self.qkv = Rows(Bf * S, 3 * self.D, NANBITS, self.qkv0)
        self.dout = Rows(Bf * S, self.D, NANBITS, self.dout0)
        self.mask = mask
        self.mk = None if mask is None else mask.to(torch.uint8).contiguous()
        self.hs = S * S if per_head else 0
        assert mask is None or mask.shape == (Bf, H if per_head else 1, S, S)
        self.names = A.expected_kernels(S, H, dh, mask is not None)
        self.what = f"Bf={Bf} S={S} H={H} dh={dh}" + ("" if mask is None else f" mask_hstride={self.hs}")

    def _mkptr(self, b=0):
        return self.mk.data_ptr() + b * self.mk.shape[1] * self.S * self.S

    def _fwd(self, out, lse, b0, nb):
        S, H, D = self.S, self.H, self.D
        a = (self.qkv.ptr(b0 * S), out.ptr(b0 * S), lse.ptr(b0 * H * S))
        if self.mk is None:
            return self.L.iq_attn_fwd(*a, nb, S, H, self.dh, stream())
        return self.L.iq_attn_fwd_masked(*a, self._mkptr(b0), self.hs, nb, S, H, self.dh, stream())

    def _bwd(self, out, lse, dqkv, b0, nb):
        S, H, D = self.S, self.H, self.D
        a = (self.qkv.ptr(b0 * S), out.ptr(b0 * S), self.dout.ptr(b0 * S), lse.ptr(b0 * H * S), dqkv.ptr(b0 * S))
        if self.mk is None:
            return self.L.iq_attn_bwd(*a, nb, S, H, self.dh, stream())
        return self.L.iq_attn_bwd_masked(*a, self._mkptr(b0), self.hs, nb, S, H, self.dh, stream())

    def fwd(self, i=0, frames=False):
        """-> out, lse after one launch of all frames (or one launch per frame) into outputs prefilled with pattern i; the
        return codes, the kernels recorded and the surroundings are asserted."""
        out, lse = Rows(self.Bf * self.S, self.D, PAT[i]), Lse(self.Bf * self.H * self.S, i)
        launches = [(b, 1) for b in range(self.Bf)] if frames else [(0, self.Bf)]
        rc = []
        rec = kernel_launches(self.L, lambda: rc.extend(self._fwd(out, lse, b0, nb) for b0, nb in launches))
        assert rc == [IQ_OK] * len(launches), f"{self.what}: forward rc {rc}"
        assert rec == {self.names[0]: len(launches)}, f"{self.what}: forward launched {rec}, expected {self.names[0]}"
        out.whole(f"{self.what} out ({self.names[0]})")
        lse.whole(f"{self.what} lse ({self.names[0]})")
        self.operands_unchanged()
        return out, lse

    def bwd(self, out, lse, i=0, frames=False):
        dqkv = Rows(self.Bf * self.S, 3 * self.D, PAT[i])
        launches = [(b, 1) for b in range(self.Bf)] if frames else [(0, self.Bf)]
        keep_out, keep_lse = out.raw.clone(), lse.f.raw.clone()
        rc = []
        rec = kernel_launches(self.L, lambda: rc.extend(self._bwd(out, lse, dqkv, b0, nb) for b0, nb in launches))
        assert rc == [IQ_OK] * len(launches), f"{self.what}: backward rc {rc}"
        assert rec == {self.names[1]: len(launches)}, f"{self.what}: backward launched {rec}, expected {self.names[1]}"
        dqkv.whole(f"{self.what} dqkv ({self.names[1]})")
        assert torch.equal(out.raw, keep_out) and torch.equal(lse.f.raw, keep_lse), f"{self.what}: the backward wrote its inputs"
        self.operands_unchanged()
        return dqkv

    def operands_unchanged(self):
        for r, v, name in ((self.qkv, self.qkv0, "qkv"), (self.dout, self.dout0, "dout")):
            assert torch.equal(r.body.view(torch.int16), v.view(torch.int16)), f"{self.what}: {name} was written"
            assert bool((r.raw[:GUARD] == NANBITS).all() and (r.raw[GUARD + r.rows:] == NANBITS).all()), f"{self.what}: {name} guards"

    def parts(self, out, lse, dqkv):
        g = (self.Bf, self.S, self.H, self.dh)
        return (A.heads_of(out.body, *g), lse.body.view(self.Bf, self.H, self.S), *A.parts_of(dqkv.body, *g))


def random_case(L, Bf, S, H, dh, mask_kind=None, seed=0):
    g = torch.Generator(device="cuda").manual_seed(7919 * S + 31 * H + dh + seed)
    D = H * dh
    qkv = torch.randn(Bf * S, 3 * D, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(Bf * S, D, device=dev(), generator=g).to(torch.bfloat16)
    mask = None
    if mask_kind:
        mask = torch.rand(Bf, H if mask_kind == "per_head" else 1, S, S, device=dev(), generator=g) > 0.3
        if S > 1:
            mask[:, :, S // 2, :] = False                       # a fully masked row
            mask[:, :, 0, :] = False                            # a row whose only unmasked key is the last live key
            mask[:, :, 0, S - 1] = True
    return Case(L, Bf, S, H, dh, qkv, dout, mask, mask_kind == "per_head")


def run(L, Bf, S, H, dh, mask_kind=None):
    """Everything section 3 of the method asks of one case."""
    c = random_case(L, Bf, S, H, dh, mask_kind)
    out, lse = c.fwd(0)
    dqkv = c.bwd(out, lse, 0)
    out2, lse2 = c.fwd(1)
    dqkv2 = c.bwd(out2, lse2, 1)
    for a, b, name in ((out.body, out2.body, "out"), (lse.body, lse2.body, "lse"), (dqkv.body, dqkv2.body, "dqkv")):
        assert torch.equal(a, b) and not a.isnan().any(), f"{c.what}: {name} differs between two launches (or holds a NaN)"
    g = (c.qkv0, c.dout0, c.mask, Bf, S, H, dh)
    f64, rnd = A.attn_fp64(*g), A.attn_rounded(*g)
    ratios = A.check_all(*c.parts(out, lse, dqkv), f64, rnd, f"{c.what} ({c.names[0]}, {c.names[1]})")
    for part, r in ratios.items():
        fam = c.names[0 if part == "out" else 1].split("<")[0]
        if r is not None:
            RATIOS.setdefault(fam, {})[part] = max(r, RATIOS.get(fam, {}).get(part, 0.0))
    print(f"{c.what}: {c.names}, error / budget " + ", ".join(f"{p} {r:.2f}" for p, r in ratios.items() if r is not None))
    return c


# ------------------------------------------------------------------------------------------------
# 2. routes and edges, derived from the restated rules
# ------------------------------------------------------------------------------------------------
def last_fitting_h(lds, S, dh):
    H = 1
    while A.use_frame(S, lds(S, H + 1, dh)):
        H += 1
    return H


def first_s(pred, lo=1):
    return next(S for S in range(lo, A.MAX_S + 1) if pred(S))


FWD_FIT = [(S, dh, last_fitting_h(A.frame_fwd_lds, S, dh)) for S, dh in ((128, 16), (65, 16), (128, 32), (128, 64))]
BWD_FIT = [(S, dh, last_fitting_h(A.frame_bwd_lds, S, dh)) for S, dh in ((65, 16), (128, 16), (128, 32), (128, 64))]


@pytest.mark.parametrize("S,dh,H", FWD_FIT)
def test_frame_forward_fit_edge(L, S, dh, H):
    """H heads fit the forward's 112 KiB image, H + 1 do not (S = 128, dh = 16, H = 9 is exactly 112 KiB)."""
    assert A.frame_fwd_lds(S, H, dh) <= A.FRAME_LDS_MAX < A.frame_fwd_lds(S, H + 1, dh)
    assert run(L, 2, S, H, dh).names[0] == f"attn_frame_fwd_kernel<{dh}>"
    assert run(L, 2, S, H + 1, dh).names[0] == f"attn_fwd_kernel<{dh}, false>"


@pytest.mark.parametrize("S,dh,H", BWD_FIT)
def test_frame_backward_fit_edge(L, S, dh, H):
    """The backward's images end earlier than the forward's: on the far side the forward still runs per frame."""
    a, b = run(L, 2, S, H, dh), run(L, 2, S, H + 1, dh)
    assert a.names[:2] == (f"attn_frame_fwd_kernel<{dh}>", f"attn_frame_bwd_kernel<{dh}>")
    assert b.names[0] == f"attn_frame_fwd_kernel<{dh}>" and "frame" not in b.names[1]
    if (S, dh) == (65, 16):
        assert H == 8            # the benchmarked cfg C shape sits on the fitting side of this edge


@pytest.mark.parametrize("dh", [16, 32, 64])
def test_frame_kernels_end_at_128_rows(L, dh):
    c = run(L, 2, A.FRAME_MAX_S, 1, dh)
    assert "frame" in c.names[0] and "frame" in c.names[1]
    c = run(L, 2, A.FRAME_MAX_S + 1, 1, dh)
    assert "frame" not in c.names[0] and "frame" not in c.names[1]


def test_once_kernel_edge(L):
    S = first_s(lambda S: not A.use_once(S, 64, False)) - 1            # 224
    assert run(L, 2, S, 1, 64).names[1:] == ("attn_bwd_once_kernel<1024>", 1, 1)
    c = run(L, 2, S + 1, 1, 64)
    assert c.names[1:] == ("attn_bwd_kernel<64, false>", 2, 2)
    assert S + 1 - A.bwd_chunk_rows(S + 1, 64) == 1                    # the last chunk holds one live key


@pytest.mark.parametrize("dh", [64, 32, 16])
def test_forward_stage_edge(L, dh):
    S = A.kchunk(A.MAX_S, dh)                                          # 224 / 384 / 1152
    Bf = 2 if dh == 64 else 1
    assert run(L, Bf, S, 1, dh).names[2] == 1
    assert run(L, Bf, S + 1, 1, dh).names[2] == 2


def chunk_edges():
    """(S, dh, chunks): both sides of the first chunk edge of attn_bwd_kernel at dh = 32 and 16, the next 32-row edge after
    it at dh = 32, and the first three-chunk length at dh = 64."""
    def chunks(dh):
        return lambda S: A.expected_kernels(S, 1, dh, False)[3]
    s32 = first_s(lambda S: chunks(32)(S) == 2, 129)                   # 385
    s16 = first_s(lambda S: chunks(16)(S) == 2, 129)                   # 1057
    s64 = first_s(lambda S: chunks(64)(S) == 3, 225)                   # 449
    n32 = A.spad_of(s32)                                               # 416
    return [(s32 - 1, 32, 1), (s32, 32, 2), (n32, 32, 2), (n32 + 1, 32, 2), (s16 - 1, 16, 1), (s16, 16, 2), (s64, 64, 3)]


@pytest.mark.parametrize("S,dh,chunks", chunk_edges())
def test_backward_chunk_edge(L, S, dh, chunks):
    c = run(L, 1 if S > 512 else 2, S, 1, dh)
    assert c.names[1] == f"attn_bwd_kernel<{dh}, false>" and c.names[3] == chunks


UNIT_S = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97)


@pytest.mark.parametrize("dh", [16, 32, 64])
@pytest.mark.parametrize("S", UNIT_S)
def test_unit_edges_frame_kernels(L, S, dh):
    """Two heads reach the per-frame kernels at dh = 16 and 32 (at dh = 64 two heads of 128 padded rows no longer fit: one)."""
    assert run(L, 2, S, 2 if dh < 64 else 1, dh).names[:2] == (f"attn_frame_fwd_kernel<{dh}>", f"attn_frame_bwd_kernel<{dh}>")


@pytest.mark.parametrize("dh", [16, 32, 64])
@pytest.mark.parametrize("S", UNIT_S)
def test_unit_edges_frame_head_kernels(L, S, dh):
    """The same lengths with enough heads to defeat the LDS fit: one workgroup per (frame, head); at dh = 64 the backward is
    the once kernel."""
    H = A.heads_defeating_frame_fwd(S, dh)
    bwd = f"attn_bwd_kernel<{dh}, false>" if dh < 64 else "attn_bwd_once_kernel<1024>"
    assert run(L, 2, S, H, dh).names[:2] == (f"attn_fwd_kernel<{dh}, false>", bwd)


@pytest.mark.parametrize("S,H", [(33, 1), (33, 3), (33, 5), (33, 7), (33, 8), (33, 9), (33, 17), (17, 17)])
def test_frame_kernels_heads_and_waves(L, S, H):
    """Fewer heads than waves (a workgroup of 64 H threads), more heads than waves (a wave runs heads w, w + 8, w + 16)."""
    c = run(L, 2, S, H, 16)
    assert c.names[0] == "attn_frame_fwd_kernel<16>"
    if (S, H) != (33, 17):                                             # 17 heads of 64 padded rows: the backward's images do not fit
        assert c.names[1] == "attn_frame_bwd_kernel<16>"


MASKED = ([(2, S, 2, 16) for S in UNIT_S] +                             # every unit edge at dh = 16
          [(2, 17, 2, 32), (2, 33, 2, 32), (2, 17, 2, 64), (2, 65, 2, 64),
           (2, 225, 2, 64), (1, 385, 2, 32), (1, 1057, 1, 16)])          # chunk edges at each dh


@pytest.mark.parametrize("kind", ["shared", "per_head"])
@pytest.mark.parametrize("Bf,S,H,dh", MASKED)
def test_masked_kernels(L, Bf, S, H, dh, kind):
    c = run(L, Bf, S, H, dh, kind)
    assert c.names[:2] == (f"attn_fwd_kernel<{dh}, true>", f"attn_bwd_kernel<{dh}, true>")
    assert c.hs == (S * S if kind == "per_head" else 0)


# ------------------------------------------------------------------------------------------------
# 4. exact cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("Bf,S,H,dh,seed", A.UNIFORM)
def test_uniform_attention_is_exact(L, Bf, S, H, dh, seed, zero):
    qkv, dout = A.uniform_inputs(Bf, S, H, dh, zero, seed)
    c = Case(L, Bf, S, H, dh, qkv, dout)
    what = f"{c.what} {zero} = 0 {c.names}"
    out, lse = c.fwd()
    got = A.heads_of(out.body, Bf, S, H, dh)
    assert torch.isfinite(got).all(), f"{what}: NaN inside out: a read outside an operand"
    n = A.check_uniform_out(got, A.uniform_out_ref(c.qkv0, Bf, S, H, dh), what)
    d = (lse.body.double() - math.log(S)).abs().max().item()
    assert d <= 4e-6, f"{what}: lse off ln S by {d:.3g} (ln(S + 1) - ln S = {math.log1p(1 / S):.3g}: a key counted or dropped?)"
    dqkv = c.bwd(out, lse)
    dq, dk, dv = A.parts_of(dqkv.body, Bf, S, H, dh)
    z, name = (dk, "dK") if zero == "q" else (dq, "dQ")
    assert bool((z == 0).all()), f"{what}: {name} must be +-0 everywhere; {int((z != 0).sum())} cells are not (first {z[z != 0][:1].tolist()})"
    assert torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all(), what
    print(f"{what}: exact, {n} midpoint cells of {got.numel()}")


# every family, the last 32-row block holding padding rows; (S, H, dh, mask)
POISON = [(33, 2, 16, None), (65, 2, 32, None), (97, 2, 16, None), (97, 2, 64, None), (33, 3, 64, None), (65, 13, 16, None),
          (97, 7, 32, None), (197, 2, 64, None), (225, 2, 64, None), (197, 2, 32, None), (225, 2, 16, None),
          (65, 2, 16, "shared"), (225, 2, 64, "per_head")]


@pytest.mark.parametrize("S,H,dh,kind", POISON)
def test_poisoned_neighbours(L, S, H, dh, kind):
    """0 * NaN: a padding key's P = 0, a padding row's zero fill, a neighbouring head's columns in a shared image -- none may
    multiply a neighbour's data into a frame that is fine."""
    Bf, D = 3, H * dh
    clean = random_case(L, Bf, S, H, dh, kind)
    out0, lse0 = clean.fwd()
    dqkv0 = clean.bwd(out0, lse0)
    keep = torch.ones(Bf, H, dtype=torch.bool, device=dev())
    keep[1, :] = False
    keep[:, 1] = False
    base = [t[keep].view(torch.int16) if t.dtype == torch.bfloat16 else t[keep].view(torch.int32)
            for t in blocks(clean, out0, lse0, dqkv0)]
    for poison in (NAN, float("inf")):
        qkv = clean.qkv0.clone().view(Bf, S, 3, H, dh)
        dout = clean.dout0.clone().view(Bf, S, H, dh)
        qkv[1], dout[1] = poison, poison
        qkv[:, :, :, 1], dout[:, :, 1] = poison, poison
        c = Case(L, Bf, S, H, dh, qkv.view(Bf * S, 3 * D), dout.view(Bf * S, D), clean.mask, kind == "per_head")
        out, lse = c.fwd()
        dqkv = c.bwd(out, lse)
        for name, a, t in zip(("out", "lse", "dQ", "dK", "dV"), base, blocks(c, out, lse, dqkv)):
            b = t[keep]
            assert torch.isfinite(b.float()).all(), (f"{c.what} {c.names}: {name} of an untouched (frame, head) block is not finite "
                                                     f"with {poison} in frame 1 and head 1: a neighbour's data was multiplied in")
            b = b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)
            assert torch.equal(a, b), f"{c.what} {c.names}: {name} of an untouched block changed with {poison} in frame 1 and head 1"


def blocks(c, out, lse, dqkv):
    """out, lse, dQ, dK, dV as [Bf, H, ...] in their stored types."""
    Bf, S, H, dh = c.Bf, c.S, c.H, c.dh
    o = out.body.view(Bf, S, H, dh).transpose(1, 2)
    q, k, v = (t.transpose(1, 2) for t in dqkv.body.view(Bf, S, 3, H, dh).unbind(2))
    return o, lse.body.view(Bf, H, S), q, k, v


BATCH = [(3, 33, 8, 16, None), (3, 65, 13, 16, None), (3, 97, 2, 32, None), (3, 197, 2, 64, None), (3, 225, 1, 64, None),
         (3, 385, 1, 32, None), (3, 33, 2, 32, "per_head"), (3, 65, 2, 64, "shared"),
         (600, 33, 8, 16, None)]       # 600 workgroups of 512 threads: more than the chip holds at once


@pytest.mark.parametrize("Bf,S,H,dh,kind", BATCH)
def test_batch_invariance(L, Bf, S, H, dh, kind):
    """Frame b of one launch equals a one-frame launch on that frame's rows alone, for every frame, by the same kernel (Case.fwd
    and Case.bwd assert {kernel: Bf launches} for the per-frame run)."""
    c = random_case(L, Bf, S, H, dh, kind)
    out, lse = c.fwd(0)
    dqkv = c.bwd(out, lse, 0)
    out1, lse1 = c.fwd(1, frames=True)
    dqkv1 = c.bwd(out1, lse1, 1, frames=True)
    for a, b, name in ((out, out1, "out"), (lse, lse1, "lse"), (dqkv, dqkv1, "dqkv")):
        if not torch.equal(a.body, b.body):
            rows = (a.body.reshape(Bf, -1) != b.body.reshape(Bf, -1)).any(1).nonzero().flatten().tolist()
            raise AssertionError(f"{c.what} {c.names}: {name} of frames {rows[:8]} depends on the batch it was launched in")
        assert not a.body.isnan().any()


def test_refusals_touch_nothing_and_record_nothing(L):
    S0, D0 = A.MAX_S + 1, 64
    qkv = Rows(S0, 3 * D0, NANBITS, torch.ones(S0, 3 * D0))
    dout = Rows(S0, D0, NANBITS, torch.ones(S0, D0))
    oin = Rows(S0, D0, NANBITS, torch.ones(S0, D0))
    lin = Lse(S0, 0)
    lin.body.fill_(1.0)
    mk = torch.ones(64 * 64, dtype=torch.uint8, device=dev())
    out, lse, dqkv = Rows(S0, D0, PAT[0]), Lse(S0, 0), Rows(S0, 3 * D0, PAT[0])
    F, B = L.iq_attn_fwd_masked, L.iq_attn_bwd_masked
    f = dict(qkv=qkv.ptr(), out=out.ptr(), lse=lse.ptr(), mask=None, hs=0, B=1, S=64, H=1, dh=64)
    b = dict(qkv=qkv.ptr(), out=oin.ptr(), dout=dout.ptr(), lse=lin.ptr(), dqkv=dqkv.ptr(), mask=None, hs=0, B=1, S=64, H=1, dh=64)
    cases = [("dh = 48", dict(dh=48), IQ_ERR_UNSUPPORTED), ("S = 4097", dict(S=S0), IQ_ERR_UNSUPPORTED),
             ("dh = 48, masked", dict(dh=48, mask=mk.data_ptr()), IQ_ERR_UNSUPPORTED),
             ("mask_hstride = 5", dict(mask=mk.data_ptr(), hs=5), IQ_ERR_ARG),
             ("mask_hstride = S", dict(mask=mk.data_ptr(), hs=64), IQ_ERR_ARG),
             ("qkv = null", dict(qkv=None), IQ_ERR_ARG), ("B = 0", dict(B=0), IQ_OK), ("B = 0, dh = 48", dict(B=0, dh=48), IQ_OK)]
    cases_f = cases + [("out = null", dict(out=None), IQ_ERR_ARG), ("lse = null", dict(lse=None), IQ_ERR_ARG)]
    cases_b = cases + [(f"{k} = null", {k: None}, IQ_ERR_ARG) for k in ("out", "dout", "lse", "dqkv")]
    for fn, base, cs in ((F, f, cases_f), (B, b, cases_b)):
        for name, change, want in cs:
            a = dict(base, **change)
            rc = []
            rec = kernel_launches(L, lambda: rc.append(fn(*a.values(), stream())))
            where = f"{'forward' if fn is F else 'backward'}, {name}"
            assert rc == [want], f"{where}: rc {rc[0]}, expected {want}"
            assert rec == {}, f"{where}: a refused call recorded {rec}"
            assert out.untouched() and lse.untouched() and dqkv.untouched(), f"{where}: a refused call wrote an output"
    assert oin.body.eq(1).all() and lin.body.eq(1).all() and qkv.body.eq(1).all() and dout.body.eq(1).all()
    assert L.iq_attn_fwd(qkv.ptr(), out.ptr(), lse.ptr(), 1, S0, 1, 64, stream()) == IQ_ERR_UNSUPPORTED
    assert L.iq_attn_bwd(qkv.ptr(), oin.ptr(), dout.ptr(), lin.ptr(), dqkv.ptr(), 1, 64, 1, 48, stream()) == IQ_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and lse.untouched() and dqkv.untouched()


def test_zz_report():
    """Not a check of its own: prints the largest block error / budget per kernel family seen by the cases above (the limit
    they assert is 2)."""
    for fam in sorted(RATIOS):
        print(f"{fam}: " + ", ".join(f"{p} {r:.3f}" for p, r in sorted(RATIOS[fam].items())))
    assert all(r <= A.SPEND for parts in RATIOS.values() for r in parts.values())
