"""GPU (MI355X): the two one-launch chain kernels (csrc/ffn_chain.hip) bit for bit, at every workgroup shape, chunk count and
row edge, through all five entry points of the C ABI: iq_ffn_chain_fwd, iq_attn_out_ffn_chain_fwd without and with the q,k,v
stage, iq_ffn_chain_bwd without and with Wot / dA, iq_qkv_dgrad_ffn_chain_bwd -- each with dropout on and off.

Method.  tests/chain_exact_ref.py states in fp64 what each entry point stores, on integer operands: every fp32 value before a
store is exact in ANY summation order (the kernels permute the k-slots of an MFMA step), and the stored value is that number
rounded once to bf16, to nearest even.  H, Z, Z1, gH, the Yq of a gamma2 = 0 launch and the dbeta halves of partial /
partial2 are compared with torch.equal on int16 / fp32 views; tests/test_chain_exact_ref_cpu.py confirms the amplitude
conditions for these very operands and that every wrong kernel of chain_exact_ref.VARIANTS would be told apart.
The real quantities carry the bounds tests/test_gpu_gemm_exact.py applies to the same quantities on exact inputs:
X / X1 within 2^-8 |ref| + 2^-16 max|ref| of fp64 taken from the exact Z, dz / dy within 2^-8 |ref| + 2^-16 rowmax|dX gamma|
rstd, mean / rstd 1e-5 and dgamma partial rows 1e-3 of the scale, a dropped dy element +0.  Two products have real inputs and
no exact statement: dA = dy Wot^T and the Yq of a real X.  They are held to `product_bound` (derived there) against fp64 of
the operand the launch itself wrote.
What a fused launch (MODE 1 / 2) writes behind its first stage equals, bit for bit, the stand-alone entry point run on the
X1 (dy2 / dz2) the fused launch wrote.

Surroundings.  Every bf16 operand sits between GUARD rows of NaN, every bf16 output is an `Out` prefilled with PAT and compared
WHOLE, every fp32 vector and output lies between sentinel words, partial / partial2 are sized exactly
iq_ffn_chain_bwd_partial_rows(M) * 2 D and prefilled with NaN (the kernel overwrites, it does not accumulate), the gate
buffer is iq_ffn_chain_gate_bytes(M, F) bytes between sentinels.  A NaN in a result is a read outside an operand.

Gate hand-over.  The forward runs into a gate buffer prefilled with zeros and into one prefilled with 0xFF; the backward on
either gives the same bits, and gH equals the host statement: bits of rows past M are never read, every live dword is written
whole.  Route: every launch asserts {kernel name: 1} with <D, NW, RG, drop, mode>; chain_exact_ref.chain_shape restates the
thresholds next to the case table (chain_exact_ref.SMALL / LARGE).  Repeat: a second launch gives the same bits everywhere.

Dropout above FEW_MILLION elements: the host mask on row bands (first 512 rows, last 300, both sides of the first and the last
workgroup edge), every other element exactly one of its two exact values.

On a mismatch the message names cells written outside the result, else the VARIANTS entry the output equals, else
gemm_exact_ref.explain's bounding box and the one 64-aligned (ring chunk) or 32-aligned (MFMA step) k range that accounts for it.
The measured worst case of every tolerance, in units of its bound, is printed by test_zz_report (profiles/chain_exact.txt).
"""
import ctypes as C
import functools

import pytest
import torch

import chain_exact_ref as CR
import gemm_exact_ref as GR
from prof_names import kernel_launches
from test_gpu_gemm_exact import FEW_MILLION, PAT, Out, fenced, mask_rows, nan_view
from test_gpu_kernels import L, _N, dev, stream  # noqa: F401  (L is a fixture)
from test_gpu_wgrad_exact import NAN, Fenced

pytestmark = pytest.mark.gpu

IQ_OK, IQ_ERR_ARG, IQ_ERR_UNSUPPORTED = 0, 1, 2
EPS = 1e-12
FWD_NAME = "ffn_chain_fwd_kernel<%d, %d, %d, %s, %d>"       # <D, waves per workgroup, 16-row groups per wave, dropout, mode>
BWD_NAME = "ffn_chain_bwd_kernel<%d, %d, %d, %s, %d>"

ORDER = {
    "iq_ffn_chain_fwd": ["X1", "W1", "b1", "drop1", "H", "W2", "b2", "drop2", "gamma", "beta", "eps", "Z", "X", "mean", "rstd", "gate"],
    "iq_attn_out_ffn_chain_fwd": ["A", "Wo", "bo", "drop0", "R", "gamma1", "beta1", "Z1", "X1", "mean1", "rstd1", "W1", "b1", "drop1", "H",
                                  "W2", "b2", "drop2", "gamma", "beta", "eps", "Z", "X", "mean", "rstd", "gate", "Wq", "bq", "Yq"],
    "iq_ffn_chain_bwd": ["dO", "W2t", "gate", "gate_scale", "gH", "W1t", "R", "z1", "mean", "rstd", "gamma", "drop", "dz", "dy", "partial",
                         "Wot", "dA"],
    "iq_qkv_dgrad_ffn_chain_bwd": ["gQKV", "Wqkv_t", "R0", "z2", "mean2", "rstd2", "gamma2", "drop2", "dz2", "dy2", "partial2", "W2t", "gate",
                                   "gate_scale", "gH", "W1t", "R", "z1", "mean", "rstd", "gamma", "drop", "dz", "dy", "partial", "Wot", "dA"],
}
REPORT = {}                  # tolerance -> (worst observed / bound, case)
INSTANCES = {}               # kernel name -> cases that launched it


def note(name, ratio, what):
    ratio = float(ratio)
    if ratio > REPORT.get(name, (-1.0, ""))[0]:
        REPORT[name] = (ratio, what)


class Gate:
    """iq_ffn_chain_gate_bytes(M, F) bytes between two 256-byte sentinel regions, prefilled with `fill`."""

    def __init__(self, nbytes, fill):
        self.n = nbytes
        self.raw = torch.full((256 + nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev())
        self.body = self.raw[256:256 + nbytes]
        self.body.fill_(fill)

    def ptr(self):
        return self.body.data_ptr()

    def fences(self):
        return bool((self.raw[:256] == 0xA5).all()) and bool((self.raw[256 + self.n:] == 0xA5).all())


def ptr_of(v):
    if isinstance(v, (Out, Fenced, Gate)):
        return v.ptr()
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def site(on, s):
    if not on:
        return None
    d = _N().Dropout()
    d.seed, d.step, d.site, d.p, d.step_dev = GR.SEED, GR.STEP, s, GR.P, None
    return d


def call(L, entry, b, M, D, F, frames=None, **override):
    """One launch of `entry` on the buffers b (name -> Out / Fenced / Gate / tensor / dropout struct / number) -> (rc, launches)."""
    args = []
    for name in ORDER[entry]:
        v = override[name] if name in override else b.get(name)
        if name.startswith("drop"):
            args.append(C.byref(v) if v is not None else None)
        elif name == "eps":
            args.append(EPS)
        elif name == "gate_scale":
            args.append(CR.GATE_SCALE)
        else:
            args.append(ptr_of(v))
    rc = []
    rec = kernel_launches(L, lambda: rc.append(getattr(L, entry)(*args, M if frames is None else frames, 1, D, F, stream())))
    torch.cuda.synchronize()
    return rc[0], rec


@functools.lru_cache(maxsize=None)          # (a dozen (D, F) pairs, 45 MB each: drawn on the host once per process)
def dev_ops(D, F):
    return {k: v.to(dev()) for k, v in CR.operands(D, F).items()}


@functools.lru_cache(maxsize=None)
def dev_preb(D):
    return tuple(t.to(dev()) for t in CR.preb_operands(D))


def op(src):
    """A contiguous bf16 operand between GUARD rows of NaN."""
    v = nan_view(src.shape[0], src.shape[1], src.shape[1])
    v.copy_(src)
    return v


def vec(src):
    return fenced(src.float())


def nan_part(M, D):
    f = Fenced(CR.partial_rows(M) * 2 * D)
    f.body.fill_(NAN)
    return f


def snapshot(b):
    """The raw bits of every output of b (fences and surroundings included)."""
    return {k: (v.flat if isinstance(v, Out) else v.raw).clone() for k, v in b.items() if isinstance(v, (Out, Fenced, Gate)) and k in b["_outs"]}


def reset(b):
    for k in b["_outs"]:
        v = b[k]
        if isinstance(v, Out):
            v.reset()
        elif isinstance(v, Fenced):
            v.body.fill_(NAN)
        else:
            v.body.fill_(b["_gate_fill"])


def same_bits(a, b_, what):
    for k in a:
        assert torch.equal(a[k], b_[k]), f"{what}: {k} differs between two launches of the same problem"


def fences_ok(b, what):
    for k, v in b.items():
        if isinstance(v, Fenced):
            assert bool(v.fences().all()), f"{what}: sentinels around {k} overwritten"
        elif isinstance(v, Gate):
            assert v.fences(), f"{what}: sentinels around the gate buffer overwritten"


def bands(M):
    nw, rg = CR.chain_shape(M)
    per = nw * 16 * rg
    return mask_rows(M, (per, (M - 1) // per * per))


def masked(got, e1, e0, M, N, s, band):
    """The expected result under dropout from its two exact candidates (kept e1, dropped e0): the host mask of site s everywhere
    (band None) or on the rows `band`, and outside them whichever candidate the output holds."""
    if band is None:
        return torch.where(CR.keep(torch.arange(M, device=dev()), N, s), e1, e0)
    want = torch.where(got.view(torch.int16) == e0.view(torch.int16), e0, e1)
    want[band] = torch.where(CR.keep(band, N, s), e1[band], e0[band])
    return want


TRUE = lambda: torch.ones((), dtype=torch.bool, device=dev())
FALSE = lambda: torch.zeros((), dtype=torch.bool, device=dev())


def exact(out, want, what, cause=None):
    """out (an Out) holds `want` in its rows and PAT everywhere else -- or the message says what it holds instead."""
    rows = torch.arange(out.rows, device=dev())
    msg = out.compare(rows, want)
    if msg is None:
        return
    got = out.gather(rows)
    if cause is not None and not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        msg += cause(got)
    raise AssertionError(f"{what}: {msg}")


def which_variant(got, alts):
    for name, make in alts.items():
        if torch.equal(make().view(torch.int16), got.view(torch.int16)):
            return f"the output is what it would be if {CR.VARIANTS[name]}"
    return None


def product_bound(a, w, ref):
    """Bound of a bf16 store of an fp32-accumulated product a w^T (K terms) against fp64 `ref` of the same bf16 operands:
    every product of two bf16 values is exact in fp32 (16 significant bits); a sum of K fp32 terms taken in any order is off
    by at most (K - 1) 2^-24 sum|terms| to first order; the store adds half a bf16 ulp, 2^-9 |value|.  K <= 192 here:
    2^-8 |ref| + 2^-16 sum_k |a_k| |w_k| holds with a factor of two to spare in either term."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -16 * (a.double().abs() @ w.double().abs().t())


def check_norm(what, tag, Zwant, gamma, beta, X, mean, rstd):
    """X, mean, rstd of a forward norm against fp64 taken from the exact bf16 Z."""
    rows = torch.arange(X.rows, device=dev())
    ref, mu, rs = CR.layernorm(Zwant, gamma, beta, EPS)
    xg = X.gather(rows)
    assert X.compare(rows, xg) is None, f"{what}: {tag} written outside its rows"
    err = (xg.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ref.abs().max()
    note(f"{tag} / (2^-8 |ref| + 2^-16 max|ref|)", (err / bound).max(), what)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what} {tag}: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"
    for f, r, name in ((mean, mu, "mean"), (rstd, rs, "rstd")):
        assert not f.body.isnan().any(), f"{what}: a {name} nobody wrote"
        scale = r.abs().max().item() + 1e-12
        e = (f.body.double() - r).abs().max().item()
        note(f"{name} / (1e-5 max|ref|)", e / (1e-5 * scale), what)
        assert e <= 1e-5 * scale, f"{what} {name}: max err {e:.4g} vs scale {scale:.4g}"


def check_lnbwd(what, tag, dX, z, mean, rstd, gamma, dz, dy, part, M, D, drop, s):
    """The LayerNorm-backward tail on the exact integer dX: dz / dy against fp64, the dbeta partial rows exactly, dgamma 1e-3."""
    rows = torch.arange(M, device=dev())
    band = bands(M) if M * D > FEW_MILLION else None
    mrows = rows if band is None else band
    rdz, _, gmax, xhat = GR.lnbwd_reference(dX, z, mean, rstd, gamma)
    floor = 2.0 ** -16 * gmax * rstd.double()[:, None]
    tol = 2.0 ** -8 * rdz.abs() + floor
    gz = dz.gather(rows)
    assert dz.compare(rows, gz) is None, f"{what}: dz{tag} written outside its rows"
    err = (gz.double() - rdz).abs()
    note("dz / (2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd)", (err / tol).max(), what)
    bad = ~(err <= tol)
    assert not bad.any(), f"{what} dz{tag}: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"
    if drop:
        gy = dy.gather(rows)
        assert dy.compare(rows, gy) is None, f"{what}: dy{tag} written outside its rows"
        keep = CR.keep(mrows, D, s)
        rdy = torch.where(keep, rdz[mrows] * GR.DROP_SCALE, torch.zeros_like(rdz[mrows]))
        tdy = 2.0 ** -8 * rdy.abs() + floor[mrows]
        ey = (gy[mrows].double() - rdy).abs()
        note("dy / (2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd)", (ey / tdy).max(), what)
        bad = ~(ey <= tdy)
        assert not bad.any(), f"{what} dy{tag}: {int(bad.sum())} cells off the host mask, first at {bad.nonzero()[0].tolist()}"
        assert bool((gy[mrows][~keep].view(torch.int16) == 0).all()), f"{what} dy{tag}: a dropped element is not +0"
        free = ~((gy.view(torch.int16) == 0) | ((gy.double() - 2 * rdz).abs() <= 2.0 ** -7 * rdz.abs() + 2 * tol))
        assert not free.any(), f"{what} dy{tag}: {int(free.sum())} cells are neither dropped nor kept"
    else:
        assert dy.untouched(), f"{what}: dy{tag} written without a dropout site"
    n = CR.partial_rows(M)
    p = part.body.view(n, 2 * D)
    want = CR.dbeta_rows(dX, M)
    if not torch.equal(p[:, D:], want.float()):
        rows_off = (p[:, D:] != want.float()).any(1).nonzero().flatten().tolist()
        hint = ""
        if torch.equal(p[:, D:], CR.dbeta_rows(dX, M, "ragged_copies").float()):
            hint = f": the output is what it would be if {CR.VARIANTS['ragged_copies']}"
        raise AssertionError(f"{what}: dbeta partial rows{tag} differ from the column sums of dX at workgroups {rows_off[:8]} of {n}{hint}")
    ref = CR.dgamma_rows(dX, xhat, M)
    scale = ref.abs().max().item() + 1e-12
    e = (p[:, :D].double() - ref).abs().max().item()
    assert not p[:, :D].isnan().any(), f"{what}: a dgamma partial{tag} nobody wrote"
    note("dgamma partial rows / (1e-3 max|ref|)", e / (1e-3 * scale), what)
    assert e <= 1e-3 * scale, f"{what} dgamma partial rows{tag}: max err {e:.4g} vs scale {scale:.4g}"


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def fwd_buffers(M, D, F, mode, gate_fill=0, beta_int=False):
    o = dev_ops(D, F)
    b = dict(W1=op(o["W1"]), W2=op(o["W2"]), b1=vec(o["b1"]), b2=vec(o["b2"]),
             gamma=vec(torch.zeros(D) if beta_int else o["gamma"]), beta=vec(o["beta_int"] if beta_int else o["beta"]),
             H=Out(M, F, F), Z=Out(M, D, D), X=Out(M, D, D), mean=nan_f(M), rstd=nan_f(M), gate=Gate(CR.gate_bytes(M, F), gate_fill))
    b["_outs"], b["_gate_fill"] = ["H", "Z", "X", "mean", "rstd", "gate"], gate_fill
    if mode == 0:
        b["X1"] = op(o["X1"][:M])
    else:
        b.update(A=op(o["A"][:M]), Wo=op(o["Wo"]), bo=vec(o["bo"]), R=op(o["R"][:M]), gamma1=vec(o["gamma1"]), beta1=vec(o["beta1"]),
                 Z1=Out(M, D, D), X1=Out(M, D, D), mean1=nan_f(M), rstd1=nan_f(M))
        b["_outs"] += ["Z1", "X1", "mean1", "rstd1"]
    if mode == 2:
        b.update(Wq=op(o["Wq"]), bq=vec(o["bq"]), Yq=Out(M, 3 * D, 3 * D))
        b["_outs"] += ["Yq"]
    return b


def nan_f(n):
    f = Fenced(n)
    f.body.fill_(NAN)
    return f


def fwd_entry(mode):
    return "iq_ffn_chain_fwd" if mode == 0 else "iq_attn_out_ffn_chain_fwd"


def fwd_sites(b, drop):
    b.update(drop0=site(drop, CR.SITE0), drop1=site(drop, CR.SITE1), drop2=site(drop, CR.SITE2))


def fwd_name(M, D, drop, mode):
    nw, rg = CR.chain_shape(M)
    return FWD_NAME % (D, nw, rg, "true" if drop else "false", mode)


def launch_fwd(L, b, M, D, F, drop, mode, what):
    fwd_sites(b, drop)
    rc, rec = call(L, fwd_entry(mode), b, M, D, F)
    assert rc == IQ_OK, f"{what}: rc {rc}"
    assert rec == {fwd_name(M, D, drop, mode): 1}, f"{what}: launched {rec}, expected {fwd_name(M, D, drop, mode)}"
    INSTANCES.setdefault(fwd_name(M, D, drop, mode), set()).add((M, F))
    fences_ok(b, what)
    assert L.iq_ffn_chain_gate_bytes(M, F) == CR.gate_bytes(M, F)


def check_core_exact(what, b, M, D, F, drop):
    """H and Z of a launch whose X1 holds integers, then norm2 from the exact Z."""
    o = dev_ops(D, F)
    X1, rows = o["X1"][:M], torch.arange(M, device=dev())
    big = drop and M * F > FEW_MILLION
    band = bands(M) if big else None
    pre = CR.hidden_pre(X1, o["W1"], o["b1"])
    assert pre.max().item() <= CR.H_LIMIT
    gotH = b["H"].gather(rows)
    e1 = GR.round_bf16(pre * (GR.DROP_SCALE if drop else 1.0))
    wantH = masked(gotH, e1, torch.zeros_like(e1), M, F, CR.SITE1, band) if drop else e1

    def cause_h(got):
        alts = {"truncate": lambda: CR.hidden(X1, o["W1"], o["b1"], CR.keep(rows, F, CR.SITE1) if drop else None, "truncate")[0],
                "b1_mod_1024": lambda: CR.hidden(X1, o["W1"], o["b1"], CR.keep(rows, F, CR.SITE1) if drop else None, "b1_mod_1024")[0]}
        if drop:
            alts["mask_stride_d"] = lambda: CR.hidden(X1, o["W1"], o["b1"], CR.keep(rows, F, CR.SITE1, stride=D))[0]

        def epi_box(rs, cs, acc):
            k = CR.keep(rows[rs], F, CR.SITE1)[:, cs] if drop else None
            return GR.round_bf16(CR._drop(torch.clamp_min(acc + o["b1"][cs].double(), 0.0), k))
        return which_variant(got, alts) or GR.explain(X1, o["W1"], got, wantH, epi_box)
    exact(b["H"], wantH, what + " H", cause_h)
    acc = CR.z_acc(wantH, o["W2"])
    assert acc.abs().max().item() < 2 ** 22
    gotZ = b["Z"].gather(rows)
    if drop:
        zband = bands(M) if M * D > FEW_MILLION else None
        wantZ = masked(gotZ, CR.z_store(acc, o["b2"], X1, TRUE()), CR.z_store(acc, o["b2"], X1, FALSE()), M, D, CR.SITE2, zband)
    else:
        wantZ = CR.z_store(acc, o["b2"], X1)

    def cause_z(got):
        k2 = CR.keep(rows, D, CR.SITE2) if drop else None
        alts = {v: (lambda v=v: CR.z_store(acc, o["b2"], X1, k2, v)) for v in ("res_after_round", "truncate")}

        def epi_box(rs, cs, a):
            return CR.z_store(a, o["b2"][cs], X1[rs, cs], k2[rs, cs] if drop else None)
        return which_variant(got, alts) or GR.explain(wantH, o["W2"], got, wantZ, epi_box)
    exact(b["Z"], wantZ, what + " Z", cause_z)
    check_norm(what, "X", wantZ, b["gamma"].body, b["beta"].body, b["X"], b["mean"], b["rstd"])
    return wantH


def fwd_core_case(L, M, D, F, drop):
    what = f"ffn_chain_fwd M={M} D={D} F={F} drop={drop}"
    b = fwd_buffers(M, D, F, 0)
    launch_fwd(L, b, M, D, F, drop, 0, what)
    check_core_exact(what, b, M, D, F, drop)
    first = snapshot(b)
    reset(b)
    launch_fwd(L, b, M, D, F, drop, 0, what + " (again)")
    same_bits(first, snapshot(b), what)


def fwd_fused_case(L, M, D, F, drop, mode):
    what = f"attn_out_ffn_chain_fwd M={M} D={D} F={F} drop={drop} mode={mode}"
    o = dev_ops(D, F)
    rows = torch.arange(M, device=dev())
    b = fwd_buffers(M, D, F, mode)
    launch_fwd(L, b, M, D, F, drop, mode, what)
    # ---- first stage: Z1 exactly, norm1 from the exact Z1 ----
    A, R = o["A"][:M], o["R"][:M]
    got = b["Z1"].gather(rows)
    if drop:
        band = bands(M) if M * D > FEW_MILLION else None
        want = masked(got, CR.z1_store(A, o["Wo"], o["bo"], R, TRUE()), CR.z1_store(A, o["Wo"], o["bo"], R, FALSE()), M, D, CR.SITE0, band)
    else:
        want = CR.z1_store(A, o["Wo"], o["bo"], R)

    def cause(got):
        k0 = CR.keep(rows, D, CR.SITE0) if drop else None
        alts = {v: (lambda v=v: CR.z1_store(A, o["Wo"], o["bo"], R, k0, v)) for v in ("res_after_round", "truncate")}

        def epi_box(rs, cs, a):
            return CR.residual_store(CR._drop(a + o["bo"][cs].double(), k0[rs, cs] if drop else None), R[rs, cs])
        return which_variant(got, alts) or GR.explain(A, o["Wo"], got, want, epi_box)
    exact(b["Z1"], want, what + " Z1", cause)
    check_norm(what, "X1", want, b["gamma1"].body, b["beta1"].body, b["X1"], b["mean1"], b["rstd1"])
    # ---- everything behind it: the stand-alone entry point on the X1 this launch wrote, bit for bit ----
    s = fwd_buffers(M, D, F, 0)
    s["X1"] = b["X1"]                                       # (its surroundings hold PAT, a NaN)
    launch_fwd(L, s, M, D, F, drop, 0, what + " (stand-alone on its X1)")
    for k in ("H", "Z", "X"):
        assert torch.equal(b[k].raw, s[k].raw), f"{what}: {k} differs from iq_ffn_chain_fwd on the X1 written"
    for k in ("mean", "rstd"):
        assert torch.equal(b[k].raw, s[k].raw), f"{what}: {k} differs from iq_ffn_chain_fwd on the X1 written"
    full = (M // (16 * CR.chain_shape(M)[1])) * (F // 64) * 256          # (the bits of rows past M: the gate hand-over test)
    assert torch.equal(b["gate"].body[:full], s["gate"].body[:full]), f"{what}: gate bits differ from iq_ffn_chain_fwd's"
    assert not b["X"].gather(rows).isnan().any() and not b["H"].gather(rows).isnan().any(), f"{what}: NaN behind the first stage"
    if mode == 2:
        X = b["X"].gather(rows)
        ref = X.double() @ o["Wq"].double().t() + o["bq"].double()
        yq = b["Yq"].gather(rows)
        assert b["Yq"].compare(rows, yq) is None, f"{what}: Yq written outside its rows"
        err, bound = (yq.double() - ref).abs(), product_bound(X, o["Wq"], ref)
        note("Yq / product_bound", (err / bound).max(), what)
        bad = ~(err <= bound)
        assert not bad.any(), f"{what} Yq: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"
    first = snapshot(b)
    reset(b)
    launch_fwd(L, b, M, D, F, drop, mode, what + " (again)")
    same_bits(first, snapshot(b), what)


def post_exact_case(L, M, D, F, drop):
    """gamma2 = 0, beta2 integers: X is beta2 in every row and Yq = beta2 Wq^T + bq exactly -- the k coverage, the column order and
    the block pairing of the q,k,v stage (9 blocks in 5 ring chunks at D = 192, the last a half chunk; 6 in 3 at D = 128)."""
    what = f"attn_out_ffn_chain_fwd gamma2=0 M={M} D={D} F={F} drop={drop}"
    o = dev_ops(D, F)
    b = fwd_buffers(M, D, F, 2, beta_int=True)
    launch_fwd(L, b, M, D, F, drop, 2, what)
    exact(b["X"], o["beta_int"].to(torch.bfloat16).expand(M, D).contiguous(), what + " X")
    row = CR.yq_of_beta(o["beta_int"], o["Wq"], o["bq"])
    want = row.expand(M, 3 * D).contiguous()

    def cause(got):
        beta = o["beta_int"].to(torch.bfloat16).expand(M, D)
        return GR.explain(beta, o["Wq"], got, want, lambda rs, cs, a: GR.round_bf16(a + o["bq"][cs].double()))
    exact(b["Yq"], want, what + " Yq", cause)


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
def gates_of(L, M, D, F, drop, what):
    """The forward's gate bits, written into a buffer prefilled with zeros and into one prefilled with 0xFF."""
    out = []
    for fill in (0x00, 0xFF):
        b = fwd_buffers(M, D, F, 0, gate_fill=fill)
        fwd_sites(b, drop)
        b["drop2"] = None
        rc, rec = call(L, "iq_ffn_chain_fwd", b, M, D, F)
        assert rc == IQ_OK and rec == {fwd_name(M, D, drop, 0): 1}, f"{what}: forward rc {rc}, launched {rec}"
        assert b["gate"].fences(), f"{what}: the forward wrote outside the gate buffer"
        out.append(b["gate"])
    return out


def bwd_name(M, D, drop, mode):
    nw, rg = CR.chain_shape(M)
    return BWD_NAME % (D, nw, rg, "true" if drop else "false", mode)


def bwd_buffers(M, D, F, gate, with_da, fused=False):
    o = dev_ops(D, F)
    zf = o["z1"][:M].double()
    b = dict(W2t=op(o["W2t"]), W1t=op(o["W1t"]), gate=gate, z1=op(o["z1"][:M]), gamma=vec(o["gamma_b"]),
             mean=vec(zf.mean(-1)), rstd=vec(1 / torch.sqrt(zf.var(-1, unbiased=False) + EPS)),
             gH=Out(M, F, F), dz=Out(M, D, D), dy=Out(M, D, D), partial=nan_part(M, D))
    b["_outs"], b["_gate_fill"] = ["gH", "dz", "dy", "partial"], None
    if with_da:
        b.update(Wot=op(o["Wot"]), dA=Out(M, D, D))
        b["_outs"] += ["dA"]
    if fused:
        A, Wt, R0, z2, gamma2 = dev_preb(D)
        z2f = z2[:M].double()
        b.update(gQKV=op(A[:M]), Wqkv_t=op(Wt), R0=op(R0[:M]), z2=op(z2[:M]), gamma2=vec(gamma2), mean2=vec(z2f.mean(-1)),
                 rstd2=vec(1 / torch.sqrt(z2f.var(-1, unbiased=False) + EPS)), dz2=Out(M, D, D), dy2=Out(M, D, D), partial2=nan_part(M, D))
        b["R"] = b["dz2"]                                   # the second stage's residual: the rows this launch writes
        b["_outs"] += ["dz2", "dy2", "partial2"]
    else:
        b.update(dO=op(o["dO"][:M]), R=op(o["Rb"][:M]))
    return b


def launch_bwd(L, b, M, D, F, drop, mode, what):
    b.update(drop=site(drop, CR.SITE0), drop2=site(drop, CR.SITE2))
    entry = "iq_qkv_dgrad_ffn_chain_bwd" if mode == 2 else "iq_ffn_chain_bwd"
    rc, rec = call(L, entry, b, M, D, F)
    assert rc == IQ_OK, f"{what}: rc {rc}"
    assert rec == {bwd_name(M, D, drop, mode): 1}, f"{what}: launched {rec}, expected {bwd_name(M, D, drop, mode)}"
    INSTANCES.setdefault(bwd_name(M, D, drop, mode), set()).add((M, F))
    fences_ok(b, what)
    assert L.iq_ffn_chain_bwd_partial_rows(M) == CR.partial_rows(M)


def check_da(what, b, M, D, F, drop):
    o = dev_ops(D, F)
    rows = torch.arange(M, device=dev())
    src = (b["dy"] if drop else b["dz"]).gather(rows)
    ref = src.double() @ o["Wot"].double().t()
    got = b["dA"].gather(rows)
    assert b["dA"].compare(rows, got) is None, f"{what}: dA written outside its rows"
    err, bound = (got.double() - ref).abs(), product_bound(src, o["Wot"], ref)
    note("dA / product_bound", (err / bound).max(), what)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what} dA: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"


def bwd_core_case(L, M, D, F, drop):
    what = f"ffn_chain_bwd M={M} D={D} F={F} drop={drop}"
    o = dev_ops(D, F)
    rows = torch.arange(M, device=dev())
    gate0, gate1 = gates_of(L, M, D, F, drop, what)
    b = bwd_buffers(M, D, F, gate0, with_da=False)
    launch_bwd(L, b, M, D, F, drop, 0, what)
    # ---- gH against the host statement of the forward's H ----
    pre = CR.hidden_pre(o["X1"][:M], o["W1"], o["b1"])
    acc = CR.gh_acc(o["dO"][:M], o["W2t"])
    e1, v1 = CR.gh_store(acc, pre)
    assert v1.abs().max().item() <= CR.GH_LIMIT
    got = b["gH"].gather(rows)
    band = bands(M) if drop and M * F > FEW_MILLION else None
    want = masked(got, e1, torch.zeros_like(e1), M, F, CR.SITE1, band) if drop else e1

    def cause(got):
        k1 = CR.keep(rows, F, CR.SITE1) if drop else None
        Hexp = CR._drop(pre, k1)
        alts = {v: (lambda v=v: CR.gh_store(acc, Hexp, v)[0]) for v in ("gate_ge", "truncate")}
        return which_variant(got, alts) or GR.explain(o["dO"][:M], o["W2t"], got, want, lambda rs, cs, a: CR.gh_store(a, Hexp[rs, cs])[0])
    exact(b["gH"], want, what + " gH", cause)
    dX = CR.dx_of(want, o["W1t"], o["Rb"][:M])
    assert dX.abs().max().item() < GR.DX_LIMIT, "the amplitude condition of the reference"
    check_lnbwd(what, "", dX, o["z1"][:M], b["mean"].body, b["rstd"].body, b["gamma"].body, b["dz"], b["dy"], b["partial"], M, D, drop, CR.SITE0)
    first = snapshot(b)
    # ---- the gate bits written over 0xFF: the same result (bits of rows past M are never read, live dwords written whole) ----
    reset(b)
    b["gate"] = gate1
    launch_bwd(L, b, M, D, F, drop, 0, what + " (gate buffer prefilled with 0xFF)")
    same_bits(first, snapshot(b), what + " (gate buffer prefilled with 0xFF)")
    # ---- with Wot / dA: the same bits, and dA from the dy (dz) written ----
    a = bwd_buffers(M, D, F, gate0, with_da=True)
    launch_bwd(L, a, M, D, F, drop, 1, what + " +dA")
    for k in ("gH", "dz", "dy", "partial"):
        assert torch.equal(a[k].flat if isinstance(a[k], Out) else a[k].raw, first[k]), f"{what} +dA: {k} differs from the launch without dA"
    check_da(what + " +dA", a, M, D, F, drop)
    second = snapshot(a)
    reset(a)
    launch_bwd(L, a, M, D, F, drop, 1, what + " +dA (again)")
    same_bits(second, snapshot(a), what + " +dA")


def bwd_fused_case(L, M, D, F, drop):
    what = f"qkv_dgrad_ffn_chain_bwd M={M} D={D} F={F} drop={drop}"
    A, Wt, R0, z2, gamma2 = dev_preb(D)
    gate0, _ = gates_of(L, M, D, F, drop, what)
    b = bwd_buffers(M, D, F, gate0, with_da=True, fused=True)
    launch_bwd(L, b, M, D, F, drop, 2, what)
    dX2 = A[:M].double() @ Wt.double().t() + R0[:M].double()
    assert dX2.abs().max().item() < GR.DX_LIMIT, "the amplitude condition of the reference"
    check_lnbwd(what, "2", dX2, z2[:M], b["mean2"].body, b["rstd2"].body, b["gamma2"].body, b["dz2"], b["dy2"], b["partial2"], M, D, drop, CR.SITE2)
    # ---- everything behind it: iq_ffn_chain_bwd on the dy2 / dz2 this launch wrote, bit for bit ----
    s = bwd_buffers(M, D, F, gate0, with_da=True)
    s["dO"], s["R"] = (b["dy2"] if drop else b["dz2"]), b["dz2"]
    launch_bwd(L, s, M, D, F, drop, 1, what + " (stand-alone on its dy2 / dz2)")
    for k in ("gH", "dz", "dy", "dA", "partial"):
        x, y = (b[k].flat, s[k].flat) if isinstance(b[k], Out) else (b[k].raw, s[k].raw)
        assert torch.equal(x, y), f"{what}: {k} differs from iq_ffn_chain_bwd on the dy2 / dz2 written"
    rows = torch.arange(M, device=dev())
    assert not b["gH"].gather(rows).isnan().any() and not b["dA"].gather(rows).isnan().any(), f"{what}: NaN behind the first stage"
    first = snapshot(b)
    reset(b)
    launch_bwd(L, b, M, D, F, drop, 2, what + " (again)")
    same_bits(first, snapshot(b), what)


# ------------------------------------------------------------------------------------------------
# the case table (chain_exact_ref.SMALL / LARGE, restated there beside chain_shape's thresholds)
# ------------------------------------------------------------------------------------------------
SMALL = [(D, F) for D in CR.SMALL for F in CR.SMALL[D]]
BIG = [(M, D) for M in CR.LARGE for D in (128, 192)]
small_ids = [f"D{d}-F{f}" for d, f in SMALL]
big_ids = [f"M{m}-D{d}" for m, d in BIG]


def sweep_small(fn, L, D, F, *more):
    for M in CR.SMALL[D][F]:
        for drop in (False, True):
            fn(L, M, D, F, drop, *more)


def sweep_big(fn, L, M, D, *more):
    for F in CR.LARGE[M][D]:
        for drop in (False, True):
            fn(L, M, D, F, drop, *more)


@pytest.mark.parametrize("D,F", SMALL, ids=small_ids)
def test_forward_core_small_rows(L, D, F):
    sweep_small(fwd_core_case, L, D, F)


@pytest.mark.parametrize("M,D", BIG, ids=big_ids)
def test_forward_core_at_the_shape_thresholds(L, M, D):
    sweep_big(fwd_core_case, L, M, D)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("D,F", SMALL, ids=small_ids)
def test_forward_fused_small_rows(L, D, F, mode):
    sweep_small(fwd_fused_case, L, D, F, mode)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("M,D", BIG, ids=big_ids)
def test_forward_fused_at_the_shape_thresholds(L, M, D, mode):
    sweep_big(fwd_fused_case, L, M, D, mode)


@pytest.mark.parametrize("D,F", SMALL, ids=small_ids)
def test_qkv_stage_exact_small_rows(L, D, F):
    sweep_small(post_exact_case, L, D, F)


@pytest.mark.parametrize("M,D", BIG, ids=big_ids)
def test_qkv_stage_exact_at_the_shape_thresholds(L, M, D):
    sweep_big(post_exact_case, L, M, D)


@pytest.mark.parametrize("D,F", SMALL, ids=small_ids)
def test_backward_core_small_rows(L, D, F):
    sweep_small(bwd_core_case, L, D, F)


@pytest.mark.parametrize("M,D", BIG, ids=big_ids)
def test_backward_core_at_the_shape_thresholds(L, M, D):
    sweep_big(bwd_core_case, L, M, D)


@pytest.mark.parametrize("D,F", SMALL, ids=small_ids)
def test_backward_fused_small_rows(L, D, F):
    sweep_small(bwd_fused_case, L, D, F)


@pytest.mark.parametrize("M,D", BIG, ids=big_ids)
def test_backward_fused_at_the_shape_thresholds(L, M, D):
    sweep_big(bwd_fused_case, L, M, D)


# ------------------------------------------------------------------------------------------------
# limits and refusals
# ------------------------------------------------------------------------------------------------
def test_lds_limit_of_supported_widths(L):
    assert L.iq_ffn_chain_supported(1, 192, 2368) == 1 and L.iq_ffn_chain_supported(1, 192, 2432) == 0
    assert L.iq_ffn_chain_supported(1, 128, 15232) == 1 and L.iq_ffn_chain_supported(1, 128, 15296) == 0


def untouched(b):
    for k in b["_outs"]:
        v = b[k]
        if isinstance(v, Out):
            if not v.untouched():
                return k
        elif isinstance(v, Fenced):
            if not (bool(v.body.isnan().all()) and bool(v.fences().all())):
                return k
        elif not (bool((v.body == b["_gate_fill"]).all()) and v.fences()):
            return k
    return None


RM, RD, RF = 17, 128, 64              # the refusal cases: one ragged workgroup


@functools.lru_cache(maxsize=None)
def refusal_fwd(mode):
    b = fwd_buffers(RM, RD, RF, mode, gate_fill=0x5A)
    fwd_sites(b, True)
    return b


@functools.lru_cache(maxsize=None)
def refusal_bwd(mode):
    b = bwd_buffers(RM, RD, RF, Gate(CR.gate_bytes(RM, RF), 0), with_da=mode >= 1, fused=mode == 2)
    b.update(drop=site(True, CR.SITE0), drop2=site(True, CR.SITE2))
    return b


def refused(L, entry, b, want, what, D=RD, F=RF, frames=None, **override):
    rc, rec = call(L, entry, b, RM, D, F, frames=frames, **override)
    assert rc == want and rec == {}, f"{what}: rc {rc} (expected {want}), launched {rec}"
    k = untouched(b)
    assert k is None, f"{what}: {k} was written by a refused call"


FWD_PTRS = ["X1", "W1", "b1", "H", "W2", "b2", "gamma", "beta", "Z", "X", "gate"]
PRE_PTRS = ["A", "Wo", "bo", "R", "gamma1", "beta1", "Z1", "Wq", "bq", "Yq"]
BWD_PTRS = ["dO", "W2t", "gate", "gH", "W1t", "R", "z1", "gamma", "dz", "dy", "partial", "Wot", "dA"]
PREB_PTRS = ["gQKV", "Wqkv_t", "R0", "z2", "gamma2", "dz2", "dy2", "partial2"]


@pytest.mark.parametrize("which", FWD_PTRS + PRE_PTRS)
def test_forward_refuses_pointers_off_16_bytes(L, which):
    mode = 2 if which in PRE_PTRS else 0
    b = refusal_fwd(mode)
    refused(L, fwd_entry(mode), b, IQ_ERR_ARG, f"{which} 8 bytes off", **{which: ptr_of(b[which]) + 8})
    rc, rec = call(L, fwd_entry(mode), b, RM, RD, RF)
    assert rc == IQ_OK and len(rec) == 1
    reset(b)


@pytest.mark.parametrize("which", BWD_PTRS + PREB_PTRS)
def test_backward_refuses_pointers_off_16_bytes(L, which):
    mode = 2 if which in PREB_PTRS else 1
    entry = "iq_qkv_dgrad_ffn_chain_bwd" if mode == 2 else "iq_ffn_chain_bwd"
    b = refusal_bwd(mode)
    refused(L, entry, b, IQ_ERR_ARG, f"{which} 8 bytes off", **{which: ptr_of(b[which]) + 8})
    rc, rec = call(L, entry, b, RM, RD, RF)
    assert rc == IQ_OK and len(rec) == 1
    reset(b)


def test_refusals_touch_nothing(L):
    for mode in (0, 2):
        b = refusal_fwd(mode)
        refused(L, fwd_entry(mode), b, IQ_ERR_UNSUPPORTED, "F = 15,296 at D = 128", F=15296)
        refused(L, fwd_entry(mode), b, IQ_ERR_UNSUPPORTED, "F = 96", F=96)
        refused(L, fwd_entry(mode), b, IQ_ERR_UNSUPPORTED, "D = 256", D=256)
        refused(L, fwd_entry(mode), b, IQ_OK, "frames = 0", frames=0)
        refused(L, fwd_entry(mode), b, IQ_OK, "frames = -3", frames=-3)
    b = refusal_fwd(2)
    refused(L, fwd_entry(2), b, IQ_ERR_ARG, "Wq without bq", bq=None)
    refused(L, fwd_entry(2), b, IQ_ERR_ARG, "Wq without Yq", Yq=None)
    refused(L, fwd_entry(2), b, IQ_ERR_ARG, "bq and Yq without Wq", Wq=None)
    for mode in (0, 1, 2):
        entry = "iq_qkv_dgrad_ffn_chain_bwd" if mode == 2 else "iq_ffn_chain_bwd"
        b = refusal_bwd(mode)
        refused(L, entry, b, IQ_ERR_UNSUPPORTED, "F = 15,296 at D = 128", F=15296)
        refused(L, entry, b, IQ_ERR_UNSUPPORTED, "D = 256", D=256)
        refused(L, entry, b, IQ_OK, "frames = 0", frames=0)
        refused(L, entry, b, IQ_ERR_ARG, "dropout on without dy", dy=None)
    b = refusal_bwd(1)
    refused(L, "iq_ffn_chain_bwd", b, IQ_ERR_ARG, "Wot without dA", dA=None)
    refused(L, "iq_ffn_chain_bwd", b, IQ_ERR_ARG, "dA without Wot", Wot=None)
    b = refusal_bwd(2)
    refused(L, "iq_qkv_dgrad_ffn_chain_bwd", b, IQ_ERR_ARG, "the fused backward without Wot / dA", Wot=None, dA=None)
    refused(L, "iq_qkv_dgrad_ffn_chain_bwd", b, IQ_ERR_ARG, "dropout on without dy2", dy2=None)
    half = site(True, CR.SITE2)
    half.p = 0.25
    refused(L, "iq_qkv_dgrad_ffn_chain_bwd", b, IQ_ERR_ARG, "p0 != p1", drop2=half)
    refused(L, "iq_qkv_dgrad_ffn_chain_bwd", b, IQ_ERR_ARG, "p0 = 0, p1 = 0.5", drop2=None)


def test_zz_report(L):
    """Prints what ran: per kernel instance the (M, F) cases that launched it, per tolerance the worst observed value in units of
    its bound.  Asserts only that a full run of this file reached every instance of the case table."""
    print()
    for name in sorted(INSTANCES):
        print(f"{name}: {len(INSTANCES[name])} shapes, M x F = {sorted(INSTANCES[name])}")
    for name in sorted(REPORT):
        print(f"worst {name} = {REPORT[name][0]:.3f}   ({REPORT[name][1]})")
    if len(INSTANCES) >= 72:                       # a full run: 2 directions x 2 D x 3 shapes x 2 dropout settings x 3 modes
        assert len(INSTANCES) == 72
        assert all(v[0] <= 1.0 for v in REPORT.values())
