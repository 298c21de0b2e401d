"""GPU (MI355X): the forward / data-gradient GEMM family bit for bit, at every launch route and tile edge:
iq_gemm_bf16_nt (csrc/gemm_nt.hip, csrc/gemm_big.hip), iq_gemm_bf16_ln (csrc/gemm_ln.hip), iq_gemm_bf16_lnbwd (csrc/gemm_lnbwd.hip).

Method.  A and B / W hold seeded integers in [-2, 2] stored as bf16; bias, positional table and residual integers in
[-8, 8]; the gate values from {-1, -0.0, 0, 1}; gate_scale 1.25; dropout p = 0.5 (thresh 32768, scale exactly 2).  Every
product, partial sum and epilogue step is then a multiple of 1/4 far below 2^22 (gemm_exact_ref.assert_exact), so the fp32
value before the store is exact in ANY summation order and the stored value is that number rounded once to bf16, to nearest
even.  tests/gemm_exact_ref.py states the header's epilogue (+bias, relu, +pe with the row remap, dropout, *gate, +residual)
in fp64 with the keep mask of tests/dropout_ref.py indexed by OUTPUT element; int16 views are compared with torch.equal.
No GEMM output carries a tolerance.  The only tolerances are the LayerNorm ones: X of iq_gemm_bf16_ln within
2^-8 |ref| + 2^-16 max|ref| of fp64 taken from the exact Z, dz / dy of iq_gemm_bf16_lnbwd within
2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd of fp64 on the exact integer dX (max|dX| < 128, asserted before the launch: a
one-unit error in dX moves dz by about rstd * gamma, far outside that), mean / rstd 1e-5 and dgamma 1e-3 of the scale.

Surroundings.  Every bf16 operand lives in a NaN-filled buffer: GUARD rows of the same ld before and after, NaN in columns
K..ld (N..ld).  Every bf16 output is GUARD + rows + GUARD rows of ld elements (ldc = N + 8 for iq_gemm_bf16_nt) prefilled
with PAT, a NaN whose payload no kernel produces, and is compared WHOLE against an image that holds PAT everywhere outside
the result -- the class-token rows of embedding mode included.  fp32 vectors sit between sentinel words (NaN as values).
A NaN inside a result is a read outside an operand.

Dropout.  Small results are compared against the host mask at every element.  Above 4 M elements the mask is compared on
row bands (the first 512 rows, the last 300, both sides of the tile / band edges the case names) and every other element
must equal exactly one of its two exact values, kept or dropped.

Routes.  Every case asserts {kernel name: launches} (prof_names.kernel_launches); the thresholds are restated where the
cases are listed, from iq_gemm_bf16_nt, gemm_big_try, band_workgroups, the rows64 rule and lnbwd_block_rows.

On a mismatch the message names cells written outside the result, else a known cause whose result the output equals
(gemm_exact_ref.VARIANTS), else the bounding box of the wrong cells and ONE contiguous range of k, aligned to 64 or 32,
whose contribution equals the error ("k 96..127 missing").
"""
import ctypes as C
import functools

import pytest
import torch

import gemm_exact_ref as GR
from prof_names import kernel_launches
from test_gpu_kernels import L, _N, close_f32, dev, stream  # noqa: F401  (L is a fixture)
from test_gpu_wgrad_exact import GUARD, NAN, Fenced

pytestmark = pytest.mark.gpu

IQ_OK, IQ_ERR_ARG = 0, 1
PAT = 0x7FE5                 # bf16 NaN with a payload: no kernel produces it (an arithmetic NaN is 0x7FC0 / 0xFFC0)
FEW_MILLION = 4 << 20        # results above this many elements compare the dropout mask on row bands
M_EDGES = [1, 63, 64, 65, 127, 128, 129, 257]

REG = "gemm_nt_kernel<%d, %d>"                       # <column tile, epilogue mode>
ASYNC = "gemm_nt_async_kernel<%d, %d, %d, false>"    # <row tile, column tile, epilogue mode>
RESK = "gemm_nt_async_kernel<128, %d, 1, true>"      # <N>
BIG = "gemm_big_kernel<%d>"                          # <epilogue mode>
LN = "gemm_ln_kernel<%d, %d>"                        # <row block, D>
LN_BAND = "gemm_ln_band_kernel<192>"
LNBWD = "gemm_lnbwd_kernel<%d, %d>"                  # <row block, D>
EPI_RES, EPI_GATE, EPI_PE = 1, 2, 4


def gen(*key):
    s = 0
    for k in key:
        s = s * 1000003 + int(k)
    return torch.Generator(device="cuda").manual_seed(s % (2 ** 62))


def nan_view(M, cols, ld, lead=0):
    """[M, cols] view inside a NaN-filled bf16 buffer of GUARD + M + GUARD rows of ld elements (`lead` elements in front move
    the base).  The view keeps the buffer alive."""
    rows = GUARD + M + GUARD
    flat = torch.full((lead + rows * ld,), NAN, dtype=torch.bfloat16, device=dev())
    return flat[lead:].view(rows, ld)[GUARD:GUARD + M, :cols]


def ints(g, M, cols, ld, amp, lead=0):
    v = nan_view(M, cols, ld, lead)
    v.copy_(torch.randint(-amp, amp + 1, (M, cols), device=dev(), generator=g))
    return v


def gates(g, M, cols, ld, lead=0):
    v = nan_view(M, cols, ld, lead)
    values = torch.tensor([-1.0, -0.0, 0.0, 1.0], dtype=torch.bfloat16, device=dev())
    v.copy_(values[torch.randint(0, 4, (M, cols), device=dev(), generator=g)])
    return v


def fenced(values):
    """fp32 values between two sentinel regions (the sentinel reads as NaN)."""
    f = Fenced(values.numel())
    f.body.copy_(values.flatten())
    return f


def ints_f32(g, n, amp=GR.AMP_E):
    return fenced(torch.randint(-amp, amp + 1, (n,), device=dev(), generator=g).float())


class Out:
    """A bf16 result of `rows` x `cols` inside GUARD + rows + GUARD rows of ld elements, all prefilled with PAT."""

    def __init__(self, rows, cols, ld, lead=0):
        self.rows, self.cols = rows, cols
        self.flat = torch.empty(lead + (GUARD + rows + GUARD) * ld, dtype=torch.int16, device=dev())
        self.raw = self.flat[lead:].view(GUARD + rows + GUARD, ld)
        self.body = self.raw[GUARD:GUARD + rows, :cols]
        self.reset()

    def reset(self):
        self.flat.fill_(PAT)

    def ptr(self):
        return self.body.data_ptr()

    def gather(self, rows):
        """bf16 [len(rows), cols]: the result rows `rows`."""
        return self.body[rows].view(torch.bfloat16)

    def compare(self, rows, want):
        """None when the buffer holds `want` (bf16 [len(rows), cols]) at result rows `rows` and PAT everywhere else; else the
        cells written outside the result, or "" when only cells inside differ."""
        img = torch.full_like(self.raw, PAT)
        img[GUARD + rows, :self.cols] = want.view(torch.int16)
        if torch.equal(self.raw, img):
            return None
        inside = torch.zeros_like(self.raw, dtype=torch.bool)
        inside[GUARD + rows, :self.cols] = True
        stray = ((self.raw != PAT) & ~inside).nonzero()
        if len(stray):
            r, c = stray[:, 0] - GUARD, stray[:, 1]
            return (f"{len(stray)} cells written OUTSIDE the result: rows {int(r.min())}..{int(r.max())} (the result has "
                    f"{self.rows}), cols {int(c.min())}..{int(c.max())} (N = {self.cols}); ")
        return ""

    def untouched(self):
        return bool((self.flat == PAT).all())


def drop_site(on):
    d = _N().Dropout()
    d.seed, d.step, d.site, d.p, d.step_dev = GR.SEED, GR.STEP, GR.SITE, (GR.P if on else 0.0), None
    return d


def mask_rows(M, edges=()):
    """Input rows whose mask is compared against the host: all of them, or the bands of a large result."""
    if not edges:
        return None
    parts = [torch.arange(0, min(512, M)), torch.arange(max(M - 300, 0), M)]
    parts += [torch.arange(max(e - 16, 0), min(e + 16, M)) for e in edges]
    return torch.unique(torch.cat(parts)).to(dev())


def with_mask(got, e1, e0, rows_out, N, band):
    """The expected result under dropout from its two exact candidates (kept e1, dropped e0): the host mask on `band` (input
    rows; None = everywhere), and outside it whichever candidate the output holds."""
    if band is None:
        return torch.where(GR.keep_rows(rows_out, N), e1, e0)
    want = torch.where(got.view(torch.int16) == e0.view(torch.int16), e0, e1)
    want[band] = torch.where(GR.keep_rows(rows_out[band], N), e1[band], e0[band])
    return want


TRUE = lambda: torch.ones((), dtype=torch.bool, device=dev())
FALSE = lambda: torch.zeros((), dtype=torch.bool, device=dev())


# ------------------------------------------------------------------------------------------------
# iq_gemm_bf16_nt
# ------------------------------------------------------------------------------------------------
class NT:
    """One iq_gemm_bf16_nt problem: operands in NaN surroundings, the fp64 accumulator, the fenced output; `run` launches one
    epilogue on it.  emb = (tok, seq, cls_off)."""

    def __init__(self, M, N, K, emb=None, lead_a=0, lda=None, seed=0):
        GR.assert_exact(K)
        self.M, self.N, self.K, self.emb, self.seed = M, N, K, emb, seed
        g = gen(seed, M, N, K)
        self.lda, self.ldb, self.ldc = lda or K + 8, K + 8, N + 8
        self.A = ints(g, M, K, self.lda, GR.AMP_A, lead_a)
        self.B = ints(g, N, K, self.ldb, GR.AMP_B)
        tok, seq, cls_off = emb or (0, 0, 0)
        self.rows = GR.out_rows(M, tok, seq, cls_off, dev())
        self.rows_out = (M + tok - 1) // tok * seq if emb else M
        self.out = Out(self.rows_out, N, self.ldc)
        self.acc = self.A.double() @ self.B.double().t()
        self.what = f"M={M} N={N} K={K} emb={emb}"

    @functools.cached_property
    def bias(self):
        return ints_f32(gen(self.seed, self.N, 1), self.N)

    @functools.cached_property
    def pe(self):
        return ints_f32(gen(self.seed, self.N, 2), self.emb[1] * self.N)

    @functools.cached_property
    def gate(self):
        return gates(gen(self.seed, self.M, self.N, 3), self.M, self.N, self.N + 8)

    @functools.cached_property
    def res(self):
        return ints(gen(self.seed, self.M, self.N, 4), self.M, self.N, self.N + 24, GR.AMP_E)

    def epilogue(self, bias=False, relu=False, drop=False, gate=False, res=False):
        """-> (the C struct, the value operands of gemm_exact_ref.epilogue in input-row order)."""
        e = _N().Epilogue()
        kw = dict(relu=bool(relu))
        if bias:
            e.bias, kw["bias"] = self.bias.ptr(), self.bias.body
        e.relu = int(relu)
        if self.emb:
            tok, seq, cls_off = self.emb
            e.pe, e.tok, e.seq, e.cls_off = self.pe.ptr(), tok, seq, cls_off
            kw["pe"] = self.pe.body.view(seq, self.N)[torch.arange(self.M, device=dev()) % tok + cls_off]
        e.drop = drop_site(drop)
        if gate:
            e.gate, e.ldg, e.gate_scale, kw["gate"] = self.gate.data_ptr(), self.gate.stride(0), GR.GATE_SCALE, self.gate
        if res:
            e.residual, e.ldr, kw["residual"] = self.res.data_ptr(), self.res.stride(0), self.res
        return e, kw

    def launch(self, L, e, A=None, B=None, Cp=None):
        self.out.reset()
        rc = []
        rec = kernel_launches(L, lambda: rc.append(L.iq_gemm_bf16_nt(
            A or self.A.data_ptr(), self.lda, B or self.B.data_ptr(), self.ldb, Cp or self.out.ptr(), self.ldc, self.M, self.N,
            self.K, C.byref(e), stream())))
        torch.cuda.synchronize()
        return rc[0], rec

    def run(self, L, want, edges=(), **flags):
        e, kw = self.epilogue(**flags)
        what = f"{self.what} {flags}"
        rc, rec = self.launch(L, e)
        assert rc == IQ_OK, f"{what}: rc {rc}"
        assert rec == want, f"{what}: launched {rec}, expected {want}"
        for name in ("bias", "pe"):
            f = self.__dict__.get(name)
            assert f is None or bool(f.fences().all()), f"{what}: sentinels around the INPUT {name} overwritten"
        got = self.out.gather(self.rows)
        drop = flags.get("drop", False)
        if drop:
            band = mask_rows(self.M, edges) if self.M * self.N > FEW_MILLION else None
            e1, e0 = GR.stored(self.acc, keep=TRUE(), **kw), GR.stored(self.acc, keep=FALSE(), **kw)
            expect = with_mask(got, e1, e0, self.rows, self.N, band)
        else:
            expect = GR.stored(self.acc, **kw)
        msg = self.out.compare(self.rows, expect)
        if msg is None:
            return
        if not torch.equal(got.view(torch.int16), expect.view(torch.int16)):
            msg += self.cause(got, expect, kw, drop)
        raise AssertionError(f"{what} {rec}: {msg}")

    def cause(self, got, expect, kw, drop):
        keep = GR.keep_rows(self.rows, self.N) if drop else None               # (the whole host mask: a failure may take its time)
        keep_in = GR.keep_rows(torch.arange(self.M, device=dev()), self.N) if drop else None
        for name, text in GR.VARIANTS.items():
            alt = GR.stored(self.acc, name, keep_in, keep=keep, **kw)
            if torch.equal(alt.view(torch.int16), got.view(torch.int16)):
                return f"the output is what it would be if {text}"

        def epi_box(rs, cs, acc):
            box = {k: (v[cs] if k == "bias" else v[rs, cs]) for k, v in kw.items() if k != "relu"}
            keep = GR.keep_rows(self.rows[rs], self.N)[:, cs] if drop else None
            return GR.stored(acc, relu=kw["relu"], keep=keep, **box)
        return GR.explain(self.A, self.B, got, expect, epi_box)


# the five epilogue modes of the kernels' EPI template argument
MODES = {0: {}, EPI_RES: dict(res=True), EPI_GATE: dict(gate=True), EPI_RES | EPI_GATE: dict(res=True, gate=True), EPI_PE: {}}
EMB_SWEEP = (4, 5, 1)                # tok, seq, cls_off of the PE mode in the sweeps: M need not be a multiple of tok
FLAGS = [dict(bias=b, relu=r, drop=d) for b in (False, True) for r in (False, True) for d in (False, True)]


def nt_sweep(L, K, Ns, name, modes, Ms=M_EDGES):
    """Every N x M of the tables; the modes listed run at every shape, the eight (bias, relu, drop) settings rotate."""
    i = 0
    for N_, bn in Ns.items():
        for M in Ms:
            for mode in modes:
                p = NT(M, N_, K, emb=EMB_SWEEP if mode == EPI_PE else None, seed=K)
                p.run(L, {name(bn, mode): 1}, **MODES[mode], **FLAGS[(i + i // 8) % 8])
                i += 1


# Register-staged fallback: K % 32 != 0.  Column tile 128 when N % 128 == 0 or N > 512, else 64: N = 520 is five 128-column
# tiles (the last holds 8 columns), the others one to three 64-column tiles, ragged but for N = 64.
REG_N = {8: 64, 40: 64, 64: 64, 72: 64, 136: 64, 520: 128}


@pytest.mark.parametrize("K", [8, 40, 72, 200])
def test_register_staged_fallback_at_every_tile_edge(L, K):
    """K = 8: one partly filled 64-deep step; 40, 72: a ragged last step; 200: four steps.  The five modes rotate with the
    flags: every (mode, flags) pair runs at several shapes of the sweep."""
    i = 0
    for N_, bn in REG_N.items():
        for M in M_EDGES:
            mode = list(MODES)[i % 5]
            p = NT(M, N_, K, emb=EMB_SWEEP if mode == EPI_PE else None, seed=K)
            p.run(L, {REG % (bn, mode): 1}, **MODES[mode], **FLAGS[(i // 5 + i) % 8])
            i += 1


# Ring kernel: K % 32 == 0.  Row tile 64 while ceil(M / 128) * ceil(N / bn) < 512 (every shape of this sweep), else 128.
ASYNC_N = {64: 64, 128: 128, 320: 64, 576: 128, 1024: 128}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K", [32, 64, 96, 128, 160])
def test_ring_kernel_at_every_stage_count_and_tile_edge(L, K, mode):
    """K / 32 = 1..5 stages against a ring of three; the early-tail variants (RES, GATE) peel their last two stages."""
    nt_sweep(L, K, ASYNC_N, lambda bn, m: ASYNC % (64, bn, m), [mode])


# N = 1024 (8 column tiles of 128): ceil(M / 128) * 8 < 512 <=> M <= 8,064.
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,bm", [(8064, 64), (8065, 128)])
def test_ring_kernel_row_tile_on_either_side_of_512_tiles(L, M, bm, mode):
    p = NT(M, 1024, 64, emb=EMB_SWEEP if mode == EPI_PE else None, seed=5)
    for flags in (FLAGS[0], FLAGS[7]):
        p.run(L, {ASYNC % (bm, 128, mode): 1}, edges=(4032,), **MODES[mode], **flags)


# Residual as K stages: epilogue RES alone (no bias, ReLU, dropout), N in {128, 192}, K >= 384.  Otherwise the 64-row ring
# kernel with column tile 128 (N = 128) or 64 (N = 192 is neither a multiple of 128 nor above 512).
@pytest.mark.parametrize("N_,bn", [(128, 128), (192, 64)])
def test_residual_as_k_stages_and_its_three_ways_out(L, N_, bn):
    for M in (1, 127, 128, 129, 1000):
        NT(M, N_, 384, seed=6).run(L, {RESK % N_: 1}, res=True)
        NT(M, N_, 352, seed=6).run(L, {ASYNC % (64, bn, EPI_RES): 1}, res=True)
        NT(M, N_, 384, seed=7).run(L, {ASYNC % (64, bn, EPI_RES): 1}, res=True, bias=True)
    NT(129, N_, 384, seed=8).run(L, {ASYNC % (64, bn, EPI_RES): 1}, res=True, drop=True)
    NT(129, N_, 384, seed=8).run(L, {ASYNC % (64, bn, EPI_RES): 1}, res=True, relu=True)
    NT(129, N_, 1024, seed=8).run(L, {RESK % N_: 1}, res=True)
    # K = 1024 with dropout: thousands of cells past 256, where bf16 holds even integers only and the ONE rounding shows
    NT(1000, N_, 1024, seed=8).run(L, {ASYNC % (64, bn, EPI_RES): 1}, res=True, bias=True, drop=True)


# Embedding mode: the output row, the table row and the mask index all follow the remap; M is no multiple of the 64- or
# 128-row tile, so one tile spans frames and the last is ragged.  K = 40 takes the fallback, K = 64 the ring kernel.
@pytest.mark.parametrize("K,N_,name", [(64, 128, ASYNC % (64, 128, EPI_PE)), (40, 72, REG % (64, EPI_PE)), (64, 320, ASYNC % (64, 64, EPI_PE))])
@pytest.mark.parametrize("emb,frames", [((4, 5, 1), 33), ((16, 16, 0), 9), ((4, 5, 1), 67)], ids=["tok4seq5cls1", "tok16seq16", "tok4-three-tiles"])
def test_embedding_mode_remaps_rows_table_and_mask(L, emb, frames, K, N_, name):
    M = frames * emb[0]
    assert M % 64 != 0
    p = NT(M, N_, K, emb=emb, seed=9)
    p.run(L, {name: 1}, bias=True, drop=True)
    p.run(L, {name: 1}, bias=True, relu=True)
    p.run(L, {name: 1}, drop=True)


# gemm_big_try: N % 256 == 0, K % 64 == 0, K >= 256, M >= 2048, modes 0 / RES / GATE, and ceil(M / 256) * (N / 256) >= 512.
# N = 3072 (12 column blocks): 10,752 rows = 42 row blocks = 504 tiles stays on the ring kernel (128 x 128: 2,016 tiles);
# 10,753 = 43 blocks = 516 tiles, the last row block holds ONE row and 256 workgroups share 516 tiles unevenly; + 255: a last
# block of 255 rows.  N = 1024 (4 blocks), 32,590 rows = 128 blocks = 512 tiles.  K / 64 = 4 (the least), 5 (odd), 12.
BIG_CASES = [(10752, 3072, 256, False), (10753, 3072, 256, True), (10753 + 255, 3072, 256, True),
             (10752, 3072, 320, False), (10753, 3072, 320, True), (10753 + 255, 3072, 320, True),
             (32513 + 77, 1024, 768, True)]


@pytest.mark.parametrize("M,N_,K,big", BIG_CASES, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}" for c in BIG_CASES])
def test_persistent_256_tile_kernel_and_its_512_tile_floor(L, M, N_, K, big):
    p = NT(M, N_, K, seed=10)
    name = lambda mode: {BIG % mode if big else ASYNC % (128, 128, mode): 1}
    edges = (256, 5120, (M - 1) // 256 * 256)
    p.run(L, name(0), edges)
    p.run(L, name(0), edges, bias=True, relu=True, drop=True)
    p.run(L, name(EPI_GATE), edges, gate=True)
    p.run(L, name(EPI_RES), edges, bias=True, drop=True, res=True)


# The residual joins BEFORE the one rounding.  With operands in [-2, 2] the value before the residual is an integer, exact in
# bf16 up to 256, so only a long contraction shows a second rounding: K = 4096 puts a fifth of the cells past 256 (sigma 128).
# With a bias, so that the residual stays in the epilogue (not streamed as K stages).  4104 % 32 != 0: the fallback.
ONCE = [(129, 128, 4096, ASYNC % (64, 128, EPI_RES)), (129, 192, 4096, ASYNC % (64, 64, EPI_RES)),
        (8065, 1024, 4096, ASYNC % (128, 128, EPI_RES)), (129, 72, 4104, REG % (64, EPI_RES)), (129, 520, 4104, REG % (128, EPI_RES)),
        (10753, 3072, 4096, BIG % EPI_RES)]


@pytest.mark.parametrize("M,N_,K,name", ONCE, ids=[f"M{c[0]}-N{c[1]}-K{c[2]}" for c in ONCE])
def test_residual_is_added_before_the_one_rounding(L, M, N_, K, name):
    p = NT(M, N_, K, seed=12)
    assert (p.acc.abs() > 256).float().mean().item() > 0.02
    p.run(L, {name: 1}, bias=True, res=True)


@pytest.mark.parametrize("which", ["A", "B", "C", "gate", "residual", "pe"])
def test_refuses_pointers_off_16_bytes(L, which):
    """Every kernel of the family, the register-staged one included, moves 16-byte vectors: a pointer 8 bytes off is refused
    (it used to select the register-staged kernel, whose loads are 16-byte vectors too).  Nothing is launched or written."""
    p = NT(65, 64, 64, emb=(4, 5, 1) if which == "pe" else None, seed=11)
    e, _ = p.epilogue(bias=True, gate=which == "gate", res=which == "residual")
    kw = {}
    if which == "A":
        kw["A"] = p.A.data_ptr() + 8
    elif which == "B":
        kw["B"] = p.B.data_ptr() + 8
    elif which == "C":
        kw["Cp"] = p.out.ptr() + 8
    else:
        setattr(e, which, getattr(e, which) + 8)
    rc, rec = p.launch(L, e, **kw)
    assert rc == IQ_ERR_ARG and rec == {}, f"rc {rc}, launched {rec}"
    assert p.out.untouched()
    rc, rec = p.launch(L, p.epilogue(bias=True, gate=which == "gate", res=which == "residual")[0])
    assert rc == IQ_OK and len(rec) == 1


# ------------------------------------------------------------------------------------------------
# iq_gemm_bf16_ln
# ------------------------------------------------------------------------------------------------
def ln_case(L, M, D, K, want, drop, lda=None, lead_a=0, edges=(), seed=20):
    """Z exactly; X, mean, rstd against fp64 taken from the exact Z."""
    GR.assert_exact(K, pe=False, gate=False)
    g = gen(seed, M, D, K)
    lda = lda or K + 64                                   # the band kernel wants lda % 64 == 0 and a 128-byte aligned base
    A = ints(g, M, K, lda, GR.AMP_A, lead_a)
    W = ints(g, D, K, K + 64, GR.AMP_B)
    R = ints(g, M, D, D + 8, GR.AMP_E)
    bias = ints_f32(g, D)
    gamma = fenced(torch.rand(D, device=dev(), generator=g) + 0.5)
    beta = fenced(torch.randn(D, device=dev(), generator=g))
    Z, X = Out(M, D, D), Out(M, D, D)
    mean, rstd = Fenced(M), Fenced(M)
    d = drop_site(drop)
    what = f"gemm_ln M={M} D={D} K={K} drop={drop} lda={lda} lead={lead_a}"
    rc = []
    rec = kernel_launches(L, lambda: rc.append(L.iq_gemm_bf16_ln(
        A.data_ptr(), lda, W.data_ptr(), K + 64, bias.ptr(), R.data_ptr(), D + 8, C.byref(d) if drop else None, gamma.ptr(),
        beta.ptr(), GR_EPS, Z.ptr(), X.ptr(), mean.ptr(), rstd.ptr(), M, D, K, stream())))
    torch.cuda.synchronize()
    assert rc[0] == IQ_OK, f"{what}: rc {rc[0]}"
    assert rec == want, f"{what}: launched {rec}, expected {want}"
    rows = torch.arange(M, device=dev())
    acc = A.double() @ W.double().t()
    kw = dict(bias=bias.body, residual=R)
    got = Z.gather(rows)
    if drop:
        band = mask_rows(M, edges) if M * D > FEW_MILLION else None
        expect = with_mask(got, GR.stored(acc, keep=TRUE(), **kw), GR.stored(acc, keep=FALSE(), **kw), rows, D, band)
    else:
        expect = GR.stored(acc, **kw)
    msg = Z.compare(rows, expect)
    if msg is not None:
        if not torch.equal(got.view(torch.int16), expect.view(torch.int16)):
            def epi_box(rs, cs, a):
                keep = GR.keep_rows(rows[rs], D)[:, cs] if drop else None
                return GR.stored(a, bias=bias.body[cs], keep=keep, residual=R[rs, cs])
            msg += GR.explain(A, W, got, expect, epi_box)
        raise AssertionError(f"{what} {rec} Z: {msg}")
    for f, name in ((mean, "mean"), (rstd, "rstd"), (bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        assert bool(f.fences().all()), f"{what}: sentinels around {name} overwritten"
    zb = expect.double()
    mu = zb.mean(-1, keepdim=True)
    var = zb.var(-1, unbiased=False, keepdim=True)
    ref = gamma.body.double() * ((zb - mu) / torch.sqrt(var + GR_EPS)) + beta.body.double()
    xg = X.gather(rows)
    assert X.compare(rows, xg) is None, f"{what}: X written outside its rows"
    err = (xg.double() - ref).abs()
    bad = ~(err <= 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ref.abs().max())              # a NaN is wrong
    assert not bad.any(), f"{what} X: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"
    assert not mean.body.isnan().any() and not rstd.body.isnan().any(), f"{what}: a statistic nobody wrote"
    close_f32(mean.body, mu.squeeze(-1), what + " mean", 1e-5)
    close_f32(rstd.body, (1 / torch.sqrt(var + GR_EPS)).squeeze(-1), what + " rstd", 1e-5)


GR_EPS = 1e-12


# Row block 64 when D == 256 or ceil(M / 128) <= 320 (M <= 40,960), else 128.
@pytest.mark.parametrize("K", [64, 96, 128, 1024])
@pytest.mark.parametrize("D", [128, 192, 256])
def test_gemm_ln_whole_row_tiles(L, D, K):
    """K / 32 = 2 (nothing but the two peeled stages), 3, 4, 32 stages."""
    for M in (1, 63, 64, 65, 129, 1000):
        for drop in (False, True):
            ln_case(L, M, D, K, {LN % (64, D): 1}, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
def test_gemm_ln_128_row_blocks_above_320_blocks(L, drop):
    ln_case(L, 40961, 128, 64, {LN % (128, 128): 1}, drop, edges=(128, 40960))


# band_workgroups: D == 192, K % 64 == 0, K >= 512, nwg = 256 * ceil(M / 65,536) workgroups of floor(M / nwg) > 192 and
# ceil(M / nwg) <= 256 rows: 49,408 <= M <= 65,536; lda % 64 == 0, ldw % 64 == 0, A and W 128-byte aligned.  Otherwise
# gemm_ln_kernel<128, 192> (these M are past 40,960).  49,408: every band 193 rows = 13 row groups (4 / 3 / 3 / 3, the last
# holds one row); 49,409: one band of 194; 53,837 = 210.3 per band: 14 groups; 58,881 = 230.0: 15; 65,535: 255 and 256 rows.
BAND_M = [(49407, False), (49408, True), (49409, True), (53837, True), (58881, True), (65535, True), (65536, True), (65537, False)]


def band_edges(M):
    return tuple(b * M // 256 for b in (1, 100, 255))


@pytest.mark.parametrize("M,band", BAND_M, ids=[f"M{m}" for m, _ in BAND_M])
@pytest.mark.parametrize("K", [512, 576, 768])
def test_gemm_ln_band_kernel_window(L, K, M, band):
    """8, 9 and 12 K-tiles of 64 (an odd count ends on the other operand set)."""
    for drop in (False, True):
        ln_case(L, M, 192, K, {LN_BAND if band else LN % (128, 192): 1}, drop, edges=band_edges(M))


@pytest.mark.parametrize("how", ["lda", "base", "K448", "eligible"])
def test_gemm_ln_band_kernel_preconditions(L, how):
    kw = {"lda": dict(lda=512 + 8), "base": dict(lead_a=32), "K448": {}, "eligible": {}}[how]      # base: 64 bytes off
    K = 448 if how == "K448" else 512
    ln_case(L, 49408, 192, K, {LN_BAND if how == "eligible" else LN % (128, 192): 1}, True, edges=band_edges(49408), seed=21, **kw)


# ------------------------------------------------------------------------------------------------
# iq_gemm_bf16_lnbwd
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def lnbwd_device_operands(D, K):
    return tuple(t.to(dev()) for t in GR.lnbwd_operands(D, K))


def lnbwd_case(L, M, D, K, drop=True):
    full = lnbwd_device_operands(D, K)
    A, R, z = nan_view(M, K, K + 8), nan_view(M, D, D + 8), nan_view(M, D, D)
    Wt = nan_view(D, K, K + 8)
    for v, src in ((A, full[0][:M]), (Wt, full[1]), (R, full[2][:M]), (z, full[3][:M])):
        v.copy_(src)
    gamma = fenced(full[4])
    zf = z.double()
    mean = fenced(zf.mean(-1).float())
    rstd = fenced((1 / torch.sqrt(zf.var(-1, unbiased=False) + GR_EPS)).float())
    dX = A.double() @ Wt.double().t() + R.double()
    assert dX.abs().max().item() < GR.DX_LIMIT, "the amplitude condition of the reference"
    block = 64 if (M + 127) // 128 <= 320 else 128                     # lnbwd_block_rows
    nrows = (M + block - 1) // block
    assert L.iq_gemm_lnbwd_partial_rows(M) == nrows
    part = Fenced(nrows * 2 * D)
    dz, dy = Out(M, D, D), Out(M, D, D)
    d = drop_site(drop)
    what = f"gemm_lnbwd M={M} D={D} K={K} drop={drop}"
    rc = []
    rec = kernel_launches(L, lambda: rc.append(L.iq_gemm_bf16_lnbwd(
        A.data_ptr(), K + 8, Wt.data_ptr(), K + 8, R.data_ptr(), D + 8, z.data_ptr(), mean.ptr(), rstd.ptr(), gamma.ptr(),
        C.byref(d) if drop else None, dz.ptr(), dy.ptr(), part.ptr(), M, D, K, stream())))
    torch.cuda.synchronize()
    assert rc[0] == IQ_OK, f"{what}: rc {rc[0]}"
    assert rec == {LNBWD % (block, D): 1}, f"{what}: launched {rec}"
    for f, name in ((part, "partial"), (mean, "mean"), (rstd, "rstd"), (gamma, "gamma")):
        assert bool(f.fences().all()), f"{what}: sentinels around {name} overwritten"
    rows = torch.arange(M, device=dev())
    band = mask_rows(M, (block, M // block * block)) if M * D > FEW_MILLION else None
    mrows = rows if band is None else band
    rdz, _, gmax, xhat = GR.lnbwd_reference(dX, z, mean.body, rstd.body, gamma.body)
    tol = 2.0 ** -8 * rdz.abs() + 2.0 ** -16 * gmax * rstd.body.double()[:, None]
    gz = dz.gather(rows)
    assert dz.compare(rows, gz) is None, f"{what}: dz written outside its rows"
    err = (gz.double() - rdz).abs()
    bad = ~(err <= tol)
    assert not bad.any(), f"{what} dz: {int(bad.sum())} cells off, first at {bad.nonzero()[0].tolist()}, max err {err.max().item():.4g}"
    if drop:
        gy = dy.gather(rows)
        assert dy.compare(rows, gy) is None, f"{what}: dy written outside its rows"
        keep = GR.keep_rows(mrows, D)
        rdy = torch.where(keep, rdz[mrows] * GR.DROP_SCALE, torch.zeros_like(rdz[mrows]))
        bad = ~((gy[mrows].double() - rdy).abs() <= 2.0 ** -8 * rdy.abs() + (tol - 2.0 ** -8 * rdz.abs())[mrows])
        assert not bad.any(), f"{what} dy: {int(bad.sum())} cells off the host mask, first at {bad.nonzero()[0].tolist()}"
        assert bool((gy[mrows][~keep].view(torch.int16) == 0).all()), f"{what} dy: a dropped element is not +0"
        # everywhere: exactly 0, or twice dz up to dy's own rounding
        free = ~((gy.view(torch.int16) == 0) | ((gy.double() - 2 * rdz).abs() <= 2.0 ** -7 * rdz.abs() + 2 * tol))
        assert not free.any(), f"{what} dy: {int(free.sum())} cells are neither dropped nor kept"
    else:
        assert dy.untouched(), f"{what}: dy written without a dropout site"
    p = part.body.view(nrows, 2 * D)
    pad = torch.zeros(nrows * block, D, dtype=torch.float64, device=dev())
    pad[:M] = dX
    dbeta = pad.view(nrows, block, D).sum(1)
    assert torch.equal(p[:, D:], dbeta.float()), f"{what}: dbeta partial rows differ from the column sums of dX at rows " \
        f"{(p[:, D:] != dbeta.float()).any(1).nonzero().flatten().tolist()[:8]}"
    pad[:M] = dX * xhat
    close_f32(p[:, :D], pad.view(nrows, block, D).sum(1), what + " dgamma partial rows", 1e-3)


# lnbwd_block_rows: 64 while ceil(M / 128) <= 320 (M <= 40,960: 640 partial rows), else 128 (40,961: 321 partial rows).
@pytest.mark.parametrize("K", [64, 96, 384, 1024])
@pytest.mark.parametrize("D", [128, 192])
def test_gemm_lnbwd(L, D, K):
    """K / 32 = 2, 3, 12, 32 operand stages, then D / 32 residual stages through the same ring."""
    for M in (1, 63, 64, 65, 129, 1000, 40960, 40961):
        lnbwd_case(L, M, D, K)
    lnbwd_case(L, 129, D, K, drop=False)
