"""GPU (MI355X): the weight-gradient family (csrc/gemm_wgrad.hip, csrc/gemm_wgrad_big.hip, wgrad_reduce_kernel) bit for bit,
at every launch route and at the edges of every M split.

Method.  dY holds seeded integers in [-3, 3] and X in [-2, 2], stored as bf16: every product and every partial sum is an
integer of magnitude <= 6 M, exact in fp32 in ANY summation order while 6 M < 2^24.  The reference is dY^T X and colsum(dY)
in fp64 cast to fp32, and every comparison is torch.equal: there is no tolerance.  accumulate = 1 starts from seeded integers
in [-50, 50] and must end at start + ref; accumulate = 0 over the same start must end at ref.

Surroundings.  Each operand lives inside a NaN-filled bf16 buffer: GUARD rows of the same ld before and after its M rows,
columns N..ld (K..ld) of every row NaN.  dW, dbias, the extra-segment outputs and the workspace sit between sentinel words
that are compared afterwards; the workspace is exactly iq_wgrad_grouped_ws_bytes long and NaN-filled before every launch.
A NaN in an output is a slab cell nobody wrote, or a read outside the operand.

Routes.  Every case asserts the kernels that ran and how often (prof_names.kernel_launches).  The wave tile of wgrad_pw_kernel
is not in its name; pw_tile gives 128 x 64 when N >= K and N >= 256, 64 x 128 when K > N and K >= 256, else 64 x 64: the
cases say which they mean.  The split arithmetic of the plans is NOT restated here: the M sweeps cover every residue
whatever the plan does.

On a mismatch the helper names the bounding box of the wrong (n, k) cells and looks for ONE contiguous row range of M,
aligned to 64 or 32 rows, whose contribution equals the error ("rows 4608..4671 missing").
"""
import pytest
import torch

from prof_names import kernel_launches
from test_gpu_kernels import L, _N, dev, stream  # noqa: F401  (L is a fixture)

pytestmark = pytest.mark.gpu

IQ_OK, IQ_ERR_ARG, IQ_ERR_UNSUPPORTED = 0, 1, 2
NAN = float("nan")
SENT = 0x7FC5A5A5            # sentinel word: a quiet NaN with a payload no kernel produces
FENCE = 64                   # sentinel floats on either side (256 B: the body stays 256-byte aligned)
GUARD = 64                   # NaN rows before and after an operand: one whole step of the 256-row kernel

RED = "wgrad_reduce_kernel"
PW = "wgrad_pw_kernel"
BIG = "wgrad_big_kernel<%d>"
SHARED = "wgrad_kernel<%d, 64>"


class Fenced:
    """n fp32 between two sentinel regions."""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((FENCE + n + FENCE,), SENT, dtype=torch.int32, device=dev())
        self.body = self.raw.view(torch.float32)[FENCE:FENCE + n]

    def ptr(self):
        return self.body.data_ptr()

    def fences(self):
        return torch.cat([self.raw[:FENCE], self.raw[FENCE + self.n:]]) == SENT


def int_operand(g, M, cols, ld, amp, lead=0):
    """[M, cols] view of seeded integers in [-amp, amp] inside a NaN-filled bf16 buffer of GUARD + M + GUARD rows of ld elements
    (`lead` elements in front move the base).  The view keeps the buffer alive."""
    rows = GUARD + M + GUARD
    flat = torch.full((lead + rows * ld,), NAN, dtype=torch.bfloat16, device=dev())
    v = flat[lead:].view(rows, ld)[GUARD:GUARD + M, :cols]
    v.copy_(torch.randint(-amp, amp + 1, (M, cols), device=dev(), generator=g))
    return v


def ints_f32(g, n, amp):
    return torch.randint(-amp, amp + 1, (n,), device=dev(), generator=g).float()


def explain(dY, X, got, ref):
    """Where a wrong [n, k] result is wrong, and whether one contiguous row range of M explains the error."""
    M = dY.shape[0]
    bad = ~(got == ref)                                   # a NaN is wrong
    idx = bad.nonzero()
    n0, n1, k0, k1 = (int(v) for v in (idx[:, 0].min(), idx[:, 0].max(), idx[:, 1].min(), idx[:, 1].max()))
    msg = f"{len(idx)} wrong cells ({int(got.isnan().sum())} NaN) within n {n0}..{n1}, k {k0}..{k1}"
    a0, b0 = int(idx[0, 0]), int(idx[0, 1])               # a 16 x 16 box at the first wrong cell: one tile, one cause
    ns, ks = slice(a0, min(a0 + 16, n1 + 1)), slice(b0, min(b0 + 16, k1 + 1))
    err = got[ns, ks].double() - ref[ns, ks].double()
    box = bad[ns, ks]
    if err[box].isnan().any():
        return msg + "; NaN at the first wrong cell: a slab cell nobody wrote, or a read outside the operand"
    where = f"(cells n {ns.start}..{ns.stop - 1}, k {ks.start}..{ks.stop - 1})"
    for unit in (64, 32):
        nb = (M + unit - 1) // unit
        Yb = torch.zeros(nb * unit, ns.stop - ns.start, dtype=torch.float64, device=dev())
        Xb = torch.zeros(nb * unit, ks.stop - ks.start, dtype=torch.float64, device=dev())
        Yb[:M] = dY[:, ns].double()
        Xb[:M] = X[:, ks].double()
        contrib = torch.einsum("bun,buk->bnk", Yb.view(nb, unit, -1), Xb.view(nb, unit, -1))
        P = torch.cat([torch.zeros_like(contrib[:1]), contrib.cumsum(0)])
        for a in range(nb):
            d = P[a + 1:] - P[a]                          # rows a * unit .. (a + 1 + j) * unit
            for sign, word in ((-1.0, "missing"), (1.0, "counted twice")):
                hit = ((d * sign == err) | ~box).flatten(1).all(1).nonzero()
                if len(hit):
                    b = a + 1 + int(hit[0])
                    return msg + f"; rows {a * unit}..{min(b * unit, M) - 1} {word} {where}"
    return msg + f"; no single 32- or 64-aligned row range explains it {where}"


class Call:
    """One iq_gemm_bf16_wgrad_grouped call: operands, fenced outputs and workspace, references.

    shapes: [(N, K)]; bias: bool or one per problem; ld: [(ldy, ldx) or None] (default: 64 NaN columns after the last valid
    one, which keeps ld % 64 == 0 where N, K are multiples of 64); lead_y: elements in front of the first problem's dY;
    extras: [(rows, n, row_stride, column offset in the partial rows)]."""

    def __init__(self, L, M, shapes, bias=True, ld=None, budget=0, extras=(), lead_y=0, seed=0):
        N = _N()
        assert 6 * M < 2 ** 24, "partial sums must stay exact in fp32 in any order"
        self.L, self.M, self.budget, self.shapes = L, M, budget, shapes
        g = torch.Generator(device="cuda").manual_seed(1000003 * seed + M)
        self.nprob, self.nextra = len(shapes), len(extras)
        bias = [bias] * self.nprob if isinstance(bias, bool) else list(bias)
        self.probs = (N.WgradProblem * max(self.nprob, 1))()
        self.segs = (N.ReduceSeg * max(self.nextra, 1))()
        self.outs = []                                    # (name, Fenced, start, ref [n, k], A [M, n], B [M, k] or None = ones)
        for i, (n, k) in enumerate(shapes):
            ldy, ldx = ld[i] if ld and ld[i] else (n + 64, k + 64)
            dY = int_operand(g, M, n, ldy, 3, lead_y if i == 0 else 0)
            X = int_operand(g, M, k, ldx, 2)
            dW = Fenced(n * k)
            assert dW.ptr() % 16 == 0
            self.outs.append((f"dW[{i}] {n}x{k}", dW, ints_f32(g, n * k, 50), (dY.double().t() @ X.double()).float(), dY, X))
            p = self.probs[i]
            p.dY, p.ldy, p.X, p.ldx, p.dW, p.dbias, p.N, p.K = dY.data_ptr(), ldy, X.data_ptr(), ldx, dW.ptr(), None, n, k
            if bias[i]:
                db = Fenced(n)
                self.outs.append((f"dbias[{i}] {n}", db, ints_f32(g, n, 50), dY.double().sum(0).float().unsqueeze(1), dY, None))
                p.dbias = db.ptr()
        for j, (rows, n, stride, off) in enumerate(extras):
            buf = torch.full((rows * stride,), NAN, device=dev())
            v = buf.view(rows, stride)[:, off:off + n]
            v.copy_(torch.randint(-8, 9, (rows, n), device=dev(), generator=g))
            out = Fenced(n)
            self.outs.append((f"extra[{j}] rows {rows} n {n} stride {stride}", out, ints_f32(g, n, 50),
                              v.double().sum(0).float().unsqueeze(1), v, None))
            s = self.segs[j]
            s.partials, s.rows, s.row_stride, s.out, s.n = v.data_ptr(), rows, stride, out.ptr(), n
        self.nbytes = L.iq_wgrad_grouped_ws_bytes(self.probs, self.nprob, M, budget) if self.nprob else 0
        assert self.nbytes % 4 == 0
        self.ws = Fenced(self.nbytes // 4) if self.nbytes else None

    def launch(self, accumulate, ws_bytes=None, nextra=None):
        """-> (return code, {kernel: launches}); outputs reset to their start values, workspace NaN-filled first."""
        for _, f, start, _, _, _ in self.outs:
            f.body.copy_(start)
        if self.ws:
            self.ws.body.fill_(NAN)
        nextra = self.nextra if nextra is None else nextra
        rc = []
        rec = kernel_launches(self.L, lambda: rc.append(self.L.iq_gemm_bf16_wgrad_grouped(
            self.probs if self.nprob else None, self.nprob, self.M, self.ws.ptr() if self.ws else None,
            self.nbytes if ws_bytes is None else ws_bytes, accumulate, self.budget, self.segs if nextra else None, nextra,
            stream())))
        return rc[0], rec

    def fences_intact(self):
        bad = [o[0] for o in self.outs if not bool(o[1].fences().all())]
        if self.ws and not bool(self.ws.fences().all()):
            bad.append("workspace")
        assert not bad, f"sentinels overwritten around: {bad}"

    def untouched(self):
        for name, f, start, _, _, _ in self.outs:
            assert torch.equal(f.body, start), f"{name} was written by a refused call"
        self.fences_intact()

    def exact(self, accumulate, what):
        for name, f, start, ref, A, B in self.outs:
            base = start.view_as(ref) if accumulate else torch.zeros_like(ref)
            got = f.body.view_as(ref)
            if not torch.equal(got, base + ref):
                B = torch.ones(A.shape[0], 1, device=dev()) if B is None else B      # a column sum
                raise AssertionError(f"{what} accumulate={accumulate} {name}: " + explain(A, B, got - base, ref))
        self.fences_intact()


def run(L, M, shapes, want, **kw):
    """Both accumulate modes of one call: return code, kernels launched, exact outputs, sentinels."""
    c = Call(L, M, shapes, **kw)
    what = f"M={M} {shapes} {kw}"
    for accumulate in (0, 1):
        rc, rec = c.launch(accumulate)
        assert rc == IQ_OK, f"{what}: rc {rc}"
        assert rec == want, f"{what}: launched {rec}, expected {want}"
        c.exact(accumulate, what)
    print(f"{what}: {want}")


# ------------------------------------------------------------------------------------------------
# 1. 256-row kernel, one problem
# ------------------------------------------------------------------------------------------------
# M = 4096 + 64 j, j = 0..16.  For the reader only -- 64-row steps of the LAST split under today's wgrad_big_plan:
#   j      0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
#   steps  8  2  3  4  5  6  7  8  8  1  2  3  4  5  6  7  8     (8 splits of 8 or 9 steps, 9 of 8 or 9, 10 of 8)
# Seventeen consecutive step counts cover every residue of the step pipeline whatever the plan becomes.
BIG_ONE = [
    # (N, K), column tile, bias          orientation, n' tile, bias side
    ((128, 128), 128, True),           # as is, one 128-row n' tile, A side
    ((320, 128), 128, True),           # as is, two n' tiles, the second holds 64 rows
    ((192, 64), 192, True),            # transposed, 64-row n' tile, B side at CT = 3
    ((64, 256), 256, True),            # as is, 64-row n' tile
    ((256, 320), 256, True),           # transposed, n' = 320 = 256 + 64 rows, B side at CT = 4
    ((128, 128), 128, False),
    ((256, 320), 256, False),
]


@pytest.mark.parametrize("shape,tk,bias", BIG_ONE, ids=[f"{s[0]}x{s[1]}-tk{t}-{'bias' if b else 'nobias'}" for s, t, b in BIG_ONE])
def test_big_kernel_one_problem_at_every_last_split_length(L, shape, tk, bias):
    for j in range(17):
        run(L, 4096 + 64 * j, [shape], {BIG % tk: 1, RED: 1}, bias=bias, seed=1)


# ------------------------------------------------------------------------------------------------
# 2. eligibility of the 256-row kernel, from the refusing side
# ------------------------------------------------------------------------------------------------
def _edge(shape, how):
    n, k = shape
    return {"M4032": (4032, {}),                                   # M < 4096
            "M4128": (4096 + 32, {}),                              # M % 64
            "ldy": (4672, {"ld": [(n + 8, k + 64)]}),              # ld % 64 (the base stays 128-byte aligned)
            "base": (4672, {"lead_y": 32}),                        # dY 64 bytes off a 128-byte boundary
            "budget": (4672, {"budget": 256}),                     # max_workgroups != 0
            "eligible": (4672, {})}[how]


@pytest.mark.parametrize("how", ["M4032", "M4128", "ldy", "base", "budget", "eligible"])
@pytest.mark.parametrize("shape,tk", [((128, 128), 128), ((192, 64), 192)], ids=["128x128", "192x64"])
def test_big_kernel_eligibility_boundary(L, shape, tk, how):
    """Every guard of wgrad_big_plan approached alone: the refused call runs the wave-private kernel (64 x 64 tiles at
    both shapes) and is exact; the untouched one runs the 256-row kernel."""
    M, kw = _edge(shape, how)
    c = Call(L, M, [shape], seed=2, **kw)
    assert c.probs[0].X % 128 == 0 and c.probs[0].ldx % 64 == 0
    assert (c.probs[0].dY % 128 == 0) == (how != "base")
    assert (c.probs[0].ldy % 64 == 0) == (how != "ldy")
    del c
    want = {BIG % tk: 1, RED: 1} if how == "eligible" else {PW: 1, RED: 1}
    run(L, M, [shape], want, seed=2, **kw)


# ------------------------------------------------------------------------------------------------
# 3. 256-row kernel, layer groups of four with the LayerNorm segments: the reduce launch the model issues per layer
# ------------------------------------------------------------------------------------------------
def layer_group(D, F):
    return [(D, F), (F, D), (D, D), (3 * D, D)]           # ffn.linear2, ffn.linear1, attention.w_concat, w_q|w_k|w_v


def layer_ld(D, F):
    return [None, None, None, (3 * D, D + 64)]            # the q,k,v gradient is dense: ldy = 3 D, as the model passes it


def ln_extras(D):
    # two tall blocks (rows >= 64), two wide ones; row_stride 2 D, the second of each pair at column D (gamma | beta rows);
    # n = D - 2 reaches the n % 4 tail
    return [(73, D, 2 * D, 0), (300, D - 2, 2 * D, D), (1, D, 2 * D, 0), (37, D, 2 * D, D)]


@pytest.mark.parametrize("nobias", [None, 1], ids=["12seg", "11seg-one-without-bias"])
@pytest.mark.parametrize("M", [4160, 4672])
@pytest.mark.parametrize("D,F,tk", [(192, 768, 192), (128, 512, 128), (256, 512, 256)])
def test_big_kernel_layer_group_with_layernorm_segments(L, D, F, tk, M, nobias):
    """One partial-tile launch and ONE reduce launch carrying 4 dW + 4 (3) dbias + 4 LayerNorm segments: 12 is the size
    of RedGroup."""
    run(L, M, layer_group(D, F), {BIG % tk: 1, RED: 1}, bias=[i != nobias for i in range(4)], ld=layer_ld(D, F),
        extras=ln_extras(D), seed=3)


# ------------------------------------------------------------------------------------------------
# 4. wave-private kernel
# ------------------------------------------------------------------------------------------------
# every residue of the 32-row stage and of the 4-wave round; one, two and three splits; splits whose last has a single row
PW_M = [1, 8, 31, 32, 33, 97, 127, 128, 129, 255, 256, 257, 385, 513, 645]
PW_ONE = [(64, 64),        # 64 x 64
          (256, 64),       # 128 x 64
          (64, 256),       # 64 x 128
          (72, 40),        # 64 x 64, ragged in n and k
          (264, 72),       # 128 x 64, ragged in n and k
          (72, 264)]       # 64 x 128, ragged in n and k


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", PW_ONE, ids=[f"{n}x{k}" for n, k in PW_ONE])
def test_pw_kernel_one_problem_at_every_stage_and_round_residue(L, shape, bias):
    for M in PW_M:
        run(L, M, [shape], {PW: 1, RED: 1}, bias=bias, seed=4)


PW_GROUPS = {"three-tiles": ([(256, 64), (64, 256), (72, 40)], [129, 645]),        # 128 x 64, 64 x 128, 64 x 64
             "vit-tiny-layer": (layer_group(192, 768), [394])}                      # 64 x 128, 128 x 64, 64 x 64, 128 x 64


@pytest.mark.parametrize("with_extras", [False, True], ids=["plain", "extras"])
@pytest.mark.parametrize("budget", [0, 40, 256])          # 40 < the ViT-Tiny group's 60 tiles: one split; 256: overlapped backward
@pytest.mark.parametrize("group", list(PW_GROUPS))
def test_pw_kernel_groups_mixing_tile_shapes(L, group, budget, with_extras):
    shapes, Ms = PW_GROUPS[group]
    for M in Ms:
        run(L, M, shapes, {PW: 1, RED: 1}, bias=[i != 1 for i in range(len(shapes))], budget=budget,
            extras=ln_extras(64)[1:3] if with_extras else (), seed=5)


# ------------------------------------------------------------------------------------------------
# 5. shared-tile kernel (N K > 512 Ki)
# ------------------------------------------------------------------------------------------------
SHARED_ONE = [((1664, 320), 64, [1, 63, 64, 65, 300, 1000]),   # K % 128 != 0, K <= 512: wgrad_kernel<64, 64>
              ((2048, 264), 64, [333]),                        # ragged k tile at TK = 64
              ((1032, 520), 128, [130])]                       # <128, 64> through K > 512, ragged in n and k


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape,tk,Ms", SHARED_ONE, ids=[f"{s[0]}x{s[1]}" for s, _, _ in SHARED_ONE])
def test_shared_tile_kernel(L, shape, tk, Ms, bias):
    for M in Ms:
        run(L, M, [shape], {SHARED % tk: 1, RED: 1}, bias=bias, seed=6)


def test_mixed_group_falls_back_to_one_launch_per_problem_and_reduces_the_extras_alone(L):
    run(L, 300, [(64, 64), (1664, 320), (72, 64)], {PW: 2, SHARED % 64: 1, RED: 4}, extras=ln_extras(64)[1:3], seed=7)


# ------------------------------------------------------------------------------------------------
# 6. the reduce alone (nprob = 0)
# ------------------------------------------------------------------------------------------------
RED_ROWS = [1, 3, 4, 5, 63, 64, 65, 300, 512]
RED_N = [4, 190, 192, 256, 260, 1048]


@pytest.mark.parametrize("n", RED_N)
def test_reduce_alone(L, n):
    """rows on either side of the wide / tall block threshold (64) and of the 4- and 16-slice rounds, n with and without
    the n % 4 tail, dense and strided partial rows, one to four segments per launch (the others rotate through the lists)."""
    c = 0
    for rows in RED_ROWS:
        for wide in (1, 2):
            segs = []
            for j in range(1 + c % 4):
                nj = RED_N[(RED_N.index(n) + j) % len(RED_N)]
                segs.append((RED_ROWS[(RED_ROWS.index(rows) + 2 * j) % len(RED_ROWS)], nj, (wide * nj + 3) // 4 * 4, 0))
            run(L, 1, [], {RED: 1}, extras=segs, seed=8 + c)
            c += 1


# ------------------------------------------------------------------------------------------------
# 7. refusals: nothing is launched, nothing is written
# ------------------------------------------------------------------------------------------------
def _refused(c, want_rc, **kw):
    rc, rec = c.launch(0, **kw)
    assert rc == want_rc and rec == {}, f"rc {rc}, launched {rec}"
    c.untouched()


@pytest.mark.parametrize("field,delta", [("N", -4), ("K", -4), ("ldy", 4), ("ldx", 4)])
def test_refuses_sizes_that_are_no_multiple_of_8(L, field, delta):
    c = Call(L, 200, [(64, 64)], extras=[(5, 64, 64, 0)], seed=9)
    setattr(c.probs[0], field, getattr(c.probs[0], field) + delta)
    _refused(c, IQ_ERR_UNSUPPORTED)


@pytest.mark.parametrize("what", ["dW", "nextra", "stride_lt_n", "stride_mod_4", "partials", "ws"])
def test_refuses_bad_arguments(L, what):
    N = _N()
    c = Call(L, 200, [(64, 64)], extras=[(5, 64, 64, 0)], seed=9)
    kw = {}
    if what == "dW":
        c.probs[0].dW += 4
    elif what == "nextra":
        five = (N.ReduceSeg * 5)()
        for j in range(5):
            for name, _ in N.ReduceSeg._fields_:
                setattr(five[j], name, getattr(c.segs[0], name))
        c.segs, kw = five, {"nextra": 5}
    elif what == "stride_lt_n":
        c.segs[0].row_stride = 60
    elif what == "stride_mod_4":
        c.segs[0].n, c.segs[0].row_stride = 60, 62
    elif what == "partials":
        c.segs[0].partials += 4
    else:
        kw = {"ws_bytes": c.nbytes - 1}
    _refused(c, IQ_ERR_ARG, **kw)


def test_empty_call_is_ok_and_launches_nothing(L):
    rc = []
    rec = kernel_launches(L, lambda: rc.append(L.iq_gemm_bf16_wgrad_grouped(None, 0, 64, None, 0, 0, 0, None, 0, stream())))
    assert rc == [IQ_OK] and rec == {}
