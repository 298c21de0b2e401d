"""GPU (MI355X): the stand-alone LayerNorm kernels (csrc/layernorm.hip) bit for bit, at every one of the 24 (LPR, NV, masked)
instances, every supported width and every row edge: iq_ln_fwd, iq_ln_bwd with dropout off and on, reducing on its own
(accumulate 0 and 1) and in partial-rows mode (dgamma == dbeta == NULL, the rows model.hip hands to iq_reduce_seg_t).

Method.  tests/ln_exact_ref.py builds operands on which every fp32 value a kernel holds is exact in ANY summation order:
z = m_r + s_r sign with as many +1 as -1, so mean = m_r, rstd = 1 / s_r, xhat = +-1 and X = gamma sign + beta; dX = g / gamma with
g = 4 k1 + sign (4 k2 + u), so c1 = 4 k1, c2 = 4 k2 and dZ = sign u / s_r; dropout p = 0.5, scale exactly 2, dy = 2 dZ or +0 by the host
mask; dbeta, dgamma and every partial row are integers below 2^24.  X, dZ, dy, mean, rstd, the partial rows, dgamma and dbeta are
compared with torch.equal on int16 / fp32 values; tests/test_ln_exact_ref_cpu.py confirms the conditions for these very numbers
in the kernel's fp32 expressions and that every wrong kernel of ln_exact_ref.VARIANTS would be told apart.
Real operands carry the bounds tests/test_gpu_gemm_exact.py and tests/test_gpu_chain_exact.py apply to the same quantities:
X within 2^-8 |ref| + 2^-16 max|ref| of fp64, dZ / dy within 2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd, mean / rstd 1e-5 and
dgamma / dbeta 1e-3 of the scale, a dropped dy element +0 by the host mask, at p = 0.1 and 0.25, eps = 1e-12 and 1e-5.

Surroundings.  z and dX sit between GUARD rows of NaN; gamma, beta, mean, rstd, dgamma, dbeta are fp32 between sentinel words; X,
dZ, dy are `Out` buffers prefilled with PAT and compared WHOLE; ws is the full iq_ln_bwd_ws_bytes(D) between sentinels, prefilled
with NaN: after a launch exactly its first partial_rows * 2 D floats are finite.  A NaN in a result is a read outside an operand.

Rows.  Every width of ln_exact_ref.WIDTHS (one per instance, 27) meets M = 1, both sides of a wave (RPW - 1, RPW) and of a
workgroup (RPB - 1, RPB, RPB + 1), 2 RPB + 1 and both sides of the backward's grid-stride loop (512 RPB, 512 RPB + 1); the four
backward settings (dropout x reduce / partial rows, accumulate) rotate over these.  The forward's loop (4096 RPB, 4096 RPB + 1)
is met once per rows-per-workgroup class at its narrowest width.  Every multiple of 8 up to 2048 runs once with 5 rows of the
centred recipe (ln_exact_ref.exact_case explains why that one is exact at the 38 widths where var misses s^2 by an ulp).
Every launch asserts {kernel name: 1} with <LPR, NV, masked> / <LPR, NV, dropout, masked>; a second launch gives the same bits.
The measured worst case of every tolerance, in units of its bound, is printed by test_zz_report (profiles/ln_exact.txt).
"""
import ctypes as C
import time

import pytest
import torch

import ln_exact_ref as LR
from prof_names import kernel_launches
from test_gpu_gemm_exact import FEW_MILLION, PAT, Out, fenced, mask_rows, nan_view
from test_gpu_kernels import L, _N, dev, stream  # noqa: F401  (L is a fixture)
from test_gpu_wgrad_exact import NAN, Fenced

pytestmark = pytest.mark.gpu

IQ_OK, IQ_ERR_ARG, IQ_ERR_UNSUPPORTED = 0, 1, 2
EPS = 1e-12
REPORT = {}                  # tolerance -> (worst observed / bound, case)
INSTANCES = {}               # kernel name -> (M, D) cases that launched it
CLOCK = {"t0": time.time()}
FWD_ARGS = ["z", "gamma", "beta", "X", "mean", "rstd"]
BWD_ARGS = ["dX", "z", "mean", "rstd", "gamma_b", "dZ", "dy", "drop", "dgamma", "dbeta", "ws"]
# the backward settings that rotate over the row edges: (dropout, reduce now, accumulate)
SETTINGS = [(False, True, 0), (True, False, 0), (True, True, 1), (False, False, 0)]


def note(name, ratio, what):
    ratio = float(ratio)
    if ratio > REPORT.get(name, (-1.0, ""))[0]:
        REPORT[name] = (ratio, what)


def ptr_of(v):
    if isinstance(v, (Out, Fenced)):
        return v.ptr()
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def site(p):
    d = _N().Dropout()
    d.seed, d.step, d.site, d.p, d.step_dev = LR.SEED, LR.STEP, LR.SITE, p, None
    return d


def op(values):
    """A contiguous bf16 operand between GUARD rows of NaN."""
    v = nan_view(values.shape[0], values.shape[1], values.shape[1])
    v.copy_(values)
    return v


def nan_f(n):
    f = Fenced(n)
    f.body.fill_(NAN)
    return f


def ints_f(n, k):
    """n fenced fp32 integers that differ from place to place (what accumulate = 1 starts from)."""
    return fenced(((torch.arange(n, device=dev()) * k) % 23 - 11).float())


def fwd(L, b, M, D, eps=EPS, **ov):
    args = [ptr_of(ov[k] if k in ov else b[k]) for k in FWD_ARGS]
    rc = []
    rec = kernel_launches(L, lambda: rc.append(L.iq_ln_fwd(*args, M, D, eps, stream())))
    torch.cuda.synchronize()
    return rc[0], rec


def bwd(L, b, M, D, accumulate=0, **ov):
    args = []
    for k in BWD_ARGS:
        v = ov[k] if k in ov else b.get(k)
        args.append((C.byref(v) if v is not None else None) if k == "drop" else ptr_of(v))
    rc = []
    rec = kernel_launches(L, lambda: rc.append(L.iq_ln_bwd(*args, accumulate, M, D, stream())))
    torch.cuda.synchronize()
    return rc[0], rec


def buffers(M, D, z, dX, gamma, beta, gamma_b):
    """Every operand and output of a forward + backward on value tensors z, dX [M, D] (any float type)."""
    return dict(z=op(z), dX=op(dX), gamma=fenced(gamma.float()), beta=fenced(beta.float()), gamma_b=fenced(gamma_b.float()),
                X=Out(M, D, D), mean=nan_f(M), rstd=nan_f(M), dZ=Out(M, D, D), dy=Out(M, D, D), ws=nan_f(LR.ws_bytes(D) // 4),
                dgamma=ints_f(D, 7), dbeta=ints_f(D, 5))


OUTS = ["X", "mean", "rstd", "dZ", "dy", "ws", "dgamma", "dbeta"]


def fences_ok(b, what):
    for k, v in b.items():
        if isinstance(v, Fenced):
            assert bool(v.fences().all()), f"{what}: sentinels around {k} overwritten"


def bits(b, names):
    return {k: (b[k].flat if isinstance(b[k], Out) else b[k].raw).clone() for k in names}


def exact(out, want, what, why=None):
    """out (an Out) holds `want` in its rows and PAT everywhere else -- or the message says what it holds instead."""
    rows = torch.arange(out.rows, device=dev())
    msg = out.compare(rows, want)
    if msg is None:
        return
    got = out.gather(rows)
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    if len(bad):
        r, c = bad[0].tolist()
        msg += (f"{len(bad)} wrong cells ({int(got.isnan().sum())} NaN) within rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, cols "
                f"{int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first [{r}, {c}] = {got[r, c].item()} for {want[r, c].item()}")
        if why is not None and got.numel() <= 1 << 20:
            msg += why(got)
    raise AssertionError(f"{what}: {msg}")


def same_f32(f, want, what):
    """A fenced fp32 vector holds exactly `want` (fp64 values an fp32 holds)."""
    w = want.float()
    if not torch.equal(f.body, w):
        bad = (f.body != w).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} values differ ({int(f.body.isnan().sum())} NaN), first at {i}: "
                             f"{f.body[i].item()!r} for {w[i].item()!r}")


def which(got, alts):
    for name, make in alts.items():
        try:
            alt = make()
        except Exception:                      # (a diagnostic must not hide the mismatch it explains)
            continue
        if torch.equal(alt.float().to(torch.bfloat16).view(torch.int16), got.view(torch.int16)):
            return f"; the output is what it would be if {LR.VARIANTS[name]}"
    return ""


# ------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------
class Exact:
    """One exact problem of M rows at width D: its host statement on the device and its buffers."""

    def __init__(self, M, D, zero_rows=(), centred=False):
        self.M, self.D, self.zero_rows = M, D, zero_rows
        self.rows = torch.arange(M, device=dev())
        self.c = LR.exact_case(self.rows, D, zero_rows, centred)
        c = self.c
        self.gamma = LR.fwd_gamma(D, dev())
        self.beta = (LR.allwidths_beta if centred else LR.fwd_beta)(D, dev())
        self.gamma_b = LR.bwd_gamma(D, dev())
        self.b = buffers(M, D, c["z"], c["dX"], self.gamma, self.beta, self.gamma_b)
        self.what = f"M={M} D={D} {LR.instance(D)}"
        self.alive = torch.ones(M, dtype=torch.bool, device=dev())
        for r in zero_rows:
            self.alive[r] = False

    def _but_dead_rows(self, want, got):
        """`want` with the all-zero rows taken from the output (they are only required to be finite)."""
        if not self.zero_rows:
            return want
        want = want.clone()
        want[~self.alive] = got[~self.alive]
        return want

    def forward(self, L):
        M, D, b, c = self.M, self.D, self.b, self.c
        what = "ln_fwd " + self.what
        rc, rec = fwd(L, b, M, D)
        assert rc == IQ_OK, f"{what}: rc {rc}"
        assert rec == {LR.fwd_name(D): 1}, f"{what}: launched {rec}, expected {LR.fwd_name(D)}"
        INSTANCES.setdefault(LR.fwd_name(D), set()).add((M, D))
        fences_ok(b, what)
        same_f32(b["mean"], c["mean"], what + " mean")
        if self.zero_rows:
            assert bool(torch.isfinite(b["rstd"].body).all()), f"{what}: rstd of an all-zero row is not finite"
        same_f32(b["rstd"], self._but_dead_rows(c["rstd"], b["rstd"].body.double()), what + " rstd")

        def why(got):
            z = b["z"]
            return which(got, {v: (lambda v=v: LR.forward64(z, self.gamma, self.beta, EPS, v)[0])
                               for v in ("var_dm1", "wide_reduce", "transposed_gamma", "tail_in_var")})
        exact(b["X"], c["X"].to(torch.bfloat16), what + " X", why)

    def backward(self, L, drop, reduce_now, accumulate):
        """On the mean / rstd the forward left in the buffers (compared there)."""
        M, D, b, c = self.M, self.D, self.b, self.c
        what = f"ln_bwd {self.what} drop={drop} reduce={reduce_now} accumulate={accumulate}"
        b["drop"] = site(LR.P) if drop else None
        before = torch.cat([b["dgamma"].body, b["dbeta"].body]).double()
        ov = {} if reduce_now else dict(dgamma=None, dbeta=None)
        rc, rec = bwd(L, b, M, D, accumulate, **ov)
        assert rc == IQ_OK, f"{what}: rc {rc}"
        assert rec == {LR.bwd_name(D, drop): 1}, f"{what}: launched {rec}, expected {LR.bwd_name(D, drop)}"
        INSTANCES.setdefault(LR.bwd_name(D, drop), set()).add((M, D))
        fences_ok(b, what)
        assert L.iq_ln_bwd_partial_rows(M, D) == LR.partial_rows(M, D) and L.iq_ln_bwd_ws_bytes(D) == LR.ws_bytes(D)
        gz = b["dZ"].gather(self.rows)
        if self.zero_rows:
            assert bool(torch.isfinite(gz.float()).all()), f"{what}: dZ of an all-zero row is not finite"
        dz = self._but_dead_rows(c["dZ"].to(torch.bfloat16), gz)

        def why(got):
            return which(got, {"padded_div": lambda: LR.backward64(b["dX"], b["z"], c["mean"], c["rstd"], self.gamma_b, "padded_div")[0]})
        exact(b["dZ"], dz, what + " dZ", why)
        if drop:
            keep = LR.keep(self.rows, D)
            dy = LR.dropped(c["dZ"], keep).to(torch.bfloat16)
            gy = b["dy"].gather(self.rows)
            if self.zero_rows:
                assert bool((gy.view(torch.int16) == 0)[~self.alive][~keep[~self.alive]].all()), f"{what}: a dropped element of the all-zero row is not +0"
            dy = self._but_dead_rows(dy, gy)

            def why_y(got):
                return which(got, {"mask_no_row": lambda: LR.dropped(c["dZ"], LR.keep(self.rows, D, row_offset=False))})
            exact(b["dy"], dy, what + " dy", why_y)
        else:
            assert b["dy"].untouched(), f"{what}: dy written without a dropout site"
        # ---- the partial rows: workgroup b's row = the sums over the rows it owns; nothing behind them ----
        n = LR.partial_rows(M, D)
        ws = b["ws"].body
        assert bool(ws[n * 2 * D:].isnan().all()), f"{what}: ws written past its {n} partial rows"
        assert bool(torch.isfinite(ws[:n * 2 * D]).all()), f"{what}: a partial row nobody wrote (or a NaN read)"
        want = LR.partials(c["dX"] * c["sign"] * c["live"], c["dX"], M, D)
        got = ws[:n * 2 * D].view(n, 2 * D)
        if not torch.equal(got, want.float()):
            off = (got != want.float()).any(1).nonzero().flatten().tolist()
            hint = ""
            if torch.equal(got, LR.partials(c["dX"] * c["sign"] * c["live"], c["dX"], M, D, "last_stripe_missing").float()):
                hint = "; " + LR.VARIANTS["last_stripe_missing"]
            elif torch.equal(got[:, :D], LR.partials(c["g"] * c["sign"] * c["live"], c["dX"], M, D).float()[:, :D]):
                hint = "; " + LR.VARIANTS["dgamma_times_gamma"]
            raise AssertionError(f"{what}: partial rows differ from the host's sums at workgroups {off[:8]} of {n}{hint}")
        after = torch.cat([b["dgamma"].body, b["dbeta"].body])
        if reduce_now:
            red = LR.reduced(want, before, accumulate)
            assert red.abs().max().item() < 2 ** 24
            if not torch.equal(after, red.float()):
                hint = "; " + LR.VARIANTS["accumulate_ignored"] if torch.equal(after, LR.reduced(want, before, accumulate, "accumulate_ignored").float()) else ""
                bad = (after != red.float()).nonzero().flatten()
                raise AssertionError(f"{what}: dgamma | dbeta differ at {len(bad)} of {2 * D} places, first {int(bad[0])}{hint}")
        else:
            assert torch.equal(after.double(), before), f"{what}: dgamma / dbeta written in partial-rows mode"

    def again(self, L, names, launch, what):
        first = bits(self.b, names)
        for k in names:
            v = self.b[k]
            v.reset() if isinstance(v, Out) else v.body.fill_(NAN)
        launch()
        second = bits(self.b, names)
        for k in names:
            assert torch.equal(first[k], second[k]), f"{what}: {k} differs between two launches of the same problem"


def edge_case(L, M, D, setting):
    drop, reduce_now, accumulate = setting
    e = Exact(M, D)
    e.forward(L)
    e.again(L, ["X", "mean", "rstd"], lambda: fwd(L, e.b, M, D), "ln_fwd " + e.what)
    e.backward(L, drop, reduce_now, accumulate)
    ov = {} if reduce_now else dict(dgamma=None, dbeta=None)
    e.again(L, ["dZ", "dy", "ws"], lambda: bwd(L, e.b, M, D, accumulate, **ov), "ln_bwd " + e.what)


@pytest.mark.parametrize("D", LR.WIDTHS)
def test_every_instance_at_every_row_edge(L, D):
    i = LR.WIDTHS.index(D)
    for n, M in enumerate(LR.row_edges(D)):
        edge_case(L, M, D, SETTINGS[(i + n) % 4])


@pytest.mark.parametrize("D", [96, 1024, 136, 8])
def test_accumulate_adds_exactly_and_zero_overwrites(L, D):
    """Both over the same prefilled integers, dropout off and on."""
    M = 2 * LR.rpb(D) + 1
    e = Exact(M, D)
    e.forward(L)
    for drop in (False, True):
        for accumulate in (0, 1, 1):
            e.b["dZ"].reset(), e.b["dy"].reset(), e.b["ws"].body.fill_(NAN)
            e.backward(L, drop, True, accumulate)


@pytest.mark.parametrize("D", [96, 1024, 136, 2040, 8])
def test_all_zero_row(L, D):
    """X = beta exactly, mean = 0, rstd and dZ finite; the row adds dX to dbeta and nothing to dgamma; its neighbours are exact."""
    M = 2 * LR.rpb(D) + 1
    for zero in (1, M - 1):
        e = Exact(M, D, zero_rows=(zero,))
        assert bool((e.b["z"][zero] == 0).all())
        e.forward(L)
        assert torch.equal(e.b["X"].gather(e.rows)[zero].float(), e.beta) and e.b["mean"].body[zero].item() == 0.0
        e.backward(L, True, True, 0)


@pytest.mark.parametrize("rpb,D", sorted(LR.fwd_cap_widths().items()))
def test_forward_grid_stride_loop(L, rpb, D):
    assert LR.rpb(D) == rpb
    for M in (LR.FWD_CAP * rpb, LR.FWD_CAP * rpb + 1):
        Exact(M, D).forward(L)


def test_every_supported_width(L):
    """5 rows of the centred recipe at every multiple of 8 up to 2048: forward, backward with p = 0.5, reduce.  X, dZ, dy, dbeta
    exactly; dgamma 1e-3 of its scale (xhat = +-(1 + d) at the widths where var misses s^2 by an ulp)."""
    M = 5
    for D in range(8, LR.D_MAX + 1, 8):
        assert L.iq_ln_supported(D) == 1
        e = Exact(M, D, centred=True)
        b, c, what = e.b, e.c, f"all widths D={D}"
        rc, rec = fwd(L, b, M, D)
        assert rc == IQ_OK and rec == {LR.fwd_name(D): 1}, f"{what}: forward rc {rc}, launched {rec}"
        exact(b["X"], c["X"].to(torch.bfloat16), what + " X")
        same_f32(b["mean"], c["mean"], what + " mean")
        err = ((b["rstd"].body.double() - c["rstd"]).abs() / c["rstd"]).max().item()
        note("rstd / (1e-5 max|ref|)", err / 1e-5, what)
        assert err <= 1e-5, f"{what}: rstd off by {err:.3g}"
        b["drop"] = site(LR.P)
        rc, rec = bwd(L, b, M, D, 0)
        assert rc == IQ_OK and rec == {LR.bwd_name(D, True): 1}, (f"{what}: backward rc {rc}, launched {rec} "
                                                                  f"({LR.lds_bytes(D)} bytes of dynamic LDS)")
        fences_ok(b, what)
        exact(b["dZ"], c["dZ"].to(torch.bfloat16), what + " dZ")
        exact(b["dy"], LR.dropped(c["dZ"], LR.keep(e.rows, D)).to(torch.bfloat16), what + " dy")
        same_f32(b["dbeta"], c["dX"].sum(0), what + " dbeta")
        ref = (c["dX"] * c["sign"]).sum(0)
        err = (b["dgamma"].body.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
        note("dgamma / (1e-3 max|ref|)", err / 1e-3, what)
        assert err <= 1e-3, f"{what}: dgamma off by {err:.3g} of its scale"
        n = LR.partial_rows(M, D)
        assert bool(b["ws"].body[n * 2 * D:].isnan().all()) and bool(torch.isfinite(b["ws"].body[:n * 2 * D]).all())
        INSTANCES.setdefault(LR.fwd_name(D), set()).add((M, D))
        INSTANCES.setdefault(LR.bwd_name(D, True), set()).add((M, D))


def test_torch_mask_is_the_host_mask_on_the_device(L):
    """ln_exact_ref.keep evaluated on the device against dropout_ref.keep_groups evaluated on the host."""
    import gemm_exact_ref as GR
    rows = torch.tensor([0, 1, 5, 4096, 131072, 1048576], device=dev())
    for D, p in ((8, 0.5), (136, 0.1), (2040, 0.25)):
        assert torch.equal(LR.keep(rows, D, p=p), GR.keep_rows(rows, D, p=p))


# ------------------------------------------------------------------------------------------------
# real operands
# ------------------------------------------------------------------------------------------------
def real_case(L, M, D, p, eps, seed):
    what = f"real M={M} D={D} p={p} eps={eps}"
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = (torch.randn(M, D, device=dev(), generator=g) * 2 + 0.3).to(torch.bfloat16)
    dX = torch.randn(M, D, device=dev(), generator=g).to(torch.bfloat16)
    gamma, beta = torch.randn(D, device=dev(), generator=g), torch.randn(D, device=dev(), generator=g)
    b = buffers(M, D, z, dX, gamma, beta, gamma)
    rows = torch.arange(M, device=dev())
    rc, rec = fwd(L, b, M, D, eps)
    assert rc == IQ_OK and rec == {LR.fwd_name(D): 1}, f"{what}: forward rc {rc}, launched {rec}"
    ref, mu, rs = LR.forward64(z, gamma, beta, eps)
    xg = b["X"].gather(rows)
    assert b["X"].compare(rows, xg) is None, f"{what}: X written outside its rows"
    err, bound = (xg.double() - ref).abs(), 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ref.abs().max()
    note("X / (2^-8 |ref| + 2^-16 max|ref|)", (err / bound).max(), what)
    assert bool((err <= bound).all()), f"{what} X: {int((~(err <= bound)).sum())} cells off, max err {err.max().item():.4g}"
    for f, r, name in ((b["mean"], mu, "mean"), (b["rstd"], rs, "rstd")):
        scale = r.abs().max().item() + 1e-12
        e = (f.body.double() - r).abs().max().item()
        note(f"{name} / (1e-5 max|ref|)", e / (1e-5 * scale), what)
        assert e <= 1e-5 * scale, f"{what} {name}: max err {e:.4g} vs scale {scale:.4g}"       # (a NaN fails here too)
    b["drop"] = site(p)
    b["dgamma"].body.fill_(NAN), b["dbeta"].body.fill_(NAN)
    rc, rec = bwd(L, b, M, D, 0)
    assert rc == IQ_OK and rec == {LR.bwd_name(D, True): 1}, f"{what}: backward rc {rc}, launched {rec}"
    fences_ok(b, what)
    rdz, rg, rb, gmax = LR.backward64(dX, z, b["mean"].body, b["rstd"].body, gamma)
    floor = 2.0 ** -16 * gmax * b["rstd"].body.double()[:, None]
    tol = 2.0 ** -8 * rdz.abs() + floor
    gz = b["dZ"].gather(rows)
    assert b["dZ"].compare(rows, gz) is None, f"{what}: dZ written outside its rows"
    err = (gz.double() - rdz).abs()
    note("dZ / (2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd)", (err / tol).max(), what)
    assert bool((err <= tol).all()), f"{what} dZ: {int((~(err <= tol)).sum())} cells off, max err {err.max().item():.4g}"
    band = mask_rows(M, (LR.rpb(D),)) if M * D > FEW_MILLION else rows
    keep = LR.keep(band, D, p=p)
    gy = b["dy"].gather(rows)
    assert b["dy"].compare(rows, gy) is None, f"{what}: dy written outside its rows"
    rdy = LR.dropped(rdz[band], keep, p)
    tdy = 2.0 ** -8 * rdy.abs() + floor[band]
    ey = (gy[band].double() - rdy).abs()
    note("dy / (2^-8 |ref| + 2^-16 rowmax|dX gamma| rstd)", (ey / tdy).max(), what)
    assert bool((ey <= tdy).all()), f"{what} dy: {int((~(ey <= tdy)).sum())} cells off the host mask"
    assert bool((gy[band][~keep].view(torch.int16) == 0).all()), f"{what} dy: a dropped element is not +0"
    for f, r, name in ((b["dgamma"], rg.sum(0), "dgamma"), (b["dbeta"], rb.sum(0), "dbeta")):
        scale = r.abs().max().item() + 1e-12
        e = (f.body.double() - r).abs().max().item()
        note(f"{name} / (1e-3 max|ref|)", e / (1e-3 * scale), what)
        assert e <= 1e-3 * scale, f"{what} {name}: max err {e:.4g} vs scale {scale:.4g}"
    INSTANCES.setdefault(LR.fwd_name(D), set()).add((M, D))
    INSTANCES.setdefault(LR.bwd_name(D, True), set()).add((M, D))


@pytest.mark.parametrize("D", LR.WIDTHS)
def test_real_operands_within_the_bounds_of_the_exact_suites(L, D):
    b = LR.rpb(D)
    for n, (p, eps) in enumerate(((0.1, 1e-12), (0.25, 1e-12), (0.1, 1e-5), (0.25, 1e-5))):
        real_case(L, (37, 2 * b + 1, b + 3, 101)[n], D, p, eps, D * 10 + n)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
RM, RD = 9, 136


def untouched(b):
    for k in OUTS:
        v = b[k]
        if isinstance(v, Out):
            if not v.untouched():
                return k
        elif not bool(v.fences().all()):
            return k
    return None


def test_refusals_touch_nothing(L):
    e = Exact(RM, RD)
    b = e.b
    b["mean"].body.copy_(e.c["mean"]), b["rstd"].body.copy_(e.c["rstd"])
    b["drop"] = site(LR.P)
    snap = bits(b, OUTS)

    def refused(call, want, what, **kw):
        rc, rec = call(L, b, kw.pop("M", RM), kw.pop("D", RD), **kw)
        assert rc == want and rec == {}, f"{what}: rc {rc} (expected {want}), launched {rec}"
        assert untouched(b) is None, f"{what}: {untouched(b)} was written by a refused call"
        now = bits(b, OUTS)
        for k in OUTS:
            assert torch.equal(snap[k], now[k]), f"{what}: {k} was written by a refused call"

    for k in FWD_ARGS:
        refused(fwd, IQ_ERR_ARG, f"forward without {k}", **{k: None})
    for k in ("dX", "z", "mean", "rstd", "gamma_b", "dZ", "ws"):
        refused(bwd, IQ_ERR_ARG, f"backward without {k}", **{k: None})
    refused(bwd, IQ_ERR_ARG, "dgamma without dbeta", dbeta=None)
    refused(bwd, IQ_ERR_ARG, "dbeta without dgamma", dgamma=None)
    refused(bwd, IQ_ERR_ARG, "dropout on without dy", dy=None)
    for D in (20, 2056, 2560, 4096, 0):
        assert L.iq_ln_supported(D) == 0 and L.iq_ln_bwd_partial_rows(RM, D) == 0
        refused(fwd, IQ_ERR_UNSUPPORTED, f"forward D = {D}", D=D)
        refused(bwd, IQ_ERR_UNSUPPORTED, f"backward D = {D}", D=D)
    refused(fwd, IQ_OK, "forward M = 0", M=0)
    refused(bwd, IQ_OK, "backward M = 0", M=0)
    # and the same buffers still run
    e.forward(L)
    e.backward(L, True, True, 0)


def test_zz_report(L):
    """Prints what ran: per kernel instance the number of (M, D) cases that launched it, per tolerance the worst observed value in
    units of its bound, the file's wall time.  Asserts only that a full run of this file reached every instance."""
    print()
    for name in sorted(INSTANCES):
        ds = sorted({d for _, d in INSTANCES[name]})
        print(f"{name}: {len(INSTANCES[name])} cases, D = {ds if len(ds) <= 8 else f'{ds[:4]} .. {ds[-2:]} ({len(ds)} widths)'}")
    for name in sorted(REPORT):
        print(f"worst {name} = {REPORT[name][0]:.3f}   ({REPORT[name][1]})")
    print(f"wall time since the import of this file: {time.time() - CLOCK['t0']:.2f} s")
    fwd_seen = [n for n in INSTANCES if n.startswith("ln_fwd")]
    if len(fwd_seen) >= 24:                       # a full run
        assert len(fwd_seen) == 24 and len(INSTANCES) == 72, f"{len(fwd_seen)} forward and {len(INSTANCES) - len(fwd_seen)} backward instances"
        assert all(v[0] <= 1.0 for v in REPORT.values())
