"""GPU (MI355X): the slab reduce of a layer's weight gradients riding in the next data-gradient launch
(iq_gemm_bf16_wgrad_grouped_deferred + iq_gemm_bf16_lnbwd_ride; csrc/wgrad_reduce.h, csrc/gemm_lnbwd.hip, csrc/model.hip).

Kernel level.  The same operands go through the two-launch form (iq_gemm_bf16_wgrad_grouped, then iq_gemm_bf16_lnbwd) and
through the riding form; every output -- four dW, four dbias, four extra-segment outputs, dZ, dY, the partial rows -- must be
torch.equal: the reduce role runs the arithmetic of wgrad_reduce_kernel in its order, so there is no tolerance.  Outputs that
a call overwrites start as NaN, accumulated ones from seeded values; every output and the slab workspace sit between guard
bands that are compared afterwards.  Which form ran is read from the profiling records (prof_names.kernel_launches), and
whether a shape has room for the job is asked of the library (iq_gemm_lnbwd_ride_workgroups, which asks the runtime for
the kernel's occupancy): the slot count is not restated here.

Model level.  The two-layer D = 128 raw-IQ model of test_gpu_route_boundaries.py at B = 505 (32,825 rows: above the row count
up to which the chain launch takes the q,k,v data gradient, so gemm_lnbwd_kernel<64, 128> is a launch of its own) and a
three-layer variant, which uses both norm2 partial-row buffers.
"""
import ctypes as C
import math

import pytest
import torch

import iq_oracle as O
from prof_names import kernel_launches

pytestmark = pytest.mark.gpu

NAN = float("nan")
RED = "wgrad_reduce_kernel"
BAND = 256                   # guard bytes on either side of a buffer
FILL = 0x5A


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vit_vs_raw_iq_amd._native as N
    return N.lib()


def _N():
    import vit_vs_raw_iq_amd._native as N
    return N


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Banded:
    """A tensor of `shape` between two guard bands of BAND bytes."""

    def __init__(self, shape, dtype):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        self.nbytes = n
        self.raw = torch.full((BAND + n + BAND,), FILL, dtype=torch.uint8, device=dev())
        self.t = self.raw[BAND:BAND + n].view(dtype).view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:BAND] == FILL).all()) and bool((self.raw[BAND + self.nbytes:] == FILL).all())


def randn_bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=dev(), generator=g) * scale).to(torch.bfloat16)


class Case:
    """The operands of one layer's weight gradients + the q,k,v data gradient with norm2 backward behind them, and two sets of
    outputs: [0] for the two-launch form, [1] for the riding form."""

    # extra segments (rows, n, row stride, column offset): "wide" with 3 rows, "tall" with 70 rows, n = 190 (the scalar tail
    # of a column count that is no multiple of 4), and a tall one with the tail
    def extras(self, D):
        return [(3, D, 2 * D, 0), (70, D, 2 * D, D), (37, 190, 256, 0), (300, 62, 64, 0)]

    def __init__(self, L, M, D, F, seed):
        N = _N()
        self.L, self.M, self.D, self.F = L, M, D, F
        g = torch.Generator(device="cuda").manual_seed(seed)
        s = 1.0 / 8
        # dY | X of ffn.linear2, ffn.linear1, attention.w_concat, w_q|w_k|w_v -- as backward_impl groups them
        self.ops = [(randn_bf16(g, M, D, scale=s), randn_bf16(g, M, F)), (randn_bf16(g, M, F, scale=s), randn_bf16(g, M, D)),
                    (randn_bf16(g, M, D, scale=s), randn_bf16(g, M, D)), (randn_bf16(g, M, 3 * D, scale=s), randn_bf16(g, M, D))]
        self.shapes = [(D, F), (F, D), (D, D), (3 * D, D)]
        self.gqkv = self.ops[3][0]
        self.wt = randn_bf16(g, D, 3 * D, scale=(3 * D) ** -0.5)
        self.res = randn_bf16(g, M, D, scale=s)
        self.z = randn_bf16(g, M, D)
        zf = self.z.float()
        self.mean = zf.mean(1).contiguous()
        self.rstd = (1.0 / torch.sqrt(zf.var(1, unbiased=False) + 1e-12)).contiguous()
        self.gamma = torch.rand(D, device=dev(), generator=g) + 0.5
        self.drop = N.Dropout(seed=77, step=3, site=5, p=0.1, step_dev=None)
        self.prows = L.iq_gemm_lnbwd_partial_rows(M)
        self.block_rows = 64 if self.prows == (M + 63) // 64 else 128
        self.host = f"gemm_lnbwd_kernel<{self.block_rows}, {D}>"
        self.parts = []
        for rows, n, stride, off in self.extras(D):
            buf = torch.randn(rows, stride, device=dev(), generator=g)
            self.parts.append(buf[:, off:off + n])
        # outputs: name -> (Banded, start values or None = overwritten: NaN)
        self.out = []
        for _ in range(2):
            o = {}
            for i, (n, k) in enumerate(self.shapes):
                o[f"dW{i}"] = Banded((n, k), torch.float32)
                o[f"db{i}"] = Banded((n,), torch.float32)
            for j, (rows, n, stride, off) in enumerate(self.extras(D)):
                o[f"extra{j}"] = Banded((n,), torch.float32)
            o["dZ"] = Banded((M, D), torch.bfloat16)
            o["dY"] = Banded((M, D), torch.bfloat16)
            o["partial"] = Banded((self.prows, 2 * D), torch.float32)
            self.out.append(o)
        self.start = {k: torch.randn(v.t.shape, device=dev(), generator=g) for k, v in self.out[0].items() if k[0] in "de" and k not in ("dZ", "dY")}
        self.probs = [(N.WgradProblem * 4)(), (N.WgradProblem * 4)()]
        self.segs = [(N.ReduceSeg * 4)(), (N.ReduceSeg * 4)()]
        for w in range(2):
            o = self.out[w]
            for i, ((dY, X), (n, k)) in enumerate(zip(self.ops, self.shapes)):
                p = self.probs[w][i]
                p.dY, p.ldy, p.X, p.ldx, p.dW, p.dbias, p.N, p.K = dY.data_ptr(), n, X.data_ptr(), k, o[f"dW{i}"].ptr(), o[f"db{i}"].ptr(), n, k
            for j, (rows, n, stride, off) in enumerate(self.extras(D)):
                sg = self.segs[w][j]
                sg.partials, sg.rows, sg.row_stride, sg.out, sg.n = self.parts[j].data_ptr(), rows, stride, o[f"extra{j}"].ptr(), n
        self.nbytes = L.iq_wgrad_grouped_ws_bytes(self.probs[0], 4, M, 0)
        self.ws = Banded((self.nbytes // 4,), torch.float32)

    def reset(self, w, accumulate):
        for k, b in self.out[w].items():
            if accumulate and k in self.start:
                b.t.copy_(self.start[k])
            else:
                b.t.fill_(NAN)
        self.ws.t.fill_(NAN)

    def lnbwd_args(self, w):
        o, D = self.out[w], self.D
        return (self.gqkv.data_ptr(), 3 * D, self.wt.data_ptr(), 3 * D, self.res.data_ptr(), D, self.z.data_ptr(),
                self.mean.data_ptr(), self.rstd.data_ptr(), self.gamma.data_ptr(), C.byref(self.drop), o["dZ"].ptr(), o["dY"].ptr(),
                o["partial"].ptr(), self.M, D, 3 * D)

    def two_launches(self, accumulate):
        N, L = _N(), self.L
        self.reset(0, accumulate)

        def go():
            N.check(L.iq_gemm_bf16_wgrad_grouped(self.probs[0], 4, self.M, self.ws.ptr(), self.nbytes, accumulate, 0, self.segs[0], 4,
                                                 stream()), "wgrad_grouped")
            N.check(L.iq_gemm_bf16_lnbwd(*self.lnbwd_args(0), stream()), "lnbwd")
        return kernel_launches(L, go)

    def riding(self, accumulate):
        """-> ({kernel: launches}, reduce workgroups the library says the launch appends)"""
        N, L = _N(), self.L
        self.reset(1, accumulate)
        job = N.ReduceJob()
        wgs = []

        def go():
            N.check(L.iq_gemm_bf16_wgrad_grouped_deferred(self.probs[1], 4, self.M, self.ws.ptr(), self.nbytes, accumulate, 0,
                                                          self.segs[1], 4, C.byref(job), stream()), "wgrad_grouped_deferred")
            wgs.append(L.iq_gemm_lnbwd_ride_workgroups(self.M, self.D, 3 * self.D, job.nblk))
            N.check(L.iq_gemm_bf16_lnbwd_ride(*self.lnbwd_args(1), C.byref(job), stream()), "lnbwd_ride")
        rec = kernel_launches(L, go)
        assert job.nseg == 12 and job.nblk > 0 and job.accumulate == accumulate
        return rec, wgs[0]

    def compare(self, what):
        torch.cuda.synchronize()
        for k in self.out[0]:
            a, b = self.out[0][k], self.out[1][k]
            assert bool(torch.isfinite(a.t.float()).all()), f"{what}: {k} of the two-launch form is not finite"
            assert torch.equal(a.t, b.t), f"{what}: {k} differs, {int((a.t != b.t).sum())} of {a.t.numel()} elements"
            assert a.intact() and b.intact(), f"{what}: guard band around {k} overwritten"
        assert self.ws.intact(), f"{what}: guard band around the slab workspace overwritten"


# (M, D, F, rides, partial-tile kernel)
#   D 192 / F 768, M = 4,096: wgrad_big_kernel<192>, 64 host blocks of 64 rows: a large hole
#   D 128 / F 256, M = 4,100: no multiple of 64 -> the wave-private kernel, and a ragged last host block (4 rows)
#   D 128 / F 256, M = 98,560: 770 host blocks of 128 rows, more than the GPU holds at once -> no hole, the call falls back
CASES = [(4096, 192, 768, True, "wgrad_big_kernel<192>"), (4100, 128, 256, True, "wgrad_pw_kernel"),
         (98560, 128, 256, False, "wgrad_big_kernel<128>")]


@pytest.mark.parametrize("M,D,F,rides,tile_kernel", CASES, ids=[f"M{c[0]}-D{c[1]}" for c in CASES])
def test_riding_form_equals_the_two_launches_bit_for_bit(L, M, D, F, rides, tile_kernel):
    c = Case(L, M, D, F, seed=M + D)
    for accumulate in (0, 1):
        what = f"M={M} D={D} F={F} accumulate={accumulate}"
        ref = c.two_launches(accumulate)
        assert ref == {tile_kernel: 1, RED: 1, c.host: 1}, f"{what}: the two-launch form ran {ref}"
        rec, wgs = c.riding(accumulate)
        print(f"{what}: riding form ran {rec}, {wgs} reduce workgroups")
        assert (wgs > 0) == rides, f"{what}: the library reports {wgs} reduce workgroups"
        want = {tile_kernel: 1, c.host: 1}
        if wgs == 0:
            want[RED] = 1                                  # no hole: the stand-alone reduce, then the plain launch
        assert rec == want, f"{what}: the riding form ran {rec}, expected {want}"
        c.compare(what)


def test_job_run_alone_equals_the_grouped_call(L):
    """deferred + iq_reduce_job_run is iq_gemm_bf16_wgrad_grouped; an empty or absent job makes the ride the plain launch."""
    N = _N()
    c = Case(L, 4100, 128, 256, seed=11)
    assert c.two_launches(0) == {"wgrad_pw_kernel": 1, RED: 1, c.host: 1}
    c.reset(1, 0)
    job = N.ReduceJob()

    def go():
        N.check(L.iq_gemm_bf16_wgrad_grouped_deferred(c.probs[1], 4, c.M, c.ws.ptr(), c.nbytes, 0, 0, c.segs[1], 4, C.byref(job),
                                                      stream()), "wgrad_grouped_deferred")
        N.check(L.iq_reduce_job_run(C.byref(job), stream()), "reduce_job_run")
        N.check(L.iq_gemm_bf16_lnbwd_ride(*c.lnbwd_args(1), None, stream()), "lnbwd_ride without a job")
    assert kernel_launches(L, go) == {"wgrad_pw_kernel": 1, RED: 1, c.host: 1}
    c.compare("deferred + run")
    empty = N.ReduceJob()
    rec = kernel_launches(L, lambda: N.check(L.iq_gemm_bf16_lnbwd_ride(*c.lnbwd_args(1), C.byref(empty), stream()), "empty job"))
    assert rec == {c.host: 1}
    c.compare("empty job")


# ------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------
KW = dict(in_channels=2, seq_length=128, num_classes=5, d_model=128, n_head=2, ffn_hidden=64, use_cls_token=True,
          embedding_type="segment", segment_size=2)
B_ROUTE = 505                # 65 rows per frame: 32,825 rows
# wgrad_reduce_kernel launches of one backward pass BEFORE the reduce rode (read once from the parent library at these
# shapes): one per encoder layer + one for the embedding's weight gradient.
REDUCES_BEFORE = {2: 3, 3: 4}
GRAD_REL, GRAD_ABS_OF_TOTAL = 5e-2, 2e-3      # the limits of tests/test_gpu_model.py for every parameter class but ffn.linear1


@pytest.mark.parametrize("n_layers", [2, 3])
def test_model_backward_with_the_reduce_riding(L, n_layers):
    import vit_vs_raw_iq_amd as P
    cfg = O.OracleConfig(kind="rawiq", drop_prob=0.0, n_layers=n_layers, **KW)
    sd = O.init_state(cfg, 4)
    m = P.AMCTransformerRawIQ(drop_prob=0.0, device="cuda", n_layers=n_layers, **KW)
    m.load_state_dict(sd)
    m.to(dev()).train()
    g = torch.Generator().manual_seed(B_ROUTE + n_layers)
    x = torch.randn(B_ROUTE, 2, 128, generator=g)
    y = torch.randint(0, 5, (B_ROUTE,), generator=g)
    xd, yd = x.to(dev()), y.to(dev())
    grads, recs = [], []
    for _ in range(2):
        for p in m.parameters():
            p.grad = None
        loss = torch.nn.functional.cross_entropy(m(xd), yd, label_smoothing=0.1)
        recs.append(kernel_launches(L, loss.backward))
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
    print(f"n_layers={n_layers}: backward ran {recs[0]}")
    for k, v in grads[0].items():
        assert bool(torch.isfinite(v).all()), f"{k}: gradient not finite"
        assert torch.equal(v, grads[1][k]), f"{k}: two backward passes from the same state differ"
    assert recs[0] == recs[1]
    assert recs[0].get("gemm_lnbwd_kernel<64, 128>") == n_layers - 1
    assert recs[0].get(RED, 0) == REDUCES_BEFORE[n_layers] - (n_layers - 1)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, _, gref = O.loss_and_grads(cfg, sd, x, y, 0.1)
    total_ref = math.sqrt(sum(float(v.double().pow(2).sum()) for v in gref.values()))
    norms = [k for k in grads[0] if ".norm1." in k or ".norm2." in k]
    assert len(norms) == 4 * n_layers, norms
    for k in norms:
        r = gref[k].double()
        e = (grads[0][k].cpu().double() - r).norm().item()
        lim = GRAD_REL * r.norm().item() + GRAD_ABS_OF_TOTAL * total_ref
        print(f"  {k}: ||err|| {e:.4g}, limit {lim:.4g}, ||ref|| {r.norm().item():.4g}")
        assert e <= lim, f"grad {k}: ||err|| {e:.4g} > {lim:.4g} (||ref|| {r.norm().item():.4g})"
