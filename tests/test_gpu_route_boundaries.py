"""GPU (MI355X): which kernels a call launches is a function of its shapes alone.  Each test stands on either side of one
threshold of the launch routes (csrc/model.hip layer_route, csrc/gemm_ln.hip, csrc/gemm_nt.hip) and reads the kernels that
ran from the profiling records (prof_names.kernel_launches).  The records are per-name launch counts, not a sequence: the
order of the two chain launches of the two-layer model follows from which layer can run which mode (forward: only the
bottom layer has a layer above whose q,k,v projection it can take, mode 2; backward: only the bottom layer has a layer
above whose q,k,v data gradient it can take, mode 2).
"""
import pytest
import torch

from prof_names import kernel_launches

pytestmark = pytest.mark.gpu


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


def chain(direction, waves, rows16, mode):
    return f"ffn_chain_{direction}_kernel<128, {waves}, {rows16}, false, {mode}>"


# S = 65 rows per frame, so M = 65 B.  The chain runs from 8,192 rows; 5 waves of 16 rows up to 20,480 rows, 8 up to 32,768,
# 7 waves of 32 rows above; up to 32,768 rows the backward launch of the bottom layer takes the q,k,v data gradient of the
# layer above + norm2 backward (mode 2), above that stage is a launch of its own (gemm_lnbwd_kernel, 64-row blocks: 257
# blocks of 128 rows <= 320).  Below 8,192 rows no chain kernel runs: the tiled route has norm1 backward of either layer and
# norm2 backward of the bottom layer in the epilogue of a data-gradient GEMM (three gemm_lnbwd launches).
ROUTES = [
    (126, {}, {"gemm_lnbwd_kernel<64, 128>": 3}),
    (127, {chain("fwd", 5, 1, 2): 1, chain("fwd", 5, 1, 1): 1}, {chain("bwd", 5, 1, 1): 1, chain("bwd", 5, 1, 2): 1}),
    (504, {chain("fwd", 8, 1, 2): 1, chain("fwd", 8, 1, 1): 1}, {chain("bwd", 8, 1, 1): 1, chain("bwd", 8, 1, 2): 1}),
    (505, {chain("fwd", 7, 2, 2): 1, chain("fwd", 7, 2, 1): 1}, {chain("bwd", 7, 2, 1): 2, "gemm_lnbwd_kernel<64, 128>": 1}),
]


@pytest.mark.parametrize("B,fwd_want,bwd_want", ROUTES, ids=[f"B{r[0]}" for r in ROUTES])
def test_model_route_on_either_side_of_each_row_threshold(L, B, fwd_want, bwd_want):
    import vit_vs_raw_iq_amd as P
    torch.manual_seed(3)
    m = P.AMCTransformerRawIQ(in_channels=2, seq_length=128, num_classes=5, d_model=128, n_head=2, n_layers=2, ffn_hidden=64,
                              drop_prob=0.0, device="cuda", use_cls_token=True, embedding_type="segment", segment_size=2).to(dev())
    m.train()
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 2, 128, generator=g).to(dev())
    y = torch.randint(0, 5, (B,), generator=g).to(dev())
    res = {}
    fwd = kernel_launches(L, lambda: res.setdefault("logits", m(x)))
    loss = torch.nn.functional.cross_entropy(res["logits"], y)
    bwd = kernel_launches(L, loss.backward)
    print(f"B={B} M={65 * B}\n  forward  {fwd}\n  backward {bwd}")
    picked = lambda rec: {n: c for n, c in rec.items() if "ffn_chain" in n or "gemm_lnbwd" in n}
    assert picked(fwd) == fwd_want
    assert picked(bwd) == bwd_want
    grad = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    assert torch.isfinite(res["logits"]).all() and torch.isfinite(grad).all()


@pytest.mark.parametrize("M,rows", [(40960, 64), (40961, 128)])
def test_gemm_ln_row_block_on_either_side_of_320_blocks(L, M, rows):
    N, D = _N(), 128
    g = torch.Generator(device="cuda").manual_seed(M)
    A = torch.randn(M, D, device=dev(), generator=g).to(torch.bfloat16)
    R = torch.randn(M, D, device=dev(), generator=g).to(torch.bfloat16)
    W = (torch.randn(D, D, device=dev(), generator=g) / D ** 0.5).to(torch.bfloat16)
    bias, gamma, beta = (torch.randn(D, device=dev(), generator=g) for _ in range(3))
    Z = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=dev())
    X = torch.full_like(Z, float("nan"))
    mean, rstd = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    rec = kernel_launches(L, lambda: N.check(L.iq_gemm_bf16_ln(
        A.data_ptr(), D, W.data_ptr(), D, bias.data_ptr(), R.data_ptr(), D, None, gamma.data_ptr(), beta.data_ptr(), 1e-12,
        Z.data_ptr(), X.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, D, D, stream()), "gemm_ln"))
    assert rec == {f"gemm_ln_kernel<{rows}, 128>": 1}
    assert torch.isfinite(Z.float()).all() and torch.isfinite(X.float()).all()


@pytest.mark.parametrize("M,rows", [(65408, 64), (65536, 128)])
def test_gemm_nt_row_tile_on_either_side_of_512_tiles(L, M, rows):
    N, K = _N(), 128
    g = torch.Generator(device="cuda").manual_seed(M)
    A = torch.randn(M, K, device=dev(), generator=g).to(torch.bfloat16)
    W = (torch.randn(K, K, device=dev(), generator=g) / K ** 0.5).to(torch.bfloat16)
    Cout = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=dev())
    rec = kernel_launches(L, lambda: N.check(L.iq_gemm_bf16_nt(
        A.data_ptr(), K, W.data_ptr(), K, Cout.data_ptr(), K, M, K, K, None, stream()), "gemm_nt"))
    assert rec == {f"gemm_nt_async_kernel<{rows}, 128, 0, false>": 1}
    assert torch.isfinite(Cout.float()).all()
