"""CPU: tests/ln_exact_ref.py is what it says it is, for exactly the numbers tests/test_gpu_ln_exact.py builds.

  * the fp64 statement (forward64 / backward64 / partials / reduced) against torch autograd in float64;
  * the launch geometry: every multiple of 8 up to 2560 falls into exactly the 24 instances, WIDTHS holds one width of each, and
    the host entry points iq_ln_supported / iq_ln_bwd_partial_rows / iq_ln_bwd_ws_bytes agree with instance / partial_rows;
  * the exactness conditions of the integer recipe in the kernel's fp32 expressions, at every width of WIDTHS and every mean kept
    (at least three per width), the bf16 representability of every operand and every expected output, |dgamma|, |dbeta| < 2^24
    at the largest M used, and that the closed forms (X = gamma sign + beta, dZ = sign u / s) ARE the fp64 statement;
  * the torch restatement of the dropout mask against dropout_ref.keep_groups;
  * every entry of VARIANTS changes a stored value at every width where it applies.
"""
import numpy as np
import pytest
import torch

import dropout_ref
import ln_exact_ref as LR

EPS = 1e-12
ids = [f"D{d}" for d in LR.WIDTHS]


def test_statement_matches_autograd():
    g = torch.Generator().manual_seed(5)
    for D, M in ((24, 7), (136, 5), (320, 19)):
        z = (torch.randn(M, D, generator=g) * 2 + 0.3).to(torch.bfloat16)
        gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
        dX = torch.randn(M, D, generator=g).to(torch.bfloat16)
        for eps in (1e-12, 1e-5):
            zr, gr, br = (t.double().requires_grad_(True) for t in (z, gamma, beta))
            out = torch.nn.functional.layer_norm(zr, (D,), gr, br, eps)
            out.backward(dX.double())
            X, mean, rstd = LR.forward64(z, gamma, beta, eps)
            assert torch.allclose(X, out.detach(), rtol=1e-12, atol=1e-12)
            assert torch.allclose(mean, z.double().mean(-1), rtol=1e-13, atol=1e-13)
            dz, rg, rb, _ = LR.backward64(dX, z, mean, rstd, gamma)
            assert torch.allclose(dz, zr.grad, rtol=1e-10, atol=1e-12)
            part = LR.partials(rg, rb, M, D)
            assert part.shape == (LR.partial_rows(M, D), 2 * D)
            red = LR.reduced(part, torch.ones(2 * D), 0)
            assert torch.allclose(red[:D], gr.grad, rtol=1e-10, atol=1e-12) and torch.allclose(red[D:], br.grad, rtol=1e-10, atol=1e-12)
            assert torch.equal(LR.reduced(part, torch.ones(2 * D), 1), red + 1)


def test_instances_cover_exactly_the_dispatch_table():
    seen = {}
    for D in range(8, 2561, 8):
        i = LR.instance(D)
        assert (i is None) == (D > 2048), D
        if i is not None:
            lpr, nv, masked = i
            assert masked or lpr * nv * 8 == D
            assert not masked or (lpr == 64 and 64 * (nv - 1) * 8 < D <= 64 * nv * 8)
            seen.setdefault(i, []).append(D)
    want = {(l, n, False) for l, n in LR.TABLE} | {(64, n, True) for n in (1, 2, 3, 4)}
    assert set(seen) == want and len(want) == 24
    assert {LR.instance(D) for D in LR.WIDTHS} == want, "WIDTHS must hit every instance"
    assert len(LR.WIDTHS) == 27 == len(set(LR.WIDTHS))
    for D in (-8, 0, 4, 20, 2056, 2560, 4096):
        assert LR.instance(D) is None
    # hand-computed: 768 = 32 lanes x 3 vectors, 8 rows per workgroup; 136 = 17 vectors, masked, one wave per row
    assert LR.instance(768) == (32, 3, False) and LR.rpb(768) == 8 and LR.rpw(768) == 2
    assert LR.instance(136) == (64, 1, True) and LR.rpb(136) == 4 and LR.rpw(136) == 1
    assert LR.instance(2040) == (64, 4, True) and LR.instance(1544) == (64, 4, True) and LR.instance(1536) == (64, 3, False)
    assert LR.rpb(8) == 256 and LR.row_edges(8) == [1, 63, 64, 255, 256, 257, 513, 131072, 131073]
    assert LR.row_edges(512) == [1, 3, 4, 5, 9, 2048, 2049]
    assert LR.partial_rows(131073, 8) == 512 and LR.partial_rows(257, 8) == 2 and LR.partial_rows(1, 8) == 1
    assert LR.fwd_cap_widths() == {4: 56, 8: 256, 16: 128, 32: 64, 64: 32, 128: 16, 256: 8}
    assert LR.lds_bytes(2040) == 65280 and LR.lds_bytes(1544) == 49408 and LR.lds_bytes(2048) == 65536 and LR.lds_bytes(1280) == 81920
    assert LR.fwd_name(768) == "ln_fwd_kernel<32, 3, false>" and LR.bwd_name(136, True) == "ln_bwd_kernel<64, 1, true, true>"


def test_host_entry_points_agree_with_the_restated_geometry():
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    for D in [-8, 0, 4] + list(range(8, 2561, 8)) + [4096]:
        assert L.iq_ln_supported(D) == (LR.instance(D) is not None), D
        for M in (-1, 0, 1, 3, 4, 5, 255, 256, 257, 2048, 2049, 131072, 131073, 1 << 20):
            assert L.iq_ln_bwd_partial_rows(M, D) == LR.partial_rows(M, D), (M, D)
    for D in LR.WIDTHS:
        assert L.iq_ln_bwd_ws_bytes(D) == LR.ws_bytes(D)
        assert LR.partial_rows(1 << 20, D) * 2 * D * 4 == LR.ws_bytes(D)


@pytest.mark.parametrize("D", LR.WIDTHS, ids=ids)
def test_fp32_expressions_are_exact(D):
    ms = LR.means(D)
    assert 0 in ms and len(set(ms)) >= 3, f"D = {D}: means {ms}"
    if D not in (56, 2040):
        assert ms == LR.CANDIDATE_MEANS
    assert LR.stats_are_exact(D), "var, rstd, c1 or c2 is off in fp32"
    # the same expressions once more, spelled out on the recipe's own sums
    inv = np.float32(1.0) / np.float32(D)
    for m in ms:
        for s in LR.SCALES:
            mean = np.float32(D * m) * inv
            var = np.float32(D * s * s) * inv
            rstd = np.float32(1.0) / np.sqrt(np.float32(var + np.float32(EPS)), dtype=np.float32)
            assert float(mean) == m and float(var) == s * s and float(rstd) == 1 / s
            assert float((np.float32(m + s) - mean) * rstd) == 1.0 and float((np.float32(m - s) - mean) * rstd) == -1.0
    print(f"D={D}: means kept {ms}")


def case_rows(D):
    """Rows that hold every (mean, scale, k1, k2, flip, e) the recipe draws, and two workgroups and a row."""
    return torch.arange(max(2 * LR.rpb(D) + 1, 48))


@pytest.mark.parametrize("D", LR.WIDTHS, ids=ids)
def test_recipe_is_exact_and_is_the_statement(D):
    rows = case_rows(D)
    M = len(rows)
    c = LR.exact_case(rows, D)
    base, ubase, ubase_nz = LR.patterns(D)
    assert int(base.sum()) == 0 and int(ubase.sum()) == 0 and int((ubase != 0).sum()) >= 4
    assert int(ubase_nz.sum()) == 0 and (ubase_nz != 0).all() and int(ubase_nz.abs().max()) == 4
    assert (c["sign"].sum(1) == 0).all()
    assert len({tuple(r.tolist()) for r in c["sign"][:8]}) == 8, "the sign order must differ from row to row"
    assert (c["mean"][1:] != c["mean"][:-1]).all(), "neighbouring rows must differ in their mean"
    p = LR.row_params(rows, D)
    assert ((p["k1"][1:] != p["k1"][:-1]) | (p["k2"][1:] != p["k2"][:-1])).all() and (p["k1"] == 0).any() and (p["k2"] == 0).any()
    assert set(p["s"].tolist()) == set(LR.SCALES) and set(p["m"].tolist()) == set(LR.means(D))
    # representable operands and outputs
    z, dX = LR.to_bf16(c["z"]), LR.to_bf16(c["dX"])
    for k in ("X", "dZ"):
        LR.to_bf16(c[k])
    LR.to_bf16(2 * c["dZ"])
    assert torch.equal(c["dX"], c["dX"].round()) and c["g"].abs().max().item() <= LR.G_LIMIT and c["dX"].abs().max().item() <= 32
    assert torch.equal(c["mean"].float().double(), c["mean"]) and torch.equal(c["rstd"].float().double(), c["rstd"])
    assert not (c["X"] == 0).logical_and(torch.signbit(c["X"])).any() and not (c["dZ"] == 0).logical_and(torch.signbit(c["dZ"])).any()
    # the closed forms are the fp64 statement (every step is exact in fp64 too)
    X, mean, rstd = LR.forward64(z, LR.fwd_gamma(D), LR.fwd_beta(D), 0.0)
    assert torch.equal(X, c["X"]) and torch.equal(mean, c["mean"]) and torch.equal(rstd, c["rstd"])
    dz, rg, rb, gmax = LR.backward64(dX, z, c["mean"], c["rstd"], LR.bwd_gamma(D))
    assert torch.equal(dz, c["dZ"]) and torch.equal(rg, c["dX"] * c["sign"]) and gmax.max().item() <= LR.G_LIMIT
    # every partial sum of the row sums is exact in fp32 whatever the order: multiples of 1/2 (z) or integers far below 2^24
    assert (c["z"].abs().sum(1) < 2 ** 22).all() and torch.equal(c["z"] * 2, (c["z"] * 2).round())
    assert (c["g"].abs().sum(1) < 2 ** 22).all() and torch.equal(c["g"], c["g"].round())
    # column sums: integers below 2^24 at the most rows any case has
    assert 32 * max(LR.row_edges(D)) < 2 ** 24 and max(LR.row_edges(D)) <= 131073
    part = LR.partials(rg, rb, M, D)
    assert torch.equal(part, part.round()) and torch.equal(part.sum(0)[D:], c["dX"].sum(0))


def test_all_widths_recipe_is_exact_whatever_the_last_bits_of_rstd():
    """The centred recipe at every supported width, in fp32 as the kernel evaluates it, with rstd as torch rounds it and pushed
    2^-22 either way (more than the ulp fl(D s^2 fl(1 / D)) can be off by): the bf16 stores are the closed forms."""
    inexact = []
    for D in range(8, LR.D_MAX + 1, 8):
        c = LR.exact_case(torch.arange(5), D, centred=True)
        z, dX = LR.to_bf16(c["z"]).float(), LR.to_bf16(c["dX"]).float()
        X, dZ = LR.to_bf16(c["X"]), LR.to_bf16(c["dZ"])
        LR.to_bf16(2 * c["dZ"])
        assert not (c["X"] == 0).any() and not (c["dZ"] == 0).any() and (c["mean"] == 0).all() and len(set(LR.row_params(torch.arange(5), D, centred=True)["s"].tolist())) >= 2
        inv = torch.tensor(1.0) / torch.tensor(float(D))
        mean = z.sum(1) * inv
        var = ((z - mean[:, None]) ** 2).sum(1) * inv
        assert (mean == 0).all()
        if not torch.equal(var.double(), (c["rstd"] ** -2)):
            inexact.append(D)
        for push in (1.0, 1 + 2.0 ** -22, 1 - 2.0 ** -22):
            rstd = (1 / torch.sqrt(var + torch.tensor(EPS))) * torch.tensor(push)
            assert ((rstd.double() * c["rstd"] ** -1 - 1).abs() <= 2.0 ** -21).all()
            xh = (z - mean[:, None]) * rstd[:, None]
            x32 = LR.fwd_gamma(D) * xh + LR.allwidths_beta(D)
            g = dX * LR.bwd_gamma(D)
            c1 = g.sum(1, keepdim=True) * inv
            c2 = (g * xh).sum(1, keepdim=True) * inv              # (need not cancel to the last bit: |c2| stays below 2^-20)
            assert (c1 == 0).all() and (c2.abs() <= 2.0 ** -20).all()
            dz32 = rstd[:, None] * (g - c1 - xh * c2)
            assert torch.equal(x32.to(torch.bfloat16).view(torch.int16), X.view(torch.int16)), D
            assert torch.equal(dz32.to(torch.bfloat16).view(torch.int16), dZ.view(torch.int16)), D
    assert LR.instance(328) is not None and 328 in inexact and not set(inexact) & set(LR.WIDTHS)
    print(f"{len(inexact)} widths where var misses s^2 in fp32: {inexact}")


def test_all_zero_row():
    rows = torch.arange(9)
    c = LR.exact_case(rows, 24, zero_rows=(5,))
    assert (c["z"][5] == 0).all() and torch.equal(c["X"][5], LR.fwd_beta(24).double()) and (c["live"][5] == 0).all()
    assert (c["z"][4] != 0).any() and torch.isfinite(c["dX"]).all()


@pytest.mark.parametrize("D,p", [(8, 0.5), (24, 0.5), (136, 0.1), (2040, 0.25)])
def test_torch_mask_is_dropout_ref(D, p):
    rows = torch.tensor([0, 1, 2, 63, 64, 131072, 1048576, (1 << 31) // D, (1 << 33) // D + 5, (1 << 36) // D + 1])
    got = LR.keep(rows, D, p=p)
    groups = rows.numpy().astype(np.uint64)[:, None] * np.uint64(D // 8) + np.arange(D // 8, dtype=np.uint64)[None, :]
    want = dropout_ref.keep_groups(LR.SEED, LR.STEP, LR.SITE, p, groups).reshape(len(rows), D)
    assert np.array_equal(got.numpy(), want)
    assert 0.5 * p < 1 - got.float().mean().item() < 1.5 * p + 0.02
    assert float(dropout_ref.dropout_scale(0.5)) == 2.0


def applies(variant, D, M):
    lpr, nv, masked = LR.instance(D)
    return {"wide_reduce": LR.rpw(D) >= 2 and M >= 2, "transposed_gamma": lpr > 1 and nv > 1, "tail_in_var": masked and LR._padded(D) > D,
            "padded_div": masked and LR._padded(D) > D, "last_stripe_missing": M > LR.BWD_CAP * LR.rpb(D)}.get(variant, True)


def stored(D, rows, variant=None, before=None):
    """Every stored value of a forward + backward (dropout on, accumulate = 1) as the statement or a variant gives it."""
    M = len(rows)
    c = LR.exact_case(rows, D)
    z, dX = LR.to_bf16(c["z"]), LR.to_bf16(c["dX"])
    X, mean, rstd = LR.forward64(z, LR.fwd_gamma(D), LR.fwd_beta(D), EPS, variant)
    dz, rg, rb, _ = LR.backward64(dX, z, c["mean"], c["rstd"], LR.bwd_gamma(D), variant)
    dy = LR.dropped(dz, LR.keep(rows, D, row_offset=variant != "mask_no_row"))
    part = LR.partials(rg, rb, M, D, variant)
    out = dict(X=X.float().to(torch.bfloat16), mean=mean.float(), rstd=rstd.float(), dz=dz.float().to(torch.bfloat16),
               dy=dy.float().to(torch.bfloat16), part=part.float(), red=LR.reduced(part, before, 1, variant).float())
    return out


@pytest.mark.parametrize("variant", list(LR.VARIANTS))
def test_every_variant_is_told_apart_at_every_width_it_applies_to(variant):
    hit = 0
    for D in LR.WIDTHS:
        Ms = [2 * LR.rpb(D) + 1]
        if variant == "last_stripe_missing":
            Ms = [LR.BWD_CAP * LR.rpb(D) + 1] if D <= 64 else []     # (the wide ones hold the same arithmetic at 100 times the cost)
        for M in Ms:
            if not applies(variant, D, M):
                continue
            rows = torch.arange(M)
            before = torch.arange(2 * D).double() % 11 + 1
            good, bad = stored(D, rows, None, before), stored(D, rows, variant, before)
            diff = [k for k in good if not torch.equal(good[k], bad[k])]
            assert diff, f"D = {D}, M = {M}: nothing stored tells '{LR.VARIANTS[variant]}' from the true result"
            hit += 1
    assert hit >= 4, f"{variant} applied at {hit} widths only"
