"""CPU: tests/chain_exact_ref.py is what it says it is, for exactly the numbers tests/test_gpu_chain_exact.py draws.

For every (D, F) of the GPU case table and the largest M used with it:
  * the amplitude conditions hold: max relu(X1 W1^T + b1) <= 128, |H W2^T| < 2^22, |gH| <= 256, max|dX1| < 128, max|dX2| < 128;
  * the expected outputs are exact in fp32 (gemm_exact_ref.round_bf16 asserts it wherever a value is stored);
  * the one rounding of Z is exercised: at least a tenth of its elements are not representable in bf16 before the store
    (under dropout at every width; without it from F = 256 on -- below that the sums stay mostly below 256, where every
    integer is a bf16 value);
  * every entry of VARIANTS changes a stored bf16 value or an exact partial on some case of the table: the GPU test would fail
    for that kind of wrong kernel.
The launch geometry restated there is pinned to hand-computed numbers.
"""
import pytest
import torch

import chain_exact_ref as CR
import gemm_exact_ref as GR

PAIRS = sorted({(D, F) for _, D, F in CR.cases()})


def inexact_share(v):
    """Share of fp64 values a bf16 does not hold."""
    return (v.float().to(torch.bfloat16).double() != v).float().mean().item()


def test_case_table_covers_what_it_claims():
    cases = CR.cases()
    assert len(set(cases)) == len(cases)
    for M in CR.SMALL_M + list(CR.LARGE):
        assert {d for m, d, f in cases if m == M} == {128, 192}, f"M = {M} must meet both widths"
    for F in CR.WIDTHS:
        shapes = {CR.chain_shape(m) for m, d, f in cases if f == F}
        assert shapes == {(5, 1), (8, 1), (7, 2)}, f"F = {F} misses a workgroup shape: {shapes}"
    for D in (128, 192):
        assert {CR.chain_shape(m) for m, d, f in cases if (d, f) == (D, 832)} == {(5, 1), (8, 1), (7, 2)}
        for F in CR.WIDTHS + [CR.F_LIMIT[D]]:
            ms = {m for m, d, f in cases if (d, f) == (D, F)}
            assert 81 in ms and ms & {16, 80} and ms & {1, 15, 17, 79}, f"D = {D}, F = {F}: {sorted(ms)}"
        assert CR.max_rows(D, CR.F_LIMIT[D]) == 81
        assert {m for m, d, f in cases if d == D and f == CR.F_LIMIT[D]} <= set(CR.SMALL_M)
    assert set(CR.LARGE) == {20480, 20481, 32768, 32769, 32785} and max(CR.LARGE) == CR.ROWS


def test_launch_geometry():
    assert [CR.chain_shape(m) for m in (1, 20480, 20481, 32768, 32769)] == [(5, 1), (5, 1), (8, 1), (8, 1), (7, 2)]
    # 20,481 rows: 1,281 units of 16 rows, 161 workgroups of 8; the last holds unit 1,280 = the one row 20,480
    assert (CR.units(20481), CR.partial_rows(20481)) == (1281, 161) and 160 * 8 * 16 == 20480
    # 32,769 rows: 1,025 units of 32, 147 workgroups of 7; the last holds units 1,022 .. 1,024: rows 32,704 .. 32,768 + three empty waves
    assert (CR.units(32769), CR.partial_rows(32769)) == (1025, 147) and 146 * 7 * 32 == 32704
    assert (CR.units(32785), CR.partial_rows(32785)) == (1025, 147)
    assert (CR.units(81), CR.partial_rows(81), CR.units(80), CR.partial_rows(80)) == (6, 2, 5, 1)
    assert CR.gate_bytes(81, 832) == 6 * 13 * 256
    # iq_ffn_chain_supported: three ring slots + (F + 9 D) floats within 160 KB
    for D, F in CR.F_LIMIT.items():
        assert 3 * 2 * 64 * D * 2 + (F + 9 * D) * 4 == 160 * 1024


@pytest.mark.parametrize("D,F", PAIRS, ids=[f"D{d}-F{f}" for d, f in PAIRS])
def test_operands_keep_every_store_exact(D, F):
    M = CR.max_rows(D, F)
    o = CR.operands(D, F)
    X1, rows = o["X1"][:M], torch.arange(M)
    # ---- forward core ----
    pre = CR.hidden_pre(X1, o["W1"], o["b1"])
    CR.assert_forward_exact(D, F, pre.max().item())
    assert pre.max().item() > 32, "the hidden activation should use the range it has"
    k1, k2 = CR.keep(rows, F, CR.SITE1), CR.keep(rows, D, CR.SITE2)
    shares = {}
    for drop in (False, True):
        H, Hv = CR.hidden(X1, o["W1"], o["b1"], k1 if drop else None)
        assert torch.equal(H.double(), Hv), "H must be representable: it is an MFMA operand"
        acc = CR.z_acc(H, o["W2"])
        assert acc.abs().max().item() < 2 ** 22
        zpre = CR._drop(acc + o["b2"].double(), k2 if drop else None) + X1.double()
        assert torch.equal(zpre, zpre.round()) and zpre.abs().max().item() < 2 ** 23
        Z = CR.z_store(acc, o["b2"], X1, k2 if drop else None)            # (asserts fp32 exactness)
        assert torch.isfinite(Z.float()).all()
        shares[drop] = inexact_share(zpre)
    print(f"D={D} F={F} M={M}: max relu = {pre.max().item():.0f}, share of Z a bf16 does not hold: {shares[False]:.3f} "
          f"without dropout, {shares[True]:.3f} with")
    assert shares[True] >= 0.1
    assert F < 256 or shares[False] >= 0.1
    # ---- PRE / POST ----
    Z1 = CR.z1_store(o["A"][:M], o["Wo"], o["bo"], o["R"][:M], CR.keep(rows, D, CR.SITE0))
    assert torch.isfinite(Z1.float()).all()
    yq = CR.yq_of_beta(o["beta_int"], o["Wq"], o["bq"])
    assert yq.abs().max().item() > 256, "Yq should pass 256, where the rounding shows"
    # ---- backward core ----
    for drop in (False, True):
        H, _ = CR.hidden(X1, o["W1"], o["b1"], k1 if drop else None)
        gH, gv = CR.gh_store(CR.gh_acc(o["dO"][:M], o["W2t"]), H)
        assert gv.abs().max().item() <= CR.GH_LIMIT and torch.equal(gH.double(), gv)
        dX = CR.dx_of(gH, o["W1t"], o["Rb"][:M])
        peak = dX.abs().max().item()
        live = (gv != 0).any(1).float().mean().item()
        print(f"   backward drop={drop}: max|gH| = {gv.abs().max().item():.0f}, max|dX1| = {peak:.0f}, rows of gH with a nonzero "
              f"cell {live:.2f}, hidden units some row reaches {(gv != 0).any(0).float().mean().item():.2f}")
        assert torch.equal(dX, dX.round()) and 8 < peak < GR.DX_LIMIT
        assert live > 0.9, "the second product must see a nonzero tile in (nearly) every row"
        assert torch.equal(CR.dbeta_rows(dX, M).float().double(), CR.dbeta_rows(dX, M))


@pytest.mark.parametrize("D", [128, 192])
def test_preb_operands_keep_dx2_below_the_limit(D):
    A, Wt, R, z, gamma = CR.preb_operands(D)
    assert A.shape == (CR.ROWS, 3 * D)
    dX = GR.lnbwd_dx(A[:CR.ROWS], Wt, R[:CR.ROWS])
    assert torch.equal(dX, dX.round()) and 16 < dX.abs().max().item() < GR.DX_LIMIT


def outputs(M, D, F, drop, variant=None):
    """Every exact quantity of one case as the statement -- or one of VARIANTS -- gives it."""
    o = CR.operands(D, F)
    X1, rows = o["X1"][:M], torch.arange(M)
    k1 = CR.keep(rows, F, CR.SITE1, stride=D if variant == "mask_stride_d" else None) if drop else None
    k2 = CR.keep(rows, D, CR.SITE2) if drop else None
    H, _ = CR.hidden(X1, o["W1"], o["b1"], k1, variant)
    Z = CR.z_store(CR.z_acc(H, o["W2"]), o["b2"], X1, k2, variant)
    Z1 = CR.z1_store(o["A"][:M], o["Wo"], o["bo"], o["R"][:M], CR.keep(rows, D, CR.SITE0) if drop else None, variant)
    Hexp, _ = CR.hidden(X1, o["W1"], o["b1"], CR.keep(rows, F, CR.SITE1) if drop else None)
    gH, _ = CR.gh_store(CR.gh_acc(o["dO"][:M], o["W2t"]), Hexp, variant)
    dbeta = CR.dbeta_rows(CR.dx_of(gH, o["W1t"], o["Rb"][:M]), M, variant)
    return dict(H=H, Z=Z, Z1=Z1, gH=gH, dbeta=dbeta.float())


PROBES = [(17, 128, 192, True), (81, 192, 832, True), (81, 192, 2368, False), (81, 128, 832, False)]


@pytest.mark.parametrize("variant", list(CR.VARIANTS))
def test_every_variant_is_caught_on_some_case(variant):
    assert all(p[:3] in CR.cases() for p in PROBES)
    caught = []
    for M, D, F, drop in PROBES:
        good, bad = outputs(M, D, F, drop), outputs(M, D, F, drop, variant)
        diff = [k for k in good if not torch.equal(good[k].view(torch.int16) if good[k].dtype == torch.bfloat16 else good[k],
                                                   bad[k].view(torch.int16) if bad[k].dtype == torch.bfloat16 else bad[k])]
        if diff:
            caught.append((M, D, F, drop, diff))
    print(variant, caught)
    assert caught, f"no probe case tells '{CR.VARIANTS[variant]}' from the true result"


def test_the_rounding_and_the_ragged_sums_are_what_they_say():
    acc = torch.tensor([[255.0]], dtype=torch.float64)
    one = torch.tensor([[1.0]]).to(torch.bfloat16)
    zero = torch.zeros(1)
    assert CR.z_store(acc, zero, one).tolist() == [[256.0]]                                   # 255 + 0 + 1
    assert CR.z_store(acc + 3, zero, one).tolist() == [[260.0]]                               # 259: the tie goes to even
    assert CR.z_store(acc + 3, zero, one, variant="truncate").tolist() == [[258.0]]
    assert CR.z_store(acc + 3, zero, one, variant="res_after_round").tolist() == [[260.0]]    # 258 + 1 -> 259 -> 260
    assert CR.z_store(acc + 5, zero, one, variant="res_after_round").tolist() == [[260.0]]    # true: 261 -> 260; 260 + 1 -> 260
    assert CR.z_store(acc + 2, zero, one, variant="res_after_round").tolist() == [[256.0]]    # true: 258; 257 -> 256, + 1 -> 256
    assert CR.z_store(acc + 2, zero, one).tolist() == [[258.0]]
    keep = torch.tensor([[False]])
    assert CR.z_store(acc, zero, one, keep).tolist() == [[1.0]] and CR.z_store(acc, zero, one, ~keep).tolist() == [[512.0]]   # 511
    dX = torch.arange(17 * 2, dtype=torch.float64).view(17, 2)
    assert CR.dbeta_rows(dX, 17).tolist() == [dX.sum(0).tolist()]
    assert CR.dbeta_rows(dX, 17, "ragged_copies").tolist() == [(dX.sum(0) + 15 * dX[16]).tolist()]
    g, _ = CR.gh_store(torch.tensor([[3.0, 3.0, 3.0]], dtype=torch.float64), torch.tensor([[0.0, -0.0, 2.0]]))
    assert g.tolist() == [[0.0, 0.0, 6.0]]
    g, _ = CR.gh_store(torch.tensor([[3.0, 3.0]], dtype=torch.float64), torch.tensor([[0.0, 2.0]]), "gate_ge")
    assert g.tolist() == [[6.0, 6.0]]
