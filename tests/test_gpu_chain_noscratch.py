"""GPU (MI355X): the chain kernels (csrc/ffn_chain.hip) at D = 192, F = 768 around the row count where the 7 x 32-row launch
shape starts, bit for bit against tests/chain_exact_ref.py -- the shapes at which a value that was parked in LDS, recomputed
from the lane index or kept past its old live range by the no-scratch change would show if it were wrong.

Rows (chain_exact_ref.chain_shape: 8 waves of 16 rows up to 32,768 rows, 7 waves of 32 above):
  32,768   whole 16-row waves, the last row count of the 8 x 16 shape (the 16-row instances must not have moved)
  32,781   7 x 32: the last wave with rows owns 13 of them (its second 16-row group is wholly past M), the four waves behind it
           in its workgroup own none and only feed the ring
  32,800   7 x 32: 1,025 whole waves -- every wave with rows takes the counted ring waits; four trailing waves without rows
  33,096   7 x 32: 168 frames of 197 rows, the last wave owns 8 rows
Variants: dropout off and on; iq_attn_out_ffn_chain_fwd without (MODE 1) and with (MODE 2) the q,k,v stage; iq_ffn_chain_bwd
without (MODE 0) and with (MODE 1) Wot / dA.

Method: the case functions of tests/test_gpu_chain_exact.py, unchanged -- H, Z, Z1, gH and the dbeta partial rows equal to the
host statement with torch.equal, the real quantities within that file's bounds, every operand between NaN guard rows, every
output prefilled with a pattern and compared whole between sentinels, the launched instance asserted by name, and every launch
made a second time into freshly poisoned buffers with the same bits everywhere (a value read from LDS before it was written
would differ between the two).  chain_exact_ref draws 32,785 rows; the rows past that repeat the first ones (row i holds row
i - 32,785: the amplitude conditions of the reference are conditions on single rows, the case functions assert them for the
rows used, and the dropout masks are indexed by the row's own number).
"""
import functools

import pytest
import torch

import chain_exact_ref as CR
import test_gpu_chain_exact as TE
from test_gpu_kernels import L  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, F = 192, 768
ROWS = [32768, 32781, 32800, 33096]
PER_ROW = ("X1", "A", "R", "Rb", "z1", "dO")
DEV_OPS = TE.dev_ops              # (the fixture below puts wide_ops in its place for the duration of a test)


@functools.lru_cache(maxsize=None)
def wide_ops(d, f):
    """test_gpu_chain_exact.dev_ops(d, f) (the device copies that file's own cases use, shared) with the per-row operands
    continued past chain_exact_ref.ROWS by repeating the first rows."""
    o = dict(DEV_OPS(d, f))
    more = max(ROWS) - CR.ROWS
    for k in PER_ROW:
        o[k] = torch.cat([o[k], o[k][:more]])
    return o


@pytest.fixture
def wide(monkeypatch):
    monkeypatch.setattr(TE, "dev_ops", wide_ops)


def test_rows_cover_both_shapes_and_their_edges():
    assert [CR.chain_shape(m) for m in ROWS] == [(8, 1), (7, 2), (7, 2), (7, 2)]
    assert 32781 % 32 == 13 and (CR.units(32781) % 7, CR.units(32800) % 7, CR.units(33096) % 7) == (3, 3, 6) and 32800 % 32 == 0 and 33096 == 168 * 197


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("M", ROWS)
def test_forward(L, wide, M, drop, mode):
    TE.fwd_fused_case(L, M, D, F, drop, mode)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("M", ROWS)
def test_backward(L, wide, M, drop):
    TE.bwd_core_case(L, M, D, F, drop)
