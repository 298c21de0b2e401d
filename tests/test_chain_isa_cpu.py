"""CPU: register and scratch budget of the two chain kernels (csrc/ffn_chain.hip), read from the kernel metadata of the gfx950
code object (hipcc cross-compiles without a GPU).  Only the metadata is read, never the instruction text.

Both kernels are launched with up to 448 threads and __launch_bounds__(NW * 64, 2): two waves per SIMD, so a wave may hold
512 / 2 = 256 VGPRs.  The D = 192 instances with 32-row waves (<192, 7, 2, ...>, what cfg B launches) sit at or near that cap.
Before this test was written the backward spilled 6 to 68 VGPRs there (28 to 212 B of scratch per lane, some of the stores and
reloads inside the chunk loop, where they are counted by the same vmcnt as the weight ring's hand-counted waits): the
LayerNorm-backward tail's row loop was unrolled.  What moved, and what it measured: profiles/chain_spills.txt.

Asserted, per instance <D, NW, RG, dropout, MODE> of both kernels:
  * ffn_chain_bwd<192, 7, 2, *, 0 | 1> (MODE 1 with dropout is what cfg B launches): no scratch, no spilled VGPR, at most 256;
  * ffn_chain_bwd<192, 7, 2, *, 2> (the variant with the q,k,v data gradient in front, not launched by cfg B) is bounded by
    what it was before, 68 / 58 spilled VGPRs, 212 / 180 B, 21 / 0 spilled SGPRs (it holds 3 / 3, 16 / 16 B, 19 / 0 now);
  * ffn_chain_fwd<192, 7, 2, true, *>: a build without its 1 to 3 spilled VGPRs and 8 to 46 spilled SGPRs was made and measured,
    and left out because it gained nothing that could be told from noise (profiles/chain_spills.txt, "The forward part"): the
    kernel's source is unchanged and the bounds are the values it has had, so that it does not get worse unnoticed;
  * every instance that had no scratch before: still none.
"""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

NAME = re.compile(r"ffn_chain_(fwd|bwd)_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d)EE")
SHAPES = [(7, 2), (5, 1), (8, 1)]                     # chain_shape's (waves per workgroup, 16-row groups per wave)
# (dropout, MODE) of the ffn_chain_bwd<192, 7, 2, ...> instances that had scratch before and have none now
ZERO = [(drop, mode) for drop in (0, 1) for mode in (0, 1)]
BWD_MODE2_BEFORE = {1: dict(scratch=212, vspill=68, sspill=21), 0: dict(scratch=180, vspill=58, sspill=0)}
# ffn_chain_fwd<192, 7, 2, true, MODE>: the no-spill build did not measure (module docstring); the values of the unchanged source
FWD_UNCHANGED = {2: dict(scratch=12, vspill=2, sspill=46), 1: dict(scratch=16, vspill=3, sspill=12), 0: dict(scratch=8, vspill=1, sspill=8)}


@pytest.fixture(scope="module")
def meta():
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    try:
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                               "-S", "--cuda-device-only", os.path.join(csrc, "ffn_chain.hip"), "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        os.unlink(out)
    text = text[text.index("amdhsa.kernels:"):]
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?"
                         r"\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
        n = NAME.search(m.group(1))
        if n:
            key = (n.group(1),) + tuple(int(x) for x in n.groups()[1:])
            found[key] = dict(scratch=int(m.group(2)), sspill=int(m.group(3)), vgpr=int(m.group(4)), vspill=int(m.group(5)))
    return found


def test_every_instance_is_there(meta):
    want = {(k, d, nw, rg, drop, mode) for k in ("fwd", "bwd") for d in (128, 192) for nw, rg in SHAPES for drop in (0, 1) for mode in (0, 1, 2)}
    assert set(meta) == want, sorted(set(meta) ^ want)


@pytest.mark.parametrize("drop,mode", ZERO, ids=[f"drop{d}-mode{m}" for d, m in ZERO])
def test_backward_with_32_row_waves_at_d192_uses_no_scratch(meta, drop, mode):
    m = meta[("bwd", 192, 7, 2, drop, mode)]
    print(f"ffn_chain_bwd_kernel<192, 7, 2, {bool(drop)}, {mode}>: {m}")
    assert m["scratch"] == 0 and m["vspill"] == 0, m
    assert m["vgpr"] <= 256, m


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_forward_with_dropout_is_no_worse(meta, mode):
    m, before = meta[("fwd", 192, 7, 2, 1, mode)], FWD_UNCHANGED[mode]
    print(f"ffn_chain_fwd_kernel<192, 7, 2, True, {mode}>: {m}")
    assert all(m[k] <= before[k] for k in before), (m, before)
    assert m["vgpr"] <= 256


def test_instances_without_scratch_keep_none(meta):
    with_scratch_before = {("bwd", 192, 7, 2, d, m) for d in (0, 1) for m in (0, 1, 2)} | {("fwd", 192, 7, 2, 1, m) for m in (0, 1, 2)}
    bad = {k: v for k, v in meta.items() if k not in with_scratch_before and (v["scratch"] or v["vspill"])}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in meta.values())


@pytest.mark.parametrize("drop", [0, 1])
def test_backward_with_the_qkv_gradient_in_front_is_no_worse(meta, drop):
    m, before = meta[("bwd", 192, 7, 2, drop, 2)], BWD_MODE2_BEFORE[drop]
    print(f"ffn_chain_bwd_kernel<192, 7, 2, {bool(drop)}, 2>: {m}")
    assert all(m[k] <= before[k] for k in before), (m, before)
    assert m["vgpr"] <= 256
