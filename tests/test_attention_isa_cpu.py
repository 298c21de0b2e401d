"""CPU: register and scratch budget of the two attention kernels of the ViT step, read from the kernel metadata of the
gfx950 code object (hipcc cross-compiles without a GPU).  Only the metadata is read, never the instruction text.

attn_bwd_once_kernel<1024> is launched with 1,024 threads, 16 waves = 4 per SIMD, so a wave may hold 512 / 4 = 128 VGPRs
(the launch fails above that).  With phase A as a strided loop over units it sat AT that cap with 12 registers spilled to
52 B of scratch per lane, which cost 3 us of its 65 us (profiles/attn_loads.txt); as one unit per wave it needs 118 and
no scratch.  attn_fwd_kernel<64, false> runs two 8-wave workgroups per CU (2 x 71,680 B of LDS at S = 197), again
4 waves per SIMD: above 128 VGPRs the second workgroup no longer fits.  Found when this test was written: 118 VGPRs
(once kernel), 109 (forward), scratch 0 for both.
"""
import os
import re
import subprocess
import tempfile

from conftest import ROOT

ONCE = "attn_bwd_once_kernelILi1024EE"
FWD = "attn_fwd_kernelILi64ELb0EE"


def kernel_metadata():
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    try:
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                               "-S", "--cuda-device-only", os.path.join(csrc, "attention.hip"), "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        os.unlink(out)
    text = text[text.index("amdhsa.kernels:"):]
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
        meta[m.group(1)] = dict(scratch=int(m.group(2)), vgpr=int(m.group(3)), spill=int(m.group(4)))
    return meta


def test_vit_attention_kernels_keep_their_registers_and_no_scratch():
    meta = kernel_metadata()
    once = [v for k, v in meta.items() if ONCE in k]
    fwd = [v for k, v in meta.items() if FWD in k]
    assert len(once) == 1 and len(fwd) == 1, sorted(meta)
    print(f"attn_bwd_once_kernel<1024>: {once[0]}   attn_fwd_kernel<64, false>: {fwd[0]}")
    assert once[0]["vgpr"] <= 128, once[0]
    assert once[0]["scratch"] == 0 and once[0]["spill"] == 0, once[0]
    assert fwd[0]["scratch"] == 0 and fwd[0]["spill"] == 0, fwd[0]
    # 512 VGPRs per SIMD lane / (2 workgroups x 2 waves per SIMD)
    assert fwd[0]["vgpr"] <= 128, f"attn_fwd_kernel<64, false> no longer fits two workgroups per CU: {fwd[0]}"
