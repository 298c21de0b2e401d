"""CPU: the relevance read-back's C ABI (exported symbols, ctypes argument counts against include/iqvit.h), the argument
validation of vit_vs_raw_iq_amd.relevance (raised before any device work), and the gfx950 ISA of the new kernels."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")
NEW = ("iq_attn_grad_probs", "iq_attn_relevance_step", "iq_model_attention_relevance")


def test_new_symbols_are_exported_with_the_header_argument_counts():
    import ctypes
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b%s\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    N.lib()


def test_package_exports():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import relevance
    assert P.attention_relevance is relevance.attention_relevance
    assert P.grad_attention_maps is relevance.grad_attention_maps
    assert {"attention_relevance", "grad_attention_maps"} <= set(P.__all__)


def vit(**kw):
    import vit_vs_raw_iq_amd as P
    g = dict(in_channels=1, img_size_h=32, img_size_w=32, patch_size=16, num_classes=11, d_model=64, n_head=4, n_layers=2,
             ffn_hidden=128)
    g.update(kw)
    return P.AMCTransformerViT(drop_prob=0.0, device="cpu", **g)


def rawiq(**kw):
    import vit_vs_raw_iq_amd as P
    g = dict(in_channels=2, seq_length=512, num_classes=5, d_model=64, n_head=4, n_layers=1, ffn_hidden=128,
             use_cls_token=True, embedding_type="segment", segment_size=32)
    g.update(kw)
    return P.AMCTransformerRawIQ(drop_prob=0.0, device="cpu", **g)


def test_argument_errors_are_raised_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import attention_relevance, grad_attention_maps
    m = vit()
    x = torch.randn(2, 1, 32, 32)
    # target: range, dtype, shape
    for fn in (attention_relevance, grad_attention_maps):
        for t in (11, -1, torch.tensor([0, 11]), torch.tensor([-1, 0])):
            with pytest.raises(ValueError):
                fn(m, x, target=t)
        for t in (torch.tensor([0.0, 1.0]), torch.tensor([True, False]), True):
            with pytest.raises(TypeError):
                fn(m, x, target=t)
        for t in (torch.tensor([0, 1, 2]), torch.zeros(2, 1, dtype=torch.int64)):
            with pytest.raises(ValueError):
                fn(m, x, target=t)
        with pytest.raises(ValueError):
            fn(m, x, batch=0)
        with pytest.raises(ValueError):
            fn(m, torch.randn(2, 32, 32))                         # wrong rank: the model's own _expect
        with pytest.raises(P.IqError):
            fn(m, x)                                              # a CPU tensor raises as model(x) does
        with pytest.raises(TypeError):
            fn(torch.nn.Linear(2, 2), x)
        with pytest.raises(TypeError):
            fn(m.encoder, x)                                      # no logits: no class to ask about
    # query / heads / layers / positive
    for kw in (dict(query="row"), dict(heads="max"), dict(layers=[2]), dict(layers=[-1]), dict(layers=[0, 0]), dict(layers=[]),
               dict(positive=1)):
        with pytest.raises((ValueError, TypeError)):
            grad_attention_maps(m, x, **kw)
    nocls = rawiq(use_cls_token=False)
    xr = torch.randn(2, 2, 512)
    with pytest.raises(ValueError, match="CLS"):
        grad_attention_maps(nocls, xr)                            # query="cls" is the default
    with pytest.raises(P.IqError):
        grad_attention_maps(nocls, xr, query="mean")
    with pytest.raises(P.IqError):
        attention_relevance(nocls, xr)
    # nothing reached the native plan: no plan built, parameters still on the CPU
    for mod in (m, nocls):
        assert mod._plan is None and mod.encoder._plan is None
        assert all(not p.is_cuda for p in mod.parameters())


def test_relevance_kernels_use_no_scratch_and_do_not_spill():
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-S", "--cuda-device-only", os.path.join(csrc, "attn_maps.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
        name, scratch, vgpr, spill = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        if "attn_grad_probs_kernel" in name or "attn_relevance_step_kernel" in name:
            seen.add(name)
            assert scratch == 0 and spill == 0, (name, scratch, vgpr, spill)
    assert len(seen) == 6, sorted(seen)
