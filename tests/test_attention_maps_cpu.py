"""CPU: the attention read-back's C ABI (exported symbols, ctypes argument counts against include/iqvit.h), the argument
validation of vit_vs_raw_iq_amd.attention_maps (raised before any device work), rollout_to_input's geometry against a numpy
statement of the patch / segment layout, and the gfx950 ISA of the new kernels."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")
NEW = ("iq_attn_probs", "iq_model_attention", "iq_model_attention_rollout")


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
    from vit_vs_raw_iq_amd import attention_maps, attention_rollout
    m = vit()
    x = torch.randn(2, 1, 32, 32)
    for kw in (dict(query="row"), dict(heads="max"), dict(layers=[2]), dict(layers=[-1]), dict(batch=0)):
        with pytest.raises(ValueError):
            attention_maps(m, x, **kw)
    with pytest.raises(ValueError):
        attention_maps(m, torch.randn(2, 32, 32))                 # wrong rank: the model's own _expect
    with pytest.raises(P.IqError):
        attention_maps(m, x)                                      # a CPU tensor raises as model(x) does
    with pytest.raises(P.IqError):
        m(x)
    with pytest.raises(ValueError):
        attention_rollout(m, x, alpha=1.5)
    with pytest.raises(P.IqError):
        attention_rollout(m, x)
    with pytest.raises(TypeError):
        attention_maps(torch.nn.Linear(2, 2), x)
    nocls = rawiq(use_cls_token=False)
    xr = torch.randn(2, 2, 512)
    with pytest.raises(ValueError, match="CLS"):
        attention_maps(nocls, xr)                                 # query="cls" is the default
    with pytest.raises(ValueError, match="CLS"):
        attention_maps(nocls.encoder, xr, query="cls")
    with pytest.raises(P.IqError):
        attention_maps(nocls, xr, query="mean")
    # nothing reached the native plan: no plan built, parameters still on the CPU
    for mod in (m, nocls):
        assert mod._plan is None and mod.encoder._plan is None
        assert all(not p.is_cuda for p in mod.parameters())
    enc = rawiq().encoder
    enc._parent_ref = None                                        # a stand-alone encoder
    with pytest.raises(ValueError):
        attention_maps(enc, xr, layers=[1])
    assert enc._plan is None


def expected_vit(roll, H, W, p):
    gh, gw = H // p, W // p
    out = np.zeros((roll.shape[0], H, W), np.float32)
    for t in range(gh * gw):                       # tokens in row-major patch-grid order (oracle.embed)
        gy, gx = divmod(t, gw)
        out[:, gy * p:(gy + 1) * p, gx * p:(gx + 1) * p] = roll[:, 1 + t, None, None]
    return out


@pytest.mark.parametrize("H,W,p", [(32, 64, 4), (32, 64, 16), (224, 224, 16), (36, 40, 16)])
def test_rollout_to_input_vit_geometry(H, W, p):
    from vit_vs_raw_iq_amd import rollout_to_input
    m = vit(img_size_h=H, img_size_w=W, patch_size=p)
    S = (H // p) * (W // p) + 1
    roll = torch.rand(3, S, generator=torch.Generator().manual_seed(S))
    got = rollout_to_input(m, roll)
    assert got.shape == (3, H, W)
    np.testing.assert_array_equal(got.numpy(), expected_vit(roll.numpy(), H, W, p))
    np.testing.assert_array_equal(rollout_to_input(m.encoder, roll).numpy(), got.numpy())


def test_rollout_to_input_vit_token_order_is_the_patch_embedding_order():
    """A token's value lands on the pixels the patch embedding (oracle.embed) reads for that token."""
    import iq_oracle as O
    from vit_vs_raw_iq_amd import rollout_to_input
    H, W, p = 32, 64, 4
    cfg = O.OracleConfig(kind="vit", img_size_h=H, img_size_w=W, patch_size=p, d_model=16, n_head=1)
    S = (H // p) * (W // p) + 1
    roll = torch.arange(S, dtype=torch.float32)[None] + 1.0
    img = rollout_to_input(vit(img_size_h=H, img_size_w=W, patch_size=p), roll)
    sd = {"encoder.patch_embedding.projection.weight": torch.ones(1, 1, p, p) / (p * p),
          "encoder.patch_embedding.projection.bias": torch.zeros(1)}
    cfg.d_model = 1
    tok = O.embed(cfg, sd, img[:, None])                          # mean over each patch
    np.testing.assert_allclose(tok[0, :, 0].numpy(), roll[0, 1:].numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("cls", [True, False])
def test_rollout_to_input_rawiq_segment(cls):
    from vit_vs_raw_iq_amd import rollout_to_input
    m = rawiq(use_cls_token=cls, seq_length=1024, segment_size=16)
    S = 64 + int(cls)
    roll = torch.rand(2, S, generator=torch.Generator().manual_seed(1))
    got = rollout_to_input(m, roll).numpy()
    r = roll.numpy()[:, 1:] if cls else roll.numpy()
    exp = np.zeros((2, 1024), np.float32)
    for t in range(64):
        exp[:, t * 16:(t + 1) * 16] = r[:, t, None]
    np.testing.assert_array_equal(got, exp)
    with pytest.raises(ValueError):
        rollout_to_input(m, roll[:, :-1])


def test_rollout_to_input_rawiq_conv1d():
    from vit_vs_raw_iq_amd import rollout_to_input
    m = rawiq(seq_length=1024, embedding_type="conv1d")
    roll = torch.rand(2, 1025, generator=torch.Generator().manual_seed(2))
    got = rollout_to_input(m, roll)
    assert got.shape == (2, 1024)
    np.testing.assert_array_equal(got.numpy(), roll.numpy()[:, 1:])


def test_attention_map_kernels_use_no_scratch_and_do_not_spill():
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-S", "--cuda-device-only", os.path.join(csrc, "attn_maps.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
        name, scratch, vgpr, spill = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        if "attn_probs_kernel" in name or "attn_rollout_kernel" in name:
            seen += 1
            assert scratch == 0 and spill == 0, (name, scratch, vgpr, spill)
    assert seen == 6
