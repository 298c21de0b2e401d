"""CPU: the input-gradient C ABI (exported symbols, ctypes argument counts against include/iqvit.h), the argument checks of
iq_embed_dgrad / iq_model_backward_input / iq_linf_step that return before any HIP call, the argument validation of
vit_vs_raw_iq_amd.saliency / adversarial (raised before any device work), and the gfx950 ISA of the new kernels."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iqvit.h")
NEW = ("iq_embed_dgrad", "iq_linf_step", "iq_model_backward_input")


def test_new_symbols_are_exported_with_the_header_argument_counts():
    import vit_vs_raw_iq_amd._native as N
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b%s\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define IQ_BWD_PARAM_GRADS 1\b", src) and N.BWD_PARAM_GRADS == 1
    N.lib()


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) // 16 * 16          # 16 B aligned host address: never dereferenced on these paths
    ARG = 1
    # iq_embed_dgrad(demb, w, Kpad, dsrc, kind, B, C, H, W, p, D, stream)
    assert L.iq_embed_dgrad(a, a, 256, a, 2, 1, 1, 32, 32, 16, 128, None) == ARG        # bad kind
    assert L.iq_embed_dgrad(a, a, 224, a, 0, 1, 1, 32, 32, 16, 128, None) == ARG        # Kpad < P = 256
    assert L.iq_embed_dgrad(a, a, 252, a, 0, 1, 1, 32, 32, 16, 128, None) == ARG        # Kpad % 8
    assert L.iq_embed_dgrad(None, a, 256, a, 0, 1, 1, 32, 32, 16, 128, None) == ARG
    assert L.iq_embed_dgrad(a, None, 256, a, 0, 1, 1, 32, 32, 16, 128, None) == ARG
    assert L.iq_embed_dgrad(a, a, 256, None, 0, 1, 1, 32, 32, 16, 128, None) == ARG
    assert L.iq_embed_dgrad(a, a, 256, a, 0, 1, 1, 32, 32, 16, 124, None) == ARG        # D % 8
    assert L.iq_embed_dgrad(a, a, 256, a, 0, 1, 1, 32, 0, 16, 128, None) == ARG         # kind 0 needs W
    assert L.iq_embed_dgrad(a, a, 256, a, 0, 1, 1, 8, 32, 16, 128, None) == ARG         # no whole patch
    assert L.iq_embed_dgrad(a + 2, a, 256, a, 0, 1, 1, 32, 32, 16, 128, None) == ARG    # misaligned demb
    assert L.iq_embed_dgrad(a, a, 32, a, 1, 1, 2, 1024, 0, 32, 128, None) == ARG        # kind 1: Kpad < P = 64
    assert L.iq_embed_dgrad(a, a, 256, a, 0, 0, 1, 32, 32, 16, 128, None) == 0          # no frames: nothing to do
    nan = float("nan")
    # iq_linf_step(x, g, x0, alpha, eps, lo, hi, n, stream)
    assert L.iq_linf_step(None, a, a, 0.1, 0.1, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, None, a, 0.1, 0.1, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, a, None, 0.1, 0.1, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, a, a, -0.1, 0.1, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, a, a, 0.1, nan, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, a, a, 0.1, math.inf, nan, nan, 4, None) == ARG
    assert L.iq_linf_step(a, a, a, 0.1, 0.1, 1.0, 0.0, 4, None) == ARG                  # lo > hi
    assert L.iq_linf_step(a, a, a, 0.1, 0.1, nan, nan, 0, None) == 0


def test_model_backward_input_refuses_before_any_hip_call():
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    cfg = N.ModelCfg(kind=0, in_channels=1, img_h=32, img_w=32, patch=16, seq_length=0, conv_k=0, use_cls=1, num_classes=11,
                     d_model=128, n_head=8, n_layers=2, ffn_hidden=512, drop_prob=0.0)
    h = ctypes.c_void_p()
    assert L.iq_model_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        buf = ctypes.create_string_buffer(1024)
        a = ctypes.addressof(buf)
        assert L.iq_model_backward_input(None, a, None, 2, a, 1024, a, 0, None) == 1
        assert L.iq_model_backward_input(h, a, None, 2, a, 1024, a, 2, None) == 1
        assert b"unknown flags" in L.iq_model_last_error(h)
        assert L.iq_model_backward_input(h, a, None, 2, a, 1024, None, 0, None) == 1
        assert b"dsrc" in L.iq_model_last_error(h)
        assert L.iq_model_backward_input(h, None, None, 2, a, 1024, a, 0, None) == 1
        assert L.iq_model_backward_input(h, a, None, 2, a, 1024, a, 0, None) == 1
        assert b"not bound" in L.iq_model_last_error(h)
    finally:
        L.iq_model_destroy(h)


def vit(**kw):
    import vit_vs_raw_iq_amd as P
    g = dict(in_channels=1, img_size_h=32, img_size_w=32, patch_size=16, num_classes=11, d_model=64, n_head=4, n_layers=2,
             ffn_hidden=128)
    g.update(kw)
    return P.AMCTransformerViT(drop_prob=0.0, device="cpu", **g)


def test_saliency_and_attack_argument_errors_are_raised_before_any_device_work():
    import vit_vs_raw_iq_amd as P
    from vit_vs_raw_iq_amd import fgsm, input_gradient, integrated_gradients, pgd, robustness_curve
    m = vit()
    x = torch.randn(2, 1, 32, 32)
    y = torch.tensor([1, 2])
    bad = [
        (ValueError, input_gradient, (m, x), dict(target=11)),
        (ValueError, input_gradient, (m, x), dict(target=torch.tensor([0, -1]))),
        (ValueError, input_gradient, (m, x), dict(target=torch.tensor([0, 1, 2]))),
        (TypeError, input_gradient, (m, x), dict(target=torch.tensor([0.5, 1.0]))),
        (ValueError, input_gradient, (m, x), dict(loss="ce")),
        (ValueError, input_gradient, (m, x), dict(loss="mse")),
        (ValueError, input_gradient, (m, x), dict(labels=y, target=1)),
        (ValueError, input_gradient, (m, x), dict(labels=y, loss="logit")),
        (ValueError, input_gradient, (m, x), dict(batch=0)),
        (ValueError, input_gradient, (m, torch.randn(2, 32, 32)), {}),
        (ValueError, integrated_gradients, (m, x), dict(steps=0)),
        (ValueError, integrated_gradients, (m, x), dict(baseline=torch.zeros(3, 1, 32, 32))),
        (TypeError, integrated_gradients, (m, x), dict(baseline=0.0)),
        (ValueError, fgsm, (m, x, y, -0.1), {}),
        (ValueError, fgsm, (m, x, y, float("nan")), {}),
        (ValueError, fgsm, (m, x, torch.tensor([1, 11]), 0.1), {}),
        (ValueError, fgsm, (m, x, y, 0.1), dict(clip=(1.0, 0.0))),
        (ValueError, fgsm, (m, x, y, 0.1), dict(clip=3.0)),
        (ValueError, pgd, (m, x, y, 0.1, 0.01, 0), {}),
        (ValueError, pgd, (m, x, y, 0.1, -0.01, 3), {}),
        (ValueError, robustness_curve, (m, x, y, [0.0]), dict(attack="cw")),
        (ValueError, robustness_curve, (m, x, y, [0.1, -1.0]), {}),
        (TypeError, robustness_curve, (m, x, y, [0.1]), dict(steps=3)),          # fgsm takes no steps
        (TypeError, input_gradient, (m.encoder, x), {}),                          # no logits
        (TypeError, fgsm, (torch.nn.Linear(2, 2), x, y, 0.1), {}),
    ]
    for exc, fn, args, kw in bad:
        with pytest.raises(exc):
            fn(*args, **kw)
    # a CPU tensor raises as model(x) does
    for fn, args in ((input_gradient, (m, x)), (integrated_gradients, (m, x)), (fgsm, (m, x, y, 0.1)),
                     (pgd, (m, x, y, 0.1, 0.01, 2)), (robustness_curve, (m, x, y, [0.0]))):
        with pytest.raises(P.IqError):
            fn(*args)
    assert m._plan is None and m.encoder._plan is None                             # nothing reached the native plan
    assert all(not p.is_cuda for p in m.parameters())


def test_input_gradient_kernels_use_no_scratch_and_do_not_spill():
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    seen = {}
    for src in ("embed_dgrad.hip", "misc.hip"):
        out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                               "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
        os.unlink(out)
        for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                             text, re.S):
            name, scratch, vgpr, spill = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
            if "embed_dgrad" in name or "linf_step_kernel" in name:
                seen[name] = (scratch, spill)
                assert scratch == 0 and spill == 0, (name, scratch, vgpr, spill)
    assert sum("embed_dgrad_mfma_kernel" in n for n in seen) == 4
    assert sum("embed_dgrad_valu_kernel" in n for n in seen) == 4
    assert sum("linf_step_kernel" in n for n in seen) == 1
