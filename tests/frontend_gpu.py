"""What the GPU suites of the front ends, generators and receiver share (tests/test_gpu_spectrogram.py, test_gpu_cyclic.py,
test_gpu_cyclic_bwd.py, test_gpu_constellation.py, ...): device helpers, guarded buffers, and one guarded call through the C ABI
of a frame kernel.  A plain helper module like the *_ref.py files beside it."""
import ctypes

import numpy as np
import torch

from prof_names import kernel_launches

GUARD = 64                     # floats in front of and behind every buffer (256 bytes: keeps the 16-byte alignment)
SENTINEL = -12345.5


def dev():
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def on_device(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dev())                  # a copy: x may be read-only


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded(a, fill):
    """A copy of `a` on the device between two guards of `fill` -> (whole buffer, the part that holds a)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * GUARD,), fill, dtype=torch.float32, device=dev())
    buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).to(dev())
    return buf, buf[GUARD:GUARD + a.size]


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu().numpy()
    return bool(np.all(np.isnan(g))) if np.isnan(fill) else bool(np.all(g == np.float32(fill)))


def small_vit(in_channels, h, w):
    import vit_vs_raw_iq_amd as P
    torch.manual_seed(3)
    return P.AMCTransformerViT(in_channels=in_channels, img_size_h=h, img_size_w=w, patch_size=16, num_classes=4, d_model=128,
                               n_head=8, n_layers=2, ffn_hidden=512, drop_prob=0.0, device="cuda").to(dev()).eval()


def abi_call(entry, kernel_name, inputs, out_shape, n, length, par, expect_kernel=True):
    """One call of the C entry point `entry`(*inputs, out, n, length, &par, stream) -> out as numpy of `out_shape`.  Every input
    (numpy, in the ABI's order) lies between NaN guards, the output between sentinels and is pre-filled with the sentinel.  With
    expect_kernel the call must launch `kernel_name` once and nothing else.  Afterwards the guards of EVERY buffer of the call
    must be intact, and the inputs must hold what they held: nothing but the output is written."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    ins = [guarded(a, np.nan) for a in inputs]
    ob, ov = guarded(np.full(out_shape, SENTINEL), SENTINEL)

    def run():
        N.check(getattr(L, entry)(*(v.data_ptr() for _, v in ins), ov.data_ptr(), n, length, ctypes.byref(par),
                                  N.stream_handle()), entry)
    if expect_kernel:
        assert kernel_launches(L, run) == {kernel_name: 1}
    else:
        run()
    torch.cuda.synchronize()
    assert guards_intact(ob, SENTINEL)
    for (buf, view), a in zip(ins, inputs):
        assert guards_intact(buf, np.nan)
        assert np.array_equal(bits(view.cpu().numpy()), bits(a).reshape(-1))
    return ov.cpu().numpy().reshape(out_shape)
