"""What the GPU suites of the front ends, generators, receiver and symbol-rate stages share (tests/test_gpu_spectrogram.py,
test_gpu_cyclic.py, test_gpu_cyclic_bwd.py, test_gpu_constellation.py, test_gpu_carrier.py, test_gpu_equaliser.py,
test_gpu_likelihood.py, ...): device helpers, guarded buffers (float32 and int32), and one guarded call through the C ABI of a
frame kernel.  A plain helper module like the *_ref.py files beside it."""
import ctypes

import numpy as np
import torch

from prof_names import kernel_launches

GUARD = 64                     # floats in front of and behind every buffer (256 bytes: keeps the 16-byte alignment)
SENTINEL = -12345.5
ISENT = -77777                 # the guard and the sentinel of an int32 buffer


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


def guarded_int(a, fill=ISENT):
    """guarded() for int32."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    buf = torch.full((a.size + 2 * GUARD,), fill, dtype=torch.int32, device=dev())
    buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).to(dev())
    return buf, buf[GUARD:GUARD + a.size]


def int_guards_intact(buf, fill=ISENT):
    return bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == fill).all())


def abi_call(entry, launches, inputs, outs, n, length, par, expect_kernel=True, side=()):
    """One call of the C entry point `entry`(*inputs, *outs, n, length, &par, stream).  inputs: numpy arrays in the ABI's order,
    int32 as it is and everything else as float32.  side: the arrays the struct points to (None: none), laid out like the inputs;
    `par` is then a function of their device addresses (None: NULL) -> the struct.  outs: one shape, for one float32 output,
    returned bare; or a list in the ABI's order of shapes (float32), (numpy.int32, *shape) and None (passed as NULL), returned as
    a list (None for None).  Every input lies between guards (NaN, ISENT), every output between sentinels (SENTINEL, ISENT) and
    is pre-filled with the sentinel.  With expect_kernel the call must launch exactly `launches`, a {kernel name: count} or one
    name for {name: 1}.  Afterwards the guards of EVERY buffer of the call must be intact, and the inputs and side arrays must
    hold the bits they held: nothing but the outputs is written."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()

    def lay(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        a = a if a.dtype == np.int32 else a.astype(np.float32)
        return (guarded_int(a) if a.dtype == np.int32 else guarded(a, np.nan)) + (a,)

    def room(o):
        if o is None:
            return None
        if o[0] is np.int32:
            return guarded_int(np.full(o[1:], ISENT)) + (o[1:],)
        return guarded(np.full(o, SENTINEL), SENTINEL) + (o,)
    ins, sides = [lay(a) for a in inputs], [lay(a) for a in side]
    obs = [room(o) for o in ([outs] if isinstance(outs, tuple) else outs)]
    if not isinstance(par, ctypes.Structure):
        par = par(*(None if b is None else b[1].data_ptr() for b in sides))

    def run():
        N.check(getattr(L, entry)(*(b[1].data_ptr() for b in ins), *(None if b is None else b[1].data_ptr() for b in obs), n, length,
                                  ctypes.byref(par), N.stream_handle()), entry)
    if expect_kernel:
        assert kernel_launches(L, run) == ({launches: 1} if isinstance(launches, str) else launches)
    else:
        run()
    torch.cuda.synchronize()
    for buf, view, _ in filter(None, obs):
        assert int_guards_intact(buf) if buf.dtype == torch.int32 else guards_intact(buf, SENTINEL)
    for buf, view, a in filter(None, ins + sides):
        assert int_guards_intact(buf) if buf.dtype == torch.int32 else guards_intact(buf, np.nan)
        assert np.array_equal(view.cpu().numpy().view(np.int32), a.reshape(-1).view(np.int32))
    res = [None if b is None else b[1].cpu().numpy().reshape(b[2]) for b in obs]
    return res[0] if isinstance(outs, tuple) else res
