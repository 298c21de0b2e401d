"""Which kernels ran: the names the launch sites recorded (IQ_PROF_K), read back through iq_prof_kernels.  The records are
sums per name, listed in the order in which the process first saw each name -- not in launch order."""
import ctypes as C

import torch


def kernel_launches(L, fn):
    """{kernel name: launches} of the kernels the launch sites recorded while fn() ran."""
    ms = (C.c_double * 8)()
    cnt = (C.c_longlong * 8)()
    torch.cuda.synchronize()
    L.iq_prof_enable(1)
    L.iq_prof_collect(ms, cnt)
    L.iq_prof_kernels(None, 0, 1)
    try:
        fn()
        L.iq_prof_collect(ms, cnt)
    finally:
        L.iq_prof_enable(0)
    need = L.iq_prof_kernels(None, 0, 0)
    buf = C.create_string_buffer(need + 1)
    L.iq_prof_kernels(buf, need + 1, 1)
    return {f[0]: int(f[2]) for f in (line.split("\t") for line in buf.value.decode().splitlines())}


def kernels_of(L, fn):
    """Names of the kernels the launch sites recorded while fn() ran."""
    return list(kernel_launches(L, fn))
