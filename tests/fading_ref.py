"""What tests/test_fading_cpu.py and tests/test_gpu_fading.py share: the arithmetic of iq_frames_fade (include/iqvit.h) restated in
fp32 for the cases that are exact, an fp64 restatement that is independent of vit_vs_raw_iq_amd.fading_reference (and can move one
tap's fractional phase to f + 1), a running-error bound for the cases with real tables, and the cases themselves.

The bound, per component of y[n], with u = 2^-24 (fp32 rounding) and E = 2^-23 (sincospif: documented maximum error 2 ulp, of a
value of at most 1):
  r_l   a product and K - 1 fmaf:                 dr <= K u sum_k |x_k| |w_k|                 (gamma_K to first order)
  g_l   NS + 1 fmaf of amp (c + dc), |dc| <= E:   dg <= (E + (NS + 1) u) sum_s |amp_s|
  t_l = rot(r_l, g_l), two roundings a component: dt <= (|g.re| + |g.im|) dr + (|r.re| + |r.im|) dg + 2 u (|r.re| + |r.im|)(|g.re| + |g.im|)
  y     L additions from +0:                      dy <= sum_l dt_l + L u sum_l (|r.re| + |r.im|)(|g.re| + |g.im|)
all magnitudes taken from the fp64 definition, times 1.01 for the second-order terms (products of two of the above are below
2^-40 of the magnitudes).  The conversion of the integer phase to fp32 belongs to the definition (both sides convert alike), so
it is no error.  The bound is for normalise = 0: the scaling is the generators' own tail."""
import numpy as np

U = 2.0 ** -24
E_SINCOS = 2.0 ** -23
SLOTS = (8, 33)
_COS = np.array([1.0, 0.0, -1.0, 0.0])
_SIN = np.array([0.0, 1.0, 0.0, -1.0])


def _positions(clock, n_out, delay_q16, n_frac):
    n = np.arange(n_out, dtype=np.int64)
    Q = int(clock[0]) + n * int(clock[1]) - (int(delay_q16) << 16)
    return Q >> 32, ((Q & 0xFFFFFFFF) * n_frac) >> 32


def _window(z, m, K, length_in):
    """x[m + k - c], zero outside the frame -> (n_out, K)"""
    idx = m[:, None] + np.arange(K, dtype=np.int64)[None, :] - (K - 1) // 2
    ok = (idx >= 0) & (idx < length_in)
    return np.where(ok, z[np.clip(idx, 0, length_in - 1)], 0.0)


def _phase_x(path, n_out):
    """(phase + n inc) mod 2^32 as int32 -> (the integer, x = fp32(p) 2^-31 in fp64)"""
    n = np.arange(n_out, dtype=np.int64)
    p = (int(path[0]) + n * int(path[1])) & 0xFFFFFFFF
    p = np.where(p >= 2 ** 31, p - 2 ** 32, p)
    return p, p.astype(np.float32).astype(np.float64) * 2.0 ** -31


def _e(path, n_out):
    """e(p) in fp64; exactly (1,0), (0,1), (-1,0), (0,-1) where p is a multiple of a quarter turn, as sincospif gives it"""
    p, x = _phase_x(path, n_out)
    c, s = np.cos(np.pi * x), np.sin(np.pi * x)
    q = (p % 2 ** 30) == 0
    k = (p >> 30) & 3
    return np.where(q, _COS[k], c), np.where(q, _SIN[k], s)


def fma32(a, b, c):
    """fmaf for fp32 arrays: the product is exact in fp64; one rounding to fp64 and one to fp32 (the same bits as fmaf wherever
    the fp64 sum is exact, which it is in every exact case)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def restate32(x, paths, amps, clock, fd):
    """iq_frames_fade without normalisation and noise, operation by operation in fp32 -> float32 (B, length_out, 2)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    tab = np.asarray(fd.interp, f32)
    B, No = len(x), fd.length_out
    out = np.zeros((B, No, 2), f32)
    for i in range(B):
        yr, yi = np.zeros(No, f32), np.zeros(No, f32)
        for l in range(fd.taps):
            m, f = _positions(clock[i], No, fd.delay_q16[l], fd.n_frac)
            wr, wi = _window(x[i, :, 0], m, fd.K, fd.length_in).astype(f32), _window(x[i, :, 1], m, fd.K, fd.length_in).astype(f32)
            w = tab[f]
            rr, ri = wr[:, 0] * w[:, 0], wi[:, 0] * w[:, 0]
            for k in range(1, fd.K):
                rr, ri = fma32(wr[:, k], w[:, k], rr), fma32(wi[:, k], w[:, k], ri)
            gr, gi = np.zeros(No, f32), np.zeros(No, f32)
            for s in range(fd.sinusoids + 1):
                a = f32(amps[i, l, s])
                if a == 0:
                    continue
                c, sn = _e(paths[i, l, s], No)
                av = np.full(No, a, f32)
                gr, gi = fma32(av, c.astype(f32), gr), fma32(av, sn.astype(f32), gi)
            tx = fma32(rr, gr, -(ri * gi))
            ty = fma32(rr, gi, ri * gr)
            yr, yi = yr + tx, yi + ty
        out[i, :, 0], out[i, :, 1] = yr, yi
    return out


def definition64(x, paths, amps, clock, fd, bump_tap=None):
    """The definition in fp64 (no normalisation) -> (y complex128 (B, length_out), bound float64 (B, length_out)): the bound of the
    module docstring for each component.  bump_tap: that tap reads its table at min(f + 1, n_frac - 1) instead of f: a definition
    that is wrong by one fractional phase."""
    x = np.asarray(x, np.float64)
    tab = np.asarray(fd.interp, np.float64)
    B, No, L, NS, K = len(x), fd.length_out, fd.taps, fd.sinusoids, fd.K
    y = np.zeros((B, No), np.complex128)
    bound = np.zeros((B, No))
    for i in range(B):
        z = x[i, :, 0] + 1j * x[i, :, 1]
        mags = np.zeros(No)
        for l in range(L):
            m, f = _positions(clock[i], No, fd.delay_q16[l], fd.n_frac)
            if bump_tap == l:
                f = np.minimum(f + 1, fd.n_frac - 1)
            win = _window(z, m, K, fd.length_in)
            r = (win * tab[f]).sum(axis=1)
            dr = K * U * (np.maximum(np.abs(win.real), np.abs(win.imag)) * np.abs(tab[f])).sum(axis=1)
            g = np.zeros(No, np.complex128)
            asum = 0.0
            for s in range(NS + 1):
                a = float(amps[i, l, s])
                if a == 0.0:
                    continue
                c, sn = _e(paths[i, l, s], No)
                g += a * (c + 1j * sn)
                asum += abs(a)
            dg = (E_SINCOS + (NS + 1) * U) * asum
            r1, g1 = np.abs(r.real) + np.abs(r.imag), np.abs(g.real) + np.abs(g.imag)
            bound[i] += g1 * dr + r1 * dg + 2 * U * r1 * g1
            mags += r1 * g1
            y[i] += g * r
        bound[i] += L * U * mags
    return y, 1.01 * bound


def clock_of(start_q32, drift, B=1):
    return np.tile(np.array([start_q32, 2 ** 32 + drift], np.int64), (B, 1))


def tables(B):
    return np.zeros((B,) + SLOTS + (2,), np.int64), np.zeros((B,) + SLOTS, np.float32)


def integer_frames(rng, B, length):
    x = rng.integers(-8, 9, size=(B, length, 2)).astype(np.float32)
    x[x == 0] = 1.0                                # no zeros: a negative zero has nothing to come from
    return x


def exact_cases():
    """name -> (Fading kwargs, x, paths, amps, clock): integer frames, integer interpolation tables, integer amplitudes, phases and
    increments that are multiples of a quarter turn: every operation of the kernel is exact in fp32.  The edges the issue lists:
    len_out 1, 2, 255, 256, 257 and an odd 1001; len_in != len_out; positions off both ends; K 1, 2, 16; n_frac 1 and 256 with the
    last phase hit; negative, zero and positive drift; delays 0 and fractional; 1 and 8 taps; NS 0, 1, 32; a zero-amplitude slot
    of junk."""
    rng = np.random.default_rng(20261021)
    Q = 2 ** 30                                    # a quarter turn
    cases = {}

    def add(name, len_in, len_out, taps, ns, K, n_frac, delay, start_q32, drift, B=2):
        table = rng.integers(-3, 4, size=(n_frac, K)).astype(np.float32)
        kw = dict(length_in=len_in, length_out=len_out, taps=taps, sinusoids=ns, K=K, n_frac=n_frac, delay=delay, normalise=False,
                  interp=table)
        x = integer_frames(rng, B, len_in)
        paths, amps = tables(B)
        paths[..., 0] = rng.integers(-2, 2, size=paths.shape[:-1]) * Q          # junk everywhere: only used slots may matter
        paths[..., 1] = rng.integers(-2, 2, size=paths.shape[:-1]) * Q
        amps[:] = rng.integers(-3, 4, size=amps.shape)
        amps[:, :taps, 0][amps[:, :taps, 0] == 0] = 2.0                         # every tap has a line of sight
        if ns >= 1:
            amps[:, 0, 1] = 0.0                                                 # the zero-amplitude slot ...
            paths[:, 0, 1] = (0x7FC00000, -0x00400001)                          # ... holding a NaN's worth of junk
        cases[name] = (kw, x, paths, amps, clock_of(start_q32, drift, B))
    add("len1", 5, 1, 1, 0, 1, 1, (0.0,), 2 << 32, 0)
    add("len2_k2", 4, 2, 1, 1, 2, 1, (0.0,), 0, 0)
    add("len255_drift_neg", 300, 255, 2, 1, 2, 256, (0.0, 1.5), (3 << 32) + 12345, -(1 << 24))
    add("len256_off_the_front", 256, 256, 1, 0, 16, 4, (0.0,), -(20 << 32), 1 << 25)
    add("len257_off_the_end", 200, 257, 8, 1, 1, 1, tuple(float(l) for l in range(8)), 0, 1 << 30)
    add("odd1001_8taps_32paths", 777, 1001, 8, 32, 2, 256, tuple(0.25 * l for l in range(8)), (1 << 32) + 0xFFFFFFFF, 1 << 20, B=1)
    add("last_phase", 64, 33, 1, 32, 16, 256, (0.0,), (8 << 32) + 0xFFFFFF00, 0)
    add("k16_frac_delay", 128, 96, 2, 0, 16, 256, (0.0, 3.0 + 255.0 / 256.0), 10 << 32, -(1 << 28))
    return cases


def clarke_tables(rng, B, taps, ns, fd_cycles, los, sigma):
    """Clarke's model drawn on the host (numpy, not the kernel's Philox): the tables of an IQ_FADE_GIVEN call."""
    paths, amps = tables(B)
    paths[:, :taps, :ns + 1, 0] = rng.integers(-2 ** 31, 2 ** 31, size=(B, taps, ns + 1))
    paths[:, :taps, :ns + 1, 1] = np.rint(fd_cycles * 2.0 ** 32 * np.cos(2 * np.pi * rng.random((B, taps, ns + 1)))).astype(np.int64)
    amps[:, :taps, 0] = los
    if ns:
        amps[:, :taps, 1:ns + 1] = np.float32(sigma * np.sqrt(2.0 / ns))
    return paths, amps


def real_cases():
    """name -> (Fading kwargs (real Kaiser tables), x, paths, amps, clock, the tap whose phase the wrong definition moves): smooth
    band-limited frames (a few tones), so that one step of the fractional phase moves the output by far more than rounding does."""
    rng = np.random.default_rng(7)
    cases = {}

    def tones(B, length):
        n = np.arange(length)
        z = sum(np.exp(2j * np.pi * (f * n + rng.random((B, 1)))) for f in (0.031, -0.077, 0.113))
        return np.stack([z.real, z.imag], axis=2).astype(np.float32)
    kw = dict(length_in=300, length_out=257, taps=3, sinusoids=8, K=9, n_frac=128, delay=(0.0, 1.25, 2.5), normalise=False)
    p, a = clarke_tables(rng, 3, 3, 8, 1e-3, 0.8, 0.3)
    cases["three_taps_k9"] = (kw, tones(3, 300), p, a, np.stack([clock_of((6 << 32) + 0x40000000 * i + 777, 40000 * (i - 1))[0] for i in range(3)]), 0)
    kw = dict(length_in=520, length_out=500, taps=1, sinusoids=32, K=16, n_frac=256, delay=(0.5,), normalise=False)
    p, a = clarke_tables(rng, 2, 1, 32, 5e-3, 0.5, 0.6)
    cases["one_tap_k16_32paths"] = (kw, tones(2, 520), p, a, np.stack([clock_of((9 << 32) + 0x12345678, 858993)[0], clock_of(9 << 32, -858993)[0]]), 0)
    kw = dict(length_in=130, length_out=129, taps=8, sinusoids=1, K=2, n_frac=64, delay=tuple(0.375 * l for l in range(8)), normalise=False)
    p, a = clarke_tables(rng, 2, 8, 1, 2e-2, 0.4, 0.2)
    cases["eight_taps_linear"] = (kw, tones(2, 130), p, a, np.stack([clock_of((3 << 32) + 99, 0)[0], clock_of((3 << 32) + 2 ** 31, 123456)[0]]), 7)
    return cases
