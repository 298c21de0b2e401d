"""Host restatements for the shaped frame source (include/iqvit.h, iq_frames_waveform), shared by tests/test_waveform_cpu.py and
tests/test_gpu_waveform.py: the counter layout on tests/dropout_ref.philox4x32 (integers, and the channel taps through an fp64
Box-Muller), and the occupied-bandwidth statistic."""
import numpy as np

from dropout_ref import philox4x32

SITE_SYNTH = 0xFFFFFFFE
M32 = 0xFFFFFFFF


def words(seed, stream, j, c):
    """Philox words of frame j for the counter values c (array) -> (len(c), 4) uint64 array."""
    c = np.asarray(c, dtype=np.uint64)
    key = np.array([seed & M32, ((seed >> 32) ^ (j >> 32)) & M32], dtype=np.uint64)
    ctr = np.stack([c, np.full_like(c, j & M32), np.full_like(c, SITE_SYNTH), np.full_like(c, stream)], axis=-1)
    return philox4x32(ctr, key, 7)


def host_frame(ws, j, stream):
    """Frame j of a ShapedSynth -> (class, snr as np.float32 (NaN without noise), theta as np.float32, q, symbols (NS,) int64,
    taps (8, 2) float64 from the fp32 los / tap_sigma the kernel is given)."""
    K, ns = ws.n_classes, len(ws.snrs_db)
    par = [int(v) for v in words(ws.seed, stream, j, [0xFFFFFFFF])[0]]
    if ws.balanced:
        cls, si = j % K, (j // K) % ns if ns else 0
    else:
        cls, si = (par[1] * K) >> 32, (par[2] * ns) >> 32
    snr = np.float32(ws.snrs_db[si]) if ns else np.float32(np.nan)
    theta = np.float32(2 * np.pi) * np.float32((par[0] >> 8) * 2.0 ** -24)
    q = (par[3] * ws.n_phase) >> 32 if ws.timing else 0
    NS = ws.n_symbols
    w = words(ws.seed, stream, j, np.arange((NS + 3) // 4)).reshape(-1)[:NS].astype(np.int64)
    kind, _, count = ws.descriptors[cls]
    if kind == 0:
        sym = (w * count) >> 32                                # 32-bit word * count < 2^63
    elif kind == 1:
        sym = w & 1
    else:
        sym = 2 * (w & 1) + ((w >> 1) & 1)
    taps = np.zeros((8, 2))
    if ws.taps == 1:
        taps[0, 0] = 1.0
    else:
        tw = words(ws.seed, stream, j, 0xFFFFFFF0 + np.arange(4)).astype(np.int64)
        for l in range(ws.taps):
            a, b = tw[l // 2, 2 * (l % 2)], tw[l // 2, 2 * (l % 2) + 1]
            r = np.sqrt(-2.0 * np.log(((a >> 8) + 1) * 2.0 ** -24))
            ang = 2.0 * np.pi * (b >> 8) * 2.0 ** -24
            sg = float(np.float32(ws.tap_sigma[l]))
            taps[l] = ((float(np.float32(ws.los)) if l == 0 else 0.0) + sg * r * np.cos(ang), sg * r * np.sin(ang))
    return cls, snr, theta, q, sym, taps


def out_of_band_fraction(frames, f_edge):
    """frames (n, len, 2) -> per frame the share of the Hann-windowed periodogram's power at |f| > f_edge cycles per sample."""
    x = np.asarray(frames, dtype=np.float64)
    z = x[:, :, 0] + 1j * x[:, :, 1]
    n = z.shape[1]
    p = np.abs(np.fft.fft(z * np.hanning(n)[None, :], axis=1)) ** 2
    f = np.abs(np.fft.fftfreq(n))
    return p[:, f > f_edge].sum(axis=1) / p.sum(axis=1)


def band_edge(alpha, sps, length):
    return (1 + alpha) / (2 * sps) + 4 / length
