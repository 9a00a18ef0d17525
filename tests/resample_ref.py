"""Float64 numpy restatement of torchaudio.functional.resample at its defaults (sinc_interp_hann, lowpass_filter_width=6,
rolloff=0.99), the reference of the resampler tests - torchaudio is not installed, so this is the published algorithm
written down twice: `resample_dense` the way the library runs it (a [new, 2W + orig] kernel, a strided dot over the padded
waveform, a crop) and `resample_direct` as the defining sum out[j] = sum_m x[m] h(m/o - j/n).  Both also return
S[j] = sum |h| |x|, the scale of the rounding error of output j."""
import math

import numpy as np

WIDTH, ROLLOFF = 6, 0.99


def geometry(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * ROLLOFF
    return o, n, base, int(math.ceil(WIDTH * o / base))


def _h(tau, o, base):
    t = np.clip(tau * base, -WIDTH, WIDTH)
    window = np.cos(t * math.pi / WIDTH / 2.0) ** 2
    t = t * math.pi
    safe = np.where(t == 0.0, 1.0, t)
    return np.where(t == 0.0, 1.0, np.sin(safe) / safe) * window * (base / o)


def dense_kernel(orig, new):
    """[n, 2W + o] float64: row p = the taps of output phase p over the padded inputs i o .. i o + 2W + o - 1."""
    o, n, base, W = geometry(orig, new)
    idx = np.arange(-W, W + o, dtype=np.float64)[None, :] / o
    return _h(-np.arange(n, dtype=np.float64)[:, None] / n + idx, o, base)


def out_length(length, orig, new):
    o, n, _, _ = geometry(orig, new)
    return -((-n * length) // o)


def resample_dense(x, orig, new):
    x = np.asarray(x, dtype=np.float64)
    o, n, _, W = geometry(orig, new)
    kern = dense_kernel(orig, new)
    frames = np.lib.stride_tricks.sliding_window_view(np.pad(x, (W, W + o)), 2 * W + o)[::o]
    J = out_length(len(x), orig, new)
    return (frames @ kern.T).reshape(-1)[:J], (np.abs(frames) @ np.abs(kern).T).reshape(-1)[:J]


def resample_direct(x, orig, new):
    x = np.asarray(x, dtype=np.float64)
    o, n, base, _ = geometry(orig, new)
    J = out_length(len(x), orig, new)
    num = np.arange(len(x), dtype=np.int64)[None, :] * n - np.arange(J, dtype=np.int64)[:, None] * o     # exact (m n - j o)
    h = _h(num.astype(np.float64) / (o * n), o, base)
    return h @ x, np.abs(h) @ np.abs(x)
