"""Audio front end on the GPU: Kaldi-compatible log-mel filterbank (vl_kaldi_fbank, csrc/vl_audio.hip) with the window and
the mel filter matrix built on the host from the published formulas (Kaldi feature-window / mel-computations, the ones
torchaudio.compliance.kaldi implements), cached per (device, geometry).  Reference call site:
AudioASTProcessorEval.convert2fbank, open_clip/modal_audio/processors/at_processor.py:854-873.

Audio at any sample rate and the training transform (csrc/vl_audio_train.hip): `resample` = torchaudio.functional.resample
at its defaults as a compact polyphase table (`sinc_resample_table`) applied by vl_resample_sinc, and `fbank_augment` = the
masks, Normalize, noise and roll of ASTProcessorTrain (:336-362) in one pass over the raw log-mel."""
import math

import numpy as np
import torch

from . import ops
from ._lib import check
from .ops import _lib, _p, _stream

_tables = {}


def _mel(f):
    return 1127.0 * np.log(1.0 + f / 700.0)


def mel_filter_matrix(num_bins: int, nfft: int, sample_freq: float, low_freq: float = 20.0, high_freq: float = 0.0) -> np.ndarray:
    """Triangular filters, equally spaced on the mel scale between low_freq and high_freq (<= 0: relative to Nyquist), over
    the FFT bins 0 .. nfft/2 - 1; one zero column for the Nyquist bin.  [num_bins, nfft/2 + 1] float32."""
    half = nfft // 2
    hi = high_freq + 0.5 * sample_freq if high_freq <= 0.0 else high_freq
    lo_m, hi_m = _mel(low_freq), _mel(hi)
    step = (hi_m - lo_m) / (num_bins + 1)
    edges = lo_m + step * np.arange(num_bins + 2, dtype=np.float64)
    bin_mel = _mel(sample_freq / nfft * np.arange(half, dtype=np.float64))
    left, mid, right = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    tri = np.minimum((bin_mel[None, :] - left) / (mid - left), (right - bin_mel[None, :]) / (right - mid))
    out = np.zeros((num_bins, half + 1), dtype=np.float32)
    out[:, :half] = np.clip(tri, 0.0, None)
    return out


def _device_tables(device, win, nfft, nmel, sample_freq):
    key = (str(device), win, nfft, nmel, sample_freq)
    if key not in _tables:
        n = np.arange(win, dtype=np.float64)
        window = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / (win - 1))).astype(np.float32)          # "hanning", symmetric
        _tables[key] = (torch.from_numpy(window).to(device), torch.from_numpy(mel_filter_matrix(nmel, nfft, sample_freq)).to(device))
    return _tables[key]


def kaldi_fbank(wave: torch.Tensor, target_length: int = 512, mel_bins: int = 128, sample_freq: float = 16000.0,
                frame_length_ms: float = 25.0, frame_shift_ms: float = 10.0, preemph: float = 0.97,
                mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    """wave [B, n] (or [n]) f32 on the GPU -> [B, target_length, mel_bins] f32: log-mel energies of the first
    target_length frames (zero rows beyond the clip's frames), normalised by (x - mean) / std."""
    if wave.device.type != "cuda":
        raise RuntimeError("kaldi_fbank runs on the MI355X kernels only")
    w = wave.reshape(1, -1) if wave.dim() == 1 else wave
    w = w.contiguous().float()
    win, shift = int(sample_freq * frame_length_ms * 0.001), int(sample_freq * frame_shift_ms * 0.001)
    nfft = 1 << (win - 1).bit_length()
    window, banks = _device_tables(w.device, win, nfft, mel_bins, float(sample_freq))
    out = torch.empty(w.shape[0], target_length, mel_bins, device=w.device, dtype=torch.float32)
    check(_lib.vl_kaldi_fbank(_p(w), w.stride(0), w.shape[0], w.shape[1], _p(window), _p(banks), _p(out), target_length, win, shift,
                              nfft, mel_bins, float(preemph), float(mean), float(std), _stream()))
    return out


# ---- resampling: torchaudio.functional.resample(sinc_interp_hann, lowpass_filter_width=6, rolloff=0.99), restated ----
LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def resample_geometry(orig_freq: int, new_freq: int):
    """-> (o, n, base, W): the rates over their gcd, the cutoff base = min(o, n) * rolloff in units of 1/o of the input rate,
    and the filter's half width in input samples W = ceil(6 o / base)."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"sampling rates must be positive, got {orig_freq} -> {new_freq}")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * ROLLOFF
    return o, n, base, int(math.ceil(LOWPASS_FILTER_WIDTH * o / base))


def resampled_length(n_in: int, orig_freq: int, new_freq: int) -> int:
    """ceil(n len / o): the number of samples `resample` gives for n_in."""
    o, n, _, _ = resample_geometry(orig_freq, new_freq)
    return -((-n * int(n_in)) // o)


def _sinc_table_host(orig_freq, new_freq):
    o, n, base, W = resample_geometry(orig_freq, new_freq)
    K = 2 * W + 1
    # phase p, dense tap k (input i o - W + k for output i n + p): tau = (k - W) / o - p / n in float64
    tau = np.arange(-W, W + o, dtype=np.float64)[None, :] / o - np.arange(n, dtype=np.float64)[:, None] / n
    live = np.abs(tau * base) < LOWPASS_FILTER_WIDTH                      # elsewhere the Hann window is zero
    t = np.clip(tau * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2.0) ** 2
    t = t * math.pi
    dense = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t)) * window * (base / o)
    dense = np.where(live, dense, 0.0)
    # the live taps of a phase are one run of at most 2W entries that starts at most at o + 1; a K-wide slice from
    # min(first, o - 1) holds all of them and stays inside the dense row
    offsets = np.minimum(np.argmax(live, axis=1), o - 1).astype(np.int32)
    taps = np.take_along_axis(dense, offsets[:, None].astype(np.int64) + np.arange(K)[None, :], axis=1)
    assert (live.sum(axis=1) <= 2 * W).all() and np.count_nonzero(dense) == np.count_nonzero(taps)
    return offsets, taps.astype(np.float32)


def sinc_resample_table(orig_freq: int, new_freq: int, device="cpu"):
    """The resampling filter as a compact polyphase table, built in float64 and rounded to float32, cached per
    (device, o, n): (offsets int32 [n], taps float32 [n, K]), K = 2W + 1 (zero padded).  Output sample j = i n + p is
    sum_k x[i o - W + offsets[p] + k] taps[p, k]."""
    o, n, _, _ = resample_geometry(orig_freq, new_freq)
    key = ("sinc", str(torch.device(device)), o, n)
    if key not in _tables:
        offsets, taps = _sinc_table_host(o, n)
        _tables[key] = (torch.from_numpy(offsets).to(device), torch.from_numpy(taps).to(device))
    return _tables[key]


def resample(wave: torch.Tensor, orig_freq: int, new_freq: int, out_first: int = 0, n_out: int = None) -> torch.Tensor:
    """wave [B, len] (or [len]) f32 on the GPU at orig_freq -> the samples out_first .. out_first + n_out - 1 (default: all
    ceil(n len / o)) of the recording at new_freq, each bit-identical to the same sample of a whole-row call."""
    if wave.device.type != "cuda":
        raise RuntimeError("resample runs on the MI355X kernels only")
    if int(orig_freq) == int(new_freq):
        return wave if out_first == 0 and n_out is None else wave[..., out_first:out_first + n_out if n_out is not None else None]
    w = wave.reshape(1, -1) if wave.dim() == 1 else wave
    w = w.float()
    if w.dim() != 2 or w.shape[1] == 0:
        raise ValueError(f"expected a waveform [B, len] or [len] with len >= 1, got {tuple(wave.shape)}")
    if w.stride(1) != 1 or (w.shape[0] > 1 and w.stride(0) < w.shape[1]):
        w = w.contiguous()
    o, n, _, W = resample_geometry(orig_freq, new_freq)
    total = -((-n * w.shape[1]) // o)
    n_out = total - out_first if n_out is None else int(n_out)
    if out_first < 0 or n_out <= 0 or out_first + n_out > total:
        raise ValueError(f"output window [{out_first}, {out_first + n_out}) outside the {total} resampled samples")
    offsets, taps = sinc_resample_table(o, n, w.device)
    out = torch.empty(w.shape[0], n_out, device=w.device, dtype=torch.float32)
    check(_lib.vl_resample_sinc(_p(w), w.stride(0) if w.shape[0] > 1 else w.shape[1], w.shape[0], w.shape[1], _p(offsets), _p(taps), o, n,
                                2 * W + 1, _p(out), n_out, int(out_first), n_out, _stream()))
    return out[0] if wave.dim() == 1 else out


# ---- the training transform after the filterbank ----
# one record per sample, as csrc/vl_audio_train.hip reads it (32 bytes)
AUGMENT_DTYPE = np.dtype([("f0", "<i4"), ("fw", "<i4"), ("t0", "<i4"), ("tw", "<i4"), ("amp", "<f4"), ("roll", "<i4"), ("seed", "<u8")])


def augment_params(rows, device) -> torch.Tensor:
    """rows: per sample (f0, fw, t0, tw, amp, roll, seed) -> the device array vl_fbank_augment reads ([B, 8] int32 words)."""
    a = np.array([tuple(r) for r in rows], dtype=AUGMENT_DTYPE)
    return torch.from_numpy(a.view(np.int32).reshape(len(a), 8)).to(device)


def fbank_augment(fbank: torch.Tensor, params: torch.Tensor, mean: float, std: float) -> torch.Tensor:
    """fbank [B, T, F] f32 raw log-mel on the GPU (kaldi_fbank(mean=0, std=1): padded rows are 0), params from
    `augment_params` -> out[b, (t + roll) mod T, f] = ((masked ? 0 : x) - mean) / std + amp * u(seed_b, t, f)."""
    if fbank.device.type != "cuda":
        raise RuntimeError("fbank_augment runs on the MI355X kernels only")
    x = fbank.contiguous().float()
    if x.dim() != 3 or params.shape != (x.shape[0], 8) or params.dtype != torch.int32 or params.device != x.device:
        raise ValueError(f"expected fbank [B, T, F] and params int32 [B, 8] on its device, got {tuple(fbank.shape)} / {tuple(params.shape)}")
    out = torch.empty_like(x)
    check(_lib.vl_fbank_augment(_p(x), _p(out), x.shape[0], x.shape[1], x.shape[2], _p(params.contiguous()), float(mean), float(std), _stream()))
    return out


# ---- clip assembly and audio mix-up (csrc/vl_audio_mix.hip) ----
# one record per output row, as vl_wave_clip_mix reads it (40 bytes; include/vitlens_hip.h)
MIX_DTYPE = np.dtype([("off_a", "<i4"), ("ch_a", "<i4"), ("len_a", "<i4"), ("start_a", "<i4"),
                      ("off_b", "<i4"), ("ch_b", "<i4"), ("len_b", "<i4"), ("start_b", "<i4"), ("lam", "<f4"), ("mu", "<f4")])


def mix_mean_chain(n_elems: int) -> int:
    """K: the most float32 additions any element passes through in a mean of vl_wave_clip_mix over n_elems elements - its
    thread's chunks (four accumulators, 256 threads), 2 to join the accumulators, 6 across the wave, 2 across the waves."""
    chunks = -(-int(n_elems) // 4)
    return -(-chunks // 256) + 10


def mix_record(a, b=None, lam=None):
    """One MIX_DTYPE row from clip A = (off, ch, len, start), its partner b (the same four, or None) and lambda: `lam` and
    `mu` are the float32 roundings of lambda and of the double 1 - lambda, as torch rounds the two Python scalars."""
    if b is None:
        return tuple(a) + (0, 0, 1, 0, 1.0, 0.0)
    if lam is None:
        raise ValueError("a row with a partner needs its lambda")
    return tuple(a) + tuple(b) + (np.float32(lam), np.float32(1.0 - float(lam)))


def check_mix_records(recs: np.ndarray, n: int, src_floats: int):
    """ValueError for what vl_wave_clip_mix's kernel would leave unwritten (include/vitlens_hip.h)."""
    if recs.dtype != MIX_DTYPE or recs.ndim != 1 or len(recs) < 1:
        raise ValueError("expected a non-empty 1-d array of MIX_DTYPE records")
    if not 1 <= int(n) <= 2 ** 31 - 1 or not 1 <= int(src_floats) <= 2 ** 31 - 1:
        raise ValueError(f"n and the source buffer's length must be in [1, 2^31 - 1], got {n} and {src_floats}")
    for i, r in enumerate(recs):
        for s in ("a", "b") if r["ch_b"] != 0 else ("a",):
            off, ch, ln, st = (int(r[k + "_" + s]) for k in ("off", "ch", "len", "start"))
            if ch < 1 or ln < 1 or not 0 <= st < ln or off < 0 or off + ch * ln > src_floats or ch * int(n) > 2 ** 31 - 1:
                raise ValueError(f"row {i}, clip {s}: off {off}, ch {ch}, len {ln}, start {st} is no clip inside {src_floats} floats "
                                 "(ch, len >= 1, 0 <= start < len, off >= 0, off + ch * len inside the buffer)")
        if r["ch_b"] != 0 and not (r["ch_a"] == r["ch_b"] or r["ch_a"] == 1 or r["ch_b"] == 1):
            raise ValueError(f"row {i}: {int(r['ch_a'])} and {int(r['ch_b'])} channels do not broadcast")


def wave_clip_mix(src: torch.Tensor, recs: np.ndarray, n: int, means: bool = False, recs_dev: torch.Tensor = None):
    """src: packed f32 recordings on the GPU, recs: MIX_DTYPE rows (host; checked here) -> out [B, n] f32, channel 0 of every
    mean-free clip / mix, in one vl_wave_clip_mix launch; with `means` also [B, 3] = mA, mB, mM.  recs_dev: the same records
    already on src's device as int32 [B, 10] (the processor sends them in the copy that brings the recordings)."""
    if src.device.type != "cuda":
        raise RuntimeError("wave_clip_mix runs on the MI355X kernels only")
    if src.dtype != torch.float32 or src.dim() != 1 or not src.is_contiguous():
        raise ValueError(f"expected a packed 1-d float32 buffer, got {src.dtype} {tuple(src.shape)}")
    check_mix_records(recs, n, src.numel())
    B = len(recs)
    if recs_dev is None:
        recs_dev = torch.from_numpy(recs.view(np.int32).reshape(B, 10)).to(src.device)
    elif recs_dev.shape != (B, 10) or recs_dev.dtype != torch.int32 or recs_dev.device != src.device or not recs_dev.is_contiguous():
        raise ValueError("recs_dev must be the records as contiguous int32 [B, 10] on src's device")
    out = torch.empty(B, int(n), device=src.device, dtype=torch.float32)
    m = torch.zeros(B, 3, device=src.device, dtype=torch.float32) if means else None
    check(ops._lib.vl_wave_clip_mix(ops._p(src), src.numel(), ops._p(recs_dev), ops._p(out), ops._p(m), B, int(n), ops._stream()))
    return (out, m) if means else out


def mix_rows(a: torch.Tensor, b: torch.Tensor, partner, lambdas, out: torch.Tensor = None) -> torch.Tensor:
    """a, b [rows, ...] f32 on the GPU, flattened per row; partner: per row an index into b or None / negative (the row of a
    is copied); lambdas: per mixed row its lambda -> out[r] = lam_r * a[r] + (1 - lam_r) * b[partner[r]] as torch rounds it,
    in one vl_mix_rows launch.  `out` may be `a`."""
    if a.device.type != "cuda":
        raise RuntimeError("mix_rows runs on the MI355X kernels only")
    rows = a.shape[0]
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape or b.device != a.device or rows < 1 or a.numel() == 0:
        raise ValueError(f"expected two float32 tensors of one shape on one device, got {tuple(a.shape)} / {tuple(b.shape)}")
    if len(partner) != rows or len(lambdas) != rows:
        raise ValueError(f"partner and lambdas need one entry per row ({rows})")
    host = np.zeros((rows, 3), dtype=np.float32)
    idx = host[:, 0].view(np.int32)
    for r, (p, lam) in enumerate(zip(partner, lambdas)):
        if p is None or int(p) < 0:
            idx[r] = -1
            continue
        if int(p) >= rows or lam is None:
            raise ValueError(f"row {r}: partner {p} is no row of b, or its lambda is missing")
        idx[r], host[r, 1], host[r, 2] = int(p), np.float32(lam), np.float32(1.0 - float(lam))
    dev = torch.from_numpy(host).to(a.device)
    part, lam_mu = dev[:, 0].contiguous().view(torch.int32), dev[:, 1:].contiguous()
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape or out.dtype != torch.float32 or out.device != a.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of a's shape on its device")
    check(ops._lib.vl_mix_rows(ops._p(a), ops._p(b), ops._p(part), ops._p(lam_mu), ops._p(out), rows, a.numel() // rows, ops._stream()))
    return out
