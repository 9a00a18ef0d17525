"""GPU: vl_resample_sinc against the float64 dense restatement (tests/resample_ref.py), vl_fbank_augment against the torch
expression on the CPU and the Philox reference (tests/philox_ref.py), and the processors that use them
(AudioASTProcessorEval at 44.1 / 48 kHz, AudioASTProcessorTrain).  Parity unpinned: torchaudio is not installed."""
import math
import os
import random
import wave

import numpy as np
import pytest
import torch

import fbank_oracle as F
import resample_ref as R
from philox_ref import noise_field

pytestmark = pytest.mark.gpu

MEAN, STD = -4.2677393, 4.5689974
# ratio o:n -> the rates that give it
RATIOS = {"3:1": (48000, 16000), "441:160": (44100, 16000), "1:2": (8000, 16000), "441:640": (11025, 16000), "3:2": (24000, 16000),
          "160:441": (16000, 44100)}
HALVED_TILE = {"441:80": (44100, 8000)}          # the input span of 2 048 outputs exceeds the staging buffer: 1 024-output tiles


def _signals(length, orig, rng):
    """white noise, a 1 kHz tone, a unit impulse at index 0 and at len - 1: [4, length] float32."""
    x = np.zeros((4, length), dtype=np.float32)
    x[0] = rng.standard_normal(length).astype(np.float32) * 0.3
    x[1] = (0.5 * np.sin(2 * math.pi * 1000.0 * np.arange(length) / orig)).astype(np.float32)
    x[2, 0] = 1.0
    x[3, length - 1] = 1.0
    return x


def _poisoned_rows(x, gap=37):
    """The rows of x as a strided view of a NaN-filled buffer: a read past a row's end meets a NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + gap), float("nan"), dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf.cuda()[:, :x.shape[1]]


def _check(got, x, orig, new, K):
    """per element |got - ref| <= (K + 2) 2^-24 S[j]: the table's float32 rounding and K float32 accumulations - plus the
    float32 underflow quantum, K 2^-149 max(1, max|x|) ~ 1e-43: a relative rounding error holds only down to the smallest
    normal number, and the float64 reference keeps the taps under the clamped end of the window (1e-50, where
    cos^2(pi/2) is 4e-33 instead of 0), which float32 holds as 0.  Without that term the impulse at len - 1 fails at outputs
    whose reference is 1e-51 and whose result is 0."""
    worst = 0.0
    for row_got, row_x in zip(got, x):
        ref, S = R.resample_dense(row_x, orig, new)
        assert row_got.shape == ref.shape and np.isfinite(row_got).all()
        err = np.abs(row_got.astype(np.float64) - ref)
        bound = (K + 2) * 2.0 ** -24 * S + K * 2.0 ** -149 * max(1.0, float(np.abs(row_x).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (float(err.max()), int(np.argmax(err - bound)))
    return worst


@pytest.mark.parametrize("ratio", list(RATIOS) + list(HALVED_TILE))
def test_resample_vs_dense_reference(ratio):
    from vitlens_hip.audio import resample
    orig, new = {**RATIOS, **HALVED_TILE}[ratio]
    o, n, _, W = R.geometry(orig, new)
    assert f"{o}:{n}" == ratio
    K = 2 * W + 1
    rng = np.random.default_rng(o * 1000 + n)
    for length in (1, W - 1, W, o + 1, 4097, 50000):
        x = _signals(length, orig, rng)
        got = resample(_poisoned_rows(x), orig, new).cpu().numpy()
        assert got.shape == (4, R.out_length(length, orig, new))
        print(f"{ratio} len {length}: worst error / bound {_check(got, x, orig, new, K):.3f}")
    x = _signals(4097, orig, rng)[:3]                                           # B = 3, in_stride > len
    view = _poisoned_rows(x, gap=5)
    assert view.shape[0] == 3 and view.stride(0) == 4102 and not view.is_contiguous()
    _check(resample(view, orig, new).cpu().numpy(), x, orig, new, K)
    one = resample(view[1], orig, new)                                          # a 1-d waveform gives a 1-d result
    assert one.dim() == 1 and torch.equal(one, resample(view, orig, new)[1])


@pytest.mark.parametrize("ratio", list(RATIOS))
def test_resample_windows_are_bit_identical_to_the_whole_row(ratio):
    from vitlens_hip.audio import resample
    orig, new = RATIOS[ratio]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(_signals(50000, orig, rng)[:3]).cuda()
    whole = resample(x, orig, new)
    J = whole.shape[1]
    assert J == R.out_length(50000, orig, new)
    # the first 10, the last 10, across the whole call's tile boundary at 2048 (tiles are powers of two up to 2048 outputs),
    # a window with a tile boundary of its own inside, the last sample alone
    for first, count in ((0, 10), (J - 10, 10), (2040, 20), (5, 2148), (J - 1, 1)):
        part = resample(x, orig, new, out_first=first, n_out=count)
        assert part.shape == (3, count) and torch.equal(part, whole[:, first:first + count]), (first, count)
    assert torch.equal(resample(x, orig, new, out_first=J - 7), whole[:, J - 7:])
    with pytest.raises(ValueError):
        resample(x, orig, new, out_first=J - 5, n_out=6)
    assert resample(x, orig, orig) is x


# ---- vl_fbank_augment ----
def _torch_augment(x, rows, mean, std):
    """The reference's order on the CPU: mask with 0, Normalize, (+ 0 * noise), roll along time."""
    out = []
    for xb, (f0, fw, t0, tw, _amp, roll, _seed) in zip(x, rows):
        m = xb.clone()
        m[t0:t0 + tw, :] = 0.0
        m[:, f0:f0 + fw] = 0.0
        out.append(torch.roll((m - mean) / std, roll, 0))
    return torch.stack(out)


@pytest.mark.parametrize("B,T,Fm", [(3, 512, 128), (2, 64, 16), (2, 64, 6)])
def test_fbank_augment_without_noise_is_the_torch_expression(B, T, Fm):
    from vitlens_hip.audio import augment_params, fbank_augment
    g = torch.Generator().manual_seed(T + Fm)
    x = torch.randn(B, T, Fm, generator=g) * 4.0 - 5.0
    masks = [(0, 0, 0, 0),                                   # no mask
             (Fm - 5, 5, T - 9, 9),                          # a mask at the far end of each axis
             (0, 3, 0, 7),                                   # and at the near end
             (2, 1, 3, 0), (1, 0, 5, 1)]                     # widths 0 and 1
    for i, roll in enumerate((0, -10, 9, T, -T - 3)):
        rows = [masks[(i + b) % len(masks)] + (0.0, roll, 11 * b) for b in range(B)]
        xin = x.clone()
        for b, (f0, fw, t0, tw, *_rest) in enumerate(rows):  # poison under the masks: the kernel must select, not multiply
            xin[b, t0:t0 + tw, ::2] = float("nan")
            xin[b, t0:t0 + tw, 1::2] = float("-inf")
            xin[b, ::3, f0:f0 + fw] = float("nan")
        got = fbank_augment(xin.cuda(), augment_params(rows, "cuda"), MEAN, STD).cpu()
        ref = _torch_augment(xin, rows, MEAN, STD)
        assert torch.isfinite(got).all() and torch.equal(got, ref), (roll, float((got - ref).abs().max()))
        band = (torch.zeros(1) - MEAN) / STD                                 # (0 - mean) / std as torch rounds it in float32
        for b, (f0, fw, t0, tw, *_rest) in enumerate(rows):
            unrolled = torch.roll(got[b], -roll, 0)
            assert (unrolled[t0:t0 + tw] == band).all() and (unrolled[:, f0:f0 + fw] == band).all()


def test_fbank_augment_noise_field():
    from vitlens_hip.audio import augment_params, fbank_augment
    B, T, Fm, amp = 3, 512, 128, 0.1
    amp32 = np.float32(amp)
    # a plane that normalises to exactly 0, so out = fl(amp * u) and u is recovered to one float32 rounding
    flat = torch.full((B, T, Fm), float(np.float32(MEAN))).cuda()
    rows = [(0, 0, 0, 0, amp, 0, 1234567890123456789), (0, 0, 0, 0, amp, 0, 42), (0, 0, 0, 0, amp, 0, 42)]
    params = augment_params(rows, "cuda")
    out0 = fbank_augment(flat, augment_params([r[:4] + (0.0,) + r[5:] for r in rows], "cuda"), MEAN, STD).cpu().numpy()
    assert (out0 == 0).all()
    out = fbank_augment(flat, params, MEAN, STD).cpu().numpy()
    assert np.array_equal(out, fbank_augment(flat, params, MEAN, STD).cpu().numpy())            # a second call: the same bits
    assert np.array_equal(out[1], out[2]) and not np.array_equal(out[0], out[1])                # seeds
    for b in (0, 1):                                                                            # the generator itself
        assert np.array_equal(out[b], amp32 * noise_field(rows[b][6], T, Fm))
    # statistics over three different seeds
    rows = [(0, 0, 0, 0, amp, 0, s) for s in (1, 2, 2 ** 63 + 5)]
    out = fbank_augment(flat, augment_params(rows, "cuda"), MEAN, STD).cpu().numpy()
    u = (out.astype(np.float64) - out0) / float(amp32)
    N = u.size
    assert N == 196608 and u.min() >= -2.0 ** -20 and u.max() < 1.0
    print(f"noise: mean {u.mean():.5f}, min {u.min():.2e}, max {u.max():.8f}")
    assert abs(u.mean() - 0.5) < 0.004                                                          # 5 sigma, sigma = 0.2887 / sqrt(N)
    c = u - u.mean()
    rho_t = (c[:, 1:, :] * c[:, :-1, :]).sum() / (c * c).sum()
    rho_f = (c[:, :, 1:] * c[:, :, :-1]).sum() / (c * c).sum()
    print(f"noise: lag-1 correlation along t {rho_t:.5f}, along f {rho_f:.5f}")
    assert abs(rho_t) < 0.012 and abs(rho_f) < 0.012                                            # 5 / sqrt(N)
    # the field is indexed by the pre-roll (t, f) and does not depend on the data: a random plane with |v| < 0.9, so that
    # |out| < 1 and one rounding of out moves u by at most 2^-25 / amp < 2^-21
    x = (torch.rand(B, T, Fm, generator=torch.Generator().manual_seed(3)) * 1.7 - 0.85) * STD + MEAN
    rolled = [r[:5] + (-13,) + r[6:] for r in rows]
    o0 = fbank_augment(x.cuda(), augment_params([r[:4] + (0.0,) + r[5:] for r in rolled], "cuda"), MEAN, STD).cpu().numpy()
    o1 = fbank_augment(x.cuda(), augment_params(rolled, "cuda"), MEAN, STD).cpu().numpy()
    assert np.abs(o0).max() < 0.9
    u2 = np.roll((o1.astype(np.float64) - o0) / float(amp32), 13, axis=1)
    assert np.abs(u2 - u).max() <= 2.0 ** -21


# ---- processors ----
def _close(got, ref, atol=2e-3):
    """The criterion of tests/test_hip_audio.py: log-mel values; where the energy sits at the float32-epsilon floor both
    sides must sit there."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    floor = (math.log(float(F.EPS)) - MEAN) / STD
    live = ref > floor + 0.5
    assert np.abs(got - ref)[live].max() < atol, np.abs(got - ref)[live].max()
    assert (got[~live] < floor + 1.0).all()


def _chirp(seconds, sr):
    t = np.arange(int(seconds * sr)) / sr
    return 0.4 * np.sin(2 * math.pi * (200.0 * t + 0.5 * 2500.0 / seconds * t * t)) + 0.01 * np.cos(2 * math.pi * 50.0 * t)


def _write_wav(path, samples, sr, width):
    """-> the float32 samples read_wav must give back."""
    scale = float(1 << (8 * width - 1))
    v = np.clip(np.round(samples * scale), -scale, scale - 1).astype(np.int64)
    if width == 3:
        raw = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        raw = v.astype("<i2").tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(width); f.setframerate(sr); f.writeframes(raw)
    return (v / scale).astype(np.float32)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("audio_train")
    rng = np.random.default_rng(11)
    out = {}
    for name, seconds, sr, width in (("chirp44", 2, 44100, 2), ("chirp48", 2, 48000, 3), ("long44", 12, 44100, 2), ("mid44", 7, 44100, 2)):
        s = _chirp(seconds, sr) + (0.05 * rng.standard_normal(int(seconds * sr)) if name in ("long44", "mid44") else 0.0)
        path = os.path.join(d, name + ".wav")
        out[name] = (path, _write_wav(path, s, sr, width), sr)
    return out


@pytest.mark.parametrize("name", ["chirp44", "chirp48"])
def test_eval_processor_resamples_a_short_file(wavs, name):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorEval
    path, samples, sr = wavs[name]
    random.seed(17)
    out = AudioASTProcessorEval()(path).cpu().numpy()
    assert out.shape == (3, 512, 128) and np.array_equal(out[0], out[1]) and np.array_equal(out[1], out[2])
    y, _ = R.resample_dense(samples, sr, 16000)
    assert len(y) == 32000
    rep = np.concatenate([y] * 4)                                     # 2 s -> 4 s -> 8 s, then the random 5 s crop
    random.seed(17)
    s = random.randint(0, (len(rep) - 1) - 80000)
    clip = rep[s:s + 80000]
    _close(out[0], F.ast_spectrogram((clip - clip.mean()).astype(np.float32)))
    # a waveform tensor with sr= takes the same road
    random.seed(17)
    assert np.array_equal(AudioASTProcessorEval()(torch.from_numpy(samples), sr=sr).cpu().numpy(), out)


def test_eval_processor_resamples_only_the_clips_of_a_long_file(wavs):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorEval, clip_timepoints
    from mm_vit_lens.data_processors import AudioProcessor
    from vitlens_hip.audio import resample
    path, samples, sr = wavs["long44"]
    proc = AudioASTProcessorEval()
    out = proc(path)
    whole = resample(torch.from_numpy(samples).cuda()[None], sr, 16000)
    assert whole.shape == (1, 192000)
    pts = clip_timepoints(12.0, 5.0, 3)
    for i, (s, e) in enumerate(pts):
        clip = whole[:, int(s * 16000):int(e * 16000)]
        assert clip.shape == (1, 80000)
        assert torch.equal(out[i], proc.convert2fbank(clip - clip.mean())[0])
    ref, _ = R.resample_dense(samples, sr, 16000)
    c = ref[int(pts[1][0] * 16000):int(pts[1][1] * 16000)]
    _close(out[1].cpu().numpy(), F.ast_spectrogram((c - c.mean()).astype(np.float32)))
    batch = AudioProcessor()([path], device="cuda")
    assert batch.shape == (1, 3, 512, 128) and batch.is_cuda and torch.equal(batch[0], out)


def test_train_processor(wavs):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorEval, AudioASTProcessorTrain
    g = torch.Generator().manual_seed(9)
    clip16 = torch.randn(80000, generator=g) * 0.1                       # exactly one clip at 16 kHz: nothing random in the cut
    long16 = torch.randn(1, 144000, generator=g) * 0.1                   # 9 s: a random 5 s clip
    out = AudioASTProcessorTrain(seed=0)(clip16)
    assert out.shape == (512, 128) and out.is_cuda and out.dtype == torch.float32 and torch.isfinite(out).all()
    # no augmentation: the eval normalisation of the same clip.  The filterbank kernel multiplies by 1 / std, the augment
    # kernel divides: 1.5 ulp apart at most (two roundings against one)
    plain = AudioASTProcessorTrain(seed=0, noise_aug=False, freqm=0, timem=0)(clip16)
    ref = AudioASTProcessorEval()(clip16)[0]
    assert ((plain - ref).abs() <= 3 * 2.0 ** -24 * ref.abs()).all(), float((plain - ref).abs().max())
    # batch = the single calls of a processor with the same seed
    items = [wavs["mid44"][0], clip16, long16, wavs["chirp48"][0]]
    batch = AudioASTProcessorTrain(seed=4).batch(items)
    single = AudioASTProcessorTrain(seed=4)
    assert batch.shape == (4, 512, 128)
    for i, it in enumerate(items):
        assert torch.equal(batch[i], single(it)), i
    assert not torch.equal(batch, AudioASTProcessorTrain(seed=5).batch(items))
    # masks only: the bands are the constant (0 - mean) / std
    masked = AudioASTProcessorTrain(seed=0, noise_aug=False)
    got = masked(long16).cpu()
    replay = AudioASTProcessorTrain(seed=0, noise_aug=False)
    replay.load_audio_clip(long16)
    f0, fw, t0, tw, amp, roll, _seed = replay.draw_params()
    assert (amp, roll) == (0.0, 0) and fw > 0 and tw > 0
    band = (torch.zeros(1) - MEAN) / STD
    assert (got[t0:t0 + tw] == band).all() and (got[:, f0:f0 + fw] == band).all()
    keep = torch.ones(512, 128, dtype=torch.bool)
    keep[t0:t0 + tw] = False
    keep[:, f0:f0 + fw] = False
    assert (got[:498][keep[:498]] != band).all()                          # 5 s = 498 frames; the rest is padding
