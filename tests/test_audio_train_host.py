"""CPU: the host side of the training-time audio front end - the random draws of AudioASTProcessorTrain (masks, clip, roll),
the parameter records vl_fbank_augment reads, read_wav at every PCM width, and the Philox reference of the noise tests."""
import os
import random
import wave
from fractions import Fraction

import numpy as np
import pytest

from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain, draw_mask, random_clip, read_wav


@pytest.mark.parametrize("size,param", [(128, 48), (512, 96), (16, 16)])
def test_draw_mask(size, param):
    rng = random.Random(1)
    widths = set()
    for _ in range(10000):
        start, width = draw_mask(size, param, rng)
        assert 0 <= width <= param - 1 and 0 <= start and start + width <= size
        widths.add(width)
    assert 0 in widths and param - 1 in widths
    assert all(draw_mask(size, 0, rng)[1] == 0 for _ in range(100))
    with pytest.raises(ValueError):
        draw_mask(size, size + 1, rng)


def test_random_clip():
    rng = random.Random(2)
    for dur in (5.0, 5.3, 12.0, 601.7):
        for _ in range(2000):
            s, e = random_clip(dur, 5.0, rng)
            assert isinstance(s, Fraction) and e - s == Fraction(5.0) and 0 <= s and e <= Fraction(dur)
    assert random_clip(2.0, 5.0, rng) == (0, 5)                       # shorter than a clip: starts at 0


def test_train_processor_draws():
    proc = AudioASTProcessorTrain(seed=0)
    rolls, amps = set(), []
    for _ in range(5000):
        f0, fw, t0, tw, amp, roll, seed = proc.draw_params()
        assert 0 <= fw <= 47 and f0 + fw <= 128 and 0 <= tw <= 95 and t0 + tw <= 512
        assert 0.0 <= amp < 0.1 and 0 <= seed < 2 ** 64
        rolls.add(roll); amps.append(amp)
    assert rolls == set(range(-10, 10))
    assert abs(np.mean(amps) - 0.05) < 0.002
    again = AudioASTProcessorTrain(seed=0)
    assert again.draw_params() == AudioASTProcessorTrain(seed=0).draw_params() != AudioASTProcessorTrain(seed=1).draw_params()
    off = AudioASTProcessorTrain(seed=0, freqm=0, timem=0, noise_aug=False)
    state = off.rng.getstate()
    assert off.draw_params() == (0, 0, 0, 0, 0.0, 0, 0) and off.rng.getstate() == state    # nothing drawn


def test_augment_param_records():
    from vitlens_hip.audio import AUGMENT_DTYPE, augment_params
    assert AUGMENT_DTYPE.itemsize == 32 and AUGMENT_DTYPE.fields["seed"][1] == 24
    t = augment_params([(1, 2, 3, 4, 0.5, -7, 0x0123456789ABCDEF), (0, 0, 0, 0, 0.0, 0, 2 ** 64 - 1)], "cpu")
    assert t.shape == (2, 8) and t.dtype.is_floating_point is False
    w = t.numpy()
    assert list(w[0, :4]) == [1, 2, 3, 4] and w[0, 4:5].view(np.float32)[0] == 0.5 and w[0, 5] == -7
    assert w[0, 6:8].view(np.uint64)[0] == 0x0123456789ABCDEF and w[1, 6:8].view(np.uint64)[0] == 2 ** 64 - 1


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_read_wav_every_pcm_width(width, tmp_path):
    rng = np.random.default_rng(width)
    bits = 8 * width
    lo, hi = (0, 256) if width == 1 else (-(1 << (bits - 1)), 1 << (bits - 1))
    v = rng.integers(lo, hi, size=(1000, 2), dtype=np.int64)
    v[0], v[1] = lo, hi - 1                                             # the extremes of the format
    if width == 3:
        u = (v & 0xFFFFFF).astype("<u4").reshape(-1)
        raw = u.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        raw = v.astype({1: "u1", 2: "<i2", 4: "<i4"}[width]).tobytes()
    path = os.path.join(tmp_path, "a.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(2); f.setsampwidth(width); f.setframerate(22050); f.writeframes(raw)
    wav, sr = read_wav(path)
    want = ((v - 128) / 128.0 if width == 1 else v / float(1 << (bits - 1))).astype(np.float32).T
    assert sr == 22050 and wav.shape == (2, 1000) and np.array_equal(wav.numpy(), want)
    assert wav.min() == -1.0 and wav.max() <= 1.0             # the top 32-bit code rounds to 1.0 in float32


def test_philox_reference_known_answers():
    """Random123's published known-answer vectors for philox4x32-10."""
    from philox_ref import noise_field, philox4x32_10
    assert [int(w) for w in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    assert [int(w) for w in philox4x32_10(f, f, f, f, f, f)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    u = noise_field(7, 5, 6)
    assert u.shape == (5, 6) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
