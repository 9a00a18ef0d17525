"""GPU: vl_wave_clip_mix and vl_mix_rows (csrc/vl_audio_mix.hip) against the expression they state, evaluated in torch float32
on the CPU - bit for bit - and AudioASTProcessorTrain with mix-up on top of them.

Sources are packed with NaN gaps between them at float offsets = 1, 2, 3 mod 4 (a read outside a source meets a NaN), and
every clip carries +0.9 / -0.9 at the first / last sample of its crop window in its last channel, so that a dropped first
sample, last sample or channel moves a mean by 0.9 / N - more than twice the bound the means are held to."""
import os
import random

import numpy as np
import pytest
import torch

import fbank_oracle as F
import resample_ref as R
from test_hip_audio_train import MEAN, STD, _chirp, _close, _write_wav      # the existing criterion and wav writer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NS = (1, 7, 4097, 80000)


class Pack:
    """Sources [ch, len] in one NaN-filled buffer, source i at a float offset = 1 + i % 3 (mod 4) behind a gap."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.parts, self.total = [], 5

    def clip(self, ch, ln, start, n):
        """A new source of noise (sigma 0.1) with the sentinels of the crop window [start, start + n) -> (off, ch, len, start)."""
        x = (self.g.standard_normal((ch, ln)) * 0.1).astype(np.float32)
        x[ch - 1, start % ln] = 0.9
        x[ch - 1, (start + n - 1) % ln] = -0.9
        off = self.total + 9
        off += (1 + len(self.parts) % 3 - off) % 4
        assert off % 4 == 1 + len(self.parts) % 3
        self.parts.append((off, x))
        self.total = off + x.size
        return off, ch, ln, start

    def buffer(self):
        buf = np.full(self.total + 11, np.nan, dtype=np.float32)
        for off, x in self.parts:
            buf[off:off + x.size] = x.reshape(-1)
        return torch.from_numpy(buf)


def _rows(n, pack):
    """The cases of one clip length: (A, B or None, lambda or None)."""
    c = pack.clip
    rows = [(c(1, n, 0, n), None, None),                                    # a: no partner, len = n, start = 0
            (c(1, 1, 0, n), None, None),                                    # b: len = 1, alone ...
            (c(2, n, 0, n), c(1, 1, 0, n), 0.41),                           #    ... and as a partner
            (c(1, n + 37, n + 36, n), None, None),                          # d: len > n, start = len - 1
            (c(2, n + 37, 37, n), c(1, n + 5, n + 4, n), 0.55),             #    start = len - n; partner from its last sample
            (c(1, n, 0, n), c(2, n + 2, 1, n), 0.37),                       # e: 1 and 2 channels
            (c(2, n + 1, 1, n), c(1, n, 0, n), 0.62),                       #    2 and 1
            (c(2, n, 0, n), c(2, n + 3, 2, n), 0.5),                        #    2 and 2
            (c(1, n, 0, n), c(1, n, 0, n), 1.0 - 2.0 ** -30),               # f: lambda rounds to 1.0
            (c(2, n, 0, n), c(2, n, 0, n), 1e-9)]                           #    lambda near 0
    if n > 1:                                                               # c: len < n, start = len - 1
        short = max(1, n // 3 + 1)
        rows += [(c(2, short, short - 1, n), None, None), (c(1, n, 0, n), c(1, n - 1, n - 2, n), 0.45)]
    return rows


def _records(rows):
    from vitlens_hip.audio import MIX_DTYPE, mix_record
    return np.array([mix_record(a, b, lam) for a, b, lam in rows], dtype=MIX_DTYPE)


def _clip(src, off, ch, ln, start, n):
    """The index formula of the header on the CPU: a[c][t] = src[off + c len + (start + t) mod len]."""
    return src[off:off + ch * ln].view(ch, ln)[:, (start + torch.arange(n)) % ln]


def _mean_bound(x, N):
    from vitlens_hip.audio import mix_mean_chain
    assert x.numel() == N
    bound = (mix_mean_chain(N) + 1) * U * float(x.double().abs().mean())
    assert 0.9 / N > 2 * bound, (N, bound)           # a lost sentinel (first / last sample, last channel) cannot hide in it
    return bound


def _expected(src, rec, means, n):
    """out of one row restated in torch float32 from the kernel's own means; the means against float64 on the way."""
    mA, mB, mM = means[0], means[1], means[2]                               # 0-d float32 tensors: every operation stays float32
    a = _clip(src, int(rec["off_a"]), int(rec["ch_a"]), int(rec["len_a"]), int(rec["start_a"]), n)
    assert abs(float(mA) - float(a.double().mean())) <= _mean_bound(a, a.numel())
    a1 = a - mA
    if rec["ch_b"] == 0:
        assert float(mB) == 0.0 and float(mM) == 0.0
        return a1[0], a, None
    b = _clip(src, int(rec["off_b"]), int(rec["ch_b"]), int(rec["len_b"]), int(rec["start_b"]), n)
    assert abs(float(mB) - float(b.double().mean())) <= _mean_bound(b, b.numel())
    b1 = b - mB
    lam, mu = torch.tensor(rec["lam"]), torch.tensor(rec["mu"])
    m = lam * a1 + mu * b1                                                  # three roundings, broadcast over channels
    assert m.shape == (max(a.shape[0], b.shape[0]), n) and m.dtype == torch.float32
    assert abs(float(mM) - float(m.double().mean())) <= _mean_bound(m, m.numel())
    return m[0] - mM, a, b


@pytest.mark.parametrize("n", NS)
def test_wave_clip_mix_is_the_stated_expression_bit_for_bit(n):
    from vitlens_hip.audio import wave_clip_mix
    pack = Pack(n)
    rows = _rows(n, pack)
    recs = _records(rows)
    assert recs["lam"][8] == 1.0 and 0 < recs["mu"][8] < 1e-9 and 0 < recs["lam"][9] < 2e-9
    src = pack.buffer()
    assert sorted({int(off) % 4 for off, _ in pack.parts}) == [1, 2, 3] and torch.isnan(src).sum() > 9 * len(pack.parts)
    dev = src.cuda()
    out, means = wave_clip_mix(dev, recs, n, means=True)
    out2, means2 = wave_clip_mix(dev, recs, n, means=True)
    plain = wave_clip_mix(dev, recs, n)
    assert out.shape == (len(rows), n) and means.shape == (len(rows), 3)
    assert torch.equal(out, out2) and torch.equal(means, means2)            # fixed summation order
    assert torch.equal(out, plain)                                          # means = NULL
    out, means = out.cpu(), means.cpu()
    assert torch.isfinite(out).all() and torch.isfinite(means).all()       # no NaN gap was read
    for i, rec in enumerate(recs):
        want, _, _ = _expected(src, rec, means[i], n)
        assert torch.equal(out[i], want), (i, float((out[i] - want).abs().max()))


def test_clips_are_the_host_audio_get_clip_on_a_doubling_case():
    """sampling_rate 4097, one second: cuts of 1 500 and 2 100 samples are doubled to 6 000 / 4 200 and cropped at a random
    offset by the reference's audio_get_clip; the records name the same samples."""
    from open_clip.modal_audio.processors.at_processor import audio_get_clip
    from vitlens_hip.audio import wave_clip_mix
    n = 4097
    pack = Pack(77)
    g = torch.Generator().manual_seed(4)
    wa, wb = torch.randn(2, 1500, generator=g) * 0.1, torch.randn(1, 2100, generator=g) * 0.1
    host_a = audio_get_clip(wa, n, 1.0, sub_mean=False, rng=random.Random(5))
    host_b = audio_get_clip(wb, n, 1.0, sub_mean=False, rng=random.Random(6))
    sa, sb = random.Random(5).randint(0, 5999 - n), random.Random(6).randint(0, 4199 - n)
    assert host_a.shape == (2, n) and torch.equal(host_a, torch.cat([wa] * 4, 1)[:, sa:sa + n])
    ca, cb = pack.clip(2, 1500, sa % 1500, n), pack.clip(1, 2100, sb % 2100, n)
    pack.parts[0][1][:], pack.parts[1][1][:] = wa.numpy(), wb.numpy()      # the recordings themselves, no sentinels
    recs = _records([(ca, cb, 0.3), (cb, None, None)])
    src = pack.buffer()
    out, means = wave_clip_mix(src.cuda(), recs, n, means=True)
    out, means = out.cpu(), means.cpu()
    a1, b1 = host_a - means[0, 0], host_b - means[0, 1]
    m = torch.tensor(recs["lam"][0]) * a1 + torch.tensor(recs["mu"][0]) * b1
    assert torch.equal(out[0], m[0] - means[0, 2])
    assert torch.equal(out[1], (host_b - means[1, 0])[0])


def test_refused_calls_and_rows_write_nothing():
    from vitlens_hip import ops
    from vitlens_hip._lib import load_library
    from vitlens_hip.audio import MIX_DTYPE, mix_record, wave_clip_mix
    n = 300
    pack = Pack(3)
    good = pack.clip(2, 310, 309, n)
    two, three = pack.clip(2, 300, 0, n), pack.clip(3, 300, 0, n)
    src = pack.buffer()
    dev = src.cuda()
    floats = src.numel()
    bad = [mix_record((good[0], 2, 0, 0)), mix_record((good[0], 0, 310, 0)), mix_record((good[0], 2, 310, 310)),
           mix_record((good[0], 2, 310, -1)), mix_record((-1, 2, 310, 0)), mix_record((floats - 619, 2, 310, 0)),
           mix_record(good, (good[0], 2, 310, 310), 0.5), mix_record(two, three, 0.5)]
    for r in bad:                                                           # the wrapper: ValueError, nothing launched
        with pytest.raises(ValueError):
            wave_clip_mix(dev, np.array([mix_record(good), r], dtype=MIX_DTYPE), n)
    # the same records straight to the entry: the kernel leaves their rows as they were and writes the good ones
    recs = np.array([mix_record(good)] + bad + [mix_record(two, (good[0], 1, 310, 5), 0.25)], dtype=MIX_DTYPE)
    recs_dev = torch.from_numpy(recs.view(np.int32).reshape(len(recs), 10)).cuda()
    out = torch.full((len(recs), n), float("nan"), device="cuda")
    means = torch.full((len(recs), 3), float("nan"), device="cuda")
    lib = load_library()
    args = (ops._p(dev), floats, ops._p(recs_dev), ops._p(out), ops._p(means), len(recs), n, ops._stream())
    assert lib.vl_wave_clip_mix(*args) == 0
    torch.cuda.synchronize()
    o, m = out.cpu(), means.cpu()
    assert torch.isnan(o[1:-1]).all() and torch.isnan(m[1:-1]).all()
    assert torch.isfinite(o[0]).all() and torch.isfinite(o[-1]).all() and torch.isfinite(m[0]).all() and torch.isfinite(m[-1]).all()
    assert torch.equal(o[0], _expected(src, recs[0], m[0], n)[0]) and torch.equal(o[-1], _expected(src, recs[-1], m[-1], n)[0])
    # what the entry itself refuses: a status, and out untouched
    out.fill_(float("nan"))
    for k, v in ((6, 0), (5, 0), (1, 0), (0, None), (2, None), (3, None)):
        a = list(args)
        a[k] = v
        assert lib.vl_wave_clip_mix(*a) != 0 and lib.vl_last_error().decode().startswith("vl_wave_clip_mix")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- vl_mix_rows ----
@pytest.mark.parametrize("rows,shape", [(1, (1,)), (3, (7,)), (5, (4097,)), (4, (3, 32, 32))])
def test_mix_rows(rows, shape):
    from vitlens_hip.audio import mix_rows
    g = torch.Generator().manual_seed(rows)
    a, b = torch.randn(rows, *shape, generator=g), torch.randn(rows, *shape, generator=g)
    partner = [(r + 1) % rows if r % 3 != 1 else None for r in range(rows)]       # row 0 of 3+ rows: a LATER row of b
    lambdas = [0.31 + 0.1 * r if p is not None else None for r, p in enumerate(partner)]
    if rows > 1:
        assert partner[0] == 1 and partner[1] is None
        a[1].view(-1)[0], a[1].view(-1)[-1] = float("inf"), -0.0                    # a copied row is a copy of every bit pattern
    want = a.clone()
    for r, p in enumerate(partner):
        if p is not None:
            lam, mu = torch.tensor(np.float32(lambdas[r])), torch.tensor(np.float32(1.0 - lambdas[r]))
            want[r] = lam * a[r] + mu * b[p]
    ad, bd = a.cuda(), b.cuda()
    got = mix_rows(ad, bd, partner, lambdas)
    assert got.shape == a.shape and torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    assert torch.equal(ad.cpu(), a)                                                 # out of place left a alone
    for r, p in enumerate(partner):
        if p is None:
            assert torch.equal(got[r].cpu().view(torch.int32), a[r].view(torch.int32))
    same = mix_rows(ad, bd, partner, lambdas, out=ad)                               # in place
    assert same is ad and torch.equal(ad.cpu(), want)
    if rows > 1:                                                                    # an unaligned view: the scalar kernel
        av, bv = a.reshape(rows, -1)[:, 1:].cuda(), b.reshape(rows, -1)[:, 1:].cuda()
        assert torch.equal(mix_rows(av, bv, partner, lambdas).cpu(), want.reshape(rows, -1)[:, 1:])
    with pytest.raises(ValueError):
        mix_rows(ad, bd, [rows] + partner[1:], [0.5] + lambdas[1:])
    with pytest.raises(ValueError):
        mix_rows(ad, bd, partner[:-1], lambdas[:-1])


# ---- the processor ----

@pytest.fixture(scope="module")
def items(tmp_path_factory):
    d = tmp_path_factory.mktemp("audio_mix")
    rng = np.random.default_rng(23)
    files = {}
    for name, seconds, sr in (("a44", 3, 44100), ("b44", 2.5, 44100), ("short16", 1.5, 16000)):
        s = _chirp(seconds, sr) + 0.05 * rng.standard_normal(int(seconds * sr))
        path = os.path.join(d, name + ".wav")
        files[name] = (path, _write_wav(path, s, sr, 2), sr)
    g = torch.Generator().manual_seed(19)
    mono, stereo, stereo2 = (torch.randn(*s, generator=g) * 0.1 for s in ((112000,), (2, 96000), (2, 80000)))
    its = [files["a44"][0], mono, stereo, files["short16"][0]]
    seconds = [stereo2, files["b44"][0], None, mono[:50000]]
    return files, its, seconds, [0.3, 0.6, None, 0.45]


def test_processor_batch_equals_single_calls_and_the_kernels_on_the_clips(items):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain
    from vitlens_hip.audio import augment_params, fbank_augment, kaldi_fbank
    _, its, seconds, lambdas = items
    batch = AudioASTProcessorTrain(seed=4, mix_up=True).batch(its, seconds=seconds, lambdas=lambdas)
    assert batch.shape == (4, 512, 128) and batch.is_cuda and torch.isfinite(batch).all()
    single = AudioASTProcessorTrain(seed=4, mix_up=True)
    for i in range(4):
        assert torch.equal(batch[i], single(its[i], second=seconds[i], lam=lambdas[i])), i
    assert not torch.equal(batch, AudioASTProcessorTrain(seed=5, mix_up=True).batch(its, seconds=seconds, lambdas=lambdas))
    replay = AudioASTProcessorTrain(seed=4, mix_up=True)
    clips, rows = replay._device_clips(its, None, None, seconds, lambdas, None)
    # rows 1 and 3 are mono with mono: the mean over channel 0 is the mean that was removed (rows 0 and 2 have a stereo side)
    assert clips.shape == (4, 80000) and float(clips[1::2].mean(dim=1).abs().max()) < 1e-6
    raw = kaldi_fbank(clips, target_length=512, mel_bins=128, sample_freq=16000.0)
    assert torch.equal(batch, fbank_augment(raw, augment_params(rows, "cuda"), MEAN, STD))


def _cut64(item, files, proc):
    """(the float64 cut [ch, len] of a recording at 16 kHz, start) as plan_clip places it, drawing from proc.rng."""
    src, a, b, start = proc.plan_clip(item)
    if isinstance(item, str):
        _, samples, sr = next(v for v in files.values() if v[0] == item)
        x = R.resample_dense(samples, sr, 16000)[0][None] if sr != 16000 else samples.astype(np.float64)[None]
    else:
        x = torch.as_tensor(item).reshape(-1, torch.as_tensor(item).shape[-1]).double().numpy()
    assert x.shape[1] == src.length
    return x[:, a:b], start


def test_processor_against_the_float64_mix(items):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain
    files, its, seconds, lambdas = items
    kw = dict(seed=9, mix_up=True, noise_aug=False, freqm=0, timem=0)
    out = AudioASTProcessorTrain(**kw).batch(its, seconds=seconds, lambdas=lambdas).cpu().numpy()
    replay = AudioASTProcessorTrain(**kw)
    t = np.arange(80000)
    for i in range(4):
        cut, start = _cut64(its[i], files, replay)
        a = cut[:, (start + t) % cut.shape[1]]
        mix = a - a.mean()
        if seconds[i] is not None:
            cut, start = _cut64(seconds[i], files, replay)
            b = cut[:, (start + t) % cut.shape[1]]
            mix = lambdas[i] * mix + (1.0 - lambdas[i]) * (b - b.mean())
            mix = mix - mix.mean()
        assert replay.draw_params() == (0, 0, 0, 0, 0.0, 0, 0)
        _close(out[i], F.ast_spectrogram(mix[0].astype(np.float32)))


def test_one_clip_launch_per_batch(items):
    from launch_trace import recording, symbols
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain
    _, its, seconds, lambdas = items
    proc = AudioASTProcessorTrain(seed=1, mix_up=True)
    with recording() as trace:                                    # the bindings of this file's entries go through the recorder
        proc.batch(its, seconds=seconds, lambdas=lambdas)
        proc.batch(its[:2], seconds=[None, None])
    torch.cuda.synchronize()
    assert symbols(trace).count("vl_wave_clip_mix") == 2 and "vl_mix_rows" not in symbols(trace)
    (_, first), (_, second) = [c for c in trace if c[0] == "vl_wave_clip_mix"]
    assert (first[5], first[6]) == (4, 80000) and (second[5], second[6]) == (2, 80000)
    frames, sec = torch.rand(4, 3, 8, 8), torch.rand(4, 3, 8, 8)
    with recording() as trace:
        proc.mix_frames(frames.cuda(), sec.cuda(), [1, None, 3, 0], [0.4, None, 0.5, 0.6])
    assert symbols(trace) == ["vl_mix_rows"]
    got = proc.mix_frames(frames, sec, [1, None, 3, 0], [0.4, None, 0.5, 0.6]).cpu()
    lam, mu = torch.tensor(np.float32(0.5)), torch.tensor(np.float32(0.5))
    assert torch.equal(got[1], frames[1]) and torch.equal(got[2], lam * frames[2] + mu * sec[3])
