"""Audio preprocessing on the GPU.

Evaluation (reference: AudioASTProcessorEval, open_clip/modal_audio/processors/at_processor.py:823-903): a waveform ->
`n_clip` clips of `clip_duration` seconds -> Kaldi log-mel filterbank [512, 128] per clip -> (x - mean) / std.  The
spectrogram runs in vl_kaldi_fbank; the clip selection is host arithmetic on sample indices.

Training (reference: ASTProcessorTrain, :313-436): one random clip -> filterbank -> FrequencyMasking / TimeMasking ->
Normalize -> uniform noise -> roll along time.  Every random number is drawn on the host from the processor's own
generator; the transform after the filterbank is one vl_fbank_augment launch for a whole batch.  With audio mix-up (the
reference's dataset, open_clip/modal_audio/datasets.py:279-326) the clips of a batch - cut, repeat, crop, mean removal and the
mix with a second recording - are assembled by one vl_wave_clip_mix launch from one packed copy.

Inputs: a waveform tensor [channels, n] / [n] (at `sampling_rate` unless `sr=` says otherwise), or the path of a PCM .wav file
(8 / 16 / 24 / 32-bit, read with the standard library; torchaudio - the reference's loader - is not available).  Audio at
another rate is resampled by vl_resample_sinc (torchaudio.functional.resample's defaults restated), and only the sample
ranges the clips need: the clip arithmetic is done in the target rate on the length the whole-file resample would have.
Clip placement for recordings longer than one clip: `clips_per_video` windows spread uniformly from the start to
(duration - clip_duration), which is what pytorchvideo's ConstantClipsPerVideoSampler computes for the reference."""
from fractions import Fraction

import torch

AST_AS_MEAN = (-4.2677393,)
AST_AS_STD = (4.5689974,)


def read_wav(path):
    """-> (waveform [channels, n] float32 in [-1, 1), sample rate): PCM 8 (unsigned) / 16 / 24 / 32-bit little-endian .wav, channel-major like
    torchaudio.load (the reference keeps every channel: `audio_get_clip` subtracts the mean over all of them and
    kaldi.fbank reads channel 0, at_processor.py:193-224,855-866)."""
    import wave

    import numpy as np
    if not str(path).lower().endswith((".wav", ".wave")):
        # the reference decodes through torchaudio's backends (at_processor.py:226-244); this image has no flac / mp3 decoder
        raise NotImplementedError(f"{path}: only PCM .wav is decoded here - convert the recording, or pass the waveform / "
                                  "the [clips, 512, 128] fbank tensor")
    with wave.open(str(path), "rb") as f:
        sr, ch, width, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
        raw = f.readframes(n)
    if width == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        a = ((v ^ 0x800000) - 0x800000).astype(np.float32) / 8388608.0               # sign-extend bit 23
    elif width == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise NotImplementedError(f"{width * 8}-bit wav")
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, ch).T)), sr


def clip_timepoints(duration: float, clip_duration: float, clips_per_video: int):
    """(start, end) seconds of every clip, uniformly spread over [0, duration - clip_duration], as exact Fractions - what
    pytorchvideo's ConstantClipsPerVideoSampler hands the reference (at_processor.py:55-65): end = start + clip_duration
    exactly, so `int(end * sr) - int(start * sr)` can never exceed the clip length by rounding start and end separately.
    (Round 3 returned floats: 4 % of the clips of long recordings came out one sample long and 0.4 % one short - a short
    clip is doubled and cropped at a RANDOM offset by audio_get_clip, i.e. non-deterministic eval input.)"""
    last = Fraction(max(duration - clip_duration, 0.0))
    step = last / max(clips_per_video - 1, 1)
    return [(step * i, step * i + Fraction(clip_duration)) for i in range(clips_per_video)]


def random_clip(duration: float, clip_duration: float, rng):
    """(start, end) seconds of one clip placed uniformly in [0, duration - clip_duration] (0 when the recording is shorter),
    as Fractions with end = start + clip_duration exactly - pytorchvideo's RandomClipSampler, which the reference's train
    processor calls (at_processor.py:329-333, 372)."""
    start = Fraction(rng.uniform(0, max(duration - clip_duration, 0)))
    return start, start + Fraction(clip_duration)


def draw_mask(size: int, param: int, rng):
    """(start, width) of one masked band along an axis of `size` cells - torchaudio's published mask_along_axis, which
    FrequencyMasking(param) / TimeMasking(param) apply: v = U param, m = U' (size - v), band [floor(m), floor(m) + floor(v)).
    0 <= width <= param - 1 and start + width <= size."""
    if param > size:
        raise ValueError(f"mask parameter {param} exceeds the axis length {size}")
    v = rng.random() * param
    m = rng.random() * (size - v)
    return int(m), int(v)


def audio_get_clip(waveform, sampling_rate, target_duration, start=None, end=None, sub_mean=True, rng=None):
    """at_processor.py:193-224: cut [start, end), repeat short recordings up to 2^6 times, crop to the target length
    (random offset, `rng.randint`), subtract the clip mean."""
    import random
    wf = waveform
    dur = float(waveform.shape[1] / sampling_rate)
    if start is not None and end is not None and start < dur and end <= dur and end - start > 0.5:
        wf = wf[:, int(start * sampling_rate):int(end * sampling_rate)]
    target = int(sampling_rate * target_duration)
    rep = 0
    while wf.shape[1] < target and rep <= 5:
        wf = torch.cat([wf, wf], dim=1)
        rep += 1
    if rep > 5:
        raise ValueError(f"Original duration {dur} too short, please skip.")
    if wf.shape[1] > target:
        s = (rng or random).randint(0, (wf.shape[1] - 1) - target)
        wf = wf[:, s:s + target]
    return wf - wf.mean() if sub_mean else wf


def _load(item, default_sr, sr=None):
    """path or waveform -> ([channels, n] float32, its sample rate)."""
    if isinstance(item, str) or hasattr(item, "__fspath__"):
        return read_wav(item)
    wav = torch.as_tensor(item, dtype=torch.float32)
    return (wav[None] if wav.dim() == 1 else wav), (default_sr if sr is None else int(sr))


class _Source:
    """A recording seen at the processor's rate: `length` samples there, of which `cut(a, b)` materialises [a, b) - a slice,
    or for another source rate one windowed vl_resample_sinc launch over all channels (bit-identical to the slice of a
    whole-file resample), so a long recording is never resampled whole for the few clips taken from it."""

    def __init__(self, wav, sr, target_sr, device):
        from vitlens_hip.audio import resampled_length
        self.sr, self.target_sr = sr, target_sr
        self.wav = wav if sr == target_sr else wav.to(device)
        self.length = wav.shape[1] if sr == target_sr else resampled_length(wav.shape[1], sr, target_sr)

    def cut(self, a=0, b=None):
        b = self.length if b is None else min(b, self.length)
        if self.sr == self.target_sr:
            return self.wav[:, a:b]
        from vitlens_hip.audio import resample
        return resample(self.wav, self.sr, self.target_sr, out_first=a, n_out=b - a)


def _get_clip(src, sampling_rate, target_duration, start=None, end=None, rng=None):
    """audio_get_clip on a _Source: the same cut condition, evaluated on the length in the target rate."""
    dur = float(src.length / sampling_rate)
    if start is not None and end is not None and start < dur and end <= dur and end - start > 0.5:
        return audio_get_clip(src.cut(int(start * sampling_rate), int(end * sampling_rate)), sampling_rate, target_duration, rng=rng)
    return audio_get_clip(src.cut(), sampling_rate, target_duration, rng=rng)


class AudioASTProcessorEval:
    def __init__(self, mean=AST_AS_MEAN, std=AST_AS_STD, sampling_rate=16000, clip_duration=5.0, n_clip=3, target_length=512,
                 mel_bins=128, device="cuda"):
        self.mean = mean if mean is not None else AST_AS_MEAN
        self.std = std if std is not None else AST_AS_STD
        self.sampling_rate, self.clip_duration, self.n_clip = sampling_rate, clip_duration, n_clip
        self.target_length, self.mel_bins, self.device = target_length, mel_bins, device

    def convert2fbank(self, waveform):
        """[1, n] or [B, n] waveform -> normalised [B, target_length, mel_bins] on the GPU."""
        from vitlens_hip.audio import kaldi_fbank
        return kaldi_fbank(waveform.to(self.device), target_length=self.target_length, mel_bins=self.mel_bins,
                           sample_freq=float(self.sampling_rate), mean=float(self.mean[0]), std=float(self.std[0]))

    def __call__(self, item, sr=None, **kwargs):
        wav, sr = _load(item, self.sampling_rate, sr)
        src = _Source(wav, sr, self.sampling_rate, self.device)
        dur = src.length / self.sampling_rate
        if dur <= self.clip_duration:
            clips = [_get_clip(src, self.sampling_rate, self.clip_duration)] * self.n_clip
        else:
            clips = [_get_clip(src, self.sampling_rate, self.clip_duration, start=s, end=e)
                     for s, e in clip_timepoints(dur, self.clip_duration, self.n_clip)]
        # kaldi.fbank takes channel 0 of each clip (its default `channel=-1` -> 0); the clip mean above was over all channels
        return self.convert2fbank(torch.cat([c[:1] for c in clips], dim=0))            # [n_clip, target_length, mel_bins]


class AudioASTProcessorTrain:
    """ASTProcessorTrain (at_processor.py:313-436) on the GPU.  `seed` starts the processor's own `random.Random`, from which
    everything random is drawn on the host, per item in this order: the clip (`random_clip`, unless `se` gives start / end
    seconds), the crop offset of a repeated short recording, the frequency mask, the time mask, the noise amplitude U / 10,
    the roll in [-10, 10) and the 64-bit key of the noise field - so `batch(items)` equals the single calls of a processor
    with the same seed.

    Mix-up (--audio_mix_up / --audio_mix_up_p; the reference's dataset, open_clip/modal_audio/datasets.py:279-326, 355-360):
    `draw_mix` decides per sample whether it is mixed, with which other sample and with which lambda ~ Beta(10, 10) - the
    reference's distributions from this processor's own generator, not its stream.  The caller loads the partner and
    passes it: `batch(items, seconds=[...], lambdas=[...])` assembles every clip on the device - one packed pinned host
    buffer, one copy, one vl_wave_clip_mix launch for all rows (cut, periodic repeat, crop, mean removal, and for a row
    with a partner lam * wf + (1 - lam) * sec_wf and the mean removal of the mix) - and goes on as before.  Per item the
    draws are: the item's clip and crop, the partner's clip and crop, then the transform's.  `seconds[i]` None is a row
    without a partner; `seconds=None` is the path without mix-up, clip by clip on the host.  A single call of a processor
    built with `mix_up=True` is the one-row batch with `seconds=[second]`, so that it equals its row of a batch bit for
    bit.  `mix_caption` joins the captions and `mix_frames` mixes the two samples' frames (vl_mix_rows)."""

    def __init__(self, mean=AST_AS_MEAN, std=AST_AS_STD, sampling_rate=16000, clip_duration=5.0, target_length=512, mel_bins=128,
                 freqm=48, timem=96, noise_aug=True, device="cuda", seed=None, mix_up=False, mix_up_p=0.5):
        import random
        if not 0.0 <= float(mix_up_p) <= 1.0:
            raise ValueError(f"mix_up_p must be in [0, 1], got {mix_up_p}")
        self.mix_up, self.mix_up_p = bool(mix_up), float(mix_up_p)
        self.mean = mean if mean is not None else AST_AS_MEAN
        self.std = std if std is not None else AST_AS_STD
        self.sampling_rate, self.clip_duration = sampling_rate, clip_duration
        self.target_length, self.mel_bins, self.device = target_length, mel_bins, device
        self.freqm, self.timem, self.noise_aug = freqm, timem, noise_aug
        self.rng = random.Random(seed)

    def load_audio_clip(self, item, se=None, sr=None):
        """-> [channels, sampling_rate * clip_duration]: the clip of at_processor.py:364-386, mean removed."""
        wav, sr = _load(item, self.sampling_rate, sr)
        src = _Source(wav, sr, self.sampling_rate, self.device)
        dur = src.length / self.sampling_rate
        start, end = random_clip(dur, self.clip_duration, self.rng) if se is None else se
        return _get_clip(src, self.sampling_rate, self.clip_duration, start=max(0.0, start), end=min(end, dur), rng=self.rng)

    def draw_params(self):
        """(f0, fw, t0, tw, amp, roll, seed) of one sample; a transform the configuration leaves out draws nothing."""
        f0, fw = draw_mask(self.mel_bins, self.freqm, self.rng) if self.freqm > 0 else (0, 0)
        t0, tw = draw_mask(self.target_length, self.timem, self.rng) if self.timem > 0 else (0, 0)
        if not self.noise_aug:
            return f0, fw, t0, tw, 0.0, 0, 0
        return f0, fw, t0, tw, self.rng.random() / 10.0, self.rng.randrange(-10, 10), self.rng.getrandbits(64)

    def draw_mix(self, n_items):
        """-> (j, lam): the index of the sample to mix with and lambda ~ Beta(10, 10), or (None, None): this sample stays as
        it is (datasets.py:284-289).  Nothing is drawn when `mix_up` is off."""
        if not self.mix_up or not self.rng.random() < self.mix_up_p:
            return None, None
        return self.rng.randint(0, n_items - 1), self.rng.betavariate(10, 10)

    @staticmethod
    def mix_caption(caption, sec_caption):
        """datasets.py:355-360: "<caption without one trailing period> and <second caption, lower case>"."""
        return (caption[:-1] if caption.endswith(".") else caption) + " and " + sec_caption.lower()

    def mix_frames(self, frames, sec_frames, partner, lambdas):
        """frames, sec_frames [B, ...] f32: out[i] = lam_i * frames[i] + (1 - lam_i) * sec_frames[partner[i]], a copy of
        frames[i] where partner[i] is None (datasets.py:318-321), in one launch."""
        from vitlens_hip.audio import mix_rows
        return mix_rows(frames.to(self.device), sec_frames.to(self.device), partner, lambdas)

    def plan_clip(self, item, se=None, sr=None):
        """-> (recording, a, b, start): the clip of `load_audio_clip` as indices - the cut [a, b) of the recording at the
        processor's rate and the crop's first sample inside the cut's periodic extension - with the same draws."""
        wav, sr = _load(item, self.sampling_rate, sr)
        src = _Source(wav, sr, self.sampling_rate, self.device)
        dur = src.length / self.sampling_rate
        start, end = random_clip(dur, self.clip_duration, self.rng) if se is None else se
        start, end = max(0.0, start), min(end, dur)
        a, b = 0, src.length
        if start < dur and end <= dur and end - start > 0.5:                # _get_clip's condition
            a, b = int(start * self.sampling_rate), min(int(end * self.sampling_rate), src.length)
        length, target = b - a, int(self.sampling_rate * self.clip_duration)
        width, rep = length, 0
        while width < target and rep <= 5:                                   # audio_get_clip's doubling
            width, rep = 2 * width, rep + 1
        if rep > 5:
            raise ValueError(f"Original duration {float(length / self.sampling_rate)} too short, please skip.")
        s = self.rng.randint(0, (width - 1) - target) if width > target else 0
        return src, a, b, s % length

    def _device_clips(self, items, se, sr, seconds, lambdas, se2, means=False):
        """The mean-free channel 0 of every row's clip / mix [B, sampling_rate * clip_duration] and the transform's draws."""
        import numpy as np
        from vitlens_hip.audio import MIX_DTYPE, mix_record, wave_clip_mix
        B = len(items)
        if len(seconds) != B or (lambdas is not None and len(lambdas) != B) or (se2 is not None and len(se2) != B):
            raise ValueError(f"seconds, lambdas and se2 need one entry per item ({B})")
        n = int(self.sampling_rate * self.clip_duration)
        head = (10 * B + 3) // 4 * 4                                         # the records lead the packed buffer
        host, pieces, total = [], [], head                                    # (offset, [ch, len] tensor) on the host / on the device
        def place(src, a, b, start):
            nonlocal total
            cut = src.cut(a, b)
            off, total = total, total + (cut.numel() + 3) // 4 * 4            # 16-byte aligned rows wherever len % 4 == 0
            (pieces if cut.is_cuda else host).append((off, cut))
            return off, cut.shape[0], cut.shape[1], start
        rows, params = [], []
        for i, item in enumerate(items):
            ca = place(*self.plan_clip(item, None if se is None else se[i], sr))
            if seconds[i] is None:
                rows.append(mix_record(ca))
            else:
                if lambdas is None or lambdas[i] is None:
                    raise ValueError(f"item {i} has a partner and no lambda")
                cb = place(*self.plan_clip(seconds[i], None if se2 is None else se2[i], sr))
                if not (ca[1] == cb[1] or ca[1] == 1 or cb[1] == 1):
                    raise ValueError(f"item {i}: {ca[1]} and {cb[1]} channels do not broadcast")
                rows.append(mix_record(ca, cb, lambdas[i]))
            params.append(self.draw_params())
        recs = np.array(rows, dtype=MIX_DTYPE)
        # the host part (records, then every recording's cut) goes over in ONE copy; what a resample left on the device
        # is put behind it there
        n_host = max([head] + [off + cut.numel() for off, cut in host])
        staged = torch.empty(n_host, dtype=torch.float32, pin_memory=torch.cuda.is_available())   # (the padding is never read)
        staged[:10 * B].view(torch.int32).copy_(torch.from_numpy(recs.view(np.int32)))
        for off, cut in host:
            staged[off:off + cut.numel()].view(cut.shape).copy_(cut)
        buf = torch.empty(total, dtype=torch.float32, device=self.device)
        buf[:n_host].copy_(staged, non_blocking=True)
        for off, cut in pieces:
            buf[off:off + cut.numel()].view(cut.shape).copy_(cut)
        got = wave_clip_mix(buf, recs, n, means=means, recs_dev=buf[:10 * B].view(torch.int32).view(B, 10))
        return got, params

    def batch(self, items, se=None, sr=None, seconds=None, lambdas=None, se2=None):
        """items: paths / waveforms -> [B, target_length, mel_bins]: one filterbank launch and one augment launch for all.
        seconds: per item the recording it is mixed with, or None (class docstring); lambdas: per mixed item its lambda;
        se2: (start, end) seconds of the partners' clips, like `se`."""
        from vitlens_hip.audio import augment_params, fbank_augment, kaldi_fbank
        if seconds is not None:
            wave, rows = self._device_clips(items, se, sr, seconds, lambdas, se2)
        else:
            clips, rows = [], []
            for i, item in enumerate(items):
                clips.append(self.load_audio_clip(item, None if se is None else se[i], sr)[:1].to(self.device))   # fbank reads channel 0
                rows.append(self.draw_params())
            wave = torch.cat(clips, dim=0)
        raw = kaldi_fbank(wave, target_length=self.target_length, mel_bins=self.mel_bins,
                          sample_freq=float(self.sampling_rate))                       # raw log-mel, padded rows 0 (ZeroPad2d)
        return fbank_augment(raw, augment_params(rows, raw.device), float(self.mean[0]), float(self.std[0]))

    def __call__(self, item, se=None, sr=None, second=None, lam=None, se2=None, **kwargs):
        seconds = [second] if (second is not None or self.mix_up) else None
        return self.batch([item], None if se is None else [se], sr, seconds=seconds, lambdas=[lam], se2=None if se2 is None else [se2])[0]
