"""Rates of the audio front end on the GPU: (a) `audio.resample` of 256 ten-second recordings from 44.1 to 16 kHz, as
bytes per second next to a device-to-device hipMemcpyAsync that moves the same number of bytes in the same run; (b)
`AudioASTProcessorTrain.batch` on 256 five-second 16 kHz clips already on the device, in clips per second, with the
filterbank launch and the augment launch timed alone.  Device events around repeated calls, the median reported.
Writes one JSON object: `python tools/audio_frontend_bench.py profiles/audio_frontend.json`.

`python tools/audio_frontend_bench.py --mixup profiles/audio_mixup.log`: the mix-up mode.  B = 32 and 256 ten-second 16 kHz
mono recordings on the host; `batch(items)` (clips assembled on the host, one copy per clip), `batch(items, seconds=[None] * B)`
(the same clips assembled by one vl_wave_clip_mix launch from one packed copy) and `batch(items, seconds=...)` with every
second row mixed with another recording, alternated in one process; wall time of each call up to the device's last kernel,
median / min / max over 20 batches after 3 warm-up rounds, one line per variant."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))

from open_clip.modal_audio.processors.at_processor import AST_AS_MEAN, AST_AS_STD, AudioASTProcessorTrain  # noqa: E402
from vitlens_hip import audio  # noqa: E402


def event_times(fn, reps, warm=2):
    """seconds of each of `reps` calls, by device events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def mixup(path=None, rounds=20, warm=3):
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    g = torch.Generator().manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name(0)}: AudioASTProcessorTrain.batch, 10 s 16 kHz mono recordings on the host, 5 s clips; "
             f"wall ms per batch incl. the device, median [min, max] over {rounds} alternated batches after {warm} warm-up rounds"]
    for B in (32, 256):
        items = [torch.randn(160000, generator=g) * 0.1 for _ in range(B)]
        seconds = [items[(i + 7) % B] if i % 2 == 0 else None for i in range(B)]
        lambdas = [0.5 if s is not None else None for s in seconds]
        proc = AudioASTProcessorTrain(seed=0, mix_up=True)
        variants = {"host clips, no mix-up (batch(items))": lambda: proc.batch(items),
                    "device clips, no row mixed (seconds=[None] * B)": lambda: proc.batch(items, seconds=[None] * B),
                    "device clips, half the rows mixed": lambda: proc.batch(items, seconds=seconds, lambdas=lambdas)}
        times = {k: [] for k in variants}
        for r in range(warm + rounds):
            for k, fn in variants.items():
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                if r >= warm:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        for k, ts in times.items():
            med = statistics.median(ts)
            lines.append(f"B={B:<4d}{k:<50s}{med:9.3f} ms [{min(ts):.3f}, {max(ts):.3f}]  {B / med * 1e3:9.1f} clips/s")
    text = "\n".join(lines)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)

    # (a) resampling
    B, sr, seconds = 256, 44100, 10
    x = (torch.randn(B, sr * seconds, generator=g) * 0.1).cuda()
    y = audio.resample(x, sr, 16000)
    nbytes = x.numel() * 4 + y.numel() * 4                                  # every input sample read once, every output written once
    ts = event_times(lambda: audio.resample(x, sr, 16000), reps=20)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    half = nbytes // 2                                                      # a copy reads and writes: the same bytes moved
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), half, 3, stream) == 0          # 3 = hipMemcpyDeviceToDevice
    tc = event_times(copy, reps=20)
    o, n, _, W = audio.resample_geometry(sr, 16000)
    res["resample"] = {"batch": B, "seconds": seconds, "orig_freq": sr, "new_freq": 16000, "o": o, "n": n, "taps_per_output": 2 * W + 1,
                       "bytes_moved": nbytes, "ms_median": round(statistics.median(ts) * 1e3, 3), "ms_min": round(min(ts) * 1e3, 3),
                       "ms_max": round(max(ts) * 1e3, 3), "gb_per_s": round(nbytes / statistics.median(ts) / 1e9, 1),
                       "audio_seconds_per_s": round(B * seconds / statistics.median(ts), 1),
                       "memcpy_d2d_same_bytes_ms_median": round(statistics.median(tc) * 1e3, 3),
                       "memcpy_d2d_gb_per_s": round(2 * half / statistics.median(tc) / 1e9, 1)}
    del x, y, src, dst

    # (b) the training processor on clips that are already on the device
    clips = [c for c in (torch.randn(B, 80000, generator=g) * 0.1).cuda()]
    proc = AudioASTProcessorTrain(seed=0)
    tb = event_times(lambda: proc.batch(clips), reps=10)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter(); proc.batch(clips); torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    stacked = torch.stack(clips)
    tf = event_times(lambda: audio.kaldi_fbank(stacked), reps=10)
    raw = audio.kaldi_fbank(stacked)
    params = audio.augment_params([proc.draw_params() for _ in range(B)], "cuda")
    ta = event_times(lambda: audio.fbank_augment(raw, params, AST_AS_MEAN[0], AST_AS_STD[0]), reps=20)
    aug_bytes = 2 * raw.numel() * 4
    res["train_processor"] = {"batch": B, "clip_seconds": 5, "batch_ms_median_events": round(statistics.median(tb) * 1e3, 3),
                              "batch_ms_median_wall": round(statistics.median(walls) * 1e3, 3),
                              "clips_per_s": round(B / statistics.median(walls), 1),
                              "fbank_launch_ms_median": round(statistics.median(tf) * 1e3, 3),
                              "augment_launch_ms_median": round(statistics.median(ta) * 1e3, 4),
                              "augment_gb_per_s": round(aug_bytes / statistics.median(ta) / 1e9, 1)}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--mixup":
        mixup(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
