"""CPU: the resampler's two float64 restatements agree (tests/resample_ref.py), and the compact polyphase table the kernel
reads (vitlens_hip.audio.sinc_resample_table) is the dense torchaudio kernel with nothing but float32 rounding lost."""
import numpy as np
import pytest

import resample_ref as R

RATES = [(48000, 16000), (44100, 16000), (32000, 16000), (24000, 16000), (22050, 16000), (11025, 16000), (8000, 16000),
         (16000, 44100)]


@pytest.mark.parametrize("orig,new", RATES)
def test_dense_and_direct_forms_agree(orig, new):
    rng = np.random.default_rng(orig)
    o, n, _, _ = R.geometry(orig, new)
    for length in (1, 5, 20, 1000):
        x = rng.standard_normal(length)
        yd, sd = R.resample_dense(x, orig, new)
        yr, sr = R.resample_direct(x, orig, new)
        assert len(yd) == len(yr) == -((-n * length) // o) == R.out_length(length, orig, new)
        err = np.abs(yd - yr).max()
        print(f"{orig}->{new} len {length}: dense vs direct {err:.2e}")
        assert err <= 1e-11 * np.abs(x).max()
        assert np.abs(sd - sr).max() <= 1e-11 * np.abs(x).max()


@pytest.mark.parametrize("orig,new", RATES)
def test_compact_table_is_the_dense_kernel(orig, new):
    from vitlens_hip.audio import resample_geometry, resampled_length, sinc_resample_table
    o, n, base, W = R.geometry(orig, new)
    assert resample_geometry(orig, new) == (o, n, base, W)
    assert resampled_length(1000, orig, new) == R.out_length(1000, orig, new)
    offsets, taps = sinc_resample_table(orig, new)
    assert sinc_resample_table(orig, new)[1] is taps                                 # cached
    offsets, taps = offsets.numpy(), taps.numpy()
    K = 2 * W + 1
    assert offsets.dtype == np.int32 and taps.dtype == np.float32 and offsets.shape == (n,) and taps.shape == (n, K)
    assert (offsets >= 0).all() and (offsets <= o - 1).all()                         # every slice lies inside the dense row
    dense = R.dense_kernel(orig, new)
    back = np.zeros_like(dense)
    for p in range(n):
        back[p, offsets[p]:offsets[p] + K] = taps[p]
    peak = np.abs(dense).max()
    assert np.abs(back - dense).max() <= 2.0 ** -24 * peak
    assert (np.count_nonzero(taps, axis=1) <= 2 * W).all()
    sums = dense.sum(axis=1)
    assert 1.00003 < sums.min() and sums.max() < 1.001


def test_launcher_refuses_bad_shapes():
    """Shape checks come before any launch, so they run without a GPU."""
    from vitlens_hip._lib import load_library
    lib = load_library()
    ok = dict(in_stride=100, batch=1, n_in=100, o=3, n=1, K=39, out_stride=34, out_first=0, n_out=34)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vl_resample_sinc(None, a["in_stride"], a["batch"], a["n_in"], None, None, a["o"], a["n"], a["K"], None,
                                    a["out_stride"], a["out_first"], a["n_out"], None)
    for bad in (dict(batch=0), dict(n_in=0), dict(K=38), dict(in_stride=99), dict(out_first=1), dict(n_out=35, out_stride=35),
                dict(out_first=-1), dict(n_out=0), dict(o=44101, n=16000, K=35, n_out=30, out_stride=30)):
        assert call(**bad) != 0, bad
        assert b"vl_resample_sinc" in lib.vl_last_error()
    assert lib.vl_fbank_augment(None, None, 1, 512, 128, None, 0.0, 0.0, None) != 0          # std = 0
    assert lib.vl_fbank_augment(None, None, 0, 512, 128, None, 0.0, 1.0, None) != 0
    assert b"vl_fbank_augment" in lib.vl_last_error()


def test_resample_refuses_cpu_tensors():
    import torch
    from vitlens_hip.audio import fbank_augment, resample
    with pytest.raises(RuntimeError):
        resample(torch.zeros(100), 44100, 16000)
    with pytest.raises(RuntimeError):
        fbank_augment(torch.zeros(1, 8, 4), torch.zeros(1, 8, dtype=torch.int32), 0.0, 1.0)
