"""CPU: the host side of audio mix-up - the record vl_wave_clip_mix reads, the draws of AudioASTProcessorTrain.draw_mix, the
joined caption, what the two entries refuse before any launch, and that a call without `seconds=` draws what it drew
before."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proc(**kw):
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain
    return AudioASTProcessorTrain(device="cpu", **kw)


def test_mix_record_layout_matches_the_header():
    from vitlens_hip.audio import MIX_DTYPE, mix_record
    names = ("off_a", "ch_a", "len_a", "start_a", "off_b", "ch_b", "len_b", "start_b", "lam", "mu")
    assert MIX_DTYPE.itemsize == 40 and MIX_DTYPE.names == names
    assert [MIX_DTYPE.fields[k][1] for k in names] == [4 * i for i in range(10)]
    assert all(MIX_DTYPE.fields[k][0] == np.dtype("<i4") for k in names[:8]) and all(MIX_DTYPE.fields[k][0] == np.dtype("<f4") for k in names[8:])
    hdr = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    doc = hdr[hdr.index("recs: DEVICE array of one 40-byte record"):hdr.index("int vl_wave_clip_mix(")]
    assert "10 little-endian 32-bit words" in doc
    fields = re.findall(r"words (\d) \.\. (\d)\s+(int32|float) ([a-z_, ]+?)\s{2,}", doc)
    listed = [(int(lo), int(hi), kind, [s.strip() for s in nm.split(",")]) for lo, hi, kind, nm in fields]
    assert listed == [(0, 3, "int32", list(names[0:4])), (4, 7, "int32", list(names[4:8])), (8, 9, "float", list(names[8:10]))], listed
    # lam / mu: the float32 roundings of lambda and of the DOUBLE 1 - lambda (torch rounds the Python scalar 1 - lam once)
    lam = 0.5 + 0.6 * 2.0 ** -24            # float32: 0.5 + 2^-24;  1 - lam = 0.5 - 1.2 * 2^-25 -> 0.5 - 2^-25, not 0.5 - 2^-24
    r =np.array([mix_record((4, 1, 9, 2), (16, 2, 5, 4), lam)], dtype=MIX_DTYPE)[0]
    assert r["lam"] == np.float32(lam) and r["mu"] == np.float32(1.0 - lam) and r["mu"] != np.float32(1.0) - np.float32(lam)
    assert (r["off_b"], r["ch_b"], r["len_b"], r["start_b"]) == (16, 2, 5, 4)
    none = np.array([mix_record((4, 1, 9, 2))], dtype=MIX_DTYPE)[0]
    assert none["ch_b"] == 0
    with pytest.raises(ValueError):
        mix_record((4, 1, 9, 2), (16, 2, 5, 4))


def test_mix_mean_chain():
    from vitlens_hip.audio import mix_mean_chain
    assert mix_mean_chain(1) == 11 and mix_mean_chain(1024) == 11 and mix_mean_chain(1025) == 12
    assert mix_mean_chain(160000) == 167 < 500


def test_draw_mix_draws_nothing_when_off():
    p = _proc(seed=3)
    state = p.rng.getstate()
    assert p.draw_mix(100) == (None, None) and p.rng.getstate() == state
    assert _proc(seed=3, mix_up=True, mix_up_p=0.0).draw_mix(100) == (None, None)
    with pytest.raises(ValueError):
        _proc(mix_up=True, mix_up_p=1.5)


@pytest.mark.parametrize("p", [0.5, 0.2])
def test_draw_mix_statistics_and_order(p):
    proc = _proc(seed=11, mix_up=True, mix_up_p=p)
    replay = random.Random(11)
    n, lam_sum, hits = 20000, 0.0, 0
    for i in range(n):
        j, lam = proc.draw_mix(57)
        if replay.random() < p:                                  # the documented order: the coin, the partner, lambda
            assert (j, lam) == (replay.randint(0, 56), replay.betavariate(10, 10))
            assert 0 <= j < 57 and 0.0 < lam < 1.0
            hits += 1
            lam_sum += lam
        else:
            assert (j, lam) == (None, None)
    assert proc.rng.getstate() == replay.getstate()
    # sigma of the rate <= 0.5 / sqrt(n) = 0.0035; Beta(10, 10) has sigma 0.109, its mean over >= 3 000 draws 0.002
    assert abs(hits / n - p) < 0.02 and abs(lam_sum / hits - 0.5) < 0.005, (hits / n, lam_sum / hits)


def test_draw_mix_is_reproducible_from_the_seed():
    a, b, c = (_proc(seed=s, mix_up=True) for s in (5, 5, 6))
    da, db, dc = ([q.draw_mix(1000) for _ in range(200)] for q in (a, b, c))
    assert da == db and da != dc


def test_mix_caption():
    from open_clip.modal_audio.processors.at_processor import AudioASTProcessorTrain as P
    assert P.mix_caption("A dog barks.", "A Car Passes.") == "A dog barks and a car passes."
    assert P.mix_caption("A dog barks", "rain") == "A dog barks and rain"
    assert P.mix_caption("Speech..", "MUSIC") == "Speech. and music"               # one trailing period only
    assert P.mix_caption("a. b", "Wind, then Thunder") == "a. b and wind, then thunder"


def ptr(i):
    """A distinct, 16-byte aligned, non-null address per operand; never read or written."""
    return C.c_void_p(0x10000 * (i + 1))


def _refused(status, entry):
    from vitlens_hip import _lib
    assert status != 0 and _lib.load_library().vl_last_error().decode().startswith(entry)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Only argument sets that must be refused are passed, so nothing is ever launched or dereferenced."""
    from vitlens_hip import _lib
    lib = _lib.load_library()
    ok = dict(src=ptr(0), src_floats=1000, recs=ptr(1), out=ptr(2), means=None, batch=2, n=80)
    def clip(**kw):
        a = {**ok, **kw}
        return lib.vl_wave_clip_mix(a["src"], a["src_floats"], a["recs"], a["out"], a["means"], a["batch"], a["n"], None)
    for bad in (dict(src=None), dict(recs=None), dict(out=None), dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(batch=0), dict(batch=-3),
                dict(src_floats=0), dict(src_floats=2 ** 31), dict(recs=C.c_void_p(0x20002))):
        _refused(clip(**bad), "vl_wave_clip_mix")
    ok = dict(a=ptr(0), b=ptr(1), partner=ptr(2), lam_mu=ptr(3), out=ptr(4), rows=3, n=7)
    def rows(**kw):
        a = {**ok, **kw}
        return lib.vl_mix_rows(a["a"], a["b"], a["partner"], a["lam_mu"], a["out"], a["rows"], a["n"], None)
    for bad in (dict(a=None), dict(b=None), dict(partner=None), dict(lam_mu=None), dict(out=None), dict(rows=0), dict(n=0),
                dict(n=65535 * 1024 + 1), dict(out=ptr(1))):
        _refused(rows(**bad), "vl_mix_rows")


def test_records_are_checked_where_they_are_packed():
    from vitlens_hip.audio import MIX_DTYPE, check_mix_records, mix_record
    good = [mix_record((0, 2, 10, 9), (20, 1, 7, 0), 0.4), mix_record((27, 1, 3, 2))]
    check_mix_records(np.array(good, dtype=MIX_DTYPE), 16, 30)
    bad = [mix_record((0, 0, 10, 0)), mix_record((0, 1, 0, 0)), mix_record((0, 1, 10, 10)), mix_record((0, 1, 10, -1)),
           mix_record((-1, 1, 10, 0)), mix_record((21, 1, 10, 0)), mix_record((0, 2, 10, 0), (20, 1, 11, 0), 0.5),
           mix_record((0, 2, 5, 0), (10, 3, 5, 0), 0.5), mix_record((0, 1, 5, 0), (10, 1, 5, 5), 0.5)]
    for r in bad:
        with pytest.raises(ValueError):
            check_mix_records(np.array([good[0], r], dtype=MIX_DTYPE), 16, 30)
    for n, floats in ((0, 30), (16, 0), (2 ** 31, 30)):
        with pytest.raises(ValueError):
            check_mix_records(np.array(good, dtype=MIX_DTYPE), n, floats)
    with pytest.raises(ValueError):
        check_mix_records(np.zeros(2, dtype=np.int32), 16, 30)


def _items():
    g = torch.Generator().manual_seed(2)
    return [torch.randn(80000, generator=g) * 0.1, torch.randn(2, 144000, generator=g) * 0.1, torch.randn(1, 30000, generator=g) * 0.1,
            torch.randn(1, 100000, generator=g) * 0.1]


def test_plan_clip_is_the_host_clip_with_the_same_draws():
    """The indices the device path works from name exactly the clip the host path builds, from the same random numbers."""
    from open_clip.modal_audio.processors.at_processor import audio_get_clip
    host, plan = _proc(seed=8), _proc(seed=8)
    for item in _items():
        ref = host.load_audio_clip(item)
        src, a, b, start = plan.plan_clip(item)
        assert plan.rng.getstate() == host.rng.getstate()
        cut = src.cut(a, b)
        t = torch.arange(80000)
        clip = cut[:, (start + t) % cut.shape[1]]
        assert torch.equal(clip - clip.mean(), ref)
    short = torch.zeros(1, 1000)                                     # 80 000 / 1 000 needs 7 doublings
    with pytest.raises(ValueError, match="too short"):
        plan.plan_clip(short)
    with pytest.raises(ValueError, match="too short"):
        audio_get_clip(short, 16000, 5.0)


def test_without_seconds_the_processor_draws_what_it_drew_before(monkeypatch):
    """batch(items) (`seconds=None`) of a mix-up processor and of a plain one leave the generator where the per-item
    sequence load_audio_clip, draw_params leaves it; the device path consumes the same for rows without a partner."""
    from vitlens_hip import audio
    items = _items()
    seen = {}
    monkeypatch.setattr(audio, "kaldi_fbank", lambda wave, **kw: seen.setdefault("wave", wave))
    monkeypatch.setattr(audio, "augment_params", lambda rows, device: rows)
    monkeypatch.setattr(audio, "fbank_augment", lambda raw, rows, mean, std: rows)
    replay = _proc(seed=21)
    want = []
    for it in items:
        replay.load_audio_clip(it)
        want.append(replay.draw_params())
    for kw in ({}, {"mix_up": True}):
        p = _proc(seed=21, **kw)
        assert p.batch(items) == want and p.rng.getstate() == replay.rng.getstate()
        assert seen.pop("wave").shape == (4, 80000)
    # the device path, stopped at the launch: the same draws for rows without a partner
    monkeypatch.setattr(audio, "wave_clip_mix", lambda buf, recs, n, means=False, recs_dev=None: recs)
    p = _proc(seed=21, mix_up=True)
    recs, rows = p._device_clips(items, None, None, [None] * 4, None, None)
    assert rows == want and p.rng.getstate() == replay.rng.getstate()
    assert (recs["ch_b"] == 0).all() and list(recs["ch_a"]) == [1, 2, 1, 1] and list(recs["len_a"]) == [80000, 80000, 30000, 80000]
    assert (recs["off_a"] % 4 == 0).all() and recs["off_a"][0] >= 40
    with pytest.raises(ValueError, match="lambda"):
        p._device_clips(items[:1], None, None, [items[1]], None, None)
    with pytest.raises(ValueError, match="broadcast"):
        p._device_clips([torch.zeros(2, 80000)], None, None, [torch.zeros(3, 80000)], [0.5], None)
