"""GPU: every evaluation driver of training/zero_shot.py on the stub model of tests/eval_stub.py, with the texts the reference's
templates produced as `templates`, against what the reference's drivers returned on the same stubs (tests/eval_recorded.py):
integer counts equal, percentages within 1e-4 points (the reference forms each batch's percentage in float32, which costs up to
1e-5 per batch), mAP within 1e-9, the recall dictionary equal; and nothing is read on the host inside the batch loop."""
import contextlib
import io
import json
from types import SimpleNamespace

import pytest
import torch

import eval_recorded
import eval_stub

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def recorded():
    return eval_recorded.recorded()


@pytest.fixture(scope="module")
def Z():
    import training.zero_shot as z
    return z


@pytest.fixture()
def args(tmp_path):
    with open(tmp_path / "templates.json", "w") as f:
        json.dump({"p": eval_stub.PC_TEMPLATES}, f)
    with open(tmp_path / "labels.json", "w") as f:
        json.dump({"d": eval_stub.PC_LABELS}, f)
    return SimpleNamespace(device=DEV, distributed=False, log_every_n_steps=1000, val_data_prompt="p", val_data="d",
                           pc_meta_data_dir=str(tmp_path))


class Watched(list):
    """A loader that notes how many host reads (`.item`, `.tolist`, `.cpu`) had happened when it handed out its first batch
    and when it was asked for the one after the last."""

    def __init__(self, loader, reads):
        super().__init__(loader)
        self.dataset, self.reads, self.marks = loader.dataset, reads, []

    def __iter__(self):
        for i, batch in enumerate(list.__iter__(self)):
            if i == 0:
                self.marks.append(self.reads[0])
            yield batch
        self.marks.append(self.reads[0])


@contextlib.contextmanager
def counting_reads():
    reads = [0]
    saved = {n: getattr(torch.Tensor, n) for n in ("item", "tolist", "cpu")}

    def wrap(fn):
        def counted(self, *a, **k):
            reads[0] += 1
            return fn(self, *a, **k)
        return counted
    for n, fn in saved.items():
        setattr(torch.Tensor, n, wrap(fn))
    try:
        yield reads
    finally:
        for n, fn in saved.items():
            setattr(torch.Tensor, n, fn)


def _run(Z, name, recorded, args, hook=None, **kw):
    driver, loader = eval_stub.cases()[name]
    rec = recorded[name]
    model, tok = eval_stub.StubModel(DEV), eval_stub.StubTokenizer()
    out = io.StringIO()
    with counting_reads() as reads, contextlib.redirect_stdout(out):
        watched = Watched(loader, reads)
        if driver == "test_zeroshot_3d_core":
            res = Z.test_zeroshot_3d_core(watched, model, tok, args, **kw)
        elif driver == "test_audio_single_ret":
            res = getattr(Z, driver)(watched, model, tok, name, args)
        else:
            res = getattr(Z, driver)(watched, model, tok, name, args, templates=eval_recorded.templates_of(rec, loader.dataset.idx2label))
    assert len(watched.marks) == 2 and watched.marks[0] == watched.marks[1], f"{name}: host reads inside the batch loop"
    assert tok.texts == rec["texts"], name                     # the same prompts, in the same order, reached the tokenizer
    return res, rec, out.getvalue()


def _check_percent(res, rec, keys):
    want = rec["result"]
    assert set(res) == set(want) == set(keys)
    for i, key in enumerate(keys):
        hits = round(res[key] * rec["n"] / 100.0)
        assert abs(res[key] - 100.0 * hits / rec["n"]) < 1e-9 and hits == rec["hits"][i], (key, res[key], rec["hits"])
        assert abs(res[key] - want[key]) <= 1e-4, (key, res[key], want[key])


@pytest.mark.parametrize("name", ("rgbd_others", "rgbd_plain", "tactile_6", "eeg"))
def test_top1_top5_drivers(Z, recorded, args, name):
    res, rec, _ = _run(Z, name, recorded, args)
    _check_percent(res, rec, ("acc1", "acc5"))


def test_tactile_below_five_classes_has_acc1_only(Z, recorded, args):
    res, rec, _ = _run(Z, "tactile_3", recorded, args)
    _check_percent(res, rec, ("acc1",))
    assert "acc5" not in res


def test_3d_driver_and_its_per_class_lines(Z, recorded, args):
    res, rec, printed = _run(Z, "3d", recorded, args)
    assert set(res) == {"modelnet40"}
    _check_percent(res["modelnet40"], {"result": rec["result"]["modelnet40"], "hits": rec["hits"], "n": rec["n"]}, ("acc1", "acc5"))
    assert printed.strip().split("\n")[-3:] == rec["per_class_lines"]
    (res2, per_class), _, _ = _run(Z, "3d", recorded, args, return_per_class=True)
    assert res2 == res and ",".join(per_class["names"]) == rec["per_class_lines"][0]
    assert sum(per_class["count"].values()) == rec["n"]
    assert ",".join(str(per_class["top5"][n]) for n in per_class["names"]) == rec["per_class_lines"][2]


def test_3d_driver_says_where_the_meta_data_goes(Z, args):
    args.pc_meta_data_dir = None
    with pytest.raises(ValueError, match="pc_meta_data_dir"):
        Z.test_zeroshot_3d_core(eval_stub.cases()["3d"][1], eval_stub.StubModel(DEV), eval_stub.StubTokenizer(), args)


@pytest.mark.parametrize("name", ("audio_map", "audio_map_1clip"))
def test_audio_map_driver(Z, recorded, args, name, monkeypatch):
    for on_device in (True, False):
        monkeypatch.setattr(Z, "MAP_ON_DEVICE", on_device)
        res, rec, _ = _run(Z, name, recorded, args)
        want = rec["result"]
        assert set(res) == set(want) and res["map_cnt"] == want["map_cnt"] and res["predict_results"] == {}
        print(f"{name} on_device={on_device}: map {res['map']!r} reference {want['map']!r}")
        assert abs(res["map"] - want["map"]) <= 1e-9 and res["acc1"] == res["map"]


@pytest.mark.parametrize("name", ("audio_cls", "audio_cls_3clip"))
def test_audio_cls_driver(Z, recorded, args, name):
    res, rec, _ = _run(Z, name, recorded, args)
    want = rec["result"]
    assert set(res) == set(want)
    assert res["score_sum"] == want["score_sum"] == rec["hits"][0] and res["score_cnt"] == want["score_cnt"] == rec["n"]
    assert res["accuracy"] == want["accuracy"] and res["acc1"] == want["acc1"] and res["predict_results"] == {}


def test_audio_ret_driver(Z, recorded, args):
    res, rec, _ = _run(Z, "audio_ret", recorded, args)
    want = rec["result"]
    assert set(res) == set(want) and not any(k.startswith("img") for k in res)
    for k, v in want.items():
        assert res[k] == pytest.approx(v, abs=1e-12) if isinstance(v, float) else res[k] == v, k


def test_core_drivers_dispatch(Z, recorded, args):
    cases = eval_stub.cases()
    model, tok = eval_stub.StubModel(DEV), eval_stub.StubTokenizer()
    for name in ("rgbd_plain", "tactile_3", "eeg", "audio_cls", "audio_map_1clip"):
        cases[name][1].dataset.templates = eval_recorded.templates_of(recorded[name], cases[name][1].dataset.idx2label)
    with contextlib.redirect_stdout(io.StringIO()):
        r = Z.test_rgbd_cls_core({"a": cases["rgbd_plain"][1]}, model, tok, args)
        t = Z.test_tactiletasks_core(cases["tactile_3"][1], model, tok, args)
        e = Z.test_eegtasks_core({"x": cases["eeg"][1]}, model, tok, args)
        a = Z.test_audiotasks_core({"cls": cases["audio_cls"][1], "map": cases["audio_map_1clip"][1], "ret": cases["audio_ret"][1]},
                                   model, tok, args)
    assert set(r) == {"a"} and abs(r["a"]["acc1"] - recorded["rgbd_plain"]["result"]["acc1"]) <= 1e-4
    assert set(t) == {"Single Eval"} and set(t["Single Eval"]) == {"acc1"}
    assert set(e) == {"x"} and abs(e["x"]["acc5"] - recorded["eeg"]["result"]["acc5"]) <= 1e-4
    assert set(a) == {"cls", "map", "ret"} and a["cls"]["acc1"] == recorded["audio_cls"]["result"]["acc1"]
    assert abs(a["map"]["acc1"] - recorded["audio_map_1clip"]["result"]["map"]) <= 1e-9
    assert a["ret"]["acc1"] == pytest.approx(recorded["audio_ret"]["result"]["acc1"], abs=1e-12)
    with pytest.raises(ValueError, match="templates"):
        Z.test_eeg_cls_single(eval_stub.cases()["eeg"][1], model, tok, "x", args)
