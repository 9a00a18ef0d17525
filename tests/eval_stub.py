"""Stub model, tokenizer, datasets and loaders for the evaluation drivers (training/zero_shot.py), shared by the script that
records the reference's drivers (tests/test_eval_host.py) and the GPU tests that replay them (tests/test_hip_eval_drivers.py).

Every feature is a table LOOKUP, so both sides see the same bits whatever the device: a sample's input tensor carries its
row of the visual table in its first element, and the tokenizer turns a text into one id (a CRC of its characters) that
selects a row of the text table.  The tables hold multiples of 2^-15 drawn from a seeded integer stream."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch

E, N_VIS, N_TXT, B = 32, 512, 4096, 48
SEED = 17
SPLITS = {"even": (16, 16, 16), "ragged": (20, 20, 8)}


def tables(seed=SEED):
    rng = np.random.default_rng(seed)
    vis = (rng.integers(-2 ** 15, 2 ** 15, (N_VIS, E)) / 2.0 ** 15).astype(np.float32)
    txt = (rng.integers(-2 ** 15, 2 ** 15, (N_TXT, E)) / 2.0 ** 15).astype(np.float32)
    return torch.from_numpy(vis), torch.from_numpy(txt)


class StubTokenizer:
    """text -> one id, deterministically; keeps the texts it was given, in order."""

    def __init__(self):
        self.texts = []

    def __call__(self, texts):
        texts = [texts] if isinstance(texts, str) else list(texts)
        self.texts.extend(texts)
        return torch.tensor([[zlib.crc32(t.encode("utf-8")) % N_TXT] for t in texts], dtype=torch.long)


class StubModel:
    def __init__(self, device="cpu", seed=SEED):
        vis, txt = tables(seed)
        self.vis, self.txt = vis.to(device), txt.to(device)

    def eval(self):
        return self

    def encode_text(self, ids):
        return self.txt[ids.reshape(ids.shape[0], -1)[:, 0]]

    def encode_visual(self, x):
        return self.vis[x.reshape(x.shape[0], -1)[:, 0].long()]


class Loader(list):
    """A list of batch dictionaries with the `dataset` attribute the drivers read."""

    def __init__(self, batches, dataset):
        super().__init__(batches)
        self.dataset = dataset


def _inputs(rows, shape):
    """Input tensors whose first element is the sample's (or clip's) row of the visual table."""
    x = torch.zeros(len(rows), *shape)
    x.reshape(len(rows), -1)[:, 0] = torch.tensor(rows, dtype=torch.float32)
    return x


def _names(C, stem):
    return [f"{stem} {i}" for i in range(C)]


def _cut(split):
    edges = np.cumsum((0,) + SPLITS[split])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def cls_case(kind, C, split, seed, first_row, as_list=False, others=None, n_clip=1, names=None):
    """A single-label case: `kind` in pc / depth / tactile / eeg / audio."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, B)
    names = names or _names(C, kind + " class")
    ds = SimpleNamespace(idx2label=names, label2idx={n: i for i, n in enumerate(names)}, split="material", eval_metric="acc")
    if others is not None:
        ds.other_idx, ds.map_to_others_idx = others
    batches = []
    for a, b in _cut(split):
        lab = labels[a:b].tolist() if as_list else torch.from_numpy(labels[a:b]).long()
        rows = list(range(first_row + a * n_clip, first_row + b * n_clip))
        if kind == "audio":
            x = _inputs(rows, (4, 4)).reshape(b - a, n_clip, 4, 4) if n_clip > 1 else _inputs(rows, (4, 4))
            batches.append({"id": list(range(a, b)), "audio": x, "label": lab})
        else:
            batch = {kind: _inputs(rows, (5, 3)), "label": lab}
            if kind == "pc":
                batch["class_name"] = [names[i] for i in labels[a:b]]
            if kind == "depth":
                batch["cleaned_label"] = [names[i] for i in labels[a:b]]
            batches.append(batch)
    return Loader(batches, ds), labels


def map_case(C, split, seed, first_row, n_clip):
    rng = np.random.default_rng(seed)
    targets = (rng.random((B, C)) < 0.3).astype(np.float32)
    targets[0, :] = 1.0                                          # every class has a positive
    names = _names(C, "sound")
    ds = SimpleNamespace(idx2label=names, eval_metric="map")
    batches = []
    for a, b in _cut(split):
        rows = list(range(first_row + a * n_clip, first_row + b * n_clip))
        x = _inputs(rows, (4, 4)).reshape(b - a, n_clip, 4, 4) if n_clip > 1 else _inputs(rows, (4, 4))
        batches.append({"id": list(range(a, b)), "audio": x, "target": torch.from_numpy(targets[a:b])})
    return Loader(batches, ds), targets


def ret_case(split, first_row, n_clip, n_texts=60):
    ds = SimpleNamespace(texts=[f"caption number {i} of the retrieval set" for i in range(n_texts)],
                         text_ids=[i % B for i in range(n_texts)], eval_metric="recall")
    batches = []
    for a, b in _cut(split):
        rows = list(range(first_row + a * n_clip, first_row + b * n_clip))
        x = _inputs(rows, (4, 4)).reshape(b - a, n_clip, 4, 4) if n_clip > 1 else _inputs(rows, (4, 4))
        batches.append({"audio": x, "uniq_id": list(range(a, b))})
    return Loader(batches, ds)


PC_LABELS = _names(12, "shape")
PC_TEMPLATES = ["a point cloud model of {}.", "there is a {} in the scene.", "a 3d rendering of a {}."]


def cases():
    """name -> (driver name, loader).  Sizes: B = 48 in batches of 16 + 16 + 16 or 20 + 20 + 8, C in {3, 6, 12}, n_clip in
    {1, 3}; every case has its own rows of the visual table."""
    return {
        "3d": ("test_zeroshot_3d_core", cls_case("pc", 12, "even", 11, 0, as_list=True, names=PC_LABELS)[0]),
        "rgbd_others": ("test_rgbd_cls_single", cls_case("depth", 12, "ragged", 12, 48, others=(11, [2, 5, 7]))[0]),
        "rgbd_plain": ("test_rgbd_cls_single", cls_case("depth", 6, "even", 13, 96)[0]),
        "audio_map": ("test_audio_single_map", map_case(12, "even", 14, 144, 3)[0]),
        "audio_map_1clip": ("test_audio_single_map", map_case(6, "ragged", 15, 288, 1)[0]),
        "audio_cls": ("test_audio_single_cls", cls_case("audio", 6, "ragged", 16, 336, n_clip=1)[0]),
        "audio_cls_3clip": ("test_audio_single_cls", cls_case("audio", 12, "even", 17, 144, as_list=True, n_clip=3)[0]),
        "audio_ret": ("test_audio_single_ret", ret_case("ragged", 144, 3)),
        "tactile_3": ("test_tactle_cls_single", cls_case("tactile", 3, "even", 18, 384)[0]),
        "tactile_6": ("test_tactle_cls_single", cls_case("tactile", 6, "ragged", 19, 432, as_list=True)[0]),
        "eeg": ("test_eeg_cls_single", cls_case("eeg", 6, "ragged", 20, 464)[0]),
    }
