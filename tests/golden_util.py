"""Helpers shared by the tests: load committed golden fixtures, build oracle specs."""
import json
import os

import numpy as np
import torch

import vitlens_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def split(case):
    sd = {k[3:]: torch.from_numpy(v) for k, v in case.items() if k.startswith("sd/")}
    ins = {k[3:]: torch.from_numpy(v) for k, v in case.items() if k.startswith("in/")}
    outs = {k[4:]: torch.from_numpy(v) for k, v in case.items() if k.startswith("out/")}
    grads = {k[5:]: torch.from_numpy(v) for k, v in case.items() if k.startswith("grad/")}
    meta = json.loads(bytes(case["meta"]).decode()) if "meta" in case else {}
    return sd, ins, outs, grads, meta


def specs_from_meta(meta):
    cfg, a = meta["model_cfg"], meta["args"]
    v, t = cfg["vision_cfg"], cfg["text_cfg"]
    tower = O.TowerSpec(width=v["width"], layers=v["layers"], heads=v["width"] // v.get("head_width", 64),
                        patch=v["patch_size"], image_size=v["image_size"], embed_dim=cfg["embed_dim"])
    text = O.TextSpec(context_length=t["context_length"], vocab_size=t["vocab_size"], width=t["width"],
                      heads=t["heads"], layers=t["layers"], embed_dim=cfg["embed_dim"])
    mod = {"3dpc": "pc", "tactile": "image"}.get(a["visual_modality_type"], a["visual_modality_type"])
    lens = O.LensSpec(
        modality=mod, perceiver_identity=bool(a.get("perceiver_as_identity", False)),
        depth=a["perceiver_depth"], self_per_cross=a["perceiver_self_per_cross_attn"],
        num_latents=a["perceiver_num_latents"], latent_dim=a["perceiver_latent_dim"],
        input_chan=a["perceiver_input_chan"], cross_heads=a["perceiver_cross_heads"],
        cross_dim_head=a["perceiver_cross_dim_head"], latent_heads=a["perceiver_latent_heads"],
        latent_dim_head=a["perceiver_latent_dim_head"],
        audio_fstride=a.get("audio_fstride", 10), audio_tstride=a.get("audio_tstride", 10),
        audio_mel_bins=a.get("audio_mel_bins", 128), audio_target_length=a.get("audio_target_length", 512),
        eeg_chans=a.get("eeg_chans", 128), eeg_time_len=a.get("eeg_time_len", 512),
        eeg_window_size=a.get("eeg_window_size", 1), eeg_stride=a.get("eeg_stride", 1),
        pc_num_group=a.get("pc_num_group", 512), pc_group_size=a.get("pc_group_size", 32),
        pc_encoder_dims=a.get("pc_encoder_dims", 256), pc_trans_dim=a.get("pc_trans_dim", 384),
        use_orig_pos=not a.get("disable_orig_pos", False),
        disable_adapter_pos=bool(a.get("disable_visual_adapter_pos", False)),
        weight_tie_layers=bool(a.get("perceiver_weight_tie_layers", False)))
    return tower, text, lens


REFERENCE = os.path.join(GOLDEN, "reference")


def _inputs_digest(script, args, outputs=()):
    """What a stored reference output was computed from: the script, and each argument - a file the script writes
    (`outputs`) or a directory (the oracle / tests folders, a scratch folder) by its kind only, an input file by its
    content, anything else as given."""
    import hashlib
    h = hashlib.sha256(script.encode())
    for a in args:
        if a in outputs:
            h.update(b"out")
        elif os.path.isfile(a):
            with open(a, "rb") as f:
                h.update(b"file:" + hashlib.sha256(f.read()).digest())
        elif os.path.isdir(a):
            h.update(b"dir")
        else:
            h.update(b"arg:" + str(a).encode())
    return h.hexdigest()


def reference_run(key, script, args=(), files=(), timeout=600):
    """The reference's side of a comparison test, from tests/golden/reference/<key>/: what `python -c script *args` printed
    after "JSON" when it ran against the imported reference (stdout.json.xz), and the files it wrote (`files`, paths among
    `args`), which are put back where the script would have written them.  The suite needs no reference tree.  inputs.sha256
    records what the output was computed from (the script, and the input files by content); a test whose script or inputs
    changed since fails here instead of comparing against a stale output.

    To record (re)generate the outputs in a tree where the reference is importable (oracle/ref_loader.py finds it through
    VITLENS_REFERENCE), run the comparison tests with VITLENS_RECORD_REFERENCE=1: the script runs and its outputs are stored."""
    import lzma
    import subprocess
    import sys
    d = os.path.join(REFERENCE, key)
    digest = _inputs_digest(script, args, files)
    if os.environ.get("VITLENS_RECORD_REFERENCE") == "1":
        r = subprocess.run([sys.executable, "-c", script, *args], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-3000:]
        os.makedirs(d, exist_ok=True)
        with lzma.open(os.path.join(d, "stdout.json.xz"), "wt", encoding="utf-8") as f:
            f.write(r.stdout[r.stdout.index("JSON") + 4:].strip() if "JSON" in r.stdout else "null")
        for p in files:
            with open(p, "rb") as src, lzma.open(os.path.join(d, os.path.basename(p) + ".xz"), "wb") as dst:
                dst.write(src.read())
        with open(os.path.join(d, "inputs.sha256"), "w") as f:
            f.write(digest + "\n")
    else:
        with open(os.path.join(d, "inputs.sha256")) as f:
            stored = f.read().strip()
        assert stored == digest, (f"tests/golden/reference/{key} was recorded from another script or other inputs than this test "
                                  "now uses: record it again with VITLENS_RECORD_REFERENCE=1 where the reference is importable")
        for p in files:
            with lzma.open(os.path.join(d, os.path.basename(p) + ".xz"), "rb") as src, open(p, "wb") as dst:
                dst.write(src.read())
    with lzma.open(os.path.join(d, "stdout.json.xz"), "rt", encoding="utf-8") as f:
        return json.loads(f.read())


def seeded_like(stats, seed):
    """A state_dict from `stats` {name: [shape, mean, std, dtype]}: per tensor, in name order, normal values of that mean and
    standard deviation from one seeded generator (an integer buffer holds its mean).  The full-size reference comparisons
    load it into the reference model when they are recorded, and hand it to the oracle when they replay: a 1.7 GB state_dict
    is reproduced from a few kB."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in sorted(stats):
        shape, mean, std, dtype = stats[k]
        dt = getattr(torch, dtype.split(".")[-1])
        if dt.is_floating_point:
            sd[k] = (torch.randn(shape, generator=g) * std + mean).to(dt)
        else:
            sd[k] = torch.full(shape, round(mean), dtype=dt)
    return sd
