"""CPU: the oracle's restatement of the `pnsa` point tokenizer (PointNet set abstraction,
open_clip/modal_3d/models/pointnet/pointnet_util.py:345-368) against the imported reference class.

The reference module imports `dgl.geometry` and `torch_redstone` at module level; neither is installed.  For THIS test
the two names are provided as empty shells: with `dgl.geometry.farthest_point_sampler` missing the reference's own
`farthest_point_sample` takes its documented fallback (pointnet_util.py:83-98, a torch FPS whose start index comes from
`torch.randint` - seeded here and replayed into the oracle), and `rst.Lambda` is the one-line module wrapper it is in
torch_redstone.  Nothing of this is product code: the product has no pnsa tokenizer yet; this pins
the oracle the kernel will be built against."""
import os
from types import SimpleNamespace

import pytest
import torch

import vitlens_oracle as O
from golden_util import reference_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = r'''
import json, sys
from types import SimpleNamespace
import torch
sys.path.insert(0, sys.argv[1])
import ref_loader
ref = ref_loader.load_pointnet_util()
training = sys.argv[2] == "train"
cfg = SimpleNamespace(num_group=24, radius=0.35, group_size=8, in_dim=3, encoder_dims=32, trans_dim=48)
torch.manual_seed(0)
tok = ref.PointNSATokenizer(cfg)
with torch.no_grad():
    for bn in tok.sa.mlp_bns:                                                 # non-trivial running statistics for eval mode
        bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5)
        bn.weight.normal_(1, 0.1); bn.bias.normal_(0, 0.1)
tok.train(training)
g = torch.Generator().manual_seed(1)
B, N = 3, 400
xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
feats = torch.rand(B, N, 3, generator=g)
sd = {k: [str(v.dtype), list(v.shape), v.detach().reshape(-1).tolist()] for k, v in tok.state_dict().items()}
torch.manual_seed(7)
start = torch.randint(0, N, (B,), dtype=torch.long)                           # what the fallback FPS draws first
torch.manual_seed(7)
with torch.no_grad():
    want = tok(feats, xyz=xyz)["x"]
torch.manual_seed(7)
cidx = ref.farthest_point_sample(xyz, cfg.num_group)
new_xyz = ref.index_points(xyz, cidx)
print("JSON" + json.dumps({"sd": sd, "start": start.tolist(), "tokens": want.tolist(), "fps": cidx.tolist(),
                           "ball": ref.query_ball_point(cfg.radius, cfg.group_size, xyz, new_xyz).tolist(),
                           "ball_tight": ref.query_ball_point(0.05, 8, xyz, new_xyz).tolist()}))
'''


@pytest.mark.parametrize("training", [False, True])
def test_pnsa_tokens_equal_the_reference(training):
    """The reference's PointNSATokenizer (imported when recorded) on seeded weights and points: its state_dict, tokens, FPS
    picks and ball-query indices, against the oracle on the same state_dict and points."""
    ref = reference_run(f"test_oracle_pnsa.test_pnsa_tokens_equal_the_reference.{'train' if training else 'eval'}", _REF,
                        [os.path.join(ROOT, "oracle"), "train" if training else "eval"])
    cfg = SimpleNamespace(num_group=24, radius=0.35, group_size=8, in_dim=3, encoder_dims=32, trans_dim=48)
    sd = {"a." + k: torch.tensor(v, dtype=getattr(torch, dt.split(".")[-1])).reshape(sh) for k, (dt, sh, v) in ref["sd"].items()}
    g = torch.Generator().manual_seed(1)
    B, N = 3, 400
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    feats = torch.rand(B, N, 3, generator=g)
    start = torch.tensor(ref["start"])
    want = torch.tensor(ref["tokens"])
    got, cidx, bidx = O.pnsa_tokens(sd, "a.", feats, xyz, cfg.num_group, cfg.radius, cfg.group_size, start, training=training)
    assert got.shape == want.shape == (B, cfg.num_group, cfg.trans_dim)
    assert float((got - want).abs().max()) < 2e-5, float((got - want).abs().max())
    # the pieces, individually: FPS picks, ball query (incl. short groups filled with the first index)
    assert torch.equal(cidx, torch.tensor(ref["fps"]))
    assert torch.equal(bidx, torch.tensor(ref["ball"]))
    new_xyz = torch.stack([xyz[b, cidx[b]] for b in range(B)])
    tight = torch.tensor(ref["ball_tight"])
    assert torch.equal(O.ball_query_indices(0.05, 8, xyz, new_xyz), tight)
    assert bool((tight == tight[..., :1]).all(-1).any())                          # some groups hold only their centre


def test_pnsa_oracle_against_the_committed_golden():
    """tests/golden/tiny_pnsa.npz (generated from the reference by oracle/gen_golden.py --only pnsa 31): tokens in eval and
    train mode, FPS / ball-query indices bit-exact, and every parameter gradient of a random upstream gradient through
    the oracle's autograd.  This is the fixture the HIP pnsa tokenizer will be checked against on the GPU box."""
    import json
    import numpy as np
    from golden_util import GOLDEN
    z = np.load(os.path.join(GOLDEN, "tiny_pnsa.npz"))
    cfg = json.loads(str(z["meta"]))["cfg"]
    sd = {"a." + k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd/")}
    xyz, feats, start = torch.tensor(z["in/xyz"]), torch.tensor(z["in/features"]), torch.tensor(z["in/fps_start"])
    args = (cfg["num_group"], cfg["radius"], cfg["group_size"], start)
    ev, cidx, bidx = O.pnsa_tokens(sd, "a.", feats, xyz, *args, training=False)
    assert torch.equal(cidx, torch.tensor(z["out/fps_idx"])) and torch.equal(bidx, torch.tensor(z["out/ball_idx"]))
    assert float((ev - torch.tensor(z["out/eval/tokens"])).abs().max()) < 2e-5
    sdr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v) for k, v in sd.items()}
    tr, _, _ = O.pnsa_tokens(sdr, "a.", feats, xyz, *args, training=True)
    assert float((tr.detach() - torch.tensor(z["out/train/tokens"])).abs().max()) < 2e-5
    tr.backward(torch.tensor(z["in/dctx"]))
    n = 0
    for k in z.files:
        if k.startswith("grad/"):
            g, want = sdr["a." + k[5:]].grad, torch.tensor(z[k])
            if "mlp_convs" in k and k.endswith(".bias"):
                # a per-channel constant in front of a train-mode BatchNorm is removed by the batch mean: identically zero
                # gradient, both sides hold round-off only
                wn = float(torch.tensor(z[k[:-4] + "weight"]).norm())
                assert float(want.norm()) < 1e-3 * wn and float(g.norm()) < 1e-3 * wn, k
            else:
                assert float((g - want).norm() / (want.norm() + 1e-12)) < 1e-4, k
            n += 1
    assert n == 16
