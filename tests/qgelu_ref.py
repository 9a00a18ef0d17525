"""Reference arithmetic for the QuickGELU tests: the activation of the OpenAI-pretrained CLIP towers, x * sigmoid(1.702 x)
(the reference's `QuickGELU`, open_clip/transformer.py:37), its derivative s + 1.702 x s (1 - s), and a way to make the oracle
(oracle/vitlens_oracle.py, which hard-codes the exact-erf GELU) compute a QuickGELU tower.

`quick_gelu_oracle()` swaps the oracle's `gelu_erf` for the fp32 QuickGELU while the block is open.  The oracle calls that one
function from the transformer blocks' MLP, the Perceiver's GEGLU and the point tokenizer's position MLP; in the reference
`quick_gelu` reaches only the first.  So the swap is for oracle calls whose sole GELU is the block MLP - encode_image,
encode_text, a Lens with an identity Perceiver - and never around a Perceiver or PointBERT Lens."""
import contextlib

import torch

import vitlens_oracle as O


def qgelu(x: torch.Tensor) -> torch.Tensor:
    """fp64 x * sigmoid(1.702 x)."""
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x: torch.Tensor) -> torch.Tensor:
    """fp64 d/dx [x * sigmoid(1.702 x)] = s + 1.702 x s (1 - s)."""
    x = x.double()
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def quick_gelu_f32(x: torch.Tensor) -> torch.Tensor:
    """The reference module's forward in the tensor's own dtype: `x * torch.sigmoid(1.702 * x)`."""
    return x * torch.sigmoid(1.702 * x)


@contextlib.contextmanager
def quick_gelu_oracle():
    saved = O.gelu_erf
    O.gelu_erf = quick_gelu_f32
    try:
        yield
    finally:
        O.gelu_erf = saved
