"""Sequential restatement, in torch on the CPU, of the tactile recipe's training transform (reference
open_clip/modal_tactile/processors/tact_processor.py:189-233): ToTensor, RandomResizedCrop(bilinear), RandomHorizontalFlip,
RandomVerticalFlip, RandomRotation((0, 360), nearest, fill 0), Normalize - one stage after the other on the whole tensor, as
the reference's Compose runs them, in float32 or float64, for given scalars; and the draw of those scalars in the order of
that pipeline.  The resampler is torch.nn.functional.interpolate itself and the rotation's sampling is torch's linspace, bmm
and grid_sample; the torchvision glue around them is restated from its published source (functional: rotate,
_get_inverse_affine_matrix; _functional_tensor: rotate, _gen_affine_grid, _apply_grid_transform; transforms: get_params of
RandomResizedCrop and RandomRotation).  Shared by tests/test_tactile_augment_host.py, tests/test_hip_tactile_augment.py and
tools/preproc_bench.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from rgbd_augment_ref import CLIP_MEAN, CLIP_STD, crop_box  # noqa: F401  (the same RandomResizedCrop.get_params)


# ------------------------------------------------------------------------------------------------ the draws
def draw(H, W, degrees=(0.0, 360.0)):
    """One sample's scalars from torch's global generator, stage by stage in the order of the reference's Compose."""
    d = {"box": crop_box(H, W)}                                                   # RandomResizedCrop
    d["flip_h"] = bool(torch.rand(1) < 0.5)                                       # RandomHorizontalFlip
    d["flip_v"] = bool(torch.rand(1) < 0.5)                                       # RandomVerticalFlip
    d["angle"] = float(torch.empty(1).uniform_(float(degrees[0]), float(degrees[1])).item())   # RandomRotation.get_params
    return d


# ------------------------------------------------------------------------------------------------ the rotation
def inverse_matrix(angle):
    """torchvision functional._get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1.0, [0, 0]) as F.rotate of a tensor calls
    it -> six Python doubles."""
    rot = math.radians(-angle)
    sx = sy = math.radians(0.0)
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    return [v / 1.0 for v in (d, -b, 0.0, -c, a, 0.0)]      # scale 1; centre and translation 0 leave entries 2 and 5 at 0


def tv_rotate(img, angle, fill=0.0):
    """F.rotate(img, angle, NEAREST, expand=False, center=None, fill) for a float32 [C, H, W] tensor, torchvision's tensor
    path: theta in the image's dtype, the base grid from torch.linspace, the grid by bmm with the rescaled theta,
    F.grid_sample(nearest, zeros, align_corners=False) on the image with a channel of ones appended, fill where that is < 0.5."""
    assert img.dtype == torch.float32 and img.dim() == 3
    h, w = img.shape[-2:]
    theta = torch.tensor(inverse_matrix(angle), dtype=img.dtype).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, h, w, 3, dtype=theta.dtype)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + d, w * 0.5 + d - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + d, h * 0.5 + d - 1, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype)
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)
    x = img.unsqueeze(0)
    x = torch.cat((x, torch.ones((1, 1, h, w), dtype=x.dtype)), dim=1)
    x = F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    mask = x[:, -1:, :, :]
    x = x[:, :-1, :, :]
    mask = mask.expand_as(x)
    fills = fill if isinstance(fill, (tuple, list)) else [float(fill)]
    fill_img = torch.tensor(fills, dtype=x.dtype).view(1, len(fills), 1, 1).expand_as(x)
    mask = mask < 0.5
    x[mask] = fill_img[mask]
    return x[0]


def tv_index(S, angle):
    """The pixel of an S x S image that `tv_rotate` puts at each output pixel -> int64 [S, S] of sy * S + sx, -1 for fill
    (an index image through tv_rotate; indices up to 224 * 224 are exact in float32)."""
    assert S * S < 2 ** 24
    img = torch.arange(1, S * S + 1, dtype=torch.float32).reshape(1, S, S)
    return tv_rotate(img, angle, fill=0.0)[0].to(torch.int64) - 1


def index_map(S, angle):
    """The float32 statement of the rotation that the kernel implements, in numpy with every operation rounded
    to float32 on its own -> int64 [S, S] of sy * S + sx, -1 for fill."""
    f = np.float32
    m = np.array(inverse_matrix(angle), dtype=np.float64).astype(np.float32)
    t00, t01, t10, t11 = (m[[0, 1, 3, 4]] / f(0.5 * S)).astype(np.float32)
    half = f(0.5) * f(S)
    c = (np.arange(S, dtype=np.float32) - half + f(0.5)).astype(np.float32)
    xb, yb = c[None, :], c[:, None]
    gx = ((xb * t00).astype(np.float32) + (yb * t01).astype(np.float32)).astype(np.float32)
    gy = ((xb * t10).astype(np.float32) + (yb * t11).astype(np.float32)).astype(np.float32)
    un = lambda g: ((((g + f(1.0)).astype(np.float32) * f(S)).astype(np.float32) - f(1.0)).astype(np.float32) / f(2.0)).astype(np.float32)
    sx, sy = np.rint(un(gx)), np.rint(un(gy))                                   # half to even
    inside = (sx >= 0) & (sx < S) & (sy >= 0) & (sy < S)
    idx = np.where(inside, sy.astype(np.int64) * S + sx.astype(np.int64), -1)
    return np.ascontiguousarray(np.broadcast_to(idx, (S, S)).astype(np.int64))


def ambiguous(S, angle):
    """bool [S, S]: the pixels whose source coordinate, computed from the double matrix in float64, lies within 2^-12 of a
    half-integer in x or y - where float32's coordinate error (a few ulp of 224, about 5e-5) may pick the other neighbour."""
    m = inverse_matrix(angle)
    c = np.arange(S, dtype=np.float64) - 0.5 * S + 0.5
    xb, yb = c[None, :], c[:, None]
    out = np.zeros((S, S), bool)
    for a, b in ((m[0], m[1]), (m[3], m[4])):
        g = xb * (a / (0.5 * S)) + yb * (b / (0.5 * S))
        i = ((g + 1.0) * S - 1.0) / 2.0
        out |= np.abs(i - np.floor(i) - 0.5) < 2.0 ** -12
    return out


# ------------------------------------------------------------------------------------------------ the pipeline
def gather(x, idx, fill=0.0):
    """x [C, S, S], idx int64 [S, S] (-1 for fill) -> x at the indexed pixels"""
    idx = torch.as_tensor(idx)
    flat = x.reshape(x.shape[0], -1)
    out = flat[:, idx.clamp(min=0).reshape(-1)].reshape(x.shape)
    return torch.where((idx < 0)[None], torch.full_like(out, fill), out)


def flips(idx_or_img, flip_h, flip_v):
    if flip_h:
        idx_or_img = idx_or_img.flip(-1)
    if flip_v:
        idx_or_img = idx_or_img.flip(-2)
    return idx_or_img


def apply(img_u8, d, S, mean=CLIP_MEAN, std=CLIP_STD, antialias=True, dtype=torch.float32):
    """img_u8 uint8 [H, W, 3], d one draw -> [3, S, S] in `dtype`.  The rotation's nearest sampling is an index map, so it is
    taken once from `tv_rotate` (float32, as the reference runs it) and applied as a gather in `dtype`.  mean / std are taken
    as the float32 numbers the transform is given (also in float64, so both runs start from the same inputs)."""
    x = torch.as_tensor(img_u8).permute(2, 0, 1).to(dtype) / 255                                  # ToTensor
    top, left, h, w = d["box"]
    x = F.interpolate(x[None, :, top:top + h, left:left + w], size=(S, S), mode="bilinear", align_corners=False,
                      antialias=antialias)[0]                                                    # RandomResizedCrop
    x = flips(x, d["flip_h"], d["flip_v"])
    x = gather(x, tv_index(S, d["angle"]))                                                       # RandomRotation
    m = torch.tensor(mean, dtype=torch.float32).to(dtype)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32).to(dtype)[:, None, None]
    return (x - m) / s


def source(H, W, seed):
    """A seeded source: random bytes with a black patch and a saturated patch"""
    rgb = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[:2, :3] = 0
    rgb[-2:, -3:] = 255
    return torch.from_numpy(rgb)
