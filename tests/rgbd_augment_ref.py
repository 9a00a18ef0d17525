"""Sequential restatement, in torch on the CPU, of the depth recipe's training transform (reference
open_clip/modal_depth/processors/vt_processor.py:94-207): ToTensor, DepthNorm, RandomResizedCrop(bilinear), RandomHorizontalFlip,
RandAugment3d (the identity on four channels), ColorJitter3d, RandomErasing, Normalize - one stage after the other on the whole
tensor, as the reference's Compose runs them, in float32 or float64, for given scalars; and the draw of those scalars in the
order of that pipeline.  The resampler is torch.nn.functional.interpolate itself; the torchvision stages are restated from its
published source (functional_tensor: _blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb; transforms: get_params of
RandomResizedCrop, ColorJitter, RandomErasing).  Shared by tests/test_rgbd_augment_host.py, tests/test_hip_rgbd_augment.py
and tools/preproc_bench.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
DEPTH_CLAMP = (0.01, 75.0, 75.0)            # DepthNorm(max_depth=75, clamp_max_before_scale=True): min, max, divisor


# ------------------------------------------------------------------------------------------------ the draws
def crop_box(H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params -> (top, left, h, w)"""
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,)).item()
            j = torch.randint(0, W - w + 1, size=(1,)).item()
            return i, j, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def erase_box(S, scale=(0.02, 0.33), ratio=(0.3, 3.3)):
    """RandomErasing.get_params on an S x S image -> (i, j, h, w), or None after ten failed attempts (the reference then
    overwrites the image with itself)."""
    area = S * S
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        h = int(round(math.sqrt(erase_area * aspect)))
        w = int(round(math.sqrt(erase_area / aspect)))
        if not (h < S and w < S):
            continue
        i = torch.randint(0, S - h + 1, size=(1,)).item()
        j = torch.randint(0, S - w + 1, size=(1,)).item()
        return i, j, h, w
    return None


def draw(H, W, S, num_ops=2, jitter=(0.4, 0.4, 0.4, 0.4), erase_p=0.25):
    """One sample's scalars from torch's global generator, stage by stage in the order of the reference's Compose."""
    d = {"box": crop_box(H, W)}                                                   # RandomResizedCrop
    d["flip"] = bool(torch.rand(1) < 0.5)                                         # RandomHorizontalFlip
    for _ in range(num_ops):                                                      # RandAugment3d: ops selected, none applied
        int(torch.randint(14, (1,)).item())
    d["order"] = tuple(torch.randperm(4).tolist())                                # ColorJitter.get_params
    for name, v, center in zip(("brightness", "contrast", "saturation", "hue"), jitter, (1.0, 1.0, 1.0, 0.0)):
        if v is None or v == 0:
            d[name] = None
        else:
            lo = center - v if name == "hue" else max(center - v, 0.0)
            d[name] = float(torch.empty(1).uniform_(lo, center + v))
    d["erase"] = erase_box(S) if torch.rand(1) < erase_p else None                # RandomErasing
    return d


# ------------------------------------------------------------------------------------------------ the stages
def _blend(a, b, r):
    return (r * a + (1.0 - r) * b).clamp(0, 1)


def _grey(x):
    r, g, b = x.unbind(-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def _rgb2hsv(img):
    r, g, b = img.unbind(-3)
    maxc, minc = torch.max(img, dim=-3).values, torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(-3)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = torch.clamp(v * (1.0 - s), 0.0, 1.0)
    q = torch.clamp(v * (1.0 - s * f), 0.0, 1.0)
    t = torch.clamp(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    pick = lambda six: torch.stack(six, dim=0).gather(0, i.unsqueeze(0))[0]
    return torch.stack((pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))), dim=-3)


def color_jitter(x, d):
    """ColorJitter.forward on [3, H, W] with the drawn order and factors; a factor of None leaves its term out."""
    for k in d["order"]:
        if k == 0 and d["brightness"] is not None:
            x = _blend(x, torch.zeros_like(x), d["brightness"])
        elif k == 1 and d["contrast"] is not None:
            x = _blend(x, torch.mean(_grey(x), dim=(-3, -2, -1), keepdim=True), d["contrast"])
        elif k == 2 and d["saturation"] is not None:
            x = _blend(x, _grey(x), d["saturation"])
        elif k == 3 and d["hue"] is not None:
            hsv = _rgb2hsv(x)
            h, s, v = hsv.unbind(-3)
            x = _hsv2rgb(torch.stack(((h + d["hue"]) % 1.0, s, v), dim=-3))
    return x


def depth_norm(x, clamp=DEPTH_CLAMP):
    lo, hi, div = clamp
    return torch.cat([x[:3], x[3:4].clamp(min=lo).clamp(max=hi) / div], dim=0)


def resized_crop(x, box, S, antialias):
    top, left, h, w = box
    return F.interpolate(x[None, :, top:top + h, left:left + w], size=(S, S), mode="bilinear", align_corners=False,
                         antialias=antialias)[0]


def apply(rgb_u8, depth, d, S, mean=CLIP_MEAN + (0.0418,), std=CLIP_STD + (0.0295,), antialias=True, dtype=torch.float32,
          clamp=DEPTH_CLAMP):
    """rgb_u8 uint8 [H, W, 3], depth float32 [H, W], d one draw -> (img [3, S, S], depth [1, S, S]) in `dtype`.  mean / std are
    taken as the float32 numbers the transform is given (also in float64, so both runs start from the same inputs)."""
    rgb_u8, depth = torch.as_tensor(rgb_u8), torch.as_tensor(depth)
    x = torch.cat([rgb_u8.permute(2, 0, 1).to(dtype) / 255, depth[None].to(dtype)], dim=0)        # ToTensor, cat
    x = depth_norm(x, clamp)
    x = resized_crop(x, d["box"], S, antialias)
    if d["flip"]:
        x = x.flip(-1)
    x = torch.cat([color_jitter(x[:3], d), x[3:4]], dim=0)                                        # ColorJitter3d
    if d["erase"] is not None:
        i, j, h, w = d["erase"]
        x = x.clone()
        x[:, i:i + h, j:j + w] = 0
    m = torch.tensor(mean, dtype=torch.float32).to(dtype)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32).to(dtype)[:, None, None]
    x = (x - m) / s
    return x[:3], x[3:4]


# ------------------------------------------------------------------------------------------------ inputs
def sample(H, W, seed):
    """A seeded source: random bytes with a grey strip (R = G = B), a black patch and a saturated patch, and a disparity map
    whose values run from below DepthNorm's minimum to above its maximum."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[H // 3:H // 3 + 2] = rgb[H // 3:H // 3 + 2, :, :1]
    rgb[:2, :3] = 0
    rgb[-2:, -3:] = 255
    depth = rng.uniform(-5.0, 90.0, (H, W)).astype(np.float32)
    depth[0, 0], depth[-1, -1] = 0.001, 200.0
    return torch.from_numpy(rgb), torch.from_numpy(depth)


CAPTIONS = ["A  Photo: of (a) Dog!!\n", "  two#words;here~ \n\n", 'He said "hi". ' + "w " * 80, "", "UPPER\tTab\n and  newline"]


def rgbd_input():
    """[4, 9, 7]: RGB in [0, 1], depth from below DepthNorm's minimum (0.01) to above its maximum (75)"""
    g = torch.Generator().manual_seed(1)
    x = torch.rand(4, 9, 7, generator=g)
    x[3] = torch.linspace(-3.0, 120.0, 63).reshape(9, 7)
    x[3, 0, 1], x[3, 0, 2] = 0.005, 75.5
    return x
