"""Depth (disparity) preprocessing ON THE GPU (reference: open_clip/modal_depth/processors/
vt_processor.py:292-337 `DepthProcessorEval`, transforms_rgbd.py:366-411 `DepthNorm`).

The reference concatenates a throw-away random RGB image with the disparity map and sends the 4-channel tensor through
DepthNorm (clamp to [min_depth, max_depth], divide by max_depth) -> Resize(224, bicubic) -> CenterCrop(224) ->
Normalize, then keeps channel 3.  Only that channel is computed here: the clamp and the division are applied as the
source is read by the horizontal resampling pass, the vertical pass finishes with (x - depth_mean) / depth_std
(csrc/vl_preproc.hip, tables from vitlens_hip/preproc.py), and only the 224 x 224 crop window is produced.

torchvision's Resize of a TENSOR is torch.nn.functional.interpolate(mode="bicubic", align_corners=False,
antialias=...), whose default changed between torchvision releases (the reference does not pin one): `antialias=True`
(torchvision >= 0.17) is the default here, `antialias=False` reproduces the older behaviour.

Same class name, constructor arguments and call convention as the reference; the result is a [1, 224, 224] float32
tensor on the GPU, which is what the depth tokenizer takes.

`RGBD_Processor_Train` (reference :94-207) is the training transform of an RGB-D pair, one `vl_rgbd_augment` call per batch
(csrc/vl_rgbd_augment.hip): ToTensor, DepthNorm, RandomResizedCrop(224, bilinear), RandomHorizontalFlip,
RandAugment3d, ColorJitter3d(0.4, 0.4, 0.4, 0.4), RandomErasing(p=0.25), Normalize.  The random scalars are drawn on the
host from torch's global CPU generator in the order in which the reference's pipeline draws them, so a `torch.manual_seed`
selects the same crop, flip, jitter and erase.  RandAugment3d is the identity on a four-channel tensor (it tests the channel
count of the WHOLE input against 3 and 1 and so never applies an op): it is two discarded `randint(14)` draws here.
torchvision is not installed where this was written: RandomResizedCrop, RandomHorizontalFlip, ColorJitter and RandomErasing
are restated from its published source, and parity with torchvision itself is NOT pinned by a test.  What is pinned: the
bilinear resampler against ATen (`F.interpolate`), DepthNorm and RandAugment3d against the reference's own classes.
`RGBD_Processor_Eval` (reference :210-289) is the evaluation counterpart on the existing float resamplers, and
`BlipCaptionProcessor` the reference's caption cleaning."""
import math
import re

import numpy as np
import torch

from open_clip.transform import image_u8, jitter_range

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class BaseProcessor:
    def __init__(self):
        self.transform = lambda x: x

    def __call__(self, item):
        return self.transform(item)

    @classmethod
    def from_config(cls, cfg=None):
        return cls()

    def build(self, **kwargs):
        return self.from_config(dict(kwargs))


class DepthProcessorEval(BaseProcessor):
    def __init__(self, img_mean=None, img_std=None, depth_mean=0.0418, depth_std=0.0295, max_depth=75,
                 clamp_max_before_scale=True, min_depth=0.01, size=224, antialias=True, device="cuda"):
        img_mean = img_mean if img_mean is not None else OPENAI_CLIP_MEAN
        img_std = img_std if img_std is not None else OPENAI_CLIP_STD
        depth_mean = depth_mean if depth_mean is not None else 0.0
        depth_std = depth_std if depth_std is not None else 1.0
        if max_depth < 0.0:
            raise ValueError("max_depth must be > 0; got %.2f" % max_depth)
        self.mean = list(img_mean) + [depth_mean]
        self.std = list(img_std) + [depth_std]
        self.max_depth, self.min_depth, self.clamp_max_before_scale = float(max_depth), float(min_depth), clamp_max_before_scale
        self.size, self.antialias, self.device = size, antialias, torch.device(device)

    def __call__(self, depth, out=None):
        """depth: [H, W] or [1, H, W] disparity (tensor or numpy) -> [1, size, size] float32 on the GPU."""
        from vitlens_hip import preproc
        if isinstance(depth, np.ndarray):
            depth = torch.from_numpy(np.ascontiguousarray(depth))
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        if depth.dim() != 2:
            raise ValueError(f"expected an [H, W] or [1, H, W] disparity map, got {tuple(depth.shape)}")
        d = depth.to(device=self.device, dtype=torch.float32, non_blocking=True)
        hi = self.max_depth if self.clamp_max_before_scale else float("inf")
        return preproc.depth_to_tensor(d, self.size, self.mean[3], self.std[3], clamp=(self.min_depth, hi, self.max_depth),
                                       antialias=self.antialias, out=out)

    def batch(self, depths):
        out = torch.empty(len(depths), 1, self.size, self.size, device=self.device, dtype=torch.float32)
        for i, d in enumerate(depths):
            self(d, out=out[i])
        return out

    @classmethod
    def from_config(cls, cfg=None):
        cfg = cfg or {}
        return cls(img_mean=cfg.get("img_mean", None), img_std=cfg.get("img_std", None), depth_mean=cfg.get("depth_mean", 0.0418),
                   depth_std=cfg.get("depth_std", 0.0295), max_depth=cfg.get("max_depth", 75),
                   clamp_max_before_scale=cfg.get("clamp_max_before_scale", True))


class _Conf(dict):
    """A plain attribute dictionary, where the reference uses an OmegaConf node."""
    __setattr__ = dict.__setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


rgbd_conf = _Conf(max_depth=75, clamp_max_before_scale=True, num_ops=2, magnitude=9)


def _conf(args, update_conf):
    """The reference's `rgbd_conf` values, overridden by `args` (a mapping or an object with those attributes), then by
    `update_conf`; the caller's objects are left as they are."""
    conf = _Conf(rgbd_conf)
    if args is not None:
        conf.update(args if hasattr(args, "keys") else {k: getattr(args, k) for k in rgbd_conf if hasattr(args, k)})
    if update_conf is not None:
        conf.update(update_conf)
    if conf.max_depth < 0.0:
        raise ValueError("max_depth must be > 0; got %.2f" % conf.max_depth)
    return conf


class BlipCaptionProcessor(BaseProcessor):
    """Lower-case, the characters . ! " ( ) * # : ; ~ to blanks, runs of white space to one blank, trailing newlines and outer
    blanks off, at most `max_words` words, the prompt in front (reference :49-91)."""

    def __init__(self, prompt="", max_words=50):
        self.prompt, self.max_words = prompt, max_words

    def __call__(self, caption):
        if caption is None:
            return None
        return self.prompt + self.pre_caption(caption)

    @classmethod
    def from_config(cls, cfg=None):
        cfg = cfg or {}
        return cls(prompt=cfg.get("prompt", ""), max_words=cfg.get("max_words", 70))

    def pre_caption(self, caption):
        caption = re.sub(r"([.!\"()*#:;~])", " ", caption.lower())
        caption = re.sub(r"\s{2,}", " ", caption).rstrip("\n").strip(" ")
        words = caption.split(" ")
        return " ".join(words[:self.max_words]) if len(words) > self.max_words else caption


def _depth_f32(depth):
    """A path (torch.load), a tensor or an array, [H, W] or [1, H, W] -> float32 [H, W] tensor."""
    if isinstance(depth, str) or hasattr(depth, "__fspath__"):
        depth = torch.load(depth)
    if isinstance(depth, np.ndarray):
        depth = torch.from_numpy(np.ascontiguousarray(depth))
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2:
        raise ValueError(f"expected an [H, W] or [1, H, W] disparity map, got {tuple(depth.shape)}")
    return depth.to(torch.float32)


class _RGBDProcessor(BaseProcessor):
    """What the training and the evaluation processor share: statistics, DepthNorm's constants, from_config."""

    def __init__(self, args=None, img_mean=None, img_std=None, depth_mean=None, depth_std=None, update_conf=None, *, size=224,
                 antialias=True, device="cuda"):
        img_mean = img_mean if img_mean is not None else OPENAI_CLIP_MEAN
        img_std = img_std if img_std is not None else OPENAI_CLIP_STD
        self.mean = list(img_mean) + [depth_mean if depth_mean is not None else 0.0]
        self.std = list(img_std) + [depth_std if depth_std is not None else 1.0]
        self.conf = _conf(args, update_conf)
        self.min_depth = 0.01
        self.size, self.antialias, self.device = int(size), bool(antialias), torch.device(device)

    @property
    def depth_clamp(self):
        """(lo, hi, divide_by) of DepthNorm(max_depth, clamp_max_before_scale, min_depth=0.01)"""
        hi = float(self.conf.max_depth) if self.conf.clamp_max_before_scale else float("inf")
        return self.min_depth, hi, float(self.conf.max_depth)

    @classmethod
    def from_config(cls, cfg=None):
        cfg = dict(cfg or {})
        update_conf = cfg.pop("update_conf", None)
        return cls(args=cfg.get("params", None), img_mean=cfg.get("img_mean", OPENAI_CLIP_MEAN),
                   img_std=cfg.get("img_std", OPENAI_CLIP_STD), depth_mean=cfg.get("depth_mean", 0.0418),
                   depth_std=cfg.get("depth_std", 0.0295), update_conf=update_conf)


class RGBD_Processor_Train(_RGBDProcessor):
    """proc(img, depth) -> (img [3, size, size], depth [1, size, size]) f32 on the GPU; `process_batch` for a batch.  See the
    module docstring.  `color_jitter` = (brightness, contrast, saturation, hue) strengths and `erase_p` are the reference's
    constants (0.4 each, 0.25); a strength of None or 0 switches its term off, and the term then draws nothing."""

    SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)                       # RandomResizedCrop's defaults
    ERASE_SCALE, ERASE_RATIO = (0.02, 0.33), (0.3, 3.3)                      # RandomErasing's defaults
    RANDAUGMENT_OPS = 14                                                     # size of RandAugment3d's op table

    def __init__(self, args=None, img_mean=None, img_std=None, depth_mean=None, depth_std=None, update_conf=None, *, size=224,
                 antialias=True, device="cuda", color_jitter=(0.4, 0.4, 0.4, 0.4), erase_p=0.25):
        super().__init__(args, img_mean, img_std, depth_mean, depth_std, update_conf, size=size, antialias=antialias, device=device)
        b, c, s, h = color_jitter
        if h is not None and not 0 <= h <= 0.5:
            raise ValueError(f"the hue strength must be in [0, 0.5], got {h}")
        self.jitter = (jitter_range(b, 1.0, 0.0), jitter_range(c, 1.0, 0.0), jitter_range(s, 1.0, 0.0), jitter_range(h, 0.0))
        self.color_jitter, self.erase_p = tuple(color_jitter), float(erase_p)

    def draw(self, H, W):
        """One sample's scalars for an H x W source, from torch's global CPU generator in the order of the reference's
        pipeline: the crop box (ten attempts, then the central fallback), the flip, `num_ops` discarded randint(14)
        (RandAugment3d selects ops and applies none), randperm(4), brightness, contrast, saturation, hue (enabled terms
        only), the erase gate and, behind an open gate, up to ten attempts at a rectangle."""
        from open_clip.transform import random_resized_crop_params
        S = self.size
        d = {"box": random_resized_crop_params(H, W, self.SCALE, self.RATIO), "flip": bool(torch.rand(1) < 0.5)}
        for _ in range(int(self.conf.num_ops)):
            torch.randint(self.RANDAUGMENT_OPS, (1,))
        d["order"] = tuple(torch.randperm(4).tolist())
        for name, rng in zip(("brightness", "contrast", "saturation", "hue"), self.jitter):
            d[name] = None if rng is None else float(torch.empty(1).uniform_(rng[0], rng[1]))
        d["erase"] = None
        if torch.rand(1) < self.erase_p:
            area = S * S
            log_ratio = torch.log(torch.tensor(self.ERASE_RATIO))
            for _ in range(10):
                erase_area = area * torch.empty(1).uniform_(self.ERASE_SCALE[0], self.ERASE_SCALE[1]).item()
                aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
                h = int(round(math.sqrt(erase_area * aspect)))
                w = int(round(math.sqrt(erase_area / aspect)))
                if not (h < S and w < S):
                    continue
                i = torch.randint(0, S - h + 1, size=(1,)).item()
                j = torch.randint(0, S - w + 1, size=(1,)).item()
                d["erase"] = (i, j, h, w)
                break                              # ten failures: the reference fills the image with itself - no erase
        return d

    def process_batch(self, images, depths, draws=None):
        """images: a list of paths / PIL images / uint8 [H, W, 3] arrays or tensors, depths: a list of paths / [H, W] or
        [1, H, W] arrays or tensors, sizes free per sample -> ([B, 3, size, size], [B, 1, size, size]) f32 on the GPU.  The
        draws are made sample by sample in order (or given: `draws`, one `draw()` result per sample, to replay a batch);
        host data goes up as one packed copy and the kernels are launched once for the batch."""
        from vitlens_hip import preproc
        ims, dps = [image_u8(im) for im in images], [_depth_f32(d) for d in depths]
        if draws is None:
            draws = [self.draw(im.shape[0], im.shape[1]) for im in ims]
        return preproc.plan_rgbd(ims, dps, draws, self.size, self.mean, self.std, self.depth_clamp, antialias=self.antialias,
                                 device=self.device).launch()

    def __call__(self, img_path, depth_path):
        img, depth = self.process_batch([img_path], [depth_path])
        return img[0], depth[0]

    def __repr__(self):
        b, c, s, h = self.color_jitter
        return ("(DataAugmentationForRGBD,\ntransform = [DepthNorm(max_depth=%s, clamp_max_before_scale=%s), "
                "RandomResizedCrop(size=%d, scale=%s, ratio=%s, interpolation=bilinear, antialias=%s), RandomHorizontalFlip(p=0.5), "
                "RandAugment3d(num_ops=%s, magnitude=%s), ColorJitter3d(brightness=%s, contrast=%s, saturation=%s, hue=%s), "
                "RandomErasing(p=%s), Normalize(mean=%s, std=%s)],\n)"
                % (self.conf.max_depth, self.conf.clamp_max_before_scale, self.size, self.SCALE, self.RATIO, self.antialias,
                   self.conf.num_ops, self.conf.magnitude, b, c, s, h, self.erase_p, self.mean, self.std))


class RGBD_Processor_Eval(_RGBDProcessor):
    """proc(img, depth) -> (img [3, size, size], depth [1, size, size]) f32 on the GPU: DepthNorm -> Resize(size, bicubic) ->
    CenterCrop(size) -> Normalize on the FLOAT four-channel tensor (reference :210-289), that is ToTensor first and the float
    resampler for every channel (`preproc.float_image_to_tensor` for RGB, `preproc.depth_to_tensor` for depth)."""

    def __call__(self, img_path, depth_path):
        from vitlens_hip import preproc
        img = image_u8(img_path).to(self.device, non_blocking=True)
        depth = _depth_f32(depth_path).to(self.device, non_blocking=True)
        if tuple(depth.shape) != tuple(img.shape[:2]):
            raise ValueError(f"image {tuple(img.shape[:2])} and depth {tuple(depth.shape)} differ in size")
        return (preproc.float_image_to_tensor(img, self.size, self.size, self.mean[:3], self.std[:3], antialias=self.antialias),
                preproc.depth_to_tensor(depth, self.size, self.mean[3], self.std[3], clamp=self.depth_clamp, antialias=self.antialias))

    def __repr__(self):
        return ("(DataAugmentationForRGBD,\ntransform = [DepthNorm(max_depth=%s, clamp_max_before_scale=%s), Resize(size=%d, "
                "interpolation=bicubic, antialias=%s), CenterCrop(size=%d), Normalize(mean=%s, std=%s)],\n)"
                % (self.conf.max_depth, self.conf.clamp_max_before_scale, self.size, self.antialias, self.size, self.mean, self.std))
