"""Tactile (GelSight RGB) preprocessing ON THE GPU (reference: open_clip/modal_tactile/processors/tact_processor.py:
281-300 `TactileRGBProcessorEval`): ToTensor -> Resize(256, bicubic) -> CenterCrop(224) -> Normalize.  Unlike the image
transform the resize runs on the FLOAT tensor (torchvision's tensor path = torch.nn.functional.interpolate, see
modal_depth/processors/vt_processor.py for the `antialias` default), so the three channels go through the float
resampler of csrc/vl_preproc.hip with ToTensor's /255 fused into the read.  Same class name and call convention as the
reference (a file path; a PIL image or an [H, W, 3] uint8 array is accepted too); result [3, 224, 224] float32 on the GPU.
`Image_Processor_Train` (reference :92-138) is the training transform of the paired image: its RandAugment runs on the 8-bit
image, one Pillow call per op, and is reproduced byte for byte by csrc/vl_image_augment.hip.  `Tactile_Processor_Train`
(reference :189-233) is the training transform of the tactile image itself, all of it on the float tensor
(csrc/vl_tactile_augment.hip), and `Tactile_Processor_Eval` (:236-278) the reference's other name for the evaluation transform."""
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


class TactileRGBProcessorEval(BaseProcessor):
    def __init__(self, img_mean=None, img_std=None, resize=256, size=224, antialias=True, device="cuda"):
        self.mean = img_mean if img_mean is not None else OPENAI_CLIP_MEAN
        self.std = img_std if img_std is not None else OPENAI_CLIP_STD
        self.resize, self.size, self.antialias, self.device = resize, size, antialias, torch.device(device)

    def __call__(self, img, out=None):
        from vitlens_hip import preproc
        if isinstance(img, (str, bytes)) or hasattr(img, "__fspath__"):
            from PIL import Image                                                 # decoding stays on the host, as in the reference
            img = Image.open(img)
        if hasattr(img, "convert"):
            img = np.array(img.convert("RGB"))
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
            raise ValueError(f"expected an [H, W, 3] uint8 image, got {tuple(img.shape)} {img.dtype}")
        return preproc.float_image_to_tensor(img.to(self.device), self.resize, self.size, self.mean, self.std,
                                             antialias=self.antialias, out=out)


tactile_transform_conf = {}


def _processor_config(cls, cfg, default_args):
    """The reference's from_config: `update_conf` is taken out of a copy of the mapping, `params` are the args."""
    cfg = dict(cfg or {})
    update_conf = cfg.pop("update_conf", None)
    return cls(args=cfg.get("params", default_args), img_mean=cfg.get("img_mean", OPENAI_CLIP_MEAN),
               img_std=cfg.get("img_std", OPENAI_CLIP_STD), update_conf=update_conf)


class Tactile_Processor_Eval(TactileRGBProcessorEval):
    """The reference's other name for the evaluation transform (:236-278): the arithmetic of `TactileRGBProcessorEval` behind
    the `(args, img_mean, img_std, update_conf)` signature of the reference's training-recipe classes.  The reference's
    `args` hold nothing this transform reads (`tactile_transform_conf` is empty)."""

    def __init__(self, args=None, img_mean=None, img_std=None, update_conf=None, device="cuda", *, resize=256, size=224,
                 antialias=True):
        super().__init__(img_mean=img_mean, img_std=img_std, resize=resize, size=size, antialias=antialias, device=device)
        self.conf = dict(args or {}, **(update_conf or {}))

    @classmethod
    def from_config(cls, cfg=None):
        return _processor_config(cls, cfg, tactile_transform_conf)


class Tactile_Processor_Train(BaseProcessor):
    """The tactile image of a training sample ON THE GPU (reference :189-233): ToTensor -> RandomResizedCrop(224, bilinear) ->
    RandomHorizontalFlip -> RandomVerticalFlip -> RandomRotation((0, 360), nearest, fill 0) -> Normalize, every stage on the
    float tensor (csrc/vl_tactile_augment.hip).

    proc(img) -> [3, size, size] f32 on the GPU for a path, a PIL image or an [H, W, 3] uint8 array; `batch` for a list.  Every
    random scalar is drawn on the host from torch's global CPU generator (`draw`), in the order of the reference's pipeline.
    `antialias`: F.interpolate's flag for the crop's resize (see modal_depth/processors/vt_processor.py for the default).
    The reference's `args` hold nothing this transform reads; they are kept as `conf`."""

    SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)                       # RandomResizedCrop's defaults

    def __init__(self, args=None, img_mean=None, img_std=None, update_conf=None, device="cuda", *, size=224, antialias=True,
                 degrees=(0.0, 360.0)):
        self.mean = list(img_mean if img_mean is not None else OPENAI_CLIP_MEAN)
        self.std = list(img_std if img_std is not None else OPENAI_CLIP_STD)
        self.conf = dict(args or {}, **(update_conf or {}))
        self.degrees = (float(degrees[0]), float(degrees[1]))
        if not self.degrees[0] <= self.degrees[1]:
            raise ValueError(f"degrees must be (min, max), got {degrees}")
        self.size, self.antialias, self.device = int(size), bool(antialias), torch.device(device)

    @classmethod
    def from_config(cls, cfg=None):
        return _processor_config(cls, cfg, tactile_transform_conf)

    def draw(self, H, W):
        """One sample's scalars for an H x W source, from torch's global CPU generator in the order of the reference's
        pipeline: the crop box (ten attempts, then the central fallback), the horizontal flip, the vertical flip, the angle."""
        from open_clip.transform import random_resized_crop_params
        return {"box": random_resized_crop_params(H, W, self.SCALE, self.RATIO), "flip_h": bool(torch.rand(1) < 0.5),
                "flip_v": bool(torch.rand(1) < 0.5), "angle": float(torch.empty(1).uniform_(self.degrees[0], self.degrees[1]))}

    def batch(self, images, draws=None):
        """images: a list of paths / PIL images / uint8 [H, W, 3] arrays or tensors, sizes free per sample -> [B, 3, size, size]
        f32 on the GPU.  The draws are made sample by sample in order (or given: `draws`, one `draw()` result per sample, so
        that a loader worker can draw ahead); host data goes up as one packed copy and the two kernels are launched once for
        the batch."""
        from vitlens_hip import preproc
        ims = [image_u8(im) for im in images]
        if draws is None:
            draws = [self.draw(im.shape[0], im.shape[1]) for im in ims]
        return preproc.plan_tactile_train(ims, draws, self.size, self.mean, self.std, antialias=self.antialias,
                                          device=self.device).launch()

    def __call__(self, img):
        return self.batch([img])[0]

    def __repr__(self):
        return ("(DataAugmentationForRGBD,\ntransform = [ToTensor(), RandomResizedCrop(size=%d, scale=%s, ratio=%s, "
                "interpolation=bilinear, antialias=%s), RandomHorizontalFlip(p=0.5), RandomVerticalFlip(p=0.5), "
                "RandomRotation(degrees=%s, interpolation=nearest, expand=False, fill=0), Normalize(mean=%s, std=%s)],\n)"
                % (self.size, self.SCALE, self.RATIO, self.antialias, list(self.degrees), self.mean, self.std))


image_transform_conf = {"num_ops": 2, "magnitude": 9}


class Image_Processor_Train(BaseProcessor):
    """The paired image of a tactile or EEG training sample ON THE GPU (reference: `Image_Processor_Train` of this module and
    of modal_eeg/processors/eeg_processor.py): RandomResizedCrop(224, bilinear) -> RandomHorizontalFlip -> RandAugment(num_ops,
    magnitude, bilinear) on the 8-bit image, each stage byte for byte the Pillow call it ends in, then ToTensor ->
    ColorJitter(0.4, 0.4, 0.4, 0.4) -> Normalize (csrc/vl_image_augment.hip).

    proc(img) -> [3, size, size] f32 on the GPU for a path, a PIL image or an [H, W, 3] uint8 array; `batch` for a list.  Every
    random scalar is drawn on the host from torch's global CPU generator (`draw`), in the order of the reference's pipeline.
    `args`: a mapping or an object with `num_ops` (0 .. 4) and `magnitude` (a bin of 31); `update_conf` overrides it.  Two
    points on which torchvision's versions differ are arguments, the reference's own copy of the op table
    (modal_depth/processors/transforms_rgbd.py) being the default: `shear_atan` (False: shear = degrees(m) about the centre;
    True: degrees(atan(m)) about (0, 0)) and `solarize_from` (256, or 255)."""

    SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)                       # RandomResizedCrop's defaults
    NUM_MAGNITUDE_BINS = 31

    def __init__(self, args=None, img_mean=None, img_std=None, update_conf=None, device="cuda", *, size=224,
                 color_jitter=(0.4, 0.4, 0.4, 0.4), shear_atan=False, solarize_from=256.0):
        from vitlens_hip import ops
        self.mean = list(img_mean if img_mean is not None else OPENAI_CLIP_MEAN)
        self.std = list(img_std if img_std is not None else OPENAI_CLIP_STD)
        conf = dict(image_transform_conf)
        if args is not None:
            conf.update(args if hasattr(args, "keys") else {k: getattr(args, k) for k in conf if hasattr(args, k)})
        if update_conf is not None:
            conf.update(update_conf)
        self.num_ops, self.magnitude = int(conf["num_ops"]), int(conf["magnitude"])
        if not 0 <= self.num_ops <= ops.IMAGE_MAX_OPS:
            raise ValueError(f"num_ops must be in [0, {ops.IMAGE_MAX_OPS}], got {self.num_ops}")
        if not 0 <= self.magnitude < self.NUM_MAGNITUDE_BINS:
            raise ValueError(f"magnitude must be a bin in [0, {self.NUM_MAGNITUDE_BINS}), got {self.magnitude}")
        b, c, s, h = color_jitter
        if h is not None and not 0 <= h <= 0.5:
            raise ValueError(f"the hue strength must be in [0, 0.5], got {h}")
        self.jitter = (jitter_range(b, 1.0, 0.0), jitter_range(c, 1.0, 0.0), jitter_range(s, 1.0, 0.0), jitter_range(h, 0.0))
        self.color_jitter, self.size, self.device = tuple(color_jitter), int(size), torch.device(device)
        self.shear_atan, self.solarize_from = bool(shear_atan), float(solarize_from)

    @classmethod
    def from_config(cls, cfg=None):
        return _processor_config(cls, cfg, image_transform_conf)

    def draw(self, H, W):
        """One sample's scalars for an H x W source, from torch's global CPU generator in the order of the reference's
        pipeline: the crop box (ten attempts, then the central fallback), the flip, per RandAugment op randint(14) and, for a
        signed op only, randint(2), then randperm(4), brightness, contrast, saturation, hue (enabled terms only)."""
        from open_clip.transform import random_resized_crop_params
        from vitlens_hip.preproc import RANDAUGMENT_SIGNED
        d = {"box": random_resized_crop_params(H, W, self.SCALE, self.RATIO), "flip": bool(torch.rand(1) < 0.5), "ops": []}
        for _ in range(self.num_ops):
            code = int(torch.randint(len(RANDAUGMENT_SIGNED), (1,)))
            negative = bool(torch.randint(2, (1,))) if RANDAUGMENT_SIGNED[code] else False
            d["ops"].append((code, negative, self.magnitude))
        d["order"] = tuple(torch.randperm(4).tolist())
        for name, rng in zip(("brightness", "contrast", "saturation", "hue"), self.jitter):
            d[name] = None if rng is None else float(torch.empty(1).uniform_(rng[0], rng[1]))
        return d

    def batch(self, images, draws=None, want_u8=False):
        """images: a list of paths / PIL images / uint8 [H, W, 3] arrays or tensors, sizes free per sample -> [B, 3, size, size]
        f32 on the GPU; with `want_u8` also the 8-bit image after RandAugment, uint8 [B, size, size, 3].  The draws are made
        sample by sample in order (or given: `draws`, one `draw()` result per sample, so that a loader worker can draw
        ahead); host data goes up as one packed copy and the kernels are launched once for the batch."""
        from vitlens_hip import preproc
        ims = [image_u8(im) for im in images]
        if draws is None:
            draws = [self.draw(im.shape[0], im.shape[1]) for im in ims]
        return preproc.plan_image_train(ims, draws, self.size, self.mean, self.std, num_bins=self.NUM_MAGNITUDE_BINS,
                                        shear_atan=self.shear_atan, solarize_from=self.solarize_from,
                                        device=self.device).launch(want_u8=want_u8)

    def __call__(self, img, want_u8=False):
        out = self.batch([img], want_u8=want_u8)
        return (out[0][0], out[1][0]) if want_u8 else out[0]

    def __repr__(self):
        b, c, s, h = self.color_jitter
        return ("(DataAugmentationForRGBD,\ntransform = [RandomResizedCrop(size=%d, scale=%s, ratio=%s, interpolation=bilinear), "
                "RandomHorizontalFlip(p=0.5), RandAugment(num_ops=%d, magnitude=%d, num_magnitude_bins=%d, interpolation=bilinear), "
                "ToTensor(), ColorJitter(brightness=%s, contrast=%s, saturation=%s, hue=%s), Normalize(mean=%s, std=%s)],\n)"
                % (self.size, self.SCALE, self.RATIO, self.num_ops, self.magnitude, self.NUM_MAGNITUDE_BINS, b, c, s, h,
                   self.mean, self.std))
