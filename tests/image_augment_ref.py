"""Sequential restatement, in numpy on the CPU, of the plain-image training transform (reference
open_clip/modal_eeg/processors/eeg_processor.py:93-139 `Image_Processor_Train`): RandomResizedCrop(224, bilinear) and
RandomHorizontalFlip on the 8-bit image, the fourteen RandAugment ops as the Pillow calls they end in, then ToTensor,
ColorJitter and Normalize on the float tensor.  Every 8-bit stage is written out from Pillow's behaviour and pinned to Pillow
at byte equality by tests/test_image_augment_host.py; `pillow_*` are the same stages made of the Pillow calls themselves (the
oracle where Pillow imports).  The float tail is the colour chain of tests/rgbd_augment_ref.py.  Shared by
tests/test_image_augment_host.py, tests/test_hip_image_augment.py and tools/preproc_bench.py."""
import math

import numpy as np
import torch

import rgbd_augment_ref as R

CLIP_MEAN, CLIP_STD = R.CLIP_MEAN, R.CLIP_STD
OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize")
SIGNED = (False, True, True, True, True, True, True, True, True, True, False, False, False, False)
GEOMETRIC, ENHANCE = (1, 2, 3, 4, 5), (6, 7, 8, 9)
PRECISION_BITS = 22


# ------------------------------------------------------------------------------------------------ the magnitudes and matrices
# kept bits per bin, as data: the row of the table recorded from the reference (tests/golden/reference/
# test_image_augment_host.randaugment_space), which tests/test_image_augment_host.py compares both this and the library with
POSTERIZE_BITS_31 = [8.0] * 4 + [7.0] * 8 + [6.0] * 7 + [5.0] * 8 + [4.0] * 4


def magnitude_table(num_bins, S):
    """name -> 31 magnitudes (float32 values as Python floats), the table of RandAugment for an S x S image"""
    assert num_bins == 31, "the Posterize row is stated as data for 31 bins"
    lin = lambda hi: [float(v) for v in torch.linspace(0.0, hi, num_bins)]
    return {"Identity": [0.0] * num_bins, "ShearX": lin(0.3), "ShearY": lin(0.3), "TranslateX": lin(150.0 / 331.0 * S),
            "TranslateY": lin(150.0 / 331.0 * S), "Rotate": lin(30.0), "Brightness": lin(0.9), "Color": lin(0.9),
            "Contrast": lin(0.9), "Sharpness": lin(0.9),
            "Posterize": POSTERIZE_BITS_31,
            "Solarize": [float(v) for v in torch.linspace(256.0, 0.0, num_bins)], "AutoContrast": [0.0] * num_bins,
            "Equalize": [0.0] * num_bins}


def inverse_affine(center, angle, translate, shear):
    """The output-to-input matrix (a, b, c, d, e, f) of a rotation by `angle`, a shear by (sx, sy) (all in degrees) about
    `center` and a translation, in doubles: M = T C R Sh C^-1 inverted in closed form."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle, w, h):
    """Image.rotate's matrix about the centre; None where it returns a copy (angle a multiple of 360)"""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def op_matrix(op, mag, size, shear_atan=False):
    """The six doubles of a geometric op at the signed magnitude `mag` on an image of `size` = (W, H) (None: a copy)"""
    W, H = size
    centre = [W * 0.5, H * 0.5]
    if op in (1, 2):
        deg = math.degrees(math.atan(mag)) if shear_atan else math.degrees(mag)
        return inverse_affine([0, 0] if shear_atan else centre, 0.0, [0, 0], [deg, 0.0] if op == 1 else [0.0, deg])
    if op in (3, 4):
        return inverse_affine(centre, 0.0, [int(mag), 0] if op == 3 else [0, int(mag)], [0.0, 0.0])
    assert op == 5
    return rotate_matrix(mag, W, H)


# ------------------------------------------------------------------------------------------------ the 8-bit ops
def to_l(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(deg, img, f) on 8-bit data: deg + f (img - deg) in float32, clipped to [0, 255], truncated"""
    f = np.float32(f)
    t = deg.astype(np.float32) + f * (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 in float32 from 0.5, the row below first; the border is copied"""
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    one, five = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    x = img.astype(np.float32)
    ss = np.full((H - 2, W - 2, 3), np.float32(0.5))
    for rows, kc in ((slice(2, H), one), (slice(1, H - 1), five), (slice(0, H - 2), one)):
        r = x[rows]
        ss = ss + ((r[:, 0:W - 2] * one + r[:, 1:W - 1] * kc) + r[:, 2:W] * one)
    out[1:H - 1, 1:W - 1] = np.clip(ss, np.float32(0), np.float32(255)).astype(np.uint8)
    return out


def affine(img, m):
    """Image.transform(size, AFFINE, m, BILINEAR): the source position of the centre of each output pixel in doubles, nothing
    contracted; outside the image 0; the four neighbours clamped into the image, blended in doubles, truncated"""
    H, W = img.shape[:2]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = (m[0] * xs + m[1] * ys) + m[2]
    yin = (m[3] * xs + m[4] * ys) + m[5]
    inside = ~((xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    x0, x1 = np.clip(x, 0, W - 1), np.clip(x + 1, 0, W - 1)
    y0 = np.clip(y, 0, H - 1)
    y1 = np.clip(y + 1, 0, H - 1)
    src = img.astype(np.float64)
    lerp = lambda a, b, d: a + (b - a) * d
    v1 = lerp(src[y0, x0], src[y0, x1], dx)
    v2 = np.where(((y + 1 >= 0) & (y + 1 < H))[..., None], lerp(src[y1, x0], src[y1, x1], dx), v1)
    out = lerp(v1, v2, dy)
    return np.where(inside[..., None], out, 0.0).astype(np.uint8)


def histograms(img):
    return [np.bincount(img[..., c].reshape(-1), minlength=256) for c in range(3)]


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def equalize_lut(h):
    nz = h[h != 0]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (int(nz.sum()) - int(nz[-1])) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    before = np.concatenate([[0], np.cumsum(h)[:-1]]).astype(np.int64)
    return np.clip((step // 2 + before) // step, 0, 255).astype(np.uint8)


def apply_luts(img, luts):
    return np.stack([luts[c][img[..., c]] for c in range(3)], axis=-1)


def contrast_mean(img):
    """ImageStat's mean of the L image, rounded as ImageEnhance.Contrast rounds it"""
    l = to_l(img)
    return int(float(l.astype(np.int64).sum()) / l.size + 0.5)


def solarize_threshold(mag):
    """i < mag for an integer i and a float mag is i < ceil(mag)"""
    return int(math.ceil(mag))


def apply_op(img, op, mag, shear_atan=False):
    """One RandAugment op at the signed magnitude `mag` (a Python float) on uint8 [S, S, 3] -> uint8 [S, S, 3]"""
    if op == 0:
        return img.copy()
    if op in GEOMETRIC:
        m = op_matrix(op, mag, (img.shape[1], img.shape[0]), shear_atan)
        return img.copy() if m is None else affine(img, m)
    if op in ENHANCE:
        f = 1.0 + mag
        if op == 6:
            deg = np.zeros_like(img)
        elif op == 7:
            deg = np.repeat(to_l(img)[..., None], 3, axis=-1)
        elif op == 8:
            deg = np.full_like(img, contrast_mean(img))
        else:
            deg = smooth(img)
        return blend(deg, img, f)
    if op == 10:
        mask = ~(2 ** (8 - int(mag)) - 1) & 0xFF
        return img & np.uint8(mask)
    if op == 11:
        i = np.arange(256)
        lut = np.where(i < solarize_threshold(mag), i, 255 - i).astype(np.uint8)
        return apply_luts(img, [lut] * 3)
    h = histograms(img)
    return apply_luts(img, [autocontrast_lut(hc) if op == 12 else equalize_lut(hc) for hc in h])


def pillow_op(img, op, mag, shear_atan=False):
    """The same op as the Pillow call torchvision makes of it"""
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(img)
    if op == 0:
        out = im
    elif op in (1, 2, 3, 4):
        out = im.transform(im.size, Image.AFFINE, op_matrix(op, mag, im.size, shear_atan), Image.BILINEAR)
    elif op == 5:
        out = im.rotate(mag, Image.BILINEAR)
    elif op in ENHANCE:
        out = (ImageEnhance.Brightness, ImageEnhance.Color, ImageEnhance.Contrast, ImageEnhance.Sharpness)[op - 6](im).enhance(1.0 + mag)
    elif op == 10:
        out = ImageOps.posterize(im, int(mag))
    elif op == 11:
        out = ImageOps.solarize(im, mag)
    elif op == 12:
        out = ImageOps.autocontrast(im)
    else:
        out = ImageOps.equalize(im)
    return np.array(out)


# ------------------------------------------------------------------------------------------------ crop, resize, flip
def resize_pass(src, bounds, kk):
    """One pass of Pillow's 8-bit resampler along axis 0 of src [n, ...]: int32 taps from 1 << 21, shift, clip"""
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for o, (lo, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for j in range(n):
            acc = acc + int(kk[o, j]) * src[lo + j].astype(np.int64)
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def crop_resize(img, box, S, tables):
    """img.crop(box).resize((S, S), BILINEAR) with `tables(in, out) -> (bounds, kk, ksize)`: horizontal pass, 8-bit
    intermediate, vertical pass"""
    top, left, bh, bw = box
    c = img[top:top + bh, left:left + bw]
    hb, hk, _ = tables(bw, S)
    vb, vk, _ = tables(bh, S)
    t = resize_pass(np.ascontiguousarray(c.transpose(1, 0, 2)), hb, hk).transpose(1, 0, 2)
    return resize_pass(np.ascontiguousarray(t), vb, vk)


def pillow_crop_resize(img, box, S):
    from PIL import Image
    top, left, bh, bw = box
    return np.array(Image.fromarray(img).crop((left, top, left + bw, top + bh)).resize((S, S), Image.BILINEAR))


def op_magnitude(table, op, negative, mag_bin):
    m = table[OPS[op]][mag_bin]
    return -m if (SIGNED[op] and negative) else m


def eight_bit(img, d, S, tables=None, shear_atan=False, solarize_from=256.0, num_bins=31):
    """The 8-bit stages for one draw `d` (box, flip, ops = [(index, negative, bin)]) -> uint8 [S, S, 3]; Pillow's calls where
    `tables` is None, the restatement otherwise"""
    x = pillow_crop_resize(img, d["box"], S) if tables is None else crop_resize(img, d["box"], S, tables)
    if d["flip"]:
        x = np.ascontiguousarray(x[:, ::-1])
    table = magnitude_table(num_bins, S)
    table["Solarize"] = [float(v) for v in torch.linspace(solarize_from, 0.0, num_bins)]
    for op, negative, mag_bin in d["ops"]:
        mag = op_magnitude(table, op, negative, mag_bin)
        x = pillow_op(x, op, mag, shear_atan) if tables is None else apply_op(x, op, mag, shear_atan)
    return x


# ------------------------------------------------------------------------------------------------ the float tail
def float_tail(u8, d, mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32):
    """ToTensor, ColorJitter in the drawn order, Normalize on uint8 [S, S, 3] -> [3, S, S] in `dtype`"""
    x = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).to(dtype) / 255
    x = R.color_jitter(x, d)
    m = torch.tensor(mean, dtype=torch.float32).to(dtype)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32).to(dtype)[:, None, None]
    return (x - m) / s


def draw(H, W, num_ops=2, mag_bin=9, jitter=(0.4, 0.4, 0.4, 0.4)):
    """One sample's scalars from torch's global generator in the order of the reference's Compose: the box, the flip, per op
    the index and (signed ops only) the sign, the permutation, brightness, contrast, saturation, hue"""
    d = {"box": R.crop_box(H, W), "flip": bool(torch.rand(1) < 0.5), "ops": []}
    for _ in range(num_ops):
        op = int(torch.randint(14, (1,)).item())
        negative = bool(torch.randint(2, (1,)).item()) if SIGNED[op] else False
        d["ops"].append((op, negative, mag_bin))
    d["order"] = tuple(torch.randperm(4).tolist())
    for name, v, center in zip(("brightness", "contrast", "saturation", "hue"), jitter, (1.0, 1.0, 1.0, 0.0)):
        if v is None or v == 0:
            d[name] = None
        else:
            lo = center - v if name == "hue" else max(center - v, 0.0)
            d[name] = float(torch.empty(1).uniform_(lo, center + v))
    return d


# ------------------------------------------------------------------------------------------------ inputs
def source(H, W, kind="random", seed=0):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full((H, W, 3), (37, 200, 5), np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if H >= 6 and W >= 6:                            # a smooth ramp (low gradients) and a grey strip beside the noise
        img[:H // 2, :W // 2] = (np.add.outer(np.arange(H // 2), np.arange(W // 2)) * 3 % 256)[..., None].astype(np.uint8)
        img[-2:] = img[-2:, :, :1]
    return img
