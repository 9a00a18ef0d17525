"""Host side of the on-GPU image / depth preprocessing (kernels in csrc/vl_preproc.hip).

The resamplers are table driven: per output index of a resized axis a first tap, a tap count and the coefficients.
The tables depend only on (input size, output size), so they are built once on the host - exactly where Pillow and
ATen build theirs - cached, and kept on the device.

  * `pil_bicubic_tables`  = Pillow `Resample.c:precompute_coeffs` + `normalize_coeffs_8bpc` (double precision, Keys
    kernel a = -0.5, support scaled when shrinking, 22-bit fixed point rounded half away from zero); `pil_bilinear_tables`
    is the same with the triangle filter, for the crop boxes of the plain-image training transform (`plan_image_train`,
    csrc/vl_image_augment.hip);
  * `aten_bicubic_tables` = ATen `UpSampleKernel.cpp` weights: antialiased (`_compute_indices_min_size_weights_aa`,
    float32, a = -0.5, normalised) or plain (`get_cubic_upsample_coefficients`, a = -0.75, 4 taps from floor(src) - 1,
    border-clamped in the kernel);
  * `aten_bilinear_tables` = the bilinear weights of the same ATen file (antialiased triangle filter, or the two plain
    taps), for the crop boxes of the depth training transform (`plan_rgbd`, csrc/vl_rgbd_augment.hip).

`image_to_tensor` / `depth_to_tensor` run Resize(shorter edge) -> CenterCrop -> Normalize restricted to the crop
window (torchvision `_compute_resized_output_size`, `center_crop`); see open_clip/transform.py and
open_clip/modal_depth/processors/vt_processor.py for the reference-facing classes."""
import collections
import ctypes
import fractions
import functools
import math

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2


def resized_output_size(h, w, size):
    """Resize(int): shorter edge -> size, longer = int(size * long / short) (torchvision functional.resize)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def center_crop_origin(h, w, size):
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def _keys(x, a):
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _pil_tables(in_size, out_size, in0, in1, filt, filter_support):
    """Pillow `Resample.c:precompute_coeffs` + `normalize_coeffs_8bpc` for one filter: operation order as in Resample.c so
    that every double is the one Pillow computes (the row sum is a left-to-right running sum)."""
    in1 = float(in_size) if in1 is None else float(in1)
    scale = (in1 - in0) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = in0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)               # C cast: truncation (values >= -1.5 -> ok)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = filt(((j + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(j < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                             # sequential, as the C loop
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fx = w * float(1 << PRECISION_BITS)
    kk = np.where(w < 0, (-0.5 + fx).astype(np.int64), (0.5 + fx).astype(np.int64)).astype(np.int32)   # (int) truncates
    kk = np.where(j < xmax[:, None], kk, 0).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return bounds, kk, ksize


@functools.lru_cache(maxsize=256)
def pil_bicubic_tables(in_size, out_size, in0=0.0, in1=None):
    """-> (bounds [out,2] int32, kk [out,ksize] int32, ksize) of Image.resize(BICUBIC): Keys kernel a = -0.5, support 2."""
    return _pil_tables(in_size, out_size, in0, in1, lambda x: _keys(x, -0.5), 2.0)


@functools.lru_cache(maxsize=1024)
def pil_bilinear_tables(in_size, out_size, in0=0.0, in1=None):
    """-> (bounds [out,2] int32, kk [out,ksize] int32, ksize) of Image.resize(BILINEAR): the triangle filter max(0, 1 - |x|),
    support 1 (times the scale when shrinking), the same 22-bit fixed point as `pil_bicubic_tables`."""
    return _pil_tables(in_size, out_size, in0, in1, lambda x: np.maximum(1.0 - np.abs(x), 0.0), 1.0)


@functools.lru_cache(maxsize=256)
def aten_bicubic_tables(in_size, out_size, antialias=True):
    """-> (bounds [out,2] int32, weights [out,ksize] float32, ksize) in float32 arithmetic, as ATen for a float input."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    i = np.arange(out_size, dtype=np.float32)
    if antialias:
        support = f(2.0) * scale if scale >= 1.0 else f(2.0)
        invscale = f(1.0) / scale if scale >= 1.0 else f(1.0)
        ksize = int(math.ceil(float(support))) * 2 + 1
        center = scale * (i + f(0.5))
        xmin = np.maximum((center - support + f(0.5)).astype(np.int64), 0)
        xsize = np.minimum((center + support + f(0.5)).astype(np.int64), in_size) - xmin
        j = np.arange(ksize, dtype=np.int64)[None, :]
        arg = (((j + xmin[:, None]).astype(np.float32) - center[:, None] + f(0.5)) * invscale).astype(np.float32)
        w = _keys(arg.astype(np.float64), -0.5).astype(np.float32)
        w = np.where(j < xsize[:, None], w, f(0.0)).astype(np.float32)
        tot = np.cumsum(w, axis=1, dtype=np.float32)[:, -1:]
        w = np.where(tot != 0, w / np.where(tot != 0, tot, f(1.0)), w).astype(np.float32)
        return np.stack([xmin, xsize], 1).astype(np.int32), np.ascontiguousarray(w), ksize
    A = -0.75
    # ATen's AVX2 build contracts scale * (i + 0.5) - 0.5 into one fused multiply-subtract: a single rounding to float32
    src = (np.float64(scale) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5).astype(np.float32).astype(np.float64)
    i0 = np.floor(src)
    t = src - i0
    c1 = lambda v: ((A + 2) * v - (A + 3)) * v * v + 1
    c2 = lambda v: ((A * v - 5 * A) * v + 8 * A) * v - 4 * A
    w = np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], 1).astype(np.float32)
    bounds = np.stack([i0.astype(np.int64) - 1, np.full(out_size, 4, np.int64)], 1).astype(np.int32)
    return bounds, np.ascontiguousarray(w), 4


@functools.lru_cache(maxsize=1024)
def aten_bilinear_tables(in_size, out_size, antialias=True):
    """-> (bounds [out,2] int32, weights [out,ksize] float32, ksize) of F.interpolate(mode="bilinear", align_corners=False)
    on a float input.  Antialiased: the triangle filter max(0, 1 - |x|) over the support `scale` (1 when enlarging), index
    arithmetic and float32 normalisation as the antialiased branch of `aten_bicubic_tables`.  Plain: two taps from
    src = max(scale (i + 0.5) - 0.5, 0), i0 = floor(src) and i0 + 1, which the kernel clamps to the last index."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    i = np.arange(out_size, dtype=np.float32)
    if antialias:
        support = scale if scale >= 1.0 else f(1.0)
        invscale = f(1.0) / scale if scale >= 1.0 else f(1.0)
        ksize = int(math.ceil(float(support))) * 2 + 1
        center = scale * (i + f(0.5))
        xmin = np.maximum((center - support + f(0.5)).astype(np.int64), 0)
        xsize = np.minimum((center + support + f(0.5)).astype(np.int64), in_size) - xmin
        j = np.arange(ksize, dtype=np.int64)[None, :]
        arg = (((j + xmin[:, None]).astype(np.float32) - center[:, None] + f(0.5)) * invscale).astype(np.float32)
        w = np.maximum(f(1.0) - np.abs(arg), f(0.0)).astype(np.float32)
        w = np.where(j < xsize[:, None], w, f(0.0)).astype(np.float32)
        tot = np.cumsum(w, axis=1, dtype=np.float32)[:, -1:]
        w = np.where(tot != 0, w / np.where(tot != 0, tot, f(1.0)), w).astype(np.float32)
        return np.stack([xmin, xsize], 1).astype(np.int32), np.ascontiguousarray(w), ksize
    # one rounding to float32 of scale * (i + 0.5) - 0.5, as in the plain branch of aten_bicubic_tables
    src = (np.float64(scale) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)
    src = np.maximum(src, f(0.0))
    i0 = np.floor(src)                                          # src <= in - 0.5: i0 <= in - 1
    t = (src - i0).astype(np.float32)
    t = np.where(i0 >= in_size - 1, f(0.0), t)                  # both taps are the last sample there: (1, 0) returns it exactly
    w = np.stack([f(1.0) - t, t], 1).astype(np.float32)
    bounds = np.stack([i0.astype(np.int64), np.full(out_size, 2, np.int64)], 1).astype(np.int32)
    return bounds, np.ascontiguousarray(w), 2


_DEVICE_TABLES = collections.OrderedDict()      # (kind, in, out[, antialias], device) -> tables; LRU, a data set has few distinct sizes
_DEVICE_TABLES_MAX = 512                        # <= ~10 KB each on the device


def _on_device(key, builder, device):
    k = (key, str(device))
    hit = _DEVICE_TABLES.get(k)
    if hit is not None:
        _DEVICE_TABLES.move_to_end(k)
        return hit
    bounds, coef, ksize = builder()
    hit = (torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device), ksize, bounds)
    _DEVICE_TABLES[k] = hit
    if len(_DEVICE_TABLES) > _DEVICE_TABLES_MAX:
        _DEVICE_TABLES.popitem(last=False)      # tensors still referenced by kernels in flight stay alive through the allocator's stream ordering
    return hit


def _window(bounds_host, first, count, limit):
    """Source rows/cols touched by outputs [first, first+count): (lo, n) clamped to [0, limit)."""
    b = bounds_host[first:first + count]
    lo = max(int(b[:, 0].min()), 0)
    hi = min(int((b[:, 0] + b[:, 1]).max()), limit)
    return lo, hi - lo


def _floats(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def image_to_tensor(img_u8, size, mean, std, out=None, box=None, want_u8=False):
    """img_u8: uint8 [H, W, C] CUDA tensor (C = 1..4).  Resize(size, BICUBIC) -> CenterCrop(size) -> ToTensor ->
    Normalize(mean, std) -> float32 [C, size, size] (written into `out` if given).
    box = (top, left, height, width) with size = (out_h, out_w): RandomResizedCrop's crop-then-resize to exactly that
    size (the caller draws the box).  want_u8: also return the resized uint8 crop [size, size, C]."""
    from . import ops
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.is_cuda
    dev = img_u8.device
    if box is not None:
        top, left, bh, bw = box
        img_u8 = img_u8[top:top + bh, left:left + bw]
        oh, ow = size if isinstance(size, (tuple, list)) else (size, size)
        nh, nw, ctop, cleft, ch, cw = oh, ow, 0, 0, oh, ow
    else:
        H, W = img_u8.shape[:2]
        nh, nw = resized_output_size(H, W, size)
        ctop, cleft = center_crop_origin(nh, nw, size)
        ch = cw = size
        if ctop < 0 or cleft < 0:
            raise ValueError("image smaller than the crop after Resize: padding is not part of the evaluation transform")
    H, W, C = img_u8.shape
    if img_u8.stride(2) != 1 or img_u8.stride(1) != C:
        img_u8 = img_u8.contiguous()
    hb, hk, hks, hb_host = _on_device(("pil", W, nw), lambda: pil_bicubic_tables(W, nw), dev)
    vb, vk, vks, vb_host = _on_device(("pil", H, nh), lambda: pil_bicubic_tables(H, nh), dev)
    row0, nrows = _window(vb_host, ctop, ch, H)
    tmp = torch.empty(nrows, cw, C, device=dev, dtype=torch.uint8)
    ops.check(ops._lib.vl_resample_h_u8(ops._p(img_u8), img_u8.stride(0), W, C, row0, nrows, ops._p(hb), ops._p(hk), hks, cleft, cw,
                                        ops._p(tmp), ops._stream()))
    if out is None:
        out = torch.empty(C, ch, cw, device=dev, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C, ch, cw)
    u8 = torch.empty(ch, cw, C, device=dev, dtype=torch.uint8) if want_u8 else None
    ops.check(ops._lib.vl_resample_v_u8_norm(ops._p(tmp), cw, C, row0, nrows, ops._p(vb), ops._p(vk), vks, ctop, ch, _floats(mean), _floats(std),
                                             ops._p(out), ops._p(u8), ops._stream()))
    return (out, u8) if want_u8 else out


def plane_to_tensor(plane, size, mean, std, clamp=None, antialias=True, out=None, crop=None):
    """plane: float32 [H, W] CUDA tensor.  clamp = (lo, hi, divide_by) is applied as the source is read (DepthNorm;
    (0, 255, 255) turns the float-cast bytes of an image channel into ToTensor's [0, 1] range).  Resize(size, bicubic)
    -> CenterCrop(crop or size) -> (x - mean) / std -> float32 [crop, crop] written to `out` (any [.., crop, crop] view)."""
    from . import ops
    assert plane.dtype == torch.float32 and plane.dim() == 2 and plane.is_cuda
    dev = plane.device
    if plane.stride(1) != 1:
        plane = plane.contiguous()
    crop = size if crop is None else crop
    H, W = plane.shape
    nh, nw = resized_output_size(H, W, size)
    ctop, cleft = center_crop_origin(nh, nw, crop)
    if ctop < 0 or cleft < 0:
        raise ValueError("input smaller than the crop after Resize")
    hb, hw, hks, _ = _on_device(("aten", W, nw, antialias), lambda: aten_bicubic_tables(W, nw, antialias), dev)
    vb, vw, vks, vb_host = _on_device(("aten", H, nh, antialias), lambda: aten_bicubic_tables(H, nh, antialias), dev)
    row0, nrows = _window(vb_host, ctop, crop, H)
    tmp = torch.empty(nrows, crop, device=dev, dtype=torch.float32)
    lo, hi, div = clamp if clamp is not None else (0.0, 0.0, 1.0)
    ops.check(ops._lib.vl_resample_h_f32(ops._p(plane), plane.stride(0), W, row0, nrows, ops._p(hb), ops._p(hw), hks, cleft, crop,
                                         int(clamp is not None), float(lo), float(hi), float(div), ops._p(tmp), ops._stream()))
    if out is None:
        out = torch.empty(crop, crop, device=dev, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == crop * crop
    ops.check(ops._lib.vl_resample_v_f32_norm(ops._p(tmp), crop, H, row0, ops._p(vb), ops._p(vw), vks, ctop, crop, float(mean),
                                              float(std), ops._p(out), ops._stream()))
    return out


def depth_to_tensor(depth, size, mean, std, clamp=None, antialias=True, out=None):
    """depth: float32 [H, W] CUDA tensor.  clamp = (lo, hi, divide_by) = DepthNorm; Resize(size, bicubic) ->
    CenterCrop(size) -> (x - mean) / std -> float32 [1, size, size]."""
    if out is None:
        out = torch.empty(1, size, size, device=depth.device, dtype=torch.float32)
    plane_to_tensor(depth, size, mean, std, clamp=clamp, antialias=antialias, out=out)
    return out


def float_image_to_tensor(img_u8, size, crop, mean, std, antialias=True, out=None):
    """ToTensor FIRST, then Resize on the float tensor (the tactile recipe, modal_tactile/processors/tact_processor.py:
    286-295): img_u8 uint8 [H, W, C] CUDA -> float32 [C, crop, crop]; each channel through the float resampler with the
    /255 of ToTensor fused into the read."""
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.is_cuda
    C = img_u8.shape[2]
    planes = img_u8.permute(2, 0, 1).to(torch.float32).contiguous()               # dtype cast only; the arithmetic is in the kernels
    if out is None:
        out = torch.empty(C, crop, crop, device=img_u8.device, dtype=torch.float32)
    for c in range(C):
        plane_to_tensor(planes[c], size, mean[c], std[c], clamp=(0.0, 255.0, 255.0), antialias=antialias, out=out[c], crop=crop)
    return out


class BatchPlan:
    """Device-side description of one batched transform: descriptors, packed tables, intermediate, and the tensors that
    keep the source bytes alive.  `launch()` enqueues the two kernels; it can be repeated (same inputs, same output)."""

    def __init__(self, desc, tables, tmp, out, n, C, ch, cw, max_nrows, mean, std, keep):
        self.desc, self.tables, self.tmp, self.out, self.keep = desc, tables, tmp, out, keep
        self.n, self.C, self.ch, self.cw, self.max_nrows, self.mean, self.std = n, C, ch, cw, max_nrows, mean, std

    def launch(self):
        from . import ops
        ops.check(ops._lib.vl_resample_batch_u8_norm(ops._p(self.desc), self.n, self.C, self.ch, self.cw, self.max_nrows,
                                                     ops._p(self.tables), ops._p(self.tmp), _floats(self.mean), _floats(self.std),
                                                     ops._p(self.out), ops._stream()))
        return self.out


def plan_images(images, size, mean, std, out=None, boxes=None):
    """Host side of `images_to_tensor`: copies host images to the device (one buffer, one slice per image - small
    pageable copies are the fast path of the HIP runtime, a single 100 MB pageable copy is not), builds the packed
    per-axis tables of the distinct sizes and one int64 descriptor row per image."""
    n = len(images)
    assert n > 0
    dev = out.device if out is not None else next((im.device for im in images if im.is_cuda), torch.device("cuda"))
    ch, cw = (size, size) if isinstance(size, int) else tuple(size)
    C = images[0].shape[2]
    host_idx = [i for i, im in enumerate(images) if not im.is_cuda]
    host_off, total = {}, 0
    for i in host_idx:
        host_off[i] = total
        total += images[i].numel()
    packed = torch.empty(total, device=dev, dtype=torch.uint8) if host_idx else None
    for i in host_idx:
        packed[host_off[i]:host_off[i] + images[i].numel()].copy_(images[i].reshape(-1), non_blocking=True)
    parts, offsets, cursor = [], {}, 0

    def table(in_size, out_size):
        nonlocal cursor
        key = (in_size, out_size)
        if key not in offsets:
            b, kk, ks = pil_bicubic_tables(in_size, out_size)
            offsets[key] = (cursor, cursor + b.size, ks, b)
            parts.extend((b.reshape(-1), kk.reshape(-1)))
            cursor += b.size + kk.size
        return offsets[key]
    desc = np.zeros((n, 16), np.int64)
    tmp_bytes, max_nrows, keep = 0, 0, [packed]
    for i, im in enumerate(images):
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == C
        H, W = im.shape[:2]
        if im.is_cuda:
            if im.stride(2) != 1 or im.stride(1) != C:
                im = im.contiguous()
            keep.append(im)
            base, stride = im.data_ptr(), im.stride(0)
        else:
            base, stride = packed.data_ptr() + host_off[i], W * C
        if boxes is not None:
            top, left, H, W = boxes[i]
            base += top * stride + left * C
            nh, nw, ctop, cleft = ch, cw, 0, 0
        else:
            nh, nw = resized_output_size(H, W, ch)
            ctop, cleft = center_crop_origin(nh, nw, ch)
            if ctop < 0 or cleft < 0:
                raise ValueError("image smaller than the crop after Resize")
        hb_off, hk_off, hks, _ = table(W, nw)
        vb_off, vk_off, vks, vb_host = table(H, nh)
        row0, nrows = _window(vb_host, ctop, ch, H)
        desc[i, :14] = (base, stride, W, row0, nrows, cleft, ctop, hb_off, hk_off, hks, vb_off, vk_off, vks, tmp_bytes)
        tmp_bytes += nrows * cw * C
        max_nrows = max(max_nrows, nrows)
    tables = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=True)
    desc_d = torch.from_numpy(desc).to(dev, non_blocking=True)
    tmp = torch.empty(tmp_bytes, device=dev, dtype=torch.uint8)
    if out is None:
        out = torch.empty(n, C, ch, cw, device=dev, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, C, ch, cw)
    return BatchPlan(desc_d, tables, tmp, out, n, C, ch, cw, max_nrows, mean, std, keep)


def images_to_tensor(images, size, mean, std, out=None, boxes=None):
    """A LIST of uint8 [H, W, C] images of different sizes (CPU or CUDA tensors, same C) -> float32 [n, C, size, size]
    in two kernel launches (vl_resample_batch_u8_norm): same arithmetic and bits as `image_to_tensor` per image.
    boxes[i] = (top, left, h, w): crop-then-resize (training)."""
    return plan_images(images, size, mean, std, out=out, boxes=boxes).launch()


def _jitter_flags(rec, draw):
    """The flip, the jitter order and the enabled terms of a draw -> the record's flag bits; writes factor and 1 - factor (the
    difference formed in double, as torchvision's _blend forms it, then rounded to float32) and the hue shift into `rec`."""
    from . import ops
    order = [int(k) for k in draw["order"]]
    if sorted(order) != [0, 1, 2, 3]:
        raise ValueError(f"the jitter order must be a permutation of 0..3, got {order}")
    flags = (ops.RGBD_FLIP if draw["flip"] else 0) | sum(k << (ops.RGBD_ORDER_SHIFT + 2 * pos) for pos, k in enumerate(order))
    for name, bit, f, f1 in (("brightness", ops.RGBD_BRIGHTNESS, "b", "b1"), ("contrast", ops.RGBD_CONTRAST, "c", "c1"),
                             ("saturation", ops.RGBD_SATURATION, "s", "s1")):
        v = draw.get(name)
        if v is not None:
            flags |= bit
            rec[f], rec[f1] = float(v), 1.0 - float(v)
    if draw.get("hue") is not None:
        flags |= ops.RGBD_HUE
        rec["hue"] = float(draw["hue"])
    return flags


def rgbd_record_scalars(rec, draw):
    """Write a draw's scalars into one RGBD_AUGMENT_DTYPE row: the box, the flip, the jitter order, the enabled terms with
    factor and 1 - factor (`_jitter_flags`), the erase rectangle.  draw: {"box": (top, left, h, w), "flip": bool, "order": 4 ids
    (0 brightness, 1 contrast, 2 saturation, 3 hue), "brightness" / "contrast" / "saturation" / "hue": a float or None (term
    off), "erase": (i, j, h, w) or None}."""
    from . import ops
    rec["top"], rec["left"], rec["bh"], rec["bw"] = draw["box"]
    flags = _jitter_flags(rec, draw)
    if draw.get("erase") is not None:
        flags |= ops.RGBD_ERASE
        rec["ei"], rec["ej"], rec["eh"], rec["ew"] = draw["erase"]
    rec["flags"] = flags


def _table_packer(build):
    """-> (table, parts): table(in_size) -> (offset of the bounds, offset of the coefficients, taps per row, host bounds) of
    `build(in_size)` = (bounds, coefficients, ksize) inside the concatenation of `parts`, counted in 32-bit words; each distinct
    size is packed once."""
    parts, offsets, cursor = [], {}, 0

    def table(in_size):
        nonlocal cursor
        if in_size not in offsets:
            b, coef, ks = build(in_size)
            offsets[in_size] = (cursor, cursor + b.size, ks, b)
            parts.extend((b.reshape(-1), coef.reshape(-1).view(np.int32)))
            cursor += b.size + coef.size
        return offsets[in_size]
    return table, parts


def _box_fields(r, box, H, W, S, table, who, i, coef="w"):
    """The crop box of sample i of plan `who` against its H x W image -> its record fields: the two tables' offsets and tap
    counts (`hb`, `h<coef>`, `hks` for the box width -> S, `v..` for the height) and the rows of the box that the vertical taps
    of the S output rows touch (`row0`, `nrows`).  -> nrows"""
    top, left, bh, bw = (int(v) for v in box)
    if not (0 <= top and 1 <= bh and top + bh <= H and 0 <= left and 1 <= bw and left + bw <= W):
        raise ValueError(f"{who}: box {box} of sample {i} is not inside its {H} x {W} image")
    r["hb"], r["h" + coef], r["hks"], _ = table(bw)
    r["vb"], r["v" + coef], r["vks"], vb_host = table(bh)
    r["row0"], r["nrows"] = _window(vb_host, 0, S, bh)
    return int(r["nrows"])


def _upload_packed(rec, pack, tables, host, dev):
    """Everything the host provides for a batch in ONE pinned buffer and ONE copy, laid out as records | tables (16-byte
    aligned) | host sources in the order given.  rec: the record array; host: (sample, pointer field, source tensor) - the
    field receives the source's device address before `pack(rec)` checks the records and gives their words.
    -> (records int32 [n, words], tables int32 [*], the device buffer that holds both and the sources)."""
    off_tables = (rec.nbytes + 15) & ~15
    cursor = off_tables + tables.nbytes
    place = []
    for i, field, t in host:
        place.append(cursor)
        cursor += t.numel() * t.element_size()
    packed = torch.empty(max(cursor, 1), device=dev, dtype=torch.uint8)
    for (i, field, _), off in zip(host, place):
        rec[i][field] = packed.data_ptr() + off
    stage = torch.empty(cursor, dtype=torch.uint8, pin_memory=dev.type == "cuda")
    buf = stage.numpy()
    buf[:rec.nbytes] = pack(rec).view(np.uint8).reshape(-1)
    buf[off_tables:off_tables + tables.nbytes] = tables.view(np.uint8)
    for (_, _, t), off in zip(host, place):
        stage[off:off + t.numel() * t.element_size()].copy_(t.contiguous().view(torch.uint8).reshape(-1))
    packed.copy_(stage, non_blocking=True)
    records = packed[:rec.nbytes].view(torch.int32).view(len(rec), -1)
    return records, packed[off_tables:off_tables + tables.nbytes].view(torch.int32), packed


class RgbdPlan:
    """Device-side description of one batch of the depth training transform: the packed buffer (records, tables, host
    sources), the intermediate and the tensors that keep device sources alive.  `launch()` enqueues vl_rgbd_augment; it can
    be repeated (same inputs, same outputs)."""

    def __init__(self, records, tables, tmp, n, S, max_nrows, mean, std, depth_clamp, keep):
        self.records, self.tables, self.tmp, self.keep = records, tables, tmp, keep
        self.n, self.S, self.max_nrows, self.mean, self.std, self.depth_clamp = n, S, max_nrows, mean, std, depth_clamp

    def launch(self, out_rgb=None, out_depth=None):
        from . import ops
        return ops.rgbd_augment(self.records, self.tables, self.tmp, self.S, self.max_nrows, self.mean, self.std, self.depth_clamp,
                                out_rgb=out_rgb, out_depth=out_depth)


def plan_rgbd(images, depths, draws, size, mean, std, depth_clamp, antialias=True, device="cuda"):
    """Host side of the depth training transform.  images[i]: uint8 [H, W, 3] tensor, depths[i]: float32 [H, W] tensor of
    the same H, W (host or device; sizes differ between samples), draws[i]: the sample's scalars (`rgbd_record_scalars`).
    Everything the host provides - records, the packed bilinear tables of the distinct (box edge -> size) pairs, host
    depth maps and host image bytes - is laid out in ONE pinned buffer and travels in ONE copy; device sources are read
    where they are."""
    from . import ops
    n, S, dev = len(images), int(size), torch.device(device)
    if n < 1 or len(depths) != n or len(draws) != n:
        raise ValueError(f"plan_rgbd: {n} images, {len(depths)} depth maps, {len(draws)} draws")
    rec = np.zeros(n, dtype=ops.RGBD_AUGMENT_DTYPE)
    table, parts = _table_packer(lambda in_size: aten_bilinear_tables(in_size, S, antialias))
    tmp_vec, keep, host = 0, [], []                    # host: (sample, record field, source tensor) to be packed
    for i, (im, dp, draw) in enumerate(zip(images, depths, draws)):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"plan_rgbd: image {i} must be uint8 [H, W, 3], got {tuple(im.shape)} {im.dtype}")
        H, W = im.shape[:2]
        if dp.dtype != torch.float32 or tuple(dp.shape) != (H, W):
            raise ValueError(f"plan_rgbd: depth {i} must be float32 [{H}, {W}] like its image, got {tuple(dp.shape)} {dp.dtype}")
        r = rec[i]
        r["H"], r["W"], r["rgb_stride"], r["depth_stride"] = H, W, 3 * W, W
        for field, t in (("rgb", im), ("depth", dp)):
            if t.is_cuda:
                t = t.contiguous()
                keep.append(t)
                r[field] = t.data_ptr()
            else:
                host.append((i, field, t))
        rgbd_record_scalars(r, draw)
        r["tmp"] = tmp_vec
        tmp_vec += _box_fields(r, draw["box"], H, W, S, table, "plan_rgbd", i) * S
    # host depth maps (4-byte aligned) go in front of host image bytes
    records, tables_d, packed = _upload_packed(rec, lambda r: ops.rgbd_augment_pack(r, S), np.concatenate(parts),
                                               sorted(host, key=lambda h: h[1] != "depth"), dev)
    tmp = torch.empty(tmp_vec, 4, device=dev, dtype=torch.float32)
    keep.append(packed)
    return RgbdPlan(records, tables_d, tmp, n, S, int(rec["nrows"].max()), list(mean), list(std), tuple(depth_clamp), keep)


# ---------------------------------------------------------------------------------------------- the tactile training transform
def tactile_record_scalars(rec, draw, S):
    """Write a draw's scalars into one TACTILE_AUGMENT_DTYPE row for an S x S output: the box, the two flips, the rotation.
    draw: {"box": (top, left, h, w), "flip_h": bool, "flip_v": bool, "angle": degrees}.  The rotation is F.rotate's of a
    tensor: `affine_inverse_matrix` for -angle about the centre in doubles, rounded to float32, its four rotation entries
    divided in float32 by float32(0.5 S) (torchvision's rescaled theta; the two translations are 0)."""
    from . import ops
    rec["top"], rec["left"], rec["bh"], rec["bw"] = draw["box"]
    rec["flags"] = (ops.TACTILE_HFLIP if draw["flip_h"] else 0) | (ops.TACTILE_VFLIP if draw["flip_v"] else 0)
    m = np.array(affine_inverse_matrix([0.0, 0.0], -float(draw["angle"]), [0.0, 0.0], [0.0, 0.0]), dtype=np.float64).astype(np.float32)
    rec["t00"], rec["t01"], rec["t10"], rec["t11"] = m[[0, 1, 3, 4]] / np.float32(0.5 * S)


class TactilePlan:
    """Device-side description of one batch of the tactile training transform: the packed buffer (records, tables, host
    sources), the intermediate and the tensors that keep device sources alive.  `launch()` enqueues vl_tactile_augment; it
    can be repeated (same inputs, same output)."""

    def __init__(self, records, tables, tmp, n, S, max_nrows, mean, std, keep):
        self.records, self.tables, self.tmp, self.keep = records, tables, tmp, keep
        self.n, self.S, self.max_nrows, self.mean, self.std = n, S, max_nrows, mean, std

    def launch(self, out=None):
        from . import ops
        return ops.tactile_augment(self.records, self.tables, self.tmp, self.S, self.max_nrows, self.mean, self.std, out=out)


def plan_tactile_train(images, draws, size, mean, std, antialias=True, device="cuda"):
    """Host side of the tactile training transform.  images[i]: uint8 [H, W, 3] tensor (host or device; sizes differ between
    samples), draws[i]: the sample's scalars (`tactile_record_scalars`).  Everything the host provides - records, the packed
    bilinear tables of the distinct (box edge -> size) pairs, host image bytes - is laid out in ONE pinned buffer and travels
    in ONE copy; device sources are read where they are."""
    from . import ops
    n, S, dev = len(images), int(size), torch.device(device)
    if n < 1 or len(draws) != n:
        raise ValueError(f"plan_tactile_train: {n} images, {len(draws)} draws")
    rec = np.zeros(n, dtype=ops.TACTILE_AUGMENT_DTYPE)
    table, parts = _table_packer(lambda in_size: aten_bilinear_tables(in_size, S, antialias))
    tmp_vec, keep, host = 0, [], []
    for i, (im, draw) in enumerate(zip(images, draws)):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"plan_tactile_train: image {i} must be uint8 [H, W, 3], got {tuple(im.shape)} {im.dtype}")
        H, W = im.shape[:2]
        r = rec[i]
        r["H"], r["W"], r["stride"] = H, W, 3 * W
        if im.is_cuda:
            im = im.contiguous()
            keep.append(im)
            r["src"] = im.data_ptr()
        else:
            host.append((i, "src", im))
        tactile_record_scalars(r, draw, S)
        r["tmp"] = tmp_vec
        tmp_vec += _box_fields(r, draw["box"], H, W, S, table, "plan_tactile_train", i) * S
    tables = np.concatenate(parts)
    records, tables_d, packed = _upload_packed(rec, lambda r: ops.tactile_augment_pack(r, S, tables.size, tmp_vec), tables, host, dev)
    tmp = torch.empty(tmp_vec, 4, device=dev, dtype=torch.float32)
    keep.append(packed)
    return TactilePlan(records, tables_d, tmp, n, S, int(rec["nrows"].max()), list(mean), list(std), keep)


# ---------------------------------------------------------------------------------------------- the plain-image training transform
RANDAUGMENT_SIGNED = (False,) + (True,) * 9 + (False,) * 4          # per op code (ops.IMAGE_OPS): the op draws a sign


@functools.lru_cache(maxsize=64)
def randaugment_magnitudes(num_bins, S, solarize_from=256.0):
    """RandAugment's magnitude table for an S x S image -> one tuple of `num_bins` Python floats per op code (float32 values,
    as torch.linspace gives them).  `solarize_from`: 256 (the reference's copy of the table) or 255 (later torchvision)."""
    lin = lambda lo, hi: tuple(float(v) for v in torch.linspace(lo, hi, num_bins))
    zero = (0.0,) * num_bins
    shear, move, enhance = lin(0.0, 0.3), lin(0.0, 150.0 / 331.0 * S), lin(0.0, 0.9)
    # Posterize keeps 8 bits at bin 0 and 4 at the last bin, in steps of one bit: 8 - round-half-even(4 i / (bins - 1)), exact
    bits = tuple(float(8 - round(fractions.Fraction(4 * i, num_bins - 1))) for i in range(num_bins))
    return (zero, shear, shear, move, move, lin(0.0, 30.0), enhance, enhance, enhance, enhance, bits, lin(float(solarize_from), 0.0),
            zero, zero)


def affine_inverse_matrix(center, angle, translate, shear):
    """The six doubles (a, b, c, d, e, f) that take an output pixel centre to its source position, x' = a x + b y + c,
    y' = d x + e y + f, for: rotate by `angle` and shear by `shear` = (sx, sy) (degrees) about `center`, then move by
    `translate`.  The forward matrix is T(translate) C R Sh C^-1 with R Sh = [[cos(r - sy) / cos sy, -cos(r - sy) tan sx / cos sy
    - sin r], [sin(r - sy) / cos sy, -sin(r - sy) tan sx / cos sy + cos r]] of determinant 1, so its inverse is the adjugate."""
    r, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    (cx, cy), (tx, ty) = center, translate
    a = math.cos(r - sy) / math.cos(sy)
    b = -math.cos(r - sy) * math.tan(sx) / math.cos(sy) - math.sin(r)
    c = math.sin(r - sy) / math.cos(sy)
    d = -math.sin(r - sy) * math.tan(sx) / math.cos(sy) + math.cos(r)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def pil_rotate_matrix(angle, w, h):
    """The matrix Image.rotate(angle) hands to Image.transform for a w x h image (rotation about the centre, entries rounded
    to 15 places as Pillow rounds them); None where Pillow returns a copy (a multiple of 360 degrees)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def randaugment_slot(slot, code, magnitude, S, shear_atan=False):
    """Write one op at the signed `magnitude` (a Python float) on an S x S image into a record's op slot (ops.IMAGE_OP_DTYPE):
    the geometric ops as the matrix of the Pillow call (ShearX/Y about the centre with shear = degrees(m), or with
    `shear_atan` about (0, 0) with degrees(atan(m)); TranslateX/Y by int(m); Rotate as Image.rotate), the enhance ops as the
    factor 1 + m, Posterize as the mask of int(m) kept bits, Solarize as the first inverted byte."""
    code = int(code)
    slot["code"], slot["ipay"], slot["fpay"], slot["pad"], slot["m"] = code, 0, 0.0, 0, 0.0
    centre = [S * 0.5, S * 0.5]
    m = None
    if code in (1, 2):
        deg = math.degrees(math.atan(magnitude)) if shear_atan else math.degrees(magnitude)
        m = affine_inverse_matrix([0, 0] if shear_atan else centre, 0.0, [0, 0], [deg, 0.0] if code == 1 else [0.0, deg])
    elif code in (3, 4):
        m = affine_inverse_matrix(centre, 0.0, [int(magnitude), 0] if code == 3 else [0, int(magnitude)], [0.0, 0.0])
    elif code == 5:
        m = pil_rotate_matrix(magnitude, S, S)
        if m is None:
            slot["code"] = 0                                                # Pillow's copy
    elif 6 <= code <= 9:
        slot["fpay"] = 1.0 + magnitude
    elif code == 10:
        bits = int(magnitude)
        if not 0 <= bits <= 8:
            raise ValueError(f"Posterize keeps 0 to 8 bits, got {bits}")
        slot["ipay"] = ~(2 ** (8 - bits) - 1) & 0xFF
    elif code == 11:
        slot["ipay"] = min(max(int(math.ceil(magnitude)), 0), 256)          # byte < m  <=>  byte < ceil(m)
    elif code not in (0, 12, 13):
        raise ValueError(f"unknown RandAugment op code {code}")
    if m is not None:
        slot["m"] = m


def image_record_scalars(rec, draw, S, num_bins=31, shear_atan=False, solarize_from=256.0):
    """Write a draw's scalars into one IMAGE_AUGMENT_DTYPE row: the box, the flip, the op slots, the jitter order and the
    enabled terms with factor and 1 - factor (`_jitter_flags`).  draw: {"box": (top, left, h, w), "flip": bool,
    "ops": [(code, negative, bin), ...] (at most 4), "order": 4 ids, "brightness" / "contrast" / "saturation" / "hue": a
    float or None (term off)}."""
    from . import ops
    rec["top"], rec["left"], rec["bh"], rec["bw"] = draw["box"]
    rec["flags"] = _jitter_flags(rec, draw)
    chosen = list(draw["ops"])
    if len(chosen) > ops.IMAGE_MAX_OPS:
        raise ValueError(f"at most {ops.IMAGE_MAX_OPS} RandAugment ops per sample, got {len(chosen)}")
    table = randaugment_magnitudes(num_bins, S, solarize_from)
    rec["num_ops"] = len(chosen)
    for k, (code, negative, mag_bin) in enumerate(chosen):
        if not (0 <= int(code) < len(table) and 0 <= int(mag_bin) < num_bins):
            raise ValueError(f"op {k}: code {code} or magnitude bin {mag_bin} out of range")
        mag = table[int(code)][int(mag_bin)]
        randaugment_slot(rec["ops"][k], code, -mag if (negative and RANDAUGMENT_SIGNED[int(code)]) else mag, S, shear_atan)


class ImagePlan:
    """Device-side description of one batch of the plain-image training transform: the packed buffer (records, tables, host
    sources), the intermediate and the tensors that keep device sources alive.  `launch()` enqueues vl_image_augment; it can
    be repeated (same inputs, same outputs)."""

    def __init__(self, records, tables, tmp, n, S, max_nrows, max_ops, mean, std, keep):
        self.records, self.tables, self.tmp, self.keep = records, tables, tmp, keep
        self.n, self.S, self.max_nrows, self.max_ops, self.mean, self.std = n, S, max_nrows, max_ops, mean, std

    def launch(self, out=None, out_u8=None, want_u8=False):
        from . import ops
        return ops.image_augment(self.records, self.tables, self.tmp, self.S, self.max_nrows, self.max_ops, self.mean, self.std,
                                 out=out, out_u8=out_u8, want_u8=want_u8)

    def crop_resize(self):
        from . import ops
        return ops.image_crop_resize_u8(self.records, self.tables, self.tmp, self.S, self.max_nrows)


def plan_image_train(images, draws, size, mean, std, num_bins=31, shear_atan=False, solarize_from=256.0, device="cuda"):
    """Host side of the plain-image training transform.  images[i]: uint8 [H, W, 3] tensor (host or device; sizes differ
    between samples), draws[i]: the sample's scalars (`image_record_scalars`).  Everything the host provides - records, the
    packed Pillow bilinear tables of the distinct (box edge -> size) pairs, host image bytes - is laid out in ONE pinned
    buffer and travels in ONE copy; device sources are read where they are."""
    from . import ops
    n, S, dev = len(images), int(size), torch.device(device)
    if n < 1 or len(draws) != n:
        raise ValueError(f"plan_image_train: {n} images, {len(draws)} draws")
    rec = np.zeros(n, dtype=ops.IMAGE_AUGMENT_DTYPE)
    table, parts = _table_packer(lambda in_size: pil_bilinear_tables(in_size, S))
    tmp_bytes, keep, host = 0, [], []
    for i, (im, draw) in enumerate(zip(images, draws)):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"plan_image_train: image {i} must be uint8 [H, W, 3], got {tuple(im.shape)} {im.dtype}")
        H, W = im.shape[:2]
        r = rec[i]
        r["H"], r["W"], r["stride"] = H, W, 3 * W
        if im.is_cuda:
            im = im.contiguous()
            keep.append(im)
            r["src"] = im.data_ptr()
        else:
            host.append((i, "src", im))
        image_record_scalars(r, draw, S, num_bins, shear_atan, solarize_from)
        r["tmp"] = tmp_bytes
        tmp_bytes += _box_fields(r, draw["box"], H, W, S, table, "plan_image_train", i, coef="k") * S * 3
    tables = np.concatenate(parts)
    records, tables_d, packed = _upload_packed(rec, lambda r: ops.image_augment_pack(r, S, tables.size, tmp_bytes), tables, host, dev)
    tmp = torch.empty(tmp_bytes, device=dev, dtype=torch.uint8)
    keep.append(packed)
    return ImagePlan(records, tables_d, tmp, n, S, int(rec["nrows"].max()), int(rec["num_ops"].max()), list(mean), list(std), keep)
