"""Throughput of the on-GPU preprocessing next to the reference's CPU pipeline on the same inputs.

GPU side: bytes already resident in HBM (the image transform's two kernels per image), and, separately, with the
host->device copy of each decoded image inside the timed region.  CPU side ("port" of what the reference's data-loader
workers run): Pillow bicubic resize + crop + torch ToTensor/Normalize for images, F.interpolate for disparity maps,
one thread.  Prints one JSON object; `python tools/preproc_bench.py > gpurun_out/preproc_bench.json`."""
# `--pc-train-only` prints the row of the 3D training transform alone (PCProcessorTrain against the numpy restatement of the
# reference's five passes on the host's cores); `--rgbd-train-only` the row of the depth training transform alone
# (RGBD_Processor_Train against the torch restatement of the reference's pipeline on the host's cores); `--image-train-only`
# the row of the plain-image training transform alone (Image_Processor_Train against the same draws applied with Pillow on one
# host thread); `--tactile-train-only` the row of the tactile training transform alone (Tactile_Processor_Train against the torch
# restatement of the same draws on one host thread)
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))

from open_clip.constants import OPENAI_DATASET_MEAN as MEAN, OPENAI_DATASET_STD as STD  # noqa: E402
from open_clip.modal_depth.processors.vt_processor import DepthProcessorEval  # noqa: E402
from open_clip.transform import image_transform  # noqa: E402
from vitlens_hip import preproc  # noqa: E402


def gpu_time(fn, n_warm=1):
    for _ in range(n_warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def pc_train_row(B=1024, N=8192, threads=16):
    """PCProcessorTrain.process_batch at B x N points, every point selected (a permutation per cloud, already on the GPU), next
    to the reference's loader-side work on the same clouds: pc_norm + random_point_dropout + scale + shift + the two
    rotations in numpy (tests/pc_augment_ref.py, pinned to the reference), on one thread and on a pool of `threads`."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pc_augment_ref as R
    from open_clip.modal_3d.processors.pc_processor import PCProcessorTrain
    from vitlens_hip import ops
    host = np.random.default_rng(1).normal(size=(B, N, 3)).astype(np.float32)
    pcs = torch.from_numpy(host).cuda()
    sub = torch.stack([torch.randperm(N) for _ in range(B)]).cuda()
    proc = PCProcessorTrain(npoint=N, uniform=True, seed=0)
    row = {"n": B, "in": [N, 3], "npoint": N}
    params = ops.pc_augment_params(proc.draw_records(B), "cuda")
    s = min(gpu_time(lambda: ops.pc_augment(pcs, sub, params), n_warm=2) for _ in range(5))
    row["gpu_kernel_us_per_batch"] = round(s * 1e6, 1)
    row["gpu_kernel_gb_per_s"] = round(B * N * (12 + 12 + 8) / s / 1e9, 1)          # points read, points written, indices read
    proc.process_batch(pcs, subset=sub); torch.cuda.synchronize()
    t0 = time.perf_counter(); proc.process_batch(pcs, subset=sub); torch.cuda.synchronize()
    row["gpu_process_batch_ms"] = round((time.perf_counter() - t0) * 1e3, 2)         # with the host's B draws and their upload
    t0 = time.perf_counter(); proc.draw_records(B)
    row["host_draws_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 2)

    def one(b):
        rng = np.random.RandomState(b)
        return R.vitlens_pipeline(R.pc_norm(host[b]), R.draw_reference(N, "vitlens", rng))

    n_cpu = min(B, 256)
    t0 = time.perf_counter()
    for b in range(n_cpu):
        one(b)
    row["cpu_1thread_ms_per_batch"] = round((time.perf_counter() - t0) / n_cpu * B * 1e3, 1)
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter(); list(pool.map(one, range(B)))
        row[f"cpu_{threads}threads_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
    row[f"cpu_1thread_over_{threads}_ms_per_batch"] = round(row["cpu_1thread_ms_per_batch"] / threads, 1)   # perfect scaling
    return row


def rgbd_train_row(B=1024, H=480, W=640, threads=16, distinct=64):
    """RGBD_Processor_Train.process_batch at B samples of H x W (`distinct` different sources, each used B / distinct times),
    next to the reference's loader-side work on the same samples: the torch restatement of its pipeline
    (tests/rgbd_augment_ref.py, float32, per-sample draws included) on one thread and on a pool of `threads`."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rgbd_augment_ref as R
    from open_clip.modal_depth.processors.vt_processor import RGBD_Processor_Train
    src = [R.sample(H, W, 100 + i) for i in range(distinct)]
    images, depths = [src[i % distinct][0] for i in range(B)], [src[i % distinct][1] for i in range(B)]
    dev = [(a.cuda(), b.cuda()) for a, b in src]
    images_d, depths_d = [dev[i % distinct][0] for i in range(B)], [dev[i % distinct][1] for i in range(B)]
    proc = RGBD_Processor_Train.from_config()
    row = {"n": B, "in": [H, W], "size": proc.size, "source_mb_per_batch": round(B * H * W * 7 / 1e6, 1)}
    torch.manual_seed(0)
    draws = [proc.draw(H, W) for _ in range(B)]
    plan = preproc.plan_rgbd(images_d, depths_d, draws, proc.size, proc.mean, proc.std, proc.depth_clamp, antialias=proc.antialias)
    row["intermediate_mb"] = round(plan.tmp.numel() * 4 / 1e6, 1)
    s = min(gpu_time(plan.launch, n_warm=2) for _ in range(5))
    row["gpu_kernels_ms_per_batch"] = round(s * 1e3, 3)                              # the three launches, sources resident

    def timed(fn):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2)
    row["gpu_process_batch_ms_resident_sources"] = timed(lambda: proc.process_batch(images_d, depths_d))   # draws, records, launch
    row["gpu_process_batch_ms_host_sources"] = timed(lambda: proc.process_batch(images, depths))           # + packing and upload
    t0 = time.perf_counter(); [proc.draw(H, W) for _ in range(B)]
    row["host_draws_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 2)

    def one(b):
        return R.apply(images[b], depths[b], R.draw(H, W, proc.size), proc.size, proc.mean, proc.std, proc.antialias, torch.float32)

    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    n_cpu = min(B, 64)
    t0 = time.perf_counter()
    for b in range(n_cpu):
        one(b)
    row["cpu_1thread_ms_per_batch"] = round((time.perf_counter() - t0) / n_cpu * B * 1e3, 1)
    n_pool = min(B, 256)
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter(); list(pool.map(one, range(n_pool)))
        row[f"cpu_{threads}threads_ms_per_batch"] = round((time.perf_counter() - t0) / n_pool * B * 1e3, 1)
    torch.set_num_threads(nt)
    row[f"cpu_1thread_over_{threads}_ms_per_batch"] = round(row["cpu_1thread_ms_per_batch"] / threads, 1)   # perfect scaling
    return row


def image_train_row(B=1024, H=480, W=640, distinct=64):
    """Image_Processor_Train.batch at B samples of H x W (`distinct` different sources, each used B / distinct times): the
    three launches alone, `batch` as a whole with resident and with host sources, the host's share (draws, planning), and
    the same draws applied with Pillow and torch on one host thread (tests/image_augment_ref.py), the yardstick."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import image_augment_ref as A
    from open_clip.modal_tactile.processors.tact_processor import Image_Processor_Train
    src = [torch.from_numpy(A.source(H, W, "random", seed=200 + i)) for i in range(distinct)]
    images = [src[i % distinct] for i in range(B)]
    dev = [a.cuda() for a in src]
    images_d = [dev[i % distinct] for i in range(B)]
    proc = Image_Processor_Train.from_config()
    row = {"n": B, "in": [H, W], "size": proc.size, "num_ops": proc.num_ops, "magnitude": proc.magnitude,
           "source_mb_per_batch": round(B * H * W * 3 / 1e6, 1)}
    torch.manual_seed(0)
    t0 = time.perf_counter(); draws = [proc.draw(H, W) for _ in range(B)]
    row["host_draws_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 2)
    plan_of = lambda ims: preproc.plan_image_train(ims, draws, proc.size, proc.mean, proc.std)
    plan = plan_of(images_d)
    row["intermediate_mb"] = round(plan.tmp.numel() / 1e6, 1)
    out = torch.empty(B, 3, proc.size, proc.size, device="cuda")
    s = min(gpu_time(lambda: plan.launch(out=out), n_warm=2) for _ in range(5))
    row["gpu_kernels_ms_per_batch"] = round(s * 1e3, 3)                              # the three launches, sources resident
    s = min(gpu_time(plan.crop_resize, n_warm=2) for _ in range(5))
    row["gpu_crop_resize_ms_per_batch"] = round(s * 1e3, 3)                          # the first two of them

    def timed(fn):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2)
    row["host_plan_ms_resident_sources"] = timed(lambda: plan_of(images_d))          # records, tables, one upload
    row["host_plan_ms_host_sources"] = timed(lambda: plan_of(images))                # + packing and upload of the image bytes
    row["gpu_batch_ms_resident_sources"] = timed(lambda: proc.batch(images_d))       # draws, planning, launches
    row["gpu_batch_ms_host_sources"] = timed(lambda: proc.batch(images))
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    n_cpu = min(B, 128)
    t0 = time.perf_counter()
    for b in range(n_cpu):
        A.float_tail(A.eight_bit(images[b].numpy(), draws[b], proc.size), draws[b], proc.mean, proc.std)
    row["pillow_1thread_ms_per_batch"] = round((time.perf_counter() - t0) / n_cpu * B * 1e3, 1)
    torch.set_num_threads(nt)
    return row


def tactile_train_row(B=1024, H=480, W=640, distinct=64):
    """Tactile_Processor_Train.batch at B samples of H x W (`distinct` different sources, each used B / distinct times): the
    two launches alone, `batch` as a whole with resident and with host sources, the host's share (draws, planning), and the
    same draws through the torch restatement on one host thread (tests/tactile_augment_ref.py), the yardstick.
    The gather of the second launch is priced by running the same boxes with angle 0 and no flips (every load coalesced, every
    pixel computed: the work of a vertical pass that materialises the resized image) and by a plain device copy of the output
    (read + write of [B,3,S,S] f32: the least a separate gather launch could cost)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tactile_augment_ref as T
    from open_clip.modal_tactile.processors.tact_processor import Tactile_Processor_Train
    src = [T.source(H, W, 300 + i) for i in range(distinct)]
    images = [src[i % distinct] for i in range(B)]
    dev = [a.cuda() for a in src]
    images_d = [dev[i % distinct] for i in range(B)]
    proc = Tactile_Processor_Train.from_config()
    row = {"n": B, "in": [H, W], "size": proc.size, "source_mb_per_batch": round(B * H * W * 3 / 1e6, 1)}
    torch.manual_seed(0)
    t0 = time.perf_counter(); draws = [proc.draw(H, W) for _ in range(B)]
    row["host_draws_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 2)
    plan_of = lambda ims, dr=draws: preproc.plan_tactile_train(ims, dr, proc.size, proc.mean, proc.std, antialias=proc.antialias)
    plan = plan_of(images_d)
    row["intermediate_mb"] = round(plan.tmp.numel() * 4 / 1e6, 1)
    row["fill_share"] = round(float(np.mean([(T.index_map(proc.size, d["angle"]) < 0).mean() for d in draws[:64]])), 4)
    out = torch.empty(B, 3, proc.size, proc.size, device="cuda")
    s = min(gpu_time(lambda: plan.launch(out=out), n_warm=2) for _ in range(5))
    row["gpu_kernels_ms_per_batch"] = round(s * 1e3, 3)                              # the two launches, sources resident
    still = plan_of(images_d, [dict(d, flip_h=False, flip_v=False, angle=0.0) for d in draws])
    s = min(gpu_time(lambda: still.launch(out=out), n_warm=2) for _ in range(5))
    row["gpu_kernels_ms_per_batch_angle0_no_flips"] = round(s * 1e3, 3)              # same boxes, the gather is the identity
    other = torch.empty_like(out)
    s = min(gpu_time(lambda: other.copy_(out), n_warm=2) for _ in range(5))
    row["device_copy_of_output_ms"] = round(s * 1e3, 3)                              # floor of a third (gather) launch
    del still, other

    def timed(fn):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2)
    row["host_plan_ms_resident_sources"] = timed(lambda: plan_of(images_d))          # records, tables, one upload
    row["host_plan_ms_host_sources"] = timed(lambda: plan_of(images))                # + packing and upload of the image bytes
    row["gpu_batch_ms_resident_sources"] = timed(lambda: proc.batch(images_d))       # draws, planning, launches
    row["gpu_batch_ms_host_sources"] = timed(lambda: proc.batch(images))
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    n_cpu = min(B, 64)
    t0 = time.perf_counter()
    for b in range(n_cpu):
        T.apply(images[b], draws[b], proc.size, proc.mean, proc.std, proc.antialias, torch.float32)
    row["cpu_1thread_ms_per_batch"] = round((time.perf_counter() - t0) / n_cpu * B * 1e3, 1)
    torch.set_num_threads(nt)
    return row


def main():
    if "--tactile-train-only" in sys.argv[1:]:
        print(json.dumps({"tactile_train": tactile_train_row()}))
        return
    if "--image-train-only" in sys.argv[1:]:
        print(json.dumps({"image_train": image_train_row()}))
        return
    if "--pc-train-only" in sys.argv[1:]:
        print(json.dumps({"pc_train": pc_train_row()}))
        return
    if "--rgbd-train-only" in sys.argv[1:]:
        print(json.dumps({"rgbd_train": rgbd_train_row()}))
        return
    N, H, W = 256, 375, 500                                                       # ImageNet-typical decoded size
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    dev = [torch.from_numpy(h).cuda() for h in host]
    t = image_transform(224, is_train=False)
    out = torch.empty(N, 3, 224, 224, device="cuda")
    res = {"image": {"n": N, "in": [H, W, 3], "out": [3, 224, 224]}}
    s = gpu_time(lambda: [preproc.image_to_tensor(d, 224, MEAN, STD, out=out[i]) for i, d in enumerate(dev)])
    res["image"]["gpu_resident_img_per_s"] = round(N / s, 1)
    res["image"]["gpu_resident_us_per_img"] = round(s / N * 1e6, 2)
    res["image"]["bytes_per_img"] = H * W * 3 + 3 * 224 * 224 * 4                  # decoded bytes read once + float32 written once
    t0 = time.perf_counter()
    for i, h in enumerate(host):
        t(h, out=out[i])
    torch.cuda.synchronize(); s2 = time.perf_counter() - t0
    res["image"]["gpu_incl_h2d_img_per_s"] = round(N / s2, 1)
    # batched: a list of images in two launches.  "kernels" = the two launches alone (descriptors prepared), the roofline
    # figure; "resident" adds the host-side planning; "incl_h2d" adds the copies of the decoded bytes
    bpi = res["image"]["bytes_per_img"]
    plan = preproc.plan_images(dev, 224, MEAN, STD, out=out)
    s = gpu_time(plan.launch, n_warm=2)
    res["image"]["batched_kernels_img_per_s"] = round(N / s, 1)
    res["image"]["batched_kernels_gb_per_s"] = round(N * bpi / s / 1e9, 1)
    res["image"]["batched_kernels_us"] = round(s * 1e6, 1)
    s = gpu_time(lambda: preproc.images_to_tensor(dev, 224, MEAN, STD, out=out))
    res["image"]["batched_resident_img_per_s"] = round(N / s, 1)
    hosts_t = [torch.from_numpy(h) for h in host]
    preproc.images_to_tensor(hosts_t, 224, MEAN, STD, out=out); torch.cuda.synchronize()
    t0 = time.perf_counter(); preproc.images_to_tensor(hosts_t, 224, MEAN, STD, out=out); torch.cuda.synchronize()
    res["image"]["batched_incl_h2d_img_per_s"] = round(N / (time.perf_counter() - t0), 1)
    sizes = [(375, 500), (500, 375), (480, 640), (333, 500), (600, 800), (256, 256), (427, 640), (768, 1024)]
    var = [torch.from_numpy(rng.integers(0, 256, (sizes[i % 8][0], sizes[i % 8][1], 3), dtype=np.uint8)).cuda() for i in range(N)]
    plan = preproc.plan_images(var, 224, MEAN, STD, out=out)
    s = gpu_time(plan.launch, n_warm=2)
    res["image"]["batched_mixed_sizes_kernels_img_per_s"] = round(N / s, 1)
    res["image"]["batched_mixed_sizes_kernels_gb_per_s"] = round((sum(v.numel() for v in var) + N * 3 * 224 * 224 * 4) / s / 1e9, 1)
    try:
        from PIL import Image
        torch.set_num_threads(1)
        n_cpu = 64
        pil = [Image.fromarray(h) for h in host[:n_cpu]]
        m, sd = torch.as_tensor(MEAN)[:, None, None], torch.as_tensor(STD)[:, None, None]
        t0 = time.perf_counter()
        for im in pil:
            nh, nw = preproc.resized_output_size(H, W, 224)
            top, left = preproc.center_crop_origin(nh, nw, 224)
            r = im.resize((nw, nh), Image.BICUBIC).crop((left, top, left + 224, top + 224)).convert("RGB")
            torch.from_numpy(np.array(r)).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(m).div_(sd)
        res["image"]["cpu_1thread_img_per_s"] = round(n_cpu / (time.perf_counter() - t0), 1)
    except ImportError:
        pass
    # disparity maps (SUN RGB-D typical 530 x 730)
    Nd, Hd, Wd = 128, 530, 730
    d_host = [torch.rand(Hd, Wd) * 80 for _ in range(Nd)]
    d_dev = [d.cuda() for d in d_host]
    proc = DepthProcessorEval()
    outd = torch.empty(Nd, 1, 224, 224, device="cuda")
    s = gpu_time(lambda: [proc(d, out=outd[i]) for i, d in enumerate(d_dev)])
    res["depth"] = {"n": Nd, "in": [Hd, Wd], "gpu_resident_maps_per_s": round(Nd / s, 1), "gpu_resident_us_per_map": round(s / Nd * 1e6, 2)}
    n_cpu = 32
    t0 = time.perf_counter()
    for d in d_host[:n_cpu]:
        x = d.clamp(min=0.01).clamp(max=75.0) / 75
        nh, nw = preproc.resized_output_size(Hd, Wd, 224)
        r = torch.nn.functional.interpolate(x[None, None], (nh, nw), mode="bicubic", align_corners=False, antialias=True)[0, 0]
        top, left = preproc.center_crop_origin(nh, nw, 224)
        (r[top:top + 224, left:left + 224] - 0.0418) / 0.0295
    res["depth"]["cpu_1thread_maps_per_s"] = round(n_cpu / (time.perf_counter() - t0), 1)
    # point clouds: 10000 -> 8192 FPS + unit sphere (the 3D recipe's loader)
    from open_clip.modal_3d.processors.pc_processor import PCProcessorEval
    B = 32
    pcs = torch.randn(B, 10000, 3).cuda()
    pp = PCProcessorEval(npoint=8192, uniform=True)
    start = np.zeros(B, dtype=np.int64)
    s = gpu_time(lambda: pp.process_batch(pcs, start=start))
    res["pc"] = {"n": B, "in": [10000, 3], "npoint": 8192, "gpu_resident_clouds_per_s": round(B / s, 1)}
    res["pc_train"] = pc_train_row()
    res["rgbd_train"] = rgbd_train_row()
    res["image_train"] = image_train_row()
    res["tactile_train"] = tactile_train_row()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
