"""The plain-image training transform as the product runs it (vl_image_augment: two resampling launches, then one workgroup
per sample for the ops and the float tail) beside the launch-per-op baseline of tools/image_aug_split_probe.hip, on one plan
(B = 1 024 samples of 480 x 640 -> 224, the recipe's num_ops = 2 and magnitude = 9, sources resident): the two are alternated
in one process, 5 rounds of 10 calls between device events, and their outputs compared (bytes equal, floats to rounding).
Prints one JSON line.
Build first: tools/build_image_aug_split_probe.sh."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vit-lens_amd"), os.path.join(ROOT, "tests")]

import image_augment_ref as A  # noqa: E402
from open_clip.modal_tactile.processors.tact_processor import Image_Processor_Train  # noqa: E402
from vitlens_hip import _lib, ops, preproc  # noqa: E402


def main(B=1024, H=480, W=640, distinct=64, rounds=5, reps=10):
    P, I = ctypes.c_void_p, ctypes.c_int
    probe = ctypes.CDLL(os.path.join(ROOT, "tools", "bin", "libimage_aug_split.so"))
    probe.probe_image_augment_split.argtypes = [P, I, I, I, I, P, P, P, P, P, P, P, P, P]
    probe.probe_split_stat_bytes.argtypes, probe.probe_split_stat_bytes.restype = [I], ctypes.c_long
    lib = _lib.load_library()
    src = [torch.from_numpy(A.source(H, W, "random", seed=200 + i)).cuda() for i in range(distinct)]
    proc = Image_Processor_Train.from_config()
    S = proc.size
    torch.manual_seed(0)
    draws = [proc.draw(H, W) for _ in range(B)]
    plan = preproc.plan_image_train([src[i % distinct] for i in range(B)], draws, S, proc.mean, proc.std)
    work = torch.empty(2, B, S, S, 3, device="cuda", dtype=torch.uint8)
    stat = torch.empty(probe.probe_split_stat_bytes(B), device="cuda", dtype=torch.uint8)
    outs = {k: (torch.full((B, 3, S, S), float("nan"), device="cuda"), torch.full((B, S, S, 3), 0xA5, device="cuda", dtype=torch.uint8))
            for k in ("fused", "split")}
    fl = lambda v: (ctypes.c_float * 3)(*v)
    head = (ops._p(plan.records), B, S, plan.max_nrows, plan.max_ops, ops._p(plan.tables), ops._p(plan.tmp), ops._p(work))

    def call(k):
        o, u = outs[k]
        tail = (fl(proc.mean), fl(proc.std), ops._p(o), ops._p(u), ops._stream())
        rc = lib.vl_image_augment(*head, *tail) if k == "fused" else probe.probe_image_augment_split(*head, ops._p(stat), *tail)
        assert rc == 0, k

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / reps, 3)
    for k in outs:
        call(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in outs}
    for _ in range(rounds):
        for k in outs:
            ms[k].append(timed(k))
    # The bytes must be the same.  The float tail is compiled twice, into two different kernels, under the default contraction:
    # which products and sums become an fma may differ between them, so the floats agree to rounding, not bit for bit.  Bound:
    # 4 e32 of the S = 224 tail (tests/test_hip_image_augment.py: e32 = 1.87e-6 is the float32 restatement's distance from float64).
    bytes_equal = bool(torch.equal(outs["fused"][1], outs["split"][1]))
    float_diff = float((outs["fused"][0] - outs["split"][0]).abs().max())
    ok = bytes_equal and float_diff <= 4 * 1.87e-6
    print(json.dumps({"image_aug_split_probe": {"n": B, "in": [H, W], "size": S, "num_ops": proc.num_ops,
                                                "launches": {"fused": 3, "split": 4 + 2 * plan.max_ops},
                                                "ms_per_batch": ms, "bytes_equal": bytes_equal, "float_max_abs_diff": float_diff}}))
    assert ok


if __name__ == "__main__":
    main()
