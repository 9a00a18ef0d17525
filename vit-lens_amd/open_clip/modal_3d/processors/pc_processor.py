"""Point-cloud preprocessing of the 3D recipe ON THE GPU (reference: open_clip/modal_3d/processors/
pc_processor.py - numpy on the data-loader workers): `uniform` farthest-point sampling of a raw cloud down to `npoint`
points (:8-29), or a random subset (:41-45), then centring and scaling into the unit sphere (`pc_norm`, :32-38).

Same class name, constructor and call convention as the reference's `PCProcessorEval`; the result lives on the GPU
(a [npoint, C] f32 tensor), where the PointBERT tokenizer consumes it.  FPS runs in `vl_fps` (the kernel of the tokenizer,
bit-exact fp32 distances, lowest index on ties like np.argmax), the rest in `vl_pc_gather_normalize`.  The random choices
(FPS start, random subset) are drawn on the host with numpy exactly where the reference draws them, so a seeded
`np.random` reproduces the reference's sample."""
import numpy as np
import torch


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


def _as_device_f32(pc, device):
    t = torch.from_numpy(np.ascontiguousarray(pc)) if isinstance(pc, np.ndarray) else pc
    return t.to(device=device, dtype=torch.float32, non_blocking=True).contiguous()


class PCProcessorEval(BaseProcessor):
    def __init__(self, npoint, uniform, idendity=False, device="cuda"):
        self.npoint, self.uniform, self.idendity, self.device = npoint, uniform, idendity, torch.device(device)

    def process_batch(self, pcs, start=None, subset=None):
        """pcs [B, N, C] (numpy or tensor, C = 3..8, xyz first) -> [B, npoint, C] f32 on the GPU.
        start [B]: FPS start indices (default: np.random.randint per cloud, as farthest_point_sample draws it);
        subset [B, npoint]: indices of the random subset when not `uniform` (default: a numpy permutation per cloud)."""
        from vitlens_hip import ops
        x = _as_device_f32(pcs, self.device)
        B, N, C = x.shape
        if self.uniform and self.npoint < N:
            if start is None:
                start = np.array([np.random.randint(0, N) for _ in range(B)], dtype=np.int64)
            st = torch.as_tensor(np.asarray(start), dtype=torch.int64, device=self.device)
            idx, _ = ops.fps(x[:, :, :3].contiguous(), st, self.npoint, want_centers=False)
        else:
            if subset is None:
                subset = np.stack([np.random.permutation(N)[:self.npoint] for _ in range(B)])
            idx = torch.as_tensor(np.asarray(subset), dtype=torch.int64, device=self.device)
        return ops.pc_gather_normalize(x, idx)

    def __call__(self, pc):
        if self.idendity:
            return _as_device_f32(pc, self.device)
        return self.process_batch(pc[None] if isinstance(pc, np.ndarray) else pc.unsqueeze(0))[0]

    @classmethod
    def from_config(cls, cfg=None):
        cfg = cfg or {}
        return cls(npoint=cfg.get("npoint", 8192), uniform=cfg.get("uniform", True))


# bits of a record's `flags` (include/vitlens_hip.h: vl_pc_augment)
PC_NORMALIZE, PC_NORM_GUARD, PC_FEAT_FILL = 1, 2, 4
MAX_DROPOUT_RATIO = 0.875


def _rot(rows):
    """[9 entries, each [B]] -> [B, 3, 3]"""
    return np.stack(np.broadcast_arrays(*rows), axis=-1).reshape(-1, 3, 3)


def compose_affine(scale, shift, angles, final_angle, final_axis, y_up=False):
    """The reference's scale, shift, perturbation and final rotation of a sample as ONE row-vector transform
    xyz . A + t, composed in fp64 and rounded to fp32:  ((p s + shift) Rp) Rf = p (s Rp Rf) + shift Rp Rf  with
    Rp = np.dot(Rz, np.dot(Ry, Rx)) (rotate_perturbation_point_cloud) and Rf the matrix of rotate_point_cloud (final_axis "y")
    or random_rotate_z ("z") exactly as the reference writes them; `y_up` puts the y/z swap in front.
    One sample (scale, shift [3], angles [3], final_angle) -> (A [3,3] f32, t [3] f32); B samples (scale [B], shift [B,3],
    angles [B,3], final_angle [B]) -> (A [B,3,3], t [B,3]), each sample's values the same bits as alone."""
    if final_axis not in ("y", "z"):
        raise ValueError(f"final_axis must be 'y' or 'z', got {final_axis!r}")
    a = np.asarray(angles, dtype=np.float64)
    single = a.ndim == 1
    a = a.reshape(-1, 3)
    c, s = np.cos(a), np.sin(a)
    one, zero = np.ones(len(a)), np.zeros(len(a))
    Rx = _rot([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]])
    Ry = _rot([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]])
    Rz = _rot([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one])
    f = np.asarray(final_angle, dtype=np.float64).reshape(-1)
    cf, sf = np.cos(f), np.sin(f)
    Rf = _rot([cf, zero, sf, zero, one, zero, -sf, zero, cf] if final_axis == "y" else [cf, -sf, zero, sf, cf, zero, zero, zero, one])
    R = np.matmul(np.matmul(Rz, np.matmul(Ry, Rx)), Rf)
    A = np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1) * R
    if y_up:
        A = A[:, [0, 2, 1], :]                  # xyz[:, [1, 2]] = xyz[:, [2, 1]] in front: rows 1 and 2 of A change places
    t = np.matmul(np.asarray(shift, dtype=np.float64).reshape(-1, 1, 3), R)[:, 0, :]
    A, t = A.astype(np.float32), t.astype(np.float32)
    return (A[0], t[0]) if single else (A, t)


class PCProcessorTrain(BaseProcessor):
    """The training transform of the 3D recipes on the GPU: sampling as `PCProcessorEval` (`vl_fps` or a random subset), then
    ONE `vl_pc_augment` launch for normalisation, point dropout, the composed scale / shift / rotations and the colour drop.

    flavour="vitlens": the ViT-Lens datasets (open_clip/modal_3d/datasets.py:471-479, 675-683) - pc_norm (no guard), then
    random_point_dropout, random_scale_point_cloud, shift_point_cloud, rotate_perturbation_point_cloud, rotate_point_cloud
    (about y).  xyz only (C == 3), as the reference's reshape((-1, 3)) admits nothing else.
    flavour="openshape": the OpenShape loader (VitLens-OpenShape/src/data.py:74-88) - the y/z swap with `y_up`, the guarded
    normalize_pc, augment_pc, random_rotate_z (about z); feature channels are kept, or all set to 0.4 with probability
    `rgb_random_drop_prob`.

    `seed` starts the processor's own np.random.RandomState.  `draw_params()` draws one sample's scalars from it in the
    reference's order - dropout ratio random() * 0.875, [here the reference draws its N-field; a 64-bit seed of the device's
    Philox field is drawn in its place], scale uniform(0.8, 1.25), shifts uniform(-0.1, 0.1, 3), perturbation angles
    clip(0.06 randn(3), -0.18, 0.18), the final angle (uniform() 2 pi, resp. uniform(0, 2 pi)), and for "openshape" the colour
    drop's rand() - and composes them on the host (`compose_affine`).  The scalars are the reference's for a RandomState seeded
    alike up to the N-field; the per-point field is not (it never leaves the GPU).
    augment=False draws nothing: identity transform, nothing dropped (ratio -1), only sampling and normalisation.

    Out of scope: `use_height`, the extra height channel (PointNeXT only; the reference hard-codes it off, datasets.py:880), and
    jitter_point_cloud, which none of the reference's loaders calls."""

    def __init__(self, npoint, uniform, augment=True, flavour="vitlens", seed=None, device="cuda", y_up=False,
                 rgb_random_drop_prob=0.0):
        if flavour not in ("vitlens", "openshape"):
            raise ValueError(f"flavour must be 'vitlens' or 'openshape', got {flavour!r}")
        if int(npoint) < 1:
            raise ValueError(f"npoint must be positive, got {npoint}")
        if not 0.0 <= float(rgb_random_drop_prob) <= 1.0:
            raise ValueError(f"rgb_random_drop_prob must be in [0, 1], got {rgb_random_drop_prob}")
        if flavour == "vitlens" and (y_up or rgb_random_drop_prob):
            raise ValueError("y_up and rgb_random_drop_prob belong to flavour='openshape'")
        self.npoint, self.uniform, self.augment, self.flavour = int(npoint), uniform, augment, flavour
        self.device, self.y_up, self.rgb_random_drop_prob = torch.device(device), bool(y_up), float(rgb_random_drop_prob)
        self.rng = np.random.RandomState(seed)

    def _draw_scalars(self):
        """(ratio, seed, scale, shift [3], angles [3], final angle, flags) of one sample, drawn in the reference's order."""
        flags = PC_NORMALIZE | (PC_NORM_GUARD if self.flavour == "openshape" else 0)
        if not self.augment:
            return -1.0, 0, 1.0, np.zeros(3), np.zeros(3), 0.0, flags
        rng = self.rng
        ratio = rng.random_sample() * MAX_DROPOUT_RATIO
        seed = (int(rng.randint(0, 2 ** 32, dtype=np.uint64)) << 32) | int(rng.randint(0, 2 ** 32, dtype=np.uint64))
        scale = rng.uniform(0.8, 1.25, 1)[0]
        shift = rng.uniform(-0.1, 0.1, (1, 3))[0]
        angles = np.clip(0.06 * rng.randn(3), -0.18, 0.18)
        if self.flavour == "vitlens":
            final = rng.uniform() * 2 * np.pi
        else:
            final = rng.uniform(0, 2 * np.pi)
            if rng.rand() < self.rgb_random_drop_prob:
                flags |= PC_FEAT_FILL
        return ratio, seed, scale, shift, angles, final, flags

    def draw_records(self, B):
        """B samples' records as one PC_AUGMENT_DTYPE array: the scalars drawn sample by sample, composed together."""
        from vitlens_hip.ops import PC_AUGMENT_DTYPE
        d = [self._draw_scalars() for _ in range(B)]
        rec = np.zeros(B, dtype=PC_AUGMENT_DTYPE)
        A, t = compose_affine(np.array([r[2] for r in d]), np.array([r[3] for r in d]).reshape(B, 3),
                              np.array([r[4] for r in d]).reshape(B, 3), np.array([r[5] for r in d]),
                              "y" if self.flavour == "vitlens" else "z", self.y_up)
        rec["A"], rec["t"] = A.reshape(B, 9), t
        rec["drop_ratio"] = np.array([r[0] for r in d], dtype=np.float32)
        rec["flags"] = [r[6] for r in d]
        rec["seed"] = np.array([r[1] for r in d], dtype=np.uint64)
        return rec

    def draw_params(self):
        """(A[9], t[3], drop_ratio, flags, seed) of one sample: a record of `vitlens_hip.ops.PC_AUGMENT_DTYPE` as a tuple."""
        r = self.draw_records(1)[0]
        return tuple(r["A"].tolist()), tuple(r["t"].tolist()), float(r["drop_ratio"]), int(r["flags"]), int(r["seed"])

    def process_batch(self, pcs, start=None, subset=None, params=None):
        """pcs [B, N, C] (numpy or tensor, xyz first; C == 3 for "vitlens", 3..8 for "openshape") -> [B, npoint, C] f32 on the
        GPU.  start / subset: as `PCProcessorEval.process_batch`.  params: B records (`draw_params()` tuples or a
        PC_AUGMENT_DTYPE array) instead of fresh draws - for tests, and to replay a sample."""
        from vitlens_hip import ops
        x = _as_device_f32(pcs, self.device)
        if x.dim() != 3:
            raise ValueError(f"expected clouds [B, N, C], got {tuple(x.shape)}")
        B, N, C = x.shape
        if self.flavour == "vitlens" and C != 3:
            raise ValueError(f"flavour='vitlens' takes xyz only (C == 3, as the reference's reshape((-1, 3))), got C = {C}")
        if params is None:
            params = self.draw_records(B)
        if len(params) != B:
            raise ValueError(f"{len(params)} parameter records for {B} clouds")
        if self.uniform and self.npoint < N:
            if start is None:
                start = np.array([np.random.randint(0, N) for _ in range(B)], dtype=np.int64)
            st = torch.as_tensor(np.asarray(start), dtype=torch.int64, device=self.device)
            idx, _ = ops.fps(x[:, :, :3].contiguous(), st, self.npoint, want_centers=False)
        else:
            if subset is None:
                subset = np.stack([np.random.permutation(N)[:self.npoint] for _ in range(B)])
            idx = torch.as_tensor(subset if isinstance(subset, torch.Tensor) else np.asarray(subset), dtype=torch.int64,
                                  device=self.device)
            if idx.shape != (B, self.npoint):
                raise ValueError(f"subset must be [B, npoint] = [{B}, {self.npoint}], got {tuple(idx.shape)}")
        return ops.pc_augment(x, idx, ops.pc_augment_params(params, self.device), feat_fill=0.4)

    def __call__(self, pc):
        return self.process_batch(pc[None] if isinstance(pc, np.ndarray) else pc.unsqueeze(0))[0]

    @classmethod
    def from_config(cls, cfg=None):
        cfg = cfg or {}
        return cls(npoint=cfg.get("npoint", 8192), uniform=cfg.get("uniform", True), augment=cfg.get("augment", True),
                   flavour=cfg.get("flavour", "vitlens"))
