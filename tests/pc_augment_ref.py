"""numpy restatement of the 3D training augmentation (helper of test_pc_augment_host.py / test_hip_pc_augment.py, no tests).

1. The reference's functions for GIVEN draws, with its dtypes and its in-place float32 / float64 behaviour
   (open_clip/modal_3d/datasets.py:97-204 and VitLens-OpenShape/src/utils/data.py): an in-place `*=` / `+=` on the float32
   batch rounds to float32, each np.dot with a float64 matrix is computed in float64 and rounded into a float32 array, and
   random_rotate_z returns float64.  test_pc_augment_host.py pins them to the recorded reference at atol = 0.
2. The legacy-RNG draws in the reference's order (`draw_reference`), the N-field of random_point_dropout included.
3. The device's per-point field u_j (Philox4x32-10, on top of philox_ref), the 64-byte record, and the host composition
   xyz . A + t of scale, shift and the rotations.
4. The pipelines in fp64 under a given mask (`sequential_f64`): what the GPU tests compare against."""
import struct

import numpy as np

from philox_ref import philox4x32_10

MAX_DROPOUT_RATIO = 0.875
NORMALIZE, NORM_GUARD, FEAT_FILL = 1, 2, 4


# ---------------------------------------------------------------------------------------------- 1. the reference, given draws
def pc_norm(pc):
    centroid = np.mean(pc, axis=0)
    pc = pc - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    return pc / m


def normalize_pc(pc):
    pc = pc - np.mean(pc, axis=0)
    if np.max(np.linalg.norm(pc, axis=1)) < 1e-6:
        return np.zeros_like(pc)
    return pc / np.max(np.linalg.norm(pc, axis=1))


def random_point_dropout(batch_pc, ratios, fields):
    """ratios [B] (already multiplied by 0.875), fields [B, N]: the draws of np.random.random() and np.random.random(N)."""
    for b in range(batch_pc.shape[0]):
        drop_idx = np.where(fields[b] <= ratios[b])[0]
        if len(drop_idx) > 0:
            batch_pc[b, drop_idx, :] = batch_pc[b, 0, :]
    return batch_pc


def random_scale_point_cloud(batch_data, scales):
    for b in range(batch_data.shape[0]):
        batch_data[b, :, :] *= scales[b]
    return batch_data


def shift_point_cloud(batch_data, shifts):
    for b in range(batch_data.shape[0]):
        batch_data[b, :, :] += shifts[b, :]
    return batch_data


def perturbation_matrix(angles):
    Rx = np.array([[1, 0, 0], [0, np.cos(angles[0]), -np.sin(angles[0])], [0, np.sin(angles[0]), np.cos(angles[0])]])
    Ry = np.array([[np.cos(angles[1]), 0, np.sin(angles[1])], [0, 1, 0], [-np.sin(angles[1]), 0, np.cos(angles[1])]])
    Rz = np.array([[np.cos(angles[2]), -np.sin(angles[2]), 0], [np.sin(angles[2]), np.cos(angles[2]), 0], [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


def rotate_perturbation_point_cloud(batch_data, angles):
    """angles [B, 3]: np.clip(0.06 * np.random.randn(3), -0.18, 0.18) per cloud."""
    rotated = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        rotated[k, ...] = np.dot(batch_data[k, ...].reshape((-1, 3)), perturbation_matrix(angles[k]))
    return rotated


def y_matrix(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def z_matrix(theta):
    return np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])


def rotate_point_cloud(batch_data, angles):
    """angles [B]: np.random.uniform() * 2 * np.pi per cloud."""
    rotated = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        rotated[k, ...] = np.dot(batch_data[k, ...].reshape((-1, 3)), y_matrix(angles[k]))
    return rotated


def random_rotate_z(pc, theta):
    return np.matmul(pc, z_matrix(theta))


def vitlens_pipeline(pc, d):
    """datasets.py:471-479 after pc_norm; `pc` is modified in place as there.  d: a dict of `draw_reference`."""
    pc = random_point_dropout(pc[None, ...], [d["ratio"]], [d["field"]])
    pc = random_scale_point_cloud(pc, d["scale"])
    pc = shift_point_cloud(pc, d["shift"])
    pc = rotate_perturbation_point_cloud(pc, [d["angles"]])
    pc = rotate_point_cloud(pc, [d["final"]])
    return pc.squeeze()


def openshape_pipeline(xyz, d):
    """augment_pc + random_rotate_z (src/data.py:79-82) after normalize_pc."""
    pc = random_point_dropout(xyz[None, ...], [d["ratio"]], [d["field"]])
    pc = random_scale_point_cloud(pc, d["scale"])
    pc = shift_point_cloud(pc, d["shift"])
    pc = rotate_perturbation_point_cloud(pc, [d["angles"]])
    return random_rotate_z(pc.squeeze(), d["final"])


# ---------------------------------------------------------------------------------------------- 2. the draws, in order
def draw_reference(n, flavour, rng=np.random):
    """One cloud's draws from the legacy generator in the order the reference makes them."""
    d = {"ratio": rng.random() * MAX_DROPOUT_RATIO}
    d["field"] = rng.random((n))
    d["scale"] = rng.uniform(0.8, 1.25, 1)
    d["shift"] = rng.uniform(-0.1, 0.1, (1, 3))
    d["angles"] = np.clip(0.06 * rng.randn(3), -0.18, 0.18)
    d["final"] = rng.uniform() * 2 * np.pi if flavour == "vitlens" else rng.uniform(0, 2 * np.pi)
    return d


# ---------------------------------------------------------------------------------------------- 3. field, record, composition
def dropout_field(seed, G):
    """u [G] float32 in [0, 1): word j % 4 of Philox4x32-10, key (lo32(seed), hi32(seed)), counter (j / 4, 0, 0, 0)."""
    groups = (G + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    z = np.zeros(groups, dtype=np.uint64)
    words = np.stack(philox4x32_10(g, z, z, z, seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)[:G]
    return (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def drop_mask(seed, G, ratio):
    return dropout_field(seed, G) <= np.float32(ratio)


def pack_record(A, t, ratio, flags, seed):
    """The 64 bytes of one sample: 9 + 3 + 1 floats, an int32 and a uint64, little-endian."""
    return struct.pack("<13fiQ", *[float(v) for v in np.asarray(A).reshape(-1)], *[float(v) for v in t], float(ratio), int(flags), int(seed))


def compose(scale, shift, angles, final, axis, y_up=False):
    """((p s + shift) Rp) Rf = p (s Rp Rf) + shift Rp Rf in fp64 -> (A [3,3], t [3]) rounded to fp32."""
    R = np.dot(perturbation_matrix(np.asarray(angles, dtype=np.float64)), y_matrix(final) if axis == "y" else z_matrix(final))
    A = float(scale) * R
    if y_up:
        swap = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=np.float64)
        A = swap @ A
    return A.astype(np.float32), np.dot(np.asarray(shift, dtype=np.float64).reshape(3), R).astype(np.float32)


def record(scale, shift, angles, final, axis, ratio, flags, seed, y_up=False):
    """A parameter record as PCProcessorTrain.process_batch(params=...) and ops.pc_augment_params take it."""
    A, t = compose(scale, shift, angles, final, axis, y_up)
    return tuple(A.reshape(-1).tolist()), tuple(t.tolist()), float(ratio), int(flags), int(seed)


def apply_composed_f32(xyz, A, t):
    """xyz . A + t as the kernel evaluates it: fma(x, A[0,c], fma(y, A[1,c], fma(z, A[2,c], t[c]))), every FMA rounded once
    (the exact fp64 product-sum of fp32 operands rounded to fp32 differs from a hardware FMA only by double rounding, far
    below what the tests resolve)."""
    x = xyz.astype(np.float32)
    acc = np.broadcast_to(t.astype(np.float32), x.shape).copy()
    for r in (2, 1, 0):
        acc = (x[:, r:r + 1].astype(np.float64) * A[r].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------- 4. fp64 under a given mask
def normalize_f64(xyz, guard):
    p = xyz.astype(np.float64)
    p = p - p.mean(axis=0)
    m = np.sqrt((p ** 2).sum(axis=1)).max()
    if guard and m < 1e-6:
        return np.zeros_like(p)
    return p / m


def sequential_f64(xyz, mask, scale, shift, angles, final, axis):
    """The reference's sequence in fp64 on already normalised (or raw) points, dropping the points of `mask`."""
    p = xyz.astype(np.float64).copy()
    if mask.any():
        p[mask] = p[0]
    p = p * float(scale)
    p = p + np.asarray(shift, dtype=np.float64).reshape(1, 3)
    p = np.dot(p, perturbation_matrix(np.asarray(angles, dtype=np.float64)))
    return np.dot(p, y_matrix(final) if axis == "y" else z_matrix(final))
