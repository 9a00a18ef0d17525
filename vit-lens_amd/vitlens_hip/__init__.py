"""vitlens_hip — MI355X-native kernels for the ViT-Lens contrastive hot path.

Thin Python face of libvitlens_hip.so (C ABI in include/vitlens_hip.h).  PyTorch is used
only for device memory, streams and torch.distributed; every FLOP on the hot path runs in
the hand-written HIP kernels under csrc/.  There is NO CPU or eager fallback: importing
`vitlens_hip.ops` without the built library, or calling an op on a non-GPU tensor, raises.
"""
from ._lib import lib_path, load_library, LibraryNotBuilt  # noqa: F401

__all__ = ["lib_path", "load_library", "LibraryNotBuilt", "clip_grad_norm_"]


def clip_grad_norm_(flat_or_tensors, max_norm):
    """torch.nn.utils.clip_grad_norm_(norm_type=2) on gradient TENSORS on the device (one flat f32 buffer such as a fused
    step's `flat_grad`, or the values of `reduced_grads()`), without a host read: returns the unclipped norm as a 0-d
    device tensor.  See `vitlens_hip.train.clip_grad_norm_` (imported on first use: it needs the built library)."""
    from .train import clip_grad_norm_ as impl
    return impl(flat_or_tensors, max_norm)
