"""Records the library launches of a forward / backward that runs on CPU tensors instead of executing them: which kernels a
host-side plan (engine.run_blocks / block_forward in any arithmetic, engine.text_features, VitEngine.trunk, TowerTrainer.forward /
backward, TextEngine.encode_text, perceiver_forward ...) enqueues, in which order and
with which arguments - without a GPU.

    with recording() as trace:
        eng.trunk(tokens, B)
    symbols(trace)            # ["vl_assemble_ln_pre", "vl_ln_row_stats", ...]
    normalised(trace)         # comparable between two runs that allocate elsewhere

`ops._lib` becomes a proxy that appends (symbol, arguments) for every call and reports success; the pure host functions
(vl_gemm_main_rows, the *_ws_floats ...) go to the real library, so the row splits the plans branch on are the real ones.
`ops._p` accepts CPU tensors, `ops._stream` and `torch.cuda.current_stream` are stubs.  The tensors' contents are whatever
`torch.empty` left: only the plan is meaningful."""
import contextlib
import ctypes

import torch

HOST_FUNCTIONS = ("vl_version", "vl_last_error", "vl_gemm_main_rows", "vl_gemm_rest_cfg", "vl_attn_bwd_fused_supported")


class Ptr:
    """A pointer argument: the tensor (kept alive, so that no two buffers of a trace share an address) and where it points."""

    def __init__(self, t):
        self.t = t
        self.base = t.untyped_storage().data_ptr()
        self.offset = t.data_ptr() - self.base


class _Stream:
    """What the wrappers read of the current stream."""
    cuda_stream = 0


class _Recorder:
    def __init__(self, real, trace):
        self._real, self._trace = real, trace

    def __getattr__(self, name):
        if name in HOST_FUNCTIONS or name.endswith("_ws_floats"):
            return getattr(self._real, name)

        def launch(*args):
            self._trace.append((name, args))
            return 0
        return launch


@contextlib.contextmanager
def recording():
    from vitlens_hip import ops
    trace = []
    saved = (ops._lib, ops._p, ops._stream, torch.cuda.current_stream)
    ops._lib = _Recorder(saved[0], trace)
    ops._p = lambda t: None if t is None else Ptr(t)
    ops._stream = lambda: "stream"
    torch.cuda.current_stream = lambda device=None: _Stream()
    try:
        yield trace
    finally:
        ops._lib, ops._p, ops._stream, torch.cuda.current_stream = saved


def symbols(trace):
    return [name for name, _ in trace]


def normalised(trace):
    """[(symbol, arguments)] with every pointer as (buffer numbered by first appearance in the trace, byte offset from that
    buffer's storage base): two runs that allocate elsewhere compare equal, and aliasing is part of what is compared."""
    number = {}
    out = []
    for name, args in trace:
        row = []
        for a in args:
            if isinstance(a, Ptr):
                row.append(("ptr", number.setdefault(a.base, len(number)), a.offset))
            elif isinstance(a, ctypes.Array):
                row.append(tuple(a))
            else:
                row.append(a)
        out.append((name, tuple(row)))
    return out


# what a trainer's launch may differ in from the engine's: the optional outputs it saves for the backward (argument indices of
# mean / rstd, lse, out2) and the activation code (the same activation with its derivative saved)
OPTIONAL_OUTPUTS = {"vl_layernorm_fwd": (10, 11), "vl_attn_fwd_bf16": (5,), "vl_attn_fwd_q1": (6,), "vl_gemm_bf16_ex": (5,),
                    "vl_gemm_lnfold_bf16": (7,)}
ACT_ARGUMENT = {"vl_gemm_bf16_ex": 14, "vl_gemm_lnfold_bf16": 14}


def shape_of(call):
    """A launch without its buffers: the symbol, every scalar, and of a pointer only whether it is there and its offset."""
    from vitlens_hip import ops
    plain_act = {ops.ACT_GELU_DSAVE: ops.ACT_GELU, ops.ACT_QGELU_DSAVE: ops.ACT_QGELU}
    name, args = call
    out = [name]
    for i, a in enumerate(args):
        if i in OPTIONAL_OUTPUTS.get(name, ()):
            continue
        if i == ACT_ARGUMENT.get(name):
            a = plain_act.get(a, a)
        out.append(("ptr", a.offset) if isinstance(a, Ptr) else (tuple(a) if hasattr(a, "_length_") else a))
    return tuple(out)
