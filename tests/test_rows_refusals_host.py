"""CPU: what the row-wise entries refuse BEFORE any launch (include/vitlens_hip.h: vl_layernorm_fwd, vl_assemble_ln_pre,
vl_assemble_ln_pre_keep, vl_add_rows, vl_text_embed, vl_layernorm_bwd_g, vl_layernorm_bwd_sres) - a dtype code they have no
kernel for, and one of mean / rstd without the other.  The entries are called through ctypes with dummy non-null pointers that
nothing may dereference: only argument sets that must be refused are ever passed, on any machine."""
import ctypes as C
import itertools

import pytest
import torch

F32, BF16, F16 = 0, 1, 2
CODES = (F32, BF16, F16, 3, -1)
LN_PAIRS = {(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16)}       # (input, output) pairs with a kernel


def _lib():
    from vitlens_hip import _lib
    return _lib.load_library()


def ptr(i):
    """A distinct, 16-byte aligned, non-null address per operand; never read or written."""
    return C.c_void_p(0x10000 * (i + 1))


def refused(status, entry, *words):
    msg = _lib().vl_last_error().decode()
    assert status != 0, f"{entry} accepted arguments it has no kernel for"
    assert msg.startswith(entry.split("|")[0]) and all(w in msg for w in words), msg


def _ln_fwd(x_dt, y_dt, mean, rstd):
    return _lib().vl_layernorm_fwd(ptr(0), x_dt, 256, None, 0, ptr(1), ptr(2), ptr(3), y_dt, 256, mean, rstd, 4, 256, 1e-5, None)


def _assemble(x_dt, y_dt, mean, rstd):
    return _lib().vl_assemble_ln_pre(ptr(0), x_dt, ptr(1), ptr(2), None, ptr(3), ptr(4), ptr(5), y_dt, None, mean, rstd,
                                     2, 3, 256, 1e-5, None)


def _assemble_keep(x_dt, y_dt, mean, rstd):
    return _lib().vl_assemble_ln_pre_keep(ptr(0), x_dt, ptr(6), ptr(1), ptr(2), None, ptr(3), ptr(4), ptr(5), y_dt, None, mean,
                                          rstd, 2, 3, 2, 256, 1e-5, None)


LN_ENTRIES = [("vl_layernorm_fwd", _ln_fwd), ("vl_assemble_ln_pre", _assemble), ("vl_assemble_ln_pre_keep", _assemble_keep)]


@pytest.mark.parametrize("entry,call", LN_ENTRIES, ids=[e for e, _ in LN_ENTRIES])
def test_layernorm_forward_entries_refuse_dtype_pairs_without_a_kernel(entry, call):
    """bf16 -> f16 was sent to the bf16 -> f32 kernel (4-byte stores into a 2-byte buffer), like every unknown code."""
    bad = [p for p in itertools.product(CODES, CODES) if p not in LN_PAIRS]
    assert (BF16, F16) in bad and len(bad) == 20
    for x_dt, y_dt in bad:
        refused(call(x_dt, y_dt, None, None), entry, "dtype")
        refused(call(x_dt, y_dt, ptr(7), ptr(8)), entry, "dtype")


@pytest.mark.parametrize("entry,call", LN_ENTRIES, ids=[e for e, _ in LN_ENTRIES])
def test_layernorm_forward_entries_refuse_mean_without_rstd(entry, call):
    """The kernel stores rstd[row] whenever mean is set: `mean` alone was a store through a null pointer."""
    for x_dt, y_dt in sorted(LN_PAIRS):
        refused(call(x_dt, y_dt, ptr(7), None), entry, "mean", "rstd")
        refused(call(x_dt, y_dt, None, ptr(8)), entry, "mean", "rstd")


def test_wrappers_raise_value_error_for_mean_without_rstd_before_any_library_call():
    from launch_trace import recording
    from vitlens_hip import ops
    D = 256
    x = torch.zeros(4, D); w = torch.ones(D); b = torch.zeros(D); y = torch.empty(4, D); m = torch.empty(4)
    tok = torch.zeros(2, 1, D); pos = torch.zeros(2, D); keep = torch.zeros(2, 1, dtype=torch.int32)
    for kw in ({"mean": m}, {"rstd": m}):
        with recording() as trace:
            with pytest.raises(ValueError, match="mean and rstd"):
                ops.layernorm(x, w, b, y, 4, D, **kw)
            with pytest.raises(ValueError, match="mean and rstd"):
                ops.assemble_ln_pre(tok, w, pos, None, w, b, y, 2, 1, D, **kw)
            with pytest.raises(ValueError, match="mean and rstd"):
                ops.assemble_ln_pre_keep(tok, keep, w, pos, None, w, b, y, 2, 1, D, **kw)
        assert trace == []
    with recording() as trace:                      # both or neither: one launch each
        ops.layernorm(x, w, b, y, 4, D, mean=m, rstd=m.clone())
        ops.layernorm(x, w, b, y, 4, D)
    assert [n for n, _ in trace] == ["vl_layernorm_fwd"] * 2


def test_add_rows_and_text_embed_refuse_dtype_codes_without_a_kernel():
    """VL_F16 was read as bf16 by both."""
    lib = _lib()
    for x_dt, y_dt in itertools.product(CODES, CODES):
        if x_dt in (F32, BF16) and y_dt in (F32, BF16):
            continue
        refused(lib.vl_add_rows(ptr(0), x_dt, ptr(1), ptr(2), y_dt, 16, 5, 72, None), "vl_add_rows", "dtype")
    for dt in (F16, 3, -1):
        refused(lib.vl_text_embed(ptr(0), ptr(1), ptr(2), ptr(3), dt, 2, 3, 72, 50, None), "vl_text_embed", "dtype")


def test_layernorm_backward_entries_refuse_dtype_codes_without_a_kernel():
    """VL_F16 in any of the three positions was read as fp32."""
    lib = _lib()
    ok = (F32, BF16)
    n = 0
    for dy_dt, x_dt, g_dt in itertools.product(CODES, CODES, CODES):
        if dy_dt in ok and x_dt in ok and g_dt in ok:
            continue
        n += 1
        refused(lib.vl_layernorm_bwd_g(ptr(0), dy_dt, 256, ptr(1), x_dt, 256, ptr(2), ptr(3), ptr(4), None, ptr(5), g_dt, None,
                                       256, 4, 256, None), "vl_layernorm_bwd", "dtype")
        refused(lib.vl_layernorm_bwd_sres(ptr(0), dy_dt, 256, ptr(1), x_dt, 256, ptr(2), ptr(3), ptr(4), ptr(6), 2, 256, ptr(5),
                                          g_dt, None, 256, 4, 256, None), "vl_layernorm_bwd", "dtype")
    assert n == 125 - 8
