"""CPU: the C ABI after the single-query attention entries - header, library exports, binding table and version agree, and the
three entries of this revision are there (tests/test_abi.py checks the sets against each other; this pins the revision)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vl_attn_fwd_q1", "vl_attn_bwd_q1", "vl_layernorm_bwd_sres")


def _header():
    src = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_entries_are_declared_exported_and_bound():
    from vitlens_hip import _lib
    names = set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_lib.lib_path())
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert names - {"vl_last_error"} == set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == len(names) - 1


def test_abi_version_counts_this_revision():
    from vitlens_hip import _lib
    want = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert want >= 607                          # 607 added the three entries above
    assert _lib.ABI_VERSION == want == int(_lib.load_library().vl_version())
