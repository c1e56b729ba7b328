"""tests/lds_poison from Python: every CU's LDS filled with a pattern before a kernel under test (poison_lds), and the positive
control that reads it back with a kernel that writes no LDS (peek_lds).  Test infrastructure, built by __graft_entry__.build();
importing this module needs neither the library nor a GPU -- it is loaded on first use."""
import ctypes as C
import os

import numpy as np

PATTERNS = (0xFFFFFFFF, 0x7FC00000, 0x00ABCDEF)   # all ones (a wild index, a NaN), the quiet NaN, a plausible index
BLOCKS = 2048                                     # workgroups of a poison / peek grid: a few times the CU count
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lds_poison", "_build", "liblds_poison.so")
        if not os.path.exists(so):
            import subprocess
            subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(so))], check=True)
        L = C.CDLL(so)
        L.lds_poison.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
        L.lds_peek.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.c_void_p]
        L.lds_cu_count.argtypes = [C.c_int]
        _LIB = L
    return _LIB


def poison_lds(pattern, device=0):
    """Every CU's LDS filled with `pattern`."""
    rc = lib().lds_poison(device, pattern, BLOCKS)
    assert rc == 0, rc


_poison_lds = poison_lds   # (the name tests/test_gpu_parity.py has always used)


def peek_lds(pattern, device=0):
    """What a kernel launched now finds in its LDS: {groups: workgroups of the peek grid, groups_found: those that read `pattern`
    in at least one word, word_share: the share of their words that held it, min_share / max_share: the same per workgroup over
    all of them}."""
    found, words, per = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    per_group = np.zeros(BLOCKS, np.uint32)
    rc = lib().lds_peek(device, pattern, BLOCKS, C.byref(found), C.byref(words), C.byref(per), per_group.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    share = per_group / float(per.value)
    return {"groups": BLOCKS, "groups_found": int(found.value),
            "word_share": float(words.value) / (found.value * per.value) if found.value else 0.0,
            "min_share": float(share.min()), "max_share": float(share.max())}


def cu_count(device=0):
    return lib().lds_cu_count(device)
