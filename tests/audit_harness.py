"""ctypes wrapper of tests/native/audit_poke.hip (built by `make probe` into tests/native/_bin/libaudit_poke.so): the graph rows of a
pyhvx index as the device holds them, and single-slot writes into them.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
POKE_LIB = os.path.join(HERE, "native", "_bin", "libaudit_poke.so")
HEADER = ("n", "s0", "su", "up_rows", "cap_rows", "cap_up_rows", "entry", "has_entry", "max_layer", "m", "m0", "has_dead")
_lib = None


def poke_lib():
    global _lib
    if _lib is None:
        import pyhvx
        pyhvx.lib()  # the product library (and the HIP runtime the process is bound to) first
        if not os.path.exists(POKE_LIB):
            raise RuntimeError(f"{POKE_LIB} is missing: run `make probe` in helix-db_amd/csrc (build() does)")
        L = C.CDLL(POKE_LIB)
        L.audit_poke_dump.restype = C.c_int
        L.audit_poke_dump.argtypes = [C.c_void_p] * 7
        L.audit_poke_write.restype = C.c_int
        L.audit_poke_write.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dump(gix):
    """the `raw` image tests/audit_twin.py audits, plus cap_rows / cap_up_rows"""
    L = poke_lib()
    hdr = np.zeros(len(HEADER), np.uint32)
    rc = L.audit_poke_dump(gix._h, _p(hdr), None, None, None, None, None)
    assert rc == 0, f"audit_poke_dump (sizes): {rc}"
    h = {k: int(v) for k, v in zip(HEADER, hdr)}
    n = h["n"]
    l0 = np.zeros((n, h["s0"]), np.uint32)
    up = np.zeros((h["up_rows"], h["su"]), np.uint32)
    level = np.zeros(n, np.uint16)
    up_base = np.zeros(n, np.uint32)
    dead = np.zeros((n + 31) // 32, np.uint32) if h["has_dead"] else None
    rc = L.audit_poke_dump(gix._h, _p(hdr), _p(l0), _p(up), _p(level), _p(up_base), _p(dead))
    assert rc == 0, f"audit_poke_dump: {rc}"
    assert {k: int(v) for k, v in zip(HEADER, hdr)} == h
    raw = {k: h[k] for k in ("n", "s0", "su", "entry", "has_entry", "max_layer", "m", "m0", "cap_rows", "cap_up_rows")}
    raw.update(l0=l0, up=up, level=level, up_base=up_base, dead=dead)
    return raw


def write(gix, upper, row, slot, value):
    rc = poke_lib().audit_poke_write(gix._h, 1 if upper else 0, int(row), int(slot), int(value) & 0xFFFFFFFF)
    assert rc == 0, f"audit_poke_write(upper={upper}, row={row}, slot={slot}): {rc}"


def write_row(gix, upper, row, ids, stride):
    """a whole row: `ids` as given, then sentinels"""
    ids = list(ids)
    assert len(ids) <= stride
    for slot in range(stride):
        write(gix, upper, row, slot, ids[slot] if slot < len(ids) else 0xFFFFFFFF)


def csr_of(raw):
    """the rows of a dump in export_graph()'s CSR layout (internal ids = row numbers), for the layout gate"""
    def pack(rows):
        lens = [int((r != 0xFFFFFFFF).sum()) for r in rows]
        off = np.zeros(len(rows) + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        nb = np.concatenate([r[r != 0xFFFFFFFF] for r in rows]).astype(np.uint64) if len(rows) else np.zeros(0, np.uint64)
        return off, nb
    l0o, l0n = pack(list(raw["l0"]))
    upo, upn = pack(list(raw["up"]))
    return {"l0_offsets": l0o, "l0_neighbors": l0n, "level": raw["level"].copy(), "up_offsets": upo, "up_neighbors": upn}
