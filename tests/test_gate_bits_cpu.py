"""CPU-only checks of the bit-packed ReLU gate entries (tg_relu_gate_pack, tg_conv_dgrad_gbits): declared, bound and exported,
and their host-side validation rejects bad arguments before any launch (so it runs without a GPU)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tg_relu_gate_pack", "tg_conv_dgrad_gbits")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    return L, L.load()


def test_new_symbols_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "terragan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L, lib = _lib()
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", txt), f"{s} not declared in terragan_hip.h"
        assert s in L.SIGNATURES, f"{s} has no ctypes signature"
        assert hasattr(lib, s), f"{s} not exported by the library"


def test_relu_gate_pack_validation():
    _L, lib = _lib()
    fake = C.c_void_p(1 << 20)                  # never dereferenced: validation fails first
    rc = lib.tg_relu_gate_pack(fake, 7, 48, fake, None)
    assert rc == -1 and b"C % 32" in lib.tg_last_error()
    rc = lib.tg_relu_gate_pack(None, 7, 64, fake, None)
    assert rc == -1 and b"null pointer" in lib.tg_last_error()
    rc = lib.tg_relu_gate_pack(fake, 7, 64, None, None)
    assert rc == -1 and b"null pointer" in lib.tg_last_error()
    rc = lib.tg_relu_gate_pack(fake, 0, 64, fake, None)
    assert rc == -1


def test_conv_dgrad_gbits_validation():
    L, lib = _lib()
    fake = C.c_void_p(1 << 20)
    ws = 1 << 20
    good = L.TgConv(1, 16, 16, 64, 16, 16, 64, 3, 1, 1, 0)
    # Cin % 32 != 0
    g48 = L.TgConv(1, 16, 16, 48, 16, 16, 64, 3, 1, 1, 0)
    rc = lib.tg_conv_dgrad_gbits(C.byref(g48), fake, fake, None, None, fake, fake, 0, fake, ws, None)
    assert rc == -1 and b"Cin % 32" in lib.tg_last_error()
    # null pointers: dy, w, gate_bits, dx, ws
    for i in range(5):
        args = [fake] * 5
        args[i] = None
        dy, w, bits, dx, wsp = args
        rc = lib.tg_conv_dgrad_gbits(C.byref(good), dy, w, None, None, bits, dx, 0, wsp, ws, None)
        assert rc == -1 and b"null pointer" in lib.tg_last_error(), i
    # inconsistent sizes (Ho / Wo do not follow from H, W, k, stride, pad)
    bad = L.TgConv(1, 16, 16, 64, 15, 16, 64, 3, 1, 1, 0)
    rc = lib.tg_conv_dgrad_gbits(C.byref(bad), fake, fake, None, None, fake, fake, 0, fake, ws, None)
    assert rc == -1 and b"inconsistent" in lib.tg_last_error()
    rc = lib.tg_conv_dgrad_gbits(None, fake, fake, None, None, fake, fake, 0, fake, ws, None)
    assert rc == -1
    # a gated dgrad does not accumulate
    rc = lib.tg_conv_dgrad_gbits(C.byref(good), fake, fake, None, None, fake, fake, 1, fake, ws, None)
    assert rc == -1 and b"accumulate" in lib.tg_last_error()
