"""tests/x25519_model.py, the CPU model of wg_x25519_batch / wg_hs_dh, against RFC 7748's known answers; its
restatement of the batch call's bounds and of wg_hs_dh; the ctypes layouts against the header; the bound
symbols; the no-device failure path. No GPU compute here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hs_model as HM
import x25519_model as M
from wgtest import ROOT, noise, wg

H = bytes.fromhex
# RFC 7748 5.2
K1, U1 = H("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"), \
    H("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
R1 = "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
K2, U2 = H("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d"), \
    H("e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493")
R2 = "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"
ITER_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
ITER_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
# RFC 7748 6.1
ALICE = H("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
ALICE_PUB = "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
BOB = H("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
BOB_PUB = "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
SHARED = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
# the points of order 8 on Curve25519 (u coordinates below p)
ORDER8 = [325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823]


def le(x: int) -> bytes:
    return (x % (1 << 256)).to_bytes(32, "little")


# ---- known answers ---------------------------------------------------------------------------------
def test_model_rfc7748_section_5_2_vectors():
    assert M.x25519(K1, U1).hex() == R1
    assert M.x25519(K2, U2).hex() == R2


def test_model_rfc7748_iterated_vector():
    k = u = M.BASE_POINT
    for it in range(1000):
        k, u = M.x25519(k, u), k
        if it == 0:
            assert k.hex() == ITER_1
    assert k.hex() == ITER_1000


def test_model_rfc7748_section_6_1_diffie_hellman():
    assert M.public_key(ALICE).hex() == ALICE_PUB and M.public_key(BOB).hex() == BOB_PUB
    assert M.x25519(ALICE, H(BOB_PUB)).hex() == SHARED == M.x25519(BOB, H(ALICE_PUB)).hex()


def test_model_clamp_bit_255_and_low_order_points():
    assert M.x25519(ALICE, le(9 + (1 << 255))) == M.public_key(ALICE)      # bit 255 of u is ignored
    assert M.x25519(ALICE, le((1 << 255) - 1)) == M.x25519(ALICE, le(18))  # a non-canonical u is reduced
    for sc in (ALICE, bytes(32), b"\xff" * 32):
        assert M.x25519(sc, U1) == M.x25519(M.clamp(sc), U1)
    for u in [0, 1, M.P - 1, M.P, M.P + 1] + ORDER8:
        assert M.x25519(ALICE, le(u)) == bytes(32), u


# ---- the batch call and wg_hs_dh, restated ---------------------------------------------------------------
def test_model_batch_bounds_flags_and_untouched_output():
    inp = K1 + U1 + ALICE + bytes(32)  # 128 bytes; [96, 128) is the point 0
    d = np.zeros(10, M.X25519_DESC)
    d[0] = (0, 32, 1, 0, 0)                  # OK
    d[1] = (64, 1 << 63, 40, M.X_BASE, 0)    # BASE: point_off is ignored
    d[2] = (64, 96, 80, 0, 0)                # ZERO: written
    d[3] = (97, 32, 120, 0, 0)               # scalar one byte past the buffer
    d[4] = (0, 97, 120, 0, 0)                # point one byte past the buffer
    d[5] = (0, 32, 169, 0, 0)                # output one byte past the buffer
    d[6] = (129, 32, 120, 0, 0)              # off > size
    d[7] = (0, 32, 120, 2, 0)                # unknown flag
    d[8] = (0, 32, 120, 0, 1)                # _pad
    d[9] = (96, 0, 168, 0, 0)                # ranges that end exactly at the end of their buffer
    out, st = M.batch(d, inp, b"\x5a" * 200)
    assert st == [0, 0, 2, 1, 1, 1, 1, 1, 1, 0]
    assert out[1:33].hex() == R1 and out[40:72].hex() == ALICE_PUB and out[80:112] == bytes(32)
    assert out[168:200] == M.x25519(bytes(32), K1)
    assert out[0:1] + out[33:40] + out[72:80] + out[112:168] == b"\x5a" * (1 + 7 + 8 + 56)


def test_model_hs_dh():
    pub = M.public_key(ALICE)
    rec = np.zeros(5, HM.HS_RECORD)
    msgs = [HM.message(1, bytes(7) + H(BOB_PUB) + bytes(range(76)), pub), HM.message(2, bytes(59), pub),
            HM.message(1, bytes(7) + le(1) + bytes(76), pub)]
    for k, m in enumerate(msgs):
        rec[k] = (k, len(m), np.frombuffer(m.ljust(148, b"\0"), np.uint8), 0)
    rec[3] = (3, 100, np.zeros(148, np.uint8), 0)
    rec[4] = rec[0]
    sh, st = M.hs_dh(rec, 4, 5, ALICE, b"\x7e" * 160, [9] * 5)
    assert st == [M.X_OK, M.X_SKIPPED, M.X_ZERO, M.X_BADDESC, 9]
    assert sh[:32].hex() == SHARED and sh[32:96] == bytes(64) and sh[96:] == b"\x7e" * 64
    sh, st = M.hs_dh(rec, None, 5, ALICE, b"\x7e" * 160, [9] * 5)
    assert st[4] == M.X_OK and sh[128:].hex() == SHARED
    assert M.hs_dh(rec, 7, 2, ALICE, b"\x7e" * 160, [9] * 5)[1] == [M.X_OK, M.X_SKIPPED, 9, 9, 9]


# ---- layouts -----------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    fields = [("wg_x25519_desc", "WgX25519Desc", ["scalar_off", "point_off", "out_off", "flags", "_pad"]),
              ("wg_hs_dh_batch", "WgHsDhBatch", ["records", "n_records", "shared", "dh_status", "n", "_reserved"])]
    consts = ["WG_X25519_OK", "WG_X25519_BADDESC", "WG_X25519_ZERO", "WG_X25519_SKIPPED", "WG_X25519_BASE"]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += "".join(f'printf("%u\\n", {c});' for c in consts)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\nint main(void){' + body + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    L = wg()._lib
    want = []
    for _, p, fs in fields:
        cls = getattr(L, p)
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    want += [getattr(L, c) for c in consts]
    assert got == want
    assert ctypes.sizeof(L.WgX25519Desc) == 32 and ctypes.sizeof(L.WgHsDhBatch) == 40
    assert [M.X_OK, M.X_BADDESC, M.X_ZERO, M.X_SKIPPED, M.X_BASE] == want[-5:]
    W = wg()
    assert W.WG_X25519_DTYPE.itemsize == 32 and W.WG_X25519_DTYPE == M.X25519_DESC
    d = W.pack_x25519_desc([1], [2], [3], [1])
    assert W.desc_as_int64(d).tolist() == [[1, 2, 3, 1]]


def test_new_calls_are_bound():
    new = ("wg_x25519_batch", "wg_hs_static_set", "wg_hs_dh")
    assert set(new) <= {name for name, _, _ in wg()._lib.SIGNATURES}
    lib = wg().lib()
    assert all(hasattr(lib, n) for n in new)
    N = noise()
    assert N.X25519.POINT_SIZE == 32 and N.X25519.SCALAR_SIZE == 32
    k = bytearray(32)
    N.X25519.generatePrivateKey(lambda n: b"\xff" * n, k)
    assert bytes(k) == M.clamp(b"\xff" * 32)
    with pytest.raises(ValueError):
        N.X25519.generatePrivateKey(os.urandom, bytearray(31))


def _has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_device_fails_loudly():
    W, N = wg(), noise()
    lib = W.lib()
    buf = (ctypes.c_uint8 * 64)()
    b = W._lib.WgHsDhBatch(None, None, None, None, 1, 0)
    assert lib.wg_x25519_batch(None, None, 1, None, 0, None, 0, None, None) < 0
    assert lib.wg_hs_static_set(None, buf, buf) < 0
    assert lib.wg_hs_dh(None, ctypes.byref(b), None) < 0
    with pytest.raises(W.WgError) as e:  # the mirror has no host arithmetic to fall back to
        N.X25519.scalarMultBase(ALICE, 0, bytearray(32), 0)
    assert e.value.code == W._lib.WG_EDEVICE
    with pytest.raises(W.WgError):
        N.NoisePrivateKey(ALICE)
