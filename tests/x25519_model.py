"""Plain-Python restatement of wg_x25519_batch, wg_hs_static_set and wg_hs_dh (include/wgaead.h): the RFC 7748
ladder on Python integers, one operand at a time. Nothing here shares a line with the library's limb arithmetic.
"""
from __future__ import annotations

import numpy as np

X_OK, X_BADDESC, X_ZERO, X_SKIPPED = 0, 1, 2, 3
X_BASE = 1
INIT_SIZE, RESP_SIZE = 148, 92
P = (1 << 255) - 19
A24 = 121665
BASE_POINT = (9).to_bytes(32, "little")

X25519_DESC = np.dtype([("scalar_off", "<u8"), ("point_off", "<u8"), ("out_off", "<u8"), ("flags", "<u4"),
                        ("_pad", "<u4")])


def clamp(scalar: bytes) -> bytes:
    """RFC 7748 5, decodeScalar25519: what the device does to every scalar."""
    k = bytearray(scalar)
    k[0] &= 0xF8
    k[31] &= 0x7F
    k[31] |= 0x40
    return bytes(k)


def ladder(k: int, x1: int) -> int:
    """The u coordinate of k times the point with u coordinate x1 (0 for the point at infinity): RFC 7748's
    Montgomery ladder over the 255 low bits of k, without any clamping."""
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2 * pow(z2, P - 2, P) % P


def x25519(scalar: bytes, u: bytes) -> bytes:
    """RFC 7748 5: X25519(k, u), 32 bytes each. Bit 255 of u is masked; u is not required to be below p."""
    assert len(scalar) == 32 and len(u) == 32
    k = int.from_bytes(clamp(scalar), "little")
    x1 = (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P
    return ladder(k, x1).to_bytes(32, "little")


ORDER = (1 << 252) + 27742317777372353535851937790883648493  # of the base point's subgroup


def operands_for_result(scalar: bytes, candidates):
    """(u, r): the first r of `candidates` (integers below p) that is the u coordinate of a point of the
    prime-order subgroup, and the u with X25519(scalar, u) = r: the point r times the inverse of the
    clamped scalar modulo the subgroup's order. None when no candidate is such a point."""
    k = int.from_bytes(clamp(scalar), "little")
    for r in candidates:
        if r > 1 and ladder(ORDER, r) == 0 and ladder(ORDER - 1, r) == r:
            return ladder(pow(k, -1, ORDER), r).to_bytes(32, "little"), r.to_bytes(32, "little")
    return None


def public_key(private: bytes) -> bytes:
    """X25519.generatePublicKey: the base point u = 9."""
    return x25519(private, BASE_POINT)


def _in32(off: int, size: int) -> bool:
    return off <= size and 32 <= size - off


def batch(desc, inp: bytes, out: bytes):
    """wg_x25519_batch. Returns (out after the call, status list). desc: X25519_DESC array."""
    inp, out = bytes(inp), bytearray(out)
    status = []
    for d in desc:
        so, po, oo, fl, pad = (int(d[f]) for f in ("scalar_off", "point_off", "out_off", "flags", "_pad"))
        base = bool(fl & X_BASE)
        ok = (fl & ~X_BASE) == 0 and pad == 0 and _in32(so, len(inp)) and (base or _in32(po, len(inp))) \
            and _in32(oo, len(out))
        if not ok:
            status.append(X_BADDESC)
            continue
        r = x25519(inp[so:so + 32], BASE_POINT if base else inp[po:po + 32])
        out[oo:oo + 32] = r
        status.append(X_OK if any(r) else X_ZERO)
    return bytes(out), status


def hs_dh(records, n_records, n: int, private: bytes, shared: bytes, dh_status):
    """wg_hs_dh over an HS_RECORD array (hs_model.HS_RECORD). n_records None: all n. Returns (shared after
    the call, status list after the call); entries behind min(n_records, n) keep what they held."""
    shared, st = bytearray(shared), list(dh_status)
    cover = n if n_records is None else min(int(n_records), n)
    for k in range(cover):
        ln = int(records[k]["len"])
        if ln == INIT_SIZE:
            r = x25519(private, records[k]["msg"][8:40].tobytes())
            shared[32 * k:32 * k + 32] = r
            st[k] = X_OK if any(r) else X_ZERO
        elif ln == RESP_SIZE:
            shared[32 * k:32 * k + 32] = bytes(32)
            st[k] = X_SKIPPED
        else:
            st[k] = X_BADDESC
    return bytes(shared), st
