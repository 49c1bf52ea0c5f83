"""Poly1305 edge states, reached through the ciphertext: a solver and two limb-exact models. CPU only, plain
Python integers; the ChaCha20 block and keystream are the oracle's py_chacha20_block / py_chacha20.

The solver. The transport AEAD's tag is Poly1305 over ct (zero-padded to 16) || LE64(aad len) || LE64(len) under
(r, s) = ChaCha20 block 0 of (key, nonce). A test knows key and counter, hence r and s, and an open takes the
ciphertext as given (a seal produces it from pt = ct XOR keystream). With blocks m_0 .. m_{n-1}, m_i = c_i + 2^128,
the accumulator before `+ s` is H = sum m_i r^(n-i) mod p, affine in any one block: H = A + m_j r^(n-j). steer()
solves m_j = (H - A) r^-(n-j) mod p and accepts it when 2^128 <= m_j < 2^129 (a full block), about one try in
four; otherwise it redraws one other block, the salt block, and tries again.

The limb models restate what the device does to its five 26-bit limbs, so that a test can say which
representation of a residue enters wg_device.h's poly_finish:

* serial_prefinish(): h += block; h = poly_mul(h, r) per block, the form of the handshake chains' poly_tag
  (wg_hs_chain.hip);
* pp_prefinish(): the per-packet server's Poly1305 wave (wg_pp.hip, mac_tag): r^(j+1) per lane by the product
  scan, one Horner step by r^64 per 64 blocks, the lane's power, the row sums, one carry pass, the sum of rows;

both on test_stitch_asm's poly_mul, the limb-exact step the stitched code is already held to. finish() restates
poly_finish and reports whether its select took g = h + 5 - 2^130, that is whether the representation that
entered it, once normalised, was >= p.

The transport kernels, k_tile and k_wave combine lane sums in other orders, and these models do not restate
them. For them the residues 0 .. 4 are still the inputs on which "select g" and "keep h" give different tags
whenever the representation is >= p: a representation of such a residue is either the residue itself or residue
+ p, and only below 5 does residue + p fit under 2^130. A kernel whose select is wrong therefore fails a residue
0 .. 4 case whichever way it arrives at the residue, provided it arrives at residue + p; for those kernels the
tests do not claim that it did.
"""
from __future__ import annotations

import random
import struct

from test_stitch_asm import poly_mul
from wgtest import oracle, splitmix_bytes

P = (1 << 130) - 5
M26, M32, M128 = (1 << 26) - 1, (1 << 32) - 1, (1 << 128) - 1
HIBIT = 1 << 128
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
MAX_TRIES = 64
FILLS = ("rand", "ff", "00")


# ---- the one-time key and the MAC input ---------------------------------------------------------------------

def one_time_key(key: bytes, counter: int, nonce: bytes | None = None) -> bytes:
    """r || s of the transport packet (key, counter), or of an explicit 12-byte nonce."""
    O = oracle()
    return O.py_chacha20_block(bytes(key), 0, O.transport_nonce(counter) if nonce is None else bytes(nonce))[:32]


def r_s(otk: bytes) -> tuple[int, int]:
    return int.from_bytes(otk[:16], "little") & CLAMP, int.from_bytes(otk[16:32], "little")


def mac_input(ct: bytes, aad: bytes = b"") -> bytes:
    """aad and ct, each zero-padded to 16, then LE64(len(aad)) || LE64(len(ct)): whole blocks only."""
    pad = lambda b: bytes(b) + bytes(-len(b) % 16)
    return pad(aad) + pad(ct) + struct.pack("<QQ", len(aad), len(ct))


def _blocks(data: bytes) -> list[int]:
    assert len(data) % 16 == 0
    return [int.from_bytes(data[o:o + 16], "little") + HIBIT for o in range(0, len(data), 16)]


def residue(otk: bytes, data: bytes) -> int:
    """The accumulator mod p before `+ s`, for a MAC input of whole blocks."""
    r, _ = r_s(otk)
    h = 0
    for m in _blocks(data):
        h = (h + m) * r % P
    return h


# ---- the solver -------------------------------------------------------------------------------------------

def steer_tries(key, counter, length, free_block, target_H, fill, rng, aad=b"", nonce=None):
    """steer(), returning (ciphertext, tries): tries = 1 when the first solution was a full block."""
    assert length >= 32 and fill in FILLS and 0 <= target_H < P  # a solved block and a salt block at the least
    nfull = length // 16
    assert 0 <= free_block < nfull
    salt = 0 if free_block else 1
    r, _ = r_s(one_time_key(key, counter, nonce))
    if r == 0:
        raise ValueError("r = 0: the tag does not depend on the ciphertext")
    ct = bytearray({"ff": b"\xff", "00": b"\x00"}[fill] * length if fill != "rand" else
                   rng.getrandbits(8 * length).to_bytes(length, "little"))
    na = (len(aad) + 15) // 16
    n = na + (length + 15) // 16 + 1
    j = na + free_block
    inv = pow(pow(r, n - j, P), -1, P)
    for tries in range(1, MAX_TRIES + 1):
        ct[16 * free_block:16 * free_block + 16] = bytes(16)
        blocks = _blocks(mac_input(ct, aad))
        blocks[j] = 0
        A = 0
        for m in blocks:
            A = (A + m) * r % P
        m = (target_H - A) * inv % P
        if HIBIT <= m < 2 * HIBIT:
            ct[16 * free_block:16 * free_block + 16] = (m - HIBIT).to_bytes(16, "little")
            return bytes(ct), tries
        ct[16 * salt:16 * salt + 16] = rng.getrandbits(128).to_bytes(16, "little")
    raise RuntimeError(f"no full block reaches the residue in {MAX_TRIES} tries")


def steer(key, counter, length, free_block, target_H, fill, rng, aad=b"", nonce=None) -> bytes:
    """A ciphertext of `length` bytes whose Poly1305 accumulator under (key, counter), taken mod p before `+ s`,
    is target_H. free_block: the full block that is solved for; the salt block (block 0, or block 1 when block 0
    is free) is redrawn from rng (getrandbits) after a miss; every other byte is `fill`: "rand", "ff" or "00". A
    last partial block is fill only. From 48 bytes on some block keeps its fill; 32 is the least. aad: blocks in front of the ciphertext's (the general AEAD); nonce: instead
    of the transport nonce of `counter`. Raises after MAX_TRIES misses."""
    return steer_tries(key, counter, length, free_block, target_H, fill, rng, aad, nonce)[0]


def tag_target(key, counter, T: bytes, nonce=None) -> list[int]:
    """The residues H < p with (H + s) mod 2^128 == T, for k = 0 .. 3 in order (a k whose candidate is >= p is
    left out: only k = 3 can be)."""
    _, s = r_s(one_time_key(key, counter, nonce))
    low = (int.from_bytes(T, "little") - s) & M128
    return [low + (k << 128) for k in range(4) if low + (k << 128) < P]


def tag_of(key, counter, ct: bytes, aad: bytes = b"", nonce=None) -> bytes:
    return oracle().py_poly1305(one_time_key(key, counter, nonce), mac_input(ct, aad))


# ---- the targets: one table for every test --------------------------------------------------------------

def _le(hexwords: str) -> bytes:
    return bytes.fromhex(hexwords)


# ("H", residue) or ("T", tag bytes, k): k indexes tag_target()'s list (taken modulo its length)
TARGETS = (
    [("H", v) for v in (0, 1, 2, 3, 4, 5, 6)]
    + [("H", P - d) for d in (1, 2, 5, 6)]           # P - 1 is also 2^130 - 6, the largest residue
    + [("H", v) for v in ((1 << 128) - 1, 1 << 128, (1 << 128) + 1, (1 << 129) - 1, 1 << 129)]
    + [("T", bytes(16), k) for k in range(4)]         # h + s = 2^128 exactly: a carry out of every word
    + [("T", b"\xff" * 16, k) for k in range(4)]
    + [("T", _le("01" + "00" * 15), 0), ("T", _le("ffffffff" + "00" * 12), 1), ("T", _le("00" * 12 + "efbeadde"), 2)]
)


def resolve(target, key, counter, nonce=None) -> int:
    """A TARGETS entry as a residue under (key, counter)."""
    if target[0] == "H":
        return target[1]
    c = tag_target(key, counter, target[1], nonce)
    return c[target[2] % len(c)]


def label(target) -> str:
    if target[0] == "T":
        return f"T={target[1].hex()}/k{target[2]}"
    v = target[1]
    for name, base in (("p", P), ("2^129", 1 << 129), ("2^128", 1 << 128)):
        if abs(v - base) <= 8:
            return f"H={name}{v - base:+d}" if v != base else f"H={name}"
    return f"H={v}"


# ---- the device's limbs -----------------------------------------------------------------------------------

def limbs(v: int) -> list[int]:
    """poly_block_limbs: four 26-bit limbs and the rest (bit 128 of a full block lands at bit 24 of limb 4)."""
    return [v & M26, (v >> 26) & M26, (v >> 52) & M26, (v >> 78) & M26, v >> 104]


def value(h) -> int:
    return sum(x << (26 * i) for i, x in enumerate(h))


def _carry_pass(h, wrap: bool):
    for i in range(4):
        c = h[i] >> 26
        h[i] &= M26
        h[i + 1] = (h[i + 1] + c) & M32
    if wrap:
        c = h[4] >> 26
        h[4] &= M26
        h[0] = (h[0] + 5 * c) & M32


def finish(h, s: int) -> tuple[bytes, bool, int]:
    """poly_finish (wg_device.h) on limbs < 2^32 in 32-bit arithmetic: (tag, took_g, v). v is the normalised
    value the select sees; took_g says that it chose g = h + 5 - 2^130, which it does exactly when v >= p."""
    h = list(h)
    assert all(0 <= x <= M32 for x in h)
    _carry_pass(h, True)
    _carry_pass(h, True)
    _carry_pass(h, False)
    v = value(h)
    g = [0] * 5
    c = 5
    for i in range(4):
        g[i] = (h[i] + c) & M32
        c = g[i] >> 26
        g[i] &= M26
    g[4] = (h[4] + c - (1 << 26)) & M32
    took = (g[4] >> 31) == 0
    assert took == (v >= P)
    if took:
        h = g
    w = [(h[0] | (h[1] << 26)) & M32, ((h[1] >> 6) | (h[2] << 20)) & M32, ((h[2] >> 12) | (h[3] << 14)) & M32,
         ((h[3] >> 18) | (h[4] << 8)) & M32]
    f, tag = 0, []
    for i in range(4):
        f = w[i] + ((s >> (32 * i)) & M32) + (f >> 32)
        tag.append(f & M32)
    return struct.pack("<4I", *tag), took, v


def serial_prefinish(otk: bytes, data: bytes) -> list[int]:
    """The limbs that poly_tag's Horner loop hands to poly_finish for a MAC input of whole blocks."""
    r = limbs(r_s(otk)[0])
    h = [0] * 5
    for m in _blocks(data):
        h = poly_mul([a + b for a, b in zip(h, limbs(m))], r)
    return h


def _pp_powers(r: int) -> list[list[int]]:
    """wg_pp.hip's product scan: lane j ends with r^(j+1), in the limbs the scan's poly_mul steps leave."""
    y = [limbs(r) for _ in range(64)]
    for n in (1, 2, 4, 8):       # row_shr n inside each row of 16
        y = [poly_mul(y[j], y[j - n]) if (j & 15) >= n else y[j] for j in range(64)]
    y = [poly_mul(y[j], y[(j & ~15) - 1]) if j & 16 else y[j] for j in range(64)]  # rows 1, 3 by the row before's r^16
    y = [poly_mul(y[j], y[31]) if j >= 32 else y[j] for j in range(64)]            # rows 2, 3 by r^32
    return y


def pp_prefinish(otk: bytes, ct: bytes) -> list[int]:
    """The limbs that the per-packet server's mac_tag hands to poly_finish for a transport packet's ciphertext."""
    blocks = _blocks(mac_input(ct))
    y = _pp_powers(r_s(otk)[0])
    R = y[63]
    M = len(blocks)
    T = (M + 63) // 64
    D = 64 * T - M
    rows = [[0] * 5 for _ in range(4)]
    for lane in range(64):
        acc = [0] * 5
        for t in range(T):
            if t:
                acc = poly_mul(acc, R)
            p = 64 * t + 63 - lane
            if p >= D:
                acc = [a + b for a, b in zip(acc, limbs(blocks[p - D]))]
        acc = poly_mul(acc, y[lane])
        rows[lane >> 4] = [(a + b) & M32 for a, b in zip(rows[lane >> 4], acc)]
    out = [0] * 5
    for row in rows:
        _carry_pass(row, True)
        out = [(a + b) & M32 for a, b in zip(out, row)]
    return out


# ---- raw one-time-key cases (RFC 8439 A.3 in kind, regenerated from the arithmetic) -----------------------

R_MAX = CLAMP.to_bytes(16, "little")
FF16 = b"\xff" * 16


def _sum_case(total: int, nblocks: int) -> bytes:
    """nblocks full blocks whose values m_i = c_i + 2^128 add up to `total`: with r = 1 the accumulator is their
    plain sum."""
    rest = total - nblocks * HIBIT
    out = []
    for _ in range(nblocks):
        c = min(rest, M128)
        out.append(c.to_bytes(16, "little"))
        rest -= c
    assert rest == 0
    return b"".join(out)


def raw_mac_cases() -> list[tuple[str, bytes, bytes, int | None]]:
    """(name, r || s, message, the residue before `+ s` where the case was built for one, else None)."""
    one, two = (1).to_bytes(16, "little"), (2).to_bytes(16, "little")
    cases = [
        # r = 2: (ff..ff + 2^128) * 2 = 2^130 - 2 = p + 3
        ("r2_ff", two + bytes(16), FF16, 3),
        ("r2_ff_sff", two + FF16, FF16, 3),
        # r = 1: the accumulator is the sum of the blocks
        ("r1_sum_p", one + FF16, _sum_case(P, 3), 0),                  # exactly p: g is taken, tag = s
        ("r1_sum_p-1", one + FF16, _sum_case(P - 1, 3), P - 1),        # the largest residue: h is kept
        ("r1_sum_p+1", one + FF16, _sum_case(P + 1, 3), 1),
        ("r1_sum_p+4", one + FF16, _sum_case(P + 4, 3), 4),            # 2^130 - 1: the last value g covers
        ("r1_sum_2^130", one + FF16, _sum_case(1 << 130, 3), 5),       # wraps in the carry, not in the select
        ("r1_sum_2p", one + FF16, _sum_case(2 * P, 7), 0),
        ("r1_sum_2p+4", one + bytes(16), _sum_case(2 * P + 4, 7), 4),
        ("r1_4ff", one + bytes(16), FF16 * 4, (4 * ((1 << 129) - 1)) % P),
        ("r1_64ff", one + FF16, FF16 * 64, (64 * ((1 << 129) - 1)) % P),
        # h + s = 2^128 exactly: the carry runs through every tag word
        ("r1_ripple", one + FF16, one, (1 << 128) + 1),
        ("r1_ripple_k3", one + (6).to_bytes(16, "little"), _sum_case(P - 1, 3), P - 1),  # p - 1 + 6 = 2^130
        # r = 0: the tag is s whatever the message
        ("r0_ff", bytes(16) + FF16, FF16 * 5, 0),
        ("r0_empty", bytes(16) + bytes(range(16)), b"", 0),
        ("r1_empty", one + FF16, b"", 0),
    ]
    for n in (16, 17, 63, 64, 1008, 1024, 2048):                      # 63 / 64 blocks: 1008 / 1024
        cases.append((f"rmax_ff_{n}", R_MAX + FF16, b"\xff" * n, None))
    for k in range(1, 16):                                           # a partial last block of every length
        cases.append((f"rmax_ff_{k}", R_MAX + FF16, b"\xff" * k, None))
        cases.append((f"rmax_ff_1008+{k}", R_MAX + FF16, b"\xff" * (1008 + k), None))
        cases.append((f"r1_ff_32+{k}", one + FF16, b"\xff" * (32 + k), None))
    return cases


# ---- per-packet cases whose select is known to take g ---------------------------------------------------------

def pp_select_cases(L, want=4, limit=64):
    """Seeded per-packet cases at residues 0 .. 4 whose modelled representation (pp_prefinish) enters poly_finish
    in [p, 2^130): [(key, counter, ct, residue)], at most `want` of them from the first `limit` seeds."""
    found = []
    for seed in range(limit):
        key = splitmix_bytes(0x5E1EC7 + 64 * L + seed, 32)
        counter = seed * 0x100000001 + L
        H = seed % 5
        ct = steer(key, counter, L, seed % (L // 16), H, FILLS[seed % 3], random.Random(seed))
        otk = one_time_key(key, counter)
        _, took, v = finish(pp_prefinish(otk, ct), r_s(otk)[1])
        if took and P <= v < (1 << 130):
            assert v == P + H
            found.append((key, counter, ct, H))
            if len(found) == want:
                break
    return found
