"""Route tables and destinations for the transmit planner's edges (wg_routes_set / wg_tx_plan,
wireguard-java_amd/csrc/wg_tx.hip): a route at every prefix length of both families, prefixes nested
inside one byte of the compiled stride-8 nodes, equal prefixes given several times, a random table with
host bits set, families without routes. No GPU here: tests/test_tx.py checks what these builders claim,
tests/test_gpu_tx_edges.py sends the same tables to the device. Routes are (ipaddress address, prefix
length, key slot) triples as Engine.routes_set and tx_model.RouteTable take them, destinations are 4 or
16 address bytes. ``Brute`` is a second longest-prefix match that does not go through ``ipaddress``
networks; tx_model.RouteTable is asserted against it on the CPU so neither can go stale alone."""
from __future__ import annotations

import functools
import ipaddress
from typing import NamedTuple

import numpy as np

import tx_model

KEY_SLOTS = 4096


class Case(NamedTuple):
    name: str
    routes: list  # (ipaddress address, prefix length, key slot)
    dests: list   # bytes of 4 or 16


def ip(b: bytes):
    return ipaddress.ip_address(bytes(b))


def flip(addr: bytes, bit: int) -> bytes:
    """addr with bit `bit` flipped, bit 0 being the first on the wire."""
    a = bytearray(addr)
    a[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(a)


# ---- the brute-force lookup ---------------------------------------------------------------------
class Brute:
    """Over all routes of the destination's family: the greatest prefix length whose top bits equal the
    destination's, the later index on ties. lookup() returns (prefix length, key slot) or None."""

    def __init__(self, routes):
        self.fam = {}
        for nb in (4, 16):
            rs = [(a.packed, p, s) for a, p, s in routes if len(a.packed) == nb]
            addr = np.array([list(r[0]) for r in rs], np.uint8).reshape(-1, nb)
            plen = np.array([r[1] for r in rs], np.int64)
            mask = np.packbits(np.arange(nb * 8)[None, :] < plen[:, None], axis=1)
            self.fam[nb] = (addr, mask, plen, [r[2] for r in rs])

    def lookup(self, dst: bytes):
        addr, mask, plen, slots = self.fam[len(dst)]
        hit = np.nonzero(~((addr ^ np.frombuffer(dst, np.uint8)) & mask).any(axis=1))[0]
        if not len(hit):
            return None
        last = int(hit[plen[hit] == plen[hit].max()][-1])
        return int(plen[last]), slots[last]


# ---- 1. ladders ---------------------------------------------------------------------------------
# Mixed bits and no byte twice, so a byte read from the wrong position shows; tests/test_tx.py checks that
# the flipped addresses are all different.
X4 = bytes([0xB6, 0x4D, 0x93, 0x2A])
X6 = bytes([0x2A, 0xD5, 0x36, 0xC9, 0x5B, 0xA4, 0x6D, 0x92, 0xB5, 0x4A, 0xD3, 0x2C, 0x69, 0x96, 0xCB, 0x35])


def ladder_slot(family: int, k: int) -> int:
    """Key slot of the ladder's /k route: one per route, spread over the table."""
    return (5 + 113 * k) % KEY_SLOTS if family == 4 else (2049 + 29 * k) % KEY_SLOTS


def ladder_lengths(family: int, odd: bool) -> list[int]:
    return [k for k in range(0, (32 if family == 4 else 128) + 1) if k % 2 or not odd]


def ladder(odd: bool = False) -> Case:
    """X/k for every k (odd k only for the odd ladder), written as X itself: every host bit behind the
    prefix is whatever X has there. Destinations per family: X with bit k flipped for every k, then X."""
    routes, dests = [], []
    for family, X in ((4, X4), (6, X6)):
        routes += [(ip(X), k, ladder_slot(family, k)) for k in ladder_lengths(family, odd)]
        dests += [flip(X, k) for k in range(len(X) * 8)] + [X]
    return Case("odd ladder" if odd else "ladder", routes, dests)


def ladder_expect(odd: bool = False) -> list:
    """Key slot (None: no route) per destination of ladder(odd), from the construction alone: bit k
    flipped leaves exactly the top k bits equal, so the longest route is /k; in the odd ladder the next
    odd length at or below k, and nothing for bit 0."""
    out = []
    for family, nbits in ((4, 32), (6, 128)):
        for k in range(nbits + 1):  # k == nbits: X itself
            best = k if not odd or k % 2 else k - 1
            out.append(ladder_slot(family, best) if best >= 0 else None)
    return out


# ---- 2. prefixes nested inside one byte ------------------------------------------------------------
NEST_BYTES = {4: (0, 1, 2, 3), 6: (0, 7, 8, 15)}
Y4 = bytes([0x5A, 0xC3, 0x96, 0x69])
Y6 = bytes([0x9C, 0x27, 0xE1, 0x58, 0x3D, 0xA6, 0x4B, 0xF2, 0x71, 0x8E, 0xD4, 0x1B, 0x65, 0xBA, 0x0F, 0xC8])
NEST_SIBLINGS = (3, 6, 8)  # lengths inside the byte at which a branch off Y's path carries a prefix too


def nest(family: int, b: int) -> Case:
    """One compiled node walked entry by entry. Routes: Y/(8b + j) for j = 1..8 (all end inside byte b),
    a prefix of length 8b + j that leaves Y's path one bit earlier for j = 3, 6 and 8 (so Y/(8b + j - 2)
    still wins where the bit after the branch differs), Y/8b (the last bit of the byte before; /0 for b = 0) and, unless b is the last byte, two prefixes ending at the first bit of the byte
    after: one below Y/(8b + 8) and one below the j = 6 branch, so their nodes are entered through an
    entry in which a shorter prefix ends. Destinations: byte b takes all 256 values with the byte after as
    Y has it, again with the byte after's first bit flipped, and (b > 0) again with the last bit of the byte
    before flipped, where nothing matches."""
    Y = Y4 if family == 4 else Y6
    nb, slot = len(Y), iter(range(77 + 211 * b + (0 if family == 4 else 700), KEY_SLOTS))
    routes = [(ip(Y), 8 * b, next(slot))]
    for j in range(1, 9):
        routes.append((ip(Y), 8 * b + j, next(slot)))
        if j in NEST_SIBLINGS:
            routes.append((ip(flip(Y, 8 * b + j - 2)), 8 * b + j, next(slot)))
    if b + 1 < nb:
        routes.append((ip(Y), 8 * b + 9, next(slot)))
        routes.append((ip(flip(Y, 8 * b + 4)), 8 * b + 9, next(slot)))
    bases = [Y] + ([flip(Y, 8 * b + 8)] if b + 1 < nb else []) + ([flip(Y, 8 * b - 1)] if b else [])
    dests = [base[:b] + bytes([v]) + base[b + 1:] for base in bases for v in range(256)]
    return Case(f"nest v{family} byte {b}", routes, dests)


def nests(family: int) -> list[Case]:
    return [nest(family, b) for b in NEST_BYTES[family]]


# ---- destinations near a table's routes -----------------------------------------------------------
def probe_dests(routes, rng, n: int) -> list:
    """As tests/test_gpu_rx.py::_packet draws them: 7 in 10 a route's address, half of those with one
    bit flipped at plen - 3 .. end; the rest random (IPv6 for 45 in 100)."""
    out = []
    for _ in range(n):
        if routes and rng.random() < 0.7:
            a, plen, _ = routes[int(rng.integers(0, len(routes)))]
            d = a.packed
            if rng.random() < 0.5:
                d = flip(d, int(rng.integers(max(plen - 3, 0), len(d) * 8)))
        else:
            d = rng.bytes(16 if rng.random() < 0.45 else 4)
        out.append(d)
    return out


def around(routes) -> list:
    """Every route's address as written, and with each bit from plen - 2 to plen + 1 flipped."""
    out = []
    for a, plen, _ in routes:
        d = a.packed
        out += [d] + [flip(d, k) for k in range(max(plen - 2, 0), min(plen + 2, len(d) * 8))]
    return out


# ---- 3. ties and order ----------------------------------------------------------------------------
def ties() -> list[Case]:
    A = ipaddress.ip_address
    twice = [(A("10.20.0.0"), 14, 301), (A("172.16.5.0"), 24, 302), (A("10.20.0.0"), 14, 303),
             (A("fd00:1234::"), 45, 304), (A("10.20.128.0"), 17, 305), (A("fd00:1234::"), 45, 306)]
    thrice = [(A("192.168.77.1"), 32, 311), (A("2001:db8:5::"), 47, 312), (A("192.168.77.1"), 32, 313),
              (A("2001:db8:5::"), 47, 314), (A("192.168.64.0"), 19, 315), (A("192.168.77.1"), 32, 316),
              (A("2001:db8:5::"), 47, 317)]
    host_bits = [(A("10.20.1.2"), 14, 321), (A("10.23.255.255"), 14, 322), (A("10.21.7.7"), 14, 323),
                 (A("fd00:1234:7:ffff::9"), 45, 324), (A("fd00:1234:5::"), 45, 325), (A("10.22.0.0"), 15, 326)]
    others = [(A("10.0.0.0"), 8, 331), (A("128.0.0.0"), 1, 332), (A("2000::"), 3, 333), (A("8000::"), 1, 334)]
    zero_first = ([(A("0.0.0.0"), 0, 341), (A("::"), 0, 342)] + others +
                  [(A("255.1.2.3"), 0, 343), (A("ffff::1"), 0, 344)])
    zero_only_later = others + [(A("1.2.3.4"), 0, 351), (A("::7"), 0, 352), (A("0.0.0.0"), 0, 353)]
    edge = [b"\0" * 4, b"\xff" * 4, b"\0" * 16, b"\xff" * 16, b"\x7f" + b"\xff" * 3, b"\x7f" + b"\xff" * 15]
    return [Case(name, r, around(r) + edge) for name, r in (
        ("a prefix given twice", twice), ("a prefix given three times", thrice),
        ("one network, other host bits", host_bits), ("/0 before and after", zero_first),
        ("/0 after the other routes", zero_only_later))]


# ---- 4. the random table --------------------------------------------------------------------------
RANDOM_SEED = 20
RANDOM_V4, RANDOM_V6 = 330, 1570  # 10 and 12 routes per length: dense enough to nest, short prefixes still win
RANDOM_DESTS = 2500               # distinct destinations (the model's lookup takes about a millisecond each)
RANDOM_DUP = 100                  # about 5 %: an earlier (address, length) again with another slot


@functools.lru_cache(maxsize=None)
def random_table() -> Case:
    """About 2,000 routes of both families: lengths uniform over 0..32 and 0..128, random host bits, key
    slots from the whole table (0 and the last among them), 100 exact duplicates with another slot, in a
    seeded order; 20,000 destinations drawn with repeats from 2,500 that probe_dests drew."""
    rng = np.random.default_rng(RANDOM_SEED)
    routes = []
    for nb, count in ((4, RANDOM_V4), (16, RANDOM_V6)):
        for _ in range(count):
            routes.append((ip(rng.bytes(nb)), int(rng.integers(0, nb * 8 + 1)), int(rng.integers(0, KEY_SLOTS))))
    for _ in range(RANDOM_DUP):
        a, p, s = routes[int(rng.integers(0, len(routes)))]
        routes.append((a, p, (s + 1 + int(rng.integers(0, KEY_SLOTS - 1))) % KEY_SLOTS))
    routes = [routes[i] for i in rng.permutation(len(routes))]
    for at, slot in ((3, 0), (len(routes) - 7, KEY_SLOTS - 1)):  # both ends of the key table are routed to
        routes[at] = (routes[at][0], routes[at][1], slot)
    pool = probe_dests(routes, rng, RANDOM_DESTS)
    return Case("random table", routes, [pool[i] for i in rng.integers(0, len(pool), 20000)])


# ---- 5. families without routes -------------------------------------------------------------------
def small_table() -> list:
    A = ipaddress.ip_address
    return [(A("10.9.0.0"), 13, 40), (A("10.9.3.0"), 27, 41), (A("203.0.113.77"), 32, 42), (A("fd77::"), 17, 43),
            (A("fd77:0:0:1::"), 64, 44), (A("fd77::1"), 128, 45)]


def empty_families() -> list[Case]:
    rng = np.random.default_rng(55)
    small = small_table()
    v4, v6 = [r for r in small if r[0].version == 4], [r for r in small if r[0].version == 6]
    dests = around(small) + probe_dests(small, rng, 200)
    zeros = [(ipaddress.ip_address("0.0.0.0"), 0, KEY_SLOTS - 1), (ipaddress.ip_address("::"), 0, 0)]
    return [Case("IPv4 routes only", v4, dests), Case("IPv6 routes only", v6, dests), Case("no routes", [], dests),
            Case("a /0 per family and nothing else", zeros, dests)]


def all_cases() -> list[Case]:
    return ([ladder(False), ladder(True)] + nests(4) + nests(6) + ties() + [random_table()] + empty_families() +
            [Case("small table", small_table(), around(small_table()))])


@functools.lru_cache(maxsize=None)
def _route_table(name: str):
    return tx_model.RouteTable(next(c.routes for c in all_cases() if c.name == name))


def route_table(case: Case):
    """tx_model.RouteTable of one of all_cases(), built once per process: it remembers the lookups it has
    answered, and the random table's take seconds."""
    return _route_table(case.name)


# ---- packets --------------------------------------------------------------------------------------
def packet(dst: bytes, total: int, rng) -> bytes:
    """`total` bytes of an IPv4 or IPv6 packet (by the length of dst) to dst, the rest seeded noise."""
    v6 = len(dst) == 16
    at = 24 if v6 else 16
    p = bytearray(rng.bytes(max(total, at + len(dst))))
    p[0] = 0x60 | (p[0] & 0x0F) if v6 else 0x45
    p[at:at + len(dst)] = dst
    return bytes(p[:total])


def packets(dests, rng, max_len: int = 60, specials: bool = True):
    """(packets, where): one packet of 20..max_len B (IPv6: 40..max_len) per destination, destination k's
    at index where[k]; with `specials`, eight more at seeded positions: a keepalive, a version-5 packet,
    IPv4 of 19 B and IPv6 of 39 B (bad IP), a packet of max_len + 1 B to a routed-looking destination and
    one of max_len + 1 B with version 5 (too long wins over bad IP), and IPv4 / IPv6 of exactly 20 / 40 B."""
    out = [(packet(d, int(rng.integers(40 if len(d) == 16 else 20, max_len + 1)), rng), k)
           for k, d in enumerate(dests)]
    if specials:
        d4 = next((d for d in dests if len(d) == 4), X4)
        d6 = next((d for d in dests if len(d) == 16), X6)
        extra = [b"", bytes([0x51]) + rng.bytes(30), packet(d4, 19, rng), packet(d6, 39, rng),
                 packet(d4, max_len + 1, rng), bytes([0x50]) + rng.bytes(max_len), packet(d4, 20, rng),
                 packet(d6, 40, rng)]
        for p in extra:
            out.insert(int(rng.integers(0, len(out) + 1)), (p, -1))
    where = np.zeros(len(dests), np.int64)
    for i, (_, k) in enumerate(out):
        if k >= 0:
            where[k] = i
    return [p for p, _ in out], where
