"""AllowedIPs filters and plaintexts for the receive-side verdict at its edges (wg_filter_set / wg_slot_filters_set,
rx_verdict in wireguard-java_amd/csrc/wg_transport.hip, the stride-8 compile in wg_rx.hip): one prefix at every
length of both families, prefixes nested and side by side around every byte boundary of a compiled node, the
filters that let nothing or everything through, and packets at the 19/20 and 39/40-byte bounds with every version
nibble. No GPU here: tests/test_rx_filter_edges.py checks what these builders claim, tests/test_gpu_rx_filter_edges.py
sends the same filters and packets down every device path. Everything is seeded; nothing reads a clock.

A filter is a list of (ipaddress address, prefix length) pairs as Engine.filter_set takes them. A probe is
(filter id, plaintext bytes, expected status, ...): the status is oracle/rx.py's (IPFilter.search and
process_decrypted, the restatement of util/IPFilter.java and TransportManager.java:98-130), never the device's."""
from __future__ import annotations

import functools
import ipaddress
from typing import NamedTuple

import numpy as np

from oracle import rx

SEED = 0x1BF1
NO_FILTER = 0xFFFFFFFF  # WG_NO_FILTER: the key slot passes every destination
NEVER_SET = 4242        # an id above every id set: wg_filter_set is never called with it
GAP_ID = 170            # an id among those of (b) that is never set either
SENTINEL = 0xA5         # fills every buffer between the packets; at least GAP bytes of it follow each packet
GAP = 16
KEY_SLOTS = 256

# Mixed bits and no byte twice (tests/tx_edge_cases.py's ladders): a byte read from the wrong position shows
X4 = bytes([0xB6, 0x4D, 0x93, 0x2A])
X6 = bytes([0x2A, 0xD5, 0x36, 0xC9, 0x5B, 0xA4, 0x6D, 0x92, 0xB5, 0x4A, 0xD3, 0x2C, 0x69, 0x96, 0xCB, 0x35])
Y4 = bytes([0x5A, 0xC3, 0x96, 0x69])
Y6 = bytes([0x9C, 0x27, 0xE1, 0x58, 0x3D, 0xA6, 0x4B, 0xF2, 0x71, 0x8E, 0xD4, 0x1B, 0x65, 0xBA, 0x0F, 0xC8])


class Probe(NamedTuple):
    fid: int      # filter id of the packet's key slot (NO_FILTER: none; NEVER_SET and GAP_ID: ids never set)
    pt: bytes     # the plaintext as the open leaves it
    status: int   # rx.process_decrypted(pt, the filter)
    part: str     # "a", "b" or "c" of the case set
    kind: str     # what the probe is, e.g. "just outside", "outer only"
    dst: bytes    # the destination the packet was built around (b"" for the packets of (c) that have none)


class Cases(NamedTuple):
    filters: dict   # filter id -> [(address, prefix length)], every id that wg_filter_set is called with
    names: dict     # filter id -> what the filter is
    slot_of: dict   # filter id (NO_FILTER, NEVER_SET and GAP_ID among them) -> its key slot
    slot_ids: list  # filter id per key slot 0 .. len - 1, the argument of slot_filters_set
    split: int      # slot_filters_set(0, slot_ids[:split]), then slot_filters_set(split, slot_ids[split:])
    probes: list    # [Probe]
    b_kinds: dict   # filter id of (b) -> the probe kinds that filter must be asked


def ip(b: bytes):
    return ipaddress.ip_address(bytes(b))


def flip(addr: bytes, bit: int) -> bytes:
    """addr with bit `bit` flipped, bit 0 being the first on the wire."""
    a = bytearray(addr)
    a[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(a)


def oracle_filter(prefixes) -> rx.IPFilter:
    f = rx.IPFilter()
    for a, p in prefixes:
        f.insert(a.packed, p)
    return f


def packet(dst: bytes, total: int, rng, low: int | None = None) -> bytes:
    """`total` bytes of an IPv4 or IPv6 packet (by the length of dst) to dst, the rest seeded noise; cut short of
    the destination where total says so. low: the low nibble of byte 0 (IPv4 default 5, IPv6 default random)."""
    v6 = len(dst) == 16
    at = 24 if v6 else 16
    p = bytearray(rng.bytes(max(total, at + len(dst))))
    p[0] = (0x60 | (p[0] & 0x0F if low is None else low)) if v6 else (0x40 | (5 if low is None else low))
    p[at:at + len(dst)] = dst
    return bytes(p[:total])


def resize(pt: bytes, total: int, rng) -> bytes:
    """pt cut to `total` bytes, or followed by seeded noise up to them (the header and the destination stay)."""
    return pt[:total] if total <= len(pt) else pt + rng.bytes(total - len(pt))


def min_len(dst: bytes) -> int:
    return 40 if len(dst) == 16 else 20


# ---- (a) every prefix length, one prefix per filter -----------------------------------------------------------------
def a_filter_id(family: int, p: int) -> int:
    return p if family == 4 else 33 + p


def _a_probes(family: int, p: int) -> list:
    """(destination, kind) for the single-prefix filter X/p."""
    X, other = (X4, X6) if family == 4 else (X6, X4)
    nbits = len(X) * 8
    out = [(X, "base")]
    if p > 0:
        out.append((flip(X, p - 1), "just outside"))
    if p < nbits:
        out.append((flip(X, p), "first host bit"))
    out += [(flip(X, nbits - 1), "last bit"), (flip(X, 0), "first bit"), (other, "other family")]
    seen, uniq = set(), []
    for d, kind in out:  # /0, /1, /nbits - 1 and /nbits name one address twice: the first name stays
        if d not in seen:
            seen.add(d)
            uniq.append((d, kind))
    return uniq


# ---- (b) nested and sibling prefixes in one filter ------------------------------------------------------------------
NESTED_KINDS = ("outer only", "both", "neither")
SET_KINDS = ("in one member", "outside all")


def _chain(base: bytes, lens) -> tuple:
    """base/p for each p of lens (ascending), each covering the next: inside the outermost only, inside all of them
    (the base and its first host bit), inside all but the innermost, outside all."""
    nbits = len(base) * 8
    probes = [(base, "both"), (flip(base, lens[0]), "outer only"), (flip(base, lens[0] - 1), "neither"),
              (flip(base, 0), "neither")]
    if lens[-1] < nbits:
        probes.append((flip(base, lens[-1]), "both"))
    for q in lens[1:]:
        probes.append((flip(base, q - 1), "outer only" if q == lens[1] else "all but the innermost"))
    if len(lens) == 2:
        probes = [(d, k) for d, k in probes if k != "all but the innermost"]
    return [(ip(base), p) for p in lens], probes, NESTED_KINDS


def _b_filters() -> list:
    """(name, prefixes, [(destination, kind)], kinds that must occur)."""
    out = []

    def chain(name, base, lens):
        out.append((name,) + _chain(base, lens))

    chain("v4 /8 and a /24 under it", Y4, (8, 24))
    out.append(("v4 /24 only", [(ip(Y4), 24)],
                [(Y4, "in one member"), (flip(Y4, 31), "in one member"), (flip(Y4, 23), "outside all"),
                 (flip(Y4, 8), "outside all"), (flip(Y4, 7), "outside all")], SET_KINDS))
    chain("v4 /7 and /9", Y4, (7, 9))
    chain("v4 /15, /16 and /17", Y4, (15, 16, 17))
    chain("v4 /23 and /25", Y4, (23, 25))
    sib = flip(Y4, 16)
    out.append(("v4 two sibling /17s", [(ip(Y4), 17), (ip(sib), 17)],
                [(Y4, "in one member"), (sib, "in one member"), (flip(Y4, 17), "in one member"),
                 (flip(sib, 31), "in one member"), (flip(Y4, 15), "outside all"), (flip(sib, 15), "outside all"),
                 (flip(Y4, 0), "outside all")], SET_KINDS))
    chain("v4 /31 together with /32", Y4, (31, 32))
    chain("v6 /63, /64 and /65", Y6, (63, 64, 65))
    chain("v6 /119, /120 and /121", Y6, (119, 120, 121))
    chain("v6 /127 together with /128", Y6, (127, 128))
    out.append(("both families: v4 /20 and v6 /52", [(ip(Y4), 20), (ip(Y6), 52)],
                [(Y4, "in one member"), (Y6, "in one member"), (flip(Y4, 20), "in one member"),
                 (flip(Y6, 52), "in one member"), (flip(Y4, 19), "outside all"), (flip(Y6, 51), "outside all"),
                 (X4, "outside all"), (X6, "outside all")], SET_KINDS))
    host4, host6 = Y4[:2] + b"\xff\xff", Y6[:5] + b"\xff" * 11  # host bits set behind /13 and /37
    out.append(("unmasked addresses: v4 /13 and v6 /37", [(ip(host4), 13), (ip(host6), 37)],
                [(host4, "in one member"), (Y4[:2] + b"\0\0", "in one member"), (Y4, "in one member"),
                 (flip(Y4, 13), "in one member"), (host6, "in one member"), (Y6, "in one member"),
                 (Y6[:5] + bytes(11), "in one member"), (flip(Y4, 12), "outside all"), (flip(Y6, 36), "outside all")],
                SET_KINDS))
    zeros = [(bytes(4), "outside all"), (bytes(16), "outside all"), (X4, "outside all"), (X6, "outside all"),
             (flip(bytes(4), 31), "outside all"), (flip(bytes(16), 127), "outside all")]
    own = [(d, "in one member" if not any(d) else k) for d, k in zeros]  # inside its /32 or /128, which match nothing
    out.append(("allowingAll(): 0.0.0.0/32 and ::/128", [(ip(bytes(4)), 32), (ip(bytes(16)), 128)], own, SET_KINDS))
    out.append(("the empty filter", [], zeros, ("outside all",)))
    return out


# ---- (c) packet edges -----------------------------------------------------------------------------------------------
def _c_packets(rng) -> list:
    """(plaintext, kind, destination or b"")."""
    out = [(b"", "keepalive", b"")]
    out += [(packet(X4, n, rng), f"0x45 of {n} B", X4 if n >= 20 else b"") for n in (1, 19, 20, 21)]
    out += [(packet(X6, n, rng, low=0), f"0x60 of {n} B", X6 if n >= 40 else b"") for n in (39, 40, 41)]
    for nib in range(16):  # the low nibble varies; 0x4F and 0x6F are the ones a mask on the wrong side would lose
        low = 0xF if nib in (4, 6) else (nib * 7 + 3) & 0xF
        p = bytearray(packet(X6, 40, rng))
        p[16:20] = X4  # a destination wherever the nibble says it is
        p[0] = nib << 4 | low
        out.append((bytes(p), f"version nibble {nib:X} (0x{p[0]:02X}) of 40 B", X4 if nib == 4 else X6 if nib == 6 else b""))
    out.append((packet(Y4, 20, rng), "v4 of 20 B ending in its destination", Y4))
    out.append((packet(Y6, 40, rng), "v6 of 40 B ending in its destination", Y6))
    return out


# ---- the whole set --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases() -> Cases:
    rng = np.random.default_rng(SEED)
    filters, names, b_kinds, probes = {}, {}, {}, []
    oracles = {}

    def add_filter(fid, name, prefixes):
        filters[fid], names[fid] = prefixes, name
        oracles[fid] = oracle_filter(prefixes)

    def add_probe(fid, pt, part, kind, dst):
        flt = None if fid == NO_FILTER else oracles.get(fid, rx.IPFilter())  # an id never set: an empty filter
        probes.append(Probe(fid, pt, rx.process_decrypted(pt, flt), part, kind, dst))

    def add_dest(fid, part, kind, dst, k):
        # every other packet ends with its destination (20 / 40 B), the others carry up to 24 bytes behind it
        total = min_len(dst) + (0 if k % 2 == 0 else int(rng.integers(1, 25)))
        add_probe(fid, packet(dst, total, rng), part, kind, dst)

    # (a) ids 0 .. 32: X4/p; ids 33 .. 161: X6/p
    for family, X in ((4, X4), (6, X6)):
        for p in range(len(X) * 8 + 1):
            fid = a_filter_id(family, p)
            add_filter(fid, f"v{family} /{p}", [(ip(X), p)])
            for k, (dst, kind) in enumerate(_a_probes(family, p)):
                add_dest(fid, "a", kind, dst, k + p)
            if p % 16 == 0:
                add_probe(fid, b"", "a", "keepalive", b"")
    # (b) ids 162 ..; GAP_ID between them is never set, so its header entry is the image's own "no roots"
    fid = 162
    for name, prefixes, dests, kinds in _b_filters():
        if fid == GAP_ID:
            fid += 1
        add_filter(fid, name, prefixes)
        b_kinds[fid] = kinds
        for k, (dst, kind) in enumerate(dests):
            add_dest(fid, "b", kind, dst, k)
        add_probe(fid, b"", "b", "keepalive", b"")
        fid += 1
    assert fid > GAP_ID
    for special, name in ((GAP_ID, "an id never set, below the highest id"), (NEVER_SET, "an id never set, above every id"),
                          (NO_FILTER, "a slot mapped to WG_NO_FILTER")):
        names[special] = name
        for k, dst in enumerate((X4, X6, Y4, Y6, bytes(4), bytes(16))):
            add_dest(special, "b", "outside all" if special != NO_FILTER else "no filter", dst, k)
        add_probe(special, b"", "b", "keepalive", b"")
    # (c) a /0 of each family and no filter
    zero4, zero6 = fid, fid + 1
    add_filter(zero4, "v4 /0 alone (c)", [(ip(Y4), 0)])
    add_filter(zero6, "v6 /0 alone (c)", [(ip(Y6), 0)])
    for pt, kind, dst in _c_packets(rng):
        for f in (zero4, zero6, NO_FILTER):
            add_probe(f, pt, "c", kind, dst)
    # (d) one key slot per filter in an order that is not the ids'; the slots behind the map keep "no filter"
    ids = sorted(filters) + [GAP_ID, NEVER_SET, NO_FILTER]
    order = np.random.default_rng(SEED + 1).permutation(len(ids))
    slot_ids = [ids[int(k)] for k in order]
    slot_of = {f: s for s, f in enumerate(slot_ids)}
    assert len(slot_ids) < KEY_SLOTS - 1
    return Cases(filters, names, slot_of, slot_ids, 77, probes, b_kinds)



def filter_of(c: Cases, fid: int):
    """The oracle's filter behind a filter id: None for NO_FILTER, an empty IPFilter for an id never set."""
    if fid == NO_FILTER:
        return None
    return oracle_filter(c.filters.get(fid, []))


def closed_form(prefixes, dst: bytes) -> bool:
    """IPFilter.search without a trie: some inserted prefix of the destination's family, shorter than the address,
    equals the destination in its first prefix_len bits."""
    nbits = len(dst) * 8
    d = int.from_bytes(dst, "big")
    for a, p in prefixes:
        if len(a.packed) == len(dst) and p < nbits and (int.from_bytes(a.packed, "big") ^ d) >> (nbits - p) == 0:
            return True
    return False


# ---- layouts --------------------------------------------------------------------------------------------------------
def layout(lengths, tag: int = 16, unaligned: bool = False):
    """(offsets, buffer size): packet i owns [off, off + len + tag); at least GAP sentinel bytes lie before the first
    packet, between any two and behind the last. unaligned: offsets at every residue mod 16, else multiples of 16."""
    lengths = np.asarray(lengths, np.int64)
    stride = ((lengths + tag + GAP + 15) // 16) * 16 + 16
    off = np.concatenate([[0], np.cumsum(stride)[:-1]]).astype(np.int64) + 16
    if unaligned:
        off += (np.arange(len(lengths)) * 7 + 1) % 16
    return off.astype(np.uint64), int(stride.sum()) + 48
