"""Plain-Python restatement of wg_tx_plan (include/wgaead.h): which peers get a tun packet, which
send counter it takes and where its wire packet goes, one packet at a time.

The longest-prefix match is Python's ``ipaddress`` module (the longest ``network`` containing the
address, the later entry on ties), so the expected routing does not depend on the library's trie.
"""
from __future__ import annotations

import ipaddress

import numpy as np

PKT_OK, PKT_BADIP, PKT_NOROUTE, PKT_TOOLONG = 0, 4, 8, 9
LEN_INVALID = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
BROADCAST, ROUTE = 0, 1

WG_PKT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("key_slot", "<u4")])


class RouteTable:
    """(address, prefix_len, key_slot) triples; lookup = longest prefix, later entry on ties."""

    def __init__(self, routes):
        self.nets = {}  # ipaddress network -> key slot (a later equal prefix replaces the earlier)
        for addr, plen, slot in routes:
            a = ipaddress.ip_address(addr) if isinstance(addr, str) else addr
            self.nets[ipaddress.ip_network((a, plen), strict=False)] = int(slot)
        # prefix lengths present per family, longest first
        self.lens = {v: sorted({n.prefixlen for n in self.nets if n.version == v}, reverse=True) for v in (4, 6)}
        self._memo = {}

    def lookup(self, dst: bytes):
        """Key slot of the longest network that contains dst (4 or 16 address bytes), or None."""
        if dst not in self._memo:
            a = ipaddress.ip_address(dst)
            hit = None
            for plen in self.lens[a.version]:  # the network of that length containing a, if it is a route
                hit = self.nets.get(ipaddress.ip_network((a, plen), strict=False))
                if hit is not None:
                    break
            self._memo[dst] = hit
        return self._memo[dst]


def destination(pkt: bytes):
    """destinationIPOf (TransportManager.java:124-130): the address bytes, or None where it throws."""
    if not pkt:
        return None
    ver = pkt[0] >> 4
    if ver == 4:
        at, nb = 16, 4
    elif ver == 6:
        at, nb = 24, 16
    else:
        return None
    return bytes(pkt[at:at + nb]) if len(pkt) >= at + nb else None


def plan(pkt_off, pkt_len, ring, mode, counters, *, peers=None, routes: RouteTable | None = None, wire_stride,
         out_size, max_len, wire_base=0, in_size=None):
    """Returns (desc as a WG_PKT array, status list, new counters dict). `counters`: slot -> send
    counter (missing: 0); `ring`: the tun ring as bytes / uint8 array."""
    ring = bytes(ring) if not isinstance(ring, (bytes, bytearray)) else ring
    in_size = len(ring) if in_size is None else in_size
    n = len(pkt_off)
    peers = list(peers or [])
    per = 1 if mode == ROUTE else len(peers)
    send = dict(counters)
    desc = np.zeros(n * per, WG_PKT)
    status = [0] * (n * per)
    slots_fit = (out_size - wire_base) // wire_stride if wire_stride and wire_base <= out_size else 0

    def put(j, off, ln, slot, ctr, st):
        desc[j] = (off & MASK64, (wire_base + j * wire_stride + 16) & MASK64, ctr & MASK64, ln, slot)
        status[j] = st

    for t in range(n):
        off, ln = int(pkt_off[t]), int(pkt_len[t])
        fits = (ln <= max_len and off + ln <= in_size and ln + 32 <= wire_stride and (t + 1) * per <= slots_fit)
        if mode == BROADCAST:
            for p, slot in enumerate(peers):
                j = t * per + p
                if fits:
                    put(j, off, ln, slot, send.get(slot, 0), PKT_OK)
                    send[slot] = (send.get(slot, 0) + 1) & MASK64
                else:
                    put(j, off, LEN_INVALID, slot, 0, PKT_TOOLONG)
            continue
        if not fits:
            put(t, off, LEN_INVALID, 0, 0, PKT_TOOLONG)
            continue
        dst = destination(ring[off:off + ln])
        if dst is None:
            put(t, off, LEN_INVALID, 0, 0, PKT_BADIP)
            continue
        slot = routes.lookup(dst) if routes is not None else None
        if slot is None:
            put(t, off, LEN_INVALID, 0, 0, PKT_NOROUTE)
            continue
        put(t, off, ln, slot, send.get(slot, 0), PKT_OK)
        send[slot] = (send.get(slot, 0) + 1) & MASK64
    return desc, status, send
