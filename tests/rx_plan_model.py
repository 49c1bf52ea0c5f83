"""Plain-Python restatement of wg_rx_plan and wg_rx_deliver (include/wgaead.h): which class a datagram
is, which session opens it, where its plaintext goes and what is written to the tun device, one packet
at a time.

The session table is a ``dict`` (receiver index -> key slot), so the expectation does not depend on the
library's hash table.
"""
from __future__ import annotations

import struct

import numpy as np

PKT_OK, PKT_BADTAG, PKT_BADHDR, PKT_KEEPALIVE, PKT_BADIP, PKT_FILTERED, PKT_REPLAY = 0, 1, 2, 3, 4, 5, 6
PKT_TOOLONG, PKT_NOSESSION, PKT_HANDSHAKE = 9, 10, 11
LEN_INVALID = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
PT_AFTER, PT_PACKED = 0, 1

WG_PKT = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("key_slot", "<u4")])
RX_ITEM = np.dtype([("off", "<u8"), ("len", "<u4"), ("key_slot", "<u4")])


def align16(x: int) -> int:
    return (x + 15) & ~15


def plan(wire, pkt_off, pkt_len, sessions: dict, *, max_len, mode, pt_base=0, pt_size=0, wire_size=None):
    """Returns (desc as a WG_PKT array, status list, host_list, summary dict(pt_used, n_open, n_host))."""
    wire = bytes(wire) if not isinstance(wire, (bytes, bytearray)) else wire
    ws = len(wire) if wire_size is None else wire_size
    n = len(pkt_off)
    desc = np.zeros(n, WG_PKT)
    status, host = [0] * n, []
    C = 0
    for i in range(n):
        o, wl = int(pkt_off[i]), int(pkt_len[i])
        fail_out = (o + wl) & MASK64 if mode == PT_AFTER else pt_base
        slot = 0

        def verdict():
            nonlocal slot, C
            if wl == 0 or o > ws or wl > ws - o:                       # 1
                return PKT_BADHDR, None
            t = wire[o]                                                # 2
            if t in (1, 2):
                return PKT_HANDSHAKE, None
            if t != 4:
                return PKT_BADHDR, None
            if wl < 32:                                                # 3
                return PKT_BADHDR, None
            ln = wl - 32
            index = struct.unpack_from("<I", wire, o + 4)[0]           # 4
            if index not in sessions:
                return PKT_NOSESSION, None
            slot = sessions[index]
            if ln > max_len:                                           # 5
                return PKT_TOOLONG, None
            if mode == PT_AFTER:                                       # 6
                if o + wl + ln > ws:
                    return PKT_BADHDR, None
                return PKT_OK, o + wl
            out = pt_base + C
            C += align16(ln)
            if out + ln > pt_size:
                return PKT_TOOLONG, None
            return PKT_OK, out

        st, out = verdict()
        status[i] = st
        if st == PKT_OK:
            ctr = struct.unpack_from("<Q", wire, o + 8)[0]
            desc[i] = ((o + 16) & MASK64, out & MASK64, ctr, wl - 32, slot)
        else:
            desc[i] = ((o + 16) & MASK64, fail_out & MASK64, 0, LEN_INVALID, slot)
        if st == PKT_HANDSHAKE:
            host.append(i)
    return desc, status, host, dict(pt_used=C, n_open=status.count(PKT_OK), n_host=len(host))


def deliver(desc, plan_status, open_status):
    """Returns (final status list, items as an RX_ITEM array, index list, dict(bytes, n_items, n_keepalive))."""
    final = [int(p) if int(p) != PKT_OK else int(q) for p, q in zip(plan_status, open_status)]
    idx = [i for i, f in enumerate(final) if f == PKT_OK]
    items = np.zeros(len(idx), RX_ITEM)
    for j, i in enumerate(idx):
        items[j] = (int(desc[i]["out_off"]), int(desc[i]["len"]), int(desc[i]["key_slot"]))
    return final, items, idx, dict(bytes=int(sum(int(desc[i]["len"]) for i in idx)), n_items=len(idx),
                                   n_keepalive=final.count(PKT_KEEPALIVE))
