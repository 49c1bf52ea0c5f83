"""Plain-Python restatement of wg_blake2s_batch, wg_hs_key_set and wg_hs_check (include/wgaead.h), one
message at a time, on the standard library's hashlib.blake2s.
"""
from __future__ import annotations

import hashlib

import numpy as np

B2S_OK, B2S_BADDESC = 0, 1
HS_OK, HS_BADLEN, HS_BADTYPE, HS_BADMAC1, HS_BADMAC2 = 0, 1, 2, 3, 4
INIT_SIZE, RESP_SIZE = 148, 92

B2S_DESC = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("key_off", "<u8"), ("len", "<u4"), ("outlen", "u1"),
                     ("keylen", "u1"), ("_pad", "u1", (2,))])
HS_RECORD = np.dtype([("index", "<u4"), ("len", "<u4"), ("msg", "u1", (148,)), ("_pad", "<u4")])


def blake2s(data: bytes, key: bytes = b"", outlen: int = 32) -> bytes:
    """BLAKE2s (RFC 7693), sequential mode: what Crypto.BLAKE2s256 and new Blake2s(outlen, key) compute."""
    return hashlib.blake2s(bytes(data), digest_size=outlen, key=bytes(key)).digest()


def mac1_key(static_public: bytes) -> bytes:
    """InitiationPacket.java:111-115: BLAKE2s-256("mac1----" || static public key)."""
    return blake2s(b"mac1----" + bytes(static_public))


def mac1(message_without_macs: bytes, static_public: bytes) -> bytes:
    """InitiationPacket.calculateMac1: BLAKE2s-128 of the message without its MACs under the mac1 key."""
    return blake2s(message_without_macs, mac1_key(static_public), 16)


def message(t: int, body: bytes, static_public: bytes) -> bytes:
    """A handshake message of type t (1: 148 B, 2: 92 B) with a correct mac1 and a zero mac2; `body` fills
    everything behind the type byte up to the MACs (cut or zero-padded to fit)."""
    L = INIT_SIZE if t == 1 else RESP_SIZE
    head = (bytes([t]) + bytes(body))[:L - 32].ljust(L - 32, b"\0")
    return head + mac1(head, static_public) + bytes(16)


def b2s_batch(desc, inp: bytes, out: bytes):
    """Returns (out after the call, status list). desc: B2S_DESC array."""
    inp, out = bytes(inp), bytearray(out)
    status = []
    for d in desc:
        io, oo, ko = int(d["in_off"]), int(d["out_off"]), int(d["key_off"])
        ln, ol, kl = int(d["len"]), int(d["outlen"]), int(d["keylen"])
        ok = (1 <= ol <= 32 and kl <= 32 and io <= len(inp) and ln <= len(inp) - io and ko <= len(inp)
              and kl <= len(inp) - ko and oo <= len(out) and ol <= len(out) - oo)
        if not ok:
            status.append(B2S_BADDESC)
            continue
        out[oo:oo + ol] = blake2s(inp[io:io + ln], inp[ko:ko + kl], ol)
        status.append(B2S_OK)
    return bytes(out), status


def check_one(wire, ws: int, pkt_off, pkt_len, n: int, i: int, key: bytes):
    """The six steps for batch index i. Returns (status, message or None)."""
    if i >= n:                                                         # 1
        return HS_BADLEN, None
    o, wl = int(pkt_off[i]), int(pkt_len[i])
    if wl == 0 or o > ws or wl > ws - o:
        return HS_BADLEN, None
    t = wire[o]                                                        # 2
    if t not in (1, 2):
        return HS_BADTYPE, None
    L = INIT_SIZE if t == 1 else RESP_SIZE                             # 3
    if wl != L:
        return HS_BADLEN, None
    msg = bytes(wire[o:o + L])
    if blake2s(msg[:L - 32], key, 16) != msg[L - 32:L - 16]:           # 4
        return HS_BADMAC1, None
    if msg[L - 16:] != bytes(16):                                      # 5
        return HS_BADMAC2, None
    return HS_OK, msg                                                  # 6


def check(wire, pkt_off, pkt_len, static_public: bytes, lst=None, wire_size=None):
    """Returns (status list by list position, records as an HS_RECORD array, summary dict(n_valid, n_init,
    n_resp, n_rejected)). lst None: the identity list; a list longer than the batch is cut to n entries."""
    wire = bytes(wire) if not isinstance(wire, (bytes, bytearray)) else wire
    ws = len(wire) if wire_size is None else wire_size
    n = len(pkt_off)
    key = mac1_key(static_public)
    lst = list(range(n)) if lst is None else [int(x) for x in lst][:n]
    status, recs = [], []
    n_init = n_resp = 0
    for i in lst:
        st, msg = check_one(wire, ws, pkt_off, pkt_len, n, i, key)
        status.append(st)
        if st == HS_OK:
            recs.append((i, len(msg), np.frombuffer(msg.ljust(148, b"\0"), np.uint8), 0))
            n_init += msg[0] == 1
            n_resp += msg[0] == 2
    records = np.zeros(len(recs), HS_RECORD)
    for j, r in enumerate(recs):
        records[j] = r
    return status, records, dict(n_valid=len(recs), n_init=int(n_init), n_resp=int(n_resp),
                                 n_rejected=len(status) - len(recs))
