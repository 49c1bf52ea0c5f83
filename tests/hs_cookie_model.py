"""Plain-Python restatement of wg_hs_admit, wg_hs_cookie_open and wg_hs_mac2 (include/wgaead.h): HChaCha20 written
out, XChaCha20-Poly1305 as HChaCha20 + the oracle's pure-Python RFC 8439 AEAD, the MACs on the standard library's
hashlib.blake2s. The ring models return every output array byte for byte, including the nonces and the cookie table
after the call. tests/test_hs_cookie.py pins the primitives to the published vectors.
"""
from __future__ import annotations

import struct

import numpy as np

import hs_model as HM
from wgtest import oracle

HS_OK, HS_BADLEN, HS_BADTYPE, HS_BADMAC1 = 0, 1, 2, 3
HS_BADSRC, HS_NONONCE, HS_NEEDCOOKIE = 5, 6, 7
CK_OK, CK_NOPENDING, CK_BADAUTH, CK_SKIPPED, CK_BADLEN = 0, 1, 2, 3, 4
MAC2_OK, MAC2_NONE, MAC2_BADDESC, MAC2_BADPEER = 0, 1, 2, 3

HS_SRC = np.dtype([("addr", "u1", (16,)), ("port", "u1", (2,)), ("family", "u1"), ("_pad", "u1", (5,))])
HS_COOKIE_REPLY = np.dtype([("index", "<u4"), ("len", "<u4"), ("msg", "u1", (64,)), ("_pad", "<u4", (2,))])
HS_LEARNED = np.dtype([("index", "<u4"), ("pending", "<u4"), ("peer", "<u4"), ("_zero", "<u4")])
HS_PENDING = np.dtype([("state", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("_zero", "<u4"),
                       ("ephemeral", "u1", (32,)), ("hash", "u1", (32,)), ("chain_key", "u1", (32,))])

M32 = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def hchacha20(key: bytes, nonce16: bytes) -> bytes:
    """draft-irtf-cfrg-xchacha-03 2.2: the 20 rounds over {constants, key, nonce16}, no final addition; words 0-3
    and 12-15."""
    assert len(key) == 32 and len(nonce16) == 16
    x = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key)) + list(struct.unpack("<4I", nonce16))

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack("<8I", *(x[0:4] + x[12:16]))


def xaead_seal(key: bytes, nonce24: bytes, pt: bytes, aad: bytes) -> bytes:
    """ct || tag"""
    assert len(nonce24) == 24
    return oracle().py_aead_seal(hchacha20(key, nonce24[:16]), bytes(4) + nonce24[16:], pt, aad)


def xaead_open(key: bytes, nonce24: bytes, sealed: bytes, aad: bytes):
    """the plaintext, or None when the tag does not verify"""
    assert len(nonce24) == 24
    return oracle().py_aead_open(hchacha20(key, nonce24[:16]), bytes(4) + nonce24[16:], sealed, aad)


def mac(key: bytes, data: bytes) -> bytes:
    return HM.blake2s(data, key, 16)


def cookie_key(static_public: bytes) -> bytes:
    return HM.blake2s(b"cookie--" + bytes(static_public))


def cookie(secret: bytes, addr: bytes, port2: bytes) -> bytes:
    """addr: 4 or 16 bytes; port2: the port's two bytes in network order"""
    return mac(secret, bytes(addr) + bytes(port2))


def cookie_of_src(secret: bytes, s) -> bytes:
    a = s["addr"].tobytes()
    return cookie(secret, a[:4] if int(s["family"]) == 4 else a, s["port"].tobytes())


def mac2(ck: bytes, message_without_mac2: bytes) -> bytes:
    return mac(ck, message_without_mac2)


def with_mac2(msg: bytes, ck: bytes) -> bytes:
    return msg[:-16] + mac2(ck, msg[:-16])


def reply(static_public: bytes, receiver: bytes, nonce24: bytes, ck: bytes, mac1: bytes) -> bytes:
    """The 64 bytes of a cookie reply from the owner of static_public to the message with this sender index and mac1."""
    return bytes([3, 0, 0, 0]) + bytes(receiver) + nonce24 + xaead_seal(cookie_key(static_public), nonce24, ck, mac1)


def admit(wire, pkt_off, pkt_len, src, nonces: bytes, static_public: bytes, secret: bytes, lst=None):
    """wg_hs_admit over a whole ring. src: HS_SRC array by batch index; nonces: 24 bytes per list position. Returns
    (status list, records as HM.HS_RECORD, summary dict, replies as HS_COOKIE_REPLY, admit summary dict, nonces after)."""
    wire = bytes(wire) if not isinstance(wire, (bytes, bytearray)) else wire
    ws, n = len(wire), len(pkt_off)
    key = HM.mac1_key(static_public)
    lst = list(range(n)) if lst is None else [int(x) for x in lst][:n]
    nonces = bytearray(nonces)
    status, recs, reps = [], [], []
    n_init = n_resp = n_non = n_bsrc = 0
    for k, i in enumerate(lst):
        st, msg = HS_BADLEN, None
        if i < n:
            o, wl = int(pkt_off[i]), int(pkt_len[i])
            if not (wl == 0 or o > ws or wl > ws - o):
                t = wire[o]
                if t not in (1, 2):
                    st = HS_BADTYPE
                elif wl == (148 if t == 1 else 92):
                    msg = bytes(wire[o:o + wl])
        if msg is not None:
            L = len(msg)
            if HM.blake2s(msg[:L - 32], key, 16) != msg[L - 32:L - 16]:
                st = HS_BADMAC1
            elif int(src[i]["family"]) not in (4, 6):
                st = HS_BADSRC
                n_bsrc += 1
            else:
                ck = cookie_of_src(secret, src[i])
                nonce = bytes(nonces[24 * k:24 * k + 24])
                if mac2(ck, msg[:L - 16]) == msg[L - 16:]:
                    st = HS_OK
                    recs.append((i, L, np.frombuffer(msg.ljust(148, b"\0"), np.uint8), 0))
                    n_init += msg[0] == 1
                    n_resp += msg[0] == 2
                elif nonce == bytes(24):
                    st = HS_NONONCE
                    n_non += 1
                else:
                    st = HS_NEEDCOOKIE
                    r = reply(static_public, msg[4:8], nonce, ck, msg[L - 32:L - 16])
                    reps.append((i, 64, np.frombuffer(r, np.uint8), (0, 0)))
                    nonces[24 * k:24 * k + 24] = bytes(24)
        status.append(st)
    records = np.zeros(len(recs), HM.HS_RECORD)
    for j, r in enumerate(recs):
        records[j] = r
    replies = np.zeros(len(reps), HS_COOKIE_REPLY)
    for j, r in enumerate(reps):
        replies[j] = r
    return (status, records, dict(n_valid=len(recs), n_init=int(n_init), n_resp=int(n_resp), n_rejected=len(status) - len(recs)),
            replies, dict(n_replies=len(reps), n_mac2_ok=len(recs), n_nononce=n_non, n_badsrc=n_bsrc), bytes(nonces))


def cookie_open(wire, pkt_off, pkt_len, sent, pending, publics, table):
    """wg_hs_cookie_open over a whole ring. sent: HM.HS_RECORD array; pending: HS_PENDING array; publics: the peer
    table's keys; table: list of (cookie bytes, have) per peer. Returns (status list by batch index, learned as
    HS_LEARNED, summary dict, table after)."""
    wire = bytes(wire) if not isinstance(wire, (bytes, bytearray)) else wire
    ws, n = len(wire), len(pkt_off)
    live = {}
    for p in range(len(pending)):
        if int(pending[p]["state"]) == 1 and int(pending[p]["peer"]) < len(publics):
            live.setdefault(int(pending[p]["local_index"]), p)  # the lowest position wins
    table = [(bytes(c), bool(h)) for c, h in table]
    status, learned, stored = [], [], set()
    for i in range(n):
        o, wl = int(pkt_off[i]), int(pkt_len[i])
        if wl == 0 or o > ws or wl > ws - o:
            status.append(CK_BADLEN)
            continue
        if wire[o] != 3:
            status.append(CK_SKIPPED)
            continue
        if wl != 64:
            status.append(CK_BADLEN)
            continue
        msg = bytes(wire[o:o + 64])
        p = live.get(struct.unpack("<I", msg[4:8])[0])
        if p is None:
            status.append(CK_NOPENDING)
            continue
        peer = int(pending[p]["peer"])
        ck = xaead_open(cookie_key(publics[peer]), msg[8:32], msg[32:64], sent[p]["msg"].tobytes()[116:132])
        if ck is None:
            status.append(CK_BADAUTH)
            continue
        status.append(CK_OK)
        learned.append((i, p, peer, 0))
        if peer not in stored:  # the lowest batch index of a peer is the one stored
            stored.add(peer)
            table[peer] = (ck, True)
    out = np.zeros(len(learned), HS_LEARNED)
    for j, r in enumerate(learned):
        out[j] = r
    return (status, out, dict(n_ok=len(learned), n_nopending=status.count(CK_NOPENDING), n_badauth=status.count(CK_BADAUTH),
                              n_skipped=status.count(CK_SKIPPED)), table)


def mac2_batch(records, peer, table):
    """wg_hs_mac2. records: HM.HS_RECORD array; table as cookie_open takes it. Returns (records after, status list,
    summary dict)."""
    records = records.copy()
    status = []
    for k in range(len(records)):
        L = int(records[k]["len"])
        if L not in (148, 92):
            status.append(MAC2_BADDESC)
        elif int(peer[k]) >= len(table):
            status.append(MAC2_BADPEER)
        elif not table[int(peer[k])][1]:
            status.append(MAC2_NONE)
        else:
            status.append(MAC2_OK)
            m = records[k]["msg"].tobytes()
            records[k]["msg"][L - 16:L] = np.frombuffer(mac2(table[int(peer[k])][0], m[:L - 16]), np.uint8)
    return records, status, dict(n_ok=status.count(MAC2_OK), n_none=status.count(MAC2_NONE),
                                 n_bad=status.count(MAC2_BADDESC) + status.count(MAC2_BADPEER))
