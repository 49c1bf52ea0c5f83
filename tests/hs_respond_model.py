"""Plain-Python restatement of ResponderHandshake.deriveKeypair, the response message, wg_hs_respond
(include/wgaead.h) and InitiatorStageOne.consumeMessageResponse, one initiation at a time: hs_open_model's BLAKE2s,
HMAC and HKDF, x25519_model's ladder, the oracle's Python ChaCha20-Poly1305, hs_model's mac1. Nothing here shares a
line with the library's kernels.
"""
from __future__ import annotations

import numpy as np

import hs_model as HM
import hs_open_model as OM
import x25519_model as XM
from wgtest import oracle

RESP_OK, RESP_NOPEER, RESP_NOEPH = 0, 1, 2
SKIP_NEWPEER = 1
NOPEER = OM.NOPEER
HS_SESSION = np.dtype([("index", "<u4"), ("init", "<u4"), ("peer", "<u4"), ("local_index", "<u4"),
                       ("response", "u1", (92,)), ("remote_index", "<u4"), ("send_key", "u1", (32,)),
                       ("recv_key", "u1", (32,))])
PSK = bytes(32)  # Handshakes.java:262
assert HS_SESSION.itemsize == 176


def respond_one(hash_: bytes, chain_key: bytes, remote_ephemeral: bytes, remote_static: bytes, ephemeral: bytes,
                local_index: int, sender_index: int):
    """deriveKeypair (Handshakes.java:250-287) and the response (ResponsePacket.java:107-117) from the state
    decryptRemoteStatic left, with the ephemeral private key passed in (clamped by the ladder). Returns
    dict(response, send_key, recv_key, ephemeral_public, encrypted_empty, hash)."""
    O = oracle()
    h, ck = bytes(hash_), bytes(chain_key)
    epub = XM.public_key(ephemeral)
    h = OM.blake2s(h, epub)
    ck = OM.derive_key(ck, epub)
    ck = OM.derive_key(ck, OM.x25519(ephemeral, remote_ephemeral))
    ck = OM.derive_key(ck, OM.x25519(ephemeral, remote_static))
    tau, key, ck = OM.derive_key(ck, PSK, 2), OM.derive_key(ck, PSK, 3), OM.derive_key(ck, PSK, 1)
    h = OM.blake2s(h, tau)
    empty = O.py_aead_seal(key, OM.ZERO_NONCE, b"", h)
    assert len(empty) == 16
    h = OM.blake2s(h, empty)
    recv_key, send_key = OM.derive_key(ck, b"", 1), OM.derive_key(ck, b"", 2)  # :286
    head = bytes([2, 0, 0, 0]) + int(local_index).to_bytes(4, "little") + int(sender_index).to_bytes(4, "little") + epub + empty
    response = head + HM.mac1(head, remote_static) + bytes(16)
    assert len(response) == 92
    return dict(response=response, send_key=send_key, recv_key=recv_key, ephemeral_public=epub, encrypted_empty=empty, hash=h)


def respond_batch(inits, n_inits, n: int, ephemerals: bytes, local_index, flags: int, resp_status, sessions: bytes, summary):
    """wg_hs_respond over an HS_INIT array. n_inits None: all n. ephemerals / resp_status / sessions / summary: what
    the four outputs hold before the call. Returns (ephemerals, resp_status list, sessions bytes, summary list) after
    it: a consumed ephemeral is zero, a non-OK entry's and those behind min(n_inits, n) keep what they held, as do
    statuses behind the cover and sessions behind n_ok."""
    assert not flags & ~SKIP_NEWPEER
    eph, st, out = bytearray(ephemerals), list(resp_status), bytearray(sessions)
    if n == 0:
        return bytes(eph), st, bytes(out), list(summary)
    cover = n if n_inits is None else min(int(n_inits), n)
    n_ok = n_nopeer = n_noeph = 0
    for k in range(cover):
        e = inits[k]
        raw = bytes(eph[32 * k:32 * k + 32])
        if flags & SKIP_NEWPEER and int(e["peer"]) == NOPEER:
            st[k] = RESP_NOPEER
            n_nopeer += 1
        elif raw == bytes(32):
            st[k] = RESP_NOEPH
            n_noeph += 1
        else:
            st[k] = RESP_OK
            r = respond_one(e["hash"].tobytes(), e["chain_key"].tobytes(), e["remote_ephemeral"].tobytes(),
                            e["remote_static"].tobytes(), raw, int(local_index[k]), int(e["sender_index"]))
            s = np.zeros(1, HS_SESSION)
            s["index"], s["init"], s["peer"], s["local_index"] = e["index"], k, e["peer"], int(local_index[k])
            s["response"][0] = np.frombuffer(r["response"], np.uint8)
            s["remote_index"] = e["sender_index"]
            s["send_key"][0] = np.frombuffer(r["send_key"], np.uint8)
            s["recv_key"][0] = np.frombuffer(r["recv_key"], np.uint8)
            out[176 * n_ok:176 * n_ok + 176] = s.tobytes()
            eph[32 * k:32 * k + 32] = bytes(32)
            n_ok += 1
    return bytes(eph), st, bytes(out), [n_ok, n_nopeer, n_noeph, 0]


def consume_response(local_private: bytes, ephemeral_private: bytes, hash_: bytes, chain_key: bytes,
                     remote_ephemeral: bytes, encrypted_empty: bytes, psk: bytes = PSK):
    """InitiatorStageOne.consumeMessageResponse (Handshakes.java:119-151), continuing from hs_open_model.initiate's
    hash / chain_key. Returns None when encrypted_empty does not verify, else dict(send_key, recv_key): the
    initiator sends with T1 and receives with T2 (:147)."""
    O = oracle()
    h, ck = bytes(hash_), bytes(chain_key)
    h = OM.blake2s(h, remote_ephemeral)
    ck = OM.derive_key(ck, remote_ephemeral)
    ck = OM.derive_key(ck, OM.x25519(ephemeral_private, remote_ephemeral))
    ck = OM.derive_key(ck, OM.x25519(local_private, remote_ephemeral))
    tau, key, ck = OM.derive_key(ck, psk, 2), OM.derive_key(ck, psk, 3), OM.derive_key(ck, psk, 1)
    h = OM.blake2s(h, tau)
    if O.py_aead_open(key, OM.ZERO_NONCE, bytes(encrypted_empty), h) is None:
        return None
    return dict(send_key=OM.derive_key(ck, b"", 1), recv_key=OM.derive_key(ck, b"", 2))
