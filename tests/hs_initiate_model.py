"""Plain-Python restatement of wg_hs_initiate and wg_hs_finish (include/wgaead.h), one entry at a time, on
hs_open_model.initiate, hs_respond_model.consume_response, hs_model.mac1 and x25519_model's ladder, and a
restatement of the responder that takes a psk (hs_respond_model.respond_one hard-codes the reference's zero).
Nothing here shares a line with the library's kernels.
"""
from __future__ import annotations

import numpy as np

import hs_model as HM
import hs_open_model as OM
import hs_respond_model as RM
import x25519_model as XM
from wgtest import oracle

INIT_OK, INIT_BADPEER, INIT_NOEPH = 0, 1, 2
FIN_OK, FIN_NOPENDING, FIN_BADAUTH, FIN_SKIPPED, FIN_BADDESC = 0, 1, 2, 3, 4
HS_PENDING = np.dtype([("state", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("_zero", "<u4"),
                       ("ephemeral", "u1", (32,)), ("hash", "u1", (32,)), ("chain_key", "u1", (32,))])
HS_ESTABLISHED = np.dtype([("index", "<u4"), ("record", "<u4"), ("pending", "<u4"), ("peer", "<u4"),
                           ("local_index", "<u4"), ("remote_index", "<u4"), ("_zero", "<u4", (2,)),
                           ("send_key", "u1", (32,)), ("recv_key", "u1", (32,))])
assert HS_PENDING.itemsize == 112 and HS_ESTABLISHED.itemsize == 96


def initiate_one(local_private: bytes, remote_public: bytes, ephemeral: bytes, timestamp: bytes, local_index: int):
    """The 148-byte initiation (OutgoingInitiation.java:22-38, InitiationPacket.java:110-120) and the state
    consumeMessageResponse goes on from. Returns dict(message, hash, chain_key)."""
    init = OM.initiate(local_private, remote_public, ephemeral, timestamp)
    head = bytes([1]) + OM.body(local_index, init)
    assert len(head) == 116
    return dict(message=head + HM.mac1(head, remote_public) + bytes(16), hash=init["hash"], chain_key=init["chain_key"])


def initiate_batch(local_private: bytes, peers, peer, ephemerals: bytes, timestamps: bytes, local_index, n: int, status,
                   records: bytes, pending: bytes, summary):
    """wg_hs_initiate. peers: the static public keys of wg_hs_peers_set. ephemerals / status / records / pending /
    summary: what the five outputs hold before the call. Returns them after it: (ephemerals, status list, records
    bytes, pending bytes, summary list); what lies behind n keeps what it held."""
    eph, st, rec, pend = bytearray(ephemerals), list(status), bytearray(records), bytearray(pending)
    if n == 0:
        return bytes(eph), st, bytes(rec), bytes(pend), list(summary)
    counts = [0, 0, 0]
    for k in range(n):
        raw = bytes(eph[32 * k:32 * k + 32])
        if int(peer[k]) >= len(peers):
            st[k] = INIT_BADPEER
        elif raw == bytes(32):
            st[k] = INIT_NOEPH
        else:
            st[k] = INIT_OK
        counts[st[k]] += 1
        r, p = np.zeros(1, HM.HS_RECORD), np.zeros(1, HS_PENDING)
        if st[k] == INIT_OK:
            li = int(local_index[k]) & 0xFFFFFFFF
            one = initiate_one(local_private, bytes(peers[int(peer[k])]), raw, bytes(timestamps[12 * k:12 * k + 12]), li)
            r["index"], r["len"] = k, 148
            r["msg"][0] = np.frombuffer(one["message"], np.uint8)
            p["state"], p["peer"], p["local_index"] = 1, int(peer[k]), li
            p["ephemeral"][0] = np.frombuffer(raw, np.uint8)
            p["hash"][0] = np.frombuffer(one["hash"], np.uint8)
            p["chain_key"][0] = np.frombuffer(one["chain_key"], np.uint8)
            eph[32 * k:32 * k + 32] = bytes(32)
        rec[160 * k:160 * k + 160] = r.tobytes()
        pend[112 * k:112 * k + 112] = p.tobytes()
    return bytes(eph), st, bytes(rec), bytes(pend), counts + [0]


def finish_batch(local_private: bytes, n_peers: int, psks, records, n_records, n: int, pending: bytes, n_pending: int,
                 fin_status, established: bytes, summary):
    """wg_hs_finish over an HS_RECORD array. psks: 32 bytes per peer. n_records None: all n. pending / fin_status /
    established / summary: what the four outputs hold before the call. Returns them after it: (pending bytes, status
    list, established bytes, summary list)."""
    pend, st, out = bytearray(pending), list(fin_status), bytearray(established)
    if n == 0:
        return bytes(pend), st, bytes(out), list(summary)
    before = np.frombuffer(bytes(pending[:112 * n_pending]), HS_PENDING)  # every record sees the entries as the call found them
    cover = n if n_records is None else min(int(n_records), n)
    n_ok = n_nop = n_bad = n_skip = 0
    consumed = []
    for k in range(cover):
        ln = int(records[k]["len"])
        msg = records[k]["msg"].tobytes()
        if ln == 148:
            st[k] = FIN_SKIPPED
            n_skip += 1
            continue
        if ln != 92:
            st[k] = FIN_BADDESC
            continue
        receiver = int.from_bytes(msg[8:12], "little")
        pos = next((p for p in range(n_pending) if int(before[p]["state"]) == 1 and int(before[p]["peer"]) < n_peers and
                    int(before[p]["local_index"]) == receiver), None)
        if pos is None:
            st[k] = FIN_NOPENDING
            n_nop += 1
            continue
        e = before[pos]
        keys = RM.consume_response(local_private, e["ephemeral"].tobytes(), e["hash"].tobytes(), e["chain_key"].tobytes(),
                                   msg[12:44], msg[44:60], bytes(psks[int(e["peer"])]))
        if keys is None:
            st[k] = FIN_BADAUTH
            n_bad += 1
            continue
        st[k] = FIN_OK
        s = np.zeros(1, HS_ESTABLISHED)
        s["index"], s["record"], s["pending"], s["peer"] = records[k]["index"], k, pos, e["peer"]
        s["local_index"], s["remote_index"] = receiver, int.from_bytes(msg[4:8], "little")
        s["send_key"][0] = np.frombuffer(keys["send_key"], np.uint8)
        s["recv_key"][0] = np.frombuffer(keys["recv_key"], np.uint8)
        out[96 * n_ok:96 * n_ok + 96] = s.tobytes()
        n_ok += 1
        consumed.append(pos)
    for pos in consumed:
        pend[112 * pos:112 * pos + 112] = bytes(112)
    return bytes(pend), st, bytes(out), [n_ok, n_nop, n_bad, n_skip]


def respond_psk(hash_: bytes, chain_key: bytes, remote_ephemeral: bytes, remote_static: bytes, ephemeral: bytes,
                local_index: int, sender_index: int, psk: bytes):
    """hs_respond_model.respond_one with the psk as an argument (deriveKeypair, Handshakes.java:250-287, where the
    reference has the zero constant). Returns dict(response, send_key, recv_key)."""
    O = oracle()
    h, ck = bytes(hash_), bytes(chain_key)
    epub = XM.public_key(ephemeral)
    h = OM.blake2s(h, epub)
    ck = OM.derive_key(ck, epub)
    ck = OM.derive_key(ck, OM.x25519(ephemeral, remote_ephemeral))
    ck = OM.derive_key(ck, OM.x25519(ephemeral, remote_static))
    tau, key, ck = OM.derive_key(ck, psk, 2), OM.derive_key(ck, psk, 3), OM.derive_key(ck, psk, 1)
    h = OM.blake2s(h, tau)
    empty = O.py_aead_seal(key, OM.ZERO_NONCE, b"", h)
    head = bytes([2, 0, 0, 0]) + int(local_index).to_bytes(4, "little") + int(sender_index).to_bytes(4, "little") + epub + empty
    return dict(response=head + HM.mac1(head, remote_static) + bytes(16), send_key=OM.derive_key(ck, b"", 2),
                recv_key=OM.derive_key(ck, b"", 1))


def answer(responder_private: bytes, initiator_public: bytes, message: bytes, ephemeral: bytes, local_index: int,
           psk: bytes = bytes(32)):
    """The model responder's answer to a 148-byte initiation of a known initiator: decryptRemoteStatic
    (hs_open_model.open_one) and respond_psk. Returns dict(response, send_key, recv_key)."""
    ss = OM.x25519(responder_private, message[8:40])
    st, res = OM.open_one(responder_private, XM.public_key(responder_private), message[8:40], message[40:88], message[88:116],
                          ss, [initiator_public])
    assert st == OM.OPEN_OK, st
    return respond_psk(res["hash"], res["chain_key"], message[8:40], res["remote_static"], ephemeral, local_index,
                       int.from_bytes(message[4:8], "little"), psk)
