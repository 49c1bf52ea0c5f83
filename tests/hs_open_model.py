"""Plain-Python restatement of Handshakes.InitiatorStageOne, Handshakes.decryptRemoteStatic, wg_hs_peers_set and
wg_hs_open (include/wgaead.h), one initiation at a time: hashlib's BLAKE2s, HMAC and HKDF written out as
Crypto.java:39-99 does them, the oracle's Python ChaCha20-Poly1305, x25519_model's ladder. Nothing here shares a
line with the library's kernels.
"""
from __future__ import annotations

import hashlib

import numpy as np

import x25519_model as XM
from wgtest import oracle

OPEN_OK, OPEN_NEWPEER, OPEN_BADAUTH, OPEN_SKIPPED, OPEN_BADDESC = 0, 1, 2, 3, 4
NOPEER = 0xFFFFFFFF
INIT_SIZE, RESP_SIZE = 148, 92
HS_INIT = np.dtype([("index", "<u4"), ("record", "<u4"), ("sender_index", "<u4"), ("peer", "<u4"),
                    ("remote_ephemeral", "u1", (32,)), ("remote_static", "u1", (32,)), ("hash", "u1", (32,)),
                    ("chain_key", "u1", (32,))])
ZERO_NONCE = bytes(12)
BLOCK = 64


def blake2s(*data: bytes) -> bytes:
    """Crypto.BLAKE2s256."""
    return hashlib.blake2s(b"".join(bytes(d) for d in data)).digest()


# Handshakes.java:20-37
INITIAL_CHAIN_KEY = blake2s(b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s")
INITIAL_HASH = blake2s(INITIAL_CHAIN_KEY, b"WireGuard v1 zx2c4 Jason@zx2c4.com")


def hmac(key: bytes, *messages: bytes) -> bytes:
    """Crypto.HMAC (Crypto.java:39-71) with a 32-byte sum."""
    k = blake2s(key) if len(key) > BLOCK else bytes(key)
    padded = k.ljust(BLOCK, b"\0")
    inner = blake2s(bytes(b ^ 0x36 for b in padded), *messages)
    return blake2s(bytes(b ^ 0x5C for b in padded), inner)


def derive_key(salt: bytes, ikm: bytes, n: int = 1) -> bytes:
    """Crypto.deriveKey (Crypto.java:74-99): HKDF_Expand(HKDF_Extract(salt, IKM), info = empty, n)[n - 1]."""
    prk = hmac(salt, ikm)
    t = b""
    for i in range(1, n + 1):
        t = hmac(prk, t, b"", bytes([i]))
    return t


def x25519(scalar: bytes, point: bytes) -> bytes:
    return XM.x25519(bytes(scalar), bytes(point))  # (through the module: a test may memoise it)


def initiate(local_private: bytes, remote_public: bytes, ephemeral_private: bytes | None, timestamp: bytes, *,
             ephemeral_public: bytes | None = None, es_secret: bytes | None = None, static_public: bytes | None = None):
    """InitiatorStageOne's constructor (Handshakes.java:77-117) with the ephemeral and the 12-byte timestamp
    passed in. ephemeral_public and es_secret replace what the ladder gives for ephemeral_private: an
    initiation whose ephemeral is a low-order point, which no private key has, sealed under the all-zero
    secret that the responder computes for it. static_public replaces the 32 bytes that are sealed as the
    initiator's static key (the same key with bit 255 set; a low-order point): the responder then continues
    from those bytes, so only its side of the chain is defined. Returns dict(ephemeral, encrypted_static,
    encrypted_timestamp, hash, chain_key)."""
    O = oracle()
    h, ck = INITIAL_HASH, INITIAL_CHAIN_KEY
    eph = ephemeral_public if ephemeral_public is not None else XM.public_key(ephemeral_private)
    h = blake2s(h, remote_public)
    ck = derive_key(ck, eph)
    h = blake2s(h, eph)
    es = es_secret if es_secret is not None else x25519(ephemeral_private, remote_public)
    key, ck = derive_key(ck, es, 2), derive_key(ck, es, 1)
    enc_static = O.py_aead_seal(key, ZERO_NONCE, static_public if static_public is not None else XM.public_key(local_private), h)
    h = blake2s(h, enc_static)
    ss = x25519(local_private, remote_public)
    key, ck = derive_key(ck, ss, 2), derive_key(ck, ss, 1)
    enc_ts = O.py_aead_seal(key, ZERO_NONCE, bytes(timestamp), h)
    h = blake2s(h, enc_ts)
    assert len(enc_static) == 48 and len(enc_ts) == 28
    return dict(ephemeral=eph, encrypted_static=enc_static, encrypted_timestamp=enc_ts, hash=h, chain_key=ck)


def body(sender_index: int, init: dict, reserved: bytes = bytes(3)) -> bytes:
    """msg[1 .. 116) of the initiation (InitiationPacket.java:21-45), for hs_model.message(1, body, pub)."""
    return bytes(reserved) + int(sender_index).to_bytes(4, "little") + init["ephemeral"] + init["encrypted_static"] + \
        init["encrypted_timestamp"]


def open_one(local_private: bytes, local_public: bytes, ephemeral: bytes, enc_static: bytes, enc_ts: bytes,
             ss: bytes, peers):
    """ResponderHandshake.decryptRemoteStatic (Handshakes.java:201-237) as wg_hs_open states it, with ss =
    sharedSecret(remoteEphemeral) passed in. peers: the static public keys of wg_hs_peers_set. Returns (status,
    None) or (status, dict(remote_static, hash, chain_key, peer)): for a key that no peer holds the chain key
    is the one before the static-static step."""
    O = oracle()
    h = blake2s(blake2s(INITIAL_HASH, local_public), ephemeral)
    ck = derive_key(INITIAL_CHAIN_KEY, ephemeral)
    key, ck = derive_key(ck, ss, 2), derive_key(ck, ss, 1)
    remote_static = O.py_aead_open(key, ZERO_NONCE, bytes(enc_static), h)
    if remote_static is None:
        return OPEN_BADAUTH, None
    h = blake2s(h, enc_static)
    peers = [bytes(p) for p in peers]
    peer = peers.index(remote_static) if remote_static in peers else NOPEER
    if peer != NOPEER:
        ck = derive_key(ck, x25519(local_private, remote_static))
    h = blake2s(h, enc_ts)
    return (OPEN_OK if peer != NOPEER else OPEN_NEWPEER), dict(remote_static=remote_static, hash=h, chain_key=ck, peer=peer)


def open_batch(records, n_records, n: int, shared: bytes, dh_status, local_private: bytes, peers, open_status,
               inits: bytes, summary):
    """wg_hs_open over an HS_RECORD array, the shared bytes and statuses of wg_hs_dh. n_records None: all n.
    open_status / inits / summary: what the three outputs hold before the call. Returns (open_status list, inits
    bytes, summary list) after it: statuses behind min(n_records, n), and entries behind n_emitted, keep what
    they held."""
    st, out = list(open_status), bytearray(inits)
    local_public = XM.public_key(local_private)
    cover = n if n_records is None else min(int(n_records), n)
    emitted = known = bad = skipped = 0
    for k in range(cover):
        ln, ds = int(records[k]["len"]), int(dh_status[k])
        if ln == RESP_SIZE:
            s, res = OPEN_SKIPPED, None
        elif ln != INIT_SIZE:
            s, res = OPEN_BADDESC, None
        elif ds == XM.X_SKIPPED:
            s, res = OPEN_SKIPPED, None
        elif ds not in (XM.X_OK, XM.X_ZERO):
            s, res = OPEN_BADDESC, None
        else:
            msg = records[k]["msg"].tobytes()
            s, res = open_one(local_private, local_public, msg[8:40], msg[40:88], msg[88:116],
                              bytes(shared[32 * k:32 * k + 32]), peers)
        st[k] = s
        bad += s == OPEN_BADAUTH
        skipped += s == OPEN_SKIPPED
        if res is not None:
            e = np.zeros(1, HS_INIT)
            e["index"], e["record"] = records[k]["index"], k
            e["sender_index"] = int.from_bytes(records[k]["msg"][4:8].tobytes(), "little")
            e["peer"] = res["peer"]
            e["remote_ephemeral"][0] = records[k]["msg"][8:40]
            for f in ("remote_static", "hash", "chain_key"):
                e[f][0] = np.frombuffer(res[f], np.uint8)
            out[144 * emitted:144 * emitted + 144] = e.tobytes()
            emitted += 1
            known += s == OPEN_OK
    if n == 0:
        return st, bytes(out), list(summary)
    return st, bytes(out), [emitted, int(known), int(bad), int(skipped)]
