"""Plain-Python restatement of wg_hs_stamp, wg_hs_stamps_set and wg_hs_stamps_get (include/wgaead.h): the chain that
leads to the timestamp's key on hs_open_model's blake2s / derive_key, the oracle's Python ChaCha20-Poly1305 and
x25519_model's ladder; the rule over a batch; and k_hs_stamp_chain's lane as an interpretation of kStampProgram
(wireguard-java_amd/csrc/wg_hs_chain.h) on hs_chain_model's machine. Nothing here shares a line with the library's
kernels.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import hs_chain_model as CM
import hs_open_model as OM
from wgtest import oracle

TS_OK, TS_REPLAY, TS_SUPERSEDED, TS_BADAUTH, TS_NOPEER, TS_BADDESC = 0, 1, 2, 3, 4, 5
NOPEER = OM.NOPEER
ZERO_TS = bytes(12)


def timestamp_key(local_public: bytes, ephemeral: bytes, enc_static: bytes, ss: bytes, ss_p: bytes):
    """(k, h) of the header's chain: the key of encrypted_timestamp and its aad."""
    h = OM.blake2s(OM.blake2s(OM.blake2s(OM.INITIAL_HASH, local_public), ephemeral), enc_static)
    ck = OM.derive_key(OM.derive_key(OM.INITIAL_CHAIN_KEY, ephemeral), ss)
    return OM.derive_key(ck, ss_p, 2), h


def open_timestamp(local_public: bytes, msg: bytes, ss: bytes, ss_p: bytes):
    """The 12 bytes of a 148-byte initiation's timestamp, or None when its tag does not verify."""
    k, h = timestamp_key(local_public, msg[8:40], msg[40:88], ss, ss_p)
    return oracle().py_aead_open(k, OM.ZERO_NONCE, bytes(msg[88:116]), h)


def rule(entries, stored):
    """Steps 4-6 over the entries that passed 1-3. entries: [(pre, p, T)] with pre None for such an entry and its
    final status otherwise; stored: {p: 12 bytes} (absent: zero). Returns (statuses, stored afterwards). One pass
    finds each peer's best entry: bytes compare as the 96-bit big-endian numbers they are."""
    best = {}
    for j, (pre, p, t) in enumerate(entries):
        if pre is None and t > stored.get(p, ZERO_TS) and (p not in best or t > best[p][0]):
            best[p] = (t, j)
    out, after = [], dict(stored)
    for j, (pre, p, t) in enumerate(entries):
        if pre is not None:
            out.append(pre)
        elif t <= stored.get(p, ZERO_TS):
            out.append(TS_REPLAY)
        elif best[p][1] != j:
            out.append(TS_SUPERSEDED)
        else:
            out.append(TS_OK)
            after[p] = t
    return out, after


def stamp_batch(inits, n_inits, n: int, records, n_rec: int, shared: bytes, local_private: bytes, peers, stored, x25519,
                public_key, ts_status, opened: bytes, fresh: bytes, summary):
    """wg_hs_stamp over an HS_INIT array (n entries), the HS_RECORD array and shared bytes wg_hs_open read. n_inits
    None: all n. peers: the static public keys of wg_hs_peers_set; stored: the table's timestamps, a list of 12-byte
    strings, which the call updates in place. ts_status / opened / fresh / summary: what the four outputs hold
    before the call. Returns them (status list, bytes, bytes, list) after it."""
    st, op, fr = list(ts_status), bytearray(opened), bytearray(fresh)
    if n == 0:
        return st, bytes(op), bytes(fr), list(summary)
    cover = n if n_inits is None else min(int(n_inits), n)
    local_public = public_key(local_private)
    entries = []
    for j in range(cover):
        p, r = int(inits[j]["peer"]), int(inits[j]["record"])
        if p == NOPEER:
            entries.append((TS_NOPEER, p, None))
        elif p >= len(peers) or r >= n_rec or int(records[r]["len"]) != OM.INIT_SIZE:
            entries.append((TS_BADDESC, p, None))
        else:
            t = open_timestamp(local_public, records[r]["msg"].tobytes(), bytes(shared[32 * r:32 * r + 32]),
                               x25519(local_private, bytes(peers[p])))
            entries.append((TS_BADAUTH, p, None) if t is None else (None, p, t))
    got, after = rule(entries, {p: bytes(t) for p, t in enumerate(stored)})
    n_ok = 0
    for j in range(cover):
        st[j] = got[j]
        op[12 * j:12 * j + 12] = entries[j][2] if entries[j][2] is not None else ZERO_TS
        if got[j] == TS_OK:
            fr[144 * n_ok:144 * n_ok + 144] = inits[j].tobytes()
            n_ok += 1
    for p in range(len(stored)):
        stored[p] = after[p]
    return st, bytes(op), bytes(fr), [n_ok, got.count(TS_REPLAY) + got.count(TS_SUPERSEDED), got.count(TS_BADAUTH),
                                      got.count(TS_NOPEER) + got.count(TS_BADDESC)]


def stamp_one(E, program, local_public: bytes, msg: bytes, ss: bytes, ss_p: bytes):
    """k_hs_stamp_chain's lane over one initiation: (the 12 bytes or None, the final h, the final ck)."""
    O = oracle()
    c = CM.new_chain()
    c.ist = CM.compress(CM.init(32), CM.words(bytes(b ^ 0x36 for b in CM.CK0) + b"\x36" * 32, 16), 64, False)  # kCk0Ipad
    c.ost = CM.compress(CM.init(32), CM.words(bytes(b ^ 0x5C for b in CM.CK0) + b"\x5c" * 32, 16), 64, False)  # kCk0Opad
    hs0 = CM.octets(CM.blake2s(CM.H0 + bytes(local_public)))
    eph, es, ets = msg[8:40], msg[40:88], msg[88:116]
    lane = SimpleNamespace(ts=None)

    def op_h0(c, s):
        c.m, c.st, c.t, c.last = CM.words(hs0 + eph, 16), CM.init(32), 64, True

    def op_ses1(c, s):
        c.m, c.st, c.t, c.last = list(c.hh) + CM.words(es[:32], 8), CM.init(32), 64, False

    def op_es2(c, s):
        c.m, c.t, c.last = CM.words(es[32:48], 16), 80, True

    def op_sts(c, s):
        lane.ts = O.py_aead_open(CM.octets(c.st), CM.ZERO_NONCE, bytes(ets), CM.octets(c.hh))
        c.m, c.st, c.t, c.last = list(c.hh) + CM.words(ets, 8), CM.init(32), 60, True

    CM.run(E, program, c, {E.SRC_E: eph, E.SRC_SS: ss, E.SRC_STATIC: ss_p},
           {E.OP_H0: op_h0, E.OP_SES1: op_ses1, E.OP_ES2: op_es2, E.OP_STS: op_sts})
    return lane.ts, CM.octets(c.hh), CM.octets(c.ck)
