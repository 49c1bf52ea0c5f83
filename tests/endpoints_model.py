"""Plain-Python restatement of wg_endpoints_start / _learn, wg_tx_sendlist / wg_hs_sendlist and the endpoint setters
over the public image (one 24-byte wg_hs_src per peer, one peer per key slot), the judge of the device's bytes. What it
restates of the reference:

  EstablishedSession.outboundPacketAddress: every session has one address. SessionManager.java:217-229 gives a
    responder's session the initiation's origin (`start` with SRC_SESSIONS), :186 and :196 give an initiator's the
    configured endpoint (`start` with SRC_ESTABLISHED and no flag changes nothing: `endpoints_set` configured it), and
    nothing in the reference moves it afterwards (a node with the reference's behaviour never calls `learn`).
  WireGuard adds roaming: the endpoint follows the source of the last authenticated packet (`learn`), and of the
    response (`start` with LEARN_RESPONSE).

An endpoint is stored normalised: IPv4 keeps addr[4 .. 16) zero, _pad is zero, no endpoint is 24 zero bytes."""
import numpy as np

NOPEER = 0xFFFFFFFF
PKT_OK, PKT_KEEPALIVE, PKT_NOENDPOINT = 0, 3, 12
LEN_INVALID = 0xFFFFFFFF
INST_OK = 0
HS_INIT_OK = 0
SRC_SESSIONS, SRC_ESTABLISHED = 0, 1
LEARN_RESPONSE = 1
SEND_GATE = 1
SEND_RESPONSES, SEND_INITIATIONS, SEND_COOKIE_REPLIES = 0, 1, 2
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

SRC_DTYPE = np.dtype([("addr", "u1", (16,)), ("port", "u1", (2,)), ("family", "u1"), ("_pad", "u1", (5,))])
ITEM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("key_slot", "<u4"), ("peer", "<u4"), ("index", "<u4"),
                       ("dst", SRC_DTYPE)])
PKT_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("key_slot", "<u4")])
START_SUMMARY = np.dtype([("n_sessions", "<u4"), ("n_learned", "<u4"), ("n_badsrc", "<u4"), ("n_nopeer", "<u4")])
LEARN_SUMMARY = np.dtype([("n_authentic", "<u4"), ("n_peers", "<u4"), ("n_roamed", "<u4"), ("n_badsrc", "<u4")])
TX_SUMMARY = np.dtype([("bytes", "<u8"), ("n_items", "<u4"), ("n_noendpoint", "<u4")])
HS_SUMMARY = np.dtype([("bytes", "<u8"), ("n_items", "<u4"), ("n_nodst", "<u4")])
# per kind: the entries' stride, the message's offset in an entry
HS_LAYOUT = {SEND_RESPONSES: (176, 16), SEND_INITIATIONS: (160, 8), SEND_COOKIE_REPLIES: (80, 8)}


def src(addr, port, family=None, pad=bytes(5)):
    """24 bytes of wg_hs_src from packed address bytes (4 or 16; longer keeps garbage behind an IPv4 address)."""
    if family is None:
        family = 4 if len(addr) == 4 else 6
    return bytes(addr).ljust(16, b"\0")[:16] + int(port).to_bytes(2, "big") + bytes([family]) + bytes(pad)


def normalise(s):
    """The stored form of a 24-byte source, or None if its family is neither 4 nor 6."""
    s = bytes(s)
    assert len(s) == 24
    if s[18] == 4:
        return s[:4] + bytes(12) + s[16:19] + bytes(5)
    if s[18] == 6:
        return s[:19] + bytes(5)
    return None


def src_list(arr):
    """A SRC_DTYPE array (or a list of 24-byte strings) as a list of 24-byte strings."""
    if isinstance(arr, np.ndarray):
        return [arr[i].tobytes() for i in range(len(arr))]
    return [bytes(x) for x in arr]


class Endpoints:
    def __init__(self, key_slots, max_peers):
        self.K, self.P = key_slots, max_peers
        self.ep = [bytes(24)] * max_peers
        self.map = [NOPEER] * key_slots

    # ---- the setters and the images wg_endpoints_get / wg_endpoint_slots_get return ----
    def endpoints_set(self, first, endpoints):
        endpoints = src_list(endpoints)
        if first + len(endpoints) > self.P:
            raise IndexError("WG_ERANGE")
        if any(e[18] not in (0, 4, 6) for e in endpoints):
            raise ValueError("WG_EINVAL")
        for k, e in enumerate(endpoints):
            self.ep[first + k] = normalise(e) or bytes(24)

    def slots_set(self, first, peers):
        if first + len(peers) > self.K:
            raise IndexError("WG_ERANGE")
        self.map[first:first + len(peers)] = [int(p) & M32 for p in peers]

    def endpoints_image(self):
        return b"".join(self.ep)

    def has(self, peer):
        return peer < self.P and self.ep[peer][18] != 0

    # ---- wg_endpoints_start ----
    def start(self, ents, send, recv, source, srcs, flags=0, cover=None):
        """ents[j] = (inst_status, position, peer, index). Returns [n_sessions, n_learned, n_badsrc, n_nopeer]."""
        srcs = src_list(srcs)
        learn = source == SRC_SESSIONS or bool(flags & LEARN_RESPONSE)
        n_sessions = n_learned = n_bad = n_nopeer = 0
        seen = set()
        for j, (st, pos, peer, index) in enumerate(ents[:len(ents) if cover is None else min(cover, len(ents))]):
            if st != INST_OK or pos >= len(send):
                continue
            s, r = send[pos], recv[pos]
            if s >= self.K or r >= self.K or s == r:
                continue
            n_sessions += 1
            peer = peer if peer < self.P else NOPEER
            self.map[s] = self.map[r] = peer
            if peer == NOPEER:
                n_nopeer += 1
                continue
            if not learn:
                continue
            first = peer not in seen  # the lowest j of a peer gives its endpoint, as it becomes current in wg_timers_start
            seen.add(peer)
            a = normalise(srcs[index]) if index < len(srcs) else None
            if a is None:
                n_bad += 1
            elif first:
                self.ep[peer] = a
                n_learned += 1
        return [n_sessions, n_learned, n_bad, n_nopeer]

    # ---- wg_endpoints_learn ----
    def learn(self, desc, status, srcs, roamed_cap):
        """Returns (roamed[: min(n_roamed, cap)], [n_authentic, n_peers, n_roamed, n_badsrc])."""
        srcs = src_list(srcs)
        last = {}
        n_auth = n_bad = 0
        for i in range(len(desc)):
            if status[i] not in (PKT_OK, PKT_KEEPALIVE):
                continue
            slot = int(desc["key_slot"][i])
            if slot >= self.K or self.map[slot] >= self.P:
                continue
            if srcs[i][18] not in (4, 6):
                n_bad += 1
                continue
            n_auth += 1
            last[self.map[slot]] = i  # the last to arrive wins
        roamed = []
        for p in sorted(last):
            a = normalise(srcs[last[p]])
            if a != self.ep[p]:
                self.ep[p] = a
                roamed.append(p)
        return roamed[:roamed_cap], [n_auth, len(last), len(roamed), n_bad]

    # ---- wg_tx_sendlist ----
    def tx_sendlist(self, desc, status, gate=False):
        """desc (PKT_DTYPE array) and status (list, or None) are changed in place under the gate. Returns (items,
        (bytes, n_items, n_noendpoint))."""
        items = []
        n_noep = 0
        for j in range(len(desc)):
            ln, slot = int(desc["len"][j]), int(desc["key_slot"][j])
            if ln == LEN_INVALID or (status is not None and status[j] != PKT_OK):
                continue
            p = self.map[slot] if slot < self.K else NOPEER
            if self.has(p):
                items.append(((int(desc["out_off"][j]) - 16) & M64, (ln + 32) & M32, slot, p, j, self.ep[p]))
                continue
            n_noep += 1
            if gate:
                desc["len"][j] = LEN_INVALID
                if status is not None:
                    status[j] = PKT_NOENDPOINT
        return _items(items), (sum(it[1] for it in items), len(items), n_noep)

    # ---- wg_hs_sendlist ----
    def hs_sendlist(self, kind, entries, srcs=(), cover=None):
        """entries[k]: (index, peer) for responses, (status, len, peer) for initiations, (index, len) for cookie
        replies. Returns (items, (bytes, n_items, n_nodst))."""
        srcs = src_list(srcs)
        stride, at = HS_LAYOUT[kind]
        items = []
        n_nodst = 0
        for k, e in enumerate(entries[:len(entries) if cover is None else min(cover, len(entries))]):
            if kind == SEND_INITIATIONS:
                st, ln, peer = e
                if st != HS_INIT_OK:
                    continue
                dst = self.ep[peer] if self.has(peer) else None
            else:
                index, ln, peer = (e[0], 92, e[1]) if kind == SEND_RESPONSES else (e[0], e[1], NOPEER)
                dst = normalise(srcs[index]) if index < len(srcs) else None
            if dst is None:
                n_nodst += 1
            else:
                items.append((stride * k + at, ln, M32, peer, k, dst))
        return _items(items), (sum(it[1] for it in items), len(items), n_nodst)


def _items(items):
    out = np.zeros(len(items), ITEM_DTYPE)
    for k, (off, ln, slot, peer, index, dst) in enumerate(items):
        out[k] = (off, ln, slot, peer, index, np.frombuffer(dst, SRC_DTYPE)[0])
    return out
