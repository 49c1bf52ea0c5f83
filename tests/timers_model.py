"""Plain-Python restatement of wg_timers_start / _mark / _sweep over the public image (wg_timer_slot, wg_timer_peer_state,
wg_timers_config, the send counters, the receiver-index table), the judge of the device's bytes: the reference's timers
are wall-clock threads, one per peer, and cannot be run as an oracle. What it restates of the reference:

  EstablishedSession.isExpired (EstablishedSession.java:28, :114): a session expires `expiration` = 120 s after its
    creation. The reference only stops WAITING on an expired session: SessionManager.sessionInitiationThread
    (SessionManager.java:92-111) then initiates again, and a failed attempt is retried after 5 s (:188). It never refuses
    to send on a session. `reference()` is therefore rekey_after_time = 120 s, rekey_timeout = 5 s, everything else off.
  KeepaliveSender (KeepaliveSender.java:29-85): with a persistent keepalive interval, one keepalive as soon as the session
    changes (:69-73), then one per interval of silence.
  `wireguard()` adds what the reference leaves out: REJECT_AFTER_TIME, the passive keepalive, lingering superseded
    sessions, the message limits and "only the initiator rekeys".

Time is a tick count; tick 0 is "never"; an age is now - t, or 0 when the clock stepped back."""
import numpy as np

NONE, SEND_INITIATOR, SEND_RESPONDER, RECV, DEAD = 0, 1, 2, 3, 4
NOSLOT = NOPEER = 0xFFFFFFFF
INITIATOR_ONLY = 1
CAN_INITIATE = 1
PKT_OK, PKT_KEEPALIVE, PKT_NOSESSION = 0, 3, 10
LEN_INVALID = 0xFFFFFFFF
INST_OK = 0
SRC_SESSIONS, SRC_ESTABLISHED = 0, 1
M64 = (1 << 64) - 1

SLOT_DTYPE = np.dtype([("state", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("partner", "<u4"), ("born", "<u8"),
                       ("last", "<u8"), ("last_data", "<u8"), ("superseded", "<u8")])
PEER_DTYPE = np.dtype([("current", "<u4"), ("flags", "<u4"), ("keepalive_interval", "<u8"), ("rekey_listed", "<u8")])
EXPIRED_DTYPE = np.dtype([("send_slot", "<u4"), ("recv_slot", "<u4"), ("peer", "<u4"), ("local_index", "<u4")])
PKT_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("key_slot", "<u4")])

FIELDS = ("rekey_after_time", "reject_after_time", "rekey_timeout", "keepalive_timeout", "linger", "rekey_after_messages",
          "reject_after_messages", "flags")


class Config:
    def __init__(self, **kw):
        for f in FIELDS:
            setattr(self, f, int(kw.pop(f, 0)))
        assert not kw, kw


def reference(ticks_per_s):
    """EstablishedSession.java:28 (120 s), SessionManager.java:188 (5 s); the reference never stops using a session."""
    return Config(rekey_after_time=120 * ticks_per_s, rekey_timeout=5 * ticks_per_s)


def wireguard(ticks_per_s):
    t = ticks_per_s
    return Config(rekey_after_time=120 * t, reject_after_time=180 * t, rekey_timeout=5 * t, keepalive_timeout=10 * t,
                  linger=180 * t, rekey_after_messages=1 << 60, reject_after_messages=(1 << 64) - (1 << 13) - 1,
                  flags=INITIATOR_ONLY)


def age(now, t):
    return now - t if now >= t else 0


def is_send(state):
    return state in (SEND_INITIATOR, SEND_RESPONDER)


class Timers:
    def __init__(self, key_slots, max_peers, config=None):
        self.K, self.P = key_slots, max_peers
        self.cfg = config or Config()
        self.slots = [dict(state=NONE, peer=0, local_index=0, partner=0, born=0, last=0, last_data=0, superseded=0)
                      for _ in range(key_slots)]
        self.peers = [dict(current=NOSLOT, flags=0, keepalive_interval=0, rekey_listed=0) for _ in range(max_peers)]
        self.send = [0] * key_slots  # the transmit state's counters
        self.table = {}              # receiver index -> recv slot, the live entries of the session table
        self.retired = 0

    # ---- images, as wg_timers_get / wg_timers_peers_get return them ----
    def slots_image(self):
        return np.array([tuple(r[f] for f in SLOT_DTYPE.names) for r in self.slots], SLOT_DTYPE)

    def peers_image(self):
        return np.array([tuple(p[f] for f in PEER_DTYPE.names) for p in self.peers], PEER_DTYPE).reshape(-1)

    def peers_set(self, first, peers):
        for k, (interval, can) in enumerate(peers):
            self.peers[first + k].update(keepalive_interval=interval, flags=CAN_INITIATE if can else 0)

    def expired(self, r, counter, now):
        """EstablishedSession.isExpired with WireGuard's other two ends of a session."""
        c = self.cfg
        return bool((c.reject_after_time and age(now, r["born"]) >= c.reject_after_time) or
                    (c.reject_after_messages and counter >= c.reject_after_messages) or
                    (c.linger and r["superseded"] and age(now, r["superseded"]) >= c.linger))

    # ---- wg_timers_start ----
    def _kill(self, slot):
        r = self.slots[slot]
        if r["state"] not in (SEND_INITIATOR, SEND_RESPONDER, RECV):
            return
        q = r["partner"]
        if q < self.K:
            self.slots[q]["state"] = DEAD
        snd = slot if is_send(r["state"]) else q
        if r["peer"] < self.P and self.peers[r["peer"]]["current"] == snd:
            self.peers[r["peer"]]["current"] = NOSLOT

    def start(self, now, entries, send_slot, recv_slot, source, cover=None, install=False):
        """entries: [(inst_status, position, peer, local_index)]. install=True also enters {local_index -> recv slot}
        into the table, as the wg_hs_install before it did."""
        if now == 0:
            return
        cover = len(entries) if cover is None else min(cover, len(entries))
        started = []
        for j in range(cover):
            st, p, peer, index = entries[j]
            if st != INST_OK or p >= len(send_slot):
                continue
            s, r = send_slot[p], recv_slot[p]
            if s >= self.K or r >= self.K or s == r:
                continue
            started.append((j, s, r, peer if peer < self.P else NOPEER, index))
        claim = {}
        for j, s, r, peer, index in started:  # the kill pass
            self._kill(s)
            self._kill(r)
            if peer != NOPEER:
                claim[peer] = min(claim.get(peer, j), j)
        role = SEND_RESPONDER if source == SRC_SESSIONS else SEND_INITIATOR
        for j, s, r, peer, index in started:  # the write pass
            win = peer != NOPEER and claim[peer] == j
            sup = now if (peer != NOPEER and not win) else 0
            self.slots[s] = dict(state=role, peer=peer, local_index=index, partner=r, born=now, last=0, last_data=0, superseded=sup)
            self.slots[r] = dict(state=RECV, peer=peer, local_index=index, partner=s, born=now, last=0, last_data=0, superseded=0)
            if install:
                self.table[index] = r
                self.send[s] = self.send[r] = 0
            if win:
                prev = self.peers[peer]["current"]
                if prev < self.K and is_send(self.slots[prev]["state"]):
                    self.slots[prev]["superseded"] = now
                self.peers[peer]["current"] = s

    # ---- wg_timers_mark ----
    def mark(self, now, desc, status, tx=False, gate=False, slot_first=0, slot_count=0):
        """desc: PKT_DTYPE array, status: list; both changed in place by the gate. Returns (n_marked, n_refused)."""
        n_marked = n_refused = 0
        if now == 0:
            return 0, 0
        c = self.cfg
        for i in range(len(desc)):
            st, slot = status[i], int(desc[i]["key_slot"])
            rec = self.slots[slot] if slot < self.K else None
            if not tx:
                if st in (PKT_OK, PKT_KEEPALIVE) and rec is not None and rec["state"] == RECV:
                    rec["last"] = max(rec["last"], now)
                    if st == PKT_OK:
                        rec["last_data"] = max(rec["last_data"], now)
                    n_marked += 1
                continue
            if st != PKT_OK:
                continue
            live = rec is not None and is_send(rec["state"])
            refused = False
            if gate and slot_first <= slot < slot_first + slot_count:
                refused = bool(not live or (c.reject_after_time and age(now, rec["born"]) >= c.reject_after_time) or
                               (c.reject_after_messages and int(desc[i]["counter"]) >= c.reject_after_messages))
            if refused:
                status[i] = PKT_NOSESSION
                desc[i]["len"] = LEN_INVALID
                n_refused += 1
            elif live:
                rec["last"] = max(rec["last"], now)
                if int(desc[i]["len"]) > 0:
                    rec["last_data"] = max(rec["last_data"], now)
                n_marked += 1
        return n_marked, n_refused

    # ---- wg_timers_sweep ----
    def sweep(self, now, cap_exp, cap_init, cap_keep, wire_base=0, wire_stride=0, out_size=0, retire=False):
        """Returns dict(expired=EXPIRED_DTYPE[n], initiate=[cap_init, padded], keepalives=PKT_DTYPE[cap_keep, padded],
        summary=[8])."""
        c = self.cfg
        due_exp, due_init, due_keep, live = [], [], [], 0
        if now != 0:
            for i, r in enumerate(self.slots):  # every verdict from the state as the call found it
                if not is_send(r["state"]):
                    continue
                live += 1
                if self.expired(r, self.send[i], now):
                    due_exp.append(i)
                    continue
                if r["peer"] >= self.P or self.peers[r["peer"]]["current"] != i:
                    continue
                pr = self.peers[r["peer"]]
                heard = self.slots[r["partner"]]["last_data"] if r["partner"] < self.K else 0
                # KeepaliveSender.java:69-73: at once when the session changes (last == 0), then per interval
                persistent = pr["keepalive_interval"] and (r["last"] == 0 or age(now, r["last"]) >= pr["keepalive_interval"])
                passive = c.keepalive_timeout and heard > r["last"] and age(now, heard) >= c.keepalive_timeout
                if persistent or passive:
                    due_keep.append(i)
            for p, pr in enumerate(self.peers):
                if not pr["flags"] & CAN_INITIATE:
                    continue
                need = True  # SessionManager.java:92-111: no session, or an expired one
                cur = pr["current"]
                if cur < self.K and is_send(self.slots[cur]["state"]) and not self.expired(self.slots[cur], self.send[cur], now):
                    r = self.slots[cur]
                    need = bool((c.rekey_after_time and age(now, r["born"]) >= c.rekey_after_time) or
                                (c.rekey_after_messages and self.send[cur] >= c.rekey_after_messages))
                    if c.flags & INITIATOR_ONLY and r["state"] != SEND_INITIATOR:
                        need = False
                # SessionManager.java:188: the next attempt rekey_timeout after the last
                if need and (pr["rekey_listed"] == 0 or age(now, pr["rekey_listed"]) >= c.rekey_timeout):
                    due_init.append(p)
        wire_slots = (out_size - wire_base) // wire_stride if wire_stride >= 32 and wire_base <= out_size else 0
        n_exp, n_init, n_keep = min(len(due_exp), cap_exp), min(len(due_init), cap_init), min(len(due_keep), cap_keep, wire_slots)
        exp = np.zeros(n_exp, EXPIRED_DTYPE)
        for j, i in enumerate(due_exp[:n_exp]):
            r = self.slots[i]
            exp[j] = (i, r["partner"], r["peer"], r["local_index"])
            if retire:
                if self.table.get(r["local_index"]) == r["partner"]:
                    del self.table[r["local_index"]]
                    self.retired += 1
                r["state"] = DEAD
                if r["partner"] < self.K:
                    self.slots[r["partner"]]["state"] = DEAD
                if r["peer"] < self.P and self.peers[r["peer"]]["current"] == i:
                    self.peers[r["peer"]]["current"] = NOSLOT
        init = due_init[:n_init] + [0xFFFFFFFF] * (cap_init - n_init)
        for p in due_init[:n_init]:
            self.peers[p]["rekey_listed"] = now
        keep = np.zeros(cap_keep, PKT_DTYPE)
        keep["len"] = LEN_INVALID
        for j, i in enumerate(due_keep[:n_keep]):
            keep[j] = (0, wire_base + j * wire_stride + 16, self.send[i], 0, i)
            self.send[i] = (self.send[i] + 1) & M64
            self.slots[i]["last"] = now
        n_live = live - (n_exp if retire else 0)
        return dict(expired=exp, initiate=init, keepalives=keep,
                    summary=[len(due_exp), n_exp, len(due_init), n_init, len(due_keep), n_keep, n_live, 0])
