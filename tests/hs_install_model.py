"""Plain-Python restatement of the device-owned session table and wg_hs_install (include/wgaead.h, "handshake
sessions installed on the device"), one entry at a time: the open-addressing table with fmix32 buckets, linear
probing and retired entries, wg_rx_sessions_retire, and the install's five steps with the all-or-nothing FULL rule.
Written from the header only. The table is modelled bucket for bucket, so chains, wraps of the table's end and retired
entries inside chains behave as on the device; tests/test_hs_install.py checks it against a plain dict.
"""
from __future__ import annotations

import numpy as np

INST_OK, INST_BADSLOT, INST_DUPSLOT, INST_DUPINDEX, INST_FULL = 0, 1, 2, 3, 4
SRC_SESSIONS, SRC_ESTABLISHED = 0, 1
RETIRED = 0xFFFFFFFF
M32 = 0xFFFFFFFF

HS_SESSION = np.dtype([("index", "<u4"), ("init", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("response", "u1", (92,)),
                       ("remote_index", "<u4"), ("send_key", "u1", (32,)), ("recv_key", "u1", (32,))])
HS_ESTABLISHED = np.dtype([("index", "<u4"), ("record", "<u4"), ("pending", "<u4"), ("peer", "<u4"), ("local_index", "<u4"),
                           ("remote_index", "<u4"), ("_zero", "<u4", (2,)), ("send_key", "u1", (32,)), ("recv_key", "u1", (32,))])
DTYPES = {SRC_SESSIONS: HS_SESSION, SRC_ESTABLISHED: HS_ESTABLISHED}
POSITION = {SRC_SESSIONS: "init", SRC_ESTABLISHED: "pending"}


def fmix32(h: int) -> int:
    """MurmurHash3's 32-bit finaliser."""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def _unshift(h: int, s: int) -> int:
    """The x with x ^ (x >> s) == h."""
    x = h
    for _ in range(32 // s + 1):
        x = h ^ (x >> s)
    return x


def fmix32_inv(h: int) -> int:
    """fmix32 is a bijection of the 32-bit words (xor-shifts and odd multipliers): its inverse."""
    h = _unshift(h & M32, 16)
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & M32
    h = _unshift(h, 13)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & M32
    return _unshift(h, 16)


def index_in_bucket(bucket: int, capacity: int, k: int = 0) -> int:
    """The k-th receiver index (k < 2^32 / capacity) whose bucket in a table of this capacity is `bucket`."""
    return fmix32_inv(bucket + k * capacity)


def capacity_for(n: int) -> int:
    """The smallest power of two >= max(16, 4 n)."""
    c = 16
    while c < 4 * n:
        c <<= 1
    return c


class Table:
    """capacity x [index, key slot + 1 (0: empty, 0xFFFFFFFF: retired)]; used = live + retired."""

    def __init__(self, max_sessions: int = 0, capacity: int | None = None):
        self.reserved = capacity if capacity is not None else capacity_for(max_sessions)
        self.set([], [])

    @property
    def capacity(self) -> int:
        return len(self.ent)

    def set(self, indices, slots) -> None:
        """wg_rx_sessions_set after a reserve: a rebuild into max(C, its own rule); retired entries are gone."""
        self.ent = [[0, 0] for _ in range(max(self.reserved, capacity_for(len(indices))))]
        self.used = 0
        for i, s in zip(indices, slots):
            assert self.lookup(i) is None, "repeated index"
            self._place(int(i), int(s) + 1)

    def reserve(self, max_sessions: int) -> None:
        """wg_rx_sessions_reserve on a table in use: the live entries are kept, the retired ones dropped."""
        live = self.live()
        self.reserved = capacity_for(max_sessions)
        self.set(list(live), list(live.values()))

    def _walk(self, index: int):
        """The buckets of the index's probe sequence, up to and including the first empty one."""
        mask = self.capacity - 1
        b = fmix32(index) & mask
        for _ in range(self.capacity):
            yield b
            if self.ent[b][1] == 0:
                return
            b = (b + 1) & mask

    def _place(self, index: int, hi: int) -> int:
        for b in self._walk(index):
            if self.ent[b][1] == 0:
                self.ent[b] = [index, hi]
                self.used += 1
                return b
        raise AssertionError("no empty bucket: used <= capacity / 2 was broken")

    def lookup(self, index: int):
        """The key slot of a live index, or None: retired entries are walked over, an empty one ends the walk."""
        for b in self._walk(index):
            e = self.ent[b]
            if e[1] not in (0, RETIRED) and e[0] == index:
                return e[1] - 1
        return None

    def retire(self, indices) -> int:
        """wg_rx_sessions_retire: every live index becomes a retired entry; returns how many entries did."""
        n = 0
        for index in indices:
            for b in self._walk(int(index)):
                e = self.ent[b]
                if e[1] not in (0, RETIRED) and e[0] == int(index):
                    e[1] = RETIRED
                    n += 1
                    break
        return n

    def live(self) -> dict:
        return {e[0]: e[1] - 1 for e in self.ent if e[1] not in (0, RETIRED)}

    def count(self):
        """wg_rx_sessions_count: (live, retired)."""
        live = len(self.live())
        return live, self.used - live

    def chain(self, index: int):
        """Probe-sequence length to the index's live entry (for tests that want to see a chain)."""
        for k, b in enumerate(self._walk(index)):
            if self.ent[b][1] not in (0, RETIRED) and self.ent[b][0] == index:
                return k + 1
        return None


class State:
    """What wg_hs_install writes besides the table: the key table, send counters, replay windows (as 'emptied'
    marks), the framer's receiver table, and the slots whose host mirror holds no key."""

    def __init__(self, key_slots: int):
        self.key_slots = key_slots
        self.keys = {}        # slot -> 32 bytes
        self.reset = set()    # slots whose counter and window the install reset
        self.receivers = {}   # send slot -> remote index
        self.no_mirror = set()


def install(table: Table, state: State, entries: np.ndarray, n_entries, send_slot, recv_slot, *, slot_first, slot_count,
            source, receivers=True, wipe=True):
    """Returns (statuses of the covered entries, summary dict); changes table, state and (wipe) entries in place."""
    pos_field = POSITION[source]
    n = len(entries)
    cover = n if n_entries is None else min(int(n_entries), n)
    state.no_mirror |= set(range(slot_first, min(slot_first + slot_count, state.key_slots)))
    status = [None] * cover
    slots = [None] * cover

    def slot_ok(s):
        return slot_first <= s < slot_first + slot_count and s < state.key_slots

    claimed, seen_index, cand = set(), set(), []
    for j in range(cover):
        p = int(entries[j][pos_field])
        if p >= len(send_slot):                                            # 1
            status[j] = INST_BADSLOT
            continue
        s, r = int(send_slot[p]), int(recv_slot[p])
        if not slot_ok(s) or not slot_ok(r) or s == r:
            status[j] = INST_BADSLOT
            continue
        slots[j] = (s, r)
        dup = s in claimed or r in claimed                                 # 2: against every lower j that passed 1
        claimed |= {s, r}
        if dup:
            status[j] = INST_DUPSLOT
            continue
        index = int(entries[j]["local_index"])                             # 3: against every lower j that passed 1-2
        dup = table.lookup(index) is not None or index in seen_index
        seen_index.add(index)
        if dup:
            status[j] = INST_DUPINDEX
            continue
        cand.append(j)
    full = table.used + len(cand) > table.capacity // 2                    # 4: all or nothing
    for j in cand:
        if full:
            status[j] = INST_FULL
            continue
        s, r = slots[j]                                                    # 5
        status[j] = INST_OK
        state.keys[s] = entries[j]["send_key"].tobytes()
        state.keys[r] = entries[j]["recv_key"].tobytes()
        state.reset |= {s, r}
        table._place(int(entries[j]["local_index"]), r + 1)
        if receivers:
            state.receivers[s] = int(entries[j]["remote_index"])
        if wipe:
            entries[j]["send_key"] = 0
            entries[j]["recv_key"] = 0
    summary = dict(n_ok=status.count(INST_OK), n_badslot=status.count(INST_BADSLOT),
                   n_dup=status.count(INST_DUPSLOT) + status.count(INST_DUPINDEX), n_full=status.count(INST_FULL))
    return status, summary
