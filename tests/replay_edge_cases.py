"""Case lists for the replay window's edges (wg_rx_check(WG_RX_REPLAY), wireguard-java_amd/csrc/wg_rx.hip):
ring offsets and jump lengths around every word and ring boundary, counters at and above 2^32 and 2^63 and
up to Reject-After-Messages, many windows jumping by a whole window in one batch, mixed high words inside
one wave, duplicates at their extremes, the largest window. No GPU here: tests/test_replay_edges.py checks
what these builders claim, tests/test_gpu_rx_replay_edges.py sends the same lists to the device. Every
expectation is oracle.rx.ReplayWindow's (``expect``); the classes the builders name are asserted against it
on the CPU so the lists cannot go stale."""
from __future__ import annotations

import functools
import random
from typing import NamedTuple

import numpy as np

from oracle import rx

OK, BADTAG, REPLAY = rx.PKT_OK, rx.PKT_BADTAG, rx.PKT_REPLAY
REJECT_AFTER = rx.REJECT_AFTER
BANDS = ("small", "2^32", "2^63", "reject_after")
GRID_WINDOWS = (64, 192, 576)


class Batch(NamedTuple):
    slots: np.ndarray     # int64 (a key slot past the table is a descriptor the check leaves alone)
    counters: np.ndarray  # uint64
    status: np.ndarray    # int64, the statuses before the check


def make_batch(slots, counters, status=None) -> Batch:
    s = np.asarray(slots, np.int64)
    c = np.array([int(x) for x in counters], dtype=np.uint64) if not isinstance(counters, np.ndarray) else counters
    st = np.zeros(len(s), np.int64) if status is None else np.asarray(status, np.int64)
    assert len(s) == len(c) == len(st) and c.dtype == np.uint64
    return Batch(s, c, st)


def shuffled(b: Batch, seed: int) -> Batch:
    p = np.random.default_rng(seed).permutation(len(b.slots))
    return Batch(b.slots[p], b.counters[p], b.status[p])


def sorted_unique(b: Batch) -> Batch:
    """The batch sorted by (slot, counter) with repeated pairs removed: strictly increasing, so the
    device skips the duplicate table."""
    order = np.lexsort((b.counters, b.slots))
    s, c, st = b.slots[order], b.counters[order], b.status[order]
    keep = np.ones(len(s), bool)
    keep[1:] = (s[1:] != s[:-1]) | (c[1:] != c[:-1])
    return Batch(s[keep], c[keep], st[keep])


def strictly_increasing(b: Batch) -> bool:
    pairs = list(zip(b.slots.tolist(), b.counters.tolist()))
    return all(x < y for x, y in zip(pairs, pairs[1:]))


def expect(window: rx.ReplayWindow, key_slots: int, b: Batch) -> list[int]:
    """ReplayWindow.check_batch over the descriptors whose key slot exists; a descriptor whose key slot
    is past the table is not the check's to judge and keeps its status."""
    idx = np.nonzero((b.slots >= 0) & (b.slots < key_slots))[0]
    st = b.status.tolist()
    got = window.check_batch(b.slots[idx].tolist(), b.counters[idx].tolist(), [st[i] for i in idx.tolist()])
    for i, x in zip(idx.tolist(), got):
        st[i] = x
    return st


def copy_window(w: rx.ReplayWindow) -> rx.ReplayWindow:
    n = rx.ReplayWindow(w.W)
    n.top = dict(w.top)
    n.seen = {s: set(v) for s, v in w.seen.items()}
    return n


# ---- 1. the boundary grid -----------------------------------------------------------------------
class GridCase(NamedTuple):
    slot: int
    W: int
    band: str
    a: int         # the ring offset asked for: T % W == a (reject_after: T is fixed by len, see grid_top)
    len: int       # the arriving counter is T + len - 1
    T: int
    top_hole: bool  # the third hole is T - 1 (the filled top is then T - 1), else T - 2 (the filled top is T)

    @property
    def holes(self):
        return (self.T - self.W, self.T - self.W // 2, self.T - 1 if self.top_hole else self.T - 2)

    @property
    def filled_top(self):
        return self.T - 1 if self.top_hole else self.T

    @property
    def arriving(self):
        return self.T + self.len - 1

    def __str__(self):
        return f"slot {self.slot}: W={self.W} band={self.band} a={self.a} len={self.len} T={self.T:#x}"


def ring_offsets(W: int) -> list[int]:
    return sorted({x % W for x in (0, 1, 63, 64, 65, W - 65, W - 64, W - 1)})


def jump_lengths(W: int, a: int) -> list[int]:
    """1, 2 and the word edges; W - a ends the cleared range at the ring's end, W - a + 1 wraps it by
    one position; W - 1, W, W + 1 and 2W + 3 around and past a whole window."""
    return sorted({1, 2, 63, 64, 65, W - a, W - a + 1, W - 1, W, W + 1, 2 * W + 3})


def grid_top(W: int, band: str, a: int, ln: int) -> int:
    """T with T % W == a and the filled window [T - W, T) in the band: a few W; 2^32 - 1 and 2^32 both
    inside; the same for 2^63. One residue has no such T (a == 2^k mod W: 0 for W = 64, 64 for W = 192):
    there T = 2^k, the filled window ends on 2^k - 1 and the arriving counter is the first past it.
    reject_after: T = REJECT_AFTER - len, so the arriving counter is the last
    acceptable one; its ring offset is then (REJECT_AFTER - len) % W, and `a` only selects the lengths."""
    if band == "small":
        return 3 * W + a
    if band == "reject_after":
        return REJECT_AFTER - ln
    p = 1 << (32 if band == "2^32" else 63)
    T = p + 1 + (a - p - 1) % W  # in [2^k + 1, 2^k + W]
    return T if T < p + W else p  # a == 2^k mod W: the filled window ends at 2^k - 1 and the top is 2^k itself


def grid_cases(W: int, top_hole: bool = True) -> list[GridCase]:
    """One key slot per (band, a, len). top_hole=True is the fill with the holes T - W, T - W // 2 and
    T - 1; since T - 1 is then never accepted the window's top after the fill is T - 1 and the jump
    clears len + 1 positions from ring offset a - 1. top_hole=False moves the third hole to T - 2, so
    the top after the fill is T itself: exactly len positions are cleared from offset a (jumps of exactly
    W - 1, W and W + 1, ranges that begin on a word boundary)."""
    out = []
    for band in BANDS:
        for a in ring_offsets(W):
            for ln in jump_lengths(W, a):
                out.append(GridCase(len(out), W, band, a, ln, grid_top(W, band, a, ln), top_hole))
    return out


def grid_fill(cases) -> Batch:
    """Counters T - W .. T - 1 of every case but its three holes, shuffled over all slots (the table path)."""
    pairs = []
    for k in cases:
        holes = set(k.holes)
        pairs += [(k.slot, c) for c in range(k.T - k.W, k.T) if c not in holes]
    random.Random(1000 + cases[0].W).shuffle(pairs)
    return make_batch([p[0] for p in pairs], [p[1] for p in pairs])


def grid_jump(cases) -> Batch:
    """One packet per slot in slot order: strictly increasing, the no-table path."""
    return make_batch([k.slot for k in cases], [k.arriving for k in cases])


def grid_probe(cases) -> Batch:
    """Every counter in [T + len - W - 2, T + len] once per slot, shuffled over all slots."""
    pairs = []
    for k in cases:
        pairs += [(k.slot, c) for c in range(k.T + k.len - k.W - 2, k.T + k.len + 1)]
    random.Random(2000 + cases[0].W).shuffle(pairs)
    return make_batch([p[0] for p in pairs], [p[1] for p in pairs])


PROBE_STATUS = {"below": REPLAY, "survivor": REPLAY, "hole": OK, "cleared": OK, "arrived": REPLAY, "next": OK,
                "next_rejected": REPLAY}


def probe_classes(k: GridCase) -> dict[int, str]:
    """counter -> what the probe must find, worked out from the case alone (the window after the jump is
    [T + len - W, T + len)): the two counters below it, the filled counters whose bits survived the
    clear, the holes still inside, the cleared positions (never accepted: T - 1 when it is a hole, and
    T .. T + len - 2), the counter that arrived, and the next one (rejected only where it is
    REJECT_AFTER itself)."""
    top = k.T + k.len
    out = {}
    for c in range(top - k.W - 2, top + 1):
        if c == top:
            out[c] = "next" if c < REJECT_AFTER else "next_rejected"
        elif c == top - 1:
            out[c] = "arrived"
        elif c < top - k.W:
            out[c] = "below"
        elif c in k.holes:
            out[c] = "hole"
        elif c < k.T:
            out[c] = "survivor"
        else:
            out[c] = "cleared"
    return out


# ---- 2. many slots jumping by a whole window in one batch ---------------------------------------
JUMP_SLOTS = 512
JUMP_KS = (1, 63, 64, 65, 300)


def jump_prefill_top(W: int, s: int) -> int:
    """Top of slot s after the prefill: every eighth slot's full window straddles 2^32, the others sit
    at staggered ring offsets a few windows up."""
    base = (1 << 32) - W // 2 + s if s % 8 == 3 else 2 * W + 37 * s
    return base + W


def jump_prefill(W: int, nslots: int = JUMP_SLOTS) -> Batch:
    """Every slot's window filled completely (a missed clear leaves stale bits), shuffled."""
    slots = np.repeat(np.arange(nslots, dtype=np.int64), W)
    tops = np.array([jump_prefill_top(W, s) for s in range(nslots)], dtype=np.uint64)
    ctr = np.repeat(tops - np.uint64(W), W) + np.tile(np.arange(W, dtype=np.uint64), nslots)
    return shuffled(Batch(slots, ctr, np.zeros(len(slots), np.int64)), 3000 + W)


class JumpPlan(NamedTuple):
    jumps: dict     # slot -> how far its top moves (0: it only receives an old counter)
    movers: list    # the k slots that jump by W or more
    batch: Batch
    probe: Batch
    tops: dict      # slot -> top after the jump batch


def jump_plan(W: int, k: int, nslots: int = JUMP_SLOTS) -> JumpPlan:
    """Exactly k slots jump by at least W (sizes cycle W, W + 1, 10 W, 2^33 + 7); of the others half
    jump by W - 1, a quarter by 1 and the rest receive top - 5 again (in the window, seen: no move)."""
    rng = np.random.default_rng(4000 + 7 * W + k)
    movers = sorted(int(x) for x in rng.choice(nslots, k, replace=False))
    big = (W, W + 1, 10 * W, (1 << 33) + 7)
    jumps = {s: big[i % 4] for i, s in enumerate(movers)}
    for i, s in enumerate(x for x in range(nslots) if x not in jumps):
        jumps[s] = (W - 1, W - 1, 1, 0)[i % 4]
    ctr, tops = [], {}
    for s in range(nslots):
        top = jump_prefill_top(W, s)
        ctr.append(top + jumps[s] - 1 if jumps[s] else top - 5)
        tops[s] = top + jumps[s]
    batch = shuffled(make_batch(list(range(nslots)), ctr), 5000 + k)
    ps, pc = [], []
    for s in range(nslots):
        for c in (tops[s] - W - 1, tops[s] - W, tops[s] - 2, tops[s] - 1):
            ps.append(s)
            pc.append(c)
    return JumpPlan(jumps, movers, batch, shuffled(make_batch(ps, pc), 6000 + k), tops)


# ---- 3. mixed high words inside one wave --------------------------------------------------------
MIXED_W = 192


def mixed_batches(nslots: int, sort: bool, seed: int = 7) -> list[Batch]:
    """Two batches of 256 packets whose counters come from three clusters (2^32 +- 40, 2^33 +- 5 and
    5 * 2^32 + j), then a probe around each slot's new top and around 2^32. The maximum of a wave has a
    small low word while smaller counters have low words near 2^32 - 1."""
    rng = np.random.default_rng(seed + nslots)
    out = []
    for b in range(2):
        kind = rng.integers(0, 3, 256)
        c = np.where(kind == 0, (1 << 32) + rng.integers(-40, 41, 256),
                     np.where(kind == 1, (1 << 33) + rng.integers(-5, 6, 256),
                              5 * (1 << 32) + 25 * b + rng.integers(0, 20, 256)))
        batch = Batch(rng.integers(0, nslots, 256).astype(np.int64), c.astype(np.uint64), np.zeros(256, np.int64))
        out.append(sorted_unique(batch) if sort else batch)
    ps, pc = [], []
    for s in range(nslots):
        m = max(int(c) for b in out for c in b.counters[b.slots == s])
        for c in list(range(m + 1 - MIXED_W - 2, m + 3)) + list(range((1 << 32) - 3, (1 << 32) + 4)):
            ps.append(s)
            pc.append(c)
    probe = make_batch(ps, pc)
    out.append(sorted_unique(probe) if sort else shuffled(probe, seed))
    return out


def mixed_word_witnesses(b: Batch) -> int:
    """Aligned groups of 64 packets (one wave) with a slot whose maximum counter's low word is smaller
    than another member's: there the largest low word does not belong to the maximum, so a maximum put
    together from independently reduced words is not the maximum."""
    found = 0
    for g in range(0, len(b.slots), 64):
        s, c = b.slots[g:g + 64], b.counters[g:g + 64]
        for slot in np.unique(s):
            m = [int(x) for x in c[s == slot]]
            if len(m) > 1 and (max(m) & 0xFFFFFFFF) < max(x & 0xFFFFFFFF for x in m):
                found += 1
    return found


# ---- 4. duplicates at their extremes and the rejection threshold --------------------------------
DUP_W = 576
DUP_N = 20000
DUP_HEAVY = (3, 7777)    # the pair sent 5,000 times
DUP_BADTAG = (5, 4242)   # the pair whose first two copies failed authentication
DUP_SHARED = 9999        # one counter on all 8 slots


class DupPlan(NamedTuple):
    batch: Batch
    heavy: np.ndarray      # indices of DUP_HEAVY's copies, ascending
    badtag: np.ndarray     # indices of DUP_BADTAG's copies, ascending (the first two carry BADTAG)
    shared: np.ndarray     # indices of DUP_SHARED on slots 0..7
    last_ok: np.ndarray    # indices of REJECT_AFTER - 1 on slot 6 (twice)
    rejected: np.ndarray   # indices of REJECT_AFTER, REJECT_AFTER + 1 and 2^64 - 1 on slot 7, each twice
    outside: np.ndarray    # indices of the descriptors whose key slot is past the table


def dup_plan(key_slots: int) -> DupPlan:
    rng = np.random.default_rng(81)
    special = ([DUP_HEAVY] * 5000 + [DUP_BADTAG] * 4 + [(s, DUP_SHARED) for s in range(8)] +
               [(6, REJECT_AFTER - 1)] * 2 + [(7, REJECT_AFTER), (7, REJECT_AFTER + 1), (7, (1 << 64) - 1)] * 2 +
               [(key_slots, 11), (0xFFFFFFFF, 12)])
    nb = DUP_N - len(special)
    slots = np.concatenate([np.array([p[0] for p in special], np.int64), rng.integers(0, 8, nb)])
    ctr = np.concatenate([np.array([p[1] for p in special], dtype=np.uint64),
                          rng.integers(0, 6000, nb).astype(np.uint64)])  # 1,900 draws per slot from 6,000: repeats
    # background draws must not collide with the named pairs
    clash = np.zeros(DUP_N, bool)
    clash[len(special):] = np.isin(ctr[len(special):], np.array([DUP_HEAVY[1], DUP_BADTAG[1]], dtype=np.uint64))
    ctr[clash] = np.uint64(5)
    p = rng.permutation(DUP_N)
    where = np.empty(DUP_N, np.int64)
    where[p] = np.arange(DUP_N)  # special[j] sits at index where[j]
    slots, ctr = slots[p], ctr[p]
    status = np.zeros(DUP_N, np.int64)
    idx = lambda lo, n: np.sort(where[lo:lo + n])  # noqa: E731
    heavy, badtag, shared = idx(0, 5000), idx(5000, 4), idx(5004, 8)
    status[badtag[:2]] = BADTAG
    return DupPlan(Batch(slots, ctr, status), heavy, badtag, shared, idx(5012, 2), idx(5014, 6), idx(5020, 2))


# ---- 5. the largest window ----------------------------------------------------------------------
MAX_W = 65536


def maxw_top(W: int, s: int) -> int:
    return (1 << 32) + W // 2 + 1000 * s  # [top - W, top) straddles 2^32


def maxw_jumps(W: int) -> tuple:
    return (W - 1, W - 1, W, W, 3, 3)


def maxw_batches(W: int = MAX_W, ends: int = 100) -> list[Batch]:
    """Six slots: a full window straddling 2^32 (no holes but top - W // 3 and top - 7), a jump by
    W - 1 on two slots, W on two and 3 on two (slot order, the no-table path), then `2 * ends` counters
    around each end of each new window."""
    nslots = 6
    slots = np.repeat(np.arange(nslots, dtype=np.int64), W)
    tops = [maxw_top(W, s) for s in range(nslots)]
    ctr = np.repeat(np.array(tops, dtype=np.uint64) - np.uint64(W), W) + np.tile(np.arange(W, dtype=np.uint64), nslots)
    keep = np.ones(len(ctr), bool)
    for s in range(nslots):
        keep[s * W + W - W // 3] = keep[s * W + W - 7] = False
    fill = shuffled(Batch(slots[keep], ctr[keep], np.zeros(int(keep.sum()), np.int64)), 9000 + W)
    new = [t + j for t, j in zip(tops, maxw_jumps(W))]
    jump = make_batch(list(range(nslots)), [t - 1 for t in new])
    ps, pc = [], []
    for s, t in enumerate(new):
        for c in list(range(t - W - ends, t - W + ends)) + list(range(t - ends, t + ends)):
            ps.append(s)
            pc.append(c)
    return [fill, jump, shuffled(make_batch(ps, pc), 9100 + W)]


# ---- references computed once and shared (never changed: callers take copy_window) --------------
@functools.lru_cache(maxsize=None)
def grid_reference(W: int, top_hole: bool):
    """(cases, [(name, batch, expected statuses, {slot: (top, words)})] for fill, jump and probe); the
    states cover every case's slot and the two slots after them, which no batch touches."""
    cases = grid_cases(W, top_hole)
    o = rx.ReplayWindow(W)
    out = []
    for name, b in (("fill", grid_fill(cases)), ("jump", grid_jump(cases)), ("probe", grid_probe(cases))):
        want = expect(o, len(cases) + 2, b)
        out.append((name, b, want, {s: o.bitmap(s) for s in range(len(cases) + 2)}))
    return cases, out


@functools.lru_cache(maxsize=None)
def jump_prefill_reference(W: int):
    """(prefill batch, its expected statuses, the oracle's windows after it)."""
    b = jump_prefill(W)
    o = rx.ReplayWindow(W)
    return b, expect(o, JUMP_SLOTS, b), o


@functools.lru_cache(maxsize=None)
def maxw_reference():
    """The three batches of maxw_batches() with the expected statuses and the oracle's (top, words) of
    slots 0..6 after each."""
    o = rx.ReplayWindow(MAX_W)
    out = []
    for b in maxw_batches():
        want = expect(o, 7, b)
        out.append((b, want, [o.bitmap(s) for s in range(7)]))
    return out
