"""The replay window's edge-case lists (tests/replay_edge_cases.py) on the CPU: what the builders claim
about their own cases (ring offsets, straddled powers of two, slot counts, which path a batch takes, what
every probe must find), asserted against oracle.rx.ReplayWindow, and the oracle itself against a second,
textbook window fed one packet per batch. tests/test_gpu_rx_replay_edges.py sends the same lists to the
device."""
import numpy as np
import pytest

import replay_edge_cases as E
from oracle import rx

OK, BADTAG, REPLAY = rx.PKT_OK, rx.PKT_BADTAG, rx.PKT_REPLAY


# ---- a textbook sliding window: an int bitmap (bit d = counter top - 1 - d) and top ---------------
class Textbook:
    def __init__(self, W):
        self.W, self.top, self.bits = W, {}, {}

    def accept(self, slot, c):
        top, bits = self.top.get(slot, 0), self.bits.get(slot, 0)
        if c >= rx.REJECT_AFTER:
            return False
        if c >= top:
            shift = c + 1 - top
            bits = ((bits << shift) & ((1 << self.W) - 1)) | 1 if shift < self.W else 1
            top = c + 1
        else:
            d = top - 1 - c
            if top - c > self.W or (bits >> d) & 1:
                return False
            bits |= 1 << d
        self.top[slot], self.bits[slot] = top, bits
        return True

    def words(self, slot):
        """(top, words) in the device's ring layout."""
        top, bits = self.top.get(slot, 0), self.bits.get(slot, 0)
        out = [0] * (self.W // 64)
        for d in range(min(self.W, top)):
            if (bits >> d) & 1:
                p = (top - 1 - d) % self.W
                out[p // 64] |= 1 << (p % 64)
        return top, out


def _one_by_one(W, batches, key_slots, state_slots):
    """Every packet as a batch of its own through the oracle and the textbook window: for one-packet
    batches the batch rules of include/wgaead.h (WG_RX_REPLAY) are the textbook's."""
    o, t = rx.ReplayWindow(W), Textbook(W)
    for b in batches:
        for s, c, st in zip(b.slots.tolist(), b.counters.tolist(), b.status.tolist()):
            if st != OK or not 0 <= s < key_slots:
                continue
            got = o.check_batch([s], [c], [OK])[0]
            assert got == (OK if t.accept(s, c) else REPLAY), (s, c)
    for s in state_slots:
        assert o.bitmap(s) == t.words(s), s


# ---- 1. the boundary grid -----------------------------------------------------------------------
def test_grid_offsets_lengths_and_size():
    assert E.ring_offsets(64) == [0, 1, 63]
    assert E.ring_offsets(192) == [0, 1, 63, 64, 65, 127, 128, 191]
    assert E.ring_offsets(576) == [0, 1, 63, 64, 65, 511, 512, 575]
    for W, per_band in ((64, 18), (192, 79), (576, 79)):
        for hole in (True, False):
            cases = E.grid_cases(W, hole)
            assert len(cases) == 4 * per_band <= 512 - 2  # the three-launch engine, two neighbours to spare
            assert [k.slot for k in cases] == list(range(len(cases)))
            for a in E.ring_offsets(W):
                ls = E.jump_lengths(W, a)
                assert {1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W + 3} <= set(ls) and min(ls) >= 1
                assert (a + (W - a)) % W == 0 and W - a in ls      # the cleared range ends at the ring's end
                assert (a + (W - a + 1)) % W == 1 and W - a + 1 in ls  # ... or wraps by one position


@pytest.mark.parametrize("W", E.GRID_WINDOWS)
def test_grid_bands(W):
    cases = E.grid_cases(W)
    straddling = 0
    for k in cases:
        lo, hi = k.T - W, k.T - 1  # the filled window
        assert lo >= 0 and len(set(k.holes)) == 3 and all(lo <= h <= hi for h in k.holes)
        if k.band == "small":
            assert k.T % W == k.a and k.T <= 4 * W
        elif k.band in ("2^32", "2^63"):
            p = 1 << int(k.band[2:])
            assert k.T % W == k.a and (lo < p <= hi or (k.T == p and k.a == p % W))
            straddling += lo < p <= hi
        else:
            assert k.arriving == rx.REJECT_AFTER - 1 and k.T + k.len == rx.REJECT_AFTER
        assert k.arriving < rx.REJECT_AFTER
    assert straddling >= len(cases) // 2 * 2 // 3  # all of both bands but the one residue that cannot


@pytest.mark.parametrize("top_hole", [True, False])
@pytest.mark.parametrize("W", E.GRID_WINDOWS)
def test_grid_oracle_finds_the_named_classes(W, top_hole):
    cases = E.grid_cases(W, top_hole)
    o = rx.ReplayWindow(W)
    fill, jump, probe = E.grid_fill(cases), E.grid_jump(cases), E.grid_probe(cases)
    assert len(fill.slots) == len(cases) * (W - 3) and not E.strictly_increasing(fill)
    assert E.expect(o, 512, fill) == [OK] * len(fill.slots)
    for k in cases:
        assert o.top[k.slot] == k.filled_top and k.filled_top >= W  # the first advance from 0 is a whole window
        if not top_hole and k.band != "reject_after":
            assert o.top[k.slot] % W == k.a
    assert E.strictly_increasing(jump)  # the no-table path
    assert E.expect(o, 512, jump) == [OK] * len(cases)
    assert not E.strictly_increasing(probe) and len(probe.slots) == len(cases) * (W + 3)
    got = E.expect(o, 512, probe)
    classes = {k.slot: E.probe_classes(k) for k in cases}
    seen = set()
    for s, c, st in zip(probe.slots.tolist(), probe.counters.tolist(), got):
        cls = classes[s][c]
        assert st == E.PROBE_STATUS[cls], (str(cases[s]), c, cls)
        seen.add(cls)
    assert seen == set(E.PROBE_STATUS)
    for k in cases:
        n = {}
        for cls in classes[k.slot].values():
            n[cls] = n.get(cls, 0) + 1
        jumped = k.T + k.len - k.filled_top
        assert n["below"] == 2 and n["arrived"] == 1 and n.get("next", 0) + n.get("next_rejected", 0) == 1
        assert n.get("cleared", 0) + (k.top_hole and jumped <= W) == min(jumped, W) - 1
        assert (n.get("next_rejected", 0) == 1) == (k.band == "reject_after")
    # exact jumps of W - 1, W and W + 1 from the filled top, and cleared ranges that begin on a word boundary
    if not top_hole:
        assert {W - 1, W, W + 1} <= {k.T + k.len - k.filled_top for k in cases}
        assert any(k.filled_top % 64 == 0 and k.len < W for k in cases)


@pytest.mark.parametrize("top_hole", [True, False])
def test_grid_oracle_is_the_textbook_window(top_hole):
    """W = 64 whole; W = 192 on every second and W = 576 on every fifth case (all of its packets), which
    still holds every band (one packet per batch costs a window's worth of work per packet)."""
    for W, step in ((64, 1), (192, 2), (576, 5)):
        cases = E.grid_cases(W, top_hole)
        pick = {k.slot for k in cases[::step]}
        batches = []
        for b in (E.grid_fill(cases), E.grid_jump(cases), E.grid_probe(cases)):
            m = np.isin(b.slots, list(pick))
            batches.append(E.Batch(b.slots[m], b.counters[m], b.status[m]))
        assert {cases[s].band for s in pick} == set(E.BANDS)
        _one_by_one(W, batches, 512, sorted(pick))


# ---- 2. many slots jumping by a whole window ----------------------------------------------------
@pytest.mark.parametrize("W", [576, 1024])
def test_jump_plans(W):
    b, want, after = E.jump_prefill_reference(W)
    assert len(b.slots) == 512 * W and want == [OK] * len(want)
    for s in range(512):
        assert after.top[s] == E.jump_prefill_top(W, s) and len(after.seen[s]) == W
    assert any(after.top[s] - W < (1 << 32) < after.top[s] for s in range(512))
    for k in E.JUMP_KS:
        p = E.jump_plan(W, k)
        assert len(p.movers) == k == sum(1 for j in p.jumps.values() if j >= W)
        assert {p.jumps[s] for s in p.movers} == set((W, W + 1, 10 * W, (1 << 33) + 7)[:min(k, 4)])
        rest = [p.jumps[s] for s in range(512) if s not in p.movers]
        assert abs(rest.count(W - 1) - len(rest) / 2) <= 2 and abs(rest.count(1) - len(rest) / 4) <= 1
        assert rest.count(0) >= len(rest) // 4 - 1
        o = E.copy_window(after)
        got = E.expect(o, 512, p.batch)
        for s, st in zip(p.batch.slots.tolist(), got):
            assert st == (OK if p.jumps[s] else REPLAY)
        assert all(o.top[s] == p.tops[s] for s in range(512))
        got = E.expect(o, 512, p.probe)
        for s, c, st in zip(p.probe.slots.tolist(), p.probe.counters.tolist(), got):
            d, j = p.tops[s] - c, p.jumps[s]
            # behind the window; the old top's neighbourhood; the cleared position below the arrival; the arrival
            want_st = {W + 1: REPLAY, W: OK if j >= W else REPLAY, 2: OK if j >= 2 else REPLAY, 1: REPLAY}[d]
            assert st == want_st, (s, j, d)
    assert after.top[0] == E.jump_prefill_top(W, 0) and len(after.seen[0]) == W  # the shared reference is unchanged


def test_jump_oracle_is_the_textbook_window():
    """The same builders on 24 slots (one packet per batch costs a window's worth of work per packet)."""
    for W in (576, 1024):
        for k in (1, 5):
            p = E.jump_plan(W, k, nslots=24)
            _one_by_one(W, [E.jump_prefill(W, nslots=24), p.batch, p.probe], 24, range(24))


# ---- 3. mixed high words inside one wave --------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("nslots", [1, 3])
def test_mixed_high_words(nslots, sort):
    bs = E.mixed_batches(nslots, sort)
    for b in bs[:2]:
        assert len(b.slots) <= 256 and E.mixed_word_witnesses(b) >= 1
        assert {int(c) >> 32 for c in b.counters} == {0, 1, 2, 5}
    assert all(E.strictly_increasing(b) == sort for b in bs)
    o = rx.ReplayWindow(E.MIXED_W)
    got = [E.expect(o, 512, b) for b in bs]
    assert REPLAY not in got[0] or not sort
    assert {OK, REPLAY} <= set(got[2])
    for s in range(nslots):
        assert o.top[s] >> 32 == 5
    _one_by_one(E.MIXED_W, bs, 512, range(nslots))


# ---- 4. duplicates and the rejection threshold --------------------------------------------------
def test_duplicate_plan():
    p = E.dup_plan(512)
    b = p.batch
    assert len(b.slots) == E.DUP_N == 20000 and not E.strictly_increasing(b)
    o = rx.ReplayWindow(E.DUP_W)
    got = E.expect(o, 512, b)
    pairs = list(zip(b.slots.tolist(), b.counters.tolist()))
    assert [pairs[i] for i in p.heavy] == [E.DUP_HEAVY] * 5000 and pairs.count(E.DUP_HEAVY) == 5000
    assert got[p.heavy[0]] == OK and all(got[i] == REPLAY for i in p.heavy[1:])
    assert pairs.count(E.DUP_BADTAG) == 4 and [got[i] for i in p.badtag] == [BADTAG, BADTAG, OK, REPLAY]
    assert sorted(pairs[i] for i in p.shared) == [(s, E.DUP_SHARED) for s in range(8)]
    assert all(got[i] == OK for i in p.shared)
    assert [pairs[i] for i in p.last_ok] == [(6, rx.REJECT_AFTER - 1)] * 2
    assert [got[i] for i in p.last_ok] == [OK, REPLAY]
    assert sorted(pairs[i][1] for i in p.rejected) == sorted([rx.REJECT_AFTER, rx.REJECT_AFTER + 1, (1 << 64) - 1] * 2)
    assert all(got[i] == REPLAY for i in p.rejected)
    assert sorted(pairs[i][0] for i in p.outside) == [512, 0xFFFFFFFF] and all(got[i] == OK for i in p.outside)
    assert o.top[6] == rx.REJECT_AFTER and 512 not in o.top
    again = E.expect(o, 512, b)
    for i, st in enumerate(again):
        assert st == (OK if i in set(p.outside.tolist()) else BADTAG if b.status[i] == BADTAG else REPLAY), i
    _one_by_one(E.DUP_W, [b, b], 512, range(8))


# ---- 5. the largest window, on a small copy -----------------------------------------------------
def test_largest_window_plan():
    """The builder of the W = 65536 case: its claims on the real size through the batch oracle (shared
    with the GPU test), the textbook comparison on W = 256 (one packet per batch at 65536 is hours)."""
    (fill, w0, s0), (jump, w1, s1), (probe, w2, s2) = E.maxw_reference()
    W = E.MAX_W
    assert w0 == [OK] * (6 * (W - 2)) and w1 == [OK] * 6 and E.strictly_increasing(jump)
    for s in range(6):
        assert s0[s][0] == E.maxw_top(W, s) and s0[s][0] - W < (1 << 32) < s0[s][0]
        assert s1[s][0] == s0[s][0] + E.maxw_jumps(W)[s]
        assert sum(bin(x).count("1") for x in s0[s][1]) == W - 2 and len(s0[s][1]) == 1024
        assert sum(bin(x).count("1") for x in s1[s][1]) == (1 if s in (2, 3) else 2 if s < 2 else W - 4)
    assert s0[6] == s1[6] == s2[6] == (0, [0] * 1024)
    assert {OK, REPLAY} <= set(w2) and len(w2) == 6 * 400
    _one_by_one(256, E.maxw_batches(256, ends=20), 7, range(7))
