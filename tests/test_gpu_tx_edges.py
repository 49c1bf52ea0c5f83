"""wg_routes_set / wg_tx_plan on the MI355X at their edges (pytest -m gpu): the tables of
tests/tx_edge_cases.py (a route at every prefix length of both families, prefixes nested inside one byte of
a compiled node, equal prefixes given again, a random table with host bits set, families without routes),
tables that change size under a captured plan, refused tables, broadcast to 2..1000 peers and over more
than 1,024 steps, and route-mode steps whose lanes hold 64, 2 or 1 distinct key slots. Every expectation is
tests/tx_model.py's; every comparison is exact: descriptors byte for byte, statuses, the send counters of
the whole key table after every plan, the guard records behind the outputs, and a sealed wire ring as a
whole against the frozen oracle. What a test claims about its cases (which route wins, which statuses
occur) is asserted on the model's output. tests/test_tx.py checks the tables and the model on the CPU."""
import ctypes

import numpy as np
import pytest

import tx_edge_cases as E
import tx_model as M
from tx_gpu import GUARD, KEY_SLOTS, open_rig, oracle_ring, plan, ring_of, same_desc, seal

pytestmark = pytest.mark.gpu

STRIDE, MAX_LEN = 96, 60  # route tests: packets of 20..60 B, 61 B is too long
assert KEY_SLOTS == E.KEY_SLOTS


@pytest.fixture(scope="module")
def rig():
    r = open_rig(0x7ED6E)
    yield r
    r.eng.close()


def _start(rig, seed):
    """Seeded send counters for the whole key table, every 7th slot two below 2^32 and every 11th at
    2^64 - 1, so most plans carry into the high word and wrap; returns them as the model's dict."""
    start = np.random.default_rng(seed).integers(0, 1 << 62, KEY_SLOTS).astype(np.uint64)
    start[::7] = (1 << 32) - 2
    start[::11] = (1 << 64) - 1
    rig.eng.tx_counters_set(0, start)
    return {s: int(start[s]) for s in range(KEY_SLOTS)}


def _counters_equal(rig, send):
    got = rig.eng.tx_counters_get(0, KEY_SLOTS).tolist()
    want = [send.get(s, 0) for s in range(KEY_SLOTS)]
    assert got == want, [(s, got[s], want[s]) for s in range(KEY_SLOTS) if got[s] != want[s]][:5]


def _route_plan(rig, table, pkts, send, seal_at=None):
    """One route-mode plan of pkts from the counters `send` against the model over `table`; seal_at =
    (first, count) also seals that slice of the descriptors and compares the whole wire ring. Returns
    the model's (descriptors, statuses, counters)."""
    ring, off, lens = ring_of(pkts)
    n = len(pkts)
    out_size = n * STRIDE
    want, want_st, new = M.plan(off, lens, ring, M.ROUTE, send, routes=table, wire_stride=STRIDE, out_size=out_size,
                                max_len=MAX_LEN)
    got, got_st, (d_ring, d_desc) = plan(rig, ring, off, lens, n, route=True, stride=STRIDE, out_size=out_size,
                                         max_len=MAX_LEN)
    bad = [(i, got_st[i], want_st[i], int(got["key_slot"][i]), int(want["key_slot"][i]), pkts[i][:40].hex())
           for i in range(n) if got_st[i] != want_st[i] or got["key_slot"][i] != want["key_slot"][i]]
    assert not bad, bad[:5]
    same_desc(got, want)
    _counters_equal(rig, new)
    if seal_at:
        a, k = seal_at
        wire = seal(rig, d_desc[a:a + k], d_ring, out_size, MAX_LEN)
        assert np.array_equal(wire, oracle_ring(rig, want[a:a + k], ring, out_size, MAX_LEN))
    return want, want_st, new


def _case_plan(rig, case, seed, seal_at=None):
    """routes_set(case.routes), then one plan of a packet per destination plus the eight special packets."""
    rng = np.random.default_rng(seed)
    pkts, where = E.packets(case.dests, rng, MAX_LEN)
    rig.eng.routes_set(case.routes)
    want, want_st, _ = _route_plan(rig, E.route_table(case), pkts, _start(rig, seed), seal_at)
    assert want_st.count(M.PKT_BADIP) == 4 and want_st.count(M.PKT_TOOLONG) == 2
    return want, want_st, where


def _slots(want, want_st, where):
    """Per destination the key slot the model routed it to, None where it has no route."""
    return [int(want["key_slot"][i]) if want_st[i] == M.PKT_OK else None for i in where.tolist()]


# ---- 1. ladders ------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True])
def test_ladders(rig, odd):
    """A route X/k for every k of 0..32 and 0..128 (the odd ladder: odd k only), written with X's own
    host bits; destination "bit k flipped" takes the /k slot (the next odd length below; none for bit 0),
    X the /32 and /128 slots, so each length of both families wins once, both /0 defaults among them."""
    case = E.ladder(odd)
    want, want_st, where = _case_plan(rig, case, 1100 + odd, seal_at=(0, len(case.dests) + 8))
    assert _slots(want, want_st, where) == E.ladder_expect(odd)
    assert [want_st[i] for i in where[[0, 33]].tolist()] == [M.PKT_NOROUTE if odd else M.PKT_OK] * 2


# ---- 2. prefixes nested inside one byte ------------------------------------------------------------
@pytest.mark.parametrize("family", [4, 6])
def test_same_byte_nests(rig, family):
    """Per byte position one table with a prefix at each of the eight lengths ending inside the byte,
    branches off their path, one prefix ending in the byte before and two in the byte after; the byte takes
    all 256 values, so every entry of that compiled node is read, and every route of the table wins."""
    for k, case in enumerate(E.nests(family)):
        want, want_st, where = _case_plan(rig, case, 1200 + 10 * family + k)
        routed = {s for s in _slots(want, want_st, where) if s is not None}
        assert routed == {s for _, _, s in case.routes}, case.name
        assert (None in _slots(want, want_st, where)) == (E.NEST_BYTES[family][k] > 0), case.name


# ---- 3. ties, host bits, the order of /0 -----------------------------------------------------------
def test_ties_host_bits_and_default_order(rig):
    """A prefix given two and three times with different slots, one network written with different host
    bits, a /0 before and after the other routes: the last entry wins, none of the earlier slots is used."""
    dead = {"a prefix given twice": {301, 304}, "a prefix given three times": {311, 312, 313, 314},
            "one network, other host bits": {321, 322, 324}, "/0 before and after": {341, 342},
            "/0 after the other routes": {351}}
    for k, case in enumerate(E.ties()):
        want, want_st, where = _case_plan(rig, case, 1300 + k)
        used = {s for s in _slots(want, want_st, where) if s is not None}
        assert used == {s for _, _, s in case.routes} - dead[case.name], case.name


# ---- 4. the random table ---------------------------------------------------------------------------
def test_random_table(rig):
    """2,000 routes of both families at lengths 0..32 and 0..128 with random host bits and 100 duplicates,
    20,000 packets; packets 9,000..11,000 are sealed and the whole wire ring compared with the oracle's."""
    case = E.random_table()
    want, want_st, where = _case_plan(rig, case, 1400, seal_at=(9000, 2000))
    slots = set(_slots(want, want_st, where))
    assert {0, KEY_SLOTS - 1} <= slots and len(slots) > 900 and None not in slots  # (it holds a /0 per family)
    assert want_st.count(M.PKT_OK) == 20002


# ---- 5. families without routes --------------------------------------------------------------------
def test_empty_families_and_the_empty_table(rig):
    """IPv4 routes only, IPv6 routes only, no routes set after a 2,000-route table, a /0 per family and
    nothing else: a family without routes gives WG_PKT_NOROUTE for every well-formed packet, while too
    long and bad IP keep their precedence."""
    v4, v6, none, zeros = E.empty_families()
    for k, case in enumerate((v4, v6)):
        want, want_st, where = _case_plan(rig, case, 1500 + k)
        empty = 16 if case is v4 else 4
        st = {len(d): set() for d in case.dests}
        for d, i in zip(case.dests, where.tolist()):
            st[len(d)].add(want_st[i])
        assert st[empty] == {M.PKT_NOROUTE} and st[20 - empty] == {M.PKT_OK, M.PKT_NOROUTE}
    rig.eng.routes_set(E.random_table().routes)
    want, want_st, where = _case_plan(rig, none, 1502)
    assert set(want_st) == {M.PKT_NOROUTE, M.PKT_BADIP, M.PKT_TOOLONG}
    assert [want_st[i] for i in where.tolist()] == [M.PKT_NOROUTE] * len(none.dests)
    want, want_st, where = _case_plan(rig, zeros, 1503)
    assert _slots(want, want_st, where) == [KEY_SLOTS - 1 if len(d) == 4 else 0 for d in zeros.dests]


# ---- 6. tables that move ---------------------------------------------------------------------------
def _moving_tables():
    small = E.Case("small table", E.small_table(), [])
    return [small, E.random_table(), small, E.empty_families()[2], E.ladder(False)]


def _moving_packets(seed):
    dests = E.around(E.small_table()) + E.random_table().dests[:400] + E.ladder(False).dests
    return E.packets(dests, np.random.default_rng(seed), MAX_LEN)[0]


def test_tables_of_changing_size(rig):
    """routes_set with 6, 2,000, 6, 0 and 162 routes in turn (the nodes grow, shrink and may move), one
    plan of the same packets after each, the counters running on from plan to plan."""
    pkts = _moving_packets(1600)
    send = _start(rig, 1600)
    seen = []
    for case in _moving_tables():
        rig.eng.routes_set(case.routes)
        want, want_st, send = _route_plan(rig, E.route_table(case), pkts, send)
        seen.append(want_st.count(M.PKT_OK))
    assert 20 < seen[0] == seen[2] < seen[1] and seen[3] == 0 and seen[1] == seen[4] == len(pkts) - 6  # (both hold /0s)


def test_captured_plan_follows_tables_of_changing_size(rig):
    """tx_reserve, one tx_plan captured, then replayed after each routes_set of the same sequence without
    re-capture: the captured launches read the table through its fixed header, wherever the nodes are."""
    torch, dev, eng = rig.torch, rig.dev, rig.eng
    pkts = _moving_packets(1601)
    ring, off, lens = ring_of(pkts)
    n = len(pkts)
    eng.routes_set([])
    send = _start(rig, 1601)
    eng.tx_reserve(n)
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    d_desc = torch.full((n + 2, 4), -0x0101010101010102, dtype=torch.int64, device=dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.tx_plan(d_ring, d_off, d_len, d_desc[:n], d_st[:n], STRIDE, n * STRIDE, MAX_LEN, route=True)
    _counters_equal(rig, send)  # capturing ran nothing
    for case in _moving_tables():
        eng.routes_set(case.routes)
        d_desc[:n].zero_()
        d_st[:n].fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, want_st, send = M.plan(off, lens, ring, M.ROUTE, send, routes=E.route_table(case), wire_stride=STRIDE,
                                     out_size=n * STRIDE, max_len=MAX_LEN)
        h_desc, h_st = d_desc.cpu().numpy(), d_st.cpu().numpy()
        assert (h_desc[n:] == -0x0101010101010102).all() and (h_st[n:] == GUARD).all(), case.name
        assert h_st[:n].tolist() == want_st, case.name
        same_desc(np.ascontiguousarray(h_desc[:n]).view(M.WG_PKT).reshape(-1), want)
        _counters_equal(rig, send)


# ---- 7. refused tables -----------------------------------------------------------------------------
def test_refused_tables_leave_the_old_one(rig):
    """wg_routes_set with family 4 / length 33, family 6 / length 129, family 5, and a key slot equal to
    key_slots as the last of 500 valid routes: WG_EINVAL, WG_EINVAL, WG_EINVAL, WG_ERANGE, and the next
    plan routes by the table set before."""
    L = rig.W._lib
    case = E.Case("small table", E.small_table(), E.around(E.small_table()))
    pkts, _ = E.packets(case.dests, np.random.default_rng(1700), MAX_LEN)
    rig.eng.routes_set(case.routes)
    send = _start(rig, 1700)

    def raw(entries):
        arr = (L.WgPrefix * len(entries))()
        slots = np.zeros(len(entries), np.uint32)
        for k, (family, plen, addr, slot) in enumerate(entries):
            arr[k].family, arr[k].prefix_len, slots[k] = family, plen, slot
            for i, x in enumerate(addr):
                arr[k].addr[i] = x
        return rig.eng._lib.wg_routes_set(rig.eng.ctx, ctypes.addressof(arr), slots.ctypes.data, len(entries))

    valid = [(4 if len(a.packed) == 4 else 6, p, a.packed, s) for a, p, s in E.random_table().routes[:499]]
    for entries, code in (([(4, 33, E.X4, 1)], L.WG_EINVAL), ([(6, 129, E.X6, 1)], L.WG_EINVAL),
                          ([(5, 8, E.X4, 1)], L.WG_EINVAL), (valid + [(4, 0, E.X4, KEY_SLOTS)], L.WG_ERANGE),
                          (valid + [(4, 33, E.X4, 1)], L.WG_EINVAL)):
        assert raw(entries) == code
        want, want_st, send = _route_plan(rig, E.route_table(case), pkts, send)
        assert want_st.count(M.PKT_OK) > 20 and M.PKT_NOROUTE in want_st
    assert raw(valid) == 0  # the valid part alone is accepted


# ---- 8. broadcast peer counts ----------------------------------------------------------------------
PEER_COUNTS = (2, 63, 64, 65, 128, 255, 256, 257, 1000)
PEER_STARTS = (0, (1 << 32) - 3, (1 << 63) - 1, (1 << 64) - 2)


@pytest.mark.parametrize("n_peers", PEER_COUNTS)
def test_broadcast_peer_counts(rig, n_peers):
    """n in {1, 63, 64, 65, 200} packets to n_peers peers spread over the key table in no order, their
    counters starting at 0, 2^32 - 3, 2^63 - 1 and 2^64 - 2 in turn: a keepalive, a packet of max_len + 1,
    one of stride - 32 + 1 and one of stride - 32, one running past in_size and a wire ring one byte short
    of its last slot (from n = 63), two plans in a row. 65 and 257 peers are sealed and the ring compared."""
    rng = np.random.default_rng(1800 + n_peers)
    max_len, stride = 100, 128
    peers = [int(s) for s in rng.permutation(KEY_SLOTS)[:n_peers]]
    peers[:2] = sorted(peers[:2], reverse=True)  # not in ascending order, whatever the draw
    rig.eng.tx_peers_set(peers)
    for n in (1, 63, 64, 65, 200):
        pkts = [rng.bytes(int(rng.integers(1, 61))) for _ in range(n)]
        pkts[0] = b""
        if n > 1:
            pkts[9], pkts[20], pkts[21] = rng.bytes(max_len + 1), rng.bytes(stride + 1 - 32), rng.bytes(stride - 32)
            pkts[n - 2], pkts[n - 1] = rng.bytes(40), rng.bytes(30)
        ring, off, lens = ring_of(pkts)
        n_desc = n * n_peers
        out_size = n_desc * stride
        if n > 1:
            lens[n - 2] = len(ring) - int(off[n - 2]) + 1  # 97 B <= max_len, but it runs one byte past in_size
            assert lens[n - 2] <= max_len
            out_size -= 1
        start = rng.integers(0, 1 << 62, KEY_SLOTS).astype(np.uint64)
        for k, s in enumerate(peers):
            start[s] = PEER_STARTS[k % 4]
        rig.eng.tx_counters_set(0, start)
        send = {s: int(start[s]) for s in range(KEY_SLOTS)}
        for again in range(2):
            want, want_st, send = M.plan(off, lens, ring, M.BROADCAST, send, peers=peers, wire_stride=stride,
                                         out_size=out_size, max_len=max_len)
            got, got_st, (d_ring, d_desc) = plan(rig, ring, off, lens, n_desc, route=False, stride=stride,
                                                 out_size=out_size, max_len=max_len)
            assert got_st == want_st, (n, again)
            same_desc(got, want)
            _counters_equal(rig, send)
            assert want_st.count(M.PKT_TOOLONG) == (4 * n_peers if n > 1 else 0) and want_st[0] == M.PKT_OK
            assert want["key_slot"][:n_desc].tolist() == peers * n
            if n_peers in (65, 257) and n in (65, 200):
                wire = seal(rig, d_desc, d_ring, out_size, max_len)
                assert np.array_equal(wire, oracle_ring(rig, want, ring, out_size, max_len))
        if n > 1:  # the peers that started at 2^64 - 2 wrapped, those at 2^32 - 3 carried
            assert send[peers[3 if n_peers > 3 else 1]] == ((PEER_STARTS[3 if n_peers > 3 else 1] + 2 * (n - 4))
                                                            & M.MASK64)
            assert send[peers[1]] == (1 << 32) - 3 + 2 * (n - 4)


# ---- 9. broadcast over more than 1,024 steps -------------------------------------------------------
def test_broadcast_runs_of_several_steps(rig):
    """66,000 packets of 20 B walked as 516 runs of two steps, to 1 peer and then to 2 (132,000
    descriptors): the single column's row prefix is advanced from the first step of a run to the second.
    One packet in 50 is too long, so ranks differ from indices; the counters start at 2^32 - 1,000."""
    n, stride, max_len = 66000, 64, 32
    off = np.arange(n, dtype=np.int64) * 32
    ring = np.zeros(n * 32 + 16, np.uint8)
    lens = np.full(n, 20, np.int64)
    lens[7::50] = max_len + 1
    for peers in ([4095], [4095, 3]):
        rig.eng.tx_peers_set(peers)
        start = np.zeros(KEY_SLOTS, np.uint64)
        start[peers] = (1 << 32) - 1000
        start[4] = 99  # a neighbour that no plan may touch
        rig.eng.tx_counters_set(0, start)
        n_desc = n * len(peers)
        want, want_st, send = M.plan(off, lens, ring, M.BROADCAST, {s: int(start[s]) for s in range(KEY_SLOTS)},
                                     peers=peers, wire_stride=stride, out_size=n_desc * stride, max_len=max_len)
        got, got_st, _ = plan(rig, ring, off, lens, n_desc, route=False, stride=stride, out_size=n_desc * stride,
                              max_len=max_len)
        assert got_st == want_st and want_st.count(M.PKT_TOOLONG) == 1320 * len(peers)
        same_desc(got, want)
        _counters_equal(rig, send)
        assert send[4095] == (1 << 32) - 1000 + 64680 and int(want["counter"].max()) == send[4095] - 1


# ---- 10. route-mode lanes --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["64_distinct_slots", "one_slot", "two_slots_alternating"])
def test_route_mode_lanes(rig, kind):
    """193 packets (three whole steps and a step with one active lane) over 64 /32 routes to 64 key slots:
    every step's lanes hold 64 distinct slots in an order that changes from step to step (64 rounds of
    wave_match), all hold one slot (one round), or they alternate between two slots whose counters start
    at 2^64 - 10 and wrap inside the first step."""
    rng = np.random.default_rng(2000)
    slots = [int(s) for s in rng.permutation(KEY_SLOTS)[:64]]
    addrs = [bytes([172, 16 + k % 5, k, 255 - k]) for k in range(64)]
    routes = [(E.ip(a), 32, s) for a, s in zip(addrs, slots)]
    n = 193
    if kind == "64_distinct_slots":
        pick = np.concatenate([rng.permutation(64) for _ in range(4)])[:n]
    elif kind == "one_slot":
        pick = np.full(n, 37)
    else:
        pick = np.where(np.arange(n) % 2 == 0, 5, 58)
    pkts = [E.packet(addrs[int(k)], int(rng.integers(20, MAX_LEN + 1)), rng) for k in pick]
    rig.eng.routes_set(routes)
    send = _start(rig, 2001)
    for s in (slots[5], slots[58]):
        send[s] = (1 << 64) - 10
        rig.eng.tx_counters_set(s, [send[s]])
    want, want_st, new = _route_plan(rig, M.RouteTable(routes), pkts, send, seal_at=(0, n))
    assert want_st == [M.PKT_OK] * n and want["key_slot"].tolist() == [slots[int(k)] for k in pick]
    for step in range(3):
        assert len(set(want["key_slot"][64 * step:64 * step + 64].tolist())) == {"64_distinct_slots": 64,
                                                                               "one_slot": 1}.get(kind, 2)
    if kind == "two_slots_alternating":
        assert new[slots[5]] == 97 - 10 and new[slots[58]] == 96 - 10
        assert want["counter"][:24:2].tolist() == [((1 << 64) - 10 + k) & M.MASK64 for k in range(12)]
