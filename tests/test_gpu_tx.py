"""wg_tx_plan on the MI355X against tests/tx_model.py (pytest -m gpu): descriptors, statuses and send
counters equal the model; the wire ring after seal(frame=True) equals the frozen oracle's
(oracle.seal_batch + oracle.frame_headers on the MODEL's descriptors), compared over the whole ring so
a stray write between packets fails too. The oracle has no validity test of its own, so it is given
the model's descriptors whose len is not WG_LEN_INVALID (the ones the seal and the framer accept)."""
import ipaddress

import numpy as np
import pytest

import tx_model as M
from tx_gpu import FILL, KEY_SLOTS, open_rig
from tx_gpu import counters as _counters
from tx_gpu import ipv4 as _ipv4
from tx_gpu import ipv6 as _ipv6
from tx_gpu import oracle_ring as _oracle_ring
from tx_gpu import plan as _plan
from tx_gpu import ring_of as _ring_of
from tx_gpu import same_desc as _same_desc
from tx_gpu import seal as _seal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    """This module's own engine (tests/tx_gpu.py::open_rig)."""
    r = open_rig()
    yield r
    r.eng.close()


# ---- 1. broadcast parity ---------------------------------------------------------------------
def test_broadcast_parity(rig):
    """70 packets of 0..300 B (one keepalive, one of max_len + 1, one running past in_size, one with
    len + 32 = stride + 1, one with len + 32 = stride), 3 peers, stride 512; the wire ring is one byte
    short of the last wire slot, so the last packet is rejected too. A second plan continues the counters."""
    rng = np.random.default_rng(101)
    max_len, stride, peers = 500, 512, [5, 4000, 17]
    pkts = [rng.bytes(int(rng.integers(1, 301))) for _ in range(70)]
    pkts[0] = b""
    pkts[9] = rng.bytes(max_len + 1)
    pkts[20] = rng.bytes(stride + 1 - 32)
    pkts[21] = rng.bytes(stride - 32)
    pkts[68], pkts[69] = rng.bytes(40), rng.bytes(30)
    ring, off, lens = _ring_of(pkts)
    lens[68] = len(ring) - int(off[68]) + 1  # 97 B <= max_len, but it runs one byte past in_size
    assert lens[68] <= max_len
    n_desc = 70 * 3
    out_size = n_desc * stride - 1
    rig.eng.tx_peers_set(peers)
    rig.eng.tx_counters_set(5, [123])
    rig.eng.tx_counters_set(4000, [(1 << 32) - 30])
    rig.eng.tx_counters_set(17, [0])
    rig.eng.tx_counters_set(6, [77])  # a neighbour that no plan may touch
    send = {5: 123, 4000: (1 << 32) - 30, 17: 0}
    for _ in range(2):
        want, want_st, send = M.plan(off, lens, ring, M.BROADCAST, send, peers=peers, wire_stride=stride,
                                     out_size=out_size, max_len=max_len)
        got, got_st, (d_ring, d_desc) = _plan(rig, ring, off, lens, n_desc, route=False, stride=stride,
                                              out_size=out_size, max_len=max_len)
        _same_desc(got, want)
        assert got_st == want_st
        assert want_st.count(M.PKT_TOOLONG) == 4 * 3 and want_st[0] == M.PKT_OK and want_st[21 * 3] == M.PKT_OK
        assert _counters(rig, peers + [6]) == {**send, 6: 77}
        wire = _seal(rig, d_desc, d_ring, out_size, max_len)
        assert np.array_equal(wire, _oracle_ring(rig, want, ring, out_size, max_len))
    assert send[5] == 123 + 2 * 66


# ---- 2. route parity -------------------------------------------------------------------------
A, B, C, D, E, F = 11, 22, 33, 4095, 0, 2048
ROUTES = [("0.0.0.0", 0, A), ("10.0.0.0", 8, B), ("10.1.0.0", 16, C), ("10.1.2.3", 32, D), ("2001:db8::", 32, E),
          ("2001:db8::1", 128, F)]
DESTS = ["10.0.255.255", "10.1.0.0", "10.1.255.255", "10.2.0.0", "11.0.0.0", "10.1.2.3", "10.1.2.2", "2001:db8::1",
         "2001:db8::2", "2001:db9::1"]


def _route_packets(rng, n, max_total=300):
    pkts = []
    for _ in range(n):
        k = rng.random()
        if k < 0.01:
            pkts.append(b"")
        elif k < 0.02:
            pkts.append(bytes([0x50 | int(rng.integers(0, 16))]) + rng.bytes(int(rng.integers(0, max_total))))
        elif k < 0.03:
            pkts.append(_ipv4("10.1.2.3", 19, rng))
        elif k < 0.04:
            pkts.append(_ipv6("2001:db8::1", 39, rng))
        else:
            dst = DESTS[int(rng.integers(0, len(DESTS)))]
            if ":" in dst:
                pkts.append(_ipv6(dst, int(rng.integers(40, max_total + 1)), rng))
            else:
                pkts.append(_ipv4(dst, int(rng.integers(20, max_total + 1)), rng))
    return pkts


def test_route_parity(rig):
    """20,000 packets over six routes (no IPv6 default), destinations on both sides of every prefix
    boundary, plus version nibble 5, a 19-B IPv4 and a 39-B IPv6 packet, keepalives and a packet longer
    than max_len. Per slot the counters read in batch order are base, base + 1, ..."""
    rng = np.random.default_rng(202)
    n, max_len, stride = 20000, 300, 336
    pkts = _route_packets(rng, n)
    pkts[0], pkts[1], pkts[2] = bytes([0x51]) + rng.bytes(50), _ipv4("10.1.2.3", 19, rng), _ipv6("2001:db8::1", 39, rng)
    pkts[3] = _ipv4("10.1.2.3", max_len + 1, rng)
    ring, off, lens = _ring_of(pkts)
    out_size = n * stride
    rig.eng.routes_set(ROUTES)
    base = {A: 5, B: (1 << 32) - 100, C: 0, D: (1 << 64) - 3, E: 1 << 40, F: 9}
    for s, v in base.items():
        rig.eng.tx_counters_set(s, [v])
    want, want_st, send = M.plan(off, lens, ring, M.ROUTE, base, routes=M.RouteTable(ROUTES), wire_stride=stride,
                                 out_size=out_size, max_len=max_len)
    got, got_st, (d_ring, d_desc) = _plan(rig, ring, off, lens, n, route=True, stride=stride, out_size=out_size,
                                          max_len=max_len)
    assert got_st == want_st
    assert {M.PKT_OK, M.PKT_BADIP, M.PKT_NOROUTE, M.PKT_TOOLONG} == set(want_st)
    assert got["key_slot"].tolist() == want["key_slot"].tolist()
    _same_desc(got, want)
    assert _counters(rig, base) == send
    ok = got["len"] != M.LEN_INVALID
    for s, v in base.items():
        ctr = got["counter"][ok & (got["key_slot"] == s)]
        assert len(ctr) > 100
        assert ctr.tolist() == [(v + k) & M.MASK64 for k in range(len(ctr))]
    wire = _seal(rig, d_desc, d_ring, out_size, max_len)
    assert np.array_equal(wire, _oracle_ring(rig, want, ring, out_size, max_len))


# ---- 3. rank across runs and under contention --------------------------------------------------
def test_rank_across_runs_and_under_contention(rig):
    """3,000 /32 routes to 3,000 key slots, 20,000 packets: half to one slot, the rest spread by a seeded
    draw; 100 slots (the heavy one among them) start at 2^32 - 5, so ranks carry into the high word.
    With 4,096 key slots this n is walked as R = 313 runs of one 64-packet step each (at most 1,024
    runs), so a slot's rank spans many runs and, for the heavy slot, about 32 lanes of every step."""
    rng = np.random.default_rng(303)
    n, nr, stride, max_len = 20000, 3000, 96, 60
    slots = rng.permutation(KEY_SLOTS)[:nr]
    addrs = [ipaddress.IPv4Address((10 << 24) + 257 * k + 1) for k in range(nr)]
    routes = [(a, 32, int(s)) for a, s in zip(addrs, slots)]
    rig.eng.routes_set(routes)
    heavy = 1234
    pick = np.where(rng.random(n) < 0.5, heavy, rng.integers(0, nr, n))
    lens = rng.integers(20, max_len + 1, n)
    ring = np.zeros(n * 64 + 16, np.uint8)
    off = np.arange(n, dtype=np.int64) * 64
    ring[off] = 0x45
    dst = np.array([list(a.packed) for a in addrs], np.uint8)[pick]
    for k in range(4):
        ring[off + 16 + k] = dst[:, k]
    high = set(int(s) for s in slots[rng.permutation(nr)[:99]]) | {int(slots[heavy])}
    start = np.zeros(KEY_SLOTS, np.uint64)
    for s in high:
        start[s] = (1 << 32) - 5
    rig.eng.tx_counters_set(0, start)
    want, want_st, send = M.plan(off, lens, ring, M.ROUTE, {s: int(start[s]) for s in range(KEY_SLOTS)},
                                 routes=M.RouteTable(routes), wire_stride=stride, out_size=n * stride, max_len=max_len)
    got, got_st, _ = _plan(rig, ring, off, lens, n, route=True, stride=stride, out_size=n * stride, max_len=max_len)
    assert want_st == [M.PKT_OK] * n
    assert got_st == want_st
    _same_desc(got, want)
    assert int(want["counter"].max()) > (1 << 32) + 9000  # the heavy slot crossed the carry
    assert rig.eng.tx_counters_get(0, KEY_SLOTS).tolist() == [send[s] for s in range(KEY_SLOTS)]


def test_runs_of_several_steps(rig):
    """More than 1,024 steps: 66,000 packets are walked as R = 516 runs of TWO steps (the row entry a
    group advanced in the first step is the prefix of the second), the last run one step short. Eight
    /32 routes, so every step holds several groups of lanes; descriptors and counters equal the model."""
    rng = np.random.default_rng(313)
    n, stride, max_len = 66000, 64, 32
    slots = [1, 64, 65, 4094, 2000, 7, 8, 9]
    addrs = [ipaddress.IPv4Address((192 << 24) + (168 << 16) + 256 * k + 1) for k in range(8)]
    routes = [(a, 32, s) for a, s in zip(addrs, slots)]
    rig.eng.routes_set(routes)
    pick = rng.integers(0, 9, n)  # 8: a destination without a route
    off = np.arange(n, dtype=np.int64) * 32
    ring = np.zeros(n * 32 + 16, np.uint8)
    ring[off] = 0x45
    dst = np.array([list(a.packed) for a in addrs] + [[192, 168, 77, 77]], np.uint8)[pick]
    for k in range(4):
        ring[off + 16 + k] = dst[:, k]
    lens = np.full(n, 20, np.int64)
    base = {s: (1 << 32) - 3000 + s for s in slots}
    for s, v in base.items():
        rig.eng.tx_counters_set(s, [v])
    want, want_st, send = M.plan(off, lens, ring, M.ROUTE, base, routes=M.RouteTable(routes), wire_stride=stride,
                                 out_size=n * stride, max_len=max_len)
    got, got_st, _ = _plan(rig, ring, off, lens, n, route=True, stride=stride, out_size=n * stride, max_len=max_len)
    assert got_st == want_st and set(want_st) == {M.PKT_OK, M.PKT_NOROUTE}
    _same_desc(got, want)
    assert _counters(rig, slots) == send


# ---- 4. edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [False, True])
def test_edges_small_batches(rig, route):
    """n in {0, 1, 63, 64, 65} (one lane, one step minus one, one step, one step plus one) in both
    modes, broadcast with 1 peer and with no peers: equal to the model, guard records intact."""
    rng = np.random.default_rng(404 + route)
    rig.eng.routes_set(ROUTES)
    stride, max_len = 336, 300
    for peers in ([7], []) if not route else ([],):
        if not route:
            rig.eng.tx_peers_set(peers)
        per = 1 if route else len(peers)
        for n in (0, 1, 63, 64, 65):
            pkts = _route_packets(rng, n)
            ring, off, lens = _ring_of(pkts)
            slots = [A, B, C, D, E, F, 7]
            base = {s: int(rng.integers(0, 1 << 62)) for s in slots}
            for s, v in base.items():
                rig.eng.tx_counters_set(s, [v])
            out_size = n * per * stride
            want, want_st, send = M.plan(off, lens, ring, M.ROUTE if route else M.BROADCAST, base, peers=peers,
                                         routes=M.RouteTable(ROUTES), wire_stride=stride, out_size=out_size,
                                         max_len=max_len)
            got, got_st, _ = _plan(rig, ring, off, lens, n * per, route=route, stride=stride, out_size=out_size,
                                   max_len=max_len)
            assert got_st == want_st, (n, peers)
            _same_desc(got, want)
            assert _counters(rig, slots) == send, (n, peers)


# ---- 5. state ------------------------------------------------------------------------------------
def test_counter_state_and_peer_validation(rig):
    eng, W = rig.eng, rig.W
    vals = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
    eng.tx_counters_set(100, vals)
    assert eng.tx_counters_get(100, 5).tolist() == vals
    # a new key is a new SymmetricKeypair: its counter starts at 0, no other slot's does
    eng.set_keys(102, rig.keys[32 * 102:32 * 103])
    assert eng.tx_counters_get(100, 5).tolist() == [0, 1, 0, 1 << 32, (1 << 64) - 1]
    eng.zero_keys(103, 1)
    eng.set_keys(103, rig.keys[32 * 103:32 * 104])
    assert eng.tx_counters_get(100, 5).tolist() == [0, 1, 0, 0, (1 << 64) - 1]
    # the same plan twice from the same counters: identical descriptor bytes
    rng = np.random.default_rng(505)
    eng.routes_set(ROUTES)
    pkts = _route_packets(rng, 3000)
    ring, off, lens = _ring_of(pkts)
    runs = []
    for _ in range(2):
        for s in (A, B, C, D, E, F):
            eng.tx_counters_set(s, [1000 + s])
        got, st, _ = _plan(rig, ring, off, lens, 3000, route=True, stride=336, out_size=3000 * 336, max_len=300)
        runs.append((got.tobytes(), st))
    assert runs[0] == runs[1]
    with pytest.raises(W.WgError) as e:
        eng.tx_peers_set([3, 9, 3])
    assert e.value.code == W._lib.WG_EINVAL
    with pytest.raises(W.WgError) as e:
        eng.tx_peers_set([3, KEY_SLOTS])
    assert e.value.code == W._lib.WG_ERANGE
    with pytest.raises(W.WgError) as e:
        eng.routes_set([("10.0.0.0", 8, KEY_SLOTS)])
    assert e.value.code == W._lib.WG_ERANGE


def test_plans_on_two_streams_are_ordered_by_the_library(rig):
    """Eight plans issued back to back on two streams, alternating, with no synchronisation between
    them: they share the counters and the scratch, so the library chains them; every plan's descriptors
    equal the model run in issue order, and set_keys afterwards zeroes a counter only after them."""
    torch, dev, eng = rig.torch, rig.dev, rig.eng
    rng = np.random.default_rng(515)
    eng.routes_set(ROUTES)
    n, stride, max_len = 5000, 336, 300
    ring, off, lens = _ring_of(_route_packets(rng, n))
    send = {s: 10 * s for s in (A, B, C, D, E, F)}
    for s, v in send.items():
        eng.tx_counters_set(s, [v])
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    outs = [(torch.zeros((n, 4), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
            for _ in range(8)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for k, (d_desc, d_st) in enumerate(outs):
        eng.tx_plan(d_ring, d_off, d_len, d_desc, d_st, stride, n * stride, max_len, route=True,
                    stream=streams[k % 2].cuda_stream)
    eng.set_keys(B, rig.keys[32 * B:32 * (B + 1)])  # ordered after the eight plans
    torch.cuda.synchronize()
    T = M.RouteTable(ROUTES)
    for d_desc, d_st in outs:
        want, want_st, send = M.plan(off, lens, ring, M.ROUTE, send, routes=T, wire_stride=stride,
                                     out_size=n * stride, max_len=max_len)
        assert d_st.cpu().numpy().tolist() == want_st
        _same_desc(d_desc.cpu().numpy().view(M.WG_PKT).reshape(-1), want)
    assert send[B] > 10 * B + 8 * 500
    assert _counters(rig, send) == {**send, B: 0}


# ---- 6. the whole path on the device ---------------------------------------------------------
def test_tun_ring_to_wire_and_back_on_the_device(rig):
    """Route plan -> seal + frame -> parse_open on the produced ring -> open -> rx_check(FILTER | REPLAY)
    with the window enabled: every routed packet is WG_PKT_OK and its plaintext equals the tun bytes; a
    second planned batch is accepted; the first ring fed in again is all WG_PKT_REPLAY."""
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    rng = np.random.default_rng(606)
    n, max_len, stride = 2000, 150, 336  # the plaintext lands behind the wire packet: 2 (len + 32) - 32 <= stride
    pkts = [p for p in _route_packets(rng, n, max_total=max_len)]
    ring, off, lens = _ring_of(pkts)
    eng.routes_set(ROUTES)
    eng.replay_enable(8192)
    for s in (A, B, C, D, E, F):
        eng.tx_counters_set(s, [0])
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    rings = []
    for batch in range(2):
        d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        wire = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
        eng.tx_seal(d_ring, d_off, d_len, d_desc, d_st, wire, stride, max_len, route=True)
        torch.cuda.synchronize()
        tx_st = d_st.cpu().numpy()
        desc = d_desc.cpu().numpy().view(M.WG_PKT).reshape(-1)
        sent = np.nonzero(tx_st == M.PKT_OK)[0]
        assert 1500 < len(sent) < n
        rings.append((wire, desc, sent))
    for feed, (wire, desc, sent) in enumerate(rings + rings[:1]):
        w_off = torch.from_numpy((sent * stride).astype(np.int64)).to(dev)
        w_len = torch.from_numpy((desc["len"][sent] + 32).astype(np.uint32).view(np.int32)).to(dev)
        w_slot = torch.from_numpy(desc["key_slot"][sent].astype(np.uint32).view(np.int32)).to(dev)
        o_desc = torch.zeros((len(sent), 4), dtype=torch.int64, device=dev)
        o_st = torch.zeros(len(sent), dtype=torch.int32, device=dev)
        eng.parse_open(wire, w_off, w_len, w_slot, o_desc, o_st)
        eng.open(o_desc, wire, wire, o_st, max_len)
        torch.cuda.synchronize()
        assert (o_st.cpu().numpy() == W._lib.WG_PKT_OK).all()
        eng.rx_check(o_desc, wire, o_st, W._lib.WG_RX_FILTER | W._lib.WG_RX_REPLAY)
        torch.cuda.synchronize()
        st = o_st.cpu().numpy()
        if feed < 2:
            assert (st == W._lib.WG_PKT_OK).all(), np.bincount(st)
            h = wire.cpu().numpy()
            for j in sent[:: max(1, len(sent) // 200)]:
                L = int(desc["len"][j])
                got = h[j * stride + 32 + L:j * stride + 32 + 2 * L]
                assert np.array_equal(got, ring[int(off[j]):int(off[j]) + L]), j
        else:
            assert (st == W._lib.WG_PKT_REPLAY).all(), np.bincount(st)
    eng.replay_enable(0)


# ---- 7. graph ----------------------------------------------------------------------------------
def test_captured_plan_replays_and_continues_the_counters(rig):
    """tx_reserve, then tx_plan + seal(frame=True) captured on torch's capture stream and replayed three
    times: each replay's ring equals the model with the counters advanced. Equal-length packets and
    WG_F_UNIFORM for the seal (a mixed-length seal inside a graph is another matter). A route change
    between replays needs no re-capture. A plan on a capturing stream that needs more scratch than was
    reserved returns WG_EINVAL."""
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    rng = np.random.default_rng(707)
    n, L, stride = 300, 64, 96
    pkts = []
    for i in range(n):
        dst = DESTS[int(rng.integers(0, len(DESTS)))]
        p = _ipv6(dst, L, rng) if ":" in dst else _ipv4(dst, L, rng)
        pkts.append(bytes([0x50]) + p[1:] if i % 37 == 5 else p)
    ring, off, lens = _ring_of(pkts)
    out_size = n * stride
    routes = list(ROUTES)
    eng.routes_set(routes)
    send = {A: 1, B: (1 << 32) - 200, C: 3, D: 4, E: 5, F: 6}
    for s, v in send.items():
        eng.tx_counters_set(s, [v])
    eng.tx_reserve(n)
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    wire = torch.full((out_size,), FILL, dtype=torch.uint8, device=dev)
    big = 70000  # more than any plan of this module reserved
    b_off = torch.zeros(big, dtype=torch.int64, device=dev)
    b_len = torch.zeros(big, dtype=torch.int32, device=dev)
    b_desc = torch.zeros((big, 4), dtype=torch.int64, device=dev)
    b_st = torch.zeros(big, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(W.WgError) as e:
            eng.tx_plan(d_ring, b_off, b_len, b_desc, b_st, stride, out_size, L, route=True)
        eng.tx_plan(d_ring, d_off, d_len, d_desc, d_st, stride, out_size, L, route=True)
        eng.seal(d_desc, d_ring, wire, L, uniform=True, frame=True)
    assert e.value.code == W._lib.WG_EINVAL and "wg_tx_reserve" in str(e.value)
    assert _counters(rig, send) == send  # capturing ran nothing
    for replay in range(3):
        if replay == 2:  # a route change between replays: the captured plan reads the new table
            routes[1] = ("10.0.0.0", 8, 77)
            eng.routes_set(routes)
            send[77] = 0
            eng.tx_counters_set(77, [0])
        wire.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, want_st, send = M.plan(off, lens, ring, M.ROUTE, send, routes=M.RouteTable(routes), wire_stride=stride,
                                     out_size=out_size, max_len=L)
        assert d_st.cpu().numpy().tolist() == want_st
        _same_desc(d_desc.cpu().numpy().view(M.WG_PKT).reshape(-1), want)
        assert np.array_equal(wire.cpu().numpy(), _oracle_ring(rig, want, ring, out_size, L))
        assert _counters(rig, send) == send
