"""wg_rx_plan / wg_rx_deliver on the MI355X against tests/rx_plan_model.py (pytest -m gpu): descriptors,
statuses, the handshake list, the delivery list and both summaries are compared exactly; the whole
receive path (plan -> open -> rx_check -> deliver) is run on rings the transmit path produced."""
import ipaddress
import struct

import numpy as np
import pytest

import rx_plan_model as M
from wgtest import oracle, splitmix_np, wg

pytestmark = pytest.mark.gpu

KEY_SLOTS = 1024
R = 256  # kRankRange of wg_plan.hip: packets per workgroup of the classify / emit launches
SCAN_CHUNK = 256  # ranges the scan launch takes per trip: more than R * SCAN_CHUNK packets take a second trip
GUARD = 0x7E7E7E7E
FILL = 0x5A
SHAPES = [0, 1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1, 5000]


@pytest.fixture(scope="module")
def rig():
    """This module's own engine (its session table, routes and counters must not leak into other
    files' tests), one key per slot, a receiver index per slot."""
    import torch
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    W = wg()
    eng = W.Engine(0, key_slots=KEY_SLOTS)
    keys = splitmix_np(0x8C5, 32 * KEY_SLOTS)
    eng.set_keys(0, keys)
    receivers = (np.arange(KEY_SLOTS, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.set_receivers(torch.from_numpy(receivers.view(np.int32)).to(dev))
    yield type("Rig", (), dict(eng=eng, keys=keys, receivers=receivers, torch=torch, dev=dev, W=W))
    eng.close()


def _bucket(index, n):
    """The bucket of include/wgaead.h's session table for n entries."""
    cap = 16
    while cap < 4 * n:
        cap *= 2
    h = index & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h & (cap - 1)


@pytest.fixture(scope="module")
def table():
    """1,000 random 32-bit receiver indices, among them 0, 0xFFFFFFFF and eight that share the bucket
    of index 0 (a probe chain of at least nine), mapped to key slots."""
    rng = np.random.default_rng(77)
    idx = {0, 0xFFFFFFFF}
    cand = rng.integers(1, 1 << 32, 400000, dtype=np.uint64)
    same = [int(x) for x in cand if _bucket(int(x), 1000) == _bucket(0, 1000)][:8]
    assert len(same) == 8
    idx.update(same)
    while len(idx) < 1000:
        idx.add(int(rng.integers(0, 1 << 32)))
    idx = sorted(idx)
    rng.shuffle(idx)
    slots = rng.integers(0, KEY_SLOTS, 1000)
    return {int(i): int(s) for i, s in zip(idx, slots)}, same


def _set_sessions(rig, sess):
    rig.eng.rx_sessions_set(list(sess.keys()), list(sess.values()))


def _mix(rng, n, sess, max_len):
    """A UDP ring of n datagrams at unaligned offsets: types 1, 2, 3, 4 and other bytes, lengths on both
    sides of every bound, about 10% unknown receiver indices; the last datagrams run past the ring, two
    start past it. Returns (ring, offsets, lengths)."""
    known = list(sess.keys())
    edge = [0, 1, 15, 31, 32, 33, 48, max_len + 31, max_len + 32, max_len + 33]
    buf, off, lens = bytearray(rng.bytes(3)), [], []
    for k in range(n):
        r = rng.random()
        t = 4 if r < 0.72 else 1 if r < 0.78 else 2 if r < 0.84 else 3 if r < 0.87 else int(rng.integers(0, 256))
        wl = int(rng.choice(edge)) if rng.random() < 0.3 else int(rng.integers(32, max_len + 34))
        index = int(rng.integers(0, 1 << 32)) if rng.random() < 0.1 else known[int(rng.integers(0, len(known)))]
        p = bytearray(rng.bytes(max(wl, 16)))
        p[0:16] = struct.pack("<BxxxIQ", t, index, int(rng.integers(0, 1 << 64, dtype=np.uint64)))
        off.append(len(buf))
        lens.append(wl)
        buf += p[:wl] + bytes(int(rng.integers(0, 4)))
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    for k in range(max(0, n - 3), n):  # the tail: lengths that run past the ring by one byte and more
        lens[k] = len(ring) - off[k] + 1 + (n - 1 - k) * 7
    if n >= 40:
        off[n // 2], off[n // 3] = len(ring) + 1, (1 << 64) - 20
        off[n // 4], lens[n // 4] = len(ring), 1  # starts exactly at the end
    return ring, np.array(off, np.uint64), np.array(lens, np.uint32)


def _plan(rig, ring, off, lens, *, max_len, packed, pt_base=0, pt_size=0, stream=None, d_ring=None):
    """Runs wg_rx_plan; returns (desc, status list, host_list[:n_host], summary dict, device tensors).
    Every output array carries guard words behind its n entries."""
    torch, dev = rig.torch, rig.dev
    n = len(off)
    d_ring = torch.from_numpy(ring).to(dev) if d_ring is None else d_ring
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32)).to(dev)
    d_desc = torch.full((n + 2, 4), -0x0101010101010102, dtype=torch.int64, device=dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_host = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sum = torch.full((4,), -1, dtype=torch.int64, device=dev)
    rig.eng.rx_plan(d_ring, d_off, d_len, d_desc[:n], d_st[:n], d_host[:n], d_sum[:2], max_len, packed=packed,
                    pt_base=pt_base, pt_size=pt_size, stream=stream)
    torch.cuda.synchronize()
    h_desc, h_st, h_host, h_sum = d_desc.cpu().numpy(), d_st.cpu().numpy(), d_host.cpu().numpy(), d_sum.cpu().numpy()
    assert (h_desc[n:] == -0x0101010101010102).all() and (h_st[n:] == GUARD).all() and (h_host[n:] == GUARD).all()
    assert (h_sum[2:] == -1).all(), "summary guard overwritten"
    s = dict(pt_used=int(h_sum[:1].view(np.uint64)[0]), n_open=int(h_sum[1:2].view(np.uint32)[0]),
             n_host=int(h_sum[1:2].view(np.uint32)[1]))
    assert (h_host[s["n_host"]:n] == GUARD).all(), "host_list written past n_host"
    desc = np.ascontiguousarray(h_desc[:n]).view(M.WG_PKT).reshape(-1)
    return desc, h_st[:n].tolist(), h_host[:s["n_host"]].tolist(), s, (d_ring, d_desc[:n], d_st[:n])


def _same_desc(got, want):
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]][:5]


def _check_plan(rig, ring, off, lens, sess, **kw):
    want, want_st, want_host, want_s = M.plan(ring, off, lens, sess, max_len=kw["max_len"],
                                              mode=M.PT_PACKED if kw["packed"] else M.PT_AFTER,
                                              pt_base=kw.get("pt_base", 0), pt_size=kw.get("pt_size", 0))
    got, got_st, got_host, got_s, dv = _plan(rig, ring, off, lens, **kw)
    assert got_st == want_st, [(i, a, b) for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:5]
    assert got_host == want_host
    assert got_s == want_s
    _same_desc(got, want)
    return want, want_st, want_host, want_s, dv


# ---- 1. plan parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_plan_parity(rig, table, packed):
    """Every shape (one lane, a wave and a workgroup range R minus / plus one, 2R + 1, 5,000) over the
    random mix, in both modes; the packed ring starts at an odd multiple of 16 and holds about 90% of the
    larger batches' plaintext, so a tail of TOOLONG packets is part of it."""
    sess, same = table
    _set_sessions(rig, sess)
    rng = np.random.default_rng(1000 + packed)
    max_len = 200
    for n in SHAPES:
        ring, off, lens = _mix(rng, n, sess, max_len)
        if n:  # the colliding indices, known and present: the probe walks the whole chain
            k = 0
            for i in range(n):
                if lens[i] >= 32 and int(off[i]) + int(lens[i]) <= len(ring) and ring[int(off[i])] == 4 and k < 8:
                    ring[int(off[i]) + 4:int(off[i]) + 8] = np.frombuffer(struct.pack("<I", same[k]), np.uint8)
                    k += 1
        kw = dict(max_len=max_len, packed=packed)
        if packed:
            full = M.plan(ring, off, lens, sess, max_len=max_len, mode=M.PT_PACKED, pt_base=48, pt_size=1 << 40)[3]
            kw.update(pt_base=48, pt_size=48 + (1 << 20 if n < 1000 else full["pt_used"] * 9 // 10))
        want, want_st, host, s, _ = _check_plan(rig, ring, off, lens, sess, **kw)
        if n == 5000:
            assert {M.PKT_OK, M.PKT_BADHDR, M.PKT_HANDSHAKE, M.PKT_NOSESSION, M.PKT_TOOLONG} == set(want_st)
            assert len(host) > 300 and want_st.count(M.PKT_NOSESSION) > 200
            if packed:
                assert s["pt_used"] > kw["pt_size"] - 48 > 100000
                assert (want["out_off"][np.array(want_st) == 0] % 16 == 0).all()
                cut = int(np.nonzero(want["out_off"] == want["out_off"].max())[0][-1])
                assert M.PKT_OK not in want_st[cut + 1:] and want_st[cut + 1:].count(M.PKT_TOOLONG) > 100


def test_plan_parity_second_scan_trip(rig, table):
    """R * SCAN_CHUNK + 1 packets: the scan launch takes a second trip over the per-range sums and carries
    the 64-bit byte prefix and both counts into it (packed mode, every packet of one of three lengths)."""
    sess, _ = table
    _set_sessions(rig, sess)
    rng = np.random.default_rng(1100)
    n, max_len = R * SCAN_CHUNK + 1, 64
    known = np.array(list(sess.keys()), np.uint32)
    wl = rng.choice(np.array([32, 49, 96], np.uint32), n)
    at = np.arange(n, dtype=np.int64) * 96 + 1
    off = at.astype(np.uint64)
    ring = np.zeros(n * 96 + 1, np.uint8)
    types = rng.choice(np.array([4, 4, 4, 4, 4, 4, 4, 1, 2, 7], np.uint8), n)
    ring[at] = types
    index = known[rng.integers(0, len(known), n)]
    index[rng.random(n) < 0.1] = 0x12345678
    assert 0x12345678 not in sess
    for k in range(4):
        ring[at + 4 + k] = ((index >> (8 * k)) & 0xFF).astype(np.uint8)
    ring[at + 8] = (np.arange(n) & 0xFF).astype(np.uint8)
    want, want_st, host, s, _ = _check_plan(rig, ring, off, wl, sess, max_len=max_len, packed=True, pt_base=0,
                                            pt_size=1 << 30)
    assert host[-1] > R * SCAN_CHUNK - 200 and s["n_open"] > 35000 and s["pt_used"] > 35000 * 16


# ---- 2. packed overflow ----------------------------------------------------------------------------
def test_packed_overflow_cuts_the_batch(rig, table):
    """2,000 known transport packets, pt_size ends inside packet 1,000's plaintext: everything from there
    on is TOOLONG, pt_used is the full sum, n_open the packets before the cut."""
    sess, _ = table
    _set_sessions(rig, sess)
    rng = np.random.default_rng(1200)
    n, max_len = 2000, 300
    known = list(sess.keys())
    lens_pt = rng.integers(0, max_len + 1, n)
    lens_pt[1000], lens_pt[1001], lens_pt[1500] = 200, 0, 0
    buf, off = bytearray(b"\0"), []
    for k in range(n):
        off.append(len(buf))
        buf += struct.pack("<BxxxIQ", 4, known[k % len(known)], k) + rng.bytes(int(lens_pt[k]) + 16)
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    cut = int(sum(M.align16(int(x)) for x in lens_pt[:1000])) + 100
    want, want_st, _, s, _ = _check_plan(rig, ring, np.array(off, np.uint64), (lens_pt + 32).astype(np.uint32), sess,
                                         max_len=max_len, packed=True, pt_base=32, pt_size=32 + cut)
    assert want_st == [M.PKT_OK] * 1000 + [M.PKT_TOOLONG] * 1000
    assert s["n_open"] == 1000 and s["pt_used"] == int(sum(M.align16(int(x)) for x in lens_pt))


# ---- 3. agreement with wg_parse_open -----------------------------------------------------------------
def test_after_mode_agrees_with_parse_open(rig, table):
    """All type 4, all known, AFTER mode: byte-identical descriptors and equal statuses to wg_parse_open
    fed the key slots a host lookup gives, the ring's last packets (whose plaintext overruns it) included."""
    torch, dev = rig.torch, rig.dev
    sess, _ = table
    _set_sessions(rig, sess)
    rng = np.random.default_rng(1300)
    n = 3000
    known = list(sess.keys())
    buf, off, lens, slots = bytearray(b"\0\0\0"), [], [], []
    for k in range(n):
        wl = int(rng.integers(32, 200)) if k < n - 1 else 100
        index = known[int(rng.integers(0, len(known)))]
        off.append(len(buf))
        lens.append(wl)
        slots.append(sess[index])
        buf += struct.pack("<BxxxIQ", 4, index, int(rng.integers(0, 1 << 63))) + rng.bytes(wl - 16 + int(rng.integers(0, 3)))
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    off, lens = np.array(off, np.uint64), np.array(lens, np.uint32)
    got, got_st, host, s, (d_ring, _, _) = _plan(rig, ring, off, lens, max_len=65535, packed=False)
    p_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    p_st = torch.zeros(n, dtype=torch.int32, device=dev)
    rig.eng.parse_open(d_ring, torch.from_numpy(off.view(np.int64)).to(dev),
                       torch.from_numpy(lens.view(np.int32)).to(dev),
                       torch.from_numpy(np.array(slots, np.uint32).view(np.int32)).to(dev), p_desc, p_st)
    torch.cuda.synchronize()
    assert got_st == p_st.cpu().numpy().tolist()
    assert got.tobytes() == p_desc.cpu().numpy().tobytes()
    assert M.PKT_BADHDR in got_st and got_st.count(M.PKT_OK) > n - 10 and host == [] and s["pt_used"] == 0


# ---- 4. deliver parity -------------------------------------------------------------------------------
def _deliver(rig, desc, plan_st, open_st, with_index=True):
    torch, dev = rig.torch, rig.dev
    n = len(desc)
    d_desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.int64).reshape(-1, 4)).to(dev) if n else \
        torch.zeros((0, 4), dtype=torch.int64, device=dev)
    d_p = torch.from_numpy(np.asarray(plan_st, np.int32)).to(dev)
    d_o = torch.from_numpy(np.asarray(open_st, np.int32)).to(dev)
    d_f = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_items = torch.full((n + 2, 2), -0x0101010101010102, dtype=torch.int64, device=dev)
    d_idx = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sum = torch.full((4,), -1, dtype=torch.int64, device=dev)
    rig.eng.rx_deliver(d_desc, d_p, d_o, d_f[:n], d_items[:n], d_sum[:2], index_out=d_idx[:n] if with_index else None)
    torch.cuda.synchronize()
    h_f, h_items, h_idx, h_sum = d_f.cpu().numpy(), d_items.cpu().numpy(), d_idx.cpu().numpy(), d_sum.cpu().numpy()
    s = dict(bytes=int(h_sum[:1].view(np.uint64)[0]), n_items=int(h_sum[1:2].view(np.uint32)[0]),
             n_keepalive=int(h_sum[1:2].view(np.uint32)[1]))
    k = s["n_items"]
    assert (h_f[n:] == GUARD).all() and (h_sum[2:] == -1).all()
    assert (h_items[k:] == -0x0101010101010102).all(), "items written past n_items"
    assert (h_idx[k if with_index else 0:] == GUARD).all(), "index_out written past n_items"
    items = np.ascontiguousarray(h_items[:k]).view(M.RX_ITEM).reshape(-1)
    return h_f[:n].tolist(), items, h_idx[:k].tolist(), s


def test_deliver_parity(rig):
    """Random plan and open statuses over every shape, plus all-OK and none-OK batches of 5,000: final
    statuses, items, index_out and the totals equal the model; index_out may be left out."""
    rng = np.random.default_rng(1400)
    cases = [(n, "mix") for n in SHAPES] + [(5000, "all"), (5000, "none"), (R * SCAN_CHUNK + 1, "mix")]
    for n, kind in cases:
        desc = np.zeros(n, M.WG_PKT)
        desc["out_off"] = rng.integers(0, 1 << 62, n, dtype=np.uint64) if n < 70000 else (1 << 40) + np.arange(n)
        desc["len"], desc["key_slot"] = rng.integers(0, 70000, n), rng.integers(0, KEY_SLOTS, n)
        desc["in_off"], desc["counter"] = rng.integers(0, 1 << 62, n, dtype=np.uint64), np.arange(n)
        if kind == "mix":
            plan_st = rng.choice([0, 0, 0, 0, 0, 0, M.PKT_BADHDR, M.PKT_TOOLONG, M.PKT_NOSESSION, M.PKT_HANDSHAKE], n)
            open_st = rng.choice([0, 0, 0, 0, M.PKT_BADTAG, M.PKT_KEEPALIVE, M.PKT_BADIP, M.PKT_FILTERED, M.PKT_REPLAY], n)
        elif kind == "all":
            plan_st, open_st = np.zeros(n, np.int64), np.zeros(n, np.int64)
        else:
            plan_st, open_st = np.full(n, M.PKT_NOSESSION), rng.choice([0, M.PKT_BADTAG, M.PKT_KEEPALIVE], n)
        want_f, want_items, want_idx, want_s = M.deliver(desc, plan_st, open_st)
        for with_index in ((True, False) if n == 5000 else (True,)):
            got_f, got_items, got_idx, got_s = _deliver(rig, desc, plan_st, open_st, with_index)
            assert got_f == want_f, (n, kind)
            assert got_s == want_s, (n, kind)
            assert got_items.tobytes() == want_items.tobytes(), (n, kind)
            if with_index:
                assert got_idx == want_idx, (n, kind)
        if kind == "all":
            assert want_s["n_items"] == n
        if kind == "none":
            assert want_s["n_items"] == 0 and want_s["n_keepalive"] == 0


# ---- 5. table validation and state ---------------------------------------------------------------------
def test_table_validation_and_state(rig):
    eng, W = rig.eng, rig.W
    rng = np.random.default_rng(1500)
    sess = {5: 1, 0: 2, 0xFFFFFFFF: 3, 0x80000000: KEY_SLOTS - 1}
    index = [5, 0, 0xFFFFFFFF, 0x80000000, 6, 5, 0, 0xFFFFFFFF]
    buf, off = bytearray(), []
    for k, x in enumerate(index):
        off.append(len(buf))
        buf += struct.pack("<BxxxIQ", 4, x, k) + rng.bytes(16 + 8 * k)
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    off, lens = np.array(off, np.uint64), np.array([32 + 8 * k for k in range(8)], np.uint32)
    kw = dict(max_len=100, packed=True, pt_base=0, pt_size=4096)
    eng.rx_sessions_set(list(sess.keys()), list(sess.values()))
    want, want_st, _, _, _ = _check_plan(rig, ring, off, lens, sess, **kw)
    assert want_st == [0, 0, 0, 0, M.PKT_NOSESSION, 0, 0, 0] and int(want["key_slot"][3]) == KEY_SLOTS - 1
    with pytest.raises(W.WgError) as e:  # a repeated index: refused, and the old table still answers
        eng.rx_sessions_set([6, 9, 6], [1, 2, 3])
    assert e.value.code == W._lib.WG_EINVAL
    _check_plan(rig, ring, off, lens, sess, **kw)
    with pytest.raises(W.WgError) as e:  # a key slot past the table
        eng.rx_sessions_set([6, 9], [1, KEY_SLOTS])
    assert e.value.code == W._lib.WG_ERANGE
    _check_plan(rig, ring, off, lens, sess, **kw)
    # a set between two plans changes the second plan only
    sess2 = {6: 7, 5: 8}
    eng.rx_sessions_set(list(sess2.keys()), list(sess2.values()))
    _, st2, _, _, _ = _check_plan(rig, ring, off, lens, sess2, **kw)
    assert st2 == [0, M.PKT_NOSESSION, M.PKT_NOSESSION, M.PKT_NOSESSION, 0, 0, M.PKT_NOSESSION, M.PKT_NOSESSION]
    eng.rx_sessions_set([], [])  # cleared: every transport packet is NOSESSION
    _, st3, _, s3, _ = _check_plan(rig, ring, off, lens, {}, **kw)
    assert st3 == [M.PKT_NOSESSION] * 8 and s3 == dict(pt_used=0, n_open=0, n_host=0)


# ---- 6. the whole path on the device -------------------------------------------------------------------
A, B, C, D, E, F = 11, 22, 33, 1023, 0, 512
ROUTES = [("0.0.0.0", 0, A), ("10.0.0.0", 8, B), ("10.1.0.0", 16, C), ("10.1.2.3", 32, D), ("2001:db8::", 32, E),
          ("2001:db8::1", 128, F)]
DESTS = ["10.0.255.255", "10.1.0.0", "10.1.255.255", "11.0.0.0", "10.1.2.3", "2001:db8::1", "2001:db8::2"]


def _ip(dst, total, rng):
    a = ipaddress.ip_address(dst)
    p = bytearray(rng.bytes(total))
    if a.version == 4:
        p[0] = 0x45
        p[16:20] = a.packed
    else:
        p[0] = 0x60 | (p[0] & 0x0F)
        p[24:40] = a.packed
    return bytes(p)


def test_tun_ring_to_wire_to_tun_ring_on_the_device(rig):
    """2,000 IPv4 / IPv6 tun packets: tx_plan(ROUTE) -> seal(frame) gives the UDP ring; the test flips tag
    bits in 2% of it, overwrites type bytes with 1, 2 and 9, rewrites receiver indices to unknown values and
    appends copies of a few packets; rx_plan(PACKED) -> open(WG_F_RX_FILTER) -> rx_check(WG_RX_REPLAY) ->
    rx_deliver. The items are exactly the model's, every item's bytes are the tun packet's, the final
    statuses are the model's merge of plan status, a bad tag, oracle/rx.py's verdict and its replay window.
    The slots the transmit plan left untouched (no route) stay filler bytes: BADHDR."""
    from oracle import rx
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    rng = np.random.default_rng(1600)
    n, max_len, stride, extra = 2000, 150, 192, 12
    pkts = []
    for i in range(n):
        dst = DESTS[int(rng.integers(0, len(DESTS)))]
        pkts.append(_ip(dst, int(rng.integers(40, max_len + 1)), rng))
    for i in range(0, n, 97):
        pkts[i] = bytes([0x50]) + pkts[i][1:]  # no route: the wire slot stays untouched
    lens = np.array([len(p) for p in pkts], np.int64)
    t_off = np.arange(n, dtype=np.int64) * 160
    tun = np.zeros(n * 160, np.uint8)
    for o, p in zip(t_off, pkts):
        tun[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    eng.routes_set(ROUTES)
    eng.replay_enable(8192)
    slots = [A, B, C, D, E, F]
    for s in slots:
        eng.tx_counters_set(s, [0])
    sess = {int(rig.receivers[s]): s for s in slots}
    _set_sessions(rig, sess)
    d_tun = torch.from_numpy(tun).to(dev)
    d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_wire = torch.full(((n + extra) * stride,), FILL, dtype=torch.uint8, device=dev)
    eng.tx_seal(d_tun, torch.from_numpy(t_off).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), d_desc, d_st,
                d_wire, stride, max_len, route=True)
    torch.cuda.synchronize()
    tx_st = d_st.cpu().numpy()
    sent = np.nonzero(tx_st == M.PKT_OK)[0]
    assert 1900 < len(sent) < n
    wire = d_wire.cpu().numpy()
    # the edits, on disjoint packets
    pick = rng.permutation(sent)
    forged, retyped, reindexed, copied = pick[:40], pick[40:49], pick[49:55], pick[55:55 + extra]
    for j in forged:
        wire[j * stride + 16 + lens[j] + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
    for k, j in enumerate(retyped):
        wire[j * stride] = (1, 2, 9)[k % 3]
    for j in reindexed:
        wire[j * stride + 4:j * stride + 8] = np.frombuffer(struct.pack("<I", 0xDEAD0000 + int(j)), np.uint8)
    src = list(range(n)) + [int(j) for j in copied]  # batch position -> tun packet
    for k, j in enumerate(copied):
        wire[(n + k) * stride:(n + k + 1) * stride] = wire[j * stride:(j + 1) * stride]
    m = n + extra
    w_off = np.arange(m, dtype=np.uint64) * stride
    w_len = np.array([int(lens[j]) + 32 for j in src], np.uint32)
    pt_size = 64 + int(sum(M.align16(int(x)) for x in lens)) + extra * 160
    # the model: plan, then what open + rx_check make of the packets the plan passed
    want, want_st, want_host, want_s = M.plan(wire, w_off, w_len, sess, max_len=max_len, mode=M.PT_PACKED, pt_base=64,
                                              pt_size=pt_size)
    is_forged = set(int(j) for j in forged)
    open_st = []
    for i in range(m):
        if want_st[i] != M.PKT_OK:
            open_st.append(M.PKT_BADTAG)
        elif src[i] in is_forged:
            open_st.append(M.PKT_BADTAG)
        else:
            open_st.append(rx.process_decrypted(pkts[src[i]], None))
    open_st = rx.ReplayWindow(8192).check_batch(want["key_slot"].tolist(), want["counter"].tolist(), open_st)
    want_f, want_items, want_idx, want_d = M.deliver(want, want_st, open_st)
    assert {M.PKT_OK, M.PKT_BADTAG, M.PKT_BADHDR, M.PKT_HANDSHAKE, M.PKT_NOSESSION, M.PKT_REPLAY} == set(want_f)
    assert want_f.count(M.PKT_REPLAY) == extra and want_f.count(M.PKT_HANDSHAKE) == 6 and len(want_host) == 6
    # the device
    d_wire = torch.from_numpy(wire).to(dev)
    d_woff = torch.from_numpy(w_off.view(np.int64)).to(dev)
    d_wlen = torch.from_numpy(w_len.view(np.int32)).to(dev)
    r_desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    r_st, r_host, o_st, f_st, r_idx = (torch.full((m,), GUARD, dtype=torch.int32, device=dev) for _ in range(5))
    r_sum, r_del = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    r_items = torch.zeros((m, 2), dtype=torch.int64, device=dev)
    d_pt = torch.full((pt_size,), FILL, dtype=torch.uint8, device=dev)
    eng.rx_open(d_wire, d_woff, d_wlen, r_desc, r_st, r_host, r_sum, d_pt, o_st, f_st, r_items, r_del, max_len,
                packed=True, pt_base=64, index_out=r_idx, replay=True)
    torch.cuda.synchronize()
    eng.replay_enable(0)
    assert r_st.cpu().numpy().tolist() == want_st
    _same_desc(r_desc.cpu().numpy().view(M.WG_PKT).reshape(-1), want)
    h_sum = r_sum.cpu().numpy()
    assert int(h_sum[0]) == want_s["pt_used"] and h_sum[1:2].view(np.uint32).tolist() == [want_s["n_open"], 6]
    assert r_host.cpu().numpy()[:6].tolist() == want_host
    assert f_st.cpu().numpy().tolist() == want_f
    h_del = r_del.cpu().numpy()
    k = want_d["n_items"]
    assert int(h_del[0]) == want_d["bytes"] and h_del[1:2].view(np.uint32).tolist() == [k, 0]
    items = np.ascontiguousarray(r_items.cpu().numpy()[:k]).view(M.RX_ITEM).reshape(-1)
    assert items.tobytes() == want_items.tobytes()
    assert r_idx.cpu().numpy()[:k].tolist() == want_idx
    used = min(want_s["pt_used"], pt_size - 64)
    pt = d_pt[64:64 + used].cpu().numpy()  # the D2H leg: plaintext only
    assert used < 0.6 * len(wire)
    for it, i in zip(items, want_idx):
        o, L = int(it["off"]) - 64, int(it["len"])
        assert pt[o:o + L].tobytes() == pkts[src[i]], i


# ---- 7. two streams ----------------------------------------------------------------------------------------
def test_plans_on_two_streams_both_match_the_model(rig, table):
    """Six plans of two different batches issued back to back on two streams, alternating, with no
    synchronisation between them: they share the scratch, the library chains them, each equals the model."""
    torch, dev, eng = rig.torch, rig.dev, rig.eng
    sess, _ = table
    _set_sessions(rig, sess)
    rng = np.random.default_rng(1700)
    max_len = 120
    batches = []
    for n in (5000, 3001):
        ring, off, lens = _mix(rng, n, sess, max_len)
        want = M.plan(ring, off, lens, sess, max_len=max_len, mode=M.PT_PACKED, pt_base=16, pt_size=1 << 24)
        batches.append((torch.from_numpy(ring).to(dev), torch.from_numpy(off.view(np.int64)).to(dev),
                        torch.from_numpy(lens.view(np.int32)).to(dev), n, want))
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = []
    torch.cuda.synchronize()
    for k in range(6):
        d_ring, d_off, d_len, n, want = batches[k % 2]
        o = (torch.zeros((n, 4), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
             torch.full((n,), GUARD, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
        eng.rx_plan(d_ring, d_off, d_len, o[0], o[1], o[2], o[3], max_len, packed=True, pt_base=16, pt_size=1 << 24,
                    stream=streams[k % 2].cuda_stream)
        outs.append((o, want))
    torch.cuda.synchronize()
    for (d_desc, d_st, d_host, d_sum), (want, want_st, want_host, want_s) in outs:
        assert d_st.cpu().numpy().tolist() == want_st
        _same_desc(d_desc.cpu().numpy().view(M.WG_PKT).reshape(-1), want)
        assert d_host.cpu().numpy()[:len(want_host)].tolist() == want_host
        h = d_sum.cpu().numpy()
        assert int(h[0]) == want_s["pt_used"] and h[1:2].view(np.uint32).tolist() == [want_s["n_open"], want_s["n_host"]]


# ---- 8. graph ------------------------------------------------------------------------------------------------
def test_captured_plan_open_deliver_replays(rig):
    """rx_reserve, then rx_plan + open(WG_F_UNIFORM | WG_F_RX_FILTER) + rx_deliver captured once over 600
    equal-length packets and replayed three times; between replays the wire ring is rewritten in place
    (other packets forged, retyped, reindexed) and wg_rx_sessions_set replaces the table, without
    re-capture. Each replay equals the model. A plan on a capturing stream that needs more scratch than was
    reserved returns WG_EINVAL."""
    from oracle import rx
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    O = oracle()
    rng = np.random.default_rng(1800)
    n, L, stride = 600, 64, 112
    slots = [3, 70, 900, 5]
    pkts = [_ip(DESTS[int(rng.integers(0, len(DESTS)))], L, rng) for _ in range(n)]
    pkts[7] = bytes([0x15]) + pkts[7][1:]  # opens, then BADIP
    pt_in = np.frombuffer(b"".join(pkts), np.uint8).copy()
    slot_of = [slots[i % 4] for i in range(n)]
    sd = np.zeros(n, M.WG_PKT)
    sd["in_off"], sd["out_off"] = np.arange(n) * L, np.arange(n) * stride + 16
    sd["counter"], sd["len"], sd["key_slot"] = np.arange(n) + 1000, L, slot_of
    clean = np.full(n * stride, FILL, np.uint8)
    O.seal_batch(sd, pt_in, clean, rig.keys, threads=4)
    O.frame_headers(sd, rig.receivers, clean, KEY_SLOTS, len(pt_in), L)
    w_off = np.arange(n, dtype=np.uint64) * stride
    w_len = np.full(n, L + 32, np.uint32)
    pt_size = n * L
    d_wire = torch.from_numpy(clean.copy()).to(dev)
    d_off = torch.from_numpy(w_off.view(np.int64)).to(dev)
    d_len = torch.from_numpy(w_len.view(np.int32)).to(dev)
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, o_st, f_st, r_idx = (torch.full((n,), GUARD, dtype=torch.int32, device=dev) for _ in range(5))
    r_sum, r_del = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    r_items = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    d_pt = torch.zeros(pt_size, dtype=torch.uint8, device=dev)
    big = 300000  # more than any batch of this module reserved
    b_off = torch.zeros(big, dtype=torch.int64, device=dev)
    b_len = torch.zeros(big, dtype=torch.int32, device=dev)
    b_desc = torch.zeros((big, 4), dtype=torch.int64, device=dev)
    b_st = torch.zeros(big, dtype=torch.int32, device=dev)
    b_host = torch.zeros(big, dtype=torch.int32, device=dev)

    def pipeline():
        eng.rx_open(d_wire, d_off, d_len, r_desc, r_st, r_host, r_sum, d_pt, o_st, f_st, r_items, r_del, L,
                    packed=True, index_out=r_idx, uniform=True)

    sess = {int(rig.receivers[s]): s for s in slots}
    _set_sessions(rig, sess)
    eng.rx_reserve(n)
    pipeline()  # eager once: the open's filter tables exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(W.WgError) as e:
            eng.rx_plan(d_wire, b_off, b_len, b_desc, b_st, b_host, r_sum, L, packed=True, pt_size=pt_size)
        pipeline()
    assert e.value.code == W._lib.WG_EINVAL and "wg_rx_reserve" in str(e.value)
    for replay in range(3):
        wire = clean.copy()
        pick = rng.permutation(n)
        forged, retyped, reindexed = set(int(j) for j in pick[:15]), pick[15:21], pick[21:25]
        for j in forged:
            wire[j * stride + 16 + L + 3] ^= 0x40
        for k, j in enumerate(retyped):
            wire[j * stride] = (1, 2, 200)[k % 3]
        for j in reindexed:
            wire[j * stride + 4:j * stride + 8] = np.frombuffer(struct.pack("<I", 0xBEEF0000 + replay), np.uint8)
        if replay == 1:  # one session fewer: the captured plan reads the new table
            sess = {int(rig.receivers[s]): s for s in slots[:3]}
            _set_sessions(rig, sess)
        if replay == 2:  # back, with the unknown index now known (under a wrong key: BADTAG)
            sess = {int(rig.receivers[s]): s for s in slots}
            sess[0xBEEF0002] = 8
            _set_sessions(rig, sess)
        d_wire.copy_(torch.from_numpy(wire))
        d_pt.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, want_st, want_host, want_s = M.plan(wire, w_off, w_len, sess, max_len=L, mode=M.PT_PACKED, pt_base=0,
                                                  pt_size=pt_size)
        open_st = [M.PKT_BADTAG if (want_st[i] != M.PKT_OK or i in forged or int(want["key_slot"][i]) != slot_of[i])
                   else rx.process_decrypted(pkts[i], None) for i in range(n)]
        want_f, want_items, want_idx, want_d = M.deliver(want, want_st, open_st)
        assert r_st.cpu().numpy().tolist() == want_st, replay
        _same_desc(r_desc.cpu().numpy().view(M.WG_PKT).reshape(-1), want)
        assert r_host.cpu().numpy()[:len(want_host)].tolist() == want_host and len(want_host) == 4
        h = r_sum.cpu().numpy()
        assert int(h[0]) == want_s["pt_used"] and h[1:2].view(np.uint32).tolist() == [want_s["n_open"], 4]
        assert f_st.cpu().numpy().tolist() == want_f, replay
        assert M.PKT_BADIP in want_f or 7 in forged or want_st[7] != 0
        k = want_d["n_items"]
        h = r_del.cpu().numpy()
        assert int(h[0]) == want_d["bytes"] == k * L and h[1:2].view(np.uint32).tolist() == [k, 0]
        assert np.ascontiguousarray(r_items.cpu().numpy()[:k]).tobytes() == want_items.tobytes()
        assert r_idx.cpu().numpy()[:k].tolist() == want_idx
        pt = d_pt.cpu().numpy()
        for it, i in zip(want_items, want_idx):
            assert pt[int(it["off"]):int(it["off"]) + L].tobytes() == pkts[i], (replay, i)
        if replay == 1:
            assert want_st.count(M.PKT_NOSESSION) > 100
        if replay == 2:
            assert want_f.count(M.PKT_BADTAG) >= 15 + 4 - 1
