"""The transmit-plan model (tests/tx_model.py) on hand-written cases, the layout of wg_tx_batch and
the new status codes; the tables of tests/tx_edge_cases.py under the model and under the builder's own
brute-force lookup. No GPU: tests/test_gpu_tx.py and tests/test_gpu_tx_edges.py hold the library to this
model on the device."""
import ctypes
import os
import re
import subprocess

import pytest

import tx_edge_cases as E
import tx_model as M
from wgtest import ROOT, wg

HEADER = os.path.join(ROOT, "include/wgaead.h")


def _ipv4(dst: str, total: int = 40) -> bytes:
    import ipaddress
    p = bytearray(max(total, 20))
    p[0] = 0x45
    p[16:20] = ipaddress.ip_address(dst).packed
    return bytes(p[:total])


def _ipv6(dst: str, total: int = 60) -> bytes:
    import ipaddress
    p = bytearray(max(total, 40))
    p[0] = 0x60
    p[24:40] = ipaddress.ip_address(dst).packed
    return bytes(p[:total])


def test_broadcast_three_packets_two_peers():
    """j = t * peers + p; counters base + r; the invalid middle packet takes no counter."""
    ring = bytes(range(256)) * 2
    off, ln = [0, 100, 300], [50, 200, 10]  # packet 1: 200 > max_len 100
    desc, st, send = M.plan(off, ln, ring, M.BROADCAST, {7: 1000, 3: 5}, peers=[7, 3], wire_stride=256,
                            out_size=6 * 256, max_len=100)
    want = [
        # in_off, out_off, counter, len, key_slot
        (0, 0 * 256 + 16, 1000, 50, 7), (0, 1 * 256 + 16, 5, 50, 3),
        (100, 2 * 256 + 16, 0, M.LEN_INVALID, 7), (100, 3 * 256 + 16, 0, M.LEN_INVALID, 3),
        (300, 4 * 256 + 16, 1001, 10, 7), (300, 5 * 256 + 16, 6, 10, 3),
    ]
    assert [tuple(int(x) for x in d) for d in desc] == want
    assert st == [0, 0, M.PKT_TOOLONG, M.PKT_TOOLONG, 0, 0]
    assert send == {7: 1002, 3: 7}


def test_broadcast_size_checks_and_keepalive():
    ring = bytes(64)
    # keepalive ok; runs past in_size; len + 32 = stride + 1; last wire slot past out_size
    desc, st, send = M.plan([0, 60, 0, 0], [0, 5, 33, 1], ring, M.BROADCAST, {}, peers=[1], wire_stride=64,
                            out_size=3 * 64 + 63, max_len=1000)
    assert st == [0, M.PKT_TOOLONG, M.PKT_TOOLONG, M.PKT_TOOLONG]
    assert int(desc[0]["len"]) == 0 and int(desc[0]["counter"]) == 0
    assert send == {1: 1}
    # no peers: nothing planned
    desc, st, send = M.plan([0], [0], ring, M.BROADCAST, {1: 9}, peers=[], wire_stride=64, out_size=64, max_len=10)
    assert len(desc) == 0 and st == [] and send == {1: 9}


def test_counter_wraps_like_a_java_long():
    desc, st, send = M.plan([0, 0, 0], [1, 1, 1], b"\0", M.BROADCAST, {0: (1 << 64) - 2}, peers=[0], wire_stride=64,
                            out_size=192, max_len=1)
    assert [int(d["counter"]) for d in desc] == [(1 << 64) - 2, (1 << 64) - 1, 0]
    assert send == {0: 1}


ROUTES = [("0.0.0.0", 0, 1), ("10.0.0.0", 8, 2), ("10.1.0.0", 16, 3), ("10.1.2.3", 32, 4), ("2001:db8::", 32, 5),
          ("2001:db8::1", 128, 6)]
EXPECT = [
    ("9.255.255.255", 1), ("10.0.0.0", 2), ("10.0.255.255", 2), ("10.1.0.0", 3), ("10.1.255.255", 3),
    ("10.2.0.0", 2), ("10.255.255.255", 2), ("11.0.0.0", 1), ("10.1.2.3", 4), ("10.1.2.2", 3), ("10.1.2.4", 3),
    ("255.255.255.255", 1),
    ("2001:db8::1", 6), ("2001:db8::", 5), ("2001:db8::2", 5), ("2001:db8:ffff:ffff:ffff:ffff:ffff:ffff", 5),
    ("2001:db9::", None), ("2001:db7:ffff:ffff:ffff:ffff:ffff:ffff", None), ("::1", None),
]


def test_route_table_by_hand():
    """Both sides of every prefix boundary; a /32 and a /128 that match; no IPv6 default route."""
    import ipaddress
    T = M.RouteTable(ROUTES)
    for addr, slot in EXPECT:
        assert T.lookup(ipaddress.ip_address(addr).packed) == slot, addr
    # of equal prefixes the later entry wins
    T2 = M.RouteTable(ROUTES + [("10.1.77.0", 16, 9)])
    assert T2.lookup(ipaddress.ip_address("10.1.0.1").packed) == 9
    assert T2.lookup(ipaddress.ip_address("10.1.2.3").packed) == 4


def test_route_plan_statuses_and_per_slot_ranks():
    pk = [_ipv4("10.1.2.3"), _ipv4("11.0.0.1"), b"", _ipv4("10.1.2.3"), bytes([0x50]) + bytes(40), _ipv6("2001:db9::1"),
          _ipv4("10.1.2.3", 19), _ipv6("2001:db8::1", 39), _ipv6("2001:db8::1", 40), _ipv4("11.0.0.1", 20),
          _ipv4("10.9.9.9", 500)]
    off, ring = [], b""
    for p in pk:
        off.append(len(ring))
        ring += p
    desc, st, send = M.plan(off, [len(p) for p in pk], ring, M.ROUTE, {4: (1 << 32) - 1, 1: 7},
                            routes=M.RouteTable(ROUTES), wire_stride=128, out_size=128 * len(pk), max_len=100)
    assert st == [0, 0, M.PKT_BADIP, 0, M.PKT_BADIP, M.PKT_NOROUTE, M.PKT_BADIP, M.PKT_BADIP, 0, 0, M.PKT_TOOLONG]
    assert [int(d["key_slot"]) for d in desc] == [4, 1, 0, 4, 0, 0, 0, 0, 6, 1, 0]
    assert [int(d["counter"]) for d in desc] == [(1 << 32) - 1, 7, 0, 1 << 32, 0, 0, 0, 0, 0, 8, 0]
    assert [int(d["len"]) for d in desc][:4] == [40, 40, M.LEN_INVALID, 40]
    assert [int(d["out_off"]) for d in desc] == [128 * j + 16 for j in range(len(pk))]
    assert send == {4: (1 << 32) + 1, 1: 9, 6: 1}


def test_tx_batch_layout_matches_header(tmp_path):
    fields = ["in", "in_size", "pkt_off", "pkt_len", "desc_out", "tx_status", "wire_base", "wire_stride", "out_size",
              "n", "max_len", "mode", "_reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\n'
                   'int main(void){printf("%zu", sizeof(wg_tx_batch));'
                   + "".join(f' printf(" %zu", offsetof(wg_tx_batch, {f}));' for f in fields)
                   + ' printf(" %u %u %u %u\\n", WG_PKT_NOROUTE, WG_PKT_TOOLONG, WG_TX_BROADCAST, WG_TX_ROUTE);'
                     ' return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    L = wg()._lib
    T = L.WgTxBatch
    names = ["in_" if f == "in" else f for f in fields]
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in names] + [
        L.WG_PKT_NOROUTE, L.WG_PKT_TOOLONG, L.WG_TX_BROADCAST, L.WG_TX_ROUTE]


def test_status_codes_match_header_and_model():
    L = wg()._lib
    src = open(HEADER).read()
    assert re.search(rf"#define WG_PKT_NOROUTE {L.WG_PKT_NOROUTE}u\b", src)
    assert re.search(rf"#define WG_PKT_TOOLONG {L.WG_PKT_TOOLONG}u\b", src)
    assert (M.PKT_NOROUTE, M.PKT_TOOLONG, M.PKT_BADIP, M.PKT_OK) == (L.WG_PKT_NOROUTE, L.WG_PKT_TOOLONG,
                                                                   L.WG_PKT_BADIP, L.WG_PKT_OK)
    assert M.LEN_INVALID == L.WG_LEN_INVALID and (M.BROADCAST, M.ROUTE) == (L.WG_TX_BROADCAST, L.WG_TX_ROUTE)
    assert M.WG_PKT == wg().WG_PKT_DTYPE


def test_engine_exposes_the_transmit_api():
    E = wg().Engine
    for name in ("tx_peers_set", "routes_set", "tx_counters_set", "tx_counters_get", "tx_reserve", "tx_plan", "tx_seal"):
        assert callable(getattr(E, name))


# ---- the edge tables (tests/tx_edge_cases.py) ----------------------------------------------------
def _winners(case):
    """Per distinct destination of the case, (prefix length, key slot) or None by the brute-force lookup."""
    B = E.Brute(case.routes)
    return {d: B.lookup(d) for d in set(case.dests)}


@pytest.mark.parametrize("case", E.all_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_model_lookup_equals_brute_force(case):
    """RouteTable.lookup (ipaddress networks) against the builder's masked byte compare, on every table
    and every destination that goes to the device."""
    T = E.route_table(case)
    for d, hit in _winners(case).items():
        assert T.lookup(d) == (hit[1] if hit else None), (case.name, E.ip(d), hit)


@pytest.mark.parametrize("odd", [False, True])
def test_ladder_resolves_bit_k_to_slash_k(odd):
    """Full ladder: bit k flipped -> the /k slot for every k of both families, X -> /32 and /128, so
    every length wins once, both /0 among them. Odd ladder: the next odd length below, nothing for bit 0."""
    case, want = E.ladder(odd), E.ladder_expect(odd)
    assert len(set(case.dests)) == len(case.dests) == 33 + 129
    assert len(case.routes) == (80 if odd else 162) and len({s for _, _, s in case.routes}) == len(case.routes)
    assert all(a.packed in (E.X4, E.X6) for a, _, _ in case.routes)  # host bits as X has them
    T, B = E.route_table(case), E.Brute(case.routes)
    assert [T.lookup(d) for d in case.dests] == want
    assert [(B.lookup(d) or (None, None))[1] for d in case.dests] == want
    if odd:
        assert want[0] is None and want[33] is None and want[32] == E.ladder_slot(4, 31)
        assert want[2] == E.ladder_slot(4, 1) and want[33 + 128] == E.ladder_slot(6, 127)
    else:
        assert want[:33] == [E.ladder_slot(4, k) for k in range(33)]
        assert want[33:] == [E.ladder_slot(6, k) for k in range(129)]
        assert sorted(B.lookup(d)[0] for d in case.dests) == sorted(list(range(33)) + list(range(129)))


@pytest.mark.parametrize("family", [4, 6])
def test_every_route_of_a_nest_wins_and_every_byte_value_is_asked(family):
    for case in E.nests(family):
        b = E.NEST_BYTES[family][E.nests(family).index(case)]
        win = _winners(case)
        assert {h[1] for h in win.values() if h} == {s for _, _, s in case.routes}, case.name
        lens = sorted(p for _, p, _ in case.routes)
        assert [lens.count(8 * b + j) for j in range(1, 9)] == [1, 1, 2, 1, 1, 2, 1, 2]  # all eight end in byte b
        assert lens[0] == 8 * b and (lens[-1] == 8 * b + 9) == (b + 1 < len(case.dests[0]))
        assert {d[b] for d in case.dests[:256]} == set(range(256))
        assert (None in win.values()) == (b > 0)


def test_ties_go_to_the_later_entry():
    by_name = {c.name: c for c in E.ties()}
    look = lambda name, addr: E.Brute(by_name[name].routes).lookup(E.ipaddress.ip_address(addr).packed)  # noqa: E731
    assert look("a prefix given twice", "10.20.3.4") == (14, 303)
    assert look("a prefix given twice", "10.20.200.4") == (17, 305)
    assert look("a prefix given twice", "fd00:1234:7::1") == (45, 306)
    assert look("a prefix given three times", "192.168.77.1") == (32, 316)
    assert look("a prefix given three times", "2001:db8:5:ffff::") == (47, 317)
    assert look("one network, other host bits", "10.20.0.0") == (14, 323)
    assert look("one network, other host bits", "10.22.9.9") == (15, 326)
    assert look("one network, other host bits", "fd00:1234:0:1::") == (45, 325)
    assert look("/0 before and after", "9.9.9.9") == (0, 343)
    assert look("/0 before and after", "::1") == (0, 344)
    assert look("/0 after the other routes", "9.9.9.9") == (0, 353)
    assert look("/0 after the other routes", "::1") == (0, 352)


def test_random_table_covers_the_prefix_lengths():
    """On the reference alone: at least 30 of the 33 IPv4 lengths and 100 of the 129 IPv6 lengths win for
    some destination, duplicates exist and decide lookups, both ends of the key table are routed to."""
    case = E.random_table()
    assert len(case.routes) == 2000 and len(case.dests) == 20000
    win = _winners(case)
    assert len({h[0] for d, h in win.items() if h and len(d) == 4}) >= 30
    assert len({h[0] for d, h in win.items() if h and len(d) == 16}) >= 100
    slots = {s for _, _, s in case.routes}
    assert 0 in slots and E.KEY_SLOTS - 1 in slots and max(slots) < E.KEY_SLOTS
    keys = [(a, p) for a, p, _ in case.routes]
    assert 80 <= len(keys) - len(set(keys)) <= 120  # about 5 % are an earlier (address, length) again
    first = {}
    for a, p, s in case.routes:
        first.setdefault((a, p), s)
    F = E.Brute([(a, p, first[(a, p)]) for a, p, _ in case.routes])  # the table if the FIRST entry won
    assert sum(F.lookup(d) != h for d, h in win.items()) > 20
    assert any(a.packed != E.ipaddress.ip_network((a, p), strict=False).network_address.packed
               for a, p, _ in case.routes)  # host bits set behind the prefix


def test_no_route_occurs_and_empty_families_route_nothing():
    cases = {c.name: c for c in E.empty_families()}
    for name, fams in (("IPv4 routes only", {4}), ("IPv6 routes only", {16}), ("no routes", set())):
        win = _winners(cases[name])
        assert {len(d) for d, h in win.items() if h} == fams and None in win.values(), name
        assert {len(d) for d in win} == {4, 16}
    win = _winners(cases["a /0 per family and nothing else"])
    assert {h for h in win.values()} == {(0, E.KEY_SLOTS - 1), (0, 0)}
    assert None in _winners(E.ladder(True)).values()


def test_packets_carry_their_destination_and_the_specials():
    import numpy as np
    case = E.ladder(False)
    pkts, where = E.packets(case.dests, np.random.default_rng(1), max_len=60)
    assert len(pkts) == len(case.dests) + 8 and sorted(len(p) for p in pkts)[0] == 0
    for k, d in enumerate(case.dests):
        p = pkts[int(where[k])]
        assert M.destination(p) == d and (40 if len(d) == 16 else 20) <= len(p) <= 60
    rest = [p for i, p in enumerate(pkts) if i not in set(where.tolist())]
    assert sorted(len(p) for p in rest) == [0, 19, 20, 31, 39, 40, 61, 61]
    assert sum(M.destination(p) is None for p in rest) == 5
