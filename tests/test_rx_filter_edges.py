"""The receive-side AllowedIPs case set (tests/rx_filter_edge_cases.py) checked against itself, so that
tests/test_gpu_rx_filter_edges.py cannot pass on cases that ask nothing: every expected status against a second
statement of IPFilter.search that has no trie, and what the builders claim about their probes (which are inside,
which outside, which packet edges occur). No GPU."""
from collections import Counter

import numpy as np
import pytest

import rx_filter_edge_cases as E
from oracle import rx

C = E.cases()


def _by_filter(part):
    out = {}
    for p in C.probes:
        if p.part == part:
            out.setdefault(p.fid, []).append(p)
    return out


def _within(a, p, dst):
    """dst lies in the network a/p (a /32 or /128 holds its one address, whatever IPFilter.search makes of it)."""
    return len(a.packed) == len(dst) and (int(a) ^ int.from_bytes(dst, "big")) >> (len(dst) * 8 - p) == 0


def test_every_status_agrees_with_the_closed_form():
    """process_decrypted's answer for every probe, from integer shifts alone: a match iff some inserted prefix of the
    destination's family with prefix_len < nbits equals the destination in its first prefix_len bits. The keepalive
    and bad-IP rules are restated here from TransportManager.java:98-130 without oracle/rx.py's helpers."""
    asked = 0
    for p in C.probes:
        pt, dst = p.pt, None
        if len(pt) == 0:
            want = rx.PKT_KEEPALIVE
        elif pt[0] >> 4 == 4 and len(pt) >= 20:
            dst = pt[16:20]
        elif pt[0] >> 4 == 6 and len(pt) >= 40:
            dst = pt[24:40]
        else:
            want = rx.PKT_BADIP
        if dst is not None:
            assert dst == p.dst, (C.names[p.fid], p.kind)
            if p.fid == E.NO_FILTER:
                want = rx.PKT_OK
            else:
                want = rx.PKT_OK if E.closed_form(C.filters.get(p.fid, []), dst) else rx.PKT_FILTERED
                assert E.filter_of(C, p.fid).search(dst) == (want == rx.PKT_OK), (C.names[p.fid], p.kind, E.ip(dst))
                asked += 1
        assert p.status == want, (C.names[p.fid], p.kind, pt[:40].hex())
    assert asked > 1000


def test_closed_form_equals_the_trie_at_every_prefix_length():
    """IPFilter.search against the closed form for X/p at every p of both families, asked with every single-bit flip
    of X and X itself: 33 x 33 + 129 x 129 searches."""
    for X in (E.X4, E.X6):
        nbits = len(X) * 8
        dests = [E.flip(X, k) for k in range(nbits)] + [X]
        for p in range(nbits + 1):
            f = E.oracle_filter([(E.ip(X), p)])
            for k, d in enumerate(dests):
                assert f.search(d) == E.closed_form([(E.ip(X), p)], d) == (p < nbits and (k >= p)), (p, k)


@pytest.mark.parametrize("family", [4, 6])
def test_single_prefix_filters_are_asked_on_both_sides(family):
    """(a): a filter per length 0 .. nbits; for 0 < p < nbits at least one probe passes and one is filtered, and the
    two addresses that differ from the base at bit p - 1 and at bit p are on opposite sides; /nbits lets nothing
    through, /0 everything of its family; the other family is always filtered."""
    nbits = 32 if family == 4 else 128
    X = E.X4 if family == 4 else E.X6
    probes = _by_filter("a")
    for p in range(nbits + 1):
        fid = E.a_filter_id(family, p)
        assert C.filters[fid] == [(E.ip(X), p)]
        ps = [q for q in probes[fid] if q.kind != "keepalive"]
        kinds = {q.kind: q for q in ps}
        same = [q for q in ps if len(q.dst) == len(X)]
        assert kinds["other family"].status == rx.PKT_FILTERED and len(kinds["other family"].dst) != len(X)
        assert kinds["base"].dst == X
        if 0 < p < nbits:
            assert kinds["base"].status == rx.PKT_OK
            assert kinds["just outside"].status == rx.PKT_FILTERED and kinds["just outside"].dst == E.flip(X, p - 1)
            assert kinds["first host bit"].status == rx.PKT_OK and kinds["first host bit"].dst == E.flip(X, p)
        elif p == nbits:
            assert {q.status for q in ps} == {rx.PKT_FILTERED}
        else:
            assert {q.status for q in same} == {rx.PKT_OK} and len(same) >= 3
        assert E.flip(X, 0) in {q.dst for q in ps} and E.flip(X, nbits - 1) in {q.dst for q in ps}
    assert len({q.dst for fid in probes for q in probes[fid]}) >= 33 + 129


def test_nested_and_sibling_filters_are_asked_every_kind():
    """(b): every filter with a covering prefix has a probe inside the outer prefix only (OK), inside both (OK) and
    inside neither (FILTERED); every other set one inside exactly one member (OK) and one outside all (FILTERED);
    the kinds are recomputed here from the prefixes, not taken from the builder's labels."""
    probes = _by_filter("b")
    names = {C.names[f] for f in C.b_kinds}
    for word in ("/8 and a /24", "/24 only", "/7 and /9", "/15, /16 and /17", "/23 and /25", "sibling /17s",
                 "/31 together with /32", "/63, /64 and /65", "/119, /120 and /121", "/127 together with /128",
                 "both families", "unmasked", "allowingAll()", "empty filter"):
        assert any(word in n for n in names), word
    for fid, kinds in C.b_kinds.items():
        pre = C.filters[fid]
        seen = Counter()
        for q in probes[fid]:
            if q.kind == "keepalive":
                continue
            inside = [_within(a, p, q.dst) for a, p in pre]
            fam = [k for k, (a, _) in enumerate(pre) if len(a.packed) == len(q.dst)]
            if kinds == E.NESTED_KINDS:
                n_in = sum(inside)
                kind = {0: "neither", 1: "outer only", len(pre): "both"}.get(n_in, "all but the innermost")
                assert inside[0] or n_in == 0  # the first prefix covers the others
                want = rx.PKT_OK if n_in else rx.PKT_FILTERED
            else:
                n_in = sum(inside[k] for k in fam)
                kind = "in one member" if n_in == 1 else "outside all"
                assert n_in <= 1
                full = n_in == 1 and pre[inside.index(True)][1] == len(q.dst) * 8  # a /32 or /128 matches nothing
                want = rx.PKT_OK if n_in and not full else rx.PKT_FILTERED
            assert kind == q.kind and q.status == want, (C.names[fid], q.kind, kind, E.ip(q.dst))
            seen[kind] += 1
        assert set(kinds) <= set(seen), (C.names[fid], seen)
    unmasked = next(f for f in C.b_kinds if "unmasked" in C.names[f])
    assert all(a.packed != E.ipaddress.ip_network((a, p), strict=False).network_address.packed
               for a, p in C.filters[unmasked])
    for special, want in ((E.GAP_ID, rx.PKT_FILTERED), (E.NEVER_SET, rx.PKT_FILTERED), (E.NO_FILTER, rx.PKT_OK)):
        assert special not in C.filters
        st = {q.status for q in probes[special] if q.kind != "keepalive"}
        assert st == {want} and {len(q.dst) for q in probes[special]} == {0, 4, 16}
    assert E.GAP_ID < max(C.filters) < E.NEVER_SET


def test_packet_edges():
    """(c): each packet under a v4 /0, a v6 /0 and no filter; the lengths on both sides of the 20- and 40-byte
    bounds; all 16 version nibbles at 40 B with 0x4F and 0x6F among the first bytes."""
    by = {}
    for p in C.probes:
        if p.part == "c":
            by.setdefault(p.pt, {})[p.fid] = p
    zero4 = next(f for f, n in C.names.items() if n.startswith("v4 /0 alone"))
    zero6 = next(f for f, n in C.names.items() if n.startswith("v6 /0 alone"))
    assert C.filters[zero4][0][1] == 0 and C.filters[zero6][0][1] == 0
    assert all(set(v) == {zero4, zero6, E.NO_FILTER} for v in by.values())
    st = {(pt[0] if pt else None, len(pt)): (v[zero4].status, v[zero6].status, v[E.NO_FILTER].status)
          for pt, v in by.items()}
    K, B, F, OK = rx.PKT_KEEPALIVE, rx.PKT_BADIP, rx.PKT_FILTERED, rx.PKT_OK
    assert st[(None, 0)] == (K, K, K)
    for n in (1, 19):
        assert st[(0x45, n)] == (B, B, B)
    for n in (20, 21):
        assert st[(0x45, n)] == (OK, F, OK)
    assert st[(0x60, 39)] == (B, B, B) and st[(0x60, 40)] == st[(0x60, 41)] == (F, OK, OK)
    firsts = sorted(pt[0] for pt in by if len(pt) == 40 and pt[0] not in (0x60,))
    assert {b >> 4 for b in firsts} == set(range(16)) and 0x4F in firsts and 0x6F in firsts
    assert len({b & 15 for b in firsts}) > 4
    for b in firsts:
        want = (OK, F, OK) if b >> 4 == 4 else (F, OK, OK) if b >> 4 == 6 else (B, B, B)
        assert st[(b, 40)] == want, hex(b)
    ends = [pt for pt in by if pt[-4:] == E.Y4 and len(pt) == 20] + [pt for pt in by if pt[-16:] == E.Y6 and len(pt) == 40]
    assert len(ends) == 2


def test_status_kinds_size_and_slot_map():
    count = Counter(p.status for p in C.probes)
    for st in (rx.PKT_OK, rx.PKT_FILTERED, rx.PKT_BADIP, rx.PKT_KEEPALIVE):
        assert count[st] >= 20, count
    assert set(count) == {rx.PKT_OK, rx.PKT_FILTERED, rx.PKT_BADIP, rx.PKT_KEEPALIVE}
    assert len(C.probes) < 2000
    assert len(C.filters) >= 162 + 14 + 2
    # (d): every filter has its own key slot, the map is not the identity and is set in two calls
    assert sorted(C.slot_ids, key=str) == sorted(list(C.filters) + [E.GAP_ID, E.NEVER_SET, E.NO_FILTER], key=str)
    assert all(C.slot_ids[C.slot_of[f]] == f for f in C.slot_of) and len(C.slot_ids) < E.KEY_SLOTS
    assert 0 < C.split < len(C.slot_ids) and sum(s == f for s, f in enumerate(C.slot_ids)) < 10
    assert {p.fid for p in C.probes} == set(C.slot_of)
    # half of the destinations sit in the last bytes of their packet
    ends = sum(len(p.pt) == E.min_len(p.dst) for p in C.probes if p.dst)
    assert 400 < ends < len(C.probes) - 400


def test_the_set_is_deterministic():
    E.cases.cache_clear()
    again = E.cases()
    assert again.probes == C.probes and again.slot_ids == C.slot_ids and again.filters == C.filters


def test_layout_keeps_a_sentinel_gap():
    lens = [len(p.pt) for p in C.probes]
    for unaligned in (False, True):
        off, size = E.layout(lens, 16, unaligned)
        off = off.astype(np.int64)
        end = off + np.asarray(lens) + 16
        assert off[0] >= E.GAP and (off[1:] - end[:-1] >= E.GAP).all() and size - end[-1] >= E.GAP
        assert len(set((off % 16).tolist())) == (16 if unaligned else 1)
