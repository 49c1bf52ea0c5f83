"""The end of a session on the device, without a GPU: tests/session_end_model.py's compaction against a plain dict, the
rekey churn that fills a table which only retires (the control) and never fills one that compacts, the min_retired
threshold, and the sweep that also zeroes the keys of the sessions it retires. The binding's constants and layout are
checked against include/wgaead.h."""
import ctypes
import re

import numpy as np
import pytest

import hs_install_model as IM
import session_end_model as EM
import timers_model as TM
from wgtest import ROOT, splitmix_bytes, wg


def _entries(n, local_index, seed, source=IM.SRC_SESSIONS):
    ent = np.frombuffer(splitmix_bytes(seed, IM.DTYPES[source].itemsize * n), IM.DTYPES[source]).copy()
    ent[IM.POSITION[source]] = list(range(n))
    ent["local_index"] = local_index
    return ent


def _crowded(cap, rng, n):
    """Distinct indices that crowd a few buckets, the table's last two among them: chains that wrap the table's end."""
    buckets = [cap - 1, cap - 2, int(rng.integers(0, cap)), int(rng.integers(0, cap))]
    out = set()
    while len(out) < n:
        out.add(IM.index_in_bucket(buckets[int(rng.integers(0, len(buckets)))], cap, int(rng.integers(0, 4 * n))))
    return sorted(out)


@pytest.mark.parametrize("max_sessions", [4, 16, 64])
def test_compaction_against_a_dict(max_sessions):
    rng = np.random.default_rng(0xE0 + max_sessions)
    for trial in range(40):
        T = IM.Table(max_sessions)
        cap = T.capacity
        n = int(rng.integers(0, cap // 2 + 1))
        indices = _crowded(cap, rng, n)
        live = {i: int(rng.integers(0, 1000)) for i in indices}
        for i, s in live.items():
            T._place(i, s + 1)
        gone = [i for i in indices if rng.integers(0, 3) == 0]
        assert T.retire(gone + gone[:1]) == len(gone)
        for i in gone:
            del live[i]
        if gone and rng.integers(0, 2):  # a retired index that lives again, behind its retired entry
            if T.used < cap // 2:
                T._place(gone[0], 777 + 1)
                live[gone[0]] = 777
        before = T.count()
        assert before == (len(live), T.used - len(live))
        min_retired = int(rng.integers(0, 4))
        did = before[1] >= max(min_retired, 1)
        assert EM.compact(T, min_retired) == ([len(live), before[1], 1, 0] if did else [len(live), 0, 0, 0])
        assert T.capacity == cap and T.live() == live
        assert T.count() == ((len(live), 0) if did else before)
        for i in indices + [0, 0xFFFFFFFF, 77]:
            assert T.lookup(i) == live.get(i)
        if did:  # no retired entry is left anywhere, and an index that was retired installs as new
            assert all(e[1] != IM.RETIRED for e in T.ent) and T.used == len(live)


def _churn(n, rounds, compact):
    """A node that holds the n sessions it reserved for and rekeys them all every round: each round installs n new
    indices on alternating slot pairs, then retires the previous round's. Returns per round (statuses, count)."""
    T, S = IM.Table(n), IM.State(4 * n)
    assert T.capacity == 4 * n
    out, prev = [], []
    for r in range(rounds):
        li = [0x10000 * (r + 1) + 13 * k for k in range(n)]
        base = 2 * n * (r & 1)
        send, recv = [base + 2 * k for k in range(n)], [base + 2 * k + 1 for k in range(n)]
        ent = _entries(n, li, 0xE100 + 64 * r + n)
        st, sm = EM.install(T, S, ent, None, send, recv, compact=compact, slot_first=0, slot_count=4 * n, source=IM.SRC_SESSIONS)
        assert sm["n_ok"] + sm["n_full"] == n
        if st == [IM.INST_OK] * n:
            T.retire(prev)
            prev = li
        out.append((st, T.count()))
    return out, T, prev


@pytest.mark.parametrize("n", [4, 64])
def test_churn_fills_a_table_that_only_retires(n):
    """The control: what the table did before there was a compaction."""
    out, T, _ = _churn(n, 6, compact=False)
    assert [st for st, _ in out[:2]] == [[IM.INST_OK] * n] * 2
    assert out[0][1] == (n, 0) and out[1][1] == (n, n) and T.used == T.capacity // 2
    for st, count in out[2:]:
        assert st == [IM.INST_FULL] * n and count == (n, n)


@pytest.mark.parametrize("n", [4, 64])
def test_churn_with_compaction_never_fills(n):
    out, T, last = _churn(n, 6, compact=True)
    for r, (st, count) in enumerate(out):
        assert st == [IM.INST_OK] * n, r
        assert count == ((n, 0) if r == 0 else (n, n))
    assert [T.lookup(i) is not None for i in last] == [True] * n and len(T.live()) == n


def test_install_compacts_only_when_the_ring_would_not_fit():
    T, S = IM.Table(4), IM.State(32)  # C = 16: at most 8 entries
    a = [0x51, 0x52, 0x53, 0x54]
    st, _ = EM.install(T, S, _entries(4, a, 0xE200), None, [0, 2, 4, 6], [1, 3, 5, 7], slot_first=0, slot_count=32, source=IM.SRC_SESSIONS)
    assert st == [0] * 4 and T.retire(a[:2]) == 2 and T.count() == (2, 2)
    # 4 + 3 <= 8: fits beside the retired entries, which stay
    st, _ = EM.install(T, S, _entries(3, [0x61, 0x62, 0x63], 0xE201), None, [8, 10, 12], [9, 11, 13], slot_first=8, slot_count=8,
                       source=IM.SRC_SESSIONS)
    assert st == [0] * 3 and T.count() == (5, 2)
    # 7 + 2 > 8: compacted to 5, then 5 + 2 fit. m counts the covered entries, whether or not they pass steps 1-3
    st, _ = EM.install(T, S, _entries(2, [0x71, 0x61], 0xE202), None, [16, 18], [17, 19], slot_first=16, slot_count=8, source=IM.SRC_SESSIONS)
    assert st == [IM.INST_OK, IM.INST_DUPINDEX] and T.count() == (6, 0)
    # nothing retired: no compaction can help, FULL means live + passing > C / 2
    st, _ = EM.install(T, S, _entries(3, [0x81, 0x82, 0x83], 0xE203), None, [20, 22, 24], [21, 23, 25], slot_first=20, slot_count=8,
                       source=IM.SRC_SESSIONS)
    assert st == [IM.INST_FULL] * 3 and T.count() == (6, 0)
    # n_entries below n: m is the covered count
    T.retire([0x71])
    st, _ = EM.install(T, S, _entries(4, [0x91, 0x92, 0x93, 0x94], 0xE204), 2, [20, 22, 24, 26], [21, 23, 25, 27], slot_first=20,
                       slot_count=8, source=IM.SRC_SESSIONS)
    assert st == [0, 0] and T.count() == (7, 1)  # 6 + 2 <= 8: fits, the retired entry stays


def test_min_retired_threshold():
    T = IM.Table(8)
    idx = [IM.index_in_bucket(31, 32, k) for k in range(6)]
    T.set(idx, list(range(6)))
    T.retire(idx[1:3])
    assert EM.compact(T, 3) == [4, 0, 0, 0] and T.count() == (4, 2)
    assert EM.compact(T, 2) == [4, 2, 1, 0] and T.count() == (4, 0)
    assert EM.compact(T, 0) == [4, 0, 0, 0] and EM.compact(T, 1) == [4, 0, 0, 0]  # nothing retired: min_retired 0 acts as 1
    T.retire(idx[:1])
    assert EM.compact(T, 0) == [3, 1, 1, 0] and [T.lookup(i) for i in idx] == [None, None, None, 3, 4, 5]
    E = IM.Table(4)
    assert EM.compact(E, 0) == [0, 0, 0, 0] and E.count() == (0, 0)
    E.set([5, 6], [1, 2])
    E.retire([5, 6])
    assert EM.compact(E, 1) == [0, 2, 1, 0] and E.count() == (0, 0) and E.lookup(5) is None and not any(e[1] for e in E.ent)


def test_sweep_with_wipe_zeroes_the_listed_sessions_only():
    K, n = 16, 4
    m = TM.Timers(K, n, TM.Config(reject_after_messages=100))
    S = IM.State(K)
    S.keys = {s: splitmix_bytes(0xE300 + s, 32) for s in range(K)}
    before = dict(S.keys)
    ents = [(0, k, k, 0x30 + k) for k in range(n)]
    send, recv = [0, 2, 4, 6], [1, 3, 5, 7]
    m.start(1000, ents, send, recv, TM.SRC_ESTABLISHED, install=True)
    m.send[0] = m.send[2] = m.send[6] = 100  # three sessions expire, two fit
    out = EM.sweep(m, S, 1001, 2, 0, 0, retire=True, wipe=True)
    assert out["summary"][:2] == [3, 2] and out["expired"]["send_slot"].tolist() == [0, 2]
    assert {s for s in range(K) if S.keys[s] != before[s]} == {0, 1, 2, 3} and all(S.keys[s] == bytes(32) for s in range(4))
    plain = TM.Timers(K, n, TM.Config(reject_after_messages=100))  # every output is the plain sweep's
    plain.start(1000, ents, send, recv, TM.SRC_ESTABLISHED, install=True)
    plain.send[0] = plain.send[2] = plain.send[6] = 100
    want = plain.sweep(1001, 2, 0, 0, retire=True)
    assert out["summary"] == want["summary"] and out["expired"].tobytes() == want["expired"].tobytes()
    assert m.slots_image().tobytes() == plain.slots_image().tobytes() and m.table == plain.table
    out = EM.sweep(m, S, 1002, 2, 0, 0, retire=True, wipe=True)  # the one that did not fit: still due, wiped now
    assert out["expired"]["send_slot"].tolist() == [6] and S.keys[6] == S.keys[7] == bytes(32) and S.keys[4] == before[4]
    out = EM.sweep(m, S, 1003, 2, 0, 0, retire=False)  # without the flags nothing is wiped
    assert S.keys[4] == before[4] and S.keys[5] == before[5]
    with pytest.raises(AssertionError):
        EM.sweep(m, S, 1004, 2, 0, 0, retire=False, wipe=True)


def test_binding_matches_the_header():
    L = wg()._lib
    src = open(f"{ROOT}/include/wgaead.h").read()
    assert f"#define WG_HS_INSTALL_COMPACT {L.WG_HS_INSTALL_COMPACT}u" in src and L.WG_HS_INSTALL_COMPACT == 4
    assert f"#define WG_TIMERS_WIPE {L.WG_TIMERS_WIPE}u" in src and L.WG_TIMERS_WIPE == 2
    assert re.search(r"typedef struct wg_rx_compact_summary \{[^}]*uint32_t live, dropped, compacted, _zero;", src)
    assert [f[0] for f in L.WgRxCompactSummary._fields_] == ["live", "dropped", "compacted", "_zero"]
    assert ctypes.sizeof(L.WgRxCompactSummary) == 16
    assert "wg_rx_sessions_compact" in {name for name, _, _ in L.SIGNATURES}
    assert hasattr(wg().lib(), "wg_rx_sessions_compact")
    import inspect
    E = wg().Engine
    assert inspect.signature(E.rx_sessions_compact).parameters["min_retired"].default == 1
    assert inspect.signature(E.hs_install).parameters["compact"].default is False
    assert inspect.signature(E.timers_sweep).parameters["wipe"].default is False
    assert inspect.signature(E.timers_tick).parameters["wipe"].default is False
