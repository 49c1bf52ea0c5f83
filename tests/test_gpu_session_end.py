"""The end of a session on the MI355X against tests/session_end_model.py (pytest -m gpu): wg_rx_sessions_compact,
wg_hs_install with WG_HS_INSTALL_COMPACT and wg_timers_sweep with WG_TIMERS_WIPE. The session table is read back through
wg_rx_plan on transport headers carrying every index, the key table through a seal of a known plaintext per slot
against the oracle; counts, statuses, summaries and the guard words behind them are compared exactly."""
import numpy as np
import pytest

import hs_install_model as IM
import session_end_model as EM
import timers_model as TM
from test_gpu_hs_initiate import GUARD, rig, t_u8, t_u32  # noqa: F401
from test_gpu_hs_install import STRIDE, _entries, _install, _key_table_is, _lookup, _tun_packet
from test_gpu_timers import RAM, T0, Pair
from wgtest import splitmix_bytes

pytestmark = pytest.mark.gpu

SESS, EST = IM.SRC_SESSIONS, IM.SRC_ESTABLISHED
ABSENT = [0, 0xFFFFFFFF, 77]


def _compact(rig, eng, min_retired=1, with_summary=True):
    """One wg_rx_sessions_compact; the summary as the device holds it, with the guard words behind it."""
    torch = rig.torch
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=rig.dev)
    eng.rx_sessions_compact(min_retired, d_sum[:4] if with_summary else None)
    torch.cuda.synchronize()
    return d_sum.cpu().numpy().view(np.uint32).tolist()


def _install_compact(rig, eng, ent, cover, send, recv, first, count, source):
    """_install with WG_HS_INSTALL_COMPACT: (statuses, summary), guards included."""
    torch, dev = rig.torch, rig.dev
    n = len(ent)
    d_ent = t_u8(rig, ent.tobytes()).reshape(n, STRIDE[source])
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    d_n = None if cover is None else t_u32(rig, [cover, 1 << 30, 1 << 30, 1 << 30])
    eng.hs_install(d_ent, d_n, t_u32(rig, send), t_u32(rig, recv), d_st[:n], d_sum[:4], first, count, source, compact=True)
    torch.cuda.synchronize()
    return d_st.cpu().numpy().view(np.uint32).tolist(), d_sum.cpu().numpy().view(np.uint32).tolist()


def _same_table(rig, eng, T, probe):
    assert _lookup(rig, eng, probe) == [T.lookup(i) for i in probe]
    assert eng.rx_sessions_count() == T.count()


# ---- 1. one wave, fewer buckets than a workgroup ---------------------------------------------------------------------------
def _wrapped_16(rig):
    """C = 16: three indices in bucket 15 and one in 14 (the chain runs 14, 15, 0, 1 across the table's end), the middle
    one of bucket 15 retired."""
    eng = rig.W.Engine(0, key_slots=32)
    pre = [IM.index_in_bucket(15, 16, k) for k in range(3)] + [IM.index_in_bucket(14, 16, 0)]
    eng.rx_sessions_reserve(4)
    eng.rx_sessions_set(pre, [0, 1, 2, 3])
    eng.rx_sessions_retire(t_u32(rig, [pre[1]]))
    T = IM.Table(4)
    T.set(pre, [0, 1, 2, 3])
    assert T.capacity == 16 and T.retire([pre[1]]) == 1 and T.chain(pre[2]) == 3
    return eng, T, pre


def test_compaction_of_a_chain_that_wraps_a_16_entry_table(rig):
    eng, T, pre = _wrapped_16(rig)
    try:
        assert eng.rx_sessions_count() == (3, 1)
        want = EM.compact(T, 1)
        assert _compact(rig, eng) == want + [GUARD] * 4 == [3, 1, 1, 0] + [GUARD] * 4
        assert eng.rx_sessions_count() == (3, 0)
        _same_table(rig, eng, T, pre + ABSENT)
        assert _lookup(rig, eng, pre) == [0, None, 2, 3]
    finally:
        eng.close()
    new = [0x9100 + k for k in range(5)]
    send, recv = [8 + 2 * k for k in range(5)], [9 + 2 * k for k in range(5)]
    for compact in (False, True):  # plain: 4 + 5 > 8, all FULL (the control); COMPACT: 3 + 5 fit
        eng, T, pre = _wrapped_16(rig)
        try:
            ent = _entries(SESS, 5, list(range(5)), new, 0xE400)
            S = IM.State(32)
            want_st, want_sum = EM.install(T, S, ent.copy(), None, send, recv, compact=compact, slot_first=8, slot_count=16, source=SESS)
            if compact:
                got_st, got_sum = _install_compact(rig, eng, ent, None, send, recv, 8, 16, SESS)
            else:
                _, got_st, got_sum = _install(rig, eng, ent, None, send, recv, 8, 16, SESS)
            assert want_st == [IM.INST_OK if compact else IM.INST_FULL] * 5
            assert got_st == want_st + [GUARD] * 4
            assert got_sum == [want_sum[k] for k in ("n_ok", "n_badslot", "n_dup", "n_full")] + [GUARD] * 4
            assert T.count() == ((8, 0) if compact else (3, 1))
            _same_table(rig, eng, T, pre + new + ABSENT)
            if compact:
                _key_table_is(rig, eng, 32, S.keys)
        finally:
            eng.close()


# ---- 2. thresholds and empties -----------------------------------------------------------------------------------------------
def test_thresholds_and_empty_tables(rig):
    W, Lb = rig.W, rig.W._lib
    eng, T, pre = _wrapped_16(rig)
    try:
        assert _compact(rig, eng, 2) == [3, 0, 0, 0] + [GUARD] * 4 == EM.compact(T, 2) + [GUARD] * 4  # one retired < 2: a no-op
        assert eng.rx_sessions_count() == (3, 1)
        _same_table(rig, eng, T, pre + ABSENT)
        assert _compact(rig, eng, 0) == [3, 1, 1, 0] + [GUARD] * 4 == EM.compact(T, 0) + [GUARD] * 4  # 0 acts as 1
        _same_table(rig, eng, T, pre + ABSENT)
        assert _compact(rig, eng, 0) == [3, 0, 0, 0] + [GUARD] * 4  # nothing retired any more
        assert _compact(rig, eng, 1, with_summary=False) == [GUARD] * 8  # the summary may be NULL
        eng.rx_sessions_retire(t_u32(rig, pre))  # every entry retired: the table becomes empty
        assert T.retire(pre) == 3 and eng.rx_sessions_count() == (0, 3)
        assert _compact(rig, eng) == [0, 3, 1, 0] + [GUARD] * 4 == EM.compact(T, 1) + [GUARD] * 4
        _same_table(rig, eng, T, pre + ABSENT)
        assert _lookup(rig, eng, pre) == [None] * 4 and eng.rx_sessions_count() == (0, 0)
        # argument errors
        d = rig.torch.zeros(8, dtype=rig.torch.int32, device=rig.dev)
        assert eng._lib.wg_rx_sessions_compact(None, 1, None, None) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_compact(eng.ctx, 1, d.data_ptr() + 4, None) == Lb.WG_EINVAL
    finally:
        eng.close()
    eng = W.Engine(0, key_slots=8)
    try:
        with pytest.raises(W.WgError) as e:  # never reserved
            eng.rx_sessions_compact()
        assert e.value.code == Lb.WG_EINVAL and "wg_rx_sessions_reserve" in str(e.value)
        eng.rx_sessions_set([5, 6], [1, 2])  # a table, but no reserve: still refused
        with pytest.raises(W.WgError) as e:
            eng.rx_sessions_compact()
        assert e.value.code == Lb.WG_EINVAL
        eng.rx_sessions_set([], [])
        eng.rx_sessions_reserve(4)  # an empty reserved table stays empty
        assert _compact(rig, eng, 0) == [0, 0, 0, 0] + [GUARD] * 4
        assert eng.rx_sessions_count() == (0, 0) and _lookup(rig, eng, ABSENT) == [None] * 3
    finally:
        eng.close()


# ---- 3. a table grown past its reserve -------------------------------------------------------------------------------------
def test_compaction_of_a_table_grown_past_its_reserve(rig):
    eng = rig.W.Engine(0, key_slots=8)
    try:
        eng.rx_sessions_reserve(1)  # C = 16
        idx = [IM.index_in_bucket(31, 32, 0), IM.index_in_bucket(31, 32, 1), IM.index_in_bucket(30, 32, 0), 0xA001, 0xA002]
        eng.rx_sessions_set(idx, [0, 1, 2, 3, 4])  # five entries: the capacity becomes 32, and the spare's with it
        T = IM.Table(1)
        T.set(idx, [0, 1, 2, 3, 4])
        assert T.capacity == 32
        eng.rx_sessions_retire(t_u32(rig, [idx[0], idx[3]]))
        assert T.retire([idx[0], idx[3]]) == 2
        assert _compact(rig, eng) == EM.compact(T, 1) + [GUARD] * 4 == [3, 2, 1, 0] + [GUARD] * 4
        _same_table(rig, eng, T, idx + ABSENT)
        # ... and a rebuild on the host after a compaction (the header names the second buffer) builds the first again
        eng.rx_sessions_set(idx[:2], [5, 6])
        T.set(idx[:2], [5, 6])
        _same_table(rig, eng, T, idx + ABSENT)
        eng.rx_sessions_retire(t_u32(rig, idx[:1]))
        T.retire(idx[:1])
        assert _compact(rig, eng) == EM.compact(T, 1) + [GUARD] * 4
        _same_table(rig, eng, T, idx + ABSENT)
    finally:
        eng.close()


def test_a_captured_compaction_follows_a_table_that_moved(rig):
    """Captured on the reserved 16-entry table, replayed after wg_rx_sessions_set built a table of 128 in new buffers: the
    launch holds neither the buffers' addresses nor the capacity."""
    torch = rig.torch
    eng = rig.W.Engine(0, key_slots=64)
    try:
        eng.rx_sessions_reserve(1)
        d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=rig.dev)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            eng.rx_sessions_compact(1, d_sum[:4])
        T = IM.Table(1)
        for n in (3, 30, 2):  # capacities 16, 128 (both buffers move), 16 again
            idx = [IM.index_in_bucket(T.reserved - 1, 128, k) for k in range(n // 2)] + [0xD000 + 5 * k for k in range(n - n // 2)]
            eng.rx_sessions_set(idx, list(range(n)))
            T.set(idx, list(range(n)))
            assert T.capacity == IM.capacity_for(n)
            for r in range(2):  # both parities on each table
                gone = idx[r::4]
                eng.rx_sessions_retire(t_u32(rig, gone))
                assert T.retire(gone) == len(gone)
                d_sum.fill_(GUARD)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                assert d_sum.cpu().numpy().view(np.uint32).tolist() == EM.compact(T, 1) + [GUARD] * 4
                _same_table(rig, eng, T, idx + ABSENT)
    finally:
        eng.close()


# ---- 4. chains across wave and table boundaries ----------------------------------------------------------------------------
def test_compaction_of_chains_longer_than_a_wave(rig):
    cap = 2048
    eng = rig.W.Engine(0, key_slots=512)
    try:
        eng.rx_sessions_reserve(512)
        end = [IM.index_in_bucket(cap - 1, cap, k) for k in range(96)]  # longer than a wave, and it wraps the table's end
        mid = [IM.index_in_bucket(60, cap, k) for k in range(96)]       # across buckets 63 / 64
        rest, k = [], 0
        while len(rest) < 320:
            i = int.from_bytes(splitmix_bytes(0xE500 + k, 4), "little")
            k += 1
            if i not in rest and i not in end and i not in mid and i not in ABSENT:
                rest.append(i)
        idx = end + mid + rest
        slots = [(5 * j + 3) % 512 for j in range(512)]
        eng.rx_sessions_set(idx, slots)
        T = IM.Table(512)
        T.set(idx, slots)
        assert T.capacity == cap and max(T.chain(i) for i in end) >= 96
        gone = end[::3] + mid[::3] + rest[:236]
        assert len(gone) == 300
        eng.rx_sessions_retire(t_u32(rig, gone))
        assert T.retire(gone) == 300
        assert _compact(rig, eng) == EM.compact(T, 1) + [GUARD] * 4 == [212, 300, 1, 0] + [GUARD] * 4
        absent = [int.from_bytes(splitmix_bytes(0xF0000 + j, 4), "little") for j in range(297)] + ABSENT
        assert not set(absent) & set(idx)
        _same_table(rig, eng, T, idx + absent)
        assert [T.lookup(i) for i in end[1:3]] == slots[1:3]
    finally:
        eng.close()


# ---- 5. the spare holds the table of two compactions ago -------------------------------------------------------------------
def test_three_compactions_in_a_row_never_revive_an_index(rig):
    eng = rig.W.Engine(0, key_slots=32)
    try:
        eng.rx_sessions_reserve(4)
        T, S = IM.Table(4), IM.State(32)
        x, y, z, w = [IM.index_in_bucket(15, 16, k) for k in range(4)]
        eng.rx_sessions_set([x, y, z, w], [0, 1, 2, 3])
        T.set([x, y, z, w], [0, 1, 2, 3])
        probe = [x, y, z, w, 0xB001, 0xB002] + ABSENT

        def step(retire, install=None):
            eng.rx_sessions_retire(t_u32(rig, retire))
            T.retire(retire)
            if install:
                index, s, r = install
                ent = _entries(EST, 1, [0], [index], 0xE700 + s)
                want, _ = IM.install(T, S, ent.copy(), None, [s], [r], slot_first=s, slot_count=2, source=EST)
                assert _install(rig, eng, ent, None, [s], [r], s, 2, EST)[1][:1] == want == [IM.INST_OK]
            assert _compact(rig, eng)[:4] == EM.compact(T, 1)
            _same_table(rig, eng, T, probe)

        step([w])                        # x is live in the buffer that now becomes the spare
        step([x], (0xB001, 8, 9))        # x retired; the second compaction builds in that buffer
        assert _lookup(rig, eng, [x]) == [None]
        step([y], (0xB002, 10, 11))      # the third builds in the buffer of the first
        assert _lookup(rig, eng, [x, y, z, w, 0xB001, 0xB002]) == [None, None, 2, None, 9, 11]
        assert eng.rx_sessions_count() == (3, 0)
    finally:
        eng.close()


# ---- 6. churn ----------------------------------------------------------------------------------------------------------------
def test_churn_at_capacity_eager_and_as_a_captured_graph(rig):
    """A node that holds the 64 sessions it reserved for and rekeys all of them every round. Without the compaction every
    round from the third on is FULL (tests/test_session_end.py shows it on the model)."""
    torch, dev, L = rig.torch, rig.dev, rig.W._lib
    n, K = 64, 256
    eng = rig.W.Engine(0, key_slots=K)
    try:
        eng.rx_sessions_reserve(n)
        T, S = IM.Table(n), IM.State(K)
        history = []

        def batch(r):
            li = [0x10000 * (r + 1) + 13 * k for k in range(n)]
            base = 2 * n * (r & 1)
            return li, [base + 2 * k for k in range(n)], [base + 2 * k + 1 for k in range(n)], _entries(SESS, n, list(range(n)), li, 0xE800 + r)

        def model(r, li, send, recv, ent):
            st, sm = EM.install(T, S, ent.copy(), None, send, recv, slot_first=0, slot_count=K, source=SESS)
            assert st == [IM.INST_OK] * n, r
            if history:
                assert T.retire(history[-1]) == n
            history.append(li)

        def check(r):
            assert T.count() == ((n, 0) if r == 0 else (n, n))
            _same_table(rig, eng, T, history[-1] + (history[-2] if r else []) + history[0] + ABSENT)

        for r in range(6):
            li, send, recv, ent = batch(r)
            got_st, got_sum = _install_compact(rig, eng, ent, None, send, recv, 0, K, SESS)
            assert got_sum == [n, 0, 0, 0] + [GUARD] * 4 and got_st == [0] * n + [GUARD] * 4, r
            if history:
                eng.rx_sessions_retire(t_u32(rig, history[-1]))
            model(r, li, send, recv, ent)
            check(r)
        _key_table_is(rig, eng, K, S.keys)
        # the same round as one graph: install(COMPACT) -> retire, the ring, the slots and the indices refreshed in place
        d_ent = torch.zeros((n, STRIDE[SESS]), dtype=torch.uint8, device=dev)
        d_send, d_recv, d_old = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        d_nret = torch.full((2,), GUARD, dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            eng.hs_install(d_ent, None, d_send, d_recv, d_st[:n], d_sum, 0, K, L.WG_HS_INSTALL_SESSIONS, compact=True)
            eng.rx_sessions_retire(d_old, d_nret[:1])
        for r in range(6, 11):  # five replays: both parities of the two buffers
            li, send, recv, ent = batch(r)
            d_ent.copy_(t_u8(rig, ent.tobytes()).reshape(n, STRIDE[SESS]))
            d_send.copy_(t_u32(rig, send))
            d_recv.copy_(t_u32(rig, recv))
            d_old.copy_(t_u32(rig, history[-1]))
            d_st.fill_(GUARD)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert d_sum.cpu().numpy().tolist() == [n, 0, 0, 0], r
            assert d_st.cpu().numpy().view(np.uint32).tolist() == [0] * n + [GUARD] * 2
            assert d_nret.cpu().numpy().view(np.uint32).tolist() == [n, GUARD]
            model(r, li, send, recv, ent)
            check(r)
        _key_table_is(rig, eng, K, S.keys)
    finally:
        eng.close()


# ---- 7. wipe -------------------------------------------------------------------------------------------------------------------
def _wipe_sweep(rig, p, S, t, caps):
    """One wg_timers_sweep(RETIRE | WIPE) on the context and on the model; every output compared, guards included."""
    bufs = p.sweep_buffers(*caps)
    p.eng.timers_sweep(p.at(t), bufs[0][:caps[0]], bufs[1][:caps[1]], bufs[2][:caps[2]], bufs[3][:8], wire_stride=32, out_size=1 << 30,
                       retire=True, wipe=True)
    want = EM.sweep(p.m, S, t, *caps, wire_stride=32, out_size=1 << 30, retire=True, wipe=True)
    rig.torch.cuda.synchronize()
    p.compare_sweep(bufs, want, caps)
    return want


def test_sweep_wipes_the_keys_of_the_sessions_it_retires(rig):
    torch, dev, W, L = rig.torch, rig.dev, rig.W, rig.W._lib
    K = 520
    Q = K // 2
    p = Pair(rig, K, 8, TM.Config(reject_after_messages=RAM))
    eng = p.eng
    try:
        eng.rx_sessions_reserve(Q)
        send, recv = [2 * q for q in range(Q)], [2 * q + 1 for q in range(Q)]
        send[127], recv[127] = 255, 254  # a send slot at the end of the first rank range, its recv slot below it
        li = [0x2000 + 7 * q for q in range(Q)]
        ent = _entries(EST, Q, list(range(Q)), li, 0xE900)
        d_rcv = torch.zeros(K, dtype=torch.int32, device=dev)
        eng.set_receivers(d_rcv)
        T, S = IM.Table(Q), IM.State(K)
        IM.install(T, S, ent.copy(), None, send, recv, slot_first=0, slot_count=K, source=EST)
        _, got_st, got_sum = _install(rig, eng, ent, None, send, recv, 0, K, EST, receivers=d_rcv)
        assert got_sum[:4] == [Q, 0, 0, 0] and len(set(S.keys.values())) == K  # every slot holds a key of its own
        sess = [0, 127, 128, Q - 1, 50, 150]  # send slots 0, 255, 256, K - 2 (the rank ranges' edges), 100, 300
        assert [send[q] for q in sess] == [0, 255, 256, K - 2, 100, 300]
        p.start(T0, [(0 if q in sess else 1, q, sess.index(q) if q in sess else 0, li[q]) for q in range(Q)], send, recv, EST)
        p.m.table = {li[q]: recv[q] for q in range(Q)}
        counters = [0] * K
        for q in sess[:4]:
            counters[send[q]] = RAM  # four sessions expire
        p.counters_set(0, counters)
        p.same(table=True)
        before = dict(S.keys)
        out = _wipe_sweep(rig, p, S, T0 + 1, (3, 0, 0))
        assert out["summary"][:2] == [4, 3] and out["expired"]["send_slot"].tolist() == [0, 255, 256]
        assert {s for s in range(K) if S.keys[s] != before[s]} == {0, 1, 254, 255, 256, 257}
        _key_table_is(rig, eng, K, S.keys)  # zeros in exactly those six, every other slot as it was
        p.same(table=True)
        assert _lookup(rig, eng, [li[q] for q in sess]) == [None, None, None, K - 1, 101, 301]
        out = _wipe_sweep(rig, p, S, T0 + 2, (3, 0, 0))  # the one that did not fit stayed due
        assert out["expired"]["send_slot"].tolist() == [K - 2] and S.keys[K - 2] == S.keys[K - 1] == bytes(32)
        _key_table_is(rig, eng, K, S.keys)
        p.same(table=True)
        assert _wipe_sweep(rig, p, S, T0 + 3, (3, 0, 0))["summary"][:2] == [0, 0]
        with pytest.raises(W.WgError) as e:  # the wipe goes with the retire only
            b = p.sweep_buffers(1, 0, 0)
            eng.timers_sweep(p.at(T0 + 4), b[0][:1], b[1][:0], b[2][:0], b[3][:8], retire=False, wipe=True)
        assert e.value.code == L.WG_EINVAL
        # nothing is sealed under a zero key: the gate refuses what is routed to a wiped send slot
        eng.routes_set([("10.1.0.0", 32, 0), ("10.1.0.1", 32, 255), ("10.1.0.2", 32, 100)])
        pkts = [_tun_packet(k, k, 48 + k) for k in range(3)]
        tun = np.zeros(128 * 3, np.uint8)
        for k, pk in enumerate(pkts):
            tun[128 * k:128 * k + len(pk)] = np.frombuffer(pk, np.uint8)
        d_tun = torch.from_numpy(tun).to(dev)
        desc = torch.zeros((3, 4), dtype=torch.int64, device=dev)
        st = torch.full((3,), GUARD, dtype=torch.int32, device=dev)
        msum = torch.zeros(2, dtype=torch.int32, device=dev)
        wire = torch.full((144 * 3,), 0x5A, dtype=torch.uint8, device=dev)
        eng.tx_plan(d_tun, torch.arange(0, 128 * 3, 128, dtype=torch.int64, device=dev), t_u32(rig, [len(pk) for pk in pkts]), desc, st,
                    144, wire.numel(), 100, route=True)
        eng.timers_mark(desc, st, p.at(T0 + 5), msum, tx=True, gate=True, slot_first=0, slot_count=K)
        eng.seal(desc, d_tun, wire, 100, frame=True)
        torch.cuda.synchronize()
        assert st.cpu().numpy().tolist() == [L.WG_PKT_NOSESSION, L.WG_PKT_NOSESSION, L.WG_PKT_OK]
        assert msum.cpu().numpy().tolist() == [1, 2]
        w = wire.cpu().numpy()
        assert (w[:288] == 0x5A).all() and w[288] == 4 and (w[288:288 + 32 + len(pkts[2])] != 0x5A).any()
    finally:
        p.close()


# ---- 8. an index installed again before the sweep --------------------------------------------------------------------------
def test_sweep_leaves_an_index_that_was_installed_again(rig):
    torch, dev = rig.torch, rig.dev
    K, index = 16, 0x4242
    p = Pair(rig, K, 2, TM.Config(reject_after_messages=RAM))
    eng = p.eng
    try:
        eng.rx_sessions_reserve(4)
        T, S = IM.Table(4), IM.State(K)
        keyed = _entries(EST, 8, list(range(8)), [0xC000 + q for q in range(8)], 0xEA00)  # every slot holds a key
        IM.install(T, S, keyed.copy(), None, list(range(0, K, 2)), list(range(1, K, 2)), slot_first=0, slot_count=K, source=EST)
        _install(rig, eng, keyed, None, list(range(0, K, 2)), list(range(1, K, 2)), 0, K, EST)
        eng.rx_sessions_retire(t_u32(rig, [0xC000 + q for q in range(8)]))
        T.retire([0xC000 + q for q in range(8)])
        assert _compact(rig, eng)[:4] == EM.compact(T, 1) == [0, 8, 1, 0]
        for seed, s, r in ((0xEA01, 2, 3), (0xEA02, 4, 5)):  # the session on (2, 3); later its index again, on (4, 5)
            if s == 4:
                eng.rx_sessions_retire(t_u32(rig, [index]))
                assert T.retire([index]) == 1
            ent = _entries(EST, 1, [0], [index], seed)
            want, _ = IM.install(T, S, ent.copy(), None, [s], [r], slot_first=s, slot_count=2, source=EST)
            assert _install(rig, eng, ent, None, [s], [r], s, 2, EST)[1][:1] == want == [IM.INST_OK]
            p.start(T0 + s, [(0, 0, s // 4, index)], [s], [r], EST)
        p.m.table, p.m.retired = {index: 5}, 1
        p.counters_set(2, [RAM])  # the old session expires
        p.same(table=True)
        before = dict(S.keys)
        out = _wipe_sweep(rig, p, S, T0 + 10, (4, 0, 0))
        assert out["expired"].tolist() == [(2, 3, 0, index)]
        assert {s for s in range(K) if S.keys[s] != before[s]} == {2, 3}
        _key_table_is(rig, eng, K, S.keys)  # the old session's two slots wiped, the new session's keys untouched
        assert _lookup(rig, eng, [index]) == [5] == [T.lookup(index)]  # ... and its table entry too
        assert eng.rx_sessions_count() == (1, 1) == T.count()
        p.same(table=True)
    finally:
        p.close()
