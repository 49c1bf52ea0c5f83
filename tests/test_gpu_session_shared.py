"""What wg_hs_install, wg_timers_start, wg_endpoints_start and the walkers of the receiver-index table share (csrc/wg_session.hip),
on the MI355X (pytest -m gpu): one table of malformed install batches refused alike by the three calls, one batch read alike by
the three, and one probe chain met by every kernel that walks the table. Everything is judged by hs_install_model, timers_model,
endpoints_model and session_end_model; contexts of 16 key slots."""
import ctypes

import numpy as np
import pytest

import endpoints_model as PM
import hs_install_model as IM
import session_end_model as EM
import timers_model as TM
from test_gpu_hs_initiate import GUARD, rig, t_u8, t_u32  # noqa: F401
from test_gpu_hs_install import STRIDE, _entries, _install, _lookup
from test_gpu_session_end import _compact, _same_table
from test_gpu_timers import RAM, T0, Pair

pytestmark = pytest.mark.gpu

SESS, EST = IM.SRC_SESSIONS, IM.SRC_ESTABLISHED
CALLS = ("wg_hs_install", "wg_timers_start", "wg_endpoints_start")


# ---- 1. the same refusals ----------------------------------------------------------------------------------------------------
def test_the_three_calls_refuse_a_malformed_batch_alike(rig):
    """The codes are those the calls returned before they shared their checks (recorded from that build)."""
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=16)
    try:
        eng.rx_sessions_reserve(8)
        eng.timers_reserve(2)
        eng.endpoints_reserve(2)
        n = 4
        d_ent = torch.full((n, 176), 0x7E, dtype=torch.uint8, device=dev)  # position 0x7E7E7E7E: BADSLOT, nothing is installed
        d_st = torch.full((n + 1,), GUARD, dtype=torch.int32, device=dev)
        d_sum, d_esum = (torch.full((4,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
        d_send, d_recv, d_n = t_u32(rig, [0, 2, 4, 6, 8]), t_u32(rig, [1, 3, 5, 7, 9]), t_u32(rig, [n, 0])
        d_now = torch.zeros(1, dtype=torch.int64, device=dev)
        d_src = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
        ent, cnt, snd, rcv, st = (t.data_ptr() for t in (d_ent, d_n, d_send, d_recv, d_st))
        batch = {"wg_hs_install": lambda: Lb.WgHsInstallBatch(ent, cnt, snd, rcv, None, st, d_sum.data_ptr(), n, n, 0, 16, SESS, 0),
                 "wg_timers_start": lambda: Lb.WgTimersStartBatch(ent, cnt, st, snd, rcv, d_now.data_ptr(), n, n, SESS, 0),
                 "wg_endpoints_start": lambda: Lb.WgEndpointsStartBatch(ent, cnt, st, snd, rcv, d_src.data_ptr(), d_esum.data_ptr(), n, n, n,
                                                                        SESS, 0, 0)}
        EINVAL, E2BIG = Lb.WG_EINVAL, Lb.WG_E2BIG
        rows = [({"source": 2}, EINVAL, CALLS),
                ({"entries": None}, EINVAL, CALLS),
                ({"entries": ent + 8}, EINVAL, CALLS),
                ({"n_entries": cnt + 2}, EINVAL, CALLS),
                ({"send_slot": None, "n_slots": 1}, EINVAL, CALLS),
                ({"recv_slot": rcv + 2}, EINVAL, CALLS),
                ({"n": (1 << 30) + 1}, E2BIG, CALLS),
                ({"inst_status": None}, EINVAL, CALLS[1:]),
                ({"inst_status": st + 2}, EINVAL, CALLS[1:])]
        for change, code, calls in rows:
            for name in calls:
                b = batch[name]()
                for field, value in change.items():
                    setattr(b, field, value)
                assert getattr(eng._lib, name)(eng.ctx, ctypes.byref(b), None) == code, (name, change)
        torch.cuda.synchronize()
        for t in (d_st, d_sum, d_esum):  # a refused call wrote nothing
            assert (t.cpu().numpy().view(np.uint32) == GUARD).all()
        for name in CALLS:  # ... and the batch they were made from is in order
            assert getattr(eng._lib, name)(eng.ctx, ctypes.byref(batch[name]()), None) == Lb.WG_OK, name
        torch.cuda.synchronize()
        assert d_st.cpu().numpy().view(np.uint32).tolist() == [IM.INST_BADSLOT] * n + [GUARD]
        assert d_sum.cpu().numpy().tolist() == [0, n, 0, 0] and d_esum.cpu().numpy().tolist() == [0, 0, 0, 0]
    finally:
        eng.close()


# ---- 2. the three readers agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [SESS, EST])
def test_install_and_both_starts_read_one_batch_alike(rig, source):
    """n = 7 entries of which the device count covers 6: a position past the slot lists, a pair that shares a slot, a peer past
    the peer tables, send slot == recv slot, and two sessions of one peer."""
    torch, dev = rig.torch, rig.dev
    K, P, n, cover, UNSET = 16, 3, 7, 6, 7
    send, recv = [0, 2, 4, 6, 8, 10], [1, 3, 5, 2, 9, 10]  # position 3 names slot 2 again, position 5 one slot twice
    pos = [0, 6, 1, 3, 4, 5, 2]
    peer = [0, 1, 0, 2, 9, 1, 2]
    dgram = [3, 1, 0, 2, 4, 5, 6]  # the handshake datagrams' batch indices
    li = [0xA100 + 5 * j for j in range(n)]
    ent = _entries(source, n, pos, li, 0xEB00 + source)
    ent["peer"], ent["index"] = peer, dgram
    srcs = [PM.src(bytes([10, 0, 0, j]), 4000 + j) for j in range(n)]
    p = Pair(rig, K, P, TM.Config())
    eng = p.eng
    try:
        eng.rx_sessions_reserve(8)
        eng.endpoints_reserve(P)
        eng.endpoint_slots_set(0, [UNSET] * K)
        d_ent = t_u8(rig, ent.tobytes()).reshape(n, STRIDE[source])
        d_n = t_u32(rig, [cover, 1 << 30])
        d_send, d_recv = t_u32(rig, send), t_u32(rig, recv)
        d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
        d_sum, d_esum = (torch.full((8,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
        d_src = t_u8(rig, b"".join(srcs)).reshape(n, 24)
        eng.hs_install(d_ent, d_n, d_send, d_recv, d_st[:n], d_sum[:4], 0, K, source)
        eng.timers_start(d_ent, d_n, d_st[:n], d_send, d_recv, p.at(T0), source)
        eng.endpoints_start(d_ent, d_n, d_st[:n], d_send, d_recv, d_src, d_esum[:4], source, learn_response=True)
        torch.cuda.synchronize()
        # the install against its model
        T, S = IM.Table(8), IM.State(K)
        want_ent = ent.copy()
        want_st, want_sum = IM.install(T, S, want_ent, cover, send, recv, slot_first=0, slot_count=K, source=source)
        assert want_st == [IM.INST_OK, IM.INST_BADSLOT, IM.INST_OK, IM.INST_DUPSLOT, IM.INST_OK, IM.INST_BADSLOT]
        got_st = d_st.cpu().numpy().view(np.uint32).tolist()
        assert got_st == want_st + [GUARD] * 3
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == [want_sum[k] for k in ("n_ok", "n_badslot", "n_dup", "n_full")] + [GUARD] * 4
        assert d_ent.cpu().numpy().tobytes() == want_ent.tobytes()
        _same_table(rig, eng, T, li)
        # both starts against theirs, from the statuses the device wrote
        p.m.start(T0, [(got_st[j], pos[j], peer[j], li[j]) for j in range(n)], send, recv, source, cover=cover, install=True)
        p.same(table=True)
        M = PM.Endpoints(K, P)
        M.slots_set(0, [UNSET] * K)
        want_esum = M.start([(got_st[j], pos[j], peer[j], dgram[j]) for j in range(n)], send, recv, source, srcs, flags=PM.LEARN_RESPONSE,
                            cover=cover)
        assert want_esum == [3, 1, 0, 1]
        assert d_esum.cpu().numpy().view(np.uint32).tolist() == want_esum + [GUARD] * 4
        slot_peer = eng.endpoint_slots_get(0, K).tolist()
        assert slot_peer == M.map and eng.endpoints_get(0, P).tobytes() == M.endpoints_image()
        assert M.ep[0] == PM.normalise(srcs[dgram[0]])  # of peer 0's two sessions the lower entry gives the endpoint
        # ... and the slots that either records are exactly those of the entries the install judged OK
        ok = [j for j in range(cover) if got_st[j] == IM.INST_OK]
        slots = sorted([send[pos[j]] for j in ok] + [recv[pos[j]] for j in ok])
        assert slots == [0, 1, 2, 3, 8, 9]
        assert np.flatnonzero(eng.timers_get(0, K)["state"] != TM.NONE).tolist() == slots
        assert [s for s in range(K) if slot_peer[s] != UNSET] == slots
    finally:
        p.close()


# ---- 3. one chain, every walker ------------------------------------------------------------------------------------------------
def test_every_walker_of_the_table_meets_one_chain(rig):
    """C = 16. Three indices of bucket 15 sit in buckets 15, 0, 1 (the host's build); the middle one is retired. Then, each step
    against the model:
    wg_rx_sessions_retire of the last; a RETIRE sweep that retires the first and leaves the last, whose index was installed again
    on other slots; an install of a fourth index of bucket 15; a compaction; wg_rx_plan's lookup of every index."""
    torch, dev = rig.torch, rig.dev
    K = 16
    a, b, c, d, never = [IM.index_in_bucket(15, 16, k) for k in range(5)]
    probe = [a, b, c, d, never]
    p = Pair(rig, K, 4, TM.Config(reject_after_messages=RAM))
    eng = p.eng
    try:
        eng.rx_sessions_reserve(4)
        T, S = IM.Table(4), IM.State(K)

        def install(indices, send, recv, seed):
            ent = _entries(EST, len(indices), list(range(len(indices))), indices, seed)
            want, _ = IM.install(T, S, ent.copy(), None, send, recv, slot_first=send[0], slot_count=2 * len(send), source=EST)
            assert _install(rig, eng, ent, None, send, recv, send[0], 2 * len(send), EST)[1][:len(indices)] == want == [IM.INST_OK] * len(indices)

        def same():
            _same_table(rig, eng, T, probe)
            p.same(table=True)

        eng.rx_sessions_set([a, b, c], [1, 3, 5])  # built on the host, in this order
        T.set([a, b, c], [1, 3, 5])
        p.start(T0, [(0, q, q, i) for q, i in enumerate([a, b, c])], [0, 2, 4], [1, 3, 5], EST)
        p.m.table = {a: 1, b: 3, c: 5}
        assert T.capacity == 16 and [T.ent[k][0] for k in (15, 0, 1)] == [a, b, c]
        eng.rx_sessions_retire(t_u32(rig, [b]))
        assert T.retire([b]) == 1 and T.chain(c) == 3
        del p.m.table[b]
        p.m.retired = 1
        same()
        # wg_rx_sessions_retire walks over the retired entry to the last
        d_nret = torch.full((2,), GUARD, dtype=torch.int32, device=dev)
        eng.rx_sessions_retire(t_u32(rig, [c, never]), d_nret[:1])
        assert T.retire([c, never]) == 1
        torch.cuda.synchronize()
        assert d_nret.cpu().numpy().view(np.uint32).tolist() == [1, GUARD]
        del p.m.table[c]
        p.m.retired = 2
        same()
        # c again, on slots (6, 7): bucket 2. Sessions (0, 1) and (4, 5) expire; the sweep retires a's entry and leaves c's
        install([c], [6], [7], 0xEC01)
        p.start(T0 + 1, [(0, 0, 2, c)], [6], [7], EST)
        p.m.table[c] = 7
        assert T.ent[2] == [c, 8]
        p.counters_set(0, [RAM, 0, 0, 0, RAM])
        out = p.sweep(T0 + 2, 4, 0, 0, retire=True)
        assert out["expired"].tolist() == [(0, 1, 0, a), (4, 5, 2, c)] and T.retire([a]) == 1
        assert p.m.table == {c: 7} and p.m.retired == 3
        same()
        # a fourth index of bucket 15 walks over three retired entries and a live one
        install([d], [8], [9], 0xEC02)
        p.m.table[d] = 9
        assert T.ent[3] == [d, 10] and T.count() == (2, 3)
        same()
        assert _compact(rig, eng) == EM.compact(T, 1) + [GUARD] * 4 == [2, 3, 1, 0] + [GUARD] * 4
        p.m.retired = 0
        same()
        assert _lookup(rig, eng, probe) == [None, None, 7, 9, None]
    finally:
        p.close()
