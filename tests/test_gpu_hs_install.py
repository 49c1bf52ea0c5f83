"""wg_hs_install, wg_rx_sessions_reserve / _retire / _count on the MI355X against tests/hs_install_model.py (pytest -m
gpu): statuses, summaries, the entries after the call and the guard words behind every output are compared exactly; the
key table is read back through a seal of a known plaintext per slot against the oracle, the session table through
wg_rx_plan on transport headers carrying every index. The closed loop completes handshakes between two contexts,
installs both sides on the device and carries tun packets from one to the other without a key reaching the host."""
import ctypes
import struct

import numpy as np
import pytest

import hs_install_model as IM
from test_gpu_hs_finish import _Loop
from test_gpu_hs_initiate import A_PRIV, B_PRIV, GUARD, rig, t_u8, t_u32  # noqa: F401
from wgtest import oracle, splitmix_bytes, splitmix_np

pytestmark = pytest.mark.gpu

SESS, EST = IM.SRC_SESSIONS, IM.SRC_ESTABLISHED
STRIDE = {SESS: 176, EST: 96}


def _entries(source, n, positions, local_index, seed):
    """n entries as wg_hs_respond / wg_hs_finish leave them: splitmix keys, every other byte defined too."""
    ent = np.frombuffer(splitmix_np(seed, STRIDE[source] * n).tobytes(), IM.DTYPES[source]).copy()
    ent[IM.POSITION[source]] = positions
    ent["local_index"] = local_index
    return ent


def _install(rig, eng, ent, cover, send, recv, first, count, source, receivers=None, wipe=True):
    """One wg_hs_install over guarded buffers: (entries, statuses, summary) as the device holds them, guards included.
    Every status word starts as GUARD, the summary too."""
    torch, dev = rig.torch, rig.dev
    n, stride = len(ent), STRIDE[source]
    d_ent = t_u8(rig, ent.tobytes() + b"\x7e" * stride).reshape(n + 1, stride)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    d_n = None if cover is None else t_u32(rig, [cover, 1 << 30, 1 << 30, 1 << 30])
    eng.hs_install(d_ent[:n], d_n, t_u32(rig, send), t_u32(rig, recv), d_st[:n], d_sum[:4], first, count, source,
                   receivers=receivers, wipe=wipe)
    torch.cuda.synchronize()
    return d_ent.cpu().numpy().tobytes(), d_st.cpu().numpy().view(np.uint32).tolist(), d_sum.cpu().numpy().view(np.uint32).tolist()


def _lookup(rig, eng, indices):
    """The session table as wg_rx_plan sees it: one empty transport packet per index; its key slot, or None."""
    torch, dev = rig.torch, rig.dev
    n = len(indices)
    wire = b"".join(struct.pack("<BxxxIQ", 4, int(i), 0) + bytes(16) for i in indices)
    d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_st, d_host = (torch.full((n,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
    d_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.rx_plan(t_u8(rig, wire), torch.arange(0, 32 * n, 32, dtype=torch.int64, device=dev),
                torch.full((n,), 32, dtype=torch.int32, device=dev), d_desc, d_st, d_host, d_sum, 0)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy().tolist()
    slot = (d_desc.cpu().numpy()[:, 3] >> 32).tolist()
    assert set(st) <= {0, 10}, st  # WG_PKT_OK or WG_PKT_NOSESSION
    return [int(s) if v == 0 else None for v, s in zip(st, slot)]


def _key_table_is(rig, eng, key_slots, keys):
    """Seals 32 known bytes under every slot (counter = the slot) and compares with the oracle under `keys`
    (slot -> 32 bytes; a slot never written holds zeros)."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    O = oracle()
    table = np.zeros(32 * key_slots, np.uint8)
    for s, k in keys.items():
        table[32 * s:32 * s + 32] = np.frombuffer(k, np.uint8)
    at = 48 * np.arange(key_slots, dtype=np.uint64)
    desc = W.pack_desc(np.zeros(key_slots, np.uint64), at, np.arange(key_slots, dtype=np.uint64), 32, np.arange(key_slots))
    pt = splitmix_np(0x7A00, 32)
    d_ct = torch.zeros(48 * key_slots, dtype=torch.uint8, device=dev)
    eng.seal(torch.from_numpy(W.desc_as_int64(desc)).to(dev), torch.from_numpy(pt).to(dev), d_ct, 32)
    torch.cuda.synchronize()
    ref = np.zeros(48 * key_slots, np.uint8)
    O.seal_batch(desc, pt, ref, table, threads=1)
    got = d_ct.cpu().numpy()
    bad = [s for s in range(key_slots) if got[48 * s:48 * s + 48].tobytes() != ref[48 * s:48 * s + 48].tobytes()]
    assert not bad, ("key slots differ from the model", bad[:8])


# ---- 1. against the model ---------------------------------------------------------------------------------------------
def _scenario(n, source):
    """The table before the call and the batch. Before: four live indices in the table's last two buckets (a chain that
    wraps its end), of which the middle one of the last bucket's chain is then retired. (Four: wg_rx_sessions_set builds
    into max(C, its own rule), and five entries would make a table of 32 of the 16 that n = 1 reserves.) The batch: entry 0
    re-installs the retired index; entries land in the last two buckets and, several, in bucket 5; from 63 entries on every
    refusal of steps 1-3 is seeded, and two entries stay behind n_entries."""
    max_sessions = n + 8 if n > 1 else 1
    cap = IM.capacity_for(max_sessions)
    key_slots = 2 * n + 24
    first, count = 4, 2 * n + 8
    pre = [IM.index_in_bucket(cap - 1, cap, k) for k in range(3)] + [IM.index_in_bucket(cap - 2, cap, 0)]
    pre_slots = [0, 1, 2, 3]
    retired = pre[1]
    li = []
    for j in range(n):
        kind = j % 6
        li.append(retired if j == 0 else IM.index_in_bucket(cap - 1, cap, 3 + j) if kind == 1 else
                  IM.index_in_bucket(cap - 2, cap, 2 + j) if kind == 2 else IM.index_in_bucket(5, cap, j) if kind == 3 else
                  int.from_bytes(splitmix_bytes(0x7B00 + 1000 * n + j, 4), "little"))
    pos = list(range(n))
    n_slots = n + 1
    send = [first + 2 * p for p in range(n_slots)]
    recv = [first + 2 * p + 1 for p in range(n_slots)]
    cover = None
    if n >= 63:
        pos[7] = n_slots                 # 1: the position is past the slot arrays
        send[9] = first - 1              # 1: a slot below the call's range
        recv[11] = send[11]              # 1: send slot == recv slot
        send[13] = key_slots             # 1: inside the range (which ends past the table), past the key table
        count = key_slots - first + 4
        pos[20] = pos[3]                 # 2: the same position, so both slots are a lower entry's
        recv[21] = send[4]               # 2: its recv slot is a lower entry's send slot
        send[22] = recv[9]               # (names a slot of entry 9, which failed step 1: no duplicate)
        li[30] = pre[0]                  # 3: live in the table at the call's start
        li[31] = li[6]                   # 3: a lower entry's
        li[32] = li[9]                   # (entry 9 failed step 1: no duplicate)
        li[33] = li[21]                  # (entry 21 failed step 2: no duplicate)
        li[34] = pre[2]                  # 3: live, behind the retired entry in its chain
        cover = n - 2
    return dict(max_sessions=max_sessions, cap=cap, key_slots=key_slots, first=first, count=count, pre=pre, pre_slots=pre_slots,
                retired=retired, ent=_entries(source, n, pos, li, 0x7C00 + n), send=send, recv=recv, cover=cover)


@pytest.mark.parametrize("source", [SESS, EST])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_install_against_the_model(rig, n, source):
    torch, dev = rig.torch, rig.dev
    sc = _scenario(n, source)
    K = sc["key_slots"]
    eng = rig.W.Engine(0, key_slots=K)
    try:
        old_keys = {s: splitmix_bytes(0x7D00 + s, 32) for s in range(K)}  # every slot holds a key before
        eng.set_keys(0, b"".join(old_keys[s] for s in range(K)))
        eng.rx_sessions_reserve(sc["max_sessions"])
        eng.rx_sessions_set(sc["pre"], sc["pre_slots"])
        d_nret = torch.full((2,), GUARD, dtype=torch.int32, device=dev)
        eng.rx_sessions_retire(t_u32(rig, [sc["retired"]]), d_nret[:1])
        T = IM.Table(sc["max_sessions"])
        assert T.capacity == sc["cap"]
        T.set(sc["pre"], sc["pre_slots"])
        assert T.retire([sc["retired"]]) == 1 and T.chain(sc["pre"][2]) == 3  # the retired entry is inside a chain
        S = IM.State(K)
        S.keys = dict(old_keys)
        d_recv = torch.full((K + 2,), GUARD, dtype=torch.int32, device=dev)
        want_ent = sc["ent"].copy()
        want_st, want_sum = IM.install(T, S, want_ent, sc["cover"], sc["send"], sc["recv"], slot_first=sc["first"],
                                       slot_count=sc["count"], source=source)
        got_ent, got_st, got_sum = _install(rig, eng, sc["ent"], sc["cover"], sc["send"], sc["recv"], sc["first"], sc["count"],
                                            source, receivers=d_recv[:K])
        assert d_nret.cpu().numpy().view(np.uint32).tolist() == [1, GUARD]
        cover = len(want_st)
        assert got_st == want_st + [GUARD] * (n + 4 - cover), [(j, a, b) for j, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:8]
        assert got_sum == [want_sum["n_ok"], want_sum["n_badslot"], want_sum["n_dup"], want_sum["n_full"]] + [GUARD] * 4
        assert got_ent == want_ent.tobytes() + b"\x7e" * STRIDE[source]  # installed keys wiped, every other byte as it was
        assert want_st[0] == IM.INST_OK  # the retired index is installed again
        if n >= 63:
            assert set(want_st) == {IM.INST_OK, IM.INST_BADSLOT, IM.INST_DUPSLOT, IM.INST_DUPINDEX}
            assert [want_st[j] for j in (7, 9, 11, 13, 20, 21, 22, 30, 31, 32, 33, 34)] == [1, 1, 1, 1, 2, 2, 0, 3, 3, 0, 0, 3]
            assert max(T.chain(i) for i in T.live()) >= 4
        _key_table_is(rig, eng, K, S.keys)
        probe = sc["pre"] + [int(x) for x in sc["ent"]["local_index"]] + [0, 0xFFFFFFFF, 0x12345678]
        assert _lookup(rig, eng, probe) == [T.lookup(i) for i in probe]
        assert eng.rx_sessions_count() == T.count()
        recv_tab = d_recv.cpu().numpy().view(np.uint32).tolist()
        assert recv_tab == [S.receivers.get(s, GUARD) for s in range(K)] + [GUARD] * 2
    finally:
        eng.close()


@pytest.mark.parametrize("source", [SESS, EST])
def test_chains_in_the_last_buckets_of_a_16_entry_table(rig, source):
    """C = 16: two live indices in bucket 15 and one in 14, the first of bucket 15 retired; the call installs the retired
    index again, two more of bucket 15 and one of bucket 14: chains run 14, 15, 0, 1, ... across the table's end."""
    eng = rig.W.Engine(0, key_slots=16)
    try:
        eng.rx_sessions_reserve(4)
        pre = [IM.index_in_bucket(15, 16, 0), IM.index_in_bucket(15, 16, 1), IM.index_in_bucket(14, 16, 0)]
        eng.rx_sessions_set(pre, [1, 2, 3])
        eng.rx_sessions_retire(t_u32(rig, [pre[0]]))
        T = IM.Table(4)
        T.set(pre, [1, 2, 3])
        T.retire([pre[0]])
        li = [pre[0], IM.index_in_bucket(15, 16, 2), IM.index_in_bucket(14, 16, 1), IM.index_in_bucket(15, 16, 3)]
        ent = _entries(source, 4, [3, 2, 1, 0], li, 0x7E00)
        send, recv = [4, 6, 8, 10], [5, 7, 9, 11]
        want_ent = ent.copy()
        S = IM.State(16)
        want_st, want_sum = IM.install(T, S, want_ent, None, send, recv, slot_first=4, slot_count=8, source=source)
        got_ent, got_st, got_sum = _install(rig, eng, ent, None, send, recv, 4, 8, source)
        assert want_st == [0, 0, 0, 0] and got_st[:4] == want_st and got_sum[:4] == [4, 0, 0, 0]
        assert got_ent[:len(want_ent.tobytes())] == want_ent.tobytes()
        assert T.used == 7 and max(T.chain(i) for i in T.live()) >= 5
        assert _lookup(rig, eng, pre + li + [77]) == [T.lookup(i) for i in pre + li + [77]]
        assert eng.rx_sessions_count() == (6, 1) == T.count()
        _key_table_is(rig, eng, 16, S.keys)
    finally:
        eng.close()


# ---- 2. the closed loop -------------------------------------------------------------------------------------------------
class _InstallLoop(_Loop):
    """_Loop with key tables large enough for every handshake's two slots."""

    def __init__(self, rig, n, key_slots):
        super().__init__(rig, n)
        self.close()
        self.A, self.B = rig.W.Engine(0, key_slots=key_slots), rig.W.Engine(0, key_slots=key_slots)
        a_pub, b_pub = self.A.hs_static_set(A_PRIV), self.B.hs_static_set(B_PRIV[0])
        self.A.hs_peers_set([b_pub])
        self.B.hs_peers_set([a_pub])


def _tun_packet(p, k, length):
    """An IPv4 packet to 10.1.(p >> 8).(p & 255), the address routed to handshake p's send slot."""
    b = bytearray(splitmix_bytes(0x7F00 + 4096 * k + p, length))
    b[0] = 0x45
    b[16:20] = bytes([10, 1, p >> 8, p & 255])
    return bytes(b)


@pytest.mark.parametrize("n", [65, 257])
def test_handshakes_installed_on_both_sides_carry_tun_packets(rig, n):
    torch, dev, L = rig.torch, rig.dev, rig.W._lib
    K = 2 * n + 2
    lp = _InstallLoop(rig, n, K)
    A, B = lp.A, lp.B
    try:
        A.set_keys(0, splitmix_bytes(0x8000, 64))  # the host's copies of slots 0 and 1 hold a key until the install
        B.replay_enable(128)
        A.rx_sessions_reserve(n)
        B.rx_sessions_reserve(n)
        lp.initiate_and_respond(n)
        lp.check_and_finish()
        torch.cuda.synchronize()
        est, sess = lp.agreed()  # (read before the installs wipe the keys: the test's own knowledge of them)
        send = t_u32(rig, [2 * p for p in range(n)])
        recv = t_u32(rig, [2 * p + 1 for p in range(n)])
        a_recv, b_recv = (torch.zeros(K, dtype=torch.int32, device=dev) for _ in range(2))
        A.set_receivers(a_recv)
        a_st, b_st = (torch.full((n,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
        a_sum, b_sum = (torch.full((4,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
        A.hs_install(lp.f_est, lp.f_sum, send, recv, a_st, a_sum, 0, 2 * n, L.WG_HS_INSTALL_ESTABLISHED, receivers=a_recv)
        B.hs_install(lp.b_sess, lp.b_rsum, send, recv, b_st, b_sum, 0, 2 * n, L.WG_HS_INSTALL_SESSIONS, receivers=b_recv)
        # A: tun ring -> UDP ring. Two packets per peer, the second round in reverse peer order.
        order = list(range(n)) + list(range(n - 1, -1, -1))
        pkts = [_tun_packet(p, k, 40 + (7 * k + p) % 60) for k, p in enumerate(order)]
        m, max_len, stride = len(pkts), 100, 144
        A.routes_set([(f"10.1.{p >> 8}.{p & 255}", 32, 2 * p) for p in range(n)])
        tun = np.zeros(128 * m, np.uint8)
        for k, pk in enumerate(pkts):
            tun[128 * k:128 * k + len(pk)] = np.frombuffer(pk, np.uint8)
        d_tun = torch.from_numpy(tun).to(dev)
        t_off = torch.arange(0, 128 * m, 128, dtype=torch.int64, device=dev)
        t_len = t_u32(rig, [len(pk) for pk in pkts])
        t_desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        t_st = torch.full((m,), GUARD, dtype=torch.int32, device=dev)
        d_wire = torch.zeros(stride * m, dtype=torch.uint8, device=dev)
        A.tx_seal(d_tun, t_off, t_len, t_desc, t_st, d_wire, stride, max_len, route=True)
        torch.cuda.synchronize()
        assert a_sum.cpu().numpy().tolist() == [n, 0, 0, 0] == b_sum.cpu().numpy().tolist()
        assert not a_st.cpu().numpy().any() and not b_st.cpu().numpy().any() and not t_st.cpu().numpy().any()
        assert (a_recv.cpu().numpy().view(np.uint32)[0:2 * n:2] == est["remote_index"]).all()
        assert (b_recv.cpu().numpy().view(np.uint32)[0:2 * n:2] == sess["remote_index"]).all()
        forged = 3
        d_wire[stride * forged + 16 + 5] ^= 1  # one flipped ciphertext byte
        # B: UDP ring -> tun list
        w_off = torch.arange(0, stride * m, stride, dtype=torch.int64, device=dev)
        w_len = t_u32(rig, [len(pk) + 32 for pk in pkts])
        r_desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        r_st, r_host, o_st, f_st, r_idx = (torch.full((m,), GUARD, dtype=torch.int32, device=dev) for _ in range(5))
        r_sum, r_del = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        r_items = torch.zeros((m, 2), dtype=torch.int64, device=dev)
        d_pt = torch.zeros(112 * m, dtype=torch.uint8, device=dev)
        B.rx_plan(d_wire, w_off, w_len, r_desc, r_st, r_host, r_sum, max_len, packed=True, pt_size=d_pt.numel())
        B.open(r_desc, d_wire, d_pt, o_st, max_len)
        B.rx_check(r_desc, d_pt, o_st, L.WG_RX_REPLAY | L.WG_RX_FILTER)
        B.rx_deliver(r_desc, r_st, o_st, f_st, r_items, r_del, index_out=r_idx)
        torch.cuda.synchronize()
        assert not r_st.cpu().numpy().any()  # every receiver index found its session
        want_f = [L.WG_PKT_BADTAG if k == forged else L.WG_PKT_OK for k in range(m)]
        assert f_st.cpu().numpy().tolist() == want_f
        keep = [k for k in range(m) if k != forged]
        assert r_del.cpu().numpy()[1:2].view(np.uint32).tolist() == [m - 1, 0] and r_idx.cpu().numpy()[:m - 1].tolist() == keep
        items = np.ascontiguousarray(r_items.cpu().numpy()[:m - 1]).view(np.dtype([("off", "<u8"), ("len", "<u4"), ("slot", "<u4")])).reshape(-1)
        pt = d_pt.cpu().numpy()
        for it, k in zip(items, keep):
            assert pt[int(it["off"]):int(it["off"]) + int(it["len"])].tobytes() == pkts[k] and int(it["slot"]) == 2 * order[k] + 1, k
        # the second packet of a peer carries counter 1, whatever its place in the ring
        ctr = r_desc.cpu().numpy()[:, 2]
        assert ctr[:n].tolist() == [0] * n and ctr[n:].tolist() == [1] * n
        # no key is left in the handshake buffers, and the host paths refuse the slots
        for buf, dt in ((lp.f_est, IM.HS_ESTABLISHED), (lp.b_sess, IM.HS_SESSION)):
            h = buf.cpu().numpy().reshape(-1).view(dt)
            assert not h["send_key"].any() and not h["recv_key"].any() and h["local_index"].all()
        for eng in (A, B):
            assert eng.rx_sessions_count() == (n, 0)
            with pytest.raises(rig.W.WgError) as e:
                eng.seal1(0, 0, b"x")
            assert e.value.code == L.WG_ENOKEY
        with pytest.raises(rig.W.WgError) as e:
            A.open1(1, 0, bytes(17))
        assert e.value.code == L.WG_ENOKEY
    finally:
        lp.close()


# ---- 3. state reset ------------------------------------------------------------------------------------------------------
def test_install_restarts_send_counters_and_replay_windows(rig):
    torch, dev, W, L = rig.torch, rig.dev, rig.W, rig.W._lib
    eng = W.Engine(0, key_slots=8)
    try:
        eng.replay_enable(128)
        eng.rx_sessions_reserve(4)
        eng.set_keys(2, splitmix_bytes(0x8100, 64))
        eng.tx_peers_set([2, 3])
        tun = torch.zeros(256, dtype=torch.uint8, device=dev)
        t_desc = torch.zeros((6, 4), dtype=torch.int64, device=dev)
        t_st = torch.zeros(6, dtype=torch.int32, device=dev)
        eng.tx_plan(tun, torch.arange(0, 96, 32, dtype=torch.int64, device=dev), torch.full((3,), 20, dtype=torch.int32, device=dev),
                    t_desc, t_st, 64, 6 * 64, 32)

        def check(counters):
            k = len(counters)
            desc = W.pack_desc(np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.array(counters, np.uint64), 4, 3)
            st = torch.zeros(k, dtype=torch.int32, device=dev)
            eng.rx_check(torch.from_numpy(W.desc_as_int64(desc)).to(dev), tun, st, L.WG_RX_REPLAY)
            torch.cuda.synchronize()
            return st.cpu().numpy().tolist()

        assert check([0, 1, 2, 70]) == [0, 0, 0, 0] and check([0]) == [L.WG_PKT_REPLAY]
        assert eng.tx_counters_get(2, 2).tolist() == [3, 3]
        top, bits = eng.replay_state(3, 128)
        assert top == 71 and bits.any()
        ent = _entries(SESS, 1, [0], [0xABCD], 0x8200)
        got_ent, got_st, got_sum = _install(rig, eng, ent, None, [2], [3], 2, 2, SESS)
        assert got_st[0] == IM.INST_OK and got_sum[:4] == [1, 0, 0, 0]
        assert eng.tx_counters_get(2, 2).tolist() == [0, 0]
        for slot in (2, 3):
            top, bits = eng.replay_state(slot, 128)
            assert top == 0 and not bits.any()
        assert check([0]) == [0] and check([0]) == [L.WG_PKT_REPLAY]  # counter 0 once more, once
        _key_table_is(rig, eng, 8, {2: ent[0]["send_key"].tobytes(), 3: ent[0]["recv_key"].tobytes()})
    finally:
        eng.close()


# ---- 4. FULL -------------------------------------------------------------------------------------------------------------
def test_full_is_all_or_nothing(rig):
    eng = rig.W.Engine(0, key_slots=32)
    try:
        eng.rx_sessions_reserve(4)  # C = 16: at most 8 entries, live or retired
        T, S = IM.Table(4), IM.State(32)
        live = [int.from_bytes(splitmix_bytes(0x8300 + k, 4), "little") for k in range(7)]
        new = [0x51, 0x52, 0x53, 0x54]

        def both(ent, send, recv, first, count):
            """The call on the device and on the model; returns the statuses after checking everything else."""
            want_ent = ent.copy()
            want_st, want_sum = IM.install(T, S, want_ent, None, send, recv, slot_first=first, slot_count=count, source=EST)
            got_ent, got_st, got_sum = _install(rig, eng, ent, None, send, recv, first, count, EST)
            assert got_st[:len(ent)] == want_st and got_sum[:4] == [want_sum[k] for k in ("n_ok", "n_badslot", "n_dup", "n_full")]
            assert got_ent[:96 * len(ent)] == want_ent.tobytes()
            assert eng.rx_sessions_count() == T.count()
            assert _lookup(rig, eng, live + new) == [T.lookup(i) for i in live + new]
            return want_st

        # seven live entries, installed (wg_rx_sessions_set of seven would build a table of 32)
        assert both(_entries(EST, 7, list(range(7)), live, 0x83F0), list(range(8, 22, 2)), list(range(9, 23, 2)), 8, 14) == [0] * 7
        assert T.capacity == 16 and T.count() == (7, 0)
        ent = _entries(EST, 2, [0, 1], new[:2], 0x8400)
        assert both(ent, [24, 26], [25, 27], 24, 8) == [IM.INST_FULL] * 2  # 7 + 2 > 8: neither, and nothing changes
        assert T.count() == (7, 0) and not set(S.keys) & {24, 25, 26, 27}
        _key_table_is(rig, eng, 32, S.keys)
        assert both(ent[:1], [24], [25], 24, 8) == [IM.INST_OK] and T.count() == (8, 0)  # 7 + 1 fits
        # retiring makes no room ...
        d_n = rig.torch.zeros(1, dtype=rig.torch.int32, device=rig.dev)
        eng.rx_sessions_retire(t_u32(rig, live[:2]), d_n)
        assert T.retire(live[:2]) == 2 and eng.rx_sessions_count() == (6, 2) and d_n.cpu().numpy().tolist() == [2]
        ent3 = _entries(EST, 1, [0], new[2:3], 0x8401)
        assert both(ent3, [28], [29], 28, 2) == [IM.INST_FULL]
        # ... a rebuild on the host does
        keep, keep_slots = live[2:5] + new[:1], [13, 15, 17, 25]
        eng.rx_sessions_set(keep, keep_slots)
        T.set(keep, keep_slots)
        assert T.capacity == 16 and eng.rx_sessions_count() == (4, 0)
        assert both(ent3, [28], [29], 28, 2) == [IM.INST_OK] and T.count() == (5, 0)
        _key_table_is(rig, eng, 32, S.keys)
        # more new indices than the table has buckets: every one FULL, whichever were placed first, and equal ones DUPINDEX
        li = [0x9000 + (j % 20) for j in range(24)]
        ent24 = _entries(SESS, 24, list(range(24)), li, 0x8402)
        eng2 = rig.W.Engine(0, key_slots=64)
        try:
            eng2.rx_sessions_reserve(4)
            _, st, sm = _install(rig, eng2, ent24, None, list(range(0, 48, 2)), list(range(1, 48, 2)), 0, 64, SESS)
            assert st[:24] == [IM.INST_FULL] * 20 + [IM.INST_DUPINDEX] * 4 and sm[:4] == [0, 0, 4, 20]
            assert eng2.rx_sessions_count() == (0, 0) and _lookup(rig, eng2, li) == [None] * 24
        finally:
            eng2.close()
    finally:
        eng.close()


# ---- 5. retire -----------------------------------------------------------------------------------------------------------
def test_retire(rig):
    torch, dev = rig.torch, rig.dev
    eng = rig.W.Engine(0, key_slots=8)
    try:
        d_n = torch.full((2,), GUARD, dtype=torch.int32, device=dev)
        eng.rx_sessions_retire(t_u32(rig, [1, 2]), d_n[:1])  # no table yet: nothing to retire
        assert eng.rx_sessions_count() == (0, 0) and d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD]
        eng.rx_sessions_reserve(4)
        chain = [IM.index_in_bucket(15, 16, k) for k in range(3)]  # buckets 15, 0, 1
        eng.rx_sessions_set(chain + [7], [1, 2, 3, 4])
        eng.rx_sessions_retire(t_u32(rig, [chain[1], 0xDEAD, chain[1], chain[1]]), d_n[:1])
        assert d_n.cpu().numpy().view(np.uint32).tolist() == [1, GUARD]  # equal indices count once, an unknown one not at all
        assert _lookup(rig, eng, chain + [7, 0xDEAD]) == [1, None, 3, 4, None]  # the index behind it is still found
        assert eng.rx_sessions_count() == (3, 1)
        eng.rx_sessions_retire(t_u32(rig, [chain[1], 7]), None)  # retired already: not again; n_retired may be NULL
        assert eng.rx_sessions_count() == (2, 2)
        eng.rx_sessions_retire(t_u32(rig, []), d_n[:1])  # n = 0 writes the count
        assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD]
        eng.rx_sessions_reserve(4)  # a rebuild drops the retired entries and keeps the live ones
        assert eng.rx_sessions_count() == (2, 0) and _lookup(rig, eng, chain + [7]) == [1, None, 3, None]
    finally:
        eng.close()


# ---- 6. graph ------------------------------------------------------------------------------------------------------------
def test_captured_respond_and_install_replays(rig):
    """Reserve, capture respond -> install once, replay three times with ephemerals, local indices and the two slot
    arrays refreshed in place; a replay without a refresh answers nothing and installs nothing. A capturing install on
    a context that has not reserved: WG_EINVAL."""
    torch, dev, W, L = rig.torch, rig.dev, rig.W, rig.W._lib
    n = 70
    K = 6 * n
    lp = _InstallLoop(rig, n, K)
    B = lp.B
    try:
        B.hs_reserve(n)
        B.rx_sessions_reserve(3 * n)
        lp.initiate_and_respond(1)  # eager once: B's inits are in place
        send, recv = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        i_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
        i_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                lp.A.hs_install(lp.b_sess, lp.b_rsum, send, recv, i_st[:n], i_sum, 0, K, L.WG_HS_INSTALL_SESSIONS)
            B.hs_respond(lp.b_init, lp.b_osum, lp.b_eph, lp.b_li, lp.b_rst, lp.b_sess, lp.b_rsum)
            B.hs_install(lp.b_sess, lp.b_rsum, send, recv, i_st[:n], i_sum, 0, K, L.WG_HS_INSTALL_SESSIONS)
        assert e.value.code == L.WG_EINVAL and "wg_rx_sessions_reserve" in str(e.value)
        from hs_respond_model import HS_SESSION
        all_li, all_slot = [], []
        for r in range(3):
            eph = splitmix_np(0x8500 + r, 32 * n)
            li = [(0x40000000 * (r + 1) + 13 * k) & 0xFFFFFFFF for k in range(n)]
            s_slots, r_slots = [2 * n * r + 2 * k for k in range(n)], [2 * n * r + 2 * k + 1 for k in range(n)]
            lp.b_eph.copy_(t_u8(rig, eph.tobytes()))
            lp.b_li.copy_(t_u32(rig, li))
            send.copy_(t_u32(rig, s_slots))
            recv.copy_(t_u32(rig, r_slots))
            i_st.fill_(GUARD)
            # what the sessions' keys will be: respond alone, eagerly, on a copy of the ephemerals
            eph2 = t_u8(rig, eph.tobytes())
            sess2 = torch.zeros((n, 176), dtype=torch.uint8, device=dev)
            st2, sum2 = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
            B.hs_respond(lp.b_init, lp.b_osum, eph2, lp.b_li, st2, sess2, sum2)
            torch.cuda.synchronize()
            want = sess2.cpu().numpy().reshape(-1).view(HS_SESSION)
            g.replay()
            torch.cuda.synchronize()
            assert lp.b_rsum.cpu().numpy().tolist() == [n, 0, 0, 0] and i_sum.cpu().numpy().tolist() == [n, 0, 0, 0]
            assert i_st.cpu().numpy().view(np.uint32).tolist() == [0] * n + [GUARD] * 2
            got = lp.b_sess.cpu().numpy().reshape(-1).view(HS_SESSION)
            assert got["response"].tobytes() == want["response"].tobytes() and not got["send_key"].any() and not got["recv_key"].any()
            all_li += li
            all_slot += r_slots
            assert B.rx_sessions_count() == (n * (r + 1), 0)
            assert _lookup(rig, B, all_li) == all_slot
            keys = {}
            for k in range(n):
                keys[s_slots[k]], keys[r_slots[k]] = want[k]["send_key"].tobytes(), want[k]["recv_key"].tobytes()
            if r == 0:
                _key_table_is(rig, B, K, keys)
            g.replay()  # no refresh: the ephemerals are consumed, nothing is answered, nothing installed
            torch.cuda.synchronize()
            assert lp.b_rsum.cpu().numpy().tolist() == [0, 0, n, 0] and i_sum.cpu().numpy().tolist() == [0, 0, 0, 0]
            assert B.rx_sessions_count() == (n * (r + 1), 0)
            assert i_st.cpu().numpy().view(np.uint32).tolist() == [0] * n + [GUARD] * 2  # (not written again)
    finally:
        lp.close()


# ---- 7. error returns ----------------------------------------------------------------------------------------------------
def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=16)
    try:
        n = 4
        d_ent = torch.full((n + 1, 176), 0x7E, dtype=torch.uint8, device=dev)
        d_st = torch.full((n + 1,), GUARD, dtype=torch.int32, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        d_send = t_u32(rig, [0, 2, 4, 6, 8])
        d_recv = t_u32(rig, [1, 3, 5, 7, 9])
        d_rcv = torch.full((16,), GUARD, dtype=torch.int32, device=dev)
        d_n = torch.zeros(4, dtype=torch.int32, device=dev)
        args = lambda: [d_ent.data_ptr(), None, d_send.data_ptr(), d_recv.data_ptr(), d_rcv.data_ptr(), d_st.data_ptr(),  # noqa: E731
                        d_sum.data_ptr(), n, n, 0, 16, Lb.WG_HS_INSTALL_SESSIONS, Lb.WG_HS_INSTALL_WIPE]
        call = lambda b: eng._lib.wg_hs_install(eng.ctx, ctypes.byref(b), None)  # noqa: E731

        def untouched():
            torch.cuda.synchronize()
            assert (d_sum.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == GUARD).all()
            assert (d_ent.cpu().numpy() == 0x7E).all() and (d_rcv.cpu().numpy() == GUARD).all()

        assert call(Lb.WgHsInstallBatch(*args())) == Lb.WG_EINVAL and "wg_rx_sessions_reserve" in W._lib.last_error()
        eng.rx_sessions_reserve(8)
        for name, value in [("flags", 2), ("flags", 0x80000001), ("source", 2),
                            ("entries", d_ent.data_ptr() + 8), ("entries", None),     # misaligned, NULL
                            ("n_entries", d_n.data_ptr() + 2),
                            ("send_slot", d_send.data_ptr() + 2), ("send_slot", None),
                            ("recv_slot", d_recv.data_ptr() + 1), ("recv_slot", None),
                            ("receivers", d_rcv.data_ptr() + 2),
                            ("inst_status", d_st.data_ptr() + 2), ("inst_status", None),
                            ("summary", d_sum.data_ptr() + 4), ("summary", None),
                            ("inst_status", d_ent.data_ptr() + 16),                   # inst_status inside entries
                            ("summary", d_ent.data_ptr() + 176 * n - 16),             # summary inside entries
                            ("summary", d_st.data_ptr() + 8),                         # summary inside inst_status
                            ("receivers", d_st.data_ptr()),                           # receivers over inst_status
                            ("n_entries", d_st.data_ptr()),                           # n_entries inside inst_status
                            ("send_slot", d_ent.data_ptr()),                          # send_slot inside entries
                            ("recv_slot", d_rcv.data_ptr())]:                         # recv_slot inside receivers
            b = Lb.WgHsInstallBatch(*args())
            setattr(b, name, value)
            assert call(b) == Lb.WG_EINVAL, (name, value)
        b = Lb.WgHsInstallBatch(*args())
        b.n = (1 << 30) + 1
        assert call(b) == Lb.WG_E2BIG
        assert eng._lib.wg_hs_install(eng.ctx, None, None) == Lb.WG_EINVAL
        assert eng._lib.wg_hs_install(None, ctypes.byref(Lb.WgHsInstallBatch(*args())), None) == Lb.WG_EINVAL
        b = Lb.WgHsInstallBatch(*args())
        b.n = 0  # a no-op
        assert call(b) == Lb.WG_OK
        untouched()
        assert eng._lib.wg_rx_sessions_reserve(eng.ctx, (1 << 29) + 1) == Lb.WG_E2BIG
        assert eng._lib.wg_rx_sessions_reserve(None, 4) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_retire(eng.ctx, None, 3, None, None) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_retire(eng.ctx, d_n.data_ptr() + 2, 1, None, None) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_retire(eng.ctx, d_n.data_ptr(), 1, d_n.data_ptr() + 6, None) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_count(None, None, None) == Lb.WG_EINVAL
        assert eng._lib.wg_rx_sessions_count(eng.ctx, None, None) == Lb.WG_OK
        assert eng.rx_sessions_count() == (0, 0)
        # and with everything in order the same buffers install (entries of 0x7E bytes: position 0x7E7E7E7E is BADSLOT)
        assert call(Lb.WgHsInstallBatch(*args())) == Lb.WG_OK
        torch.cuda.synchronize()
        assert d_st.cpu().numpy().view(np.uint32).tolist() == [IM.INST_BADSLOT] * n + [GUARD]
        assert d_sum.cpu().numpy().tolist() == [0, n, 0, 0]
    finally:
        eng.close()
