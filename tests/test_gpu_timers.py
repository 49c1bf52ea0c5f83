"""wg_timers_start / _mark / _sweep on the MI355X against tests/timers_model.py (pytest -m gpu), byte for byte: the lists,
the summaries, the guard words behind every output, wg_timers_get, wg_timers_peers_get, wg_tx_counters_get and the session
table's counts. The closed loop runs a session's whole life between two contexts: handshake, install, start, traffic
through the gate, a keepalive, the rekey the sweep asks for, and the retirement of the superseded session."""
import struct

import numpy as np
import pytest

import hs_install_model as IM
import timers_model as TM
from test_gpu_hs_initiate import GUARD, initiator, rig, t_u8, t_u32  # noqa: F401
from test_gpu_hs_install import _InstallLoop, _lookup, _tun_packet
from wgtest import splitmix_np

pytestmark = pytest.mark.gpu

SESS, EST = TM.SRC_SESSIONS, TM.SRC_ESTABLISHED
STRIDE = {SESS: 176, EST: 96}
G64 = 0x7E7E7E7E7E7E7E7E
T0 = 5_000_000


def _pkg_cfg(W, c):
    return W.TimersConfig(**{f: getattr(c, f) for f in TM.FIELDS})


class Pair:
    """A context and the model side by side: every call goes to both and the outputs are compared at once."""

    def __init__(self, rig, K, P, cfg, peers=None, eng=None):
        self.rig, self.K, self.P = rig, K, P
        self.own = eng is None
        self.eng = eng or rig.W.Engine(0, key_slots=K)
        self.eng.timers_reserve(P)
        self.eng.timers_config_set(_pkg_cfg(rig.W, cfg))
        self.m = TM.Timers(K, P, cfg)
        if peers:
            self.peers_set(0, peers)
        self.now = rig.torch.zeros(1, dtype=rig.torch.int64, device=rig.dev)

    def close(self):
        if self.own:
            self.eng.close()

    def peers_set(self, first, peers):
        self.eng.timers_peers_set(first, peers)
        self.m.peers_set(first, peers)

    def at(self, t, now=None):
        now = self.now if now is None else now
        now.copy_(self.rig.torch.from_numpy(np.array([t], np.uint64).view(np.int64)).to(self.rig.dev))
        return now

    def counters_set(self, first, values):
        self.eng.tx_counters_set(first, values)
        self.m.send[first:first + len(values)] = [int(v) for v in values]

    def table_set(self, indices, slots):
        self.eng.rx_sessions_reserve(len(indices))
        self.eng.rx_sessions_set(indices, slots)
        self.m.table = dict(zip(indices, slots))

    def entries(self, ents, source, seed=0x9100):
        n = len(ents)
        e = np.frombuffer(splitmix_np(seed + n, STRIDE[source] * n).tobytes(), IM.DTYPES[source]).copy()
        e[IM.POSITION[source]] = [x[1] for x in ents]
        e["peer"] = [x[2] for x in ents]
        e["local_index"] = [x[3] for x in ents]
        return t_u8(self.rig, e.tobytes()).reshape(n, STRIDE[source])

    def start(self, t, ents, send, recv, source, cover=None):
        d_n = None if cover is None else t_u32(self.rig, [cover, 1 << 30])
        self.eng.timers_start(self.entries(ents, source), d_n, t_u32(self.rig, [x[0] for x in ents]), t_u32(self.rig, send),
                              t_u32(self.rig, recv), self.at(t), source)
        self.m.start(t, ents, send, recv, source, cover=cover)

    def mark(self, t, desc, status, tx=False, gate=False, first=0, count=0, stream=None, now=None):
        torch, dev = self.rig.torch, self.rig.dev
        n = len(desc)
        d_desc = torch.full((n + 1, 4), G64, dtype=torch.int64, device=dev)
        d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        if n:
            d_desc[:n] = torch.from_numpy(self.rig.W.desc_as_int64(desc)).to(dev)
            d_st[:n] = t_u32(self.rig, status)
        now = self.at(t, now)
        if stream is not None:  # the buffers were filled on the current stream
            torch.cuda.synchronize()
        self.eng.timers_mark(d_desc[:n], d_st[:n], now, d_sum[:2], tx=tx, gate=gate, slot_first=first, slot_count=count,
                             stream=stream)
        want_d, want_s = desc.copy(), list(status)
        want_sum = self.m.mark(t, want_d, want_s, tx=tx, gate=gate, slot_first=first, slot_count=count)
        torch.cuda.synchronize()
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == list(want_sum) + [GUARD] * 2
        assert d_st.cpu().numpy().view(np.uint32).tolist() == want_s + [GUARD] * 2
        assert d_desc.cpu().numpy().tobytes() == want_d.tobytes() + struct.pack("<4Q", *[G64] * 4)
        return want_sum, want_d, want_s

    def sweep_buffers(self, cap_exp, cap_init, cap_keep):
        torch, dev = self.rig.torch, self.rig.dev
        return (torch.full((cap_exp + 1, 4), GUARD, dtype=torch.int32, device=dev),
                torch.full((cap_init + 2,), GUARD, dtype=torch.int32, device=dev),
                torch.full((cap_keep + 1, 4), G64, dtype=torch.int64, device=dev),
                torch.full((10,), GUARD, dtype=torch.int32, device=dev))

    def compare_sweep(self, bufs, want, caps):
        d_exp, d_init, d_keep, d_sum = bufs
        cap_exp, cap_init, cap_keep = caps
        n_exp = len(want["expired"])
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == want["summary"] + [GUARD] * 2
        assert d_exp.cpu().numpy().tobytes() == want["expired"].tobytes() + struct.pack("<I", GUARD) * (4 * (cap_exp + 1 - n_exp))
        assert d_init.cpu().numpy().view(np.uint32).tolist() == want["initiate"] + [GUARD] * 2
        assert d_keep.cpu().numpy().tobytes() == want["keepalives"].tobytes() + struct.pack("<4Q", *[G64] * 4)

    def sweep(self, t, cap_exp, cap_init, cap_keep, wire_base=0, wire_stride=32, out_size=1 << 30, retire=False):
        bufs = self.sweep_buffers(cap_exp, cap_init, cap_keep)
        self.eng.timers_sweep(self.at(t), bufs[0][:cap_exp], bufs[1][:cap_init], bufs[2][:cap_keep], bufs[3][:8],
                              wire_stride=wire_stride, out_size=out_size, wire_base=wire_base, retire=retire)
        want = self.m.sweep(t, cap_exp, cap_init, cap_keep, wire_base=wire_base, wire_stride=wire_stride, out_size=out_size,
                            retire=retire)
        self.rig.torch.cuda.synchronize()
        self.compare_sweep(bufs, want, (cap_exp, cap_init, cap_keep))
        return want

    def same(self, table=False):
        got = self.eng.timers_get(0, self.K)
        want = self.m.slots_image()
        assert got.tobytes() == want.tobytes(), [(i, g, w) for i, (g, w) in enumerate(zip(got.tolist(), want.tolist())) if g != w][:4]
        assert self.eng.timers_peers_get(0, self.P).tobytes() == self.m.peers_image().tobytes()
        assert self.eng.tx_counters_get(0, self.K).tolist() == self.m.send
        if table:
            assert self.eng.rx_sessions_count() == (len(self.m.table), self.m.retired)


# ---- 1. sweep -------------------------------------------------------------------------------------------------------------
RAM, REKEY_MSG = 1000, 500  # reject_after_messages, rekey_after_messages of the sweep scenarios


def _sweep_mix(n, mix):
    """Per session k (send slot k, recv slot n + k, peer k): expired?, rekey due?, keepalive due?"""
    if mix == "none":
        return [(False, False, False)] * n
    if mix == "all_expired":  # expired, and so listed for initiation; an expired session gets no keepalive
        return [(True, False, True)] * n
    if mix == "all_rekey_keep":
        return [(False, True, True)] * n
    if mix == "seeded":
        r = splitmix_np(0x9200 + n, 3 * n)
        return [(bool(r[3 * k] & 1), bool(r[3 * k + 1] & 1), bool(r[3 * k + 2] & 1)) for k in range(n)]
    edges = {0, n - 1} | {k for k in (255, 256, 511, 512, 1023, 1024) if k < n}  # first and last position of the rank ranges
    assert mix == "range_edges"
    return [(k in edges and k % 2 == 0, k in edges and k % 2 == 1, k in edges) for k in range(n)]


@pytest.mark.parametrize("mix", ["none", "all_expired", "all_rekey_keep", "seeded", "range_edges"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sweep_against_the_model(rig, n, mix):
    flags = _sweep_mix(n, mix)
    cfg = TM.Config(reject_after_messages=RAM, rekey_after_messages=REKEY_MSG, rekey_timeout=0, flags=TM.INITIATOR_ONLY)
    K, P = 2 * n + 3, n + 2  # peers n (can initiate, no session: always due) and n + 1 (cannot) have no session
    p = Pair(rig, K, P, cfg, peers=[(1 if f[2] else 0, True) for f in flags] + [(0, mix != "none"), (9, False)])
    try:
        p.table_set([0x1000 + 7 * k for k in range(n)], [n + k for k in range(n)])
        half = (n + 1) // 2  # the lower half initiated, the upper half responded: under INITIATOR_ONLY it never rekeys
        for src, lo, hi in ((EST, 0, half), (SESS, half, n)):
            if hi > lo:
                p.start(T0, [(0, k, k, 0x1000 + 7 * k) for k in range(lo, hi)], list(range(n)), list(range(n, 2 * n)), src)
        p.counters_set(0, [RAM + k if f[0] else REKEY_MSG if f[1] else 0 for k, f in enumerate(flags)])
        p.same(table=True)
        first = p.sweep(T0 + 1, n + 1, P, n + 1)
        d_exp, d_init, d_keep = first["summary"][0], first["summary"][2], first["summary"][4]
        assert d_exp == sum(f[0] for f in flags) and d_keep == sum(f[2] and not f[0] for f in flags)
        assert d_init == sum((f[0] or (f[1] and k < half)) for k, f in enumerate(flags)) + (mix != "none")
        p.same()
        t = T0 + 1
        for caps in [(0, 0, 0), (1, 1, 1), (max(d_exp - 1, 0), max(d_init - 1, 0), max(d_keep - 1, 0)), (d_exp, d_init, d_keep)]:
            t += 1
            out = p.sweep(t, *caps, wire_base=48, wire_stride=40)
            assert out["summary"][:6:2] == [d_exp, d_init, d_keep]
        p.same()
        out = p.sweep(t + 1, max(d_exp - 1, 0), P, n, retire=True)  # all but the last expired session retired
        assert out["summary"][1] == max(d_exp - 1, 0) and out["summary"][6] == n - max(d_exp - 1, 0)
        p.same(table=True)
        out = p.sweep(t + 2, n, P, n, retire=True)  # ... and the last one
        assert out["summary"][:2] == [min(d_exp, 1)] * 2 and out["summary"][6] == n - d_exp
        p.same(table=True)
        assert p.sweep(t + 3, n, P, n, retire=True)["summary"][:2] == [0, 0]
    finally:
        p.close()


@pytest.mark.parametrize("t0", [(1 << 32) - 5, (1 << 63) - 5, (1 << 64) - 40])
def test_sweep_ticks_at_the_word_edges_and_a_clock_behind_the_birth(rig, t0):
    cfg = TM.Config(rekey_after_time=6, reject_after_time=10, rekey_timeout=2, keepalive_timeout=3, linger=4, flags=TM.INITIATOR_ONLY)
    p = Pair(rig, 12, 3, cfg, peers=[(4, True), (0, True), (0, True)])
    try:
        p.start(t0, [(0, 0, 0, 0x31), (0, 1, 1, 0x32)], [0, 2], [1, 3], EST)
        out = p.sweep(t0 - 10, 4, 4, 4, retire=True)  # born > now: no age, but the new session's keepalive and peer 2
        assert out["summary"] == [0, 0, 1, 1, 1, 1, 2, 0]
        d = np.zeros(1, TM.PKT_DTYPE)
        d[0] = (0, 0, 0, 8, 3)
        p.mark(t0 + 1, d, [TM.PKT_OK])  # data from peer 1, never answered: a passive keepalive 3 ticks later
        p.start(t0 + 2, [(0, 0, 0, 0x33)], [4], [5], EST)  # peer 0 rekeys: session (0, 1) lingers for 4 ticks
        for dt in range(3, 14):
            p.sweep(t0 + dt, 4, 4, 4, wire_stride=32, out_size=96, retire=dt % 2 == 0)
            p.same()
        assert p.m.slots[0]["state"] == TM.DEAD and p.m.slots[2]["state"] == TM.DEAD and p.m.slots[4]["state"] == TM.DEAD
    finally:
        p.close()


# ---- 2. mark --------------------------------------------------------------------------------------------------------------
def _mark_rig(rig, n):
    """K key slots in pairs (2q, 2q + 1): q % 4 == 0 we initiated, 1 we responded, 2 no record, 3 retired (both DEAD)."""
    K = max((n - 4) & ~1, 8) if n <= 4096 else n
    Q = K // 2
    cfg = TM.Config(reject_after_time=1000, reject_after_messages=RAM)
    p = Pair(rig, K, Q, cfg)
    for src, sel in ((EST, 0), (SESS, 1), (EST, 3)):
        qs = [q for q in range(Q) if q % 4 == sel]
        if qs:
            p.start(T0, [(0, q, q, 0x2000 + q) for q in qs], [2 * q for q in range(Q)], [2 * q + 1 for q in range(Q)], src)
    dead = [2 * q for q in range(Q) if q % 4 == 3]
    p.counters_set(0, [RAM if s in set(dead) else 0 for s in range(K)])
    out = p.sweep(T0, Q, 0, 0, retire=True)
    assert out["summary"][1] == len(dead)
    return p, K


@pytest.mark.parametrize("spread", ["one", "own"])
@pytest.mark.parametrize("n", [1, 64, 65, 257, 4096])
def test_mark_against_the_model(rig, n, spread):
    p, K = _mark_rig(rig, n)
    try:
        r = splitmix_np(0x9300 + n, 4 * n)
        status = [[0, 0, 0, 3, 3, 1, 9, 6][int(x) & 7] for x in r[:n]]
        desc = np.zeros(n, TM.PKT_DTYPE)
        desc["len"] = [0 if x & 3 == 0 else 1 + int(x) for x in r[n:2 * n]]
        desc["counter"] = [int(x) for x in r[2 * n:3 * n]]
        desc["in_off"], desc["out_off"] = 32 * np.arange(n), 64 * np.arange(n)
        t = T0 + 10
        for tx in (False, True):
            for one_slot in ([1, 3, 5, 7] if not tx else [0, 2, 4, 6]):  # records of every state: RECV / SEND, none, DEAD
                if spread == "one":
                    desc["key_slot"] = one_slot
                else:
                    desc["key_slot"] = np.arange(n) + (one_slot >> 1)  # each on its own slot, the last ones past the key table
                    if one_slot > 3:
                        continue
                t += 1
                p.mark(t, desc, status, tx=tx)
                if tx:  # the gate over a slot range that cuts the batch
                    t += 1
                    p.mark(t, desc, status, tx=True, gate=True, first=K // 4, count=K // 2)
                    p.mark(t, desc, status, tx=True, gate=True, first=0, count=0xFFFFFFFF)
        p.same()
        # the limits of the gate, on a live send slot: counter at reject_after_messages - 1, at it, past it; age at the bound
        g = np.zeros(4, TM.PKT_DTYPE)
        g["key_slot"], g["len"], g["counter"] = 0, [5, 5, 5, 0], [RAM - 1, RAM, RAM + 1, 0]
        s, gd, gs = p.mark(T0 + 999, g, [0, 0, 0, 0], tx=True, gate=True, first=0, count=1)
        assert s == (2, 2) and gs == [0, TM.PKT_NOSESSION, TM.PKT_NOSESSION, 0] and gd["len"].tolist() == [5, TM.LEN_INVALID, TM.LEN_INVALID, 0]
        s, gd, gs = p.mark(T0 + 1000, g, [0, 0, 0, 0], tx=True, gate=True, first=0, count=1)
        assert s == (0, 4)
        assert p.mark(T0 + 1000, g, [0, 0, 0, 0], tx=True, gate=True, first=1, count=5)[0] == (4, 0)  # outside the gated range
        assert p.mark(T0 + 1000, g, [0, 0, 0, 0], tx=True)[0] == (4, 0)                                  # no gate
        assert p.mark(0, g, [0, 0, 0, 0], tx=True, gate=True, first=0, count=1)[0] == (0, 0)            # tick 0: nothing
        assert p.mark(T0, g[:0], [])[0] == (0, 0)                                                        # n = 0: a zero summary
        p.same()
    finally:
        p.close()


def test_marks_on_two_streams_with_different_clocks_keep_the_larger_stamp(rig):
    torch, dev = rig.torch, rig.dev
    p, K = _mark_rig(rig, 64)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        now2 = torch.zeros(1, dtype=torch.int64, device=dev)
        d = np.zeros(65, TM.PKT_DTYPE)
        d["key_slot"], d["len"] = 1, 9
        torch.cuda.synchronize()
        p.mark(T0 + 700, d, [0] * 65, stream=s1.cuda_stream)
        p.mark(T0 + 300, d, [0] * 65, stream=s2.cuda_stream, now=now2)  # the later call carries the earlier clock
        d["key_slot"] = 0
        p.mark(T0 + 200, d, [0] * 65, tx=True, stream=s2.cuda_stream, now=now2)
        p.mark(T0 + 900, d, [0] * 65, tx=True, stream=s1.cuda_stream)
        p.same()
        got = p.eng.timers_get(0, 2)
        assert got["last"].tolist() == [T0 + 900, T0 + 700] and got["last_data"].tolist() == [T0 + 900, T0 + 700]
    finally:
        p.close()


# ---- 3. start -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linger", [0, 50])
def test_start_against_the_model(rig, linger):
    cfg = TM.Config(linger=linger, rekey_timeout=1 << 40)
    p = Pair(rig, 600, 4, cfg, peers=[(0, True)] * 4)
    try:
        p.start(T0, [(0, 0, 0, 0x10), (0, 1, 1, 0x11), (0, 2, 2, 0x12)], [0, 2, 4], [1, 3, 5], SESS)
        p.same()
        assert [x["current"] for x in p.m.peers] == [0, 2, 4, TM.NOSLOT]
        # 0 refused by the install; 1 and 2 both peer 0's (1 becomes current, 2 starts superseded); 3 takes the recv slot of
        # peer 1's session and kills it; 4 has a peer past the table; 5 takes both slots of peer 2's session, crosswise, for
        # peer 3; 6 is behind n_entries
        ent = [(2, 0, 0, 0x20), (0, 1, 0, 0x21), (0, 2, 0, 0x22), (0, 3, 0, 0x23), (0, 4, 7, 0x24), (0, 5, 3, 0x25), (0, 6, 3, 0x26)]
        p.start(T0 + 5, ent, [9, 10, 12, 14, 16, 5, 18], [9, 11, 13, 3, 17, 4, 19], EST, cover=6)
        p.same()
        m = p.m
        assert m.peers[0]["current"] == 10 and m.slots[0]["superseded"] == T0 + 5 and m.slots[12]["superseded"] == T0 + 5
        assert m.slots[2]["state"] == TM.DEAD and m.peers[1]["current"] == TM.NOSLOT and m.slots[16]["peer"] == TM.NOPEER
        assert m.peers[2]["current"] == TM.NOSLOT and m.peers[3]["current"] == 5 and m.slots[18]["state"] == TM.NONE
        out = p.sweep(T0 + 5 + 49, 8, 4, 8, retire=True)
        assert out["summary"][:2] == [0, 0]
        out = p.sweep(T0 + 5 + 50, 8, 4, 8, retire=True)  # the superseded sessions, if they linger at all
        assert out["expired"]["send_slot"].tolist() == ([0, 12, 14] if linger else [])
        p.same()
        # more sessions of one peer than a wave, than a workgroup: the lowest entry wins whatever the dispatch order
        n = 260
        ent = [(0 if k % 7 else 3, k, k % 3, 0x4000 + k) for k in range(n)]
        p.start(T0 + 100, ent, [40 + 2 * k for k in range(n)], [41 + 2 * k for k in range(n)], SESS)
        p.same()
        assert [m.peers[k]["current"] for k in range(3)] == [40 + 2 * 3, 40 + 2, 40 + 4]
        p.start(0, [(0, 0, 0, 0x77)], [30], [31], EST)  # tick 0: nothing
        p.same()
    finally:
        p.close()


def test_start_behind_a_real_install_reads_wiped_entries(rig):
    torch, dev, L = rig.torch, rig.dev, rig.W._lib
    p = Pair(rig, 16, 2, TM.Config())
    try:
        p.eng.rx_sessions_reserve(8)
        ents = [(0, 0, 0, 0x51), (0, 1, 1, 0x52), (0, 1, 1, 0x53), (0, 2, 0, 0x51)]  # 2: DUPSLOT, 3: DUPINDEX
        d_ent = p.entries(ents, SESS)
        send, recv = t_u32(rig, [2, 4, 6]), t_u32(rig, [3, 5, 7])
        i_st = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        i_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        p.eng.hs_install(d_ent, None, send, recv, i_st, i_sum, 0, 16, L.WG_HS_INSTALL_SESSIONS, wipe=True)
        p.eng.timers_start(d_ent, None, i_st, send, recv, p.at(T0), L.WG_HS_INSTALL_SESSIONS)
        torch.cuda.synchronize()
        st = i_st.cpu().numpy().tolist()
        assert st == [0, 0, IM.INST_DUPSLOT, IM.INST_DUPINDEX]
        e = d_ent.cpu().numpy().reshape(-1).view(IM.HS_SESSION)
        assert not e["send_key"][:2].any() and e["send_key"][2].any() and e["send_key"][3].any()  # installed: wiped
        p.m.start(T0, [(s,) + x[1:] for s, x in zip(st, ents)], [2, 4, 6], [3, 5, 7], SESS)
        p.same()
        assert p.m.slots[2]["state"] == TM.SEND_RESPONDER and p.m.slots[6]["state"] == TM.NONE
    finally:
        p.close()


# ---- 4. graphs ------------------------------------------------------------------------------------------------------------
def test_captured_mark_and_sweep_replay_with_the_clock_rewritten_in_place(rig):
    torch, dev = rig.torch, rig.dev
    cfg = TM.Config(rekey_after_time=40, rekey_timeout=15, keepalive_timeout=10, reject_after_time=70)
    p = Pair(rig, 300, 140, cfg, peers=[(k % 3 * 7, k % 2 == 0) for k in range(140)])
    try:
        n = 130
        p.start(T0, [(0, k, k, 0x100 + k) for k in range(n)], [2 * k for k in range(n)], [2 * k + 1 for k in range(n)], EST)
        desc = np.zeros(257, TM.PKT_DTYPE)
        desc["key_slot"] = 2 * (np.arange(257) % 100) + 1  # data from the first 100 peers
        desc["len"] = 1 + np.arange(257) % 5
        status = [0 if k % 4 else 3 for k in range(257)]
        d_desc = torch.from_numpy(rig.W.desc_as_int64(desc)).to(dev)
        d_st, m_sum = t_u32(rig, status), torch.zeros(2, dtype=torch.int32, device=dev)
        bufs = p.sweep_buffers(8, 16, 200)
        p.at(T0 + 1)
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            p.eng.timers_mark(d_desc, d_st, p.now, m_sum, stream=side.cuda_stream)
            p.eng.timers_sweep(p.now, bufs[0][:8], bufs[1][:16], bufs[2][:200], bufs[3][:8], wire_stride=32, out_size=32 * 150,
                               retire=True, stream=side.cuda_stream)
        for t in (T0 + 12, T0 + 45, T0 + 71):
            for b, fill in zip(bufs, (GUARD, GUARD, G64, GUARD)):
                b.fill_(fill)
            p.at(t)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert m_sum.cpu().numpy().tolist() == list(p.m.mark(t, desc.copy(), list(status)))
            p.compare_sweep(bufs, p.m.sweep(t, 8, 16, 200, wire_stride=32, out_size=32 * 150, retire=True), (8, 16, 200))
            p.same()
    finally:
        p.close()


def test_captured_sweep_and_initiate_over_the_whole_capacity(rig):
    """Two of four peers are due; wg_hs_initiate over the list's four places initiates two handshakes, answers the padding
    BADPEER and leaves the ephemerals behind them as they were."""
    torch, dev, L = rig.torch, rig.dev, rig.W._lib
    eng = initiator(rig)
    p = Pair(rig, 16, 4, TM.reference(1000), peers=[(0, False), (0, True), (0, False), (0, True)], eng=eng)
    try:
        eng.hs_reserve(4)
        bufs = p.sweep_buffers(2, 4, 2)
        eph = torch.zeros(32 * 4, dtype=torch.uint8, device=dev)
        ts, li = t_u8(rig, bytes(range(48))), t_u32(rig, [0x71, 0x72, 0x73, 0x74])
        st = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        rec, pend = torch.zeros((4, 160), dtype=torch.uint8, device=dev), torch.zeros((4, 112), dtype=torch.uint8, device=dev)
        i_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        p.at(T0)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            eng.timers_sweep(p.now, bufs[0][:2], bufs[1][:4], bufs[2][:2], bufs[3][:8], stream=side.cuda_stream)
            eng.hs_initiate(bufs[1][:4], eph, ts, li, st, rec, pend, i_sum, stream=side.cuda_stream)
        for t, want_listed in ((T0, [1, 3]), (T0 + 4_999, []), (T0 + 5_000, [1, 3])):
            fresh = splitmix_np(0x9400 + t % 1000, 128)
            eph.copy_(torch.from_numpy(fresh).to(dev))
            p.at(t)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = p.m.sweep(t, 2, 4, 2)
            assert want["initiate"] == want_listed + [0xFFFFFFFF] * (4 - len(want_listed))
            p.compare_sweep(bufs, want, (2, 4, 2))
            k = len(want_listed)
            assert st.cpu().numpy().tolist() == [L.WG_HS_INIT_OK] * k + [L.WG_HS_INIT_BADPEER] * (4 - k)
            assert i_sum.cpu().numpy().tolist() == [k, 4 - k, 0, 0]
            left = eph.cpu().numpy()
            assert not left[:32 * k].any() and left[32 * k:].tobytes() == fresh[32 * k:].tobytes()  # the padding consumed none
            assert pend.cpu().numpy().reshape(-1).view(rig.W.WG_HS_PENDING_DTYPE)["peer"][:k].tolist() == want_listed
    finally:
        eng.close()


# ---- 5. the closed loop ---------------------------------------------------------------------------------------------------
class _Side:
    """One context's transport buffers for rings of up to m packets."""

    def __init__(self, rig, m):
        torch, dev = rig.torch, rig.dev
        self.desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        self.st, self.host, self.ost, self.fst = (torch.full((m,), GUARD, dtype=torch.int32, device=dev) for _ in range(4))
        self.sum, self.deliv = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        self.items = torch.zeros((m, 2), dtype=torch.int64, device=dev)
        self.pt = torch.zeros(128 * m, dtype=torch.uint8, device=dev)
        self.msum = torch.zeros(2, dtype=torch.int32, device=dev)


def test_closed_loop_a_session_lives_rekeys_and_is_retired(rig):
    torch, dev, W, L = rig.torch, rig.dev, rig.W, rig.W._lib
    lp = _InstallLoop(rig, 1, 8)
    A, B = lp.A, lp.B
    try:
        cfg = W.TimersConfig.wireguard(1000)
        cfg.linger = 10_000
        for eng, peer in ((A, (25_000, True)), (B, (0, False))):
            eng.rx_sessions_reserve(4)
            eng.replay_enable(128)
            eng.timers_reserve(1)
            eng.timers_config_set(cfg)
            eng.timers_peers_set(0, [peer])
        a_recv, b_recv = (torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(2))
        A.set_receivers(a_recv)
        now = torch.zeros(1, dtype=torch.int64, device=dev)
        i_st, i_sum = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        ra, rb = _Side(rig, 4), _Side(rig, 4)
        stride, max_len = 144, 100
        wire = torch.zeros(stride * 4, dtype=torch.uint8, device=dev)

        def handshake(seed, s, r, t):
            """1 / 5: handshake, install and start on both sides; the host chooses slots, indices and `now`."""
            lp.initiate_and_respond(seed)
            lp.check_and_finish()
            now.fill_(t)
            send, recv = t_u32(rig, [s]), t_u32(rig, [r])
            for eng, ent, n_ok, src, rcv in ((A, lp.f_est, lp.f_sum, L.WG_HS_INSTALL_ESTABLISHED, a_recv),
                                             (B, lp.b_sess, lp.b_rsum, L.WG_HS_INSTALL_SESSIONS, b_recv)):
                eng.hs_install(ent, n_ok, send, recv, i_st, i_sum, 0, 8, src, receivers=rcv)
                eng.timers_start(ent, n_ok, i_st, send, recv, now, src)
                torch.cuda.synchronize()
                assert i_sum.cpu().numpy().tolist() == [1, 0, 0, 0]

        def carry(pkts, t, want_tx, want_final, ring=None, lens=None):
            """2: A plans, gates and seals the tun packets (or `ring` is taken as sealed already); B plans, opens, checks,
            delivers and marks. Returns B's final statuses."""
            m = len(want_final)
            now.fill_(t)
            if ring is None:
                tun = np.zeros(128 * m, np.uint8)
                for k, pk in enumerate(pkts):
                    tun[128 * k:128 * k + len(pk)] = np.frombuffer(pk, np.uint8)
                d_tun = torch.from_numpy(tun).to(dev)
                t_off, t_len = torch.arange(0, 128 * m, 128, dtype=torch.int64, device=dev), t_u32(rig, [len(pk) for pk in pkts])
                wire.zero_()
                A.tx_plan(d_tun, t_off, t_len, ra.desc[:m], ra.st[:m], stride, wire.numel(), max_len, route=True)
                A.timers_mark(ra.desc[:m], ra.st[:m], now, ra.msum, tx=True, gate=True, slot_first=0, slot_count=8)
                A.seal(ra.desc[:m], d_tun, wire, max_len, frame=True)
                torch.cuda.synchronize()
                assert ra.st[:m].cpu().numpy().tolist() == want_tx
                ring, lens = wire, [len(pk) + 32 for pk in pkts]
            w_off = torch.arange(0, stride * m, stride, dtype=torch.int64, device=dev)
            B.rx_plan(ring, w_off, t_u32(rig, lens), rb.desc[:m], rb.st[:m], rb.host[:m], rb.sum, max_len, packed=True, pt_size=rb.pt.numel())
            B.open(rb.desc[:m], ring, rb.pt, rb.ost[:m], max_len, rx_filter=True)
            B.rx_check(rb.desc[:m], rb.pt, rb.ost[:m], L.WG_RX_REPLAY)
            B.rx_deliver(rb.desc[:m], rb.st[:m], rb.ost[:m], rb.fst[:m], rb.items[:m], rb.deliv)
            B.timers_mark(rb.desc[:m], rb.fst[:m], now, rb.msum)
            torch.cuda.synchronize()
            assert rb.fst[:m].cpu().numpy().tolist() == want_final
            return ring

        handshake(1, 2, 3, T0)
        A.routes_set([("10.1.0.0", 32, 2)])
        pkts = [_tun_packet(0, k, 60 + k) for k in range(3)]
        carry(pkts, T0 + 1_000, [0, 0, 0], [0, 0, 0])
        assert ra.msum.cpu().numpy().tolist() == [3, 0] and rb.msum.cpu().numpy().tolist() == [3, 0]
        a, b = A.timers_get(0, 8), B.timers_get(0, 8)
        assert (a[2]["state"], a[3]["state"], b[2]["state"], b[3]["state"]) == (TM.SEND_INITIATOR, TM.RECV, TM.SEND_RESPONDER, TM.RECV)
        assert (int(a[2]["last"]), int(a[2]["last_data"]), int(b[3]["last"]), int(b[3]["last_data"])) == (T0 + 1_000,) * 4
        # 3 / 4: the clock advances; A's tick lists its peer and emits a keepalive, sealed and framed
        t1 = T0 + 120_000
        now.fill_(t1)
        exp, init = torch.full((2, 4), GUARD, dtype=torch.int32, device=dev), torch.full((2,), GUARD, dtype=torch.int32, device=dev)
        keep, s_sum = torch.zeros((2, 4), dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
        ka_ring = torch.zeros(stride * 2, dtype=torch.uint8, device=dev)
        A.timers_tick(now, exp, init, keep, s_sum, ka_ring, stride)
        torch.cuda.synchronize()
        assert s_sum.cpu().numpy().tolist() == [0, 0, 1, 1, 1, 1, 1, 0] and init.cpu().numpy().view(np.uint32).tolist() == [0, 0xFFFFFFFF]
        assert A.tx_counters_get(2, 1).tolist() == [4] and ka_ring[:32].cpu().numpy().any() and not ka_ring[32:].cpu().numpy().any()
        carry(None, t1 + 1, None, [L.WG_PKT_KEEPALIVE], ring=ka_ring, lens=[32])
        b = B.timers_get(3, 1)[0]
        assert (int(b["last"]), int(b["last_data"])) == (t1 + 1, T0 + 1_000) and rb.msum.cpu().numpy().tolist() == [1, 0]
        # 5 / 6: the listed peer goes through initiate ... start; the old session is superseded on both sides
        old_index = int(A.timers_get(2, 1)[0]["local_index"])
        lp.peer.copy_(init[:1])
        t2 = t1 + 2_000
        handshake(2, 4, 5, t2)
        for eng in (A, B):
            s = eng.timers_get(0, 8)
            assert int(s[2]["superseded"]) == t2 and int(s[4]["born"]) == t2 and eng.timers_peers_get(0, 1)[0]["current"] == 4
            assert eng.rx_sessions_count() == (2, 0)
        # 7: linger later the sweep retires it
        now.fill_(t2 + 10_000)
        A.timers_sweep(now, exp, init, keep, s_sum, wire_stride=stride, out_size=ka_ring.numel(), retire=True)
        torch.cuda.synchronize()
        assert s_sum.cpu().numpy().tolist()[:2] == [1, 1] and s_sum.cpu().numpy().tolist()[6] == 1
        assert exp.cpu().numpy().view(np.uint32)[0].tolist() == [2, 3, 0, old_index]
        assert A.rx_sessions_count() == (1, 1) and _lookup(rig, A, [old_index]) == [None]
        assert [int(x) for x in A.timers_get(2, 2)["state"]] == [TM.DEAD, TM.DEAD]
        # traffic still routed to the old send slot is refused by the gate, and the seal leaves its wire slot alone
        carry(pkts[:1], t2 + 10_001, [L.WG_PKT_NOSESSION], [L.WG_PKT_BADHDR])
        assert ra.msum.cpu().numpy().tolist() == [0, 1] and not wire.cpu().numpy().any()
        assert int(ra.desc[0, 3].cpu()) & 0xFFFFFFFF == L.WG_LEN_INVALID
        # ... and on the new session it flows
        A.routes_set([("10.1.0.0", 32, 4)])
        carry(pkts, t2 + 10_002, [0, 0, 0], [0, 0, 0])
        got = np.ascontiguousarray(rb.items[:3].cpu().numpy()).view(np.dtype([("off", "<u8"), ("len", "<u4"), ("slot", "<u4")])).reshape(-1)
        pt = rb.pt.cpu().numpy()
        for it, pk in zip(got, pkts):
            assert pt[int(it["off"]):int(it["off"]) + int(it["len"])].tobytes() == pk and int(it["slot"]) == 5
        assert int(B.timers_get(5, 1)[0]["last_data"]) == t2 + 10_002
    finally:
        lp.close()


# ---- 6. untouched paths ---------------------------------------------------------------------------------------------------
def test_a_context_without_timers_is_byte_for_byte_what_it_was(rig):
    """A guard, not a measurement: two contexts that never call wg_timers_* and one that reserves them plan, seal and
    install the same bytes."""
    torch, dev, L = rig.torch, rig.dev, rig.W._lib
    outs = []
    for with_timers in (False, False, True):
        eng = rig.W.Engine(0, key_slots=16)
        try:
            if with_timers:
                eng.timers_reserve(4)
            eng.rx_sessions_reserve(4)
            ents = [(0, 0, 0, 0x51), (0, 1, 1, 0x52)]
            e = np.frombuffer(splitmix_np(0x9500, 176 * 2).tobytes(), IM.HS_SESSION).copy()
            e["init"], e["local_index"] = [0, 1], [0x51, 0x52]
            d_ent = t_u8(rig, e.tobytes()).reshape(2, 176)
            recvs = torch.zeros(16, dtype=torch.int32, device=dev)
            eng.set_receivers(recvs)
            i_st, i_sum = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
            eng.hs_install(d_ent, None, t_u32(rig, [2, 4]), t_u32(rig, [3, 5]), i_st, i_sum, 0, 16, L.WG_HS_INSTALL_SESSIONS, receivers=recvs)
            eng.routes_set([("10.1.0.0", 32, 2), ("10.1.0.1", 32, 4)])
            pkts = [_tun_packet(k & 1, k, 40 + k) for k in range(5)] + [b""]
            tun = np.zeros(128 * 6, np.uint8)
            for k, pk in enumerate(pkts):
                tun[128 * k:128 * k + len(pk)] = np.frombuffer(pk, np.uint8)
            desc, st = torch.zeros((6, 4), dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int32, device=dev)
            wire = torch.zeros(144 * 6, dtype=torch.uint8, device=dev)
            eng.tx_seal(torch.from_numpy(tun).to(dev), torch.arange(0, 128 * 6, 128, dtype=torch.int64, device=dev),
                        t_u32(rig, [len(pk) for pk in pkts]), desc, st, wire, 144, 100, route=True)
            torch.cuda.synchronize()
            outs.append((d_ent.cpu().numpy().tobytes(), i_st.cpu().numpy().tobytes(), i_sum.cpu().numpy().tobytes(),
                         desc.cpu().numpy().tobytes(), st.cpu().numpy().tobytes(), wire.cpu().numpy().tobytes(),
                         eng.tx_counters_get(0, 16).tobytes(), eng.rx_sessions_count()))
        finally:
            eng.close()
    assert outs[0] == outs[1] == outs[2]
    assert outs[0][4] == np.array([0, 0, 0, 0, 0, L.WG_PKT_BADIP], np.int32).tobytes()


def test_error_returns(rig):
    import ctypes
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=8)
    try:
        now = torch.zeros(2, dtype=torch.int64, device=dev)
        summ = torch.zeros(8, dtype=torch.int32, device=dev)
        desc, st = torch.zeros((4, 4), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        mark = lambda **kw: Lb.WgTimersMarkBatch(**{**dict(desc=desc.data_ptr(), status=st.data_ptr(), now=now.data_ptr(),  # noqa: E731
                                                           summary=summ.data_ptr(), n=4), **kw})
        sweep = lambda **kw: Lb.WgTimersSweepBatch(**{**dict(now=now.data_ptr(), summary=summ.data_ptr()), **kw})  # noqa: E731
        lib = eng._lib
        assert lib.wg_timers_mark(eng.ctx, ctypes.byref(mark()), None) == Lb.WG_EINVAL and "wg_timers_reserve" in Lb.last_error()
        assert lib.wg_timers_sweep(eng.ctx, ctypes.byref(sweep()), None) == Lb.WG_EINVAL
        assert lib.wg_timers_get(eng.ctx, 0, 1, now.data_ptr()) == Lb.WG_EINVAL
        assert lib.wg_timers_reserve(eng.ctx, (1 << 30) + 1) == Lb.WG_E2BIG and lib.wg_timers_reserve(None, 1) == Lb.WG_EINVAL
        eng.timers_reserve(4)
        eng.timers_reserve(3)  # not above the first: a no-op
        assert lib.wg_timers_reserve(eng.ctx, 5) == Lb.WG_EINVAL
        for kw in (dict(dir=2), dict(flags=2), dict(flags=1, dir=0), dict(_reserved=1), dict(now=None), dict(now=now.data_ptr() + 4),
                   dict(summary=None), dict(summary=summ.data_ptr() + 4), dict(desc=None), dict(desc=desc.data_ptr() + 8),
                   dict(status=st.data_ptr() + 2)):
            assert lib.wg_timers_mark(eng.ctx, ctypes.byref(mark(**kw)), None) == Lb.WG_EINVAL, kw
        for kw in (dict(flags=2), dict(now=None), dict(summary=summ.data_ptr() + 4), dict(expired_cap=1), dict(initiate_cap=1),
                   dict(keepalive_cap=1, keepalives=desc.data_ptr() + 8)):
            assert lib.wg_timers_sweep(eng.ctx, ctypes.byref(sweep(**kw)), None) == Lb.WG_EINVAL, kw
        assert lib.wg_timers_sweep(eng.ctx, ctypes.byref(sweep(initiate_cap=(1 << 30) + 1, initiate=st.data_ptr())), None) == Lb.WG_E2BIG
        assert lib.wg_timers_get(eng.ctx, 7, 2, now.data_ptr()) == Lb.WG_ERANGE
        assert lib.wg_timers_peers_get(eng.ctx, 4, 1, now.data_ptr()) == Lb.WG_ERANGE
        with pytest.raises(W.WgError):
            eng.timers_peers_set(3, [(0, True), (0, True)])
        bad = W.TimersConfig(flags=2)
        with pytest.raises(W.WgError):
            eng.timers_config_set(bad)
        assert lib.wg_timers_sweep(eng.ctx, ctypes.byref(sweep()), None) == Lb.WG_OK  # no list at all: the summary alone
        torch.cuda.synchronize()
        assert summ.cpu().numpy().tolist() == [0] * 8
    finally:
        eng.close()
