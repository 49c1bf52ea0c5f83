"""tests/timers_model.py pinned to the reference's rules (EstablishedSession.java:28,:114, SessionManager.java:92-111,:188,
KeepaliveSender.java:29-85) and to WireGuard's constants; and the package's two presets against the model's."""
import importlib
import random

import numpy as np
import pytest

import timers_model as TM

T0 = 1_000_000  # the tick of the sessions' start (any tick but 0, which is "never")


def _one(cfg, source=TM.SRC_ESTABLISHED, interval=0, can=True, now=T0):
    """One peer with one session on slots (send 2, recv 3), index 0x51."""
    m = TM.Timers(8, 2, cfg)
    m.peers_set(0, [(interval, can)])
    m.start(now, [(TM.INST_OK, 0, 0, 0x51)], [2], [3], source, install=True)
    return m


def _sweep(m, now, **kw):
    args = dict(cap_exp=8, cap_init=4, cap_keep=8, wire_stride=32, out_size=32 * 8)
    args.update(kw)
    return m.sweep(now, **args)


def _listed(out):
    return [p for p in out["initiate"] if p != 0xFFFFFFFF]


def test_presets_match_the_package():
    wg = importlib.import_module("wireguard-java_amd")
    for name in ("reference", "wireguard"):
        a, b = getattr(wg.TimersConfig, name)(1000), getattr(TM, name)(1000)
        assert [getattr(a, f) for f in TM.FIELDS] == [getattr(b, f) for f in TM.FIELDS]
    r, w = TM.reference(1000), TM.wireguard(1000)
    assert (r.rekey_after_time, r.rekey_timeout) == (120_000, 5_000)
    assert not any((r.reject_after_time, r.keepalive_timeout, r.linger, r.rekey_after_messages, r.reject_after_messages, r.flags))
    assert (w.rekey_after_time, w.reject_after_time, w.rekey_timeout, w.keepalive_timeout, w.linger) == (120_000, 180_000, 5_000, 10_000, 180_000)
    assert (w.rekey_after_messages, w.reject_after_messages, w.flags) == (2 ** 60, 2 ** 64 - 2 ** 13 - 1, TM.INITIATOR_ONLY)
    assert TM.SLOT_DTYPE.itemsize == 48 and TM.PEER_DTYPE.itemsize == 24 and TM.SLOT_DTYPE == wg.WG_TIMER_SLOT_DTYPE


def test_reference_reinitiates_at_120_s_and_retries_after_5_s():
    m = _one(TM.reference(1000))
    assert _listed(_sweep(m, T0 + 119_999)) == []
    assert _listed(_sweep(m, T0 + 120_000)) == [0] and m.peers[0]["rekey_listed"] == T0 + 120_000
    assert _listed(_sweep(m, T0 + 120_000 + 4_999)) == []
    out = _sweep(m, T0 + 125_000)
    assert _listed(out) == [0] and out["initiate"] == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    # the reference never stops using a session: nothing expires, however old
    assert _sweep(m, T0 + 10 ** 9, retire=True)["summary"][:2] == [0, 0] and m.slots[2]["state"] == TM.SEND_INITIATOR
    # ... and the responder's side is listed too (the reference has no "only the initiator")
    assert _listed(_sweep(_one(TM.reference(1000), source=TM.SRC_SESSIONS), T0 + 120_000)) == [0]


def test_reference_lists_nothing_without_can_initiate():
    m = _one(TM.reference(1000), can=False)
    for dt in (0, 120_000, 10 ** 7):
        assert _listed(_sweep(m, T0 + dt)) == []
    m2 = TM.Timers(8, 2, TM.reference(1000))  # no session at all
    assert _listed(_sweep(m2, T0)) == []
    m2.peers_set(1, [(0, True)])
    assert _listed(_sweep(m2, T0)) == [1]


def test_reference_persistent_keepalive_at_the_first_sweep_then_every_interval():
    m = _one(TM.reference(1000), interval=25_000)
    out = _sweep(m, T0 + 1, wire_base=64, wire_stride=48, out_size=64 + 48 * 8)
    assert out["summary"][4:6] == [1, 1]
    assert out["keepalives"][0].tolist() == (0, 64 + 16, 0, 0, 2) and m.send[2] == 1 and m.slots[2]["last"] == T0 + 1
    assert out["keepalives"][1].tolist() == (0, 0, 0, TM.LEN_INVALID, 0)
    assert _sweep(m, T0 + 1 + 24_999)["summary"][4] == 0
    out = _sweep(m, T0 + 1 + 25_000)
    assert out["summary"][4:6] == [1, 1] and int(out["keepalives"][0]["counter"]) == 1 and m.send[2] == 2
    # traffic we send postpones it
    d = np.zeros(1, TM.PKT_DTYPE)
    d[0] = (0, 0, 2, 100, 2)
    assert m.mark(T0 + 40_000, d, [TM.PKT_OK], tx=True) == (1, 0)
    assert _sweep(m, T0 + 64_999)["summary"][4] == 0 and _sweep(m, T0 + 65_000)["summary"][4] == 1
    # without an interval the reference sends none
    assert _sweep(_one(TM.reference(1000)), T0 + 10 ** 6)["summary"][4] == 0


def test_wireguard_responder_is_never_listed_for_rekey():
    m = _one(TM.wireguard(1000), source=TM.SRC_SESSIONS)
    for dt in (120_000, 150_000, 179_999):
        assert _listed(_sweep(m, T0 + dt)) == []
    mi = _one(TM.wireguard(1000))
    assert _listed(_sweep(mi, T0 + 119_999)) == [] and _listed(_sweep(mi, T0 + 120_000)) == [0]
    # by messages too
    mi2 = _one(TM.wireguard(1000))
    mi2.send[2] = 2 ** 60 - 1
    assert _listed(_sweep(mi2, T0 + 1)) == []
    mi2.send[2] = 2 ** 60
    assert _listed(_sweep(mi2, T0 + 1)) == [0]
    m.send[2] = 2 ** 60
    assert _listed(_sweep(m, T0 + 1)) == []


def test_wireguard_passive_keepalive_only_after_data():
    m = _one(TM.wireguard(1000))
    assert _sweep(m, T0 + 50_000)["summary"][4] == 0  # silence on both sides: none
    d = np.zeros(1, TM.PKT_DTYPE)
    d[0] = (0, 0, 0, 0, 3)
    assert m.mark(T0 + 60_000, d, [TM.PKT_KEEPALIVE]) == (1, 0)  # a keepalive is not data
    assert (m.slots[3]["last"], m.slots[3]["last_data"]) == (T0 + 60_000, 0)
    assert _sweep(m, T0 + 75_000)["summary"][4] == 0
    d[0]["len"] = 64
    assert m.mark(T0 + 80_000, d, [TM.PKT_OK]) == (1, 0)
    assert _sweep(m, T0 + 89_999)["summary"][4] == 0
    out = _sweep(m, T0 + 90_000)
    assert out["summary"][4:6] == [1, 1] and int(out["keepalives"][0]["key_slot"]) == 2
    assert _sweep(m, T0 + 100_000)["summary"][4] == 0  # answered: last >= last_data
    # data answered in the same tick counts as answered
    ds = np.zeros(1, TM.PKT_DTYPE)
    ds[0] = (0, 0, 1, 10, 2)
    m.mark(T0 + 110_000, d, [TM.PKT_OK])
    m.mark(T0 + 110_000, ds, [TM.PKT_OK], tx=True)
    assert _sweep(m, T0 + 125_000, cap_init=0)["summary"][4] == 0


def test_wireguard_expiry_at_180_s():
    m = _one(TM.wireguard(1000))
    m.peers[0]["rekey_listed"] = T0 + 179_000  # (keeps the rekey list out of the picture)
    assert _sweep(m, T0 + 179_999, retire=True)["summary"][:2] == [0, 0]
    d = np.zeros(2, TM.PKT_DTYPE)
    d["key_slot"], d["len"] = 2, 5
    st = [TM.PKT_OK, TM.PKT_OK]
    assert m.mark(T0 + 179_999, d, st, tx=True, gate=True, slot_first=0, slot_count=8) == (2, 0)
    assert m.mark(T0 + 180_000, d, st, tx=True, gate=True, slot_first=0, slot_count=8) == (0, 2)  # the gate stops it at the packet
    assert st == [TM.PKT_NOSESSION] * 2 and d["len"].tolist() == [TM.LEN_INVALID] * 2
    out = _sweep(m, T0 + 180_000)  # without RETIRE: listed, at every sweep
    assert out["summary"][:2] == [1, 1] and out["expired"][0].tolist() == (2, 3, 0, 0x51) and m.slots[2]["state"] == TM.SEND_INITIATOR
    out = _sweep(m, T0 + 180_001, retire=True)
    assert out["summary"][:2] == [1, 1] and out["summary"][6] == 0
    assert (m.slots[2]["state"], m.slots[3]["state"], m.peers[0]["current"]) == (TM.DEAD, TM.DEAD, TM.NOSLOT)
    assert m.table == {} and m.retired == 1
    assert _sweep(m, T0 + 180_002, retire=True)["summary"][:2] == [0, 0]
    # the peer lost its session: listed although we were ... the initiator or not
    m2 = _one(TM.wireguard(1000), source=TM.SRC_SESSIONS)
    assert _listed(_sweep(m2, T0 + 180_000, retire=True)) == [0]


def test_superseded_sessions_linger():
    for linger in (0, 7_000):
        cfg = TM.wireguard(1000)
        cfg.linger = linger
        m = _one(cfg)
        m.start(T0 + 1_000, [(TM.INST_OK, 0, 0, 0x52)], [4], [5], TM.SRC_ESTABLISHED, install=True)
        assert m.peers[0]["current"] == 4 and m.slots[2]["superseded"] == T0 + 1_000 and m.slots[4]["superseded"] == 0
        assert _sweep(m, T0 + 1_000 + 6_999)["summary"][0] == 0
        assert _sweep(m, T0 + 1_000 + 7_000)["summary"][0] == (1 if linger else 0)


def test_marks_of_one_tick_commute():
    rng = random.Random(7)
    marks = []
    for k in range(40):
        d = np.zeros(3, TM.PKT_DTYPE)
        d["key_slot"] = [rng.randrange(0, 10) for _ in range(3)]
        d["len"] = [rng.choice([0, 1, 1400]) for _ in range(3)]
        marks.append((T0 + rng.choice([5, 9, 9, 20]), d, [rng.choice([0, 0, 3, 1, 6]) for _ in range(3)], bool(k & 1)))

    def run(order):
        m = TM.Timers(8, 2, TM.wireguard(1000))
        m.peers_set(0, [(0, True), (3, True)])
        m.start(T0, [(0, 0, 0, 1), (0, 1, 1, 2)], [0, 4], [1, 5], TM.SRC_ESTABLISHED, install=True)
        for k in order:
            now, d, st, tx = marks[k]
            m.mark(now, d.copy(), list(st), tx=tx)
        return m.slots_image().tobytes(), m.peers_image().tobytes()

    want = run(range(40))
    for seed in range(5):
        order = list(range(40))
        random.Random(seed).shuffle(order)
        assert run(order) == want


def test_carry_over_past_each_capacity():
    cfg = TM.Config(reject_after_time=100, rekey_timeout=50)
    m = TM.Timers(16, 5, cfg)
    m.peers_set(0, [(10, True)] * 5)
    # peers 0..2: sessions that expire at T0 + 100; peers 3, 4: none. Keepalives due at once for 0..2.
    m.start(T0, [(0, p, p, 0x60 + p) for p in range(3)], [0, 2, 4], [1, 3, 5], TM.SRC_ESTABLISHED, install=True)
    out = _sweep(m, T0 + 1, cap_keep=2, cap_init=1)
    assert out["summary"] == [0, 0, 2, 1, 3, 2, 3, 0] and _listed(out) == [3]
    assert [int(k) for k in out["keepalives"]["key_slot"]] == [0, 2] and m.send[:5] == [1, 0, 1, 0, 0]
    out = _sweep(m, T0 + 2, cap_keep=2, cap_init=1)  # what did not fit stayed due, and only that
    assert out["summary"] == [0, 0, 1, 1, 1, 1, 3, 0] and _listed(out) == [4] and int(out["keepalives"][0]["key_slot"]) == 4
    # a ring with room for one wire slot only
    m.slots[0]["last"] = m.slots[2]["last"] = 0
    assert _sweep(m, T0 + 3, cap_init=0, wire_stride=32, out_size=63)["summary"][4:6] == [2, 1]
    assert _sweep(m, T0 + 3, cap_init=0, wire_stride=31, out_size=640)["summary"][4:6] == [1, 0]
    out = _sweep(m, T0 + 100, cap_exp=2, cap_init=0, retire=True)
    assert out["summary"][:2] == [3, 2] and out["expired"]["send_slot"].tolist() == [0, 2] and out["summary"][6] == 1
    out = _sweep(m, T0 + 100, cap_exp=2, cap_init=0, retire=True)
    assert out["summary"][:2] == [1, 1] and out["expired"]["send_slot"].tolist() == [4] and out["summary"][6] == 0


def test_now_zero_and_a_clock_stepping_back():
    m = _one(TM.wireguard(1000), interval=10)
    before = (m.slots_image().tobytes(), m.peers_image().tobytes(), list(m.send))
    out = _sweep(m, 0)
    assert out["summary"] == [0] * 8 and out["initiate"] == [0xFFFFFFFF] * 4 and len(out["expired"]) == 0
    d = np.zeros(1, TM.PKT_DTYPE)
    d[0] = (0, 0, 0, 9, 3)
    st = [TM.PKT_OK]
    assert m.mark(0, d, st) == (0, 0)
    m.start(0, [(0, 0, 0, 0x99)], [6], [7], TM.SRC_ESTABLISHED)
    assert (m.slots_image().tobytes(), m.peers_image().tobytes(), list(m.send)) == before
    # a clock behind the session's birth ages nothing: no expiry, no rekey, no refusal; and a mark does not lower a stamp
    m.mark(T0 + 500, d, st)
    m.slots[2]["last"] = T0 + 400
    assert m.mark(T0 - 999_000, d, st) == (1, 0) and m.slots[3]["last"] == T0 + 500
    out = _sweep(m, T0 - 999_000, retire=True)
    assert out["summary"] == [0, 0, 0, 0, 0, 0, 1, 0]
    ds = np.zeros(1, TM.PKT_DTYPE)
    ds[0] = (0, 0, 5, 9, 2)
    assert m.mark(T0 - 999_000, ds, [TM.PKT_OK], tx=True, gate=True, slot_first=2, slot_count=1) == (1, 0)


def test_start_kills_the_owner_of_a_reused_slot_and_picks_the_lowest_entry():
    m = TM.Timers(12, 2, TM.wireguard(1000))
    m.peers_set(0, [(0, True), (0, True)])
    m.start(T0, [(0, 0, 0, 0x10), (0, 1, 1, 0x11)], [0, 2], [1, 3], TM.SRC_SESSIONS, install=True)
    assert [p["current"] for p in m.peers] == [0, 2]
    # entry 0 is refused by the install; 1 and 2 are both peer 0's (1 wins); 3 takes peer 1's recv slot; 4 has no peer
    ent = [(2, 0, 0, 0x20), (0, 1, 0, 0x21), (0, 2, 0, 0x22), (0, 3, 0, 0x23), (0, 4, 7, 0x24)]
    m.start(T0 + 5, ent, [9, 4, 6, 8, 10], [9, 5, 7, 3, 11], TM.SRC_ESTABLISHED, install=True)
    assert m.peers[0]["current"] == 4 and m.slots[0]["superseded"] == T0 + 5
    assert m.slots[6]["superseded"] == T0 + 5 and m.slots[8]["superseded"] == T0 + 5 and m.slots[4]["superseded"] == 0
    assert m.slots[2]["state"] == TM.DEAD and m.peers[1]["current"] == TM.NOSLOT and m.slots[3]["partner"] == 8
    assert m.slots[9]["state"] == TM.NONE and m.slots[10]["peer"] == TM.NOPEER and m.slots[10]["superseded"] == 0
    assert m.slots[4]["state"] == TM.SEND_INITIATOR and m.slots[0]["state"] == TM.SEND_RESPONDER
