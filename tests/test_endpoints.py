"""The endpoint rules on tests/endpoints_model.py (no GPU): the reference's (a session's address is fixed when the session
is made), WireGuard's (the last authenticated packet moves it), each call against an independent brute-force
restatement on seeded batches, and the package's struct layouts against the model's."""
import ctypes

import numpy as np
import pytest

import endpoints_cases as EC
import endpoints_model as EM
from wgtest import wg

A1, A2, A3 = EM.src(bytes([192, 0, 2, 1]), 1000), EM.src(bytes([192, 0, 2, 2]), 2000), EM.src(bytes([198, 51, 100, 9]), 3000)


def _pkt(slots, ln=40):
    d = np.zeros(len(slots), EM.PKT_DTYPE)
    d["key_slot"], d["len"], d["out_off"] = slots, ln, [16 + 128 * j for j in range(len(slots))]
    return d


# ---- the reference's rules ------------------------------------------------------------------------------------------
def test_a_responder_session_gets_the_initiations_origin():
    """SessionManager.performHandshakeResponse, SessionManager.java:217-229: the response goes to
    initiation.originAddress() (:229) and the session is made with it."""
    m = EM.Endpoints(8, 2)
    srcs = [A3, A1, A2]
    got = m.start([(EM.INST_OK, 0, 1, 2)], [4], [5], EM.SRC_SESSIONS, srcs)
    assert got == [1, 1, 0, 0] and m.ep == [bytes(24), A2] and m.map[4] == m.map[5] == 1
    items, summary = m.hs_sendlist(EM.SEND_RESPONSES, [(2, 1)], srcs)
    assert items["dst"].tobytes() == A2 and items["off"].tolist() == [16] and summary == (92, 1, 0)
    items, _ = m.tx_sendlist(_pkt([4]), [EM.PKT_OK])
    assert items["dst"].tobytes() == A2 and items["peer"].tolist() == [1]


def test_an_initiator_session_keeps_the_configured_endpoint():
    """SessionManager.performHandshakeInitiation transmits to connectionInfo.endpoint() (SessionManager.java:186) and
    makes the session with it (:196), wherever the response came from."""
    m = EM.Endpoints(8, 1)
    m.endpoints_set(0, [A1])
    items, _ = m.hs_sendlist(EM.SEND_INITIATIONS, [(EM.HS_INIT_OK, 148, 0)])
    assert items["dst"].tobytes() == A1 and items["off"].tolist() == [8] and items["len"].tolist() == [148]
    assert m.start([(EM.INST_OK, 0, 0, 0)], [2], [3], EM.SRC_ESTABLISHED, [A3]) == [1, 0, 0, 0]
    assert m.ep == [A1] and m.map[2:4] == [0, 0]
    # WireGuard's rule for the same entry: the response's source
    assert m.start([(EM.INST_OK, 0, 0, 0)], [2], [3], EM.SRC_ESTABLISHED, [A3], flags=EM.LEARN_RESPONSE) == [1, 1, 0, 0]
    assert m.ep == [A3]


def test_nothing_moves_a_reference_sessions_address():
    """EstablishedSession.outboundPacketAddress is final (EstablishedSession.java:22, set at :50, used at :63): a node
    that keeps the reference's behaviour never calls learn, and no other call writes an endpoint."""
    m = EM.Endpoints(8, 1)
    m.endpoints_set(0, [A1])
    m.slots_set(2, [0, 0])
    before = m.endpoints_image()
    d = _pkt([2, 3, 2])
    m.tx_sendlist(d, [0, 0, 0], gate=True)
    m.hs_sendlist(EM.SEND_COOKIE_REPLIES, [(0, 64)], [A2])
    m.hs_sendlist(EM.SEND_RESPONSES, [(0, 0)], [A2])
    assert m.endpoints_image() == before


# ---- WireGuard's rule ----------------------------------------------------------------------------------------------
def test_the_last_authenticated_packet_wins():
    m = EM.Endpoints(8, 2)
    m.endpoints_set(0, [A1, A1])
    m.slots_set(0, [0, 0, 1])
    d = _pkt([1, 0, 1, 2])
    roamed, summary = m.learn(d, [EM.PKT_OK, EM.PKT_KEEPALIVE, EM.PKT_OK, EM.PKT_OK], [A2, A3, A2, A1], 4)
    assert m.ep == [A2, A1] and roamed == [0] and summary == [4, 2, 1, 0]  # peer 1 heard from its own address


@pytest.mark.parametrize("status", [1, 2, 4, 5, 6, 7, 8, 9, 10, 11])
def test_unauthenticated_replayed_and_filtered_packets_move_nothing(status):
    """BADTAG (1), FILTERED (5), REPLAY (6) and every other status but OK and KEEPALIVE."""
    m = EM.Endpoints(4, 1)
    m.endpoints_set(0, [A1])
    m.slots_set(0, [0])
    roamed, summary = m.learn(_pkt([0, 0]), [EM.PKT_OK, status], [A2, A3], 4)
    assert m.ep == [A2] and roamed == [0] and summary == [1, 1, 1, 0]
    roamed, summary = m.learn(_pkt([0]), [status], [A3], 4)
    assert m.ep == [A2] and roamed == [] and summary == [0, 0, 0, 0]


def test_sources_are_stored_normalised():
    dirty = EM.src(bytes([192, 0, 2, 1]) + bytes([0xEE] * 12), 1000, family=4, pad=bytes([1, 2, 3, 4, 5]))
    assert EM.normalise(dirty) == A1 and EM.normalise(EM.src(bytes(4), 1, family=9)) is None
    m = EM.Endpoints(4, 1)
    m.endpoints_set(0, [dirty])
    m.slots_set(0, [0])
    assert m.ep == [A1]
    assert m.learn(_pkt([0]), [0], [dirty], 1) == ([], [1, 1, 0, 0])  # equal to the clean one: not roamed
    with pytest.raises(ValueError):
        m.endpoints_set(0, [EM.src(bytes(4), 1, family=5)])
    with pytest.raises(IndexError):
        m.endpoints_set(1, [A1])


# ---- brute force: a loop per peer over the batch -----------------------------------------------------------------------
def _brute_learn(m, d, status, srcs, cap):
    ep, roamed, n_peers = list(m.ep), [], 0
    for p in range(m.P):
        mine = [i for i in range(len(d)) if status[i] in (0, 3) and int(d["key_slot"][i]) < m.K and
                m.map[int(d["key_slot"][i])] == p and srcs[i][18] in (4, 6)]
        if mine:
            n_peers += 1
            w = EM.normalise(srcs[max(mine)])
            if w != ep[p]:
                ep[p] = w
                roamed.append(p)
    n_auth = sum(1 for i in range(len(d)) if status[i] in (0, 3) and int(d["key_slot"][i]) < m.K and
                 m.map[int(d["key_slot"][i])] < m.P and srcs[i][18] in (4, 6))
    n_bad = sum(1 for i in range(len(d)) if status[i] in (0, 3) and int(d["key_slot"][i]) < m.K and
                m.map[int(d["key_slot"][i])] < m.P and srcs[i][18] not in (4, 6))
    return ep, roamed[:cap], [n_auth, n_peers, len(roamed), n_bad]


@pytest.mark.parametrize("n, peers", [(1, 70), (64, 70), (513, 1), (513, 70)])
def test_learn_against_brute_force(n, peers):
    m = EC.state()
    d, status = EC.learn_batch(n, 0xE100 + n, peers)
    srcs = EM.src_list(EC.sources(n, 0xE200 + n))
    for cap in (0, 3, 100):
        want_ep, want_roamed, want_sum = _brute_learn(m, d, status, srcs, cap)
        roamed, summary = m.learn(d, status, srcs, cap)
        assert (m.ep, roamed, summary) == (want_ep, want_roamed, want_sum)
        m = EC.state()
    if n == 513:
        assert want_sum[2] > (0 if peers == 1 else 20) and want_sum[3] > 0 and want_sum[0] < n


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("n", [1, 257, 513])
def test_tx_sendlist_against_brute_force(n, gate):
    m = EC.state()
    d, status = EC.descriptors(n, 0xE300 + n)
    d0, s0 = d.copy(), list(status)
    items, summary = m.tx_sendlist(d, status, gate=gate)
    want = []
    for p in range(m.P):  # per peer, then merged back into ring order
        if m.ep[p][18]:
            want += [j for j in range(n) if s0[j] == 0 and d0["len"][j] != EM.LEN_INVALID and int(d0["key_slot"][j]) < m.K and
                     m.map[int(d0["key_slot"][j])] == p]
    want.sort()
    live = [j for j in range(n) if s0[j] == 0 and d0["len"][j] != EM.LEN_INVALID]
    assert items["index"].tolist() == want and summary[1:] == (len(want), len(live) - len(want))
    assert items["off"].tolist() == [int(d0["out_off"][j]) - 16 for j in want]
    assert items["len"].tolist() == [int(d0["len"][j]) + 32 for j in want] and summary[0] == int(items["len"].sum())
    assert [x.tobytes() for x in items["dst"]] == [m.ep[m.map[int(d0["key_slot"][j])]] for j in want]
    refused = sorted(set(live) - set(want)) if gate else []
    for j in range(n):
        assert status[j] == (EM.PKT_NOENDPOINT if j in refused else s0[j])
        assert d["len"][j] == (EM.LEN_INVALID if j in refused else d0["len"][j])
    if n > 1:
        assert want and len(live) > len(want)


@pytest.mark.parametrize("kind", [EM.SEND_RESPONSES, EM.SEND_INITIATIONS, EM.SEND_COOKIE_REPLIES])
def test_hs_sendlist_against_brute_force(kind):
    m = EC.state()
    n = 257
    srcs = EM.src_list(EC.sources(300, 0xE400))
    r = EC._r32(0xE500 + kind, 2 * n)
    if kind == EM.SEND_INITIATIONS:
        ents = [(int(r[2 * k]) % 3, 148, int(r[2 * k + 1]) % 80) for k in range(n)]
        usable = [k for k, (st, ln, p) in enumerate(ents) if st == 0 and p < m.P and m.ep[p][18]]
        there = [k for k, e in enumerate(ents) if e[0] == 0]
    else:
        ents = [(int(r[2 * k]) % 320, 64 if kind == EM.SEND_COOKIE_REPLIES else int(r[2 * k + 1]) % 70) for k in range(n)]
        usable = [k for k, e in enumerate(ents) if e[0] < 300 and srcs[e[0]][18] in (4, 6)]
        there = list(range(n))
    for cover in (None, 100):
        items, summary = m.hs_sendlist(kind, ents, srcs, cover=cover)
        lim = n if cover is None else cover
        want = [k for k in usable if k < lim]
        stride, at = EM.HS_LAYOUT[kind]
        assert items["index"].tolist() == want and items["off"].tolist() == [stride * k + at for k in want]
        assert summary[1:] == (len(want), len([k for k in there if k < lim]) - len(want)) and summary[2] > 0
        assert set(items["key_slot"].tolist()) == {0xFFFFFFFF}


def test_start_against_brute_force():
    n = 300
    r = EC._r32(0xE600, 3 * n)
    srcs = EM.src_list(EC.sources(280, 0xE700))
    ents = [(0 if r[3 * j] % 4 else 1 + int(r[3 * j]) % 3, j if j % 17 else 1000, int(r[3 * j + 1]) % 76, int(r[3 * j + 2]) % 290) for j in range(n)]
    send, recv = [2 * j for j in range(n)], [2 * j + 1 for j in range(n)]
    for source, flags in ((EM.SRC_SESSIONS, 0), (EM.SRC_ESTABLISHED, 0), (EM.SRC_ESTABLISHED, EM.LEARN_RESPONSE)):
        for cover in (None, 200):
            m = EM.Endpoints(2 * n - 20, EC.P)  # the last ten entries' slots are past the key table
            m.endpoints_set(0, EC.endpoints())
            before = list(m.ep)
            got = m.start(ents, send, recv, source, srcs, flags=flags, cover=cover)
            ok = [j for j in range(n if cover is None else cover) if ents[j][0] == 0 and ents[j][1] < n and recv[ents[j][1]] < m.K]
            learn = source == EM.SRC_SESSIONS or flags
            n_learned = n_bad = 0
            for p in range(EC.P):
                mine = [j for j in ok if ents[j][2] == p]
                bad = [j for j in mine if ents[j][3] >= 280 or srcs[ents[j][3]][18] not in (4, 6)]
                if learn and mine and mine[0] not in bad:
                    assert m.ep[p] == EM.normalise(srcs[ents[mine[0]][3]])
                    n_learned += 1
                else:
                    assert m.ep[p] == before[p]
                n_bad += len(bad) if learn else 0
            assert got == [len(ok), n_learned, n_bad, sum(1 for j in ok if ents[j][2] >= EC.P)]
            for j in ok:
                want = ents[j][2] if ents[j][2] < EC.P else EM.NOPEER
                assert m.map[send[ents[j][1]]] == m.map[recv[ents[j][1]]] == want
            assert sum(1 for x in m.map if x != EM.NOPEER) <= 2 * len(ok)


# ---- struct layouts ---------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_models_dtypes():
    W = wg()
    L = W._lib
    for struct, dtype, size in ((L.WgHsSrc, EM.SRC_DTYPE, 24), (L.WgTxItem, EM.ITEM_DTYPE, 48), (L.WgEndpointsStartSummary, EM.START_SUMMARY, 16),
                                (L.WgEndpointsLearnSummary, EM.LEARN_SUMMARY, 16), (L.WgTxSendlistSummary, EM.TX_SUMMARY, 16),
                                (L.WgHsSendlistSummary, EM.HS_SUMMARY, 16)):
        assert ctypes.sizeof(struct) == dtype.itemsize == size
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], (struct.__name__, name)
    assert W.WG_TX_ITEM_DTYPE == EM.ITEM_DTYPE and W.WG_HS_SRC_DTYPE == EM.SRC_DTYPE
    assert (L.WG_PKT_NOENDPOINT, L.WG_EP_LEARN_RESPONSE, L.WG_SEND_GATE) == (EM.PKT_NOENDPOINT, EM.LEARN_RESPONSE, EM.SEND_GATE)
    assert (L.WG_HS_SEND_RESPONSES, L.WG_HS_SEND_INITIATIONS, L.WG_HS_SEND_COOKIE_REPLIES) == (0, 1, 2)
    assert ctypes.sizeof(L.WgEndpointsStartBatch) == 80 and ctypes.sizeof(L.WgEndpointsLearnBatch) == 48
    assert ctypes.sizeof(L.WgTxSendlistBatch) == 40 and ctypes.sizeof(L.WgHsSendlistBatch) == 72
