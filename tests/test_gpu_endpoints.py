"""wg_endpoints_start / _learn, wg_tx_sendlist and wg_hs_sendlist on the MI355X against tests/endpoints_model.py (pytest -m
gpu), byte for byte: the items, the roamed lists, the summaries, the gated descriptors and statuses, the guard words
behind every output, and the state read back through wg_endpoints_get / wg_endpoint_slots_get. The closed loop runs a
handshake between two contexts, answers it to the initiation's source, sends on the installed session to the learned
endpoint, and follows the initiator to a new port."""
import ctypes
import struct

import numpy as np
import pytest

import endpoints_cases as EC
import endpoints_model as EM
import hs_install_model as IM
import tx_gpu as TG
import tx_model as TXM
from test_gpu_hs_initiate import GUARD, rig, t_u8, t_u32  # noqa: F401
from test_gpu_hs_install import _InstallLoop, _tun_packet
from test_gpu_timers import _Side
from wgtest import splitmix_np

pytestmark = pytest.mark.gpu

G64 = 0x7E7E7E7E7E7E7E7E
SESS, EST = EM.SRC_SESSIONS, EM.SRC_ESTABLISHED
STRIDE = {SESS: 176, EST: 96}


def t_src(rig, srcs):
    """A SRC_DTYPE array (or list of 24-byte strings) as a uint8 [n, 24] tensor (8-byte aligned: a fresh allocation)."""
    raw = srcs.tobytes() if isinstance(srcs, np.ndarray) else b"".join(srcs)
    n = len(raw) // 24
    return t_u8(rig, raw + bytes(24)).reshape(n + 1, 24)[:n]


def _summary64(t):
    h = t.cpu().numpy()
    return (int(h[0].view(np.uint64)), int(h[1]) & 0xFFFFFFFF, (int(h[1]) >> 32) & 0xFFFFFFFF), [int(x) for x in h[2:].view(np.uint64)]


class Pair:
    """A context and the model side by side: every call goes to both and the outputs are compared at once."""

    def __init__(self, rig, K=EC.K, P=EC.P, populate=True, eng=None):
        self.rig, self.K, self.P = rig, K, P
        self.own = eng is None
        self.eng = eng or rig.W.Engine(0, key_slots=K)
        self.eng.endpoints_reserve(P)
        self.m = EM.Endpoints(K, P)
        if populate:
            self.slots_set(0, EC.slot_map())
            self.endpoints_set(0, EC.endpoints())

    def close(self):
        if self.own:
            self.eng.close()

    def endpoints_set(self, first, eps):
        self.eng.endpoints_set(first, np.frombuffer(b"".join(eps), EM.SRC_DTYPE))
        self.m.endpoints_set(first, eps)

    def slots_set(self, first, peers):
        self.eng.endpoint_slots_set(first, peers)
        self.m.slots_set(first, peers)

    def same(self):
        got, want = self.eng.endpoints_get(0, self.P).tobytes(), self.m.endpoints_image()
        assert got == want, [(p, got[24 * p:24 * p + 24], want[24 * p:24 * p + 24]) for p in range(self.P) if got[24 * p:24 * p + 24] != want[24 * p:24 * p + 24]][:3]
        assert self.eng.endpoint_slots_get(0, self.K).tolist() == self.m.map

    def tx_sendlist(self, desc, status, gate=False):
        torch, dev = self.rig.torch, self.rig.dev
        n = len(desc)
        d_desc = torch.full((n + 1, 4), G64, dtype=torch.int64, device=dev)
        d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device=dev)
        d_items = torch.full((n + 1, 48), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((3,), G64, dtype=torch.int64, device=dev)
        if n:
            d_desc[:n] = torch.from_numpy(self.rig.W.desc_as_int64(desc)).to(dev)
            if status is not None:
                d_st[:n] = t_u32(self.rig, status)
        self.eng.tx_sendlist(d_desc[:n], d_st[:n] if status is not None else None, d_items[:n], d_sum[:2], gate=gate)
        want_d, want_s = desc.copy(), (list(status) if status is not None else None)
        items, summary = self.m.tx_sendlist(want_d, want_s, gate=gate)
        torch.cuda.synchronize()
        assert _summary64(d_sum) == (summary, [G64])
        got = d_items.cpu().numpy().tobytes()
        assert got[:48 * len(items)] == items.tobytes(), [k for k in range(len(items)) if got[48 * k:48 * k + 48] != items[k].tobytes()][:4]
        assert got[48 * len(items):] == b"\x7e" * (48 * (n + 1 - len(items)))
        assert d_desc.cpu().numpy().tobytes() == want_d.tobytes() + struct.pack("<4Q", *[G64] * 4)
        assert d_st.cpu().numpy().view(np.uint32).tolist() == (want_s if status is not None else [GUARD] * n) + [GUARD] * 2
        return items, summary

    def learn(self, desc, status, srcs, cap, extra=2):
        torch, dev = self.rig.torch, self.rig.dev
        n = len(desc)
        d_roam = torch.full((cap + extra,), GUARD, dtype=torch.int32, device=dev)
        d_sum = torch.full((6,), GUARD, dtype=torch.int32, device=dev)
        d_desc = torch.from_numpy(self.rig.W.desc_as_int64(desc)).to(dev) if n else torch.zeros((0, 4), dtype=torch.int64, device=dev)
        self.eng.endpoints_learn(d_desc, t_u32(self.rig, status), t_src(self.rig, srcs), d_roam[:cap], d_sum[:4])
        roamed, summary = self.m.learn(desc, status, srcs, cap)
        torch.cuda.synchronize()
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == summary + [GUARD] * 2
        assert d_roam.cpu().numpy().view(np.uint32).tolist() == roamed + [GUARD] * (cap + extra - len(roamed))
        self.same()
        return roamed, summary

    def entries(self, ents, source, seed=0xE900):
        n = len(ents)
        e = np.frombuffer(splitmix_np(seed + n, STRIDE[source] * n).tobytes(), IM.DTYPES[source]).copy()
        e[IM.POSITION[source]] = [x[1] for x in ents]
        e["peer"] = [x[2] for x in ents]
        e["index"] = [x[3] for x in ents]
        return t_u8(self.rig, e.tobytes()).reshape(n, STRIDE[source])

    def start(self, ents, send, recv, source, srcs, learn_response=False, cover=None):
        torch, dev = self.rig.torch, self.rig.dev
        d_n = None if cover is None else t_u32(self.rig, [cover, 1 << 30])
        d_sum = torch.full((6,), GUARD, dtype=torch.int32, device=dev)
        self.eng.endpoints_start(self.entries(ents, source), d_n, t_u32(self.rig, [x[0] for x in ents]), t_u32(self.rig, send),
                                 t_u32(self.rig, recv), t_src(self.rig, srcs), d_sum[:4], source, learn_response=learn_response)
        want = self.m.start(ents, send, recv, source, srcs, flags=EM.LEARN_RESPONSE if learn_response else 0, cover=cover)
        torch.cuda.synchronize()
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == want + [GUARD] * 2
        self.same()
        return want

    def hs_sendlist(self, kind, ents, srcs, cover=None):
        torch, dev, W = self.rig.torch, self.rig.dev, self.rig.W
        n = len(ents)
        stride = EM.HS_LAYOUT[kind][0]
        dt = {EM.SEND_RESPONSES: W.WG_HS_SESSION_DTYPE, EM.SEND_INITIATIONS: W.WG_HS_RECORD_DTYPE, EM.SEND_COOKIE_REPLIES: W.WG_HS_COOKIE_REPLY_DTYPE}[kind]
        e = np.frombuffer(splitmix_np(0xEA00 + n, stride * max(n, 1)).tobytes(), dt).copy()[:n]
        status = peer = None
        if kind == EM.SEND_INITIATIONS:
            e["len"] = [x[1] for x in ents]
            status, peer = t_u32(self.rig, [x[0] for x in ents] + [0]), t_u32(self.rig, [x[2] for x in ents] + [0])
        elif kind == EM.SEND_RESPONSES:
            e["index"], e["peer"] = [x[0] for x in ents], [x[1] for x in ents]
        else:
            e["index"], e["len"] = [x[0] for x in ents], [x[1] for x in ents]
        d_ent = t_u8(self.rig, e.tobytes() + bytes(stride)).reshape(n + 1, stride)[:n]
        d_items = torch.full((n + 1, 48), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((3,), G64, dtype=torch.int64, device=dev)
        d_n = None if cover is None else t_u32(self.rig, [cover, 1 << 30])
        self.eng.hs_sendlist(kind, d_ent, d_n, d_items[:n], d_sum[:2], src=t_src(self.rig, srcs) if kind != EM.SEND_INITIATIONS else None,
                             status=status, peer=peer)
        items, summary = self.m.hs_sendlist(kind, ents, srcs, cover=cover)
        torch.cuda.synchronize()
        assert _summary64(d_sum) == (summary, [G64])
        got = d_items.cpu().numpy().tobytes()
        assert got[:48 * len(items)] == items.tobytes(), [k for k in range(len(items)) if got[48 * k:48 * k + 48] != items[k].tobytes()][:4]
        assert got[48 * len(items):] == b"\x7e" * (48 * (n + 1 - len(items)))
        return items, summary


@pytest.fixture(scope="module")
def pair(rig):
    p = Pair(rig)
    yield p
    p.close()


# ---- 1. wg_tx_sendlist ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_tx_sendlist_against_the_model(pair, n, gate):
    desc, status = EC.descriptors(n, 0xE300 + n)
    items, summary = pair.tx_sendlist(desc, status, gate=gate)
    if n >= 255:  # the ring meets every case: listed in both families, no endpoint, no peer, a peer past max_peers, past the key table
        fam = {int(x) for x in items["dst"]["family"]}
        assert fam == {4, 6} and summary[2] > 0 and len({int(p) for p in items["peer"]}) > 40
        live = [j for j in range(n) if status[j] == 0 and desc["len"][j] != EM.LEN_INVALID]
        slots = {int(desc["key_slot"][j]) for j in live}
        assert any(s >= EC.K for s in slots) and any(140 <= s < EC.K for s in slots) and any(s % 75 >= 70 for s in slots if s < 140)
        assert any(desc["len"][j] == 0 for j in live) and set(status) == set(range(12))
    pair.same()


@pytest.mark.parametrize("gate", [False, True])
def test_tx_sendlist_over_a_padded_keepalive_list_without_statuses(pair, gate):
    desc, status = EC.descriptors(257, 0xE380, sweep_style=True)
    assert status is None
    items, summary = pair.tx_sendlist(desc, None, gate=gate)
    assert set(items["len"].tolist()) == {32} and 0 < summary[1] < 171 and summary[1] + summary[2] == 171


# ---- 2. wg_endpoints_learn ---------------------------------------------------------------------------------------------------
def test_learn_513_packets_of_one_peer(rig):
    p = Pair(rig)
    try:
        n = 513
        desc, status = EC.learn_batch(n, 0xE100 + n, 1)
        srcs = EC.sources(n, 0xE200 + n)
        roamed, summary = p.learn(desc, status, srcs, 4)
        win = max(i for i in range(n) if status[i] in (0, 3) and srcs[i]["family"] in (4, 6))
        assert roamed == [5] and summary[1:3] == [1, 1] and p.m.ep[5] == EM.normalise(srcs[win].tobytes()) and win >= 510
        assert p.learn(desc, status, srcs, 4) == ([], [summary[0], 1, 0, summary[3]])  # the same ring again: nobody roams
    finally:
        p.close()


@pytest.mark.parametrize("cap", [0, 5, 80])
def test_learn_513_packets_of_70_peers(rig, cap):
    p = Pair(rig)
    try:
        n = 513
        desc, status = EC.learn_batch(n, 0xE100 + n, 70)
        srcs = EC.sources(n, 0xE200 + n)
        probe = EC.state()
        probe.learn(desc, status, srcs, 0)  # every third peer already sits at the address it will be heard from, in clean form
        stay = [q for q in range(0, EC.P, 3)]
        for q in stay:
            p.endpoints_set(q, [probe.ep[q]])
        roamed, summary = p.learn(desc, status, srcs, cap)
        assert summary[1] > 60 and 30 < summary[2] <= summary[1] - 20 and summary[3] > 0 and len(roamed) == min(cap, summary[2])
        assert not set(roamed) & set(stay)
        dirty = [i for i in range(n) if srcs[i]["_pad"].any()]
        assert any(p.m.ep[q] == EM.normalise(srcs[i].tobytes()) for q in stay for i in dirty)  # a garbage source equal to a clean endpoint
    finally:
        p.close()


def test_learn_of_nothing_writes_a_zero_summary(pair):
    assert pair.learn(np.zeros(0, EM.PKT_DTYPE), [], [], 3) == ([], [0, 0, 0, 0])


# ---- 3. wg_endpoints_start ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source, learn_response", [(SESS, False), (EST, False), (EST, True)])
def test_start_against_the_model(rig, source, learn_response):
    n = 300
    r = EC._r32(0xE600, 3 * n)
    srcs = EC.sources(280, 0xE700)
    # refused install statuses, positions past n_slots, peers at and past max_peers, indices past n_src
    ents = [(0 if r[3 * j] % 4 else 1 + (int(r[3 * j]) >> 2) % 4, j if j % 17 else 1000, int(r[3 * j + 1]) % 76, int(r[3 * j + 2]) % 290) for j in range(n)]
    ents[1] = (0, 1, 9, 0)
    ents[2] = (0, 2, 9, 1)  # two OK entries of peer 9: the lower gives the endpoint
    send, recv = [2 * j for j in range(n)], [2 * j + 1 for j in range(n)]
    for cover in (None, 200):
        p = Pair(rig, K=2 * n - 20, populate=False)  # the last ten entries' slots are past the key table
        try:
            p.endpoints_set(0, EC.endpoints())
            got = p.start(ents, send, recv, source, srcs, learn_response=learn_response, cover=cover)
            learn = source == SESS or learn_response
            assert got[0] > 100 and got[3] > 5 and (got[1] > 40 and got[2] > 5 if learn else got[1:3] == [0, 0])
            assert p.m.ep[9] == (EM.normalise(srcs[0].tobytes()) if learn else EC.endpoints()[9])
        finally:
            p.close()


# ---- 4. wg_hs_sendlist -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("kind", [EM.SEND_RESPONSES, EM.SEND_INITIATIONS, EM.SEND_COOKIE_REPLIES])
def test_hs_sendlist_against_the_model(pair, kind, n):
    srcs = EC.sources(300, 0xE400)
    r = EC._r32(0xE500 + kind, 2 * max(n, 1))
    if kind == EM.SEND_INITIATIONS:  # statuses 0 .. 2, peers without an endpoint and past max_peers (and 0xFFFFFFFF)
        ents = [(int(r[2 * k]) % 3, 148 if k % 2 else 92, int(r[2 * k + 1]) % 80 if k % 19 else EM.NOPEER) for k in range(n)]
    else:  # indices past n_src, and on the family-0 and family-9 sources
        ents = [(int(r[2 * k]) % 320 if k % 9 else 7 + 12 * (k % 2), 64 if kind == EM.SEND_COOKIE_REPLIES else int(r[2 * k + 1]) % 70) for k in range(n)]
    if n == 1:
        ents = [(0, 148, 0)] if kind == EM.SEND_INITIATIONS else [(1, ents[0][1])]
    for cover in ((None, 100) if n > 100 else (None,)):
        items, summary = pair.hs_sendlist(kind, ents, srcs, cover=cover)
        if n == 1:
            assert summary[1:] == (1, 0)
        if n > 100 and cover is None:
            assert summary[1] > 30 and summary[2] > 5
    pair.same()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=8)
    try:
        lib = eng._lib
        summ = torch.zeros(8, dtype=torch.int32, device=dev)
        desc, st = torch.zeros((4, 4), dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        items = torch.zeros((6, 48), dtype=torch.uint8, device=dev)
        src = torch.zeros((4, 24), dtype=torch.uint8, device=dev)
        ent = torch.zeros((4, 176), dtype=torch.uint8, device=dev)
        roam = torch.zeros(4, dtype=torch.int32, device=dev)
        host = np.zeros(8, EM.SRC_DTYPE)
        send = lambda **kw: Lb.WgTxSendlistBatch(**{**dict(desc=desc.data_ptr(), status=st.data_ptr(), items=items.data_ptr(),  # noqa: E731
                                                            summary=summ.data_ptr(), n=4), **kw})
        hs = lambda **kw: Lb.WgHsSendlistBatch(**{**dict(entries=ent.data_ptr(), src=src.data_ptr(), items=items.data_ptr(),  # noqa: E731
                                                          summary=summ.data_ptr(), n=4, n_src=4), **kw})
        learn = lambda **kw: Lb.WgEndpointsLearnBatch(**{**dict(desc=desc.data_ptr(), final_status=st.data_ptr(), src=src.data_ptr(),  # noqa: E731
                                                                roamed=roam.data_ptr(), summary=summ.data_ptr(), n=4, roamed_cap=4), **kw})
        start = lambda **kw: Lb.WgEndpointsStartBatch(**{**dict(entries=ent.data_ptr(), inst_status=st.data_ptr(), send_slot=roam.data_ptr(),  # noqa: E731
                                                                recv_slot=roam.data_ptr(), src=src.data_ptr(), summary=summ.data_ptr(), n=4,
                                                                n_slots=4, n_src=4), **kw})
        calls = ((lib.wg_tx_sendlist, send), (lib.wg_hs_sendlist, hs), (lib.wg_endpoints_learn, learn), (lib.wg_endpoints_start, start))
        # before the reserve, a capturing stream included
        for fn, mk in calls:
            assert fn(eng.ctx, ctypes.byref(mk()), None) == Lb.WG_EINVAL and "wg_endpoints_reserve" in Lb.last_error()
        for fn in (lib.wg_endpoints_get, lib.wg_endpoints_set, lib.wg_endpoint_slots_get, lib.wg_endpoint_slots_set):
            assert fn(eng.ctx, 0, 1, host.ctypes.data) == Lb.WG_EINVAL
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = lib.wg_tx_sendlist(eng.ctx, ctypes.byref(send()), side.cuda_stream)
            summ.zero_()  # (a capture must hold a node)
        assert rc == Lb.WG_EINVAL
        assert lib.wg_endpoints_reserve(eng.ctx, (1 << 30) + 1) == Lb.WG_E2BIG and lib.wg_endpoints_reserve(None, 1) == Lb.WG_EINVAL
        eng.endpoints_reserve(4)
        eng.endpoints_reserve(3)  # not above the first: a no-op
        assert lib.wg_endpoints_reserve(eng.ctx, 5) == Lb.WG_EINVAL
        # the setters: a bad family changes nothing, ranges
        good = [EC.address(0), EC.address(1)]
        eng.endpoints_set(0, np.frombuffer(b"".join(good), EM.SRC_DTYPE))
        bad = np.frombuffer(EC.address(2) + EM.src(bytes(4), 9, family=5), EM.SRC_DTYPE)
        assert lib.wg_endpoints_set(eng.ctx, 0, 2, bad.ctypes.data) == Lb.WG_EINVAL
        assert eng.endpoints_get(0, 4).tobytes() == b"".join(good) + bytes(48)
        assert lib.wg_endpoints_set(eng.ctx, 3, 2, host.ctypes.data) == Lb.WG_ERANGE
        assert lib.wg_endpoints_get(eng.ctx, 4, 1, host.ctypes.data) == Lb.WG_ERANGE
        assert lib.wg_endpoint_slots_set(eng.ctx, 7, 2, host.ctypes.data) == Lb.WG_ERANGE
        assert lib.wg_endpoint_slots_get(eng.ctx, 8, 1, host.ctypes.data) == Lb.WG_ERANGE
        assert eng.endpoint_slots_get(0, 8).tolist() == [EM.NOPEER] * 8
        # alignment, overlap, flags, sizes
        for kw in (dict(flags=2), dict(summary=None), dict(summary=summ.data_ptr() + 4), dict(desc=None), dict(desc=desc.data_ptr() + 8),
                   dict(status=st.data_ptr() + 2), dict(items=None), dict(items=items.data_ptr() + 8), dict(items=desc.data_ptr()),
                   dict(items=items.data_ptr(), summary=items.data_ptr() + 48), dict(items=desc.data_ptr(), flags=1)):
            assert lib.wg_tx_sendlist(eng.ctx, ctypes.byref(send(**kw)), None) == Lb.WG_EINVAL, kw
        assert lib.wg_tx_sendlist(eng.ctx, ctypes.byref(send(n=(1 << 30) + 1)), None) == Lb.WG_E2BIG
        assert lib.wg_tx_sendlist(eng.ctx, ctypes.byref(send(status=None, flags=1)), None) == Lb.WG_OK  # the gate without statuses
        for kw in (dict(flags=1), dict(kind=3), dict(entries=ent.data_ptr() + 8), dict(src=src.data_ptr() + 4), dict(items=items.data_ptr() + 4),
                   dict(items=ent.data_ptr()), dict(summary=summ.data_ptr() + 4), dict(kind=1), dict(src=None)):
            assert lib.wg_hs_sendlist(eng.ctx, ctypes.byref(hs(**kw)), None) == Lb.WG_EINVAL, kw
        assert lib.wg_hs_sendlist(eng.ctx, ctypes.byref(hs(n=(1 << 30) + 1)), None) == Lb.WG_E2BIG
        for kw in (dict(summary=summ.data_ptr() + 4), dict(desc=desc.data_ptr() + 8), dict(src=src.data_ptr() + 4), dict(roamed=None),
                   dict(roamed=st.data_ptr()), dict(roamed=summ.data_ptr())):
            assert lib.wg_endpoints_learn(eng.ctx, ctypes.byref(learn(**kw)), None) == Lb.WG_EINVAL, kw
        assert lib.wg_endpoints_learn(eng.ctx, ctypes.byref(learn(n=(1 << 30) + 1)), None) == Lb.WG_E2BIG
        for kw in (dict(flags=2), dict(source=2), dict(_reserved=1), dict(summary=None), dict(entries=ent.data_ptr() + 8), dict(src=src.data_ptr() + 4),
                   dict(summary=st.data_ptr())):
            assert lib.wg_endpoints_start(eng.ctx, ctypes.byref(start(**kw)), None) == Lb.WG_EINVAL, kw
        assert lib.wg_endpoints_start(eng.ctx, ctypes.byref(start(n=(1 << 30) + 1)), None) == Lb.WG_E2BIG
        torch.cuda.synchronize()
    finally:
        eng.close()


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------
def test_captured_plan_sendlist_and_seal_replay_and_follow_the_setters():
    """tx_plan -> tx_sendlist(gate) -> seal captured once; wg_endpoints_set between replays moves one peer and removes
    another's endpoint with no re-capture. Listed wire slots hold the oracle's bytes, refused ones their fill."""
    r = TG.open_rig()
    torch, dev, eng = r.torch, r.dev, r.eng
    try:
        peers = [3 + 5 * k for k in range(6)]  # broadcast: six peers, key slot = peers[k], peer position k
        eng.tx_peers_set(peers)
        eng.endpoints_reserve(8)
        m = EM.Endpoints(TG.KEY_SLOTS, 8)
        for k, s in enumerate(peers):
            eng.endpoint_slots_set(s, [k])
            m.slots_set(s, [k])
        eps = [EC.address(k) for k in range(5)] + [bytes(24)]  # peer 5 has none
        eng.endpoints_set(0, np.frombuffer(b"".join(eps), EM.SRC_DTYPE))
        m.endpoints_set(0, eps)
        rng = np.random.default_rng(0xEB00)
        pkts = [rng.bytes(int(ln)) for ln in (64, 64, 64, 64, 64, 64, 200)]  # equal lengths for the captured uniform seal; 200 > max_len: TOOLONG
        ring, off, lens = TG.ring_of(pkts)
        n, nd, stride, max_len = len(pkts), len(pkts) * 6, 160, 128
        out_size = stride * nd
        eng.tx_reserve(n)
        d_ring = torch.from_numpy(ring).to(dev)
        d_off, d_len = torch.from_numpy(off).to(dev), t_u32(r, lens.tolist())
        d_desc = torch.zeros((nd, 4), dtype=torch.int64, device=dev)
        d_st = torch.zeros(nd, dtype=torch.int32, device=dev)
        d_items = torch.zeros((nd + 1, 48), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(2, dtype=torch.int64, device=dev)
        d_out = torch.zeros(out_size, dtype=torch.uint8, device=dev)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            eng.tx_send(d_ring, d_off, d_len, d_desc, d_st, d_out, d_items[:nd], d_sum, stride, max_len, uniform=True)
        send = {}
        for step in range(3):
            if step == 1:  # peer 1 moves
                moved = [EC.address(1, port=40000)]
                eng.endpoints_set(1, np.frombuffer(moved[0], EM.SRC_DTYPE))
                m.endpoints_set(1, moved)
            if step == 2:  # peer 2 loses its endpoint, peer 5 gets one
                eng.endpoints_set(2, [None])
                m.endpoints_set(2, [bytes(24)])
                eng.endpoints_set(5, [("2001:db8::5", 5555)])
                m.endpoints_set(5, [EM.src(bytes([0x20, 1, 0x0D, 0xB8] + [0] * 11 + [5]), 5555)])
            d_out.fill_(TG.FILL)
            d_items.fill_(0x7E)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want_d, want_s, send = TXM.plan(off, lens, ring, TXM.BROADCAST, send, peers=peers, wire_stride=stride, out_size=out_size, max_len=max_len)
            items, summary = m.tx_sendlist(want_d, want_s, gate=True)
            assert d_st.cpu().numpy().view(np.uint32).tolist() == want_s
            TG.same_desc(np.ascontiguousarray(d_desc.cpu().numpy()).view(TXM.WG_PKT).reshape(-1), want_d)
            assert _summary64(d_sum)[0] == summary
            got = d_items.cpu().numpy().tobytes()
            assert got == items.tobytes() + b"\x7e" * (48 * (nd + 1 - len(items)))
            assert d_out.cpu().numpy().tobytes() == TG.oracle_ring(r, want_d, ring, out_size, max_len).tobytes()
            n_ok = 6 * 6  # six packets pass the size checks
            assert summary[1:] == ((n_ok * 5) // 6, n_ok // 6) and want_s.count(EM.PKT_NOENDPOINT) == 6
            if step:
                assert items[items["peer"] == 1]["dst"][0].tobytes() == moved[0]
            assert {int(p) for p in items["peer"]} == ({0, 1, 2, 3, 4} if step < 2 else {0, 1, 3, 4, 5})
            for it in items:  # what a sendmmsg loop reads: the datagram starts with the transport header
                assert d_out[int(it["off"])].item() == 4
    finally:
        eng.close()


# ---- 7. the closed loop ------------------------------------------------------------------------------------------------------
def test_closed_loop_answer_the_origin_send_to_it_and_follow_a_roaming_peer(rig):
    torch, dev, W, L = rig.torch, rig.dev, rig.W, rig.W._lib
    n = 3
    lp = _InstallLoop(rig, n, 16)
    A, B = lp.A, lp.B
    try:
        for eng in (A, B):
            eng.rx_sessions_reserve(8)
            eng.replay_enable(128)
            eng.endpoints_reserve(1)
        a_addr = [EM.src(bytes([203, 0, 113, 7]) + bytes([0xCC] * 12), 40001 + k, family=4, pad=bytes([9] * 5)) for k in range(n)]
        b_addr = EM.src(bytes([198, 51, 100, 1]), 51820)
        A.endpoints_set(0, [("198.51.100.1", 51820)])  # Endpoint = on the initiator; the responder has none configured
        a_recv, b_recv = (torch.zeros(16, dtype=torch.int32, device=dev) for _ in range(2))
        A.set_receivers(a_recv)
        B.set_receivers(b_recv)
        lp.initiate_and_respond(7)
        items, s64, s32 = torch.zeros((8, 48), dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        as_items = lambda k: np.ascontiguousarray(items.cpu().numpy()[:k]).reshape(-1).view(EM.ITEM_DTYPE)  # noqa: E731
        # the initiations go to the configured endpoint
        A.hs_sendlist(L.WG_HS_SEND_INITIATIONS, lp.a_rec, lp.a_sum, items[:n], s64, status=lp.a_st, peer=lp.peer)
        torch.cuda.synchronize()
        got = as_items(n)
        assert _summary64(s64)[0] == (148 * n, n, 0) and got["off"].tolist() == [160 * k + 8 for k in range(n)]
        assert all(x.tobytes() == b_addr for x in got["dst"]) and got["len"].tolist() == [148] * n
        # the responses go to the initiations' sources (by batch index: sessions[j].index)
        d_src = t_src(rig, a_addr)
        B.hs_sendlist(L.WG_HS_SEND_RESPONSES, lp.b_sess, lp.b_rsum, items[:n], s64, src=d_src)
        torch.cuda.synchronize()
        got = as_items(n)
        sess = lp.b_sess.cpu().numpy().reshape(-1).view(W.WG_HS_SESSION_DTYPE)
        assert got["off"].tolist() == [176 * k + 16 for k in range(n)] and got["len"].tolist() == [92] * n
        assert [x.tobytes() for x in got["dst"]] == [EM.normalise(a_addr[int(i)]) for i in sess["index"]]
        lp.check_and_finish()
        send, recv = t_u32(rig, [2 * p for p in range(n)]), t_u32(rig, [2 * p + 1 for p in range(n)])
        i_st, i_sum = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        A.hs_install(lp.f_est, lp.f_sum, send, recv, i_st, i_sum, 0, 16, L.WG_HS_INSTALL_ESTABLISHED, receivers=a_recv)
        A.endpoints_start(lp.f_est, lp.f_sum, i_st, send, recv, None, s32, L.WG_HS_INSTALL_ESTABLISHED)
        torch.cuda.synchronize()
        assert s32.cpu().numpy().tolist() == [n, 0, 0, 0] and A.endpoints_get(0, 1).tobytes() == b_addr
        B.hs_install(lp.b_sess, lp.b_rsum, send, recv, i_st, i_sum, 0, 16, L.WG_HS_INSTALL_SESSIONS, receivers=b_recv)
        B.endpoints_start(lp.b_sess, lp.b_rsum, i_st, send, recv, d_src, s32, L.WG_HS_INSTALL_SESSIONS)
        torch.cuda.synchronize()
        assert s32.cpu().numpy().tolist() == [n, 1, 0, 0]  # three sessions of one peer: the lowest entry gives the endpoint
        assert B.endpoints_get(0, 1).tobytes() == EM.normalise(a_addr[int(sess["index"][0])])
        assert A.endpoint_slots_get(0, 8).tolist() == [0] * (2 * n) + [EM.NOPEER] * (8 - 2 * n) == B.endpoint_slots_get(0, 8).tolist()

        stride, max_len = 144, 100
        side = {id(A): _Side(rig, 4), id(B): _Side(rig, 4)}
        wire = torch.zeros(stride * 4, dtype=torch.uint8, device=dev)

        def tx_send(eng, pkts, slot):
            """eng routes the tun packets to `slot` and sends them: the items of its send list."""
            m, s = len(pkts), side[id(eng)]
            eng.routes_set([("10.1.0.0", 32, slot)])
            tun = np.zeros(128 * m, np.uint8)
            for k, pk in enumerate(pkts):
                tun[128 * k:128 * k + len(pk)] = np.frombuffer(pk, np.uint8)
            wire.zero_()
            eng.tx_send(torch.from_numpy(tun).to(dev), torch.arange(0, 128 * m, 128, dtype=torch.int64, device=dev), t_u32(rig, [len(pk) for pk in pkts]),
                        s.desc[:m], s.st[:m], wire, items[:m], s64, stride, max_len, route=True)
            torch.cuda.synchronize()
            assert not s.st[:m].cpu().numpy().any() and _summary64(s64)[0] == (sum(len(pk) + 32 for pk in pkts), m, 0)
            got = as_items(m)
            assert got["off"].tolist() == [stride * k for k in range(m)] and got["len"].tolist() == [len(pk) + 32 for pk in pkts]
            assert got["key_slot"].tolist() == [slot] * m and got["peer"].tolist() == [0] * m and got["index"].tolist() == list(range(m))
            return got

        def rx(eng, lens, srcs):
            """eng receives `wire` from `srcs`: rx chain -> endpoints_learn. Returns (final statuses, roamed, summary)."""
            m, s = len(lens), side[id(eng)]
            roam = torch.full((3,), GUARD, dtype=torch.int32, device=dev)
            eng.rx_plan(wire, torch.arange(0, stride * m, stride, dtype=torch.int64, device=dev), t_u32(rig, lens), s.desc[:m], s.st[:m], s.host[:m],
                        s.sum, max_len, packed=True, pt_size=s.pt.numel())
            eng.open(s.desc[:m], wire, s.pt, s.ost[:m], max_len, rx_filter=True)
            eng.rx_check(s.desc[:m], s.pt, s.ost[:m], L.WG_RX_REPLAY)
            eng.rx_deliver(s.desc[:m], s.st[:m], s.ost[:m], s.fst[:m], s.items[:m], s.deliv)
            eng.endpoints_learn(s.desc[:m], s.fst[:m], t_src(rig, srcs), roam[:2], s32)
            torch.cuda.synchronize()
            return s.fst[:m].cpu().numpy().tolist(), roam.cpu().numpy().view(np.uint32).tolist(), s32.cpu().numpy().tolist()

        pkts = [_tun_packet(0, k, 60 + k) for k in range(2)]
        # the responder sends on its first session: the items name the initiator's source
        got = tx_send(B, pkts, 0)
        assert all(x.tobytes() == EM.normalise(a_addr[int(sess["index"][0])]) for x in got["dst"])
        assert rx(A, [len(pk) + 32 for pk in pkts], [b_addr] * 2) == ([0, 0], [GUARD] * 3, [2, 1, 0, 0])  # from the configured address: no roam
        # the initiator sends from a new port: the responder follows it
        tx_send(A, pkts, 0)
        new = EM.src(bytes([203, 0, 113, 7]), 50505)
        third = EM.src(bytes([192, 0, 2, 66]), 6666)
        assert rx(B, [len(pk) + 32 for pk in pkts], [third, new]) == ([0, 0], [0, GUARD, GUARD], [2, 1, 1, 0])
        assert B.endpoints_get(0, 1).tobytes() == new
        got = tx_send(B, pkts, 0)
        assert all(x.tobytes() == new for x in got["dst"])
        # a forged transport packet from a third address moves nothing
        tx_send(A, pkts[:1], 0)
        wire[16 + 5] ^= 1
        fst, roamed, summ = rx(B, [len(pkts[0]) + 32], [third])
        assert fst == [L.WG_PKT_BADTAG] and roamed == [GUARD] * 3 and summ == [0, 0, 0, 0] and B.endpoints_get(0, 1).tobytes() == new
    finally:
        lp.close()


# ---- 8. untouched paths --------------------------------------------------------------------------------------------------------
def test_a_context_that_reserves_endpoints_plans_and_seals_the_same_bytes(rig):
    torch, dev = rig.torch, rig.dev
    outs = []
    for with_ep in (False, True):
        eng = rig.W.Engine(0, key_slots=16)
        try:
            if with_ep:
                eng.endpoints_reserve(4)
            eng.set_keys(0, splitmix_np(0xEC00, 32 * 16))
            eng.set_receivers(torch.arange(16, dtype=torch.int32, device=dev))
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
            outs.append((desc.cpu().numpy().tobytes(), st.cpu().numpy().tobytes(), wire.cpu().numpy().tobytes(), eng.tx_counters_get(0, 16).tobytes()))
        finally:
            eng.close()
    assert outs[0] == outs[1]
