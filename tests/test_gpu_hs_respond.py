"""wg_hs_respond on the MI355X against tests/hs_respond_model.py (pytest -m gpu): statuses, sessions, summaries and
the ephemerals after the call are compared exactly, and every output array carries guard bytes or words behind what
the call may write. Entries come from test_gpu_hs_open's pool of 24 (ephemeral, initiator) pairs and the responder's
ephemerals from a pool of 8, so the memoised ladder model of test_gpu_x25519 stays at a few hundred operands."""
import ctypes
import functools

import numpy as np
import pytest

import hs_model as HM
import hs_open_model as OM
import hs_respond_model as RM
import x25519_model as M
from test_gpu_hs_open import EPHK, INITK, _hello, _OpenChain, _open_ring, _peers, _pub
from test_gpu_x25519 import FILL, GUARD, LOW, STATIC, STATIC2, _engine, _Memo
from wgtest import noise, oracle, splitmix_np, wg

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 21, 22, 63, 64, 65, 86, 255, 256, 257]  # a wave, the 256 entries of one partial, 3 n across a wave
REPH = [bytes(splitmix_np(0x6300 + j, 32)) for j in range(8)]  # the responder's ephemeral private keys
LATE = bytes([7]) + bytes(31)                                   # the all-zero scalar only after clamping


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    yield type("Rig", (), dict(eng=None, torch=torch, dev=torch.device("cuda", 0), W=wg()))


@functools.lru_cache(maxsize=None)
def _opened(responder, k):
    """Pool entry k's initiation as wg_hs_open leaves it (hs_open_model), for the responder with this key."""
    h = _hello(responder, k)
    with _Memo():
        st, res = OM.open_one(responder, _pub(responder), h["ephemeral"], h["encrypted_static"], h["encrypted_timestamp"],
                              M.x25519(responder, h["ephemeral"]), _peers())
    assert st in (OM.OPEN_OK, OM.OPEN_NEWPEER)
    return res


_respond_one = functools.lru_cache(maxsize=None)(RM.respond_one)


class _MemoResp(_Memo):
    """... and hs_respond_model's respond_one memoised on its arguments: the runs of one shape share their entries."""

    def __enter__(self):
        super().__enter__()
        self.keep_r, RM.respond_one = RM.respond_one, _respond_one

    def __exit__(self, *a):
        RM.respond_one = self.keep_r
        super().__exit__(*a)


def _entries(n):
    """n wg_hs_init entries made from the pool: known peers, entries without a peer, and every seventh with a
    low-order remote_ephemeral or remote_static in its place (their secrets are all zero and go through)."""
    ent = np.zeros(n, OM.HS_INIT)
    for k in range(n):
        p = (5 * k + 3) % 24
        res = _opened(STATIC, p)
        ent[k]["index"], ent[k]["record"], ent[k]["sender_index"], ent[k]["peer"] = 3 * k + 1, k, 0x9E3779B9 * (k + 1) & 0xFFFFFFFF, res["peer"]
        ent[k]["remote_ephemeral"] = np.frombuffer(_hello(STATIC, p)["ephemeral"], np.uint8)
        for f in ("remote_static", "hash", "chain_key"):
            ent[k][f] = np.frombuffer(res[f], np.uint8)
        if k % 7 == 3:
            ent[k]["remote_ephemeral" if k % 14 == 3 else "remote_static"] = np.frombuffer(LOW[k % len(LOW)], np.uint8)
    return ent


def _ephemerals(n):
    """32 n bytes: the pool's keys, every fifth all zero, LATE at 2 and 66."""
    out = bytearray()
    for k in range(n):
        out += bytes(32) if k % 5 == 4 else LATE if k in (2, 66) else REPH[k % 8]
    return bytes(out)


def _call(rig2, ent, n_inits, eph, li, flags):
    """One wg_hs_respond over guarded outputs; returns (ephemerals, status list, sessions, summary list) as the device
    holds them, guards included, and the model's."""
    torch, dev, eng = rig2.torch, rig2.dev, rig2.eng
    n = len(ent)
    d_ent = torch.from_numpy(ent.view(np.uint8).reshape(n, 144).copy()).to(dev)
    d_eph = torch.from_numpy(np.frombuffer(eph + bytes([FILL]) * 32, np.uint8).copy()).to(dev)
    d_li = torch.from_numpy(np.array(li, np.uint32).view(np.int32).copy()).to(dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sess = torch.full((n + 1, 176), 0x7E, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    d_osum = torch.from_numpy(np.array([0 if n_inits is None else n_inits, 1 << 30, 1 << 30, 1 << 30], np.int32)).to(dev)
    eng.hs_respond(d_ent, None if n_inits is None else d_osum, d_eph[:32 * n], d_li, d_st[:n], d_sess[:n], d_sum[:4],
                   skip_newpeer=bool(flags))
    torch.cuda.synchronize()
    got = (d_eph.cpu().numpy().tobytes(), d_st.cpu().numpy().view(np.uint32).tolist(), d_sess.cpu().numpy().tobytes(),
           d_sum.cpu().numpy().view(np.uint32).tolist())
    with _MemoResp():
        e2, st, out, sm = RM.respond_batch(ent, n_inits, n, eph + bytes([FILL]) * 32, li, flags, [GUARD] * (n + 4),
                                           b"\x7e" * (176 * (n + 1)), [GUARD] * 4)
    return got, (e2, st, out, sm + [GUARD] * 4)


def _same(got, want, n):
    assert got[1] == want[1], [(k, a, b) for k, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:5]
    assert got[3] == want[3]
    if got[2] != want[2]:
        bad = [j for j in range(n + 1) if got[2][176 * j:176 * j + 176] != want[2][176 * j:176 * j + 176]][:3]
        raise AssertionError(("sessions differ", bad, [np.frombuffer(got[2][176 * j:176 * j + 176], RM.HS_SESSION) for j in bad],
                              [np.frombuffer(want[2][176 * j:176 * j + 176], RM.HS_SESSION) for j in bad]))
    assert got[0] == want[0], [k for k in range(n + 1) if got[0][32 * k:32 * k + 32] != want[0][32 * k:32 * k + 32]][:5]


# ---- direct ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_entries_made_by_hand(rig, n):
    """Both flag settings, with the entry count below, equal to (on the device and as NULL) and above n."""
    eng, rig2 = _engine(rig)
    try:
        eng.hs_static_set(STATIC)
        ent, eph, li = _entries(n), _ephemerals(n), [0x5000 + 17 * k for k in range(n)]
        seen = set()
        for flags, n_inits in [(1, max(n - 3, 0)), (0, n), (1, n + 5), (0, None)]:
            got, want = _call(rig2, ent, n_inits, eph, li, flags)
            _same(got, want, n)
            seen |= {(flags, s) for s in want[1][:n] if s != GUARD}  # (behind the cover: the guard)
        if n >= 22:
            assert seen == {(1, RM.RESP_OK), (1, RM.RESP_NOPEER), (1, RM.RESP_NOEPH), (0, RM.RESP_OK), (0, RM.RESP_NOEPH)}
    finally:
        eng.close()


# ---- the chain ---------------------------------------------------------------------------------------------------
class _RespChain(_OpenChain):
    """plan -> check -> dh -> open -> respond back to back on the current stream; the host reads nothing in between."""

    def __init__(self, rig, n, ring_size):
        super().__init__(rig, n, ring_size)
        torch, dev = rig.torch, rig.dev
        self.r_eph = torch.zeros((n + 1) * 32, dtype=torch.uint8, device=dev)
        self.r_li = torch.zeros(n, dtype=torch.int32, device=dev)
        self.r_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        self.r_sess = torch.full((n + 1, 176), 0x7E, dtype=torch.uint8, device=dev)
        self.r_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)

    def refresh(self, seed):
        """New ephemerals and session indices, in place (what the host does between replays)."""
        torch, n = self.rig.torch, self.n
        self.eph = bytes(splitmix_np(seed, 32 * n)) + bytes([FILL]) * 32
        self.li = [(0x01000000 + seed * 4096 + k) & 0xFFFFFFFF for k in range(n)]
        self.r_eph.copy_(torch.from_numpy(np.frombuffer(self.eph, np.uint8).copy()))
        self.r_li.copy_(torch.from_numpy(np.array(self.li, np.uint32).view(np.int32)))

    def load(self, ring, off, lens):
        super().load(ring, off, lens)
        self.r_st.fill_(GUARD)
        self.r_sess.fill_(0x7E)
        self.r_sum.fill_(GUARD)

    def run(self, with_summary=True):
        super().run(with_summary)
        n = self.n
        self.rig.eng.hs_respond(self.o_init[:n], self.o_sum[:4], self.r_eph[:32 * n], self.r_li, self.r_st[:n], self.r_sess[:n],
                                self.r_sum[:4], skip_newpeer=True)

    def compare_respond(self, pub, private, peers, eph=None):
        """The earlier stages against their models, then the respond's four outputs, whole, against hs_respond_model
        over the model's entries. Returns (covered status list, sessions)."""
        _, inits = self.compare_open(pub, private, peers)
        n = self.n
        ent = np.zeros(n, OM.HS_INIT)
        ent[:len(inits)] = inits
        with _Memo():
            e2, st, out, sm = RM.respond_batch(ent, len(inits), n, self.eph if eph is None else eph, self.li, RM.SKIP_NEWPEER,
                                               [GUARD] * (n + 4), b"\x7e" * (176 * (n + 1)), [GUARD] * 4)
        got = (self.r_eph.cpu().numpy().tobytes(), self.r_st.cpu().numpy().view(np.uint32).tolist(),
               self.r_sess.cpu().numpy().tobytes(), self.r_sum.cpu().numpy().view(np.uint32).tolist())
        _same(got, (e2, st, out, sm + [GUARD] * 4), n)
        return st[:len(inits)], np.frombuffer(out[:176 * sm[0]], RM.HS_SESSION), inits


def _initiator_of(responder):
    """remote_ephemeral -> (pool entry, its initiation) for the pool's genuine initiations."""
    return {_hello(responder, k)["ephemeral"]: (k, _hello(responder, k)) for k in range(24)}


@pytest.mark.parametrize("n_list", [65, 257])
def test_plan_check_dh_open_respond_on_one_stream(rig, n_list):
    torch, dev = rig.torch, rig.dev
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = _peers()
        eng.hs_peers_set(peers)
        rng = np.random.default_rng(6400 + n_list)
        ring, off, lens = _open_ring(rng, n_list, STATIC)
        ch = _RespChain(rig2, len(off) + 5, len(ring) + 64)
        ch.refresh(n_list)
        ch.load(ring, off, lens)
        ch.run()
        st, sess, inits = ch.compare_respond(pub, STATIC, peers)
        assert set(st) == {RM.RESP_OK, RM.RESP_NOPEER} and len(sess) >= 5
        # every response on the matching pool initiator: it verifies exactly when the responder hashed what the
        # initiator sent (a flipped timestamp bit passes the open and changes the hash)
        pool = _initiator_of(STATIC)
        by_peer, agreed = {p: [] for p in range(4)}, 0
        for s in sess:
            e = inits[int(s["init"])]
            resp = s["response"].tobytes()
            assert int(s["peer"]) == int(e["peer"]) < 4 and int(s["remote_index"]) == int(e["sender_index"])
            by_peer[int(s["peer"])].append(resp)
            hit = pool.get(e["remote_ephemeral"].tobytes())
            if hit is None:  # a low-order ephemeral: nobody holds its private key
                continue
            k, hello = hit
            with _Memo():
                keys = RM.consume_response(INITK[k % 6], EPHK[k], hello["hash"], hello["chain_key"], resp[12:44], resp[44:60])
            if e["hash"].tobytes() == hello["hash"]:
                assert keys is not None and keys["recv_key"] == s["send_key"].tobytes() and keys["send_key"] == s["recv_key"].tobytes()
                agreed += 1
            else:
                assert keys is None
        assert agreed >= 3
        # the responses as a ring, checked under each initiator's public key
        for p, resps in by_peer.items():
            if not resps:
                continue
            m = len(resps)
            wire = torch.from_numpy(np.frombuffer(b"".join(resps), np.uint8).copy()).to(dev)
            w_off = torch.arange(0, 92 * m, 92, dtype=torch.int64, device=dev)
            w_len = torch.full((m,), 92, dtype=torch.int32, device=dev)
            h_st = torch.full((m,), GUARD, dtype=torch.int32, device=dev)
            h_rec = torch.zeros((m, 160), dtype=torch.uint8, device=dev)
            h_sum = torch.zeros(4, dtype=torch.int32, device=dev)
            eng.hs_key_set(peers[p])
            eng.hs_check(wire, w_off, w_len, h_st, h_rec, h_sum)
            torch.cuda.synchronize()
            assert (h_st.cpu().numpy() == HM.HS_OK).all() and h_sum.cpu().numpy().tolist() == [m, 0, m, 0]
            rec = h_rec.cpu().numpy().view(HM.HS_RECORD).reshape(-1)
            assert (rec["len"] == 92).all() and rec["msg"][:, :92].tobytes() == b"".join(resps)
    finally:
        eng.close()


# ---- transport ---------------------------------------------------------------------------------------------------
def test_transport_round_trip_under_the_session_keys(rig):
    """A session's keys installed with set_keys: packets sealed on the device under send_key open with the oracle
    under the initiator's receive key, and the initiator's packets open on the device under recv_key."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    O = oracle()
    eng, rig2 = _engine(rig)
    try:
        eng.hs_static_set(STATIC)
        k = 8  # initiator 2, a peer
        hello, res = _hello(STATIC, k), _opened(STATIC, k)
        ent = np.zeros(1, OM.HS_INIT)
        ent[0]["sender_index"], ent[0]["peer"] = 0x31323334, res["peer"]
        ent[0]["remote_ephemeral"] = np.frombuffer(hello["ephemeral"], np.uint8)
        for f in ("remote_static", "hash", "chain_key"):
            ent[0][f] = np.frombuffer(res[f], np.uint8)
        st, sess = eng.hs_respond_host(ent[0], REPH[1], 0x41424344)
        assert st == RM.RESP_OK and sess is not None
        resp = sess["response"].tobytes()
        with _Memo():
            keys = RM.consume_response(INITK[k % 6], EPHK[k], hello["hash"], hello["chain_key"], resp[12:44], resp[44:60])
        assert keys is not None
        eng.set_keys(2, sess["send_key"].tobytes())
        eng.set_keys(3, sess["recv_key"].tobytes())
        lens = np.array([1, 16, 64, 100], np.uint32)
        at = 128 * np.arange(4, dtype=np.uint64)
        ctr = np.array([0, 1, 2, 1 << 33], np.uint64)
        pt = splitmix_np(0x6500, 512)
        d = torch.from_numpy(W.desc_as_int64(W.pack_desc(at, at, ctr, lens, 2))).to(dev)
        ct = torch.zeros(512, dtype=torch.uint8, device=dev)
        eng.seal(d, torch.from_numpy(pt).to(dev), ct, 100)
        torch.cuda.synchronize()
        got = ct.cpu().numpy().tobytes()
        for i in range(4):
            o, ln = int(at[i]), int(lens[i])
            assert O.py_aead_open(keys["recv_key"], O.transport_nonce(int(ctr[i])), got[o:o + ln + 16]) == pt[o:o + ln].tobytes()
        # the other direction
        wire = bytearray(512)
        for i in range(4):
            o, ln = int(at[i]), int(lens[i])
            wire[o:o + ln + 16] = O.py_aead_seal(keys["send_key"], O.transport_nonce(int(ctr[i])), pt[o:o + ln].tobytes())
        wire[int(at[3]) + 5] ^= 1  # ... and one forged packet
        d = torch.from_numpy(W.desc_as_int64(W.pack_desc(at, at, ctr, lens, 3))).to(dev)
        back = torch.zeros(512, dtype=torch.uint8, device=dev)
        ost = torch.full((4,), 7, dtype=torch.int32, device=dev)
        eng.open(d, torch.from_numpy(np.frombuffer(bytes(wire), np.uint8).copy()).to(dev), back, ost, 100)
        torch.cuda.synchronize()
        assert ost.cpu().numpy().tolist() == [0, 0, 0, 1]
        b = back.cpu().numpy()
        for i in range(3):
            o, ln = int(at[i]), int(lens[i])
            assert b[o:o + ln].tobytes() == pt[o:o + ln].tobytes()
    finally:
        eng.close()


# ---- graphs ------------------------------------------------------------------------------------------------------
def test_captured_five_stages_replay(rig):
    """Reserve, then the five stages captured once and replayed with refreshed ephemerals and indices; a replay
    without a refresh answers nothing (the consumed ephemerals are zero); wg_hs_peers_set and wg_hs_static_set
    between the replays need no re-capture. A respond on a capturing stream that needs more scratch than was
    reserved returns WG_EINVAL."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        pub2 = _pub(STATIC2)
        peers = _peers()
        eng.hs_peers_set(peers)
        rng = np.random.default_rng(6600)
        rings = [_open_ring(rng, 70, STATIC), _open_ring(rng, 90, STATIC2)]
        n = max(len(r[1]) for r in rings) + 3
        ch = _RespChain(rig2, n, max(len(r[0]) for r in rings) + 64)
        big = 8 * n  # more than this context reserved
        b_init = torch.zeros((big, 144), dtype=torch.uint8, device=dev)
        b_eph = torch.zeros(32 * big, dtype=torch.uint8, device=dev)
        b_li, b_st = (torch.zeros(big, dtype=torch.int32, device=dev) for _ in range(2))
        b_sess = torch.zeros((big, 176), dtype=torch.uint8, device=dev)
        eng.rx_reserve(n)
        eng.hs_reserve(n)
        ch.refresh(1)
        ch.load(*rings[0])
        ch.run()  # eager once
        ch.compare_respond(pub, STATIC, peers)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                eng.hs_respond(b_init, None, b_eph, b_li, b_st, b_sess, ch.r_sum[4:8])
            ch.run()
        assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
        for replay, (key, p, table) in enumerate([(STATIC, pub, peers), (STATIC2, pub2, peers[:2])]):
            if replay == 1:
                assert eng.hs_static_set(STATIC2) == pub2
                eng.hs_peers_set(table)
            ch.refresh(2 + replay)
            ch.load(*rings[replay])
            torch.cuda.synchronize()
            g.replay()
            st, sess, _ = ch.compare_respond(p, key, table)
            assert st.count(RM.RESP_OK) >= 3 and RM.RESP_NOPEER in st
            # no refresh: the ephemerals the last replay consumed are zero
            after = ch.r_eph.cpu().numpy().tobytes()
            ch.load(*rings[replay])
            torch.cuda.synchronize()
            g.replay()
            st2, sess2, _ = ch.compare_respond(p, key, table, eph=after)
            assert len(sess2) == 0 and RM.RESP_OK not in st2 and st2.count(RM.RESP_NOEPH) == st.count(RM.RESP_OK)
            assert ch.r_sum.cpu().numpy()[0] == 0
    finally:
        eng.close()


# ---- the mirror --------------------------------------------------------------------------------------------------
def test_mirror_responder_handshake(rig):
    """A known and an unknown initiator (the engine of the mirror holds no peer table: the first is made known
    here); the unknown one takes the NEWPEER path, whose chain key the mirror finishes on the host."""
    N, O = noise(), oracle()
    W = rig.W
    local = N.NoisePrivateKey(STATIC)
    eng = W.Engine(0, key_slots=16)
    try:
        for k, known in ((1, True), (4, False)):  # initiators 1 (a peer) and 4 (not one)
            eng.hs_static_set(STATIC)
            eng.hs_peers_set(_peers())
            hello = _hello(STATIC, k)
            with _Memo():
                full = dict(_opened(STATIC, k))
                assert (full["peer"] != OM.NOPEER) == known
                if not known:
                    full["chain_key"] = OM.derive_key(full["chain_key"], M.x25519(STATIC, full["remote_static"]))
                want = RM.respond_one(full["hash"], full["chain_key"], hello["ephemeral"], full["remote_static"], REPH[k], 0x55667788, 0)
                keys = RM.consume_response(INITK[k % 6], EPHK[k], hello["hash"], hello["chain_key"], want["response"][12:44],
                                           want["response"][44:60])
            hs = N.Handshakes.responderHandshake(local, N.NoisePublicKey(hello["ephemeral"]), hello["encrypted_static"],
                                                 hello["encrypted_timestamp"], engine=eng, ephemeral=REPH[k], localIndex=0x55667788)
            assert hs.response == want["response"] and hs.getEncryptedEmpty() == want["encrypted_empty"]
            assert hs.getLocalEphemeral() == N.NoisePublicKey(want["ephemeral_public"])
            assert hs.getRemotePublicKey() == N.NoisePublicKey(_pub(INITK[k % 6]))
            kp = hs.getKeypair()
            sealed = O.py_aead_seal(keys["send_key"], O.transport_nonce(5), b"from the initiator")
            out = bytearray(18)
            kp.decipher(5, sealed, out)
            assert bytes(out) == b"from the initiator"
            dst = bytearray(4 + 16)
            c = kp.cipher(b"pong", dst)
            assert O.py_aead_open(keys["recv_key"], O.transport_nonce(c), bytes(dst)) == b"pong"
            kp.clean()
        # a fresh ephemeral when none is given: two answers to one initiation differ, and the initiator takes both
        hello = _hello(STATIC, 1)
        a, b = (N.Handshakes.responderHandshake(local, N.NoisePublicKey(hello["ephemeral"]), hello["encrypted_static"],
                                                hello["encrypted_timestamp"], engine=eng) for _ in range(2))
        assert a.response[12:44] != b.response[12:44] and a.response[4:8] == bytes(4)
        with pytest.raises(N.BadPaddingException):
            N.Handshakes.responderHandshake(local, N.NoisePublicKey(hello["ephemeral"]), hello["encrypted_static"][:-1] + b"\0",
                                            hello["encrypted_timestamp"], engine=eng)
        a.getKeypair().clean()
        b.getKeypair().clean()
    finally:
        eng.close()


# ---- errors ------------------------------------------------------------------------------------------------------
def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng, rig2 = _engine(rig)
    try:
        n = 4
        d_ent = torch.zeros((n + 1, 144), dtype=torch.uint8, device=dev)
        d_eph = torch.full((32 * (n + 1),), 0x33, dtype=torch.uint8, device=dev)
        d_li = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        d_st = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
        d_sess = torch.full((n + 1, 176), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        good = lambda: [d_ent[:n], None, d_eph[:32 * n], d_li[:n], d_st, d_sess[:n], d_sum]  # noqa: E731

        def untouched():
            torch.cuda.synchronize()
            assert (d_sum.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == GUARD).all()
            assert (d_sess.cpu().numpy() == 0x7E).all() and (d_eph.cpu().numpy() == 0x33).all()

        for step in range(2):  # before any static key, also after a wg_hs_key_set
            with pytest.raises(W.WgError) as e:
                eng.hs_respond(*good())
            assert e.value.code == Lb.WG_ENOKEY
            eng.hs_key_set(_pub(STATIC))
        untouched()
        eng.hs_static_set(STATIC)
        flat, eflat = d_sess.reshape(-1), d_ent.reshape(-1)
        bads = []
        for at, val in [(2, d_eph[8:8 + 32 * n]),                               # ephemerals misaligned
                        (5, flat[8:8 + 176 * n].reshape(n, 176)),               # sessions misaligned
                        (0, eflat[8:8 + 144 * n].reshape(n, 144)),              # inits misaligned
                        (2, flat[0:32 * n]),                                    # ephemerals inside sessions
                        (4, flat[0:16].view(torch.int32)),                      # resp_status inside sessions
                        (6, flat[16:32].view(torch.int32)),                     # summary inside sessions
                        (5, d_ent[1:n + 1]),                                     # sessions inside inits
                        (2, eflat[0:32 * n]),                                   # ephemerals inside inits
                        (4, d_li[1:n + 1])]:                                    # resp_status inside local_index
            a = good()
            a[at] = val
            bads.append(a)
        for a in bads:
            with pytest.raises(W.WgError) as e:
                eng.hs_respond(*a)
            assert e.value.code == Lb.WG_EINVAL
        for name in ("inits", "ephemerals", "local_index", "resp_status", "sessions", "summary"):  # a NULL pointer
            b = Lb.WgHsRespondBatch(d_ent.data_ptr(), None, d_eph.data_ptr(), d_li.data_ptr(), d_st.data_ptr(), d_sess.data_ptr(),
                                    d_sum.data_ptr(), n, 0)
            setattr(b, name, None)
            assert eng._lib.wg_hs_respond(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        for flags in (2, 0x80000001):  # an unknown flag
            b = Lb.WgHsRespondBatch(d_ent.data_ptr(), None, d_eph.data_ptr(), d_li.data_ptr(), d_st.data_ptr(), d_sess.data_ptr(),
                                    d_sum.data_ptr(), n, flags)
            assert eng._lib.wg_hs_respond(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        untouched()
        eng.hs_respond(d_ent[:0], None, d_eph[:0], d_li[:0], d_st[:0], d_sess[:0], d_sum)  # n = 0: a no-op
        untouched()
    finally:
        eng.close()
