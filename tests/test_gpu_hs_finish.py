"""wg_hs_finish on the MI355X against tests/hs_initiate_model.py (pytest -m gpu), and the closed loop: two contexts on
one device complete whole handshakes between them and exchange a transport packet under the derived keys. Statuses,
established entries, summaries and the pending entries after the call are compared exactly; every output array
carries guard bytes or words behind what the call may write."""
import ctypes
import functools

import numpy as np
import pytest

import hs_initiate_model as IM
import hs_model as HM
from test_gpu_hs_initiate import (A_PRIV, B_PRIV, EPH, GUARD, PSKS, REPH, SHAPES, TABLE, Memo, initiator, peers, pub, rig, t_u8,  # noqa: F401
                                  t_u32)
from wgtest import splitmix_bytes, splitmix_np

pytestmark = pytest.mark.gpu

TS = splitmix_bytes(0x6900, 12)


@functools.lru_cache(maxsize=None)
def _hello(e, p):
    """The model's initiation (sender index 0) with pool ephemeral e to table position p."""
    with Memo():
        return IM.initiate_one(A_PRIV, peers()[p], EPH[e], TS, 0)


@functools.lru_cache(maxsize=None)
def _answer(e, p, r, zero_psk=False):
    """... and the model responder's answer to it with its ephemeral r, under the position's psk."""
    with Memo():
        return IM.answer(B_PRIV[TABLE[p]], pub(A_PRIV), _hello(e, p)["message"], REPH[r], 0, bytes(32) if zero_psk else PSKS[p])


def _index(pos):
    return (0x00C0FFEE + 0x9E3779B1 * pos) & 0xFFFFFFFF


def _pending(n_pending):
    """n_pending live entries as wg_hs_initiate leaves them (the chain does not depend on the sender index, mac1
    does, and the response does not cover it), with: an empty entry at 4 (n_pending > 8), entry 5 sharing entry 2's
    local_index, entry 3's peer past the table."""
    pe = np.zeros(n_pending, IM.HS_PENDING)
    for q in range(n_pending):
        e, p = q % 8, (q // 8 + q) % 4
        h = _hello(e, p)
        pe[q]["state"], pe[q]["peer"], pe[q]["local_index"] = 1, p, _index(q)
        pe[q]["ephemeral"] = np.frombuffer(EPH[e], np.uint8)
        pe[q]["hash"] = np.frombuffer(h["hash"], np.uint8)
        pe[q]["chain_key"] = np.frombuffer(h["chain_key"], np.uint8)
    if n_pending > 8:
        pe[4] = np.zeros(1, IM.HS_PENDING)[0]
        pe[5]["local_index"] = pe[2]["local_index"]
        pe[3]["peer"] = 9
    return pe


def _response(q, r, receiver, remote_index, pe):
    """The responder's 92 bytes to pending entry q, with mac1 (which covers both indices) made again."""
    a = _answer(q % 8, int(pe[q]["peer"]) % 4, r)
    head = bytes([2, 0, 0, 0]) + int(remote_index).to_bytes(4, "little") + int(receiver).to_bytes(4, "little") + a["response"][12:60]
    return head + HM.mac1(head, pub(A_PRIV)) + bytes(16)


def _records(n, pe, seed):
    """n records against the pending entries, in shuffled order: responses, and among them a flipped last and first
    tag byte, an unknown receiver index, an initiation, a record of 91 bytes, a second authentic response to an entry
    that already has one, and responses to the entries _pending() made special."""
    rng = np.random.default_rng(seed)
    npend = len(pe)
    order = rng.permutation(max(npend, 1))
    recs = np.zeros(n, HM.HS_RECORD)
    for j in range(n):
        q = int(order[j % len(order)]) if npend else 0
        kind = j % 13
        recs[j]["index"] = 7 * j + 2
        if not npend or kind == 11:  # an unknown receiver index
            m = _response(0, 0, 0x0BADBEEF + j, j, _pending(1)) if not npend else _response(q, j % 4, 0x0BADBEEF + j, j, pe)
        elif kind == 6 and j % 2:
            m = _hello(j % 8, j % 4)["message"]
        else:
            if kind == 9 and j >= 13:
                q = int(order[(j - 9) % len(order)])  # the entry record j - 9 answered: a second authentic response
            m = bytearray(_response(q, j % 4, int(pe[q]["local_index"]), 0x7000 + j, pe))
            if kind == 3:
                m[59] ^= 0x80
            elif kind == 7:
                m[44] ^= 0x01
            m = bytes(m)
        recs[j]["len"] = len(m)
        recs[j]["msg"][:len(m)] = np.frombuffer(m, np.uint8)
        if kind == 6 and not j % 2:
            recs[j]["len"] = 91
    return recs


def _call(rig, eng, recs, n_records, pe):
    torch, dev = rig.torch, rig.dev
    n, npend = len(recs), len(pe)
    d_rec = t_u8(rig, recs.tobytes()).reshape(n, 160)
    d_pend = t_u8(rig, pe.tobytes() + b"\x7e" * 112).reshape(npend + 1, 112)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_est = torch.full((n + 1, 96), 0x7E, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    d_hsum = t_u32(rig, [0 if n_records is None else n_records, 1 << 30, 1 << 30, 1 << 30])
    eng.hs_finish(d_rec, None if n_records is None else d_hsum, d_pend[:npend], d_st[:n], d_est[:n], d_sum[:4])
    torch.cuda.synchronize()
    return (d_pend.cpu().numpy().tobytes(), d_st.cpu().numpy().view(np.uint32).tolist(), d_est.cpu().numpy().tobytes(),
            d_sum.cpu().numpy().view(np.uint32).tolist())


def _model(recs, n_records, pend_bytes, npend):
    n = len(recs)
    with Memo():
        p2, st, est, sm = IM.finish_batch(A_PRIV, 4, PSKS, recs, n_records, n, pend_bytes, npend, [GUARD] * (n + 4),
                                          b"\x7e" * (96 * (n + 1)), [GUARD] * 4)
    return p2, st, est, sm + [GUARD] * 4


def _same(got, want, n, npend):
    assert got[1] == want[1], [(k, a, b) for k, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:5]
    assert got[3] == want[3]
    if got[2] != want[2]:
        bad = [j for j in range(n + 1) if got[2][96 * j:96 * j + 96] != want[2][96 * j:96 * j + 96]][:2]
        raise AssertionError(("established", bad, [np.frombuffer(got[2][96 * j:96 * j + 96], IM.HS_ESTABLISHED) for j in bad],
                              [np.frombuffer(want[2][96 * j:96 * j + 96], IM.HS_ESTABLISHED) for j in bad]))
    assert got[0] == want[0], [q for q in range(npend + 1) if got[0][112 * q:112 * q + 112] != want[0][112 * q:112 * q + 112]][:5]


@pytest.mark.parametrize("n", SHAPES)
def test_responses_against_the_model(rig, n):
    """n_pending smaller and larger than n, the record count below n (on the device) and as NULL; then the same
    records again over what the first call left: the consumed entries answer NOPENDING."""
    eng = initiator(rig, with_psks=True)
    try:
        seen = set()
        for npend, n_records in [(max(n // 2, 1), None), (n + 9, max(n - 2, 0))]:
            pe = _pending(npend)
            recs = _records(n, pe, 7000 + n)
            got = _call(rig, eng, recs, n_records, pe)
            want = _model(recs, n_records, pe.tobytes() + b"\x7e" * 112, npend)
            _same(got, want, n, npend)
            cover = n if n_records is None else min(n, n_records)
            seen |= set(want[1][:cover])
            # a BADAUTH leaves its entry as it was, an OK zeroes it (the model says so; here against the input)
            before = pe.tobytes()
            est = np.frombuffer(want[2][:96 * want[3][0]], IM.HS_ESTABLISHED)
            gone = {int(s["pending"]) for s in est}
            for q in range(npend):
                assert got[0][112 * q:112 * q + 112] == (bytes(112) if q in gone else before[112 * q:112 * q + 112])
            # again: what was OK finds nothing
            pe2 = np.frombuffer(got[0][:112 * npend], IM.HS_PENDING).copy()
            got2 = _call(rig, eng, recs, n_records, pe2)
            _same(got2, _model(recs, n_records, got[0], npend), n, npend)
            # (entries 2 and 5 share a local_index: with 2 consumed, 5 is the one found, and that index's records
            # are judged against it)
            shared = int(pe[2]["local_index"]) if npend > 8 else None
            for k in range(cover):
                if want[1][k] == IM.FIN_OK and int.from_bytes(recs[k]["msg"][8:12].tobytes(), "little") != shared:
                    assert got2[1][k] == IM.FIN_NOPENDING, k
        if n >= 63:
            assert seen == {IM.FIN_OK, IM.FIN_NOPENDING, IM.FIN_BADAUTH, IM.FIN_SKIPPED, IM.FIN_BADDESC}
    finally:
        eng.close()


def test_the_special_pending_entries(rig):
    """Two live entries with one local_index: the lower position answers, and a response made for the higher one fails
    its tag against the lower. An entry whose peer is past the table is not live. Two authentic responses to one entry in
    one call are both emitted, in record order, with the same `pending`."""
    eng = initiator(rig, with_psks=True)
    try:
        pe = _pending(12)
        li2 = int(pe[2]["local_index"])
        msgs = [_response(2, 0, li2, 1, pe), _response(5, 1, li2, 2, pe), _response(3, 0, int(pe[3]["local_index"]), 3, pe),
                _response(7, 2, int(pe[7]["local_index"]), 4, pe), _response(7, 3, int(pe[7]["local_index"]), 5, pe),
                _response(4, 0, 0, 6, _pending(8))]  # the empty entry's index 0 names nothing
        recs = np.zeros(len(msgs), HM.HS_RECORD)
        for j, m in enumerate(msgs):
            recs[j]["index"], recs[j]["len"] = j, 92
            recs[j]["msg"][:92] = np.frombuffer(m, np.uint8)
        got = _call(rig, eng, recs, None, pe)
        want = _model(recs, None, pe.tobytes() + b"\x7e" * 112, 12)
        _same(got, want, len(msgs), 12)
        assert got[1][:6] == [IM.FIN_OK, IM.FIN_BADAUTH, IM.FIN_NOPENDING, IM.FIN_OK, IM.FIN_OK, IM.FIN_NOPENDING]
        est = np.frombuffer(got[2][:96 * 3], IM.HS_ESTABLISHED)
        assert est["pending"].tolist() == [2, 7, 7] and est["record"].tolist() == [0, 3, 4] and est["remote_index"].tolist() == [1, 4, 5]
        assert est[1]["send_key"].tobytes() != est[2]["send_key"].tobytes()
    finally:
        eng.close()


# ---- the closed loop -------------------------------------------------------------------------------------------------
class _Loop:
    """A (the initiator, one peer: B) and B (the responder, one peer: A) on one device. Everything between the host's
    random bytes and the key pairs runs on the device; the host only lays the messages out as rings."""

    def __init__(self, rig, n):
        torch, dev = rig.torch, rig.dev
        self.rig, self.n = rig, n
        self.A, self.B = rig.W.Engine(0, key_slots=16), rig.W.Engine(0, key_slots=16)
        a_pub, b_pub = self.A.hs_static_set(A_PRIV), self.B.hs_static_set(B_PRIV[0])
        self.A.hs_peers_set([b_pub])
        self.B.hs_peers_set([a_pub])
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        self.peer, self.a_li, self.a_st, self.a_sum = z32(n), z32(n), z32(n), z32(4)
        self.a_eph, self.ts, self.a_rec, self.pend = z8(32 * n), z8(12 * n), z8(n, 160), z8(n, 112)
        self.off148 = torch.arange(0, 148 * n, 148, dtype=torch.int64, device=dev)
        self.len148 = torch.full((n,), 148, dtype=torch.int32, device=dev)
        self.b_hst, self.b_hsum, self.b_rec = z32(n), z32(4), z8(n, 160)
        self.b_sh, self.b_dh, self.b_ost, self.b_init, self.b_osum = z8(n, 32), z32(n), z32(n), z8(n, 144), z32(4)
        self.b_eph, self.b_li, self.b_rst, self.b_sess, self.b_rsum = z8(32 * n), z32(n), z32(n), z8(n, 176), z32(4)
        self.ring92 = z8(92 * n)
        self.off92 = torch.arange(0, 92 * n, 92, dtype=torch.int64, device=dev)
        self.len92 = torch.full((n,), 92, dtype=torch.int32, device=dev)
        self.f_hst, self.f_hsum, self.f_rec = z32(n), z32(4), z8(n, 160)
        self.f_st, self.f_est, self.f_sum = z32(n), z8(n, 96), z32(4)

    def close(self):
        self.A.close()
        self.B.close()

    def initiate_and_respond(self, seed):
        """A initiates n entries to B; B runs check -> dh -> open -> respond on A's records laid out as a ring. Leaves B's
        responses in ring92."""
        rig, n, A, B = self.rig, self.n, self.A, self.B
        self.a_eph.copy_(t_u8(rig, splitmix_np(seed, 32 * n).tobytes()))
        self.b_eph.copy_(t_u8(rig, splitmix_np(seed + 1, 32 * n).tobytes()))
        self.ts.copy_(t_u8(rig, splitmix_np(seed + 2, 12 * n).tobytes()))
        self.a_li.copy_(t_u32(rig, [(0x1000 * seed + 3 * k + 1) & 0xFFFFFFFF for k in range(n)]))
        self.b_li.copy_(t_u32(rig, [(0x80000000 + 0x1000 * seed + 5 * k) & 0xFFFFFFFF for k in range(n)]))
        A.hs_initiate(self.peer, self.a_eph, self.ts, self.a_li, self.a_st, self.a_rec, self.pend, self.a_sum)
        ring = self.a_rec[:, 8:156].contiguous().reshape(-1)
        B.hs_check(ring, self.off148, self.len148, self.b_hst, self.b_rec, self.b_hsum)
        B.hs_dh(self.b_rec, self.b_hsum, self.b_sh, self.b_dh)
        B.hs_open(self.b_rec, self.b_hsum, self.b_sh, self.b_dh, self.b_ost, self.b_init, self.b_osum)
        B.hs_respond(self.b_init, self.b_osum, self.b_eph, self.b_li, self.b_rst, self.b_sess, self.b_rsum)
        self.ring92.copy_(self.b_sess[:, 16:108].contiguous().reshape(-1))
        rig.torch.cuda.synchronize()
        assert self.a_sum.cpu().numpy().tolist() == [n, 0, 0, 0] and self.b_hsum.cpu().numpy().tolist() == [n, n, 0, 0]
        assert self.b_osum.cpu().numpy().tolist() == [n, n, 0, 0] and self.b_rsum.cpu().numpy().tolist() == [n, 0, 0, 0]

    def check_and_finish(self):
        self.A.hs_check(self.ring92, self.off92, self.len92, self.f_hst, self.f_rec, self.f_hsum)
        self.A.hs_finish(self.f_rec, self.f_hsum, self.pend, self.f_st, self.f_est, self.f_sum)

    def agreed(self):
        """A's entries against B's sessions: every handshake completed, keys crosswise equal."""
        n = self.n
        assert self.f_hsum.cpu().numpy().tolist() == [n, 0, n, 0] and self.f_sum.cpu().numpy().tolist() == [n, 0, 0, 0]
        assert (self.f_st.cpu().numpy() == IM.FIN_OK).all() and not self.pend.cpu().numpy().any()
        est = self.f_est.cpu().numpy().reshape(-1).view(IM.HS_ESTABLISHED)
        from hs_respond_model import HS_SESSION
        sess = self.b_sess.cpu().numpy().reshape(-1).view(HS_SESSION)
        assert est["record"].tolist() == list(range(n)) == est["pending"].tolist() and not est["peer"].any()
        assert (est["local_index"] == sess["remote_index"]).all() and (est["remote_index"] == sess["local_index"]).all()
        assert est["send_key"].tobytes() == sess["recv_key"].tobytes() and est["recv_key"].tobytes() == sess["send_key"].tobytes()
        assert len({s.tobytes() for s in est["send_key"]}) == n
        return est, sess


@pytest.mark.parametrize("n", [65, 257])
def test_two_contexts_complete_handshakes_and_exchange_a_packet(rig, n):
    torch, dev, W = rig.torch, rig.dev, rig.W
    lp = _Loop(rig, n)
    try:
        lp.initiate_and_respond(n)
        lp.check_and_finish()
        torch.cuda.synchronize()
        est, sess = lp.agreed()
        # one transport round trip under the last entry's keys: sealed on A, opened on B
        lp.A.set_keys(2, est[n - 1]["send_key"].tobytes())
        lp.B.set_keys(3, sess[n - 1]["recv_key"].tobytes())
        lens = np.array([1, 16, 100], np.uint32)
        at = 128 * np.arange(3, dtype=np.uint64)
        ctr = np.array([0, 1, 1 << 33], np.uint64)
        pt = splitmix_np(0x6A00, 384)
        d = torch.from_numpy(W.desc_as_int64(W.pack_desc(at, at, ctr, lens, 2))).to(dev)
        ct = torch.zeros(384, dtype=torch.uint8, device=dev)
        lp.A.seal(d, torch.from_numpy(pt).to(dev), ct, 100)
        torch.cuda.synchronize()
        ct[int(at[2]) + 3] ^= 1  # ... and one forged packet
        d = torch.from_numpy(W.desc_as_int64(W.pack_desc(at, at, ctr, lens, 3))).to(dev)
        back = torch.zeros(384, dtype=torch.uint8, device=dev)
        ost = torch.full((3,), 7, dtype=torch.int32, device=dev)
        lp.B.open(d, ct, back, ost, 100)
        torch.cuda.synchronize()
        assert ost.cpu().numpy().tolist() == [0, 0, 1]
        b = back.cpu().numpy()
        for i in range(2):
            o, ln = int(at[i]), int(lens[i])
            assert b[o:o + ln].tobytes() == pt[o:o + ln].tobytes()
    finally:
        lp.close()


def test_captured_check_and_finish_replays(rig):
    """Reserve, capture check -> finish once, replay with the pending entries and the ring refreshed in place; a replay
    without a refresh finds nothing pending; wg_hs_psks_set between replays needs no re-capture (with a non-zero psk B's
    zero-psk responses fail their tags, and the entries stay). A capturing finish that would have to grow its scratch:
    WG_EINVAL."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    n = 70
    lp = _Loop(rig, n)
    try:
        lp.A.hs_reserve(n)
        lp.initiate_and_respond(1)
        lp.check_and_finish()  # eager once
        torch.cuda.synchronize()
        lp.agreed()
        big = 8 * n
        b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)
        b_pend = torch.zeros((big, 112), dtype=torch.uint8, device=dev)
        b_st = torch.zeros(big, dtype=torch.int32, device=dev)
        b_est = torch.zeros((big, 96), dtype=torch.uint8, device=dev)
        b_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                lp.A.hs_finish(b_rec, None, b_pend, b_st, b_est, b_sum)
            lp.check_and_finish()
        assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
        for replay in range(2):
            lp.initiate_and_respond(2 + 3 * replay)  # pend and ring92 refreshed in place
            g.replay()
            torch.cuda.synchronize()
            lp.agreed()
            g.replay()  # no refresh: the entries are consumed
            torch.cuda.synchronize()
            assert (lp.f_st.cpu().numpy() == IM.FIN_NOPENDING).all() and lp.f_sum.cpu().numpy().tolist() == [0, n, 0, 0]
        lp.initiate_and_respond(9)
        before = lp.pend.cpu().numpy().tobytes()
        lp.A.hs_psks_set([splitmix_bytes(0x6A10, 32)])
        g.replay()
        torch.cuda.synchronize()
        assert (lp.f_st.cpu().numpy() == IM.FIN_BADAUTH).all() and lp.f_sum.cpu().numpy().tolist() == [0, 0, n, 0]
        assert lp.pend.cpu().numpy().tobytes() == before
        lp.A.hs_psks_set([bytes(32)])
        g.replay()
        torch.cuda.synchronize()
        lp.agreed()
    finally:
        lp.close()


def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=16)
    try:
        n = 4
        d_rec = torch.zeros((n + 1, 160), dtype=torch.uint8, device=dev)
        d_pend = torch.full((n + 1, 112), 0x7E, dtype=torch.uint8, device=dev)
        d_st = torch.full((n + 1,), GUARD, dtype=torch.int32, device=dev)
        d_est = torch.full((n + 1, 96), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        d_hsum = torch.zeros(4, dtype=torch.int32, device=dev)
        good = lambda: [d_rec[:n], None, d_pend[:n], d_st[:n], d_est[:n], d_sum]  # noqa: E731

        def untouched():
            torch.cuda.synchronize()
            assert (d_sum.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == GUARD).all()
            assert (d_est.cpu().numpy() == 0x7E).all() and (d_pend.cpu().numpy() == 0x7E).all()

        for step in range(2):  # before any static key, also after a wg_hs_key_set
            with pytest.raises(W.WgError) as e:
                eng.hs_finish(*good())
            assert e.value.code == Lb.WG_ENOKEY
            eng.hs_key_set(pub(A_PRIV))
        eng.hs_static_set(A_PRIV)
        rflat, pflat, eflat = d_rec.reshape(-1), d_pend.reshape(-1), d_est.reshape(-1)
        bads = []
        for at, val in [(0, rflat[8:8 + 160 * n].reshape(n, 160)),            # records misaligned
                        (2, pflat[8:8 + 112 * n].reshape(n, 112)),            # pending misaligned
                        (4, eflat[8:8 + 96 * n].reshape(n, 96)),              # established misaligned
                        (2, eflat[0:112 * 3].reshape(3, 112)),                # pending inside established
                        (3, pflat[0:16].view(torch.int32)),                   # fin_status inside pending
                        (5, eflat[16:32].view(torch.int32)),                  # summary inside established
                        (4, rflat[0:96 * n].reshape(n, 96)),                  # established inside records
                        (2, rflat[0:112 * n].reshape(n, 112)),                # pending inside records
                        (1, d_st)]:                                           # n_records inside fin_status
            a = good()
            a[at] = val
            bads.append(a)
        for a in bads:
            with pytest.raises(W.WgError) as e:
                eng.hs_finish(*a)
            assert e.value.code == Lb.WG_EINVAL
        args = [d_rec.data_ptr(), None, d_pend.data_ptr(), d_st.data_ptr(), d_est.data_ptr(), d_sum.data_ptr()]
        for name in ("records", "pending", "fin_status", "established", "summary"):  # a NULL pointer
            b = Lb.WgHsFinishBatch(*args, n, n)
            setattr(b, name, None)
            assert eng._lib.wg_hs_finish(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        b = Lb.WgHsFinishBatch(*args, n, n)
        b.n_records = d_hsum.data_ptr() + 2  # misaligned
        assert eng._lib.wg_hs_finish(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        assert eng._lib.wg_hs_finish(eng.ctx, ctypes.byref(Lb.WgHsFinishBatch(*args, (1 << 30) + 1, n)), None) == Lb.WG_E2BIG
        assert eng._lib.wg_hs_finish(eng.ctx, ctypes.byref(Lb.WgHsFinishBatch(*args, n, (1 << 28) + 1)), None) == Lb.WG_E2BIG
        untouched()
        eng.hs_finish(d_rec[:0], None, d_pend[:n], d_st[:0], d_est[:0], d_sum)  # n = 0: a no-op
        untouched()
    finally:
        eng.close()
