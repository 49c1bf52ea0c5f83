"""wg_hs_psks_set and wg_hs_initiate on the MI355X against tests/hs_initiate_model.py (pytest -m gpu): statuses,
records, pending entries, summaries and the ephemerals after the call are compared exactly, and every output array
carries guard bytes or words behind what the call may write. Ephemerals come from a pool of 8 and peers from a table
of 4, so the memoised pure-Python ladder stays at a few dozen operands."""
import ctypes
import functools

import numpy as np
import pytest

import hs_initiate_model as IM
import hs_model as HM
import x25519_model as XM
from wgtest import noise, splitmix_bytes, wg

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]  # a wave of ladders holds 32 entries, a workgroup of the chain 256
GUARD = 0x7E7E7E7E
FILL = 0x5A
A_PRIV = splitmix_bytes(0x6700, 32)                                # the initiator's static private key
B_PRIV = [splitmix_bytes(0x6710 + j, 32) for j in range(4)]        # the responders': A's peers, in table order 2, 0, 3, 1
TABLE = [2, 0, 3, 1]
EPH = [splitmix_bytes(0x6720 + j, 32) for j in range(8)]           # the pool's ephemeral private keys
REPH = [splitmix_bytes(0x6730 + j, 32) for j in range(4)]          # the responders' ephemerals
PSKS = [bytes(32), splitmix_bytes(0x6740, 32), bytes(32), splitmix_bytes(0x6741, 32)]  # by table position
LATE = bytes([7]) + bytes(31)                                      # the all-zero scalar only after clamping

ladder = functools.lru_cache(maxsize=None)(XM.x25519)


class Memo:
    """The models with the memoised ladder (they call it through x25519_model)."""

    def __enter__(self):
        self.keep, XM.x25519 = XM.x25519, ladder

    def __exit__(self, *a):
        XM.x25519 = self.keep


def pub(private):
    return ladder(private, XM.BASE_POINT)


def peers():
    return [pub(B_PRIV[j]) for j in TABLE]


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    yield type("Rig", (), dict(torch=torch, dev=torch.device("cuda", 0), W=wg()))


def initiator(rig, with_psks=False):
    eng = rig.W.Engine(0, key_slots=16)
    assert eng.hs_static_set(A_PRIV) == pub(A_PRIV)
    eng.hs_peers_set(peers())
    if with_psks:
        eng.hs_psks_set(PSKS)
    return eng


def inputs(n):
    """peer (positions out of order, every eleventh past the table), ephemerals (the pool's, every fifth all zero, LATE
    at 2 and 66), timestamps, local_index."""
    peer = [(3 * k + 1) % 4 if k % 11 != 5 else (4 + k % 3 if k % 2 else 0xFFFFFFFF) for k in range(n)]
    eph = b"".join(bytes(32) if k % 5 == 4 else LATE if k in (2, 66) else EPH[k % 8] for k in range(n))
    ts = b"".join(splitmix_bytes(0x6800 + k, 12) for k in range(n))
    li = [(0x5000 + 0x01000193 * k) & 0xFFFFFFFF for k in range(n)]
    return peer, eph, ts, li


def t_u32(rig, values):
    return rig.torch.from_numpy(np.array(values, np.uint32).view(np.int32).copy()).to(rig.dev)


def t_u8(rig, data):
    return rig.torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(rig.dev)


def call_initiate(rig, eng, peer, eph, ts, li):
    """One wg_hs_initiate over guarded outputs: (ephemerals, status list, records, pending, summary list) as the
    device holds them, guards included."""
    torch, dev = rig.torch, rig.dev
    n = len(peer)
    d_eph = t_u8(rig, eph + bytes([FILL]) * 32)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_rec = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
    d_pend = torch.full((n + 1, 112), 0x7E, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    eng.hs_initiate(t_u32(rig, peer), d_eph[:32 * n], t_u8(rig, ts + b"\0" * 4), t_u32(rig, li), d_st[:n], d_rec[:n], d_pend[:n],
                    d_sum[:4])
    torch.cuda.synchronize()
    return (d_eph.cpu().numpy().tobytes(), d_st.cpu().numpy().view(np.uint32).tolist(), d_rec.cpu().numpy().tobytes(),
            d_pend.cpu().numpy().tobytes(), d_sum.cpu().numpy().view(np.uint32).tolist())


def model_initiate(peer, eph, ts, li):
    n = len(peer)
    with Memo():
        e2, st, rec, pend, sm = IM.initiate_batch(A_PRIV, peers(), peer, eph + bytes([FILL]) * 32, ts, li, n, [GUARD] * (n + 4),
                                                  b"\x7e" * (160 * (n + 1)), b"\x7e" * (112 * (n + 1)), [GUARD] * 4)
    return e2, st, rec, pend, sm + [GUARD] * 4


def same_initiate(got, want, n):
    assert got[1] == want[1], [(k, a, b) for k, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:5]
    assert got[4] == want[4]
    for name, i, size, dt in (("records", 2, 160, HM.HS_RECORD), ("pending", 3, 112, IM.HS_PENDING)):
        if got[i] != want[i]:
            bad = [j for j in range(n + 1) if got[i][size * j:size * j + size] != want[i][size * j:size * j + size]][:2]
            raise AssertionError((name, bad, [np.frombuffer(got[i][size * j:size * j + size], dt) for j in bad],
                                  [np.frombuffer(want[i][size * j:size * j + size], dt) for j in bad]))
    assert got[0] == want[0], [k for k in range(n + 1) if got[0][32 * k:32 * k + 32] != want[0][32 * k:32 * k + 32]][:5]


@pytest.mark.parametrize("n", SHAPES)
def test_initiations_against_the_model(rig, n):
    eng = initiator(rig)
    try:
        peer, eph, ts, li = inputs(n)
        got = call_initiate(rig, eng, peer, eph, ts, li)
        want = model_initiate(peer, eph, ts, li)
        same_initiate(got, want, n)
        if n >= 31:
            assert set(want[1][:n]) == {IM.INIT_OK, IM.INIT_BADPEER, IM.INIT_NOEPH}
            assert want[1][2] == IM.INIT_OK  # LATE goes through
        # the records pass the responder's admission check under its key
        tab, rec = peers(), np.frombuffer(got[2][:160 * n], HM.HS_RECORD)
        for k in range(n):
            if want[1][k] == IM.INIT_OK:
                msg = rec[k]["msg"].tobytes()
                assert HM.check_one(msg, 148, [0], [148], 1, 0, HM.mac1_key(tab[peer[k]])) == (HM.HS_OK, msg)
    finally:
        eng.close()


def test_captured_initiate_replays_and_consumes_its_ephemerals(rig):
    """Reserve, capture, replay with fresh ephemerals; a replay without them initiates nothing (all NOEPH or BADPEER);
    wg_hs_peers_set between replays needs no re-capture. A capturing call that would have to grow its scratch:
    WG_EINVAL."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    eng = initiator(rig)
    try:
        n = 70
        peer, eph, ts, li = inputs(n)
        d_peer, d_ts, d_li = t_u32(rig, peer), t_u8(rig, ts), t_u32(rig, li)
        d_eph = t_u8(rig, eph)
        d_st = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
        d_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
        d_pend = torch.zeros((n, 112), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        big = 8 * n
        b_u32 = torch.zeros(big, dtype=torch.int32, device=dev)
        b_st, b_li = (torch.zeros(big, dtype=torch.int32, device=dev) for _ in range(2))
        b_eph, b_ts = torch.ones(32 * big, dtype=torch.uint8, device=dev), torch.zeros(12 * big, dtype=torch.uint8, device=dev)
        b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)
        b_pend = torch.zeros((big, 112), dtype=torch.uint8, device=dev)
        b_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        eng.hs_reserve(n)
        eng.hs_initiate(d_peer, d_eph, d_ts, d_li, d_st, d_rec, d_pend, d_sum)  # eager once
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                eng.hs_initiate(b_u32, b_eph, b_ts, b_li, b_st, b_rec, b_pend, b_sum)
            eng.hs_initiate(d_peer, d_eph, d_ts, d_li, d_st, d_rec, d_pend, d_sum)
        assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
        want = model_initiate(peer, eph, ts, li)
        for replay in range(2):
            if replay == 1:
                eng.hs_peers_set(peers())  # the table is rebuilt (and may move)
            d_eph.copy_(t_u8(rig, eph))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert d_st.cpu().numpy().view(np.uint32).tolist() == want[1][:n]
            assert d_rec.cpu().numpy().tobytes() == want[2][:160 * n] and d_pend.cpu().numpy().tobytes() == want[3][:112 * n]
            assert d_sum.cpu().numpy().view(np.uint32).tolist() == want[4][:4] and d_eph.cpu().numpy().tobytes() == want[0][:32 * n]
            g.replay()  # no fresh ephemerals
            torch.cuda.synchronize()
            st = d_st.cpu().numpy().view(np.uint32).tolist()
            assert IM.INIT_OK not in st and st.count(IM.INIT_NOEPH) == want[1][:n].count(IM.INIT_OK) + want[1][:n].count(IM.INIT_NOEPH)
            assert int(d_sum.cpu().numpy()[0]) == 0 and not d_rec.cpu().numpy().any() and not d_pend.cpu().numpy().any()
    finally:
        eng.close()


def test_mirror_initiator_against_the_mirror_responder(rig):
    """initiateHandshake(...).consumeMessageResponse(...) against the mirror's own responderHandshake: the keys are
    crosswise equal, a forged encryptedEmpty raises BadPaddingException and leaves the stage usable."""
    N, W = noise(), rig.W
    eng = W.Engine(0, key_slots=16)
    try:
        a, b = N.NoisePrivateKey(A_PRIV), N.NoisePrivateKey(B_PRIV[0])
        ts = N.Crypto.TAI64N(1_700_000_000_000)
        one = N.Handshakes.initiateHandshake(a, b.publicKey(), N.NoisePresharedKey.zero(), engine=eng, ephemeral=EPH[0], timestamp=ts,
                                             senderIndex=0x11223344)
        with Memo():
            want = IM.initiate_one(A_PRIV, pub(B_PRIV[0]), EPH[0], ts, 0x11223344)
        msg = one.initiation(0x11223344)
        assert msg == want["message"] and one.initiation() == msg
        assert (one.getEncryptedStatic(), one.getEncryptedTimestamp()) == (msg[40:88], msg[88:116])
        assert one.getLocalEphemeral().publicKey() == N.NoisePublicKey(msg[8:40])
        other = one.initiation(5)
        assert other[4:8] == (5).to_bytes(4, "little") and other[116:132] == HM.mac1(other[:116], pub(B_PRIV[0]))
        resp = N.Handshakes.responderHandshake(b, N.NoisePublicKey(msg[8:40]), msg[40:88], msg[88:116], engine=eng, ephemeral=REPH[0],
                                               localIndex=0x55667788)
        assert resp.getRemotePublicKey() == a.publicKey()
        forged = bytearray(resp.getEncryptedEmpty())
        forged[15] ^= 1
        with pytest.raises(N.BadPaddingException):
            one.consumeMessageResponse(resp.getLocalEphemeral(), bytes(forged))
        kp_a, kp_b = one.consumeMessageResponse(resp.getLocalEphemeral(), resp.getEncryptedEmpty()), resp.getKeypair()
        dst = bytearray(4 + 16)
        c = kp_a.cipher(b"ping", dst)
        out = bytearray(4)
        kp_b.decipher(c, bytes(dst), out)
        assert bytes(out) == b"ping"
        c = kp_b.cipher(b"pong", dst)
        kp_a.decipher(c, bytes(dst), out)
        assert bytes(out) == b"pong"
        kp_a.clean()
        kp_b.clean()
        # fresh ephemerals and the clock when none are given
        x, y = (N.Handshakes.initiateHandshake(a, b.publicKey(), engine=eng) for _ in range(2))
        assert x.initiation()[8:40] != y.initiation()[8:40] and len(x.initiation(1)) == 148
    finally:
        eng.close()


def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng = W.Engine(0, key_slots=16)
    try:
        n = 4
        d_peer, d_li = (torch.zeros(n + 1, dtype=torch.int32, device=dev) for _ in range(2))
        d_eph = torch.full((32 * (n + 1),), 0x33, dtype=torch.uint8, device=dev)
        d_ts = torch.zeros(12 * (n + 1), dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
        d_rec = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
        d_pend = torch.full((n + 1, 112), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        good = lambda: [d_peer[:n], d_eph[:32 * n], d_ts[:12 * n], d_li[:n], d_st, d_rec[:n], d_pend[:n], d_sum]  # noqa: E731

        def untouched():
            torch.cuda.synchronize()
            assert (d_sum.cpu().numpy() == GUARD).all() and (d_st.cpu().numpy() == GUARD).all()
            assert (d_rec.cpu().numpy() == 0x7E).all() and (d_pend.cpu().numpy() == 0x7E).all() and (d_eph.cpu().numpy() == 0x33).all()

        for step in range(2):  # before any static key, also after a wg_hs_key_set
            with pytest.raises(W.WgError) as e:
                eng.hs_initiate(*good())
            assert e.value.code == Lb.WG_ENOKEY
            eng.hs_key_set(pub(A_PRIV))
        with pytest.raises(W.WgError) as e:  # no table: only zero psks fit
            eng.hs_psks_set(PSKS)
        assert e.value.code == Lb.WG_EINVAL
        eng.hs_psks_set(b"")
        untouched()
        eng.hs_static_set(A_PRIV)
        eng.hs_peers_set(peers())
        for bad in (PSKS[:3], PSKS + [bytes(32)], b""):  # a count that is not the table's
            with pytest.raises(W.WgError) as e:
                eng.hs_psks_set(bad)
            assert e.value.code == Lb.WG_EINVAL
        eng.hs_psks_set(PSKS)
        rflat, pflat = d_rec.reshape(-1), d_pend.reshape(-1)
        bads = []
        for at, val in [(1, d_eph[8:8 + 32 * n]),                              # ephemerals misaligned
                        (5, rflat[8:8 + 160 * n].reshape(n, 160)),             # records misaligned
                        (6, pflat[8:8 + 112 * n].reshape(n, 112)),             # pending misaligned
                        (2, d_ts[1:1 + 12 * n]),                               # timestamps misaligned
                        (1, rflat[0:32 * n]),                                  # ephemerals inside records
                        (4, pflat[0:16].view(torch.int32)),                    # status inside pending
                        (7, rflat[16:32].view(torch.int32)),                   # summary inside records
                        (6, rflat[0:112 * n].reshape(n, 112)),                 # pending inside records
                        (4, d_li[1:n + 1]),                                    # status inside local_index
                        (1, d_ts[0:32 * n]),                                   # ephemerals inside timestamps (12 n < 32 n: overlap)
                        (4, d_peer[1:n + 1])]:                                 # status inside peer
            a = good()
            a[at] = val
            bads.append(a)
        for a in bads:
            with pytest.raises(W.WgError) as e:
                eng.hs_initiate(*a)
            assert e.value.code == Lb.WG_EINVAL
        args = [d_peer.data_ptr(), d_eph.data_ptr(), d_ts.data_ptr(), d_li.data_ptr(), d_st.data_ptr(), d_rec.data_ptr(),
                d_pend.data_ptr(), d_sum.data_ptr()]
        for name in ("peer", "ephemerals", "timestamps", "local_index", "status", "records", "pending", "summary"):  # a NULL pointer
            b = Lb.WgHsInitiateBatch(*args, n, 0)
            setattr(b, name, None)
            assert eng._lib.wg_hs_initiate(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        b = Lb.WgHsInitiateBatch(*args, n, 1)  # _reserved
        assert eng._lib.wg_hs_initiate(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        b = Lb.WgHsInitiateBatch(*args, (1 << 30) + 1, 0)
        assert eng._lib.wg_hs_initiate(eng.ctx, ctypes.byref(b), None) == Lb.WG_E2BIG
        untouched()
        eng.hs_initiate(d_peer[:0], d_eph[:0], d_ts[:0], d_li[:0], d_st[:0], d_rec[:0], d_pend[:0], d_sum)  # n = 0: a no-op
        untouched()
    finally:
        eng.close()
