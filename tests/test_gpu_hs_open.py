"""wg_hs_peers_set and wg_hs_open on the MI355X against tests/hs_open_model.py (pytest -m gpu): statuses, entries
and summaries are compared exactly, and every output array carries guard bytes or words behind what the call may
write. The initiations come from a pool of 24 (ephemeral, initiator) pairs, so the memoised ladder model of
test_gpu_x25519 stays at a few hundred distinct operands."""
import functools

import numpy as np
import pytest

import hs_model as HM
import hs_open_model as OM
import x25519_model as M
from test_gpu_x25519 import FILL, GUARD, LOW, SESS, STATIC, STATIC2, _Chain, _engine, _Memo, le, model
from wgtest import noise, splitmix_np, wg

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 63, 64, 65, 255, 256, 257]  # a wave, and the 256 records of one partial
EPHK = [bytes(splitmix_np(0x5000 + k, 32)) for k in range(24)]   # the pool's ephemeral private keys
INITK = [bytes(splitmix_np(0x5100 + j, 32)) for j in range(6)]   # initiators: 0..3 are peers, 4 and 5 are not
TS = bytes(splitmix_np(0x5200, 12))
ALL5 = {OM.OPEN_OK, OM.OPEN_NEWPEER, OM.OPEN_BADAUTH, OM.OPEN_SKIPPED, OM.OPEN_BADDESC}


def _pub(private):
    return model(private, M.BASE_POINT)


def _peers():
    return [_pub(k) for k in INITK[:4]]


@functools.lru_cache(maxsize=None)
def _hello(responder, k, static_public=None):
    """Pool entry k's genuine initiation to the responder with this private key."""
    with _Memo():
        return OM.initiate(INITK[k % 6], _pub(responder), EPHK[k], TS, static_public=static_public)


@functools.lru_cache(maxsize=None)
def _hello_low(responder, low, j):
    """Initiator j's initiation with the low-order ephemeral LOW[low], sealed under the all-zero secret."""
    with _Memo():
        return OM.initiate(INITK[j], _pub(responder), None, TS, ephemeral_public=LOW[low], es_secret=bytes(32))


def _flip(b, at, bit):
    return b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]


def _open_ring(rng, n_list, responder):
    """test_gpu_x25519._chain_ring's recipe with genuine initiations: a UDP ring whose plan lists exactly n_list
    handshake datagrams, at unaligned offsets, among transport packets. Initiations of known and unknown
    initiators, as they are or with one flipped bit in encrypted_static's ciphertext, in its tag, in the
    ephemeral (always the same bit, so the pool of ephemerals only doubles) or in encrypted_timestamp;
    initiations with low-order ephemerals sealed under ss = 0; responses; messages with a flipped mac1 bit."""
    import struct
    pub = _pub(responder)
    known = list(SESS.keys())
    buf, off, lens = bytearray(rng.bytes(3)), [], []

    def put(m):
        off.append(len(buf))
        lens.append(len(m))
        buf.extend(m + rng.bytes(int(rng.integers(0, 4))))

    for k in range(n_list):
        r = rng.random()
        forced = k in (0, 63, 64, 255, 256)
        sender, reserved = int(rng.integers(0, 1 << 32)), rng.bytes(3)
        if forced or r < 0.45:
            b = OM.body(sender, _hello(responder, int(rng.integers(0, 24))), reserved)  # E 7..39, ct 39..71, tag 71..87, ts 87..115
            q = 1.0 if forced else rng.random()
            if q < 0.1:
                b = _flip(b, int(rng.integers(39, 71)), int(rng.integers(0, 8)))
            elif q < 0.2:
                b = _flip(b, int(rng.integers(71, 87)), int(rng.integers(0, 8)))
            elif q < 0.3:
                b = _flip(b, 10, 0)
            elif q < 0.4:
                b = _flip(b, int(rng.integers(87, 115)), int(rng.integers(0, 8)))
            m = HM.message(1, b, pub)
        elif r < 0.57:
            m = HM.message(1, OM.body(sender, _hello_low(responder, int(rng.integers(0, len(LOW))), int(rng.integers(0, 6))), reserved), pub)
        elif r < 0.8:
            m = HM.message(2, rng.bytes(59), pub)
        else:
            m = HM.message(1 + int(rng.integers(0, 2)), rng.bytes(120), pub)
            at = len(m) - 32 + int(rng.integers(0, 16))
            m = _flip(m, at, 2)
        put(m)
        for _ in range(int(rng.integers(0, 3))):
            wl = int(rng.integers(32, 90))
            put(struct.pack("<BxxxIQ", 4, known[int(rng.integers(0, len(known)))], k) + rng.bytes(wl - 16))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32)


class _OpenChain(_Chain):
    """plan -> check -> dh -> open back to back on the current stream; the host reads nothing in between."""

    def __init__(self, rig, n, ring_size, max_len=120):
        super().__init__(rig, n, ring_size, max_len)
        torch, dev = rig.torch, rig.dev
        self.o_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        self.o_init = torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev)
        self.o_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)

    def load(self, ring, off, lens):
        super().load(ring, off, lens)
        self.o_st.fill_(GUARD)
        self.o_init.fill_(0x7E)
        self.o_sum.fill_(GUARD)

    def run(self, with_summary=True):
        super().run(with_summary)
        n = self.n
        self.rig.eng.hs_open(self.d_rec[:n], self.d_sum[:4] if with_summary else None, self.d_shared[:n], self.d_dh[:n],
                             self.o_st[:n], self.o_init[:n], self.o_sum[:4])

    def compare_open(self, pub, private, peers, with_summary=True):
        """The earlier stages against their models (test_gpu_x25519), then the open's three outputs, whole,
        against hs_open_model over what the device holds. Returns (status list of the covered records, entries)."""
        rec, _ = self.compare(pub, private, with_summary)
        n = self.n
        all_rec = np.ascontiguousarray(self.d_rec.cpu().numpy()[:n]).view(HM.HS_RECORD).reshape(-1)
        shared = self.d_shared.cpu().numpy().tobytes()
        dh = self.d_dh.cpu().numpy().view(np.uint32).tolist()
        with _Memo():
            st, inits, sm = OM.open_batch(all_rec, len(rec) if with_summary else None, n, shared, dh, private, peers,
                                          [GUARD] * (n + 4), b"\x7e" * (144 * (n + 1)), [GUARD] * 4)
        got = self.o_st.cpu().numpy().view(np.uint32).tolist()
        assert got == st, [(k, a, b) for k, (a, b) in enumerate(zip(got, st)) if a != b][:5]
        osum = self.o_sum.cpu().numpy().view(np.uint32)
        assert osum[:4].tolist() == sm and (osum[4:] == GUARD).all()
        got_init = self.o_init.cpu().numpy().tobytes()
        if got_init != inits:
            bad = [j for j in range(n + 1) if got_init[144 * j:144 * j + 144] != inits[144 * j:144 * j + 144]][:3]
            raise AssertionError(("entries differ", bad, [np.frombuffer(got_init[144 * j:144 * j + 144], OM.HS_INIT) for j in bad],
                                  [np.frombuffer(inits[144 * j:144 * j + 144], OM.HS_INIT) for j in bad]))
        cover = len(rec) if with_summary else n
        return st[:cover], np.frombuffer(inits[:144 * sm[0]], OM.HS_INIT)


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    yield type("Rig", (), dict(eng=None, torch=torch, dev=torch.device("cuda", 0), W=wg()))


# ---- the chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_list", SHAPES)
def test_plan_check_dh_open_on_one_stream(rig, n_list):
    """With the record count read on the device a record is an initiation or a response with a status of
    wg_hs_dh, so four statuses can occur, and for n_list >= 255 all four must, with both OK and NEWPEER among
    the entries; the fifth, BADDESC, is what n_records = NULL gives for the records behind n_valid, and the
    second run must show all five."""
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = _peers()
        eng.hs_peers_set(peers)
        rng = np.random.default_rng(5300 + n_list)
        ring, off, lens = _open_ring(rng, n_list, STATIC)
        n = len(off) + 5
        ch = _OpenChain(rig2, n, len(ring) + 64)
        ch.load(ring, off, lens)
        ch.run()
        st, inits = ch.compare_open(pub, STATIC, peers)
        if n_list >= 255:
            assert set(st) == ALL5 - {OM.OPEN_BADDESC}
            assert {int(p) for p in inits["peer"]} == {0, 1, 2, 3, OM.NOPEER}
            dh = ch.d_dh.cpu().numpy()[:len(st)]
            assert any(s in (OM.OPEN_OK, OM.OPEN_NEWPEER) and d == M.X_ZERO for s, d in zip(st, dh))  # ss = 0 is accepted
            assert (np.diff(inits["record"].astype(np.int64)) > 0).all()
        ch.load(ring, off, lens)
        ch.run(with_summary=False)
        st, _ = ch.compare_open(pub, STATIC, peers, with_summary=False)
        assert st[-5:] == [OM.OPEN_BADDESC] * 5
        if n_list >= 255:
            assert set(st) == ALL5
    finally:
        eng.close()


def test_opens_on_two_streams(rig):
    """Six opens of two rings issued back to back on two streams, alternating, with no synchronisation between
    them: they share the scratch (with each other and with wg_hs_check), the library chains them, and each equals
    what its ring's chain gave on one stream, which compare_open has checked against the model. Ring A lists 300
    handshake datagrams (two ranges of 256, the second part-filled), ring B 70 (one part-filled range, two waves):
    calls of different size take the scratch in turn."""
    torch, dev = rig.torch, rig.dev
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = _peers()
        eng.hs_peers_set(peers)
        rng = np.random.default_rng(5800)
        chains = []
        for n_list in (300, 70):
            ring, off, lens = _open_ring(rng, n_list, STATIC)
            ch = _OpenChain(rig2, len(off) + 5, len(ring) + 64)
            ch.load(ring, off, lens)
            ch.run()
            st, inits = ch.compare_open(pub, STATIC, peers)
            assert {OM.OPEN_OK, OM.OPEN_NEWPEER, OM.OPEN_BADAUTH} <= set(st) and len(inits) > 0
            want = tuple(t.cpu().numpy().tobytes() for t in (ch.o_st, ch.o_init, ch.o_sum))
            chains.append((ch, want))
        outs = []
        for k in range(6):  # every call's own outputs, with the guards compare_open's expectation carries
            n = chains[k % 2][0].n
            outs.append((torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev),
                         torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev),
                         torch.full((8,), GUARD, dtype=torch.int32, device=dev)))
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        torch.cuda.synchronize()
        for k in range(6):
            ch, n = chains[k % 2][0], chains[k % 2][0].n
            o_st, o_init, o_sum = outs[k]
            eng.hs_open(ch.d_rec[:n], ch.d_sum[:4], ch.d_shared[:n], ch.d_dh[:n], o_st[:n], o_init[:n], o_sum[:4],
                        stream=streams[k % 2].cuda_stream)
        torch.cuda.synchronize()
        for k, (o_st, o_init, o_sum) in enumerate(outs):
            n, want = chains[k % 2][0].n, chains[k % 2][1]
            got = tuple(t.cpu().numpy().tobytes() for t in (o_st, o_init, o_sum))
            assert got[0] == want[0], ("status", k)
            assert got[1] == want[1], ("entries", k)
            assert got[2] == want[2], ("summary", k)
            assert (o_st.cpu().numpy()[n:] == GUARD).all() and (o_sum.cpu().numpy()[4:] == GUARD).all()
            assert (o_init.cpu().numpy()[int(o_sum[0]):] == 0x7E).all()  # behind the n_emitted entries
    finally:
        eng.close()


# ---- the peer table ------------------------------------------------------------------------------------------------
def _direct(rig2, msgs, private, peers):
    """Records made by hand through wg_hs_dh + wg_hs_open (n_records = NULL), compared whole with the models.
    Returns (status list, entries)."""
    torch, dev, eng = rig2.torch, rig2.dev, rig2.eng
    n = len(msgs)
    rec = np.zeros(n, HM.HS_RECORD)
    for k, m in enumerate(msgs):
        rec[k] = (100 + k, len(m), np.frombuffer(m.ljust(148, b"\0"), np.uint8), 0)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(n, 160).copy()).to(dev)
    d_sh = torch.full((n + 1, 32), FILL, dtype=torch.uint8, device=dev)
    d_dh, o_st = (torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
    o_init = torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev)
    o_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    eng.hs_dh(d_rec, None, d_sh[:n], d_dh[:n])
    eng.hs_open(d_rec, None, d_sh[:n], d_dh[:n], o_st[:n], o_init[:n], o_sum[:4])
    torch.cuda.synchronize()
    with _Memo():
        sh, dh = M.hs_dh(rec, None, n, private, bytes([FILL]) * (32 * (n + 1)), [GUARD] * (n + 4))
        st, inits, sm = OM.open_batch(rec, None, n, sh, dh, private, peers, [GUARD] * (n + 4), b"\x7e" * (144 * (n + 1)), [GUARD] * 4)
    assert d_sh.cpu().numpy().tobytes() == sh and d_dh.cpu().numpy().view(np.uint32).tolist() == dh
    assert o_st.cpu().numpy().view(np.uint32).tolist() == st
    osum = o_sum.cpu().numpy().view(np.uint32)
    assert osum[:4].tolist() == sm and (osum[4:] == GUARD).all()
    assert o_init.cpu().numpy().tobytes() == inits
    return st[:n], np.frombuffer(inits[:144 * sm[0]], OM.HS_INIT)


def test_peer_table(rig):
    """0, 1 and 300 peers. In the large table the initiator's key A sits behind a key with A's first 8 bytes
    (the same bucket: the probe walks past it) and a key that differs from A in the last byte only; A with bit
    255 set is another peer, and a low-order point is a peer whose static-static secret is zero. Equal keys
    are refused and change nothing; a new static key recomputes the stored secrets."""
    W = rig.W
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        A, B = _pub(INITK[0]), _pub(INITK[1])
        A8 = A[:8] + bytes(splitmix_np(0x5400, 24))
        A31 = A[:31] + bytes([A[31] ^ 1])
        A255 = A[:31] + bytes([A[31] ^ 0x80])
        LOWP = le(1)

        def msgs(responder):
            hs = [_hello(responder, 0), _hello(responder, 1), _hello(responder, 6, A255), _hello(responder, 12, LOWP),
                  _hello(responder, 18, A31)]
            return [HM.message(1, OM.body(0x11110000 + k, h), _pub(responder)) for k, h in enumerate(hs)]

        m1 = msgs(STATIC)
        st, _ = _direct(rig2, m1, STATIC, [])  # never set
        assert st == [OM.OPEN_NEWPEER] * 5
        eng.hs_peers_set([A])
        st, inits = _direct(rig2, m1, STATIC, [A])
        assert st == [OM.OPEN_OK] + [OM.OPEN_NEWPEER] * 4 and inits["peer"].tolist() == [0] + [OM.NOPEER] * 4
        table = [A8, A31] + [bytes(splitmix_np(0x5500 + k, 32)) for k in range(298)]
        table[150], table[151], table[152] = A, A255, LOWP
        eng.hs_peers_set(b"".join(table))
        st, inits = _direct(rig2, m1, STATIC, table)
        assert st == [OM.OPEN_OK, OM.OPEN_NEWPEER, OM.OPEN_OK, OM.OPEN_OK, OM.OPEN_OK]
        assert inits["peer"].tolist() == [150, OM.NOPEER, 151, 152, 1]
        first_ck = inits["chain_key"].copy()
        for bad in ([A, B, A], table + [table[299]]):
            with pytest.raises(W.WgError) as e:
                eng.hs_peers_set(bad)
            assert e.value.code == W._lib.WG_EINVAL
        assert _direct(rig2, m1, STATIC, table)[0] == st  # nothing changed
        # a new static key: the stored peers' secrets are recomputed (messages made for the new public key)
        pub2 = eng.hs_static_set(STATIC2)
        assert pub2 == _pub(STATIC2) != pub
        st2, inits2 = _direct(rig2, msgs(STATIC2), STATIC2, table)
        assert st2 == st and inits2["peer"].tolist() == [150, OM.NOPEER, 151, 152, 1]
        assert all((inits2["chain_key"][k] != first_ck[k]).any() for k in range(5))
        assert _direct(rig2, m1, STATIC2, table)[0] == [OM.OPEN_BADAUTH] * 5  # (made for the old key)
        eng.hs_peers_set([])  # n = 0 empties the table
        assert _direct(rig2, msgs(STATIC2), STATIC2, [])[0] == [OM.OPEN_NEWPEER] * 5
    finally:
        eng.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_error_returns(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng, rig2 = _engine(rig)
    try:
        n = 4
        d_rec = torch.zeros((n + 1, 160), dtype=torch.uint8, device=dev)
        d_sh = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_dh, o_st = (torch.full((n,), GUARD, dtype=torch.int32, device=dev) for _ in range(2))
        o_init = torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev)
        o_sum = torch.full((4,), GUARD, dtype=torch.int32, device=dev)
        args = lambda: (d_rec[:n], None, d_sh, d_dh, o_st, o_init[:n], o_sum)  # noqa: E731
        for step in range(2):  # before any static key, also after a wg_hs_key_set
            with pytest.raises(W.WgError) as e:
                eng.hs_open(*args())
            assert e.value.code == Lb.WG_ENOKEY
            with pytest.raises(W.WgError) as e:
                eng.hs_peers_set([_pub(INITK[0])])
            assert e.value.code == Lb.WG_ENOKEY
            eng.hs_key_set(_pub(STATIC))
        eng.hs_static_set(STATIC)
        flat = o_init.reshape(-1)
        for bad in [(d_rec[:n], None, d_sh, d_dh, d_dh, o_init[:n], o_sum),                    # open_status is dh_status
                    (d_rec[:n], None, d_sh, d_dh, o_st, d_rec[1:n + 1], o_sum),                # inits inside records
                    (d_rec[:n], None, d_sh, d_dh, o_st, o_init[:n], flat[16:32].view(torch.int32)),  # summary inside inits
                    (d_rec[:n], None, d_sh, d_dh, flat[0:16].view(torch.int32), o_init[:n], o_sum),  # open_status inside inits
                    (d_rec[:n], None, d_sh, d_dh, o_st, flat[8:8 + 144 * n].reshape(n, 144), o_sum)]:  # inits misaligned
            with pytest.raises(W.WgError) as e:
                eng.hs_open(*bad)
            assert e.value.code == Lb.WG_EINVAL
        eng.hs_open(d_rec[:0], None, d_sh[:0], d_dh[:0], o_st[:0], o_init[:0], o_sum)  # n = 0: a no-op
        torch.cuda.synchronize()
        assert (o_sum.cpu().numpy() == GUARD).all() and (o_st.cpu().numpy() == GUARD).all()
        assert (o_init.cpu().numpy() == 0x7E).all()
    finally:
        eng.close()


# ---- graphs --------------------------------------------------------------------------------------------------------------
def test_captured_plan_check_dh_open_replay(rig):
    """Reserve, then plan + check + dh + open captured once and replayed over two rings, with wg_hs_peers_set and
    wg_hs_static_set between the replays and no re-capture. An open on a capturing stream that needs more
    scratch than was reserved returns WG_EINVAL."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        pub2 = _pub(STATIC2)
        peers = _peers()
        rng = np.random.default_rng(5600)
        rings = [_open_ring(rng, 70, STATIC), _open_ring(rng, 90, STATIC2)]
        n = max(len(r[1]) for r in rings) + 3
        ch = _OpenChain(rig2, n, max(len(r[0]) for r in rings) + 64)
        big = 8 * n  # more than this context reserved
        b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)
        b_sh = torch.zeros((big, 32), dtype=torch.uint8, device=dev)
        b_dh, b_st = (torch.zeros(big, dtype=torch.int32, device=dev) for _ in range(2))
        b_init = torch.zeros((big, 144), dtype=torch.uint8, device=dev)
        eng.rx_reserve(n)
        eng.hs_reserve(n)
        ch.load(*rings[0])
        ch.run()  # eager once, with an empty table: every authentic initiation is a NEWPEER
        st, _ = ch.compare_open(pub, STATIC, [])
        assert OM.OPEN_NEWPEER in st and OM.OPEN_OK not in st
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                eng.hs_open(b_rec, None, b_sh, b_dh, b_st, b_init, ch.o_sum[4:8])
            ch.run()
        assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
        eng.hs_peers_set(peers)
        counts = []
        for replay, (key, p, table) in enumerate([(STATIC, pub, peers), (STATIC2, pub2, peers[:2])]):
            if replay == 1:
                assert eng.hs_static_set(STATIC2) == pub2
                eng.hs_peers_set(table)
            ch.load(*rings[replay])
            torch.cuda.synchronize()
            g.replay()
            st, inits = ch.compare_open(p, key, table)
            counts.append((st.count(OM.OPEN_OK), st.count(OM.OPEN_NEWPEER), st.count(OM.OPEN_BADAUTH)))
            assert {int(x) for x in inits["peer"]} <= set(range(len(table))) | {OM.NOPEER}
        assert all(min(c) >= 3 for c in counts)
    finally:
        eng.close()


# ---- the mirror ---------------------------------------------------------------------------------------------------------
def test_mirror_decrypt_remote_static_and_derive_key(rig):
    N = noise()
    local = N.NoisePrivateKey(STATIC)
    h = _hello(STATIC, 5)
    eph = N.NoisePublicKey(h["ephemeral"])
    got = N.Handshakes.decryptRemoteStatic(local, eph, h["encrypted_static"], h["encrypted_timestamp"])
    assert got == N.NoisePublicKey(_pub(INITK[5]))  # a key no peer holds is returned like any other
    with pytest.raises(N.BadPaddingException):
        N.Handshakes.decryptRemoteStatic(local, eph, _flip(h["encrypted_static"], 47, 7), h["encrypted_timestamp"])
    with pytest.raises(N.BadPaddingException):
        N.Handshakes.decryptRemoteStatic(local, N.NoisePublicKey(_flip(h["ephemeral"], 0, 0)), h["encrypted_static"],
                                         h["encrypted_timestamp"])
    assert N.Handshakes.decryptRemoteStatic(local, eph, h["encrypted_static"], _flip(h["encrypted_timestamp"], 3, 3)) == got
    salt, ikm = bytes(splitmix_np(0x5700, 32)), bytes(splitmix_np(0x5701, 32))
    for n in (1, 2, 3):
        assert N.Crypto.deriveKey(salt, ikm, n) == OM.derive_key(salt, ikm, n)
    assert N.Crypto.deriveKey(OM.INITIAL_CHAIN_KEY, h["ephemeral"]) == OM.derive_key(OM.INITIAL_CHAIN_KEY, h["ephemeral"])
    out = bytearray(16)
    N.Crypto.HMAC(out, b"k" * 70, b"ab", b"c")
    assert bytes(out) == OM.hmac(b"k" * 70, b"abc")[:16]
