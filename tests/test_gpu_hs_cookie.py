"""wg_hs_cookie_secret_set, wg_hs_admit, wg_hs_cookie_open, wg_hs_cookies_get / _set and wg_hs_mac2 on the MI355X
against tests/hs_cookie_model.py (pytest -m gpu): statuses, records, replies, learned entries, summaries, the nonces
and the cookie table after each call are compared byte for byte, and every output array carries guard bytes or words
behind what the call may write."""
import struct

import numpy as np
import pytest

import hs_cookie_model as CM
import hs_model as HM
import rx_plan_model as RM
from wgtest import splitmix_bytes, splitmix_np, wg

pytestmark = pytest.mark.gpu

GUARD = 0x7E7E7E7E
PUB = bytes(splitmix_np(0x7100, 32))        # the responder's static public key (admit needs no private key)
SECRET = splitmix_bytes(0x7101, 32)
SECRET2 = splitmix_bytes(0x7102, 32)
A_PRIV = splitmix_bytes(0x7110, 32)         # the initiator's static private key
PEERS = [splitmix_bytes(0x7120 + j, 32) for j in range(4)]  # its peers' static public keys (any 32 bytes serve here)
SESS = {0x01020304: 1, 7: 2}
LIST_LENGTHS = [0, 1, 63, 64, 65, 256, 257, 1000]  # a wave, one range of 256 positions, more than one range
# what a listed position can hold; each position's source address is its own
KINDS = ["ok4", "ok6", "zero", "flip0", "flip15", "port", "fam0", "zn_need", "zn_ok", "r_ok", "r_zero", "size", "mac1"]
UNLISTED = ["type", "bounds", "transport"]


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    W = wg()
    eng = W.Engine(0, key_slots=16)
    eng.hs_key_set(PUB)
    eng.hs_cookie_secret_set(SECRET)
    eng.rx_sessions_set(list(SESS.keys()), list(SESS.values()))
    yield type("Rig", (), dict(eng=eng, torch=torch, dev=torch.device("cuda", 0), W=W))
    eng.close()


def t_u8(rig, data):
    return rig.torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(rig.dev)


def t_u32(rig, values):
    return rig.torch.from_numpy(np.array(values, np.uint32).view(np.int32).copy()).to(rig.dev)


def _src(rng, family):
    s = np.zeros(1, CM.HS_SRC)
    s["addr"][0] = np.frombuffer(rng.bytes(16), np.uint8)  # (an IPv4 source keeps random bytes behind its address)
    s["port"][0] = np.frombuffer(rng.bytes(2), np.uint8)
    s["family"] = family
    s["_pad"][0] = np.frombuffer(rng.bytes(5), np.uint8)
    return s[0]


def _datagram(rng, kind, secret):
    """(bytes in the ring, stated length, source, whether the position's nonce is zero) for one datagram."""
    fam = 6 if kind == "ok6" or rng.random() < 0.4 else 4
    if kind == "ok4":
        fam = 4
    if kind == "fam0":
        fam = int(rng.choice([0, 5, 7, 255]))
    s = _src(rng, fam)
    t = 2 if kind in ("r_ok", "r_zero") else 1
    L = 148 if t == 1 else 92
    m = HM.message(t, rng.bytes(120), PUB)
    wl, zero_nonce = L, kind in ("zn_need", "zn_ok")
    if kind in ("ok4", "ok6", "zn_ok", "r_ok", "flip0", "flip15"):
        m = CM.with_mac2(m, CM.cookie_of_src(secret, s))
        if kind == "flip0":
            m = m[:L - 16] + bytes([m[L - 16] ^ 0x01]) + m[L - 15:]
        if kind == "flip15":
            m = m[:L - 1] + bytes([m[L - 1] ^ 0x80])
    elif kind == "port":
        other = s.copy()
        other["port"][1] ^= 1
        m = CM.with_mac2(m, CM.cookie_of_src(secret, other))
    elif kind == "fam0":
        m = m[:L - 16] + rng.bytes(16)
    elif kind == "size":
        wl = int(rng.choice([147, 149, 91, 93]))
        m = (m + rng.bytes(2))[:wl] if wl in (147, 149) else (HM.message(2, rng.bytes(120), PUB) + rng.bytes(2))[:wl]
    elif kind == "mac1":
        m = m[:L - 20] + bytes([m[L - 20] ^ 4]) + m[L - 19:]
    elif kind == "type":
        m = bytes([3]) + m[1:]
    elif kind == "transport":
        wl = int(rng.integers(32, 100))
        m = struct.pack("<BxxxIQ", 4, 7, 1) + rng.bytes(wl - 16)
    return m, wl, s, zero_nonce


def _ring(rng, n_list, secret=SECRET, interleave=False, kinds=None):
    """A ring whose listed datagrams (type 1 or 2, in bounds) number n_list, at every alignment of the ring offset;
    with `interleave`, transport packets, type-3 datagrams and a datagram past the ring lie between them."""
    buf, off, lens, src, zn = bytearray(rng.bytes(1)), [], [], [], []
    pool = kinds or KINDS
    listed = 0
    tail = 1 if interleave else 0  # (the plan's ring never ends with a listed datagram, and is never empty)
    while listed < n_list or tail:
        if interleave and (listed == n_list or rng.random() < 0.3):
            tail -= listed == n_list
            kind = UNLISTED[int(rng.integers(0, len(UNLISTED)))]
        else:
            kind = pool[listed % len(pool)] if listed < 2 * len(pool) else pool[int(rng.integers(0, len(pool)))]
            listed += 1
        m, wl, s, z = _datagram(rng, kind, secret)
        off.append(len(buf) if kind != "bounds" else 1 << 40)
        lens.append(wl)
        src.append(s)
        zn.append(z)
        buf += m + rng.bytes(int(rng.integers(0, 4)))
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    return (ring, np.array(off, np.uint64), np.array(lens, np.uint32), np.array(src, CM.HS_SRC).reshape(-1), zn)


def _nonces(rng, lst, zn):
    """24 random bytes per list position, zeros where the datagram of that position asks for them"""
    return b"".join(bytes(24) if zn[i] else rng.bytes(24) for i in lst)


class _Admit:
    """Device buffers of one admit over n datagrams, guards behind every output."""

    def __init__(self, rig, n, ring_size):
        torch, dev = rig.torch, rig.dev
        self.rig, self.n = rig, n
        self.d_ring = torch.zeros(max(ring_size, 1), dtype=torch.uint8, device=dev)
        self.d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        self.d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_src = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
        self.d_non = torch.zeros((n + 1, 24), dtype=torch.uint8, device=dev)
        self.d_st = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        self.d_rec = torch.zeros((n + 1, 160), dtype=torch.uint8, device=dev)
        self.d_sum = torch.zeros(8, dtype=torch.int32, device=dev)
        self.d_rep = torch.zeros((n + 1, 80), dtype=torch.uint8, device=dev)
        self.d_asum = torch.zeros(8, dtype=torch.int32, device=dev)
        # the plan's outputs
        self.d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        self.p_st = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_host = torch.zeros(n, dtype=torch.int32, device=dev)
        self.p_sum = torch.zeros(2, dtype=torch.int64, device=dev)

    def load(self, ring, off, lens, src, nonces):
        torch, n = self.rig.torch, self.n
        self.d_ring.zero_()
        self.d_ring[:len(ring)].copy_(torch.from_numpy(ring))
        self.d_off.copy_(torch.from_numpy(off.view(np.int64)))
        self.d_len.copy_(torch.from_numpy(lens.view(np.int32)))
        if n:
            self.d_src.copy_(torch.from_numpy(src.view(np.uint8).reshape(n, 24)))
        self.d_non.fill_(0x7E)
        nl = len(nonces) // 24
        if nl:
            self.d_non[:nl].copy_(torch.from_numpy(np.frombuffer(nonces, np.uint8).reshape(nl, 24).copy()))
        self.d_st.fill_(GUARD)
        self.d_rec.fill_(0x7E)
        self.d_sum.fill_(GUARD)
        self.d_rep.fill_(0x7E)
        self.d_asum.fill_(GUARD)

    def run(self, eng=None, plan=False, max_len=120):
        eng, n = eng or self.rig.eng, self.n
        kw = {}
        if plan:
            eng.rx_plan(self.d_ring, self.d_off, self.d_len, self.d_desc, self.p_st, self.d_host, self.p_sum, max_len)
            kw = dict(host_list=self.d_host, rx_summary=self.p_sum)
        eng.hs_admit(self.d_ring, self.d_off, self.d_len, self.d_src, self.d_non[:n], self.d_st[:n], self.d_rec[:n],
                     self.d_sum[:4], self.d_rep[:n], self.d_asum[:4], **kw)

    def read(self, nl):
        """Everything the call may have written, after the guard checks."""
        self.rig.torch.cuda.synchronize()
        n = self.n
        st, rec, sm = self.d_st.cpu().numpy(), self.d_rec.cpu().numpy(), self.d_sum.cpu().numpy()
        rep, asm, non = self.d_rep.cpu().numpy(), self.d_asum.cpu().numpy(), self.d_non.cpu().numpy()
        assert (sm[4:] == GUARD).all() and (asm[4:] == GUARD).all(), "summary guard overwritten"
        s = dict(n_valid=int(sm[0]), n_init=int(sm[1]), n_resp=int(sm[2]), n_rejected=int(sm[3]))
        a = dict(n_replies=int(asm[0]), n_mac2_ok=int(asm[1]), n_nononce=int(asm[2]), n_badsrc=int(asm[3]))
        assert (st[nl:] == GUARD).all(), "hs_status written past the list"
        assert s["n_valid"] <= n and (rec[s["n_valid"]:] == 0x7E).all(), "records written past n_valid"
        assert a["n_replies"] <= n and (rep[a["n_replies"]:] == 0x7E).all(), "replies written past n_replies"
        assert (non[nl:] == 0x7E).all(), "nonces written past the list"
        return (st[:nl].tolist(), np.ascontiguousarray(rec[:s["n_valid"]]).view(HM.HS_RECORD).reshape(-1), s,
                np.ascontiguousarray(rep[:a["n_replies"]]).view(CM.HS_COOKIE_REPLY).reshape(-1), a, non[:nl].tobytes())


def _same_admit(got, want):
    assert got[0] == want[0], [(k, a, b) for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:5]
    assert got[2] == want[2] and got[4] == want[4], (got[2], want[2], got[4], want[4])
    assert got[1].tobytes() == want[1].tobytes(), "records"
    if got[3].tobytes() != want[3].tobytes():
        bad = [j for j in range(len(want[3])) if got[3][j].tobytes() != want[3][j].tobytes()][:2]
        raise AssertionError(("replies", bad, [(got[3][j], want[3][j]) for j in bad]))
    assert got[5] == want[5], "nonces after the call"


# ---- wg_hs_admit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [False, True], ids=["identity", "host_list"])
@pytest.mark.parametrize("n_list", LIST_LENGTHS)
def test_admit_over_list_lengths(rig, n_list, plan):
    """Every kind of datagram, at odd ring offsets, through the identity list and through the plan's host_list (with
    transport packets, type-3 datagrams and a datagram past the ring between the listed ones)."""
    rng = np.random.default_rng(7200 + 2 * n_list + plan)
    ring, off, lens, src, zn = _ring(rng, n_list, interleave=plan)
    n = len(off)
    if plan:
        _, _, lst, _ = RM.plan(ring, off, lens, SESS, max_len=120, mode=RM.PT_AFTER)
    else:
        lst = list(range(n))
    assert len(lst) == n_list and (n_list < 65 or {int(o) & 3 for o in off if o < (1 << 40)} == {0, 1, 2, 3})
    nonces = _nonces(rng, lst, zn)
    ad = _Admit(rig, n, len(ring))
    ad.load(ring, off, lens, src, nonces)
    ad.run(plan=plan)
    got = ad.read(n_list)
    want = CM.admit(ring, off, lens, src, nonces, PUB, SECRET, lst=lst if plan else None)
    _same_admit(got, want)
    if plan:
        assert ad.d_host.cpu().numpy()[:n_list].tolist() == lst
    if n_list >= 63:  # the mix did not degenerate (positions 0 .. 25 hold every kind twice; five kinds need a cookie)
        assert set(want[0]) == {CM.HS_OK, CM.HS_BADLEN, CM.HS_BADMAC1, CM.HS_BADSRC, CM.HS_NONONCE, CM.HS_NEEDCOOKIE}
        assert want[2]["n_resp"] > 0 and want[4]["n_replies"] >= 10
        assert {int(r["msg"][0]) for r in want[3]} == {3} and want[4]["n_mac2_ok"] == want[2]["n_valid"]


def test_admit_identity_list_rejects_other_types_and_bounds(rig):
    """The identity list also meets what the plan never lists: type 3 (BADTYPE) and a datagram past the ring."""
    rng = np.random.default_rng(7300)
    ring, off, lens, src, zn = _ring(rng, 40, kinds=["ok4", "zero", "type", "bounds"])
    n = len(off)
    nonces = _nonces(rng, range(n), zn)
    ad = _Admit(rig, n, len(ring))
    ad.load(ring, off, lens, src, nonces)
    ad.run()
    want = CM.admit(ring, off, lens, src, nonces, PUB, SECRET)
    _same_admit(ad.read(n), want)
    assert set(want[0]) == {CM.HS_OK, CM.HS_NEEDCOOKIE, CM.HS_BADTYPE, CM.HS_BADLEN}


@pytest.mark.parametrize("kind", ["zero", "ok6"])
def test_admit_rings_of_one_status(rig, kind):
    """257 positions that all need a cookie, and 257 that are all accepted: each compaction rank alone."""
    rng = np.random.default_rng(7400 + len(kind))
    ring, off, lens, src, zn = _ring(rng, 257, kinds=[kind])
    nonces = _nonces(rng, range(257), zn)
    ad = _Admit(rig, 257, len(ring))
    ad.load(ring, off, lens, src, nonces)
    ad.run()
    want = CM.admit(ring, off, lens, src, nonces, PUB, SECRET)
    _same_admit(ad.read(257), want)
    assert (want[4]["n_replies"], want[2]["n_valid"]) == ((257, 0) if kind == "zero" else (0, 257))
    assert (want[5] == bytes(24 * 257)) == (kind == "zero")


def test_secret_rotation(rig):
    """After wg_hs_cookie_secret_set, yesterday's mac2 needs a cookie again."""
    rng = np.random.default_rng(7500)
    ring, off, lens, src, zn = _ring(rng, 70, kinds=["ok4", "ok6", "r_ok"])
    nonces = _nonces(rng, range(70), zn)
    ad = _Admit(rig, 70, len(ring))
    try:
        ad.load(ring, off, lens, src, nonces)
        ad.run()
        _same_admit(ad.read(70), CM.admit(ring, off, lens, src, nonces, PUB, SECRET))
        assert ad.d_sum.cpu().numpy()[0] == 70 and ad.d_sum.cpu().numpy()[2] > 0
        rig.eng.hs_cookie_secret_set(SECRET2)
        ad.load(ring, off, lens, src, nonces)
        ad.run()
        want = CM.admit(ring, off, lens, src, nonces, PUB, SECRET2)
        _same_admit(ad.read(70), want)
        assert want[0] == [CM.HS_NEEDCOOKIE] * 70
    finally:
        rig.eng.hs_cookie_secret_set(SECRET)


def test_captured_plan_and_admit_replay(rig):
    """plan + admit captured once. Replayed with fresh nonces it equals the model (and so the eager call); replayed
    without, it sends no reply and every position that needs a cookie answers NONONCE; a new secret between replays
    needs no re-capture. A capturing admit that would have to grow its scratch: WG_EINVAL."""
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    rng = np.random.default_rng(7600)
    ring, off, lens, src, zn = _ring(rng, 300, interleave=True)
    n = len(off)
    _, _, lst, _ = RM.plan(ring, off, lens, SESS, max_len=120, mode=RM.PT_AFTER)
    nonces = _nonces(rng, lst, zn)
    ad = _Admit(rig, n, len(ring))
    eng.rx_reserve(n)
    eng.hs_reserve(n)
    ad.load(ring, off, lens, src, nonces)
    ad.run(plan=True)  # eager once
    want = CM.admit(ring, off, lens, src, nonces, PUB, SECRET, lst=lst)
    _same_admit(ad.read(300), want)
    big = 400000  # more than anything in this module reserved
    b_off = torch.zeros(big, dtype=torch.int64, device=dev)
    b_len = torch.zeros(big, dtype=torch.int32, device=dev)
    b_st = torch.zeros(big, dtype=torch.int32, device=dev)
    b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)
    b_src = torch.zeros((big, 24), dtype=torch.uint8, device=dev)
    b_non = torch.zeros((big, 24), dtype=torch.uint8, device=dev)
    b_rep = torch.zeros((big, 80), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(W.WgError) as e:
            eng.hs_admit(ad.d_ring, b_off, b_len, b_src, b_non, b_st, b_rec, ad.d_sum[:4], b_rep, ad.d_asum[:4])
        ad.run(plan=True)
    assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
    try:
        ad.load(ring, off, lens, src, nonces)
        torch.cuda.synchronize()
        g.replay()
        _same_admit(ad.read(300), want)
        # the nonces were consumed: the same graph again, outputs reset, nonces left as the replay left them
        after = want[5]
        for t in (ad.d_st, ad.d_sum, ad.d_asum):
            t.fill_(GUARD)
        ad.d_rec.fill_(0x7E)
        ad.d_rep.fill_(0x7E)
        torch.cuda.synchronize()
        g.replay()
        got = ad.read(300)
        stale = CM.admit(ring, off, lens, src, after, PUB, SECRET, lst=lst)
        _same_admit(got, stale)
        assert stale[4]["n_replies"] == 0 and len(got[3]) == 0
        assert [b for a, b in zip(want[0], stale[0]) if a == CM.HS_NEEDCOOKIE] == [CM.HS_NONONCE] * want[4]["n_replies"]
        assert stale[2] == want[2] and stale[1].tobytes() == want[1].tobytes()  # the accepted ones are accepted again
        # a new secret, fresh nonces, the same graph
        eng.hs_cookie_secret_set(SECRET2)
        ad.load(ring, off, lens, src, nonces)
        torch.cuda.synchronize()
        g.replay()
        rot = CM.admit(ring, off, lens, src, nonces, PUB, SECRET2, lst=lst)
        _same_admit(ad.read(300), rot)
        assert rot[2]["n_valid"] == 0 and rot[4]["n_replies"] > want[4]["n_replies"]
    finally:
        eng.hs_cookie_secret_set(SECRET)


# ---- wg_hs_cookie_open, the table, wg_hs_mac2 ---------------------------------------------------------------------
def initiator(rig):
    eng = rig.W.Engine(0, key_slots=4)
    eng.hs_static_set(A_PRIV)
    eng.hs_peers_set(PEERS)
    return eng


def _sent_and_pending(rng, n_pending):
    """Pending entries and the records sent for them: only the indices, the peers and the records' mac1 matter here.
    Entry 5 shares entry 2's index, entry 4 is empty, entry 3's peer is past the table."""
    sent = np.zeros(n_pending, HM.HS_RECORD)
    pend = np.zeros(n_pending, CM.HS_PENDING)
    for q in range(n_pending):
        peer = (3 * q + 1) % 4
        li = (0x00C0FFEE + 0x9E3779B1 * q) & 0xFFFFFFFF
        m = HM.message(1, bytes(3) + li.to_bytes(4, "little") + rng.bytes(108), PEERS[peer])
        sent[q] = (q, 148, np.frombuffer(m, np.uint8), 0)
        pend[q]["state"], pend[q]["peer"], pend[q]["local_index"] = 1, peer, li
        for f in ("ephemeral", "hash", "chain_key"):
            pend[q][f] = np.frombuffer(rng.bytes(32), np.uint8)
    if n_pending > 8:
        pend[4] = np.zeros(1, CM.HS_PENDING)[0]
        pend[5]["local_index"] = pend[2]["local_index"]
        pend[3]["peer"] = 9
    return sent, pend


def _reply_to(rng, sent, pend, q, peer=None):
    """The peer's cookie reply to pending entry q (a fresh cookie each time)."""
    p = int(pend[q]["peer"]) % 4 if peer is None else peer
    m = sent[q]["msg"].tobytes()
    return CM.reply(PEERS[p], int(pend[q]["local_index"]).to_bytes(4, "little"), rng.bytes(24), rng.bytes(16), m[116:132])


FORGERIES = [4, 8, 23, 24, 31, 32, 47, 63]  # a bit in the receiver, nonce bytes 0 / 15 / 16 / 23, the ciphertext's ends, tag byte 15


def _reply_ring(rng, sent, pend, n):
    """n datagrams: replies (the first of them to entries 0, 1, 2, ... so that peers repeat), and among them transport
    packets, initiations, 63- and 65-byte type-3 datagrams, garbage, a datagram past the ring, replies to unknown
    indices and to the special entries, and one forgery of each kind."""
    npend = len(pend)
    buf, off, lens = bytearray(rng.bytes(3)), [], []
    for j in range(n):
        kind = j % 16
        q = (j // 2) % max(npend, 1)
        if not npend:
            m = CM.reply(PEERS[0], rng.bytes(4), rng.bytes(24), rng.bytes(16), rng.bytes(16))
        else:
            m = _reply_to(rng, sent, pend, q)
        wl = 64
        if kind == 3:
            wl = int(rng.integers(32, 100))
            m = struct.pack("<BxxxIQ", 4, 7, j) + rng.bytes(wl - 16)
        elif kind == 5:
            m, wl = HM.message(1, rng.bytes(120), PUB), 148
        elif kind == 7:
            wl = 63 if j % 32 == 7 else 65
            m = (m + rng.bytes(1))[:wl]
        elif kind == 9:
            m = bytes([int(rng.choice([0, 5, 255]))]) + rng.bytes(63)
        elif kind == 11:
            m = m[:4] + rng.bytes(4) + m[8:]  # an index nobody waits for
        elif kind == 13 and npend:
            at = FORGERIES[(j // 16) % len(FORGERIES)]
            m = m[:at] + bytes([m[at] ^ (1 << int(rng.integers(0, 8)))]) + m[at + 1:]
        off.append(len(buf) if kind != 15 else (1 << 41))
        lens.append(wl)
        buf += m + rng.bytes(int(rng.integers(0, 4)))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32)


def _table(eng, n=4):
    ck, have = eng.hs_cookies_get(0, n)
    return list(zip(ck, have))


def _cookie_open(rig, eng, ring, off, lens, sent, pend):
    """One wg_hs_cookie_open over guarded outputs: (status list, learned, summary dict, pending after, table after)."""
    torch, dev = rig.torch, rig.dev
    n, npend = len(off), len(pend)
    d_pend = t_u8(rig, pend.tobytes() + b"\x7e" * 112).reshape(npend + 1, 112)
    d_sent = t_u8(rig, sent.tobytes() + b"\x7e" * 160).reshape(npend + 1, 160)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_lrn = torch.full((n + 1, 16), 0x7E, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    eng.hs_cookie_open(t_u8(rig, ring), torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(lens.view(np.int32)).to(dev),
                       d_sent[:npend], d_pend[:npend], d_st[:n], d_lrn[:n], d_sum[:4])
    torch.cuda.synchronize()
    st, lrn, sm = d_st.cpu().numpy(), d_lrn.cpu().numpy(), d_sum.cpu().numpy()
    assert (st[n:] == GUARD).all() and (sm[4:] == GUARD).all()
    if n == 0:  # a no-op: not even the summary
        assert (sm == GUARD).all()
        sm = np.zeros(8, np.int32)
    s = dict(n_ok=int(sm[0]), n_nopending=int(sm[1]), n_badauth=int(sm[2]), n_skipped=int(sm[3]))
    assert s["n_ok"] <= n and (lrn[s["n_ok"]:] == 0x7E).all(), "learned written past n_ok"
    assert d_pend.cpu().numpy().tobytes() == pend.tobytes() + b"\x7e" * 112, "pending is read only"
    assert d_sent.cpu().numpy().tobytes() == sent.tobytes() + b"\x7e" * 160
    return st[:n].tolist(), np.ascontiguousarray(lrn[:s["n_ok"]]).view(CM.HS_LEARNED).reshape(-1), s, _table(eng)


@pytest.mark.parametrize("n,npend", [(0, 5), (1, 1), (64, 0), (65, 3), (257, 20), (600, 300)])
def test_cookie_open_against_the_model(rig, n, npend):
    rng = np.random.default_rng(7700 + n)
    eng = initiator(rig)
    try:
        sent, pend = _sent_and_pending(rng, npend)
        ring, off, lens = _reply_ring(rng, sent, pend, n)
        before = [(rng.bytes(16), True), (bytes(16), False), (rng.bytes(16), True), (bytes(16), False)]
        eng.hs_cookies_set(0, [c for c, _ in before], [h for _, h in before])
        assert _table(eng) == before
        got = _cookie_open(rig, eng, ring, off, lens, sent, pend)
        want = CM.cookie_open(ring, off, lens, sent, pend, PEERS, before)
        assert got[0] == want[0], [(k, a, b) for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:5]
        assert got[2] == want[2] and got[1].tobytes() == want[1].tobytes()
        assert got[3] == want[3], "the cookie table after the call"
        if n >= 257:
            assert set(want[0]) == {CM.CK_OK, CM.CK_NOPENDING, CM.CK_BADAUTH, CM.CK_SKIPPED, CM.CK_BADLEN}
            peers_ok = want[1]["peer"].tolist()
            assert len(peers_ok) > len(set(peers_ok)) == 4, "several valid replies for one peer"
            assert 2 in want[1]["pending"].tolist() and 5 not in want[1]["pending"].tolist()  # the shared index
    finally:
        eng.close()


def test_forged_replies_change_nothing(rig):
    """One authentic reply, then each forgery of it alone in a ring: BADAUTH (NOPENDING for the receiver's bit), and the
    cookie table and pending are byte for byte as they were."""
    rng = np.random.default_rng(7800)
    eng = initiator(rig)
    try:
        sent, pend = _sent_and_pending(rng, 3)
        good = _reply_to(rng, sent, pend, 1)
        before = [(rng.bytes(16), True), (rng.bytes(16), True), (bytes(16), False), (bytes(16), False)]
        eng.hs_cookies_set(0, [c for c, _ in before], [h for _, h in before])
        ring = np.frombuffer(b"".join(good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:] for at in FORGERIES), np.uint8).copy()
        off = 64 * np.arange(len(FORGERIES), dtype=np.uint64)
        lens = np.full(len(FORGERIES), 64, np.uint32)
        st, lrn, s, table = _cookie_open(rig, eng, ring, off, lens, sent, pend)
        assert st == [CM.CK_NOPENDING] + [CM.CK_BADAUTH] * (len(FORGERIES) - 1) and len(lrn) == 0 and table == before
        st, lrn, s, table = _cookie_open(rig, eng, np.frombuffer(good, np.uint8).copy(), off[:1], lens[:1], sent, pend)
        peer = int(pend[1]["peer"])
        assert st == [CM.CK_OK] and lrn.tolist() == [(0, 1, peer, 0)]
        assert table[peer][1] and table[peer][0] != before[peer][0] and [t for k, t in enumerate(table) if k != peer] == \
            [t for k, t in enumerate(before) if k != peer]
    finally:
        eng.close()


def _mac2(rig, eng, recs, peer, graph=None):
    torch, dev = rig.torch, rig.dev
    n = len(recs)
    d_rec = t_u8(rig, recs.tobytes() + b"\x7e" * 160).reshape(n + 1, 160)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    eng.hs_mac2(d_rec[:n], t_u32(rig, peer), d_st[:n], d_sum[:4])
    torch.cuda.synchronize()
    out, st, sm = d_rec.cpu().numpy().tobytes(), d_st.cpu().numpy().view(np.uint32), d_sum.cpu().numpy().view(np.uint32)
    assert out[160 * n:] == b"\x7e" * 160 and (st[n:] == GUARD).all() and (sm[4:] == GUARD).all()
    if n == 0:  # a no-op: not even the summary
        assert (sm == GUARD).all()
        sm = np.zeros(8, np.uint32)
    assert sm[3] == 0
    return np.frombuffer(out[:160 * n], HM.HS_RECORD), st[:n].tolist(), dict(n_ok=int(sm[0]), n_none=int(sm[1]), n_bad=int(sm[2]))


@pytest.mark.parametrize("n", [0, 1, 64, 257])
def test_mac2_against_the_model(rig, n):
    """Peers with and without a cookie, 148- and 92-byte records, bad lengths, peers past the table; only the 16 bytes
    of mac2 change (the whole record array is compared, the records' _pad and tail bytes are not zero)."""
    rng = np.random.default_rng(7900 + n)
    eng = initiator(rig)
    try:
        table = [(rng.bytes(16), True), (bytes(16), False), (rng.bytes(16), True), (bytes(16), False)]
        eng.hs_cookies_set(0, [c for c, _ in table], [h for _, h in table])
        recs = np.frombuffer(rng.bytes(160 * n), HM.HS_RECORD).copy()
        peer = []
        for k in range(n):
            recs[k]["len"] = [148, 92, 148, 148, 92, 0, 147, 148][k % 8]
            peer.append([0, 2, 1, 3, 0, 0, 2, 4 if k % 16 == 7 else 0xFFFFFFFF][k % 8])
        got = _mac2(rig, eng, recs, peer)
        want = CM.mac2_batch(recs, peer, table)
        assert got[1] == want[1] and got[2] == want[2]
        assert got[0].tobytes() == want[0].tobytes()
        if n >= 64:
            assert set(want[1]) == {CM.MAC2_OK, CM.MAC2_NONE, CM.MAC2_BADDESC, CM.MAC2_BADPEER}
    finally:
        eng.close()


def test_captured_initiate_and_mac2_follow_the_table(rig):
    """initiate + mac2 captured once; between replays the cookie table changes and the ephemerals are refreshed: the
    records' mac2 follows the table without re-capture."""
    torch, dev = rig.torch, rig.dev
    eng = initiator(rig)
    try:
        n = 70
        rng = np.random.default_rng(8000)
        peer = [k % 4 for k in range(n)]
        eph = rng.bytes(32 * n)
        d_peer, d_li = t_u32(rig, peer), t_u32(rig, [0x100 + k for k in range(n)])
        d_eph, d_ts = t_u8(rig, eph), t_u8(rig, rng.bytes(12 * n))
        d_st, d_sum = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        d_rec, d_pend = torch.zeros((n, 160), dtype=torch.uint8, device=dev), torch.zeros((n, 112), dtype=torch.uint8, device=dev)
        m_st, m_sum = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        eng.hs_reserve(n)

        def both():
            eng.hs_initiate(d_peer, d_eph, d_ts, d_li, d_st, d_rec, d_pend, d_sum)
            eng.hs_mac2(d_rec, d_peer, m_st, m_sum)

        both()  # eager once: no cookies yet
        torch.cuda.synchronize()
        plain = d_rec.cpu().numpy().reshape(-1).view(HM.HS_RECORD).copy()
        assert m_sum.cpu().numpy().tolist() == [0, n, 0, 0] and not plain["msg"][:, 132:].any() and d_sum.cpu().numpy()[0] == n
        g = torch.cuda.CUDAGraph()
        d_eph.copy_(t_u8(rig, eph))
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            both()
        for table in ([(rng.bytes(16), True), (bytes(16), False), (rng.bytes(16), True), (bytes(16), False)],
                      [(bytes(16), False), (rng.bytes(16), True), (bytes(16), False), (bytes(16), False)]):
            eng.hs_cookies_set(0, [c for c, _ in table], [h for _, h in table])
            d_eph.copy_(t_u8(rig, eph))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = CM.mac2_batch(plain, peer, table)
            assert d_rec.cpu().numpy().tobytes() == want[0].tobytes()
            assert m_st.cpu().numpy().tolist() == want[1] and m_sum.cpu().numpy().tolist()[:3] == list(want[2].values())
    finally:
        eng.close()


# ---- two contexts, end to end ----------------------------------------------------------------------------------------
def test_two_contexts_cookie_round_trip_then_a_whole_handshake(rig):
    """A initiates; B, under load, answers every initiation with a cookie reply; A opens the replies, initiates again
    and writes mac2; B admits, runs dh -> open -> stamp -> respond; A checks and finishes; both hold the same keys."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    from hs_respond_model import HS_SESSION
    import hs_initiate_model as IM
    n = 65
    A, B = W.Engine(0, key_slots=4), W.Engine(0, key_slots=4)
    try:
        b_priv = splitmix_bytes(0x7130, 32)
        a_pub, b_pub = A.hs_static_set(A_PRIV), B.hs_static_set(b_priv)
        A.hs_peers_set([b_pub])
        B.hs_peers_set([a_pub])
        B.hs_cookie_secret_set(SECRET)
        rng = np.random.default_rng(8100)
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        off148 = torch.arange(0, 148 * n, 148, dtype=torch.int64, device=dev)
        len148 = torch.full((n,), 148, dtype=torch.int32, device=dev)
        off92 = torch.arange(0, 92 * n, 92, dtype=torch.int64, device=dev)
        len92 = torch.full((n,), 92, dtype=torch.int32, device=dev)
        off64 = torch.arange(0, 64 * n, 64, dtype=torch.int64, device=dev)
        len64 = torch.full((n,), 64, dtype=torch.int32, device=dev)
        src = np.array([_src(rng, 4 if k % 2 else 6) for k in range(n)], CM.HS_SRC).reshape(-1)  # all from A's one address
        src[:] = src[0]
        d_src = t_u8(rig, src.tobytes()).reshape(n, 24)
        peer, a_st, a_sum, a_rec, pend = z32(n), z32(n), z32(4), z8(n, 160), z8(n, 112)
        a_li = t_u32(rig, [0x4000 + 3 * k for k in range(n)])
        ts = t_u8(rig, b"".join(bytes(4) + (0x4000000000000000 + k).to_bytes(8, "big") for k in range(n)))
        b_st, b_sum, b_rec, b_rep, b_asum = z32(n), z32(4), z8(n, 160), z8(n, 80), z32(4)
        # 1-2. A initiates, B admits: every message needs a cookie
        A.hs_initiate(peer, t_u8(rig, rng.bytes(32 * n)), ts, a_li, a_st, a_rec, pend, a_sum)
        ring = a_rec[:, 8:156].contiguous().reshape(-1)
        B.hs_admit(ring, off148, len148, d_src, t_u8(rig, rng.bytes(24 * n)).reshape(n, 24), b_st, b_rec, b_sum, b_rep, b_asum)
        torch.cuda.synchronize()
        assert a_sum.cpu().numpy().tolist() == [n, 0, 0, 0] and b_sum.cpu().numpy().tolist() == [0, 0, 0, n]
        assert b_asum.cpu().numpy().tolist() == [n, 0, 0, 0] and (b_st.cpu().numpy() == CM.HS_NEEDCOOKIE).all()
        # 3-4. B's replies are A's ring; A learns B's cookie
        ring64 = b_rep[:, 8:72].contiguous().reshape(-1)
        c_st, c_lrn, c_sum = z32(n), z8(n, 16), z32(4)
        A.hs_cookie_open(ring64, off64, len64, a_rec, pend, c_st, c_lrn, c_sum)
        torch.cuda.synchronize()
        assert c_sum.cpu().numpy().tolist() == [n, 0, 0, 0]
        ck, have = A.hs_cookies_get(0, 1)
        assert have == [True] and ck[0] == CM.cookie_of_src(SECRET, src[0])
        # 5-6. A initiates again (newer timestamps) with mac2; B admits all of them
        ts2 = t_u8(rig, b"".join(bytes(4) + (0x4000000000001000 + k).to_bytes(8, "big") for k in range(n)))
        m_st, m_sum = z32(n), z32(4)
        A.hs_initiate(peer, t_u8(rig, rng.bytes(32 * n)), ts2, a_li, a_st, a_rec, pend, a_sum)
        A.hs_mac2(a_rec, peer, m_st, m_sum)
        ring = a_rec[:, 8:156].contiguous().reshape(-1)
        B.hs_admit(ring, off148, len148, d_src, t_u8(rig, rng.bytes(24 * n)).reshape(n, 24), b_st, b_rec, b_sum, b_rep, b_asum)
        # 7. dh -> open -> stamp -> respond: only the newest initiation of the one peer is answered
        b_sh, b_dh, b_ost, b_init, b_osum = z8(n, 32), z32(n), z32(n), z8(n, 144), z32(4)
        s_st, s_open, s_fresh, s_sum = z32(n), z8(n, 12), z8(n, 144), z32(4)
        b_li, b_rst, b_sess, b_rsum = t_u32(rig, [0x80000000 + k for k in range(n)]), z32(n), z8(n, 176), z32(4)
        B.hs_dh(b_rec, b_sum, b_sh, b_dh)
        B.hs_open(b_rec, b_sum, b_sh, b_dh, b_ost, b_init, b_osum)
        B.hs_stamp(b_init, b_osum, b_rec, b_sh, s_st, s_open, s_fresh, s_sum)
        B.hs_respond(s_fresh, s_sum, t_u8(rig, rng.bytes(32 * n)), b_li, b_rst, b_sess, b_rsum)
        torch.cuda.synchronize()
        assert m_sum.cpu().numpy().tolist() == [n, 0, 0, 0]
        assert b_sum.cpu().numpy().tolist() == [n, n, 0, 0] and b_asum.cpu().numpy().tolist() == [0, n, 0, 0]
        assert b_osum.cpu().numpy().tolist() == [n, n, 0, 0]
        assert s_sum.cpu().numpy().tolist() == [1, n - 1, 0, 0] and b_rsum.cpu().numpy().tolist() == [1, 0, 0, 0]
        # 8-9. A checks B's response and finishes
        ring92 = b_sess[:1, 16:108].contiguous().reshape(-1)
        f_hst, f_hsum, f_rec = z32(1), z32(4), z8(1, 160)
        f_st, f_est, f_sum = z32(1), z8(1, 96), z32(4)
        A.hs_check(ring92, off92[:1], len92[:1], f_hst, f_rec, f_hsum)
        A.hs_finish(f_rec, f_hsum, pend, f_st, f_est, f_sum)
        torch.cuda.synchronize()
        assert f_hsum.cpu().numpy().tolist() == [1, 0, 1, 0] and f_sum.cpu().numpy().tolist() == [1, 0, 0, 0]
        est = f_est.cpu().numpy().reshape(-1).view(IM.HS_ESTABLISHED)[0]
        sess = b_sess.cpu().numpy().reshape(-1).view(HS_SESSION)[0]
        assert int(est["pending"]) == n - 1 and int(est["local_index"]) == int(sess["remote_index"]) == 0x4000 + 3 * (n - 1)
        assert est["send_key"].tobytes() == sess["recv_key"].tobytes() and est["recv_key"].tobytes() == sess["send_key"].tobytes()
        assert est["send_key"].any() and est["send_key"].tobytes() != est["recv_key"].tobytes()
    finally:
        A.close()
        B.close()


# ---- errors and state ------------------------------------------------------------------------------------------------
def test_errors_and_state(rig):
    torch, dev, W = rig.torch, rig.dev, rig.W
    EINVAL, ENOKEY, ERANGE = W._lib.WG_EINVAL, W._lib.WG_ENOKEY, W._lib.WG_ERANGE
    rng = np.random.default_rng(8200)
    ring, off, lens, src, zn = _ring(rng, 8, kinds=["zero", "ok4"])
    nonces = _nonces(rng, range(8), zn)
    eng = W.Engine(0, key_slots=4)
    try:
        ad = _Admit(rig, 8, len(ring))
        ad.load(ring, off, lens, src, nonces)

        def code(fn):
            with pytest.raises(W.WgError) as e:
                fn()
            return e.value.code

        assert code(lambda: ad.run(eng)) == ENOKEY  # no key
        eng.hs_key_set(PUB)
        assert code(lambda: ad.run(eng)) == ENOKEY  # a key, no secret
        eng.hs_cookie_secret_set(SECRET)
        ad.run(eng)
        _same_admit(ad.read(8), CM.admit(ring, off, lens, src, nonces, PUB, SECRET))
        # overlaps: replies over records, nonces over src, admit_summary over summary
        args = lambda **kw: {**dict(wire=ad.d_ring, pkt_off=ad.d_off, pkt_len=ad.d_len, src=ad.d_src, nonces=ad.d_non[:8],  # noqa: E731
                                    hs_status=ad.d_st[:8], records=ad.d_rec[:8], hs_summary=ad.d_sum[:4], replies=ad.d_rep[:8],
                                    admit_summary=ad.d_asum[:4]), **kw}
        assert code(lambda: eng.hs_admit(**args(replies=ad.d_rec.reshape(-1)[80:].reshape(-1, 80)[:8]))) == EINVAL
        assert code(lambda: eng.hs_admit(**args(nonces=ad.d_src))) == EINVAL
        assert code(lambda: eng.hs_admit(**args(admit_summary=ad.d_sum[:4]))) == EINVAL
        assert code(lambda: eng.hs_admit(**args(nonces=ad.d_non.reshape(-1)[8:8 + 24 * 8]))) == EINVAL  # not 16-byte aligned
        # the cookie calls of a context without a private key or peers
        z = torch.zeros(64, dtype=torch.int32, device=dev)
        assert code(lambda: eng.hs_cookie_open(ad.d_ring, ad.d_off, ad.d_len, ad.d_rec[:0], ad.d_rec[:0, :112], z[:8], ad.d_rep[:8, :16],
                                                z[8:12])) == ENOKEY
        assert code(lambda: eng.hs_cookies_get(0, 1)) == ERANGE
        eng.hs_cookies_set(0, [], [])
        eng.hs_static_set(A_PRIV)
        eng.hs_peers_set(PEERS)
        # a capturing stream without a reserve
        eng.hs_reserve(16)
        big = 300000
        b_off = torch.zeros(big, dtype=torch.int64, device=dev)
        b_len = torch.zeros(big, dtype=torch.int32, device=dev)
        b_st = torch.zeros(big, dtype=torch.int32, device=dev)
        b_lrn = torch.zeros((big, 16), dtype=torch.uint8, device=dev)
        b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c1 = code(lambda: eng.hs_cookie_open(ad.d_ring, b_off, b_len, ad.d_rec[:0], ad.d_rec[:0, :112], b_st, b_lrn, z[8:12]))
            c2 = code(lambda: eng.hs_mac2(b_rec, b_st, b_len, z[8:12]))
            eng.hs_mac2(b_rec[:8], b_st[:8], b_len[:8], z[8:12])
        assert c1 == EINVAL and c2 == EINVAL
        # the table: a round trip, ranges, and a new peer table clears it
        cookies = [rng.bytes(16) for _ in range(4)]
        eng.hs_cookies_set(0, cookies, [True, False, True, True])
        assert _table(eng) == [(cookies[0], True), (bytes(16), False), (cookies[2], True), (cookies[3], True)]
        eng.hs_cookies_set(2, [bytes(16)], [False])  # the host expires one
        assert eng.hs_cookies_get(1, 3) == ([bytes(16), bytes(16), cookies[3]], [False, False, True])
        assert code(lambda: eng.hs_cookies_set(3, cookies[:2], [True, True])) == ERANGE
        assert code(lambda: eng.hs_cookies_get(0, 5)) == ERANGE
        eng.hs_peers_set(PEERS[::-1])
        assert _table(eng) == [(bytes(16), False)] * 4
        eng.hs_peers_set(PEERS[:2])
        assert code(lambda: eng.hs_cookies_get(0, 3)) == ERANGE and _table(eng, 2) == [(bytes(16), False)] * 2
    finally:
        eng.close()
