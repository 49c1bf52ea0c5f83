"""wg_hs_stamp, wg_hs_stamps_set and wg_hs_stamps_get on the MI355X against tests/hs_stamp_model.py (pytest -m gpu):
statuses, opened timestamps, fresh entries, summaries and stored stamps are compared exactly, and every output array
carries guard bytes or words behind what the call may write. Every run is the full chain plan -> check -> dh -> open ->
stamp on the current stream with no host read in between. The initiations come from test_gpu_hs_open's pool of 24
(ephemeral, initiator) pairs, re-sealed with other timestamps, which costs no new ladder."""
import ctypes
import functools

import numpy as np
import pytest

import hs_initiate_model as IM
import hs_model as HM
import hs_open_model as OM
import hs_respond_model as RM
import hs_stamp_model as SM
import x25519_model as M
from test_gpu_hs_open import EPHK, INITK, _flip, _OpenChain, _pub
from test_gpu_hs_respond import _same as _same_sessions
from test_gpu_x25519 import FILL, GUARD, SESS, STATIC, STATIC2, _engine, _Memo, model
from wgtest import noise, splitmix_np, wg

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 600]  # a wave, one range of 256 records, three ranges
ZERO = bytes(12)
P9 = bytes(range(0x10, 0x19))
S0 = P9 + b"\x00\x00\x80"  # the stored timestamp the ordering cases are measured against


def _t(v: int) -> bytes:
    return int(v).to_bytes(12, "big")


# six timestamps for the random rings: zero, values around two stored ones, and the greatest there is
TSET = [ZERO, _t(5), _t(6), _t((7 << 64) + 1), _t((7 << 64) + (1 << 32)), b"\xff" * 12]


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    yield type("Rig", (), dict(eng=None, torch=torch, dev=torch.device("cuda", 0), W=wg()))


@functools.lru_cache(maxsize=None)
def _hello(responder, k, ts):
    """Pool entry k's genuine initiation to the responder with this private key, sealed with this timestamp."""
    with _Memo():
        return OM.initiate(INITK[k % 6], _pub(responder), EPHK[k], ts)


def _msg(responder, k, ts, sender=0x1000, flip=None):
    """The 148-byte message; flip = (offset in msg[1 .. 116), bit) is made before mac1 is computed."""
    b = OM.body(sender, _hello(responder, k, ts))
    if flip is not None:
        b = _flip(b, *flip)
    return HM.message(1, b, _pub(responder))


def _ring(msgs, rng=None):
    """A UDP ring of these handshake messages at unaligned offsets (rng: with transport packets among them)."""
    import struct
    buf, off, lens = bytearray(b"\x00\x00\x00"), [], []
    known = list(SESS.keys())
    for k, m in enumerate(msgs):
        off.append(len(buf))
        lens.append(len(m))
        buf.extend(m + bytes(k % 4))
        for _ in range(int(rng.integers(0, 3)) if rng is not None else 0):
            wl = int(rng.integers(32, 90))
            off.append(len(buf))
            lens.append(wl)
            buf.extend(struct.pack("<BxxxIQ", 4, known[int(rng.integers(0, len(known)))], k) + rng.bytes(wl - 16))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32)


ETS_FLIPS = [87, 98, 99, 114]  # in msg[1 .. 116): ets' first and last ciphertext byte, its first and last tag byte


def _stamp_ring(rng, n_list, responder, epoch=0, tset=None):
    """n_list handshake datagrams among transport packets: initiations of known (pool entries with k % 6 < 4) and
    unknown initiators with timestamps of TSET (epoch > 0: later ones, the same otherwise), as they are, with a
    flipped bit in encrypted_static (they never reach the stamp) or in encrypted_timestamp at one of ETS_FLIPS;
    responses; messages with a flipped mac1 bit."""
    pub = _pub(responder)
    tset = tset or TSET
    msgs = []
    for k in range(n_list):
        r = rng.random()
        forced = k in (0, 63, 64, 255, 256, 599)
        sender, pool, ts, q, at, bit = (int(rng.integers(0, 1 << 32)), int(rng.integers(0, 24)), tset[int(rng.integers(0, 6))],
                                        rng.random(), int(rng.integers(0, 4)), int(rng.integers(0, 8)))
        filler = rng.bytes(120)
        if epoch:
            ts = _t(min(int.from_bytes(ts, "big") + epoch, (1 << 96) - 1))
        if forced or r < 0.6:
            flip = None if forced or q >= 0.3 else (int(39 + 8 * at), bit) if q < 0.08 else (ETS_FLIPS[at], bit)
            msgs.append(_msg(responder, pool, ts, sender, flip))
        elif r < 0.8:
            msgs.append(HM.message(2, filler[:59], pub))
        else:
            m = HM.message(1 + (bit & 1), filler, pub)
            msgs.append(_flip(m, len(m) - 32 + at, 2))
    return _ring(msgs, rng)


class _StampChain(_OpenChain):
    """plan -> check -> dh -> open -> stamp (-> respond) back to back on the current stream."""

    def __init__(self, rig, n, ring_size, respond=False):
        super().__init__(rig, n, ring_size)
        torch, dev = rig.torch, rig.dev
        self.respond = respond
        self.s_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        self.s_op = torch.full((12 * (n + 1),), 0x7E, dtype=torch.uint8, device=dev)
        self.s_fresh = torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev)
        self.s_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
        self.r_eph = torch.zeros((n + 1) * 32, dtype=torch.uint8, device=dev)
        self.r_li = torch.zeros(n, dtype=torch.int32, device=dev)
        self.r_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        self.r_sess = torch.full((n + 1, 176), 0x7E, dtype=torch.uint8, device=dev)
        self.r_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)

    def refresh(self, seed):
        """New ephemerals and session indices, in place (what the host does between replays)."""
        torch, n = self.rig.torch, self.n
        self.eph = bytes(splitmix_np(seed, 32 * n)) + bytes([FILL]) * 32
        self.li = [(0x02000000 + seed * 4096 + k) & 0xFFFFFFFF for k in range(n)]
        self.r_eph.copy_(torch.from_numpy(np.frombuffer(self.eph, np.uint8).copy()))
        self.r_li.copy_(torch.from_numpy(np.array(self.li, np.uint32).view(np.int32)))

    def load(self, ring, off, lens):
        super().load(ring, off, lens)
        for t, v in ((self.s_st, GUARD), (self.s_op, 0x7E), (self.s_fresh, 0x7E), (self.s_sum, GUARD), (self.r_st, GUARD),
                     (self.r_sess, 0x7E), (self.r_sum, GUARD)):
            t.fill_(v)

    def run(self, with_summary=True, stamp_summary=True):
        super().run(with_summary)
        n, eng = self.n, self.rig.eng
        eng.hs_stamp(self.o_init[:n], self.o_sum[:4] if stamp_summary else None, self.d_rec[:n], self.d_shared[:n],
                     self.s_st[:n], self.s_op[:12 * n], self.s_fresh[:n], self.s_sum[:4])
        if self.respond:
            eng.hs_respond(self.s_fresh[:n], self.s_sum[:4], self.r_eph[:32 * n], self.r_li, self.r_st[:n], self.r_sess[:n],
                           self.r_sum[:4], skip_newpeer=True)

    def compare_stamp(self, pub, private, peers, stored, with_summary=True, stamp_summary=True):
        """The earlier stages against their models, then the stamp's four outputs, whole, and the stored stamps, against
        hs_stamp_model over what the device holds. `stored` (a list of 12-byte strings, one per peer) is what the table
        held before the run; it is updated. Returns (status list of the covered entries, the entries, the fresh ones)."""
        _, inits = self.compare_open(pub, private, peers, with_summary)
        n = self.n
        all_rec = np.ascontiguousarray(self.d_rec.cpu().numpy()[:n]).view(HM.HS_RECORD).reshape(-1)
        ent = np.ascontiguousarray(self.o_init.cpu().numpy()[:n]).view(OM.HS_INIT).reshape(-1)  # (behind n_emitted: 0x7E bytes)
        shared = self.d_shared.cpu().numpy().tobytes()
        with _Memo():
            st, op, fr, sm = SM.stamp_batch(ent, len(inits) if stamp_summary else None, n, all_rec, n, shared, private, peers, stored,
                                            model, _pub, [GUARD] * (n + 4), b"\x7e" * (12 * (n + 1)), b"\x7e" * (144 * (n + 1)),
                                            [GUARD] * 4)
        got = self.s_st.cpu().numpy().view(np.uint32).tolist()
        assert got == st, [(k, a, b) for k, (a, b) in enumerate(zip(got, st)) if a != b][:5]
        ssum = self.s_sum.cpu().numpy().view(np.uint32)
        assert ssum[:4].tolist() == sm and (ssum[4:] == GUARD).all()
        got_op = self.s_op.cpu().numpy().tobytes()
        assert got_op == op, [(j, got_op[12 * j:12 * j + 12], op[12 * j:12 * j + 12]) for j in range(n + 1)
                              if got_op[12 * j:12 * j + 12] != op[12 * j:12 * j + 12]][:3]
        got_fr = self.s_fresh.cpu().numpy().tobytes()
        assert got_fr == fr, [j for j in range(n + 1) if got_fr[144 * j:144 * j + 144] != fr[144 * j:144 * j + 144]][:3]
        assert self.rig.eng.hs_stamps_get(0, len(peers)) == stored
        cover = len(inits) if stamp_summary else n
        return st[:cover], ent[:cover], np.frombuffer(fr[:144 * sm[0]], OM.HS_INIT)

    def compare_respond(self, fresh, eph=None):
        """wg_hs_respond's outputs against hs_respond_model over the fresh entries."""
        n = self.n
        ent = np.zeros(n, OM.HS_INIT)
        ent[:len(fresh)] = fresh
        with _Memo():
            e2, st, out, sm = RM.respond_batch(ent, len(fresh), n, self.eph if eph is None else eph, self.li, RM.SKIP_NEWPEER,
                                               [GUARD] * (n + 4), b"\x7e" * (176 * (n + 1)), [GUARD] * 4)
        got = (self.r_eph.cpu().numpy().tobytes(), self.r_st.cpu().numpy().view(np.uint32).tolist(),
               self.r_sess.cpu().numpy().tobytes(), self.r_sum.cpu().numpy().view(np.uint32).tolist())
        _same_sessions(got, (e2, st, out, sm + [GUARD] * 4), n)
        return np.frombuffer(out[:176 * sm[0]], RM.HS_SESSION)


def _peers4():
    return [_pub(k) for k in INITK[:4]]


# ---- 1. sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_list", SIZES)
def test_sizes(rig, n_list):
    """Random rings against stored stamps that make some of TSET stale; for n_list >= 255 every status must occur. The
    second run, over the same ring with n_inits = NULL, covers the entries behind n_emitted too (BADDESC: their peer
    field is the guard pattern) and finds the first run's winners stale."""
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = _peers4()
        eng.hs_peers_set(peers)
        stored = [TSET[2], ZERO, TSET[4], ZERO]
        eng.hs_stamps_set(0, stored)
        assert eng.hs_stamps_get(0, 4) == stored
        rng = np.random.default_rng(7600 + n_list)
        ring, off, lens = _stamp_ring(rng, n_list, STATIC)
        n = len(off) + 5
        ch = _StampChain(rig2, n, len(ring) + 64)
        ch.load(ring, off, lens)
        ch.run()
        st, ent, fresh = ch.compare_stamp(pub, STATIC, peers, stored)
        if n_list >= 255:
            assert set(st) == {SM.TS_OK, SM.TS_REPLAY, SM.TS_SUPERSEDED, SM.TS_BADAUTH, SM.TS_NOPEER}
            assert sorted(int(p) for p in fresh["peer"]) == [0, 1, 2, 3]
            assert (np.diff(fresh["record"].astype(np.int64)) > 0).all()
        ch.load(ring, off, lens)
        ch.run(stamp_summary=False)
        st2, _, fresh2 = ch.compare_stamp(pub, STATIC, peers, stored, stamp_summary=False)
        assert len(st2) == n and len(fresh2) == 0 and SM.TS_OK not in st2
        if n_list:
            assert st2[-5:] == [SM.TS_BADDESC] * 5
            # what the first run accepted or superseded is stale now; nothing else has changed
            assert st2[:len(st)] == [SM.TS_REPLAY if s in (SM.TS_OK, SM.TS_SUPERSEDED) else s for s in st]
    finally:
        eng.close()


# ---- 2. the order of 96 bits ---------------------------------------------------------------------------------------
def _bump(ts, at, d):
    return ts[:at] + bytes([ts[at] + d]) + ts[at + 1:]


ORDER = [("byte11+1", S0, _bump(S0, 11, 1), SM.TS_OK), ("byte11-1", S0, _bump(S0, 11, -1), SM.TS_REPLAY),
         ("byte7+1", S0, _bump(S0, 7, 1), SM.TS_OK), ("byte7-1", S0, _bump(S0, 7, -1), SM.TS_REPLAY),
         ("byte3+1", S0, _bump(S0, 3, 1), SM.TS_OK), ("byte3-1", S0, _bump(S0, 3, -1), SM.TS_REPLAY),
         ("byte0+1", S0, _bump(S0, 0, 1), SM.TS_OK), ("byte0-1", S0, _bump(S0, 0, -1), SM.TS_REPLAY),
         # big-endian: 00 01 00 > 00 00 ff > 00 00 80; read as little-endian words the middle one would be the greatest
         ("be_pair_a", S0, P9 + b"\x00\x01\x00", SM.TS_OK), ("be_pair_b", S0, P9 + b"\x00\x00\xff", SM.TS_OK),
         # a low word that is smaller beside a high part that is greater, and the other way round
         ("hi_up_lo_down", S0, _bump(S0, 7, 1)[:8] + bytes(4), SM.TS_OK), ("hi_down_lo_up", S0, _bump(S0, 7, -1)[:8] + b"\xff" * 4, SM.TS_REPLAY),
         ("equal", S0, S0, SM.TS_REPLAY), ("zero_on_nothing", ZERO, ZERO, SM.TS_REPLAY), ("all_ff", S0, b"\xff" * 12, SM.TS_OK),
         ("all_ff_on_all_ff", b"\xff" * 12, b"\xff" * 12, SM.TS_REPLAY)]


def test_order_of_96_bits(rig):
    """One peer. Each timestamp alone (n = 1) against its stored value, then all of them in one call."""
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = [_pub(INITK[0])]
        eng.hs_peers_set(peers)
        ch = _StampChain(rig2, len(ORDER) + 2, 148 * len(ORDER) + 256)
        for name, have, ts, want in ORDER:
            stored = [have]
            eng.hs_stamps_set(0, stored)
            ch.load(*_ring([_msg(STATIC, 0, ts)]))
            ch.run()
            st, _, fresh = ch.compare_stamp(pub, STATIC, peers, stored)
            assert st == [want], name
            assert stored == [ts if want == SM.TS_OK else have] and len(fresh) == (want == SM.TS_OK), name
        stored = [S0]
        eng.hs_stamps_set(0, stored)
        ch.load(*_ring([_msg(STATIC, 0, ts, 0x2000 + j) for j, (_, _, ts, _) in enumerate(ORDER)]))
        ch.run()
        st, _, fresh = ch.compare_stamp(pub, STATIC, peers, stored)
        first_ff = [ts for _, _, ts, _ in ORDER].index(b"\xff" * 12)
        assert [j for j, s in enumerate(st) if s == SM.TS_OK] == [first_ff] and stored == [b"\xff" * 12]
        assert [s for (_, _, ts, _), s in zip(ORDER, st) if ts <= S0] == [SM.TS_REPLAY] * sum(ts <= S0 for _, _, ts, _ in ORDER)
        assert st.count(SM.TS_SUPERSEDED) == len(ORDER) - 1 - st.count(SM.TS_REPLAY)
        # without the all-ff entries the big-endian pair decides: 00 01 00 wins, 00 00 ff is superseded
        keep = [(nm, ts) for nm, _, ts, _ in ORDER if ts != b"\xff" * 12 and not nm.startswith(("byte", "hi_"))]
        stored = [S0]
        eng.hs_stamps_set(0, stored)
        ch.load(*_ring([_msg(STATIC, 0, ts, 0x3000 + j) for j, (_, ts) in enumerate(keep)]))
        ch.run()
        st, _, _ = ch.compare_stamp(pub, STATIC, peers, stored)
        by = dict(zip([nm for nm, _ in keep], st))
        assert by["be_pair_a"] == SM.TS_OK and by["be_pair_b"] == SM.TS_SUPERSEDED and stored == [P9 + b"\x00\x01\x00"]
    finally:
        eng.close()


# ---- 3. ties and distance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_ties_and_distance(rig, variant):
    """600 entries, 72 peers with the pool's four known initiators at positions 0, 40, 68 and 71 (the last). Three pairs
    of one peer's entries: j = 3 and 500 (different workgroups), 64 and 65 (neighbouring lanes), 0 and n - 1; each is
    newer-first, newer-last or equal (the lower j wins) in one of the three variants. A BADAUTH entry with the greatest
    would-be timestamp and NOPEER entries sit between them and count for nothing."""
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        table = [bytes(splitmix_np(0x7700 + k, 32)) for k in range(72)]
        at = {0: 0, 1: 40, 2: 68, 3: 71}  # initiator -> position
        for i, p in at.items():
            table[p] = _pub(INITK[i])
        eng.hs_peers_set(b"".join(table))
        stored = [ZERO] * 72
        stored[40] = _t(90)
        eng.hs_stamps_set(40, [stored[40]])
        n = 600
        old, new = _t(100), _t((1 << 64) + 7)  # (new's low word is smaller than old's, its high part greater)
        orders = [(new, old), (old, new), (new, new)]
        pairs = {0: (3, 500), 1: (64, 65), 2: (0, n - 1)}  # initiator -> its two positions
        plan = {}
        for i, (a, b) in pairs.items():
            ta, tb = orders[(variant + i) % 3]
            plan[a], plan[b] = (6 * (a % 4) + i, ta, None), (6 * (b % 4) + i, tb, None)
        plan[10] = (0, b"\xff" * 12, (99, 0))       # initiator 0, the tag's first byte flipped: BADAUTH
        plan[70] = (1, b"\xff" * 12, (87, 7))       # initiator 1, the ciphertext's first byte flipped
        msgs = []
        for j in range(n):
            if j in plan:
                k, ts, flip = plan[j]
            elif j % 3 == 0:  # the last peer, timestamps with many ties
                k, ts, flip = 6 * (j % 4) + 3, _t(50 + (j * 7) % 5), None
            else:  # no peer holds initiators 4 and 5: NOPEER, whatever the timestamp
                k, ts, flip = 6 * (j % 4) + 4 + (j % 2), b"\xff" * 12, None
            msgs.append(_msg(STATIC, k, ts, 0x4000 + j, flip))
        ring, off, lens = _ring(msgs)
        ch = _StampChain(rig2, n, len(ring) + 64)
        ch.load(ring, off, lens)
        ch.run()
        st, ent, fresh = ch.compare_stamp(pub, STATIC, table, stored)
        assert len(st) == n and ent["record"].tolist() == list(range(n))
        for i, (a, b) in pairs.items():
            ta, tb = orders[(variant + i) % 3]
            assert (st[a], st[b]) == ((SM.TS_OK, SM.TS_SUPERSEDED) if ta >= tb else (SM.TS_SUPERSEDED, SM.TS_OK)), (i, a, b)
            assert stored[at[i]] == new
        assert st[10] == st[70] == SM.TS_BADAUTH and st[4] == st[100] == SM.TS_NOPEER
        ties = [j for j in range(0, n, 3) if j not in plan and (j * 7) % 5 == 4]
        assert st[ties[0]] == SM.TS_OK and {st[j] for j in ties[1:]} == {SM.TS_SUPERSEDED} and stored[71] == _t(54)
        assert sorted(int(p) for p in fresh["peer"]) == [0, 40, 68, 71]
    finally:
        eng.close()


# ---- 5. state and errors -------------------------------------------------------------------------------------------
def test_state_and_errors(rig):
    W, torch, dev = rig.W, rig.torch, rig.dev
    Lb = W._lib
    eng, rig2 = _engine(rig)
    try:
        n = 4
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        d_init, d_rec, d_sh = z8(n + 1, 144), z8(n, 160), z8(n, 32)
        s_st, s_sum = (torch.full((k,), GUARD, dtype=torch.int32, device=dev) for k in (n, 4))
        s_op, s_fresh = torch.full((12 * n,), 0x7E, dtype=torch.uint8, device=dev), torch.full((n + 1, 144), 0x7E, dtype=torch.uint8, device=dev)
        good = lambda: (d_init[:n], None, d_rec, d_sh, s_st, s_op, s_fresh[:n], s_sum)  # noqa: E731
        with pytest.raises(W.WgError) as e:
            eng.hs_stamp(*good())
        assert e.value.code == Lb.WG_ENOKEY
        with pytest.raises(W.WgError) as e:  # no table yet
            eng.hs_stamps_get(0, 1)
        assert e.value.code == Lb.WG_ERANGE
        pub = eng.hs_static_set(STATIC)
        peers = _peers4()
        eng.hs_peers_set(peers)
        # set, get, ranges
        assert eng.hs_stamps_get(0, 4) == [ZERO] * 4
        eng.hs_stamps_set(1, [S0, b"\xff" * 12])
        assert eng.hs_stamps_get(0, 4) == [ZERO, S0, b"\xff" * 12, ZERO] and eng.hs_stamps_get(2, 1) == [b"\xff" * 12]
        eng.hs_stamps_set(4, [])  # an empty range at the table's end
        for first, cnt in ((4, 1), (0, 5), (0xFFFFFFFF, 2)):
            with pytest.raises(W.WgError) as e:
                eng.hs_stamps_get(first, cnt)
            assert e.value.code == Lb.WG_ERANGE
            with pytest.raises(W.WgError) as e:
                eng.hs_stamps_set(first, [S0] * cnt)
            assert e.value.code == Lb.WG_ERANGE
        # a stamp against the set values; wg_hs_static_set keeps the stamps, wg_hs_peers_set zeroes them
        ch = _StampChain(rig2, 6, 1024)
        stored = [ZERO, S0, b"\xff" * 12, ZERO]
        ch.load(*_ring([_msg(STATIC, 1, _bump(S0, 11, 1)), _msg(STATIC, 2, _t(1 << 90)), _msg(STATIC, 3, _t(1))]))
        ch.run()
        st, _, _ = ch.compare_stamp(pub, STATIC, peers, stored)
        assert st == [SM.TS_OK, SM.TS_REPLAY, SM.TS_OK] and stored == [ZERO, _bump(S0, 11, 1), b"\xff" * 12, _t(1)]
        pub2 = eng.hs_static_set(STATIC2)
        assert eng.hs_stamps_get(0, 4) == stored
        ch.load(*_ring([_msg(STATIC2, 1, _bump(S0, 11, 1)), _msg(STATIC2, 3, _t(2))]))
        ch.run()
        st, _, _ = ch.compare_stamp(pub2, STATIC2, peers, stored)  # (the secrets follow the key, the stamps stay)
        assert st == [SM.TS_REPLAY, SM.TS_OK]
        eng.hs_peers_set(peers[:3])
        assert eng.hs_stamps_get(0, 3) == [ZERO] * 3
        with pytest.raises(W.WgError) as e:
            eng.hs_stamps_get(0, 4)
        assert e.value.code == Lb.WG_ERANGE
        # argument errors
        flat = s_fresh.reshape(-1)
        for bad in [(d_init[:n], None, d_rec, d_sh, s_st, s_op, d_init[1:n + 1], s_sum),                     # fresh inside inits
                    (d_init[:n], None, d_rec, d_sh, s_st, s_op, d_rec.reshape(-1)[:144 * n].reshape(n, 144), s_sum),  # ... inside records
                    (d_init[:n], None, d_rec, d_sh, flat[0:16].view(torch.int32), s_op, s_fresh[:n], s_sum),  # ts_status inside fresh
                    (d_init[:n], None, d_rec, d_sh, s_st, flat[0:12 * n], s_fresh[:n], s_sum),               # opened inside fresh
                    (d_init[:n], None, d_rec, d_sh, s_st, s_op, s_fresh[:n], flat[16:32].view(torch.int32)),  # summary inside fresh
                    (d_init[:n], None, d_rec, d_sh, s_st, s_op, flat[8:8 + 144 * n].reshape(n, 144), s_sum),  # fresh misaligned
                    (d_init[:n], None, d_rec, d_sh, s_st, s_op[2:], s_fresh[:n], s_sum),                     # opened misaligned
                    (d_init.reshape(-1)[8:8 + 144 * n].reshape(n, 144), None, d_rec, d_sh, s_st, s_op, s_fresh[:n], s_sum)]:
            with pytest.raises(W.WgError) as e:
                eng.hs_stamp(*bad)
            assert e.value.code == Lb.WG_EINVAL
        for flags, reserved in ((1, 0), (0, 1), (0x80000000, 0)):
            b = Lb.WgHsStampBatch(d_init.data_ptr(), None, d_rec.data_ptr(), d_sh.data_ptr(), s_st.data_ptr(), s_op.data_ptr(),
                                  s_fresh.data_ptr(), s_sum.data_ptr(), n, n, flags, reserved)
            assert W.lib().wg_hs_stamp(eng.ctx, ctypes.byref(b), None) == Lb.WG_EINVAL
        for nn, nr in (((1 << 30) + 1, n), (n, (1 << 30) + 1)):
            b = Lb.WgHsStampBatch(d_init.data_ptr(), None, d_rec.data_ptr(), d_sh.data_ptr(), s_st.data_ptr(), s_op.data_ptr(),
                                  s_fresh.data_ptr(), s_sum.data_ptr(), nn, nr, 0, 0)
            assert W.lib().wg_hs_stamp(eng.ctx, ctypes.byref(b), None) == Lb.WG_E2BIG
        eng.hs_stamp(d_init[:0], None, d_rec, d_sh, s_st[:0], s_op[:0], s_fresh[:0], s_sum)  # n = 0: a no-op
        torch.cuda.synchronize()
        assert (s_sum.cpu().numpy() == GUARD).all() and (s_st.cpu().numpy() == GUARD).all()
        assert (s_op.cpu().numpy() == 0x7E).all() and (s_fresh.cpu().numpy() == 0x7E).all()
    finally:
        eng.close()


def test_a_capturing_stream_cannot_allocate_the_state(rig):
    """The first wg_hs_stamp of a context on a capturing stream: WG_EINVAL, which names the way out. The state that
    wg_hs_stamps_set(ctx, 0, 0, NULL) then allocates starts with the scratch wg_hs_reserve was asked for before; a
    captured stamp of more entries than that is WG_EINVAL again."""
    W, torch, dev = rig.W, rig.torch, rig.dev
    eng, rig2 = _engine(rig)
    try:
        eng.hs_static_set(STATIC)
        eng.hs_peers_set(_peers4())
        n = 300
        eng.hs_reserve(n)
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        d_init, d_rec, d_sh, s_op, s_fresh = z8(2 * n, 144), z8(2 * n, 160), z8(2 * n, 32), z8(24 * n), z8(2 * n, 144)
        d_init[:, 12:16] = 0xFF  # every entry: WG_HS_NOPEER
        s_st, s_sum = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (2 * n, 4))
        args = lambda m: (d_init[:m], None, d_rec[:m], d_sh[:m], s_st[:m], s_op[:12 * m], s_fresh[:m], s_sum)  # noqa: E731
        torch.cuda.synchronize()
        errs = []
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                eng.hs_stamp(*args(n))
            errs.append(e.value)
            s_st.zero_()
        assert errs[0].code == W._lib.WG_EINVAL and "wg_hs_stamps_set" in str(errs[0])
        eng.hs_stamps_set(0, [])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(W.WgError) as e:
                eng.hs_stamp(*args(2 * n))
            errs.append(e.value)
            eng.hs_stamp(*args(n))
        assert errs[1].code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(errs[1])
        g.replay()
        torch.cuda.synchronize()
        assert s_st.cpu().numpy()[:n].tolist() == [SM.TS_NOPEER] * n and s_sum.cpu().numpy().tolist() == [0, 0, 0, n]
    finally:
        eng.close()


# ---- 6. graphs -----------------------------------------------------------------------------------------------------
def test_captured_six_stages_replay(rig):
    """plan -> check -> dh -> open -> stamp -> respond captured once, after the reserves. The first replay answers the
    fresh initiations; the second, over the same ring, finds every timestamp stale, answers nothing and consumes no
    ephemeral; after the ring's initiations are sealed again with later timestamps and the ephemerals refreshed, the
    third answers again."""
    torch = rig.torch
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        peers = _peers4()
        eng.hs_peers_set(peers)
        tset = TSET[:5] + [_t(1 << 80)]  # (none so great that nothing later is left)
        rings = [_stamp_ring(np.random.default_rng(7800), 70, STATIC, epoch, tset) for epoch in (0, 1 << 40)]
        assert [len(r[1]) for r in rings] == [len(rings[0][1])] * 2
        n = len(rings[0][1]) + 3
        ch = _StampChain(rig2, n, max(len(r[0]) for r in rings) + 64, respond=True)
        eng.rx_reserve(n)
        eng.hs_stamps_set(0, [])
        eng.hs_reserve(n)
        ch.refresh(1)
        ch.load(*rings[0])
        ch.run()  # eager once; its stamps are taken back below
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ch.run()
        stored = [ZERO] * 4
        eng.hs_stamps_set(0, stored)

        def replay(ring, seed):
            if seed is not None:
                ch.refresh(seed)
            ch.load(*ring)
            torch.cuda.synchronize()
            g.replay()
            st, _, fresh = ch.compare_stamp(pub, STATIC, peers, stored)
            return st, fresh, ch.compare_respond(fresh, eph=None if seed is not None else before)

        st, fresh, sess = replay(rings[0], 2)
        assert len(fresh) == len(sess) == 4 and sorted(int(s["peer"]) for s in sess) == [0, 1, 2, 3]
        assert sess["init"].tolist() == [0, 1, 2, 3]  # positions in fresh, not in inits
        before = ch.r_eph.cpu().numpy().tobytes()
        known = sum(s in (SM.TS_OK, SM.TS_REPLAY, SM.TS_SUPERSEDED) for s in st)
        st2, fresh2, sess2 = replay(rings[0], None)
        assert st2.count(SM.TS_REPLAY) == known and SM.TS_OK not in st2 and SM.TS_SUPERSEDED not in st2
        assert len(fresh2) == len(sess2) == 0 and ch.r_sum.cpu().numpy()[0] == 0
        assert ch.r_eph.cpu().numpy().tobytes() == before  # no ephemeral was consumed
        st3, fresh3, sess3 = replay(rings[1], 3)
        assert len(fresh3) == len(sess3) == 4 and st3.count(SM.TS_OK) == 4
    finally:
        eng.close()


# ---- 7. two contexts -----------------------------------------------------------------------------------------------
def test_two_contexts_fresh_then_replayed(rig):
    """Three initiators (one context that takes their static keys in turn) initiate to a responder context with
    increasing host timestamps, two rounds; the responder runs check -> dh -> open -> stamp -> respond, every
    handshake is established by wg_hs_finish and the keys agree. The same initiation records fed a second time, the
    newest round's and the older round's: all REPLAY, and no session."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    A, B = W.Engine(0, key_slots=16), W.Engine(0, key_slots=16)
    try:
        m = 3
        a_priv = [bytes(splitmix_np(0x7900 + k, 32)) for k in range(m)]
        b_priv = bytes(splitmix_np(0x7910, 32))
        b_pub = B.hs_static_set(b_priv)
        a_pub = [A.hs_static_set(k) for k in a_priv]
        A.hs_peers_set([b_pub])
        B.hs_peers_set(a_pub)
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        u8 = lambda b: torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev)  # noqa: E731
        u32 = lambda v: torch.from_numpy(np.array(v, np.uint32).view(np.int32)).to(dev)  # noqa: E731
        off148, len148 = torch.arange(0, 148 * m, 148, dtype=torch.int64, device=dev), torch.full((m,), 148, dtype=torch.int32, device=dev)
        off92, len92 = torch.arange(0, 92 * m, 92, dtype=torch.int64, device=dev), torch.full((m,), 92, dtype=torch.int32, device=dev)
        rounds = []
        for rnd in range(2):
            a_rec, pend = z8(m, 160), z8(m, 112)
            for k in range(m):  # initiator k: one initiation, a later timestamp each round
                A.hs_static_set(a_priv[k])
                a_st, a_sum = z32(1), z32(4)
                A.hs_initiate(z32(1), u8(splitmix_np(0x7920 + 8 * rnd + k, 32)), u8(_t(((1000 + rnd) << 32) + k)), u32([0x100 * rnd + k + 1]),
                              a_st, a_rec[k:k + 1], pend[k:k + 1], a_sum)
                torch.cuda.synchronize()
                assert a_sum.cpu().numpy().tolist() == [1, 0, 0, 0]
            ring = a_rec[:, 8:156].contiguous().reshape(-1)
            b = dict(hst=z32(m), hsum=z32(4), rec=z8(m, 160), sh=z8(m, 32), dh=z32(m), ost=z32(m), init=z8(m, 144), osum=z32(4),
                     sst=z32(m), sop=z8(12 * m), fresh=z8(m, 144), ssum=z32(4), eph=u8(splitmix_np(0x7940 + rnd, 32 * m)),
                     li=u32([0x80000000 + 0x100 * rnd + k for k in range(m)]), rst=z32(m), sess=z8(m, 176), rsum=z32(4))

            def respond(b=b, ring=ring):
                B.hs_check(ring, off148, len148, b["hst"], b["rec"], b["hsum"])
                B.hs_dh(b["rec"], b["hsum"], b["sh"], b["dh"])
                B.hs_open(b["rec"], b["hsum"], b["sh"], b["dh"], b["ost"], b["init"], b["osum"])
                B.hs_stamp(b["init"], b["osum"], b["rec"], b["sh"], b["sst"], b["sop"], b["fresh"], b["ssum"])
                B.hs_respond(b["fresh"], b["ssum"], b["eph"], b["li"], b["rst"], b["sess"], b["rsum"])
                torch.cuda.synchronize()
                return [x.cpu().numpy().tolist() for x in (b["osum"], b["sst"], b["ssum"], b["rsum"])]

            osum, sst, ssum, rsum = respond()
            assert osum == [m, m, 0, 0] and sst == [SM.TS_OK] * m and ssum == [m, 0, 0, 0] and rsum == [m, 0, 0, 0]
            assert b["sop"].cpu().numpy().tobytes() == b"".join(_t(((1000 + rnd) << 32) + k) for k in range(m))
            assert B.hs_stamps_get(0, m) == [_t(((1000 + rnd) << 32) + k) for k in range(m)]
            sess = b["sess"].cpu().numpy().reshape(-1).view(RM.HS_SESSION).copy()
            ring92 = b["sess"][:, 16:108].contiguous().reshape(-1)
            for k in range(m):  # initiator k finishes: the other two responses fail its mac1
                A.hs_static_set(a_priv[k])
                f_hst, f_hsum, f_rec, f_st, f_est, f_sum = z32(m), z32(4), z8(m, 160), z32(m), z8(m, 96), z32(4)
                A.hs_check(ring92, off92, len92, f_hst, f_rec, f_hsum)
                A.hs_finish(f_rec, f_hsum, pend[k:k + 1], f_st, f_est, f_sum)
                torch.cuda.synchronize()
                assert f_hsum.cpu().numpy().tolist() == [1, 0, 1, m - 1] and f_sum.cpu().numpy().tolist() == [1, 0, 0, 0]
                est = f_est.cpu().numpy().reshape(-1).view(IM.HS_ESTABLISHED)[0]
                s = sess[k]
                assert int(s["peer"]) == k and int(s["init"]) == k
                assert est["send_key"].tobytes() == s["recv_key"].tobytes() and est["recv_key"].tobytes() == s["send_key"].tobytes()
                assert int(est["local_index"]) == int(s["remote_index"]) and int(est["remote_index"]) == int(s["local_index"])
            rounds.append((b, respond))
        for b, respond in reversed(rounds):  # the newest round's records again, then the older round's
            b["eph"].copy_(u8(splitmix_np(0x7950, 32 * m)))
            b["sess"].zero_()
            osum, sst, ssum, rsum = respond()
            assert osum == [m, m, 0, 0] and sst == [SM.TS_REPLAY] * m and ssum == [0, m, 0, 0] and rsum == [0, 0, 0, 0]
            assert not b["sess"].cpu().numpy().any() and b["eph"].cpu().numpy().tobytes() == splitmix_np(0x7950, 32 * m).tobytes()
    finally:
        A.close()
        B.close()


# ---- the mirror ----------------------------------------------------------------------------------------------------
def test_mirror_open_timestamp(rig):
    """noise.Handshakes.openTimestamp on what the initiator mirror sealed and on the model's initiation."""
    N = noise()
    local, remote = N.NoisePrivateKey(STATIC), N.NoisePrivateKey(INITK[4])
    ts = _t((1 << 62) + 12345)
    stage = N.Handshakes.initiateHandshake(remote, N.NoisePublicKey(_pub(STATIC)), ephemeral=EPHK[5], timestamp=ts, senderIndex=7)
    msg = stage.initiation()
    got = N.Handshakes.openTimestamp(local, N.NoisePublicKey(msg[8:40]), msg[40:88], msg[88:116])
    assert got == ts
    with _Memo():
        assert SM.open_timestamp(_pub(STATIC), msg, M.x25519(STATIC, msg[8:40]), M.x25519(STATIC, _pub(INITK[4]))) == ts
    h = _hello(STATIC, 2, TSET[3])
    eph = N.NoisePublicKey(h["ephemeral"])
    assert N.Handshakes.openTimestamp(local, eph, h["encrypted_static"], h["encrypted_timestamp"]) == TSET[3]
    for at in (0, 11, 12, 27):
        with pytest.raises(N.BadPaddingException):
            N.Handshakes.openTimestamp(local, eph, h["encrypted_static"], _flip(h["encrypted_timestamp"], at, at % 8))
    with pytest.raises(N.BadPaddingException):
        N.Handshakes.openTimestamp(local, eph, _flip(h["encrypted_static"], 5, 1), h["encrypted_timestamp"])
