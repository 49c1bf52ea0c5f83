"""wg_blake2s_batch, wg_hs_key_set and wg_hs_check on the MI355X against tests/hs_model.py (pytest -m gpu):
digests, statuses, records and summaries are compared exactly; every output array carries guard words
behind what the call may write."""
import struct

import numpy as np
import pytest

import hs_model as M
import rx_plan_model as RM
from wgtest import noise, splitmix_np, wg

pytestmark = pytest.mark.gpu

R = 256  # kRankRange of wg_plan.hip: list positions per workgroup of the check / emit launches
GUARD = 0x7E7E7E7E
FILL = 0x5A
PUB = bytes(splitmix_np(0x45, 32))
PUB2 = bytes(splitmix_np(0x46, 32))
LENGTHS = [0, 1, 55, 56, 60, 63, 64, 65, 116, 127, 128, 129, 191, 192, 193, 5000]
KEYLENS = [0, 1, 16, 31, 32]
OUTLENS = [1, 3, 16, 20, 31, 32]
SHAPES = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    W = wg()
    eng = W.Engine(0, key_slots=16)
    eng.set_keys(0, splitmix_np(0x47, 32 * 16))
    yield type("Rig", (), dict(eng=eng, torch=torch, dev=dev, W=W))
    eng.close()


# ---- wg_blake2s_batch ------------------------------------------------------------------------------------
def _b2s(rig, desc, inp, out_size):
    """Runs wg_blake2s_batch over an output buffer of FILL bytes; returns (out bytes, status list). The
    status array has guard words behind its n entries; the whole output is compared by the caller."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    n = len(desc)
    d_desc = torch.from_numpy(W.desc_as_int64(desc).copy()).to(dev) if n else torch.zeros((0, 4), dtype=torch.int64, device=dev)
    d_in = torch.from_numpy(np.frombuffer(bytes(inp), np.uint8).copy()).to(dev)
    d_out = torch.full((out_size,), FILL, dtype=torch.uint8, device=dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    rig.eng.blake2s(d_desc, d_in, d_out, d_st[:n])
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    assert (st[n:] == GUARD).all()
    return d_out.cpu().numpy().tobytes(), st[:n].tolist()


def _same_b2s(rig, desc, inp, out_size):
    want, want_st = M.b2s_batch(desc, inp, bytes([FILL]) * out_size)
    got, got_st = _b2s(rig, desc, inp, out_size)
    assert got_st == want_st, [(i, a, b) for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:5]
    if got != want:
        bad = [i for i, d in enumerate(desc) if got[int(d["out_off"]):int(d["out_off"]) + 32] !=
               want[int(d["out_off"]):int(d["out_off"]) + 32]][:5]
        raise AssertionError(("digest or bytes around it differ", bad, [desc[i] for i in bad]))
    return want, want_st


def test_known_answers_on_the_device(rig):
    inp = b"?abc" + bytes(range(32)) + b"mac1----" + bytes(32)
    d = rig.W.pack_b2s_desc([1, 4, 4], [1, 33, 65], [0, 4, 0], [3, 0, 0], [32, 32, 32], [0, 32, 0])
    out, st = _b2s(rig, d, inp, 100)
    assert st == [0, 0, 0]
    assert out[1:33].hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    assert out[33:65].hex() == "48a8997da407876b3d79c0d92325ad3b89cbb754d86ab71aee047ad345fd2c49"
    assert out[65:97] == M.blake2s(b"") and out[0] == FILL and out[97:] == bytes([FILL]) * 3


def test_hash_lengths_keys_and_digest_sizes(rig):
    """Every length x key length x digest size, in one batch: the key block as the last block (keyed, empty
    input), multiples of 64 (no empty block follows), a last digest word that is partly written. Offsets
    take every alignment; out_off steps by 37, so every digest has FILL bytes on both sides."""
    rng = np.random.default_rng(2100)
    inp = rng.bytes(6000)
    rows = []
    for ln in LENGTHS:
        for kl in KEYLENS:
            for ol in OUTLENS:
                k = len(rows)
                rows.append((int(rng.integers(0, 6000 - ln + 1)), 3 + 37 * k, int(rng.integers(0, 6000 - kl + 1)), ln, ol, kl))
    assert len(rows) == 480
    d = rig.W.pack_b2s_desc(*(np.array(c, np.uint64) for c in zip(*rows)))
    assert {int(x) & 3 for x in d["in_off"]} == {0, 1, 2, 3} == {int(x) & 3 for x in d["out_off"]}
    _same_b2s(rig, d, inp, 3 + 37 * 480 + 5)


def test_batch_shapes_mixed_lengths_odd_offsets(rig):
    """n around a wave and a workgroup; inside one wave a 5,000-B message among 1-B ones and random short
    ones; in_off, key_off and out_off all odd."""
    rng = np.random.default_rng(2200)
    inp = rng.bytes(8192)
    for n in SHAPES:
        ln = np.where(rng.random(n) < 0.5, 1, rng.integers(0, 200, n))
        if n > 1:
            ln[n // 2] = 5000
        kl = rng.choice(np.array(KEYLENS), n)
        ol = rng.choice(np.array(OUTLENS), n)
        in_off = np.array([int(rng.integers(0, (8192 - int(x)) // 2)) * 2 + 1 for x in ln], np.uint64)
        key_off = np.array([int(rng.integers(0, 4000)) * 2 + 1 for _ in range(n)], np.uint64)
        out_off = 1 + 34 * np.arange(n, dtype=np.uint64)
        d = rig.W.pack_b2s_desc(in_off, out_off, key_off, ln, ol, kl)
        _same_b2s(rig, d, inp, 34 * n + 8)


def test_bad_descriptors_leave_the_output_untouched(rig):
    """About 3% bad descriptors of every kind among 2,000: digest size 0 and 33, key length 33, each of the
    three ranges past its buffer by one byte, offsets near 2^64 (a sum would wrap). BADDESC, and the whole
    output buffer equals the model's, which leaves those digests' bytes alone."""
    rng = np.random.default_rng(2300)
    n, in_size, out_size = 2000, 4096, 2000 * 32
    inp = rng.bytes(in_size)
    ln = rng.integers(0, 130, n)
    kl = rng.choice(np.array(KEYLENS), n)
    ol = rng.choice(np.array(OUTLENS), n)
    d = rig.W.pack_b2s_desc([int(rng.integers(0, in_size - int(x) + 1)) for x in ln], 32 * np.arange(n, dtype=np.uint64),
                            [int(rng.integers(0, in_size - int(x) + 1)) for x in kl], ln, ol, kl)
    bad = rng.permutation(n)[:60]
    for j, i in enumerate(bad):
        kind = j % 10
        if kind == 0:
            d["outlen"][i] = 0
        elif kind == 1:
            d["outlen"][i] = 33
        elif kind == 2:
            d["keylen"][i] = 33
        elif kind == 3:
            d["in_off"][i] = in_size + 1 - int(d[i]["len"])
        elif kind == 4:
            d["keylen"][i], d["key_off"][i] = 32, in_size - 31
        elif kind == 5:
            d["out_off"][i] = out_size + 1 - int(d[i]["outlen"])
        elif kind == 6:
            d["in_off"][i], d["len"][i] = (1 << 64) - 1, 2
        elif kind == 7:
            d["key_off"][i], d["keylen"][i] = (1 << 64) - 16, 32
        elif kind == 8:
            d["out_off"][i] = (1 << 64) - 1
        else:
            d["len"][i], d["in_off"][i] = 0xFFFFFFFF, 1
    _, st = _same_b2s(rig, d, inp, out_size)
    assert st.count(M.B2S_BADDESC) == 60 and all(st[i] == M.B2S_BADDESC for i in bad)
    # ranges that end exactly at the end of their buffer are good
    e = rig.W.pack_b2s_desc([in_size - 100, in_size], [out_size - 32, 0], [in_size - 32, in_size], [100, 0], [32, 1], [32, 0])
    _, st = _same_b2s(rig, e, inp, out_size)
    assert st == [0, 0]


def test_batch_argument_errors(rig):
    torch, dev, W = rig.torch, rig.dev, rig.W
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    d = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(W.WgError) as e:  # out inside in
        rig.eng.blake2s(d, buf, buf[64:128], st)
    assert e.value.code == W._lib.WG_EINVAL
    rig.eng.blake2s(d[:0], buf[:128], buf[128:], st[:0])  # n = 0: a no-op
    torch.cuda.synchronize()


# ---- wg_hs_check ---------------------------------------------------------------------------------------------
def _flip(m, at, rng):
    return m[:at] + bytes([m[at] ^ (1 << int(rng.integers(0, 8)))]) + m[at + 1:]


def _hs_datagram(rng, kind, pub):
    """(bytes in the ring, stated length) of one datagram of the given kind."""
    t = 1 + int(rng.integers(0, 2))
    L = 148 if t == 1 else 92
    m = M.message(t, rng.bytes(120), pub)
    if kind == "ok":
        return m, L
    if kind == "body":
        return _flip(m, int(rng.integers(1, L - 32)), rng), L
    if kind == "mac1":
        return _flip(m, int(rng.integers(L - 32, L - 16)), rng), L
    if kind == "mac2":
        return _flip(m, int(rng.integers(L - 16, L)), rng), L
    if kind == "len":
        wl = int(rng.choice([0, 91, 93, 147, 149]))
        t = 2 if wl in (91, 93) else 1
        m = M.message(t, rng.bytes(120), pub)
        return (m + rng.bytes(2))[:max(wl, 1)], wl
    assert kind == "type"
    return bytes([int(rng.choice([3, 4, 0]))]) + m[1:], L


KINDS = ["ok"] * 10 + ["body", "mac1", "mac2", "len", "len", "type", "type"] + ["mac1", "mac2", "body"]


def _hs_ring(rng, n, pub, forced=(0, 63, 64, 255, 256)):
    """A ring of n datagrams at unaligned offsets: valid initiations and responses (forced at the given list
    positions and at n - 1, so the rank crosses wave and workgroup boundaries), one flipped bit in body,
    mac1 or mac2, lengths 0 / 91 / 93 / 147 / 149, types 3 / 4 / 0; with n >= 8, datagram n / 2 ends one
    byte past the ring and datagram n / 2 + 1 starts past it."""
    buf, off, lens = bytearray(rng.bytes(1)), [], []
    for k in range(n):
        kind = "ok" if k in forced or k == n - 1 else KINDS[int(rng.integers(0, len(KINDS)))]
        m, wl = _hs_datagram(rng, kind, pub)
        off.append(len(buf))
        lens.append(wl)
        buf += m + rng.bytes(int(rng.integers(0, 4)))
    ring = np.frombuffer(bytes(buf), np.uint8).copy()
    if n >= 8:
        off[n // 2], lens[n // 2] = len(ring) - 147, 148
        off[n // 2 + 1], lens[n // 2 + 1] = len(ring) + 1, 148
    return ring, np.array(off, np.uint64), np.array(lens, np.uint32)


def _hs_buffers(rig, n):
    torch, dev = rig.torch, rig.dev
    return (torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev),
            torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev),
            torch.full((8,), GUARD, dtype=torch.int32, device=dev))


def _hs_read(n, nl, d_st, d_rec, d_sum):
    """(status list, records, summary dict) of one check, after the guard checks: nothing behind the list's
    length in hs_status, nothing behind n_valid records, nothing behind the 16-B summary."""
    st, rec, sm = d_st.cpu().numpy(), d_rec.cpu().numpy(), d_sum.cpu().numpy()
    assert (sm[4:] == GUARD).all(), "summary guard overwritten"
    s = dict(n_valid=int(sm[0]), n_init=int(sm[1]), n_resp=int(sm[2]), n_rejected=int(sm[3]))
    assert (st[nl:] == GUARD).all(), "hs_status written past the list"
    assert s["n_valid"] <= n and (rec[s["n_valid"]:] == 0x7E).all(), "records written past n_valid"
    return st[:nl].tolist(), np.ascontiguousarray(rec[:s["n_valid"]]).view(M.HS_RECORD).reshape(-1), s


def _check_identity(rig, ring, off, lens, pub):
    torch, dev = rig.torch, rig.dev
    n = len(off)
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32)).to(dev)
    d_st, d_rec, d_sum = _hs_buffers(rig, n)
    rig.eng.hs_check(d_ring, d_off, d_len, d_st[:n], d_rec[:n], d_sum[:4])
    torch.cuda.synchronize()
    got = _hs_read(n, n, d_st, d_rec, d_sum)
    want = M.check(ring, off, lens, pub)
    assert got[0] == want[0], [(i, a, b) for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:5]
    assert got[2] == want[2]
    assert got[1].tobytes() == want[1].tobytes()
    return want


def test_no_key_then_two_keys(rig):
    """A context that never had wg_hs_key_set refuses the check (WG_ENOKEY); under a second key everything the
    first accepted fails mac1."""
    W = rig.W
    eng = W.Engine(0, key_slots=4)
    try:
        rig2 = type("Rig", (), dict(eng=eng, torch=rig.torch, dev=rig.dev, W=W))
        rng = np.random.default_rng(2400)
        ring, off, lens = _hs_ring(rng, 100, PUB)
        with pytest.raises(W.WgError) as e:
            _check_identity(rig2, ring, off, lens, PUB)
        assert e.value.code == W._lib.WG_ENOKEY
        eng.hs_key_set(PUB)
        st, rec, s = _check_identity(rig2, ring, off, lens, PUB)
        assert s["n_valid"] > 30
        eng.hs_key_set(PUB2)
        st2, rec2, s2 = _check_identity(rig2, ring, off, lens, PUB2)
        assert s2["n_valid"] == 0 and all(b == M.HS_BADMAC1 for a, b in zip(st, st2) if a == M.HS_OK)
    finally:
        eng.close()


@pytest.mark.parametrize("n", SHAPES + [5000])
def test_check_identity_list(rig, n):
    """Every datagram of the ring checked (list = NULL). From 63 datagrams on, the model's result must
    accept between 20% and 80%; from 255 on it must hold every status, so a mix that degenerates cannot
    pass silently (a ring of 0 or 1 datagrams cannot hold a mix)."""
    rig.eng.hs_key_set(PUB)
    rng = np.random.default_rng(2500 + n)
    ring, off, lens = _hs_ring(rng, n, PUB)
    st, rec, s = _check_identity(rig, ring, off, lens, PUB)
    if n >= 63:
        assert 0.2 * n <= s["n_valid"] <= 0.8 * n
        assert s["n_init"] > 0 and s["n_resp"] > 0
    if n >= 255:
        assert set(st) == {M.HS_OK, M.HS_BADLEN, M.HS_BADTYPE, M.HS_BADMAC1, M.HS_BADMAC2}
        assert all(st[k] == M.HS_OK for k in (0, 63, 64, n - 1)) and (n < 257 or st[255] == st[256] == M.HS_OK)


def _mixed_ring(rng, n, sess, max_len, pub, p_hs=0.12):
    """This file's own mixed UDP ring for the plan: transport packets of known and unknown receiver indices,
    junk types, and about p_hs handshake datagrams of every kind of _hs_datagram."""
    known = list(sess.keys())
    buf, off, lens = bytearray(rng.bytes(3)), [], []
    for k in range(n):
        r = rng.random()
        if r < p_hs:
            m, wl = _hs_datagram(rng, KINDS[int(rng.integers(0, len(KINDS)))], pub)  # (a retyped one is not listed)
        else:
            t = 4 if r < 0.9 else int(rng.integers(3, 256))
            wl = int(rng.integers(32, max_len + 34))
            index = int(rng.integers(0, 1 << 32)) if rng.random() < 0.1 else known[int(rng.integers(0, len(known)))]
            m = struct.pack("<BxxxIQ", t, index, k) + rng.bytes(wl - 16)
        off.append(len(buf))
        lens.append(wl)
        buf += m + rng.bytes(int(rng.integers(0, 4)))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32)


class _PlanCheck:
    """Device buffers of one plan + check pipeline over n datagrams; run() issues both calls back to back
    on the current stream, and the host reads nothing in between."""

    def __init__(self, rig, n, ring_size, max_len):
        torch, dev = rig.torch, rig.dev
        self.rig, self.n, self.max_len = rig, n, max_len
        self.d_ring = torch.zeros(ring_size, dtype=torch.uint8, device=dev)
        self.d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        self.d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        self.p_st = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_host = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
        self.p_sum = torch.zeros(2, dtype=torch.int64, device=dev)
        self.d_st, self.d_rec, self.d_sum = _hs_buffers(rig, n)

    def load(self, ring, off, lens):
        torch = self.rig.torch
        assert len(ring) <= self.d_ring.numel()
        self.d_ring[:len(ring)].copy_(torch.from_numpy(ring))
        self.view = self.d_ring[:len(ring)]
        self.d_off.copy_(torch.from_numpy(off.view(np.int64)))
        self.d_len.copy_(torch.from_numpy(lens.view(np.int32)))
        self.d_st.fill_(GUARD)
        self.d_rec.fill_(0x7E)
        self.d_sum.fill_(GUARD)

    def run(self, view=None):
        eng, n = self.rig.eng, self.n
        w = self.view if view is None else view
        eng.rx_plan(w, self.d_off, self.d_len, self.d_desc, self.p_st, self.d_host, self.p_sum, self.max_len)
        eng.hs_check(w, self.d_off, self.d_len, self.d_st[:n], self.d_rec[:n], self.d_sum[:4], host_list=self.d_host,
                     rx_summary=self.p_sum)

    def compare(self, ring, off, lens, sess, pub):
        self.rig.torch.cuda.synchronize()
        _, _, want_host, _ = RM.plan(ring, off, lens, sess, max_len=self.max_len, mode=RM.PT_AFTER)
        assert int(self.p_sum.cpu().numpy()[1:2].view(np.uint32)[1]) == len(want_host)
        assert self.d_host.cpu().numpy()[:len(want_host)].tolist() == want_host
        got = _hs_read(self.n, len(want_host), self.d_st, self.d_rec, self.d_sum)
        want = M.check(ring, off, lens, pub, lst=want_host)
        assert got[0] == want[0]
        assert got[2] == want[2]
        assert got[1].tobytes() == want[1].tobytes()
        return want, want_host


SESS = {0x01020304: 1, 7: 2, 0xFFFFFFF0: 3, 0x80000001: 4}


def test_plan_then_check_on_one_stream(rig):
    """wg_rx_plan and wg_hs_check back to back: the check takes the plan's host_list and the address of its
    n_host. 3,000 datagrams with about 12% handshake datagrams; then a ring without any (n_host = 0), which
    writes only a zero summary."""
    eng = rig.eng
    eng.hs_key_set(PUB)
    eng.rx_sessions_set(list(SESS.keys()), list(SESS.values()))
    rng = np.random.default_rng(2600)
    n, max_len = 3000, 120
    ring, off, lens = _mixed_ring(rng, n, SESS, max_len, PUB)
    pc = _PlanCheck(rig, n, len(ring) + 64, max_len)
    pc.load(ring, off, lens)
    pc.run()
    (st, rec, s), host = pc.compare(ring, off, lens, SESS, PUB)
    assert len(host) > 250 and 0.2 * len(host) <= s["n_valid"] <= 0.8 * len(host)
    assert {M.HS_OK, M.HS_BADLEN, M.HS_BADMAC1, M.HS_BADMAC2} == set(st)
    assert rec["index"].tolist() == [i for i, x in zip(host, st) if x == M.HS_OK]
    ring2, off2, lens2 = _mixed_ring(rng, n, SESS, max_len, PUB, p_hs=0.0)
    pc.load(ring2, off2, lens2)
    pc.run()
    (st, rec, s), host = pc.compare(ring2, off2, lens2, SESS, PUB)
    assert host == [] and st == [] and s == dict(n_valid=0, n_init=0, n_resp=0, n_rejected=0)


def test_captured_plan_and_check_replay(rig):
    """wg_hs_reserve, then plan + check captured once over 700 datagrams and replayed three times; the ring
    changes between replays, and wg_hs_key_set changes the key between the last two, without re-capture.
    A check on a capturing stream that needs more scratch than was reserved returns WG_EINVAL."""
    torch, dev, eng, W = rig.torch, rig.dev, rig.eng, rig.W
    eng.hs_key_set(PUB)
    eng.rx_sessions_set(list(SESS.keys()), list(SESS.values()))
    rng = np.random.default_rng(2700)
    n, max_len, ring_size = 700, 100, 700 * 160
    pc = _PlanCheck(rig, n, ring_size, max_len)
    big = 400000  # more than any check of this module reserved
    b_off = torch.zeros(big, dtype=torch.int64, device=dev)
    b_len = torch.zeros(big, dtype=torch.int32, device=dev)
    b_st = torch.zeros(big, dtype=torch.int32, device=dev)
    b_rec = torch.zeros((big, 160), dtype=torch.uint8, device=dev)

    def ring_for(pub, p_hs):
        ring, off, lens = _mixed_ring(rng, n, SESS, max_len, pub, p_hs=p_hs)
        full = np.zeros(ring_size, np.uint8)  # the captured ring has one size: the datagrams lie at its front
        full[:len(ring)] = ring
        return full, off, lens

    eng.rx_reserve(n)
    eng.hs_reserve(n)
    first = ring_for(PUB, 0.3)
    pc.load(*first)
    pc.run(pc.d_ring)  # eager once
    pc.compare(first[0], first[1], first[2], SESS, PUB)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(W.WgError) as e:
            eng.hs_check(pc.d_ring, b_off, b_len, b_st, b_rec, pc.d_sum[:4])
        pc.run(pc.d_ring)
    assert e.value.code == W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
    valid = []
    for replay, (pub, p_hs) in enumerate([(PUB, 0.5), (PUB, 0.05), (PUB2, 0.5)]):
        ring, off, lens = ring_for(PUB, p_hs)  # (the messages are always made for PUB)
        if replay == 2:
            eng.hs_key_set(PUB2)
        pc.load(ring, off, lens)
        torch.cuda.synchronize()
        g.replay()
        (st, rec, s), host = pc.compare(ring, off, lens, SESS, pub)
        valid.append(s["n_valid"])
    assert valid[0] > 50 and 0 < valid[1] < valid[0] and valid[2] == 0


def test_checks_on_two_streams_both_match_the_model(rig):
    """Six checks of two different rings issued back to back on two streams, alternating, with no
    synchronisation between them: they share the scratch, the library chains them, each equals the model."""
    torch, dev, eng = rig.torch, rig.dev, rig.eng
    eng.hs_key_set(PUB)
    rng = np.random.default_rng(2900)
    batches = []
    for n in (5000, 3001):
        ring, off, lens = _hs_ring(rng, n, PUB)
        batches.append((torch.from_numpy(ring).to(dev), torch.from_numpy(off.view(np.int64)).to(dev),
                        torch.from_numpy(lens.view(np.int32)).to(dev), n, M.check(ring, off, lens, PUB)))
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = []
    torch.cuda.synchronize()
    for k in range(6):
        d_ring, d_off, d_len, n, want = batches[k % 2]
        o = _hs_buffers(rig, n)
        eng.hs_check(d_ring, d_off, d_len, o[0][:n], o[1][:n], o[2][:4], stream=streams[k % 2].cuda_stream)
        outs.append((n, o, want))
    torch.cuda.synchronize()
    for n, o, want in outs:
        got = _hs_read(n, n, *o)
        assert got[0] == want[0] and got[2] == want[2] and got[1].tobytes() == want[1].tobytes()


# ---- the mirror ---------------------------------------------------------------------------------------------------
def test_mirror_equals_hashlib_and_its_mac1_is_accepted(rig):
    N = noise()
    rng = np.random.default_rng(2800)
    for ln, kl, ol in [(0, 0, 32), (0, 32, 32), (64, 0, 1), (65, 16, 31), (300, 32, 16)]:
        data, key = rng.bytes(ln), rng.bytes(kl)
        h = N.Blake2s(ol, key)
        h.update(data[:ln // 2])
        h.update(data, ln // 2, ln - ln // 2)
        assert h.digest() == M.blake2s(data, key, ol)
        assert h.digest() == M.blake2s(b"", key, ol)  # reset by digest (Blake2s.java:140)
    assert N.BLAKE2s256(b"mac1----", PUB) == M.mac1_key(PUB)
    assert N.BLAKE2s256(b"abc").hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    head = bytes([1]) + rng.bytes(115)
    mac = N.calculate_mac1(head, PUB)
    assert mac == M.mac1(head, PUB)
    assert N.calculate_mac1(bytes(116), bytes(32)).hex() == "a27f47acf041191bf95a6748dc26d89e"
    ring = np.frombuffer(b"\0\0\0" + head + mac + bytes(16), np.uint8).copy()
    rig.eng.hs_key_set(PUB)
    st, rec, s = _check_identity(rig, ring, [3], [148], PUB)
    assert st == [M.HS_OK] and rec[0]["msg"].tobytes() == ring[3:].tobytes()
