"""wg_x25519_batch, wg_hs_static_set and wg_hs_dh on the MI355X against tests/x25519_model.py (pytest -m gpu):
outputs and statuses are compared exactly; every output array carries guard bytes behind what the call may
write. The model costs a millisecond or two per ladder, so its results are memoised and the module stays
under about 1,500 distinct operands."""
import functools
import struct

import numpy as np
import pytest

import hs_model as HM
import rx_plan_model as RM
import x25519_model as M
from wgtest import noise, splitmix_np, wg

pytestmark = pytest.mark.gpu

GUARD = 0x7E7E7E7E
FILL = 0x5A
SHAPES = [0, 1, 63, 64, 65, 255, 256, 257]
H = bytes.fromhex
K1, U1 = H("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"), \
    H("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
R1 = "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
K2, U2 = H("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d"), \
    H("e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493")
R2 = "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"
ITER_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
ITER_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
ALICE = H("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
ALICE_PUB = "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
BOB = H("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
BOB_PUB = "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
SHARED = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
ORDER8 = [325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823]
LOW_ORDER = [0, 1] + ORDER8 + [M.P - 1, M.P, M.P + 1]
SCALARS = {"alice": ALICE, "zero": bytes(32), "ones": b"\xff" * 32}
LIMB_BITS = [26, 51, 77, 102, 128, 153, 179, 204, 230, 255]
STATIC, STATIC2 = bytes(splitmix_np(0x61, 32)), bytes(splitmix_np(0x62, 32))


def le(x: int) -> bytes:
    return (x % (1 << 256)).to_bytes(32, "little")


model = functools.lru_cache(maxsize=None)(M.x25519)


class _Memo:
    """x25519_model's batch / hs_dh with the memoised ladder."""

    def __enter__(self):
        self.keep, M.x25519 = M.x25519, model

    def __exit__(self, *a):
        M.x25519 = self.keep


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


# ---- wg_x25519_batch -------------------------------------------------------------------------------------
def _run(rig, desc, inp, out_size):
    """Runs wg_x25519_batch over an output buffer of FILL bytes; returns (out bytes, status list). The status
    array has guard words behind its n entries; the whole output is compared by the caller."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    n = len(desc)
    d_desc = torch.from_numpy(W.desc_as_int64(desc).copy()).to(dev) if n else torch.zeros((0, 4), dtype=torch.int64, device=dev)
    d_in = torch.from_numpy(np.frombuffer(bytes(inp), np.uint8).copy()).to(dev)
    d_out = torch.full((out_size,), FILL, dtype=torch.uint8, device=dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    rig.eng.x25519(d_desc, d_in, d_out, d_st[:n])
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    assert (st[n:] == GUARD).all()
    return d_out.cpu().numpy().tobytes(), st[:n].tolist()


def _same(rig, desc, inp, out_size):
    with _Memo():
        want, want_st = M.batch(desc, inp, bytes([FILL]) * out_size)
    got, got_st = _run(rig, desc, inp, out_size)
    assert got_st == want_st, [(i, a, b) for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:5]
    if got != want:
        bad = [i for i, d in enumerate(desc) if got[int(d["out_off"]):int(d["out_off"]) + 32] !=
               want[int(d["out_off"]):int(d["out_off"]) + 32]][:5]
        raise AssertionError(("result or bytes around it differ", bad, [desc[i] for i in bad],
                              [got[int(desc[i]["out_off"]):int(desc[i]["out_off"]) + 32].hex() for i in bad]))
    return want, want_st


def _pairs(rig, pairs):
    """[(scalar, point or None)] -> (buffers for one batch: scalars and points packed, outputs 34 bytes apart
    from offset 1, so every result has FILL bytes on both sides)."""
    n = len(pairs)
    inp = b"".join(k + (u if u is not None else bytes(32)) for k, u in pairs) + b"\0"
    at = 64 * np.arange(n, dtype=np.uint64)
    flags = np.array([rig.W._lib.WG_X25519_BASE if u is None else 0 for _, u in pairs], np.uint32)
    d = rig.W.pack_x25519_desc(at, at + np.uint64(32), 1 + 34 * np.arange(n, dtype=np.uint64), flags)
    return d, inp, 34 * n + 8


def test_known_answers_on_the_device(rig):
    """RFC 7748 5.2 and 6.1; WG_X25519_BASE against an explicit u = 9."""
    pairs = [(K1, U1), (K2, U2), (M.BASE_POINT, M.BASE_POINT), (ALICE, None), (BOB, None), (ALICE, M.BASE_POINT),
             (ALICE, H(BOB_PUB)), (BOB, H(ALICE_PUB))]
    d, inp, size = _pairs(rig, pairs)
    out, st = _run(rig, d, inp, size)
    assert st == [0] * 8
    got = [out[1 + 34 * k:33 + 34 * k].hex() for k in range(8)]
    assert got == [R1, R2, ITER_1, ALICE_PUB, BOB_PUB, ALICE_PUB, SHARED, SHARED]
    assert out == _same(rig, d, inp, size)[0]


def test_iterated_vector_1000_launches(rig):
    """RFC 7748 5.2's iteration as 1,000 launches of one descriptor, with device-side copies between them:
    k, u = X25519(k, u), k."""
    torch, dev, W = rig.torch, rig.dev, rig.W
    d_desc = torch.from_numpy(W.desc_as_int64(W.pack_x25519_desc([0], [32], [0]))).to(dev)
    d_in = torch.from_numpy(np.frombuffer(M.BASE_POINT * 2, np.uint8).copy()).to(dev)
    d_out = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    first = None
    for it in range(1000):
        rig.eng.x25519(d_desc, d_in, d_out, d_st)
        d_in[32:].copy_(d_in[:32])
        d_in[:32].copy_(d_out)
        bad |= d_st
        if it == 0:
            first = d_out.clone()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert first.cpu().numpy().tobytes().hex() == ITER_1
    assert d_out.cpu().numpy().tobytes().hex() == ITER_1000


@pytest.mark.parametrize("name", list(SCALARS))
def test_edge_operands(rig, name):
    """Where the carries and the final reduction can go wrong: u = p - 1, p, p + 1, 2^255 - 1, 9 + 2^255; 2^k - 1
    and 2^k at every limb boundary; the low-order points. Each under the scalar as it is and clamped: the two
    give the same bytes. The low-order points give WG_X25519_ZERO with 32 zero bytes written."""
    sc = SCALARS[name]
    us = [M.P - 1, M.P, M.P + 1, (1 << 255) - 1, 9 + (1 << 255)] + [0, 1] + ORDER8
    for k in LIMB_BITS:
        us += [(1 << k) - 1, 1 << k]
    pairs = [(s, le(u)) for u in us for s in (sc, M.clamp(sc))]
    d, inp, size = _pairs(rig, pairs)
    out, st = _same(rig, d, inp, size)
    res = [out[1 + 34 * k:33 + 34 * k] for k in range(len(pairs))]
    assert res[0::2] == res[1::2] and st[0::2] == st[1::2]
    for j, u in enumerate(us):
        low = u % (1 << 255) % M.P in [x % M.P for x in LOW_ORDER]
        assert st[2 * j] == (M.X_ZERO if low else M.X_OK), u
        assert (res[2 * j] == bytes(32)) == low
    assert res[2 * us.index((1 << 255) - 1)] == model(sc, le(18)) and res[2 * us.index(9 + (1 << 255))] == model(sc, le(9))


def test_results_just_below_p_and_just_above_zero(rig):
    """Results whose bytes 1..30 are all 0xFF (just below p, and in the middle of the range), and results just
    above 0. A search of
    2^16 random operands cannot find such a result (one in 2^240 has it), so the operands are constructed:
    for a wanted r that is a point of the prime-order subgroup, u = r times the inverse of the clamped
    scalar modulo the group order (x25519_model.operands_for_result), checked with the model's ladder."""
    groups = {"below p": [M.P - j for j in range(1, 400)],
              "above 0": list(range(2, 400)),
              "in the middle": [(0x3A << 248) | (((1 << 240) - 1) << 8) | j for j in range(256)]}
    pairs, want = [], []
    for name, cand in groups.items():
        for sc in SCALARS.values():
            ur = M.operands_for_result(sc, cand)
            assert ur is not None, name
            assert model(sc, ur[0]) == ur[1]
            pairs.append((sc, ur[0]))
            want.append(ur[1])
    assert all(r[1:31] == b"\xff" * 30 for r in want[:3] + want[6:]) and all(r[1:] == bytes(31) for r in want[3:6])
    d, inp, size = _pairs(rig, pairs)
    out, st = _same(rig, d, inp, size)
    assert st == [0] * len(pairs) and [out[1 + 34 * k:33 + 34 * k] for k in range(len(pairs))] == want


@pytest.mark.parametrize("n", SHAPES)
def test_batch_shapes_random_operands(rig, n):
    """n around a wave and a block of four waves, random operands, odd offsets."""
    raw = splitmix_np(0x3000 + n, 64 * n + 1).tobytes()
    inp = b"\x11" + raw
    at = 1 + 64 * np.arange(n, dtype=np.uint64)
    d = rig.W.pack_x25519_desc(at, at + np.uint64(32), 3 + 34 * np.arange(n, dtype=np.uint64))
    _, st = _same(rig, d, inp, 34 * n + 8)
    assert st == [M.X_OK] * n


def test_every_offset_alignment_in_one_batch(rig):
    """Every scalar, point and output offset modulo 4: 64 descriptors over four operand pairs."""
    raw = splitmix_np(0x3100, 8 * 32).tobytes()
    inp = bytearray(b"\x22" * 4)
    so, po = {}, {}
    for a in range(4):      # pair a's scalar at alignment a, and its point at every alignment
        for b in range(4):
            while len(inp) % 4 != a:
                inp += b"\x33"
            so[a, b] = len(inp)
            inp += raw[64 * a:64 * a + 32]
            while len(inp) % 4 != b:
                inp += b"\x33"
            po[a, b] = len(inp)
            inp += raw[64 * a + 32:64 * a + 64]
    rows, at = [], 0
    for a in range(4):
        for b in range(4):
            for c in range(4):
                at = (at + 36) // 4 * 4 + c
                rows.append((so[a, b], po[a, b], at))
    d = rig.W.pack_x25519_desc(*(np.array(col, np.uint64) for col in zip(*rows)))
    assert {(int(x["scalar_off"]) & 3, int(x["point_off"]) & 3, int(x["out_off"]) & 3) for x in d} == \
        {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
    _, st = _same(rig, d, bytes(inp), at + 40)
    assert st == [M.X_OK] * 64


def test_ok_zero_and_baddesc_mixed(rig):
    """One batch of OK, ZERO and BADDESC descriptors: each range out of bounds by one byte, off > size, offsets
    near 2^64 (a sum would wrap), an unknown flag bit, a non-zero _pad. The whole output equals the model's,
    which leaves every BADDESC output alone."""
    W = rig.W
    raw = splitmix_np(0x3200, 6 * 32).tobytes()
    inp = raw + le(1) + le(ORDER8[0])  # 256 bytes: points of low order at 192 and 224
    size, out_size = len(inp), 40 * 40 + 40
    rows = []
    for j in range(40):
        rows.append([32 * (j % 6), 32 * ((j + 1) % 6), 3 + 40 * j, 0, 0])
    for j, edit in {1: (1, 192), 5: (1, 224), 9: (0, size - 31), 12: (1, size - 31), 15: (2, out_size - 31),
                    18: (0, size + 1), 20: (1, size + 1), 22: (2, out_size + 1), 24: (0, (1 << 64) - 16),
                    26: (1, (1 << 64) - 1), 28: (2, (1 << 64) - 32), 30: (3, 2), 31: (3, 0x80000001), 33: (4, 1),
                    35: (4, 1 << 31), 37: (2, out_size - 32), 38: (0, size - 32), 39: (1, size)}.items():
        rows[j][edit[0]] = edit[1]
    rows[39][3] = W._lib.WG_X25519_BASE  # BASE: a point range past the buffer does not matter
    d = W.pack_x25519_desc(*(np.array(col, np.uint64) for col in list(zip(*rows))[:4]))
    d["_pad"] = np.array([r[4] for r in rows], np.uint32)
    _, st = _same(rig, d, inp, out_size)
    bad = {9, 12, 15, 18, 20, 22, 24, 26, 28, 30, 31, 33, 35}
    assert [i for i, s in enumerate(st) if s == M.X_BADDESC] == sorted(bad)
    assert [i for i, s in enumerate(st) if s == M.X_ZERO] == [1, 5]


def test_batch_argument_errors(rig):
    torch, dev, W = rig.torch, rig.dev, rig.W
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    d = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(W.WgError) as e:  # out inside in
        rig.eng.x25519(d, buf, buf[64:128], st)
    assert e.value.code == W._lib.WG_EINVAL
    rig.eng.x25519(d[:0], buf[:128], buf[128:], st[:0])  # n = 0: a no-op
    torch.cuda.synchronize()


def test_diffie_hellman_both_sides_on_the_device(rig):
    """64 random pairs: X25519(a, X25519(b, 9)) == X25519(b, X25519(a, 9)), every multiplication on the
    device; the first eight pairs also against the model."""
    raw = splitmix_np(0x3300, 128 * 32).tobytes()
    keys = [raw[32 * k:32 * k + 32] for k in range(128)]
    pubs = [r for r, _ in rig.eng.x25519_host([(k, None) for k in keys])]
    a, b = keys[:64], keys[64:]
    ab = rig.eng.x25519_host([(a[k], pubs[64 + k]) for k in range(64)])
    ba = rig.eng.x25519_host([(b[k], pubs[k]) for k in range(64)])
    assert ab == ba and all(s == M.X_OK for _, s in ab) and len({r for r, _ in ab}) == 64
    for k in range(8):
        assert pubs[k] == model(a[k], M.BASE_POINT) and ab[k][0] == model(a[k], model(b[k], M.BASE_POINT))


# ---- wg_hs_static_set / wg_hs_dh ----------------------------------------------------------------------------
SESS = {0x01020304: 1, 7: 2, 0xFFFFFFF0: 3, 0x80000001: 4}
EPH = [bytes(splitmix_np(0x3400 + k, 32)) for k in range(24)]  # the initiations' ephemerals (the model is memoised)
LOW = [le(0), le(1), le(ORDER8[0]), le(ORDER8[1]), le(M.P), le(M.P + 1)]


def _chain_ring(rng, n_list, pub):
    """A UDP ring whose plan lists exactly n_list handshake datagrams, at unaligned offsets, among transport
    packets: initiations with ephemerals of EPH, initiations with low-order ephemerals, responses, and
    messages with one flipped mac1 bit (they never reach the DH)."""
    known = list(SESS.keys())
    buf, off, lens = bytearray(rng.bytes(3)), [], []

    def put(m):
        off.append(len(buf))
        lens.append(len(m))
        buf.extend(m + rng.bytes(int(rng.integers(0, 4))))

    for k in range(n_list):
        r = rng.random()
        if k in (0, 63, 64, 255, 256) or r < 0.45:
            m = HM.message(1, rng.bytes(7) + EPH[int(rng.integers(0, len(EPH)))] + rng.bytes(76), pub)
        elif r < 0.6:
            m = HM.message(1, rng.bytes(7) + LOW[int(rng.integers(0, len(LOW)))] + rng.bytes(76), pub)
        elif r < 0.85:
            m = HM.message(2, rng.bytes(59), pub)
        else:
            m = HM.message(1 + int(rng.integers(0, 2)), rng.bytes(120), pub)
            at = len(m) - 32 + int(rng.integers(0, 16))
            m = m[:at] + bytes([m[at] ^ 0x04]) + m[at + 1:]
        put(m)
        for _ in range(int(rng.integers(0, 3))):
            wl = int(rng.integers(32, 90))
            put(struct.pack("<BxxxIQ", 4, known[int(rng.integers(0, len(known)))], k) + rng.bytes(wl - 16))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32)


class _Chain:
    """Device buffers of one plan -> check -> dh pipeline over up to n datagrams; run() issues the three calls
    back to back on the current stream, and the host reads nothing in between."""

    def __init__(self, rig, n, ring_size, max_len=120):
        torch, dev = rig.torch, rig.dev
        self.rig, self.n, self.max_len = rig, n, max_len
        self.d_ring = torch.zeros(ring_size, dtype=torch.uint8, device=dev)
        self.d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        self.d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        self.p_st = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_host = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
        self.p_sum = torch.zeros(2, dtype=torch.int64, device=dev)
        self.d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        self.d_rec = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
        self.d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
        self.d_shared = torch.full((n + 1, 32), FILL, dtype=torch.uint8, device=dev)
        self.d_dh = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)

    def load(self, ring, off, lens):
        """The ring at the front of d_ring; packet table entries behind the ring's datagrams have length 0."""
        torch = self.rig.torch
        assert len(ring) <= self.d_ring.numel() and len(off) <= self.n
        self.d_ring.zero_()
        self.d_ring[:len(ring)].copy_(torch.from_numpy(ring))
        o, ln = np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint32)
        o[:len(off)], ln[:len(off)] = off, lens
        self.d_off.copy_(torch.from_numpy(o.view(np.int64)))
        self.d_len.copy_(torch.from_numpy(ln.view(np.int32)))
        self.host = (np.concatenate([ring, np.zeros(self.d_ring.numel() - len(ring), np.uint8)]), o, ln)
        self.d_st.fill_(GUARD)
        self.d_rec.fill_(0x7E)
        self.d_sum.fill_(GUARD)
        self.d_shared.fill_(FILL)
        self.d_dh.fill_(GUARD)

    def run(self, with_summary=True):
        eng, n, w = self.rig.eng, self.n, self.d_ring
        eng.rx_plan(w, self.d_off, self.d_len, self.d_desc, self.p_st, self.d_host, self.p_sum, self.max_len)
        eng.hs_check(w, self.d_off, self.d_len, self.d_st[:n], self.d_rec[:n], self.d_sum[:4], host_list=self.d_host,
                     rx_summary=self.p_sum)
        eng.hs_dh(self.d_rec[:n], self.d_sum[:4] if with_summary else None, self.d_shared[:n], self.d_dh[:n])

    def compare(self, pub, private, with_summary=True):
        """The three calls' outputs against the models; returns (records, dh status list)."""
        self.rig.torch.cuda.synchronize()
        ring, off, lens = self.host
        n = self.n
        _, _, want_host, _ = RM.plan(ring, off, lens, SESS, max_len=self.max_len, mode=RM.PT_AFTER)
        _, rec, s = HM.check(ring, off, lens, pub, lst=want_host)
        sm = self.d_sum.cpu().numpy()
        assert sm[:4].tolist() == [s["n_valid"], s["n_init"], s["n_resp"], s["n_rejected"]] and (sm[4:] == GUARD).all()
        got_rec = self.d_rec.cpu().numpy()
        assert got_rec[:len(rec)].tobytes() == rec.tobytes()
        all_rec = np.ascontiguousarray(got_rec[:n]).view(HM.HS_RECORD).reshape(-1)  # (behind n_valid: 0x7E bytes)
        with _Memo():
            want_sh, want_st = M.hs_dh(all_rec, s["n_valid"] if with_summary else None, n, private,
                                       bytes([FILL]) * (32 * (n + 1)), [GUARD] * (n + 4))
        assert self.d_dh.cpu().numpy().view(np.uint32).tolist() == want_st
        assert self.d_shared.cpu().numpy().tobytes() == want_sh
        return rec, want_st[:s["n_valid"]]


def _engine(rig):
    eng = rig.W.Engine(0, key_slots=16)
    eng.rx_sessions_set(list(SESS.keys()), list(SESS.values()))
    return eng, type("Rig", (), dict(eng=eng, torch=rig.torch, dev=rig.dev, W=rig.W))


def test_static_set_returns_the_public_key_and_sets_the_mac1_key(rig):
    """wg_hs_dh before any wg_hs_static_set: WG_ENOKEY, also after a wg_hs_key_set. wg_hs_static_set returns
    the model's public key, and wg_hs_check then accepts messages made for it; a later wg_hs_key_set
    replaces only the mac1 key."""
    W, torch, dev = rig.W, rig.torch, rig.dev
    eng, rig2 = _engine(rig)
    try:
        ch = _Chain(rig2, 8, 2048)
        pub = M.public_key(ALICE)
        assert pub.hex() == ALICE_PUB
        ring, off, lens = _chain_ring(np.random.default_rng(3500), 3, pub)
        ch.load(ring, off[:8], lens[:8])
        for step in range(2):
            with pytest.raises(W.WgError) as e:
                eng.hs_dh(ch.d_rec[:8], None, ch.d_shared[:8], ch.d_dh[:8])
            assert e.value.code == W._lib.WG_ENOKEY
            eng.hs_key_set(pub)
        assert eng.hs_static_set(ALICE) == pub
        ch.run()
        rec, st = ch.compare(pub, ALICE)
        assert len(rec) >= 1 and st[0] == M.X_OK
        eng.hs_key_set(M.public_key(BOB))  # the mac1 key alone: nothing is accepted, the DH key stays
        ch.load(ring, off[:8], lens[:8])
        ch.run()
        assert len(ch.compare(M.public_key(BOB), ALICE)[0]) == 0
        ch.load(ring, off[:8], lens[:8])
        ch.d_rec[:len(rec)].copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1, 160)))
        eng.hs_dh(ch.d_rec[:8], None, ch.d_shared[:8], ch.d_dh[:8])
        torch.cuda.synchronize()
        assert ch.d_shared[0].cpu().numpy().tobytes() == model(ALICE, rec[0]["msg"][8:40].tobytes())
    finally:
        eng.close()


@pytest.mark.parametrize("n_list", [0, 1, 255, 256, 257])
def test_plan_check_dh_on_one_stream(rig, n_list):
    """wg_rx_plan -> wg_hs_check -> wg_hs_dh back to back, the record count read on the device: shared and
    dh_status equal the model's, nothing is written behind n_valid entries; then n_records = NULL, which
    covers all n records (those behind n_valid hold no message: BADDESC, untouched); then a second static
    key, with no other call in between, changes the results."""
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        assert pub == model(STATIC, M.BASE_POINT)
        rng = np.random.default_rng(3600 + n_list)
        ring, off, lens = _chain_ring(rng, n_list, pub)
        n = len(off) + 5
        ch = _Chain(rig2, n, len(ring) + 64)
        ch.load(ring, off, lens)
        ch.run()
        rec, st = ch.compare(pub, STATIC)
        first = ch.d_shared.cpu().numpy().copy()
        if n_list >= 255:
            assert {M.X_OK, M.X_ZERO, M.X_SKIPPED} == set(st) and 0.5 * n_list < len(rec) < n_list
            assert st[0] == M.X_OK
        ch.load(ring, off, lens)
        ch.run(with_summary=False)
        ch.compare(pub, STATIC, with_summary=False)
        # a second static key: the records are there already, only the DH runs
        pub2 = eng.hs_static_set(STATIC2)
        assert pub2 == model(STATIC2, M.BASE_POINT) and pub2 != pub
        ch.d_shared.fill_(FILL)
        ch.d_dh.fill_(GUARD)
        eng.hs_dh(ch.d_rec[:n], ch.d_sum[:4], ch.d_shared[:n], ch.d_dh[:n])
        rig.torch.cuda.synchronize()
        all_rec = np.ascontiguousarray(ch.d_rec.cpu().numpy()[:n]).view(HM.HS_RECORD).reshape(-1)
        with _Memo():
            want_sh, want_st = M.hs_dh(all_rec, len(rec), n, STATIC2, bytes([FILL]) * (32 * (n + 1)), [GUARD] * (n + 4))
        assert ch.d_dh.cpu().numpy().view(np.uint32).tolist() == want_st
        second = ch.d_shared.cpu().numpy()
        assert second.tobytes() == want_sh
        ok = [k for k, s in enumerate(st) if s == M.X_OK]
        assert all((first[k] != second[k]).any() for k in ok)
    finally:
        eng.close()


def test_captured_plan_check_dh_replay(rig):
    """rx_reserve / hs_reserve, then plan + check + dh captured once and replayed over two different rings; a
    new static key between the replays needs no re-capture (the messages of the second ring are made for
    the new public key)."""
    torch = rig.torch
    eng, rig2 = _engine(rig)
    try:
        pub = eng.hs_static_set(STATIC)
        pub2 = model(STATIC2, M.BASE_POINT)
        rng = np.random.default_rng(3700)
        rings = [_chain_ring(rng, 70, pub), _chain_ring(rng, 90, pub2)]
        n = max(len(r[1]) for r in rings) + 3
        ch = _Chain(rig2, n, max(len(r[0]) for r in rings) + 64)
        eng.rx_reserve(n)
        eng.hs_reserve(n)
        ch.load(*rings[0])
        ch.run()  # eager once
        ch.compare(pub, STATIC)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ch.run()
        counts = []
        for replay, (key, p) in enumerate([(STATIC, pub), (STATIC2, pub2)]):
            if replay == 1:
                assert eng.hs_static_set(STATIC2) == pub2
            ch.load(*rings[replay])
            torch.cuda.synchronize()
            g.replay()
            rec, st = ch.compare(p, key)
            counts.append((len(rec), st.count(M.X_OK)))
        assert all(a > 30 and b > 15 for a, b in counts)
    finally:
        eng.close()


# ---- the mirror ---------------------------------------------------------------------------------------------------
def test_mirror_agreement_and_private_key(rig):
    N = noise()
    r = bytearray(b"\x5a" * 34)
    assert N.X25519.calculateAgreement(ALICE, 0, le(ORDER8[0]), 0, r, 1) is False
    assert bytes(r) == b"\x5a" + bytes(32) + b"\x5a"
    assert N.X25519.calculateAgreement(b"?" + ALICE, 1, b"??" + H(BOB_PUB), 2, r, 1) is True
    assert bytes(r[1:33]).hex() == SHARED
    N.X25519.scalarMult(K1, 0, U1, 0, r, 0)
    assert bytes(r[:32]).hex() == R1
    N.X25519.scalarMultBase(BOB, 0, r, 2)
    assert bytes(r[2:34]).hex() == BOB_PUB
    a, b = N.NoisePrivateKey(ALICE), N.NoisePrivateKey(BOB)
    assert a.publicKey().data().hex() == ALICE_PUB and b.publicKey().data().hex() == BOB_PUB
    assert a.sharedSecret(b.publicKey()).data().hex() == SHARED == b.sharedSecret(a.publicKey()).data().hex()
    assert a.sharedSecret(N.NoisePublicKey(le(1))).data() == bytes(32)  # the bool is ignored
    k = N.NoisePrivateKey.newPrivateKey()
    assert bytes(k.data()) == M.clamp(bytes(k.data())) and k.publicKey().data() == model(bytes(k.data()), M.BASE_POINT)
