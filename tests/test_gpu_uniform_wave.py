"""The uniform-wave body of the transport kernel (wg_transport.hip, transport_body_uni) on an MI355X
(pytest -m gpu): waves whose 8 slots hold valid packets of one length, 16-B aligned, under one key take
it; every other wave of the same launch takes transport_body. Every byte against the oracle, no
tolerance. Engines are created with WG_UNIFORM16=0, so small batches take 8-lane slots."""
import os

import numpy as np
import pytest

from wgtest import oracle, splitmix_np, wg

pytestmark = pytest.mark.gpu
O = oracle()
SENT = 0xA5  # prefill of every output buffer: bytes no packet owns must keep it
BADTAG = 1


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def _engine(env=None, key_slots=4):
    """An engine created under WG_UNIFORM16=0 (and `env`); the knobs are read at creation only."""
    env = dict(env or {}, WG_UNIFORM16="0")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = wg().Engine(0, key_slots=key_slots)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    keys = splitmix_np(0x517, 32 * key_slots)
    e.set_keys(0, keys.tobytes())
    return e, keys


@pytest.fixture(scope="module")
def eng():
    e, keys = _engine()
    yield e, keys
    e.close()


def _offsets(n, max_len):
    """Packet i's 16-B aligned base, with room for a shift of up to 15 bytes and the tag."""
    stride = ((max_len + 16 + 15) // 16) * 16 + 32
    return (np.arange(n, dtype=np.int64) * stride + 16), n * stride + 64


class Case:
    """One batch: seal descriptors (in_off -> ct_off), open descriptors (ct_off -> back_off), the oracle's
    ciphertext buffer and the expected plaintext buffer. `invalid`: packets whose descriptor the kernel must
    reject (the oracle skips them; their output stays at the sentinel, their open status is BADTAG)."""

    def __init__(self, lens, in_off, ct_off, back_off, size, keys, slots=None, max_len=None, invalid=(), seed=1):
        W = wg()
        n = len(lens)
        self.n, self.size, self.keys = n, size, keys
        self.lens = np.asarray(lens, np.int64)
        self.max_len = int(self.lens.max()) if max_len is None else max_len
        self.slots = np.zeros(n, np.int64) if slots is None else np.asarray(slots, np.int64)
        self.ctr = np.arange(n, dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(seed)
        self.in_off, self.ct_off, self.back_off = (np.asarray(a, np.uint64) for a in (in_off, ct_off, back_off))
        self.valid = np.ones(n, bool)
        self.valid[list(invalid)] = False
        self.pt = splitmix_np(0xAB00 + seed, size)
        self.desc_s = W.pack_desc(self.in_off, self.ct_off, self.ctr, self.lens, self.slots)
        self.desc_o = W.pack_desc(self.ct_off, self.back_off, self.ctr, self.lens, self.slots)
        self.ref = np.full(size, SENT, np.uint8)
        O.seal_batch(self.desc_s[self.valid], self.pt, self.ref, keys, threads=4)
        self.exp_back = np.full(size, SENT, np.uint8)
        for i in np.nonzero(self.valid)[0]:
            a, b, L = int(self.in_off[i]), int(self.back_off[i]), int(self.lens[i])
            self.exp_back[b:b + L] = self.pt[a:a + L]
        self.exp_st = np.where(self.valid, 0, BADTAG)

    def dev(self, a):
        torch, dev = _dev()
        return torch.from_numpy(a).to(dev)

    def check_seal(self, engine):
        W = wg()
        torch, dev = _dev()
        dct = self.dev(np.full(self.size, SENT, np.uint8))
        engine.seal(self.dev(W.desc_as_int64(self.desc_s)), self.dev(self.pt), dct, self.max_len, uniform=True)
        torch.cuda.synchronize()
        self._same(dct.cpu().numpy(), self.ref, self.ct_off, 16, "seal")

    def check_open(self, engine, forged=()):
        """Open the oracle's ciphertext; `forged`: packets with one ciphertext bit flipped first."""
        W = wg()
        torch, dev = _dev()
        ct = self.ref.copy()
        exp, st_exp = self.exp_back.copy(), self.exp_st.copy()
        for i in forged:
            L = int(self.lens[i])
            ct[int(self.ct_off[i]) + L // 2] ^= 0x04
            exp[int(self.back_off[i]):int(self.back_off[i]) + L] = 0  # the plaintext range is scrubbed
            st_exp[i] = BADTAG
        dback = self.dev(np.full(self.size, SENT, np.uint8))
        st = self.dev(np.full(self.n, 9, np.int32))
        engine.open(self.dev(W.desc_as_int64(self.desc_o)), self.dev(ct), dback, st, self.max_len, uniform=True)
        torch.cuda.synchronize()
        assert st.cpu().numpy().tolist() == st_exp.tolist()
        self._same(dback.cpu().numpy(), exp, self.back_off, 0, "open")

    def check_step(self, engine):
        """wg_duplex_batch(seal, open | WG_F_AFTER_SEAL): one k_step launch."""
        W = wg()
        torch, dev = _dev()
        dct = self.dev(np.full(self.size, SENT, np.uint8))
        dback = self.dev(np.full(self.size, SENT, np.uint8))
        st = self.dev(np.full(self.n, 9, np.int32))
        engine.duplex(self.dev(W.desc_as_int64(self.desc_s)), self.dev(self.pt), dct, self.max_len,
                      self.dev(W.desc_as_int64(self.desc_o)), dct, dback, st, self.max_len, uniform=True,
                      after_seal=True)
        torch.cuda.synchronize()
        self._same(dct.cpu().numpy(), self.ref, self.ct_off, 16, "step seal")
        assert st.cpu().numpy().tolist() == self.exp_st.tolist()
        self._same(dback.cpu().numpy(), self.exp_back, self.back_off, 0, "step open")

    def _same(self, got, want, off, extra, what):
        if np.array_equal(got, want):
            return
        for i in range(self.n):  # name the first packet that differs
            o, L = int(off[i]), int(self.lens[i]) + extra
            assert np.array_equal(got[o:o + L], want[o:o + L]), f"{what}: packet {i} (len {self.lens[i]})"
        raise AssertionError(f"{what}: bytes outside every packet's range were written")


# chunk and block edges, the end of round 0 and 1 (448, 960 B), a whole number of blocks (1472), lengths whose
# MAC front padding is zero (112, 1520), lengths whose length block is taken at the finish (448, 960, 1472),
# the keepalive (0)
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 112, 447, 448, 449, 511, 512, 513, 960, 1420, 1424, 1472, 1520, 2048]


@pytest.mark.parametrize("L", LENGTHS)
def test_one_length(eng, L):
    """n = 77: nine full waves and a wave with five live slots, all uniform."""
    engine, keys = eng
    n = 77
    base, size = _offsets(n, L)
    c = Case(np.full(n, L), base, base, base, size, keys, seed=L + 1)
    c.check_seal(engine)
    c.check_open(engine)
    c.check_step(engine)


FALLBACK = ["short_mid", "bad_len", "bad_off", "in1_one", "in4_one", "in1_all", "in4_all", "out4", "keys_alt"]


@pytest.mark.parametrize("what", FALLBACK)
def test_waves_that_fall_back(eng, what):
    """L = 1420, n = 64: a wave with any packet off the pattern runs transport_body; the other waves of the
    launch stay on the uniform body. An invalid descriptor's seal output stays at the sentinel, its open
    status is BADTAG, its seven neighbours are exact."""
    engine, keys = eng
    n, L = 64, 1420
    base, size = _offsets(n, L + 1)
    lens = np.full(n, L)
    in_off, ct_off, back_off = base.copy(), base.copy(), base.copy()
    slots, invalid, max_len = None, (), L
    if what == "short_mid":
        lens[27] = 1419
    elif what == "bad_len":
        lens[13] = L + 1  # > max_len
        invalid = (13,)
    elif what == "bad_off":
        invalid = (13,)
    elif what.startswith("in"):
        k = int(what[2])
        sel = slice(None) if what.endswith("all") else 27
        in_off[sel] += k   # the seal's input
        ct_off[sel] += k   # the seal's output = the open's input
    elif what == "out4":
        ct_off += 4
        back_off += 4
    elif what == "keys_alt":
        slots = np.arange(n) % 2
    c = Case(lens, in_off, ct_off, back_off, size, keys, slots=slots, max_len=max_len, invalid=invalid, seed=7)
    if what == "bad_off":  # out of range in both directions' input
        c.desc_s["in_off"][13] = size + 1
        c.desc_o["in_off"][13] = 1 << 40
    c.check_seal(engine)
    c.check_open(engine)
    c.check_step(engine)


def test_in_place_seal(eng):
    engine, keys = eng
    W = wg()
    torch, dev = _dev()
    n, L = 64, 1420
    base, size = _offsets(n, L)
    c = Case(np.full(n, L), base, base, base, size, keys, seed=11)
    want = c.pt.copy()
    O.seal_batch(c.desc_s, c.pt, want, keys, threads=4)
    buf = c.dev(c.pt.copy())
    engine.seal(c.dev(W.desc_as_int64(c.desc_s)), buf, buf, L, uniform=True)
    torch.cuda.synchronize()
    c._same(buf.cpu().numpy(), want, c.ct_off, 16, "in-place seal")


@pytest.mark.parametrize("L", [1420, 449])
def test_forged_packet_in_a_uniform_wave(eng, L):
    engine, keys = eng
    n = 77
    base, size = _offsets(n, L)
    c = Case(np.full(n, L), base, base, base, size, keys, seed=13)
    c.check_open(engine, forged=(3, 42, 76))


def test_receive_filter_over_uniform_waves(eng):
    """WG_F_RX_FILTER on an open whose waves are uniform: the verdicts of open followed by wg_rx_check."""
    engine, keys = eng
    W = wg()
    torch, dev = _dev()
    engine.filter_set(0, [("10.0.0.0", 8), ("2001:db8::", 32)])
    engine.slot_filters_set(0, [0])
    n, L = 77, 300
    base, size = _offsets(n, L)
    c = Case(np.full(n, L), base, base, base, size, keys, seed=17)
    rng = np.random.default_rng(5)
    for i in range(n):  # IP-ish plaintexts: v4 inside / outside the prefix, v6, a bad version nibble
        o = int(base[i])
        kind = i % 5
        if kind < 3:
            c.pt[o] = 0x45
            c.pt[o + 16] = 10 if kind < 2 else 11
        elif kind == 3:
            c.pt[o] = 0x60
            c.pt[o + 24:o + 28] = [0x20, 0x01, 0x0d, 0xb8] if rng.random() < 0.5 else [0x20, 0x01, 0x0d, 0xb9]
        else:
            c.pt[o] = 0x85
    c.ref[:] = SENT
    O.seal_batch(c.desc_s, c.pt, c.ref, keys, threads=4)
    ct = c.ref.copy()
    ct[int(base[9]) + 5] ^= 1  # one forged packet
    d = c.dev(W.desc_as_int64(c.desc_o))
    dct = c.dev(ct)
    back = c.dev(np.full(size, SENT, np.uint8))
    st_fused = c.dev(np.full(n, 9, np.int32))
    engine.open(d, dct, back, st_fused, L, uniform=True, rx_filter=True)
    back2 = c.dev(np.full(size, SENT, np.uint8))
    st2 = c.dev(np.full(n, 9, np.int32))
    engine.open(d, dct, back2, st2, L, uniform=True)
    engine.rx_check(d, back2, st2, W._lib.WG_RX_FILTER)
    torch.cuda.synchronize()
    got, want = st_fused.cpu().numpy().tolist(), st2.cpu().numpy().tolist()
    assert got == want
    assert {0, 1, 4, 5} <= set(want)  # OK, BADTAG, BADIP, FILTERED all occur
    assert np.array_equal(back.cpu().numpy(), back2.cpu().numpy())


@pytest.mark.parametrize("ragged", [False, True])
def test_knob_parity(ragged):
    """WG_UNI=0 (k_transport<MODE, 8> / k_step<8>) and WG_UNI=1 write the same bytes: one seeded uniform batch
    and one ragged WG_F_UNIFORM batch (lengths 1400..1420 mixed)."""
    W = wg()
    torch, dev = _dev()
    n = 200
    lens = (1400 + splitmix_np(31, n).astype(np.int64) % 21) if ragged else np.full(n, 1420)
    base, size = _offsets(n, 1420)
    out = {}
    for knob in ("0", "1"):
        engine, keys = _engine({"WG_UNI": knob})
        try:
            c = Case(lens, base, base, base, size, keys, max_len=1420, seed=19)
            dct = c.dev(np.full(size, SENT, np.uint8))
            dback = c.dev(np.full(size, SENT, np.uint8))
            st = c.dev(np.full(n, 9, np.int32))
            ds, do = c.dev(W.desc_as_int64(c.desc_s)), c.dev(W.desc_as_int64(c.desc_o))
            engine.seal(ds, c.dev(c.pt), dct, 1420, uniform=True)
            engine.open(do, dct, dback, st, 1420, uniform=True)
            dct2 = c.dev(np.full(size, SENT, np.uint8))
            dback2 = c.dev(np.full(size, SENT, np.uint8))
            st2 = c.dev(np.full(n, 9, np.int32))
            engine.duplex(ds, c.dev(c.pt), dct2, 1420, do, dct2, dback2, st2, 1420, uniform=True, after_seal=True)
            torch.cuda.synchronize()
            out[knob] = [t.cpu().numpy() for t in (dct, dback, st, dct2, dback2, st2)]
            assert np.array_equal(out[knob][0], c.ref) and np.array_equal(out[knob][1], c.exp_back)
            assert (out[knob][2] == 0).all()
        finally:
            engine.close()
    for a, b in zip(out["0"], out["1"]):
        assert np.array_equal(a, b)
