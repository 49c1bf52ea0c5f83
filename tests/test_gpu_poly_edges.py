"""Poly1305 edge states on every kernel that computes a tag (pytest -m gpu), steered through the ciphertext by
tests/poly_edge_model.py: final accumulators at 0 .. 6, p - 1 .. p - 6, around 2^128 and 2^129, and tags whose
`+ s` carries through every word (00 .. 00, ff .. ff), under all-ones, all-zero and random ciphertext, with the
solved block first, in the middle or last in the packet. Each path opens the steered ct || tag (OK, the exact
plaintext), opens it with the tag's last byte changed (BADTAG, the range scrubbed, the neighbours exact) and seals
pt = ct XOR keystream (exactly ct || tag). Expected bytes are the oracle's and the model's; nothing is read back
from the device to form them. Output buffers are prefilled with a sentinel that bytes no packet owns must keep.

Which representation of a residue a kernel hands to poly_finish is modelled for the per-packet server and for the
handshake chains' poly_tag only (poly_edge_model's docstring): there the tests assert on the CPU that the cases at
residues 0 .. 4 enter it in [p, 2^130). The other kernels run the same residues without that claim.

The raw one-time-key cases at the end go through WG_MODE_MAC (k_tile), the only place where r can be chosen."""
import functools
import os
import random

import numpy as np
import pytest

import hs_open_model as OM
import poly_edge_model as PM
import x25519_model as XM
from wgtest import oracle, splitmix_bytes, splitmix_np, wg

pytestmark = pytest.mark.gpu
O = oracle()
SENT = 0xA5
OK, BADTAG = 0, 1
KEY_SLOTS = 4
KEYS = splitmix_np(0x517, 32 * KEY_SLOTS)
NT = len(PM.TARGETS)
POSITIONS = ("first", "middle", "last")


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def _engine(env=None):
    """An engine created under `env`; the plan knobs are read at creation only."""
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = wg().Engine(0, key_slots=KEY_SLOTS)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.set_keys(0, KEYS.tobytes())
    return e


def _free_block(pos, nfull):
    return {"first": 0, "middle": nfull // 2, "last": nfull - 1}[pos]


class Steered:
    """One seeded batch: packet i takes target i mod len(TARGETS), and over the batch's repeats of a target
    another fill and another position of the solved block. `wire` holds every ct || tag, `plain` every plaintext
    (the oracle's open of `wire`), both over the sentinel."""

    def __init__(self, lens, seed, one_key=False):
        W = wg()
        n = len(lens)
        self.n, self.lens = n, np.asarray(lens, np.int64)
        self.max_len = int(self.lens.max())
        stride = ((self.max_len + 16 + 15) // 16) * 16 + 32
        self.off = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(16)
        self.size = n * stride + 64
        slots = np.zeros(n, np.int64) if one_key else np.arange(n) % KEY_SLOTS
        ctr = np.arange(n, dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(seed)
        self.desc = W.pack_desc(self.off, self.off, ctr, self.lens, slots)
        self.wire = np.full(self.size, SENT, np.uint8)
        self.what = []
        for i in range(n):
            rep = i // NT
            target = PM.TARGETS[(i + seed) % NT]
            fill = PM.FILLS[(i + rep) % 3]
            pos = POSITIONS[(i // 3 + rep) % 3]
            L, key = int(self.lens[i]), KEYS[32 * slots[i]:32 * slots[i] + 32].tobytes()
            H = PM.resolve(target, key, int(ctr[i]))
            ct = PM.steer(key, int(ctr[i]), L, _free_block(pos, L // 16), H, fill, random.Random(1000 * seed + i))
            o = int(self.off[i])
            self.wire[o:o + L + 16] = np.frombuffer(ct + PM.tag_of(key, int(ctr[i]), ct), np.uint8)
            self.what.append(f"packet {i}: len {L}, {PM.label(target)}, fill {fill}, solved block {pos}")
        self.plain = np.full(self.size, SENT, np.uint8)
        assert not O.open_batch(self.desc, self.wire, self.plain, KEYS, threads=4).any()
        again = np.full(self.size, SENT, np.uint8)
        O.seal_batch(self.desc, self.plain, again, KEYS, threads=4)
        assert np.array_equal(again, self.wire)  # the oracle's seal of that plaintext is the steered ct || tag
        self.forged = [i for i in range(n) if i % 4 == 1]  # every forged packet between two intact ones

    # -- device buffers ------------------------------------------------------------------------------------
    def t(self, a):
        torch, dev = _dev()
        return torch.from_numpy(a).to(dev)

    def d_desc(self):
        return self.t(wg().desc_as_int64(self.desc))

    def fresh(self):
        return self.t(np.full(self.size, SENT, np.uint8))

    def status(self):
        return self.t(np.full(self.n, 9, np.int32))

    def forged_wire(self):
        """(wire with the last tag byte of every forged packet changed, expected plaintext buffer, statuses)."""
        wire, exp, st = self.wire.copy(), self.plain.copy(), np.zeros(self.n, np.int64)
        for i in self.forged:
            o, L = int(self.off[i]), int(self.lens[i])
            wire[o + L + 15] ^= 0x80
            exp[o:o + L] = 0
            st[i] = BADTAG
        return wire, exp, st

    # -- comparisons -----------------------------------------------------------------------------------------
    def same(self, got, want, extra, what):
        if np.array_equal(got, want):
            return
        for i in range(self.n):  # name the first packet that differs
            o, L = int(self.off[i]), int(self.lens[i]) + extra
            assert np.array_equal(got[o:o + L], want[o:o + L]), f"{what}: {self.what[i]}"
        raise AssertionError(f"{what}: bytes outside every packet's range were written")

    def same_status(self, st, want, what):
        got = st.cpu().numpy().tolist()
        for i in range(self.n):
            assert got[i] == want[i], f"{what}: status {got[i]}, {self.what[i]}"

    # -- the three checks, and the one-launch forms -------------------------------------------------------------
    def check_open(self, engine, uniform):
        torch, _ = _dev()
        back, st = self.fresh(), self.status()
        engine.open(self.d_desc(), self.t(self.wire), back, st, self.max_len, uniform=uniform)
        torch.cuda.synchronize()
        self.same_status(st, [OK] * self.n, "open")
        self.same(back.cpu().numpy(), self.plain, 0, "open")

    def check_open_forged(self, engine, uniform):
        torch, _ = _dev()
        wire, exp, exp_st = self.forged_wire()
        back, st = self.fresh(), self.status()
        engine.open(self.d_desc(), self.t(wire), back, st, self.max_len, uniform=uniform)
        torch.cuda.synchronize()
        self.same_status(st, exp_st, "open of forged tags")
        self.same(back.cpu().numpy(), exp, 0, "open of forged tags")

    def check_seal(self, engine, uniform):
        torch, _ = _dev()
        ct = self.fresh()
        engine.seal(self.d_desc(), self.t(self.plain), ct, self.max_len, uniform=uniform)
        torch.cuda.synchronize()
        self.same(ct.cpu().numpy(), self.wire, 16, "seal")

    def check_step(self, engine, uniform):
        """duplex(..., after_seal=True): seal, and open what was sealed, in one launch."""
        torch, _ = _dev()
        ct, back, st = self.fresh(), self.fresh(), self.status()
        d = self.d_desc()
        engine.duplex(d, self.t(self.plain), ct, self.max_len, d, ct, back, st, self.max_len, uniform=uniform,
                      after_seal=True)
        torch.cuda.synchronize()
        self.same(ct.cpu().numpy(), self.wire, 16, "step seal")
        self.same_status(st, [OK] * self.n, "step open")
        self.same(back.cpu().numpy(), self.plain, 0, "step open")

    def check_all(self, engine, uniform, step=True):
        self.check_open(engine, uniform)
        self.check_open_forged(engine, uniform)
        self.check_seal(engine, uniform)
        if step:
            self.check_step(engine, uniform)


def check_duplex(engine, a, b, uniform):
    """One duplex launch that seals batch a and opens batch b, some of b's tags forged."""
    torch, _ = _dev()
    wire, exp, exp_st = b.forged_wire()
    ct, back, st = a.fresh(), b.fresh(), b.status()
    engine.duplex(a.d_desc(), a.t(a.plain), ct, a.max_len, b.d_desc(), b.t(wire), back, st, b.max_len, uniform=uniform)
    torch.cuda.synchronize()
    a.same(ct.cpu().numpy(), a.wire, 16, "duplex seal")
    b.same_status(st, exp_st, "duplex open")
    b.same(back.cpu().numpy(), exp, 0, "duplex open")


@functools.lru_cache(maxsize=None)
def uniform_batch(L, one_key):
    return Steered([L] * 64, seed=L, one_key=one_key)


MIXED = (48, 112, 448, 576, 1500, 2048)


@functools.lru_cache(maxsize=None)
def mixed_batch(seed):
    return Steered([MIXED[(i + i // len(MIXED)) % len(MIXED)] for i in range(64)], seed=seed)


# ---- the uniform-wave body and its fallback ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def uni_engines():
    engines = {}

    def get(knob):
        if knob not in engines:
            engines[knob] = _engine({"WG_UNIFORM16": "0", "WG_UNI": knob})
        return engines[knob]
    yield get
    for e in engines.values():
        e.close()


# 48: the smallest packet with a solved block, a salt block and one more; 64: one whole ChaCha20 block; the ends of
# round 0 and 1 (448, 960) and a whole number of blocks (1472), whose length block is taken at the finish; one chunk
# past a round's end (464); 1424: the longest multiple of 16 under the benchmark's 1420 + 16
UNIFORM = [(L, "1", True) for L in (48, 64, 448, 464, 960, 1424, 1472)] + \
    [(448, "1", False), (1424, "1", False), (448, "0", True), (1424, "0", True)]


@pytest.mark.parametrize("L,knob,one_key", UNIFORM, ids=lambda v: {True: "one_key", False: "four_keys"}.get(v, str(v)))
def test_uniform_waves(uni_engines, L, knob, one_key):
    """WG_F_UNIFORM batches of 64 packets of one length. Under one key every wave takes the uniform-wave body
    (WG_UNI=1); with the keys alternating no wave is uniform and the same launch runs its fallback body; WG_UNI=0
    is the 8-lane slots the body replaced (k_transport<MODE, 8> / k_step<8>)."""
    uniform_batch(L, one_key).check_all(uni_engines(knob), uniform=True)


# ---- mixed plans -----------------------------------------------------------------------------------------------------

# the default plan of a small mixed batch (the long packets in 16-lane slots, the rest in 8), 16-lane slots, 4-lane
# slots, long packets in 16 and the rest in 4 lanes (its step puts the shortest in 2-lane slots), the same with the
# 2-lane part off, and WG_SLOT2=2 on the default plan
PLANS = [{}, {"WG_SLOT16": "1"}, {"WG_SLOT4": "1"}, {"WG_SLOT4": "2"}, {"WG_SLOT4": "2", "WG_SLOT2": "2"},
         {"WG_SLOT2": "2"}]


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "default")
def test_mixed_plans(plan):
    """64 packets of 48 .. 2048 B without WG_F_UNIFORM: seal, open, the one-launch step, and a duplex launch over
    two separate batches."""
    engine = _engine(plan)
    try:
        a, b = mixed_batch(1), mixed_batch(2)
        a.check_all(engine, uniform=False)
        check_duplex(engine, a, b, uniform=False)
    finally:
        engine.close()


@pytest.mark.parametrize("kernel", ["tile", "wave1"])
def test_selectable_kernels(kernel):
    engine = _engine()
    try:
        engine.set_kernel(kernel)
        mixed_batch(3).check_all(engine, uniform=False, step=False)
    finally:
        engine.set_kernel("default")
        engine.close()


# ---- the per-packet server ---------------------------------------------------------------------------------------------

def _pp_roundtrip(engine, key, counter, ct, what):
    nonce = O.transport_nonce(counter)
    sealed = ct + PM.tag_of(key, counter, ct)
    pt = O.py_chacha20(key, nonce, 1, ct)
    engine.set_keys(0, key)
    assert engine.open1(0, counter, sealed) == pt, f"open1: {what}"
    assert engine.open1(0, counter, sealed[:-1] + bytes([sealed[-1] ^ 0x80])) is None, f"open1 of a forged tag: {what}"
    assert engine.seal1(0, counter, pt) == sealed, f"seal1: {what}"


@pytest.fixture(scope="module")
def pp_engine():
    e = wg().Engine(0, key_slots=KEY_SLOTS)
    yield e
    e.close()


@pytest.mark.parametrize("L", [48, 1424])
def test_per_packet_server_every_target(pp_engine, L):
    for ti, target in enumerate(PM.TARGETS):
        key = splitmix_bytes(0x9900 + 100 * L + ti, 32)
        counter = (ti << 32) | L
        pos = POSITIONS[ti % 3]
        ct = PM.steer(key, counter, L, _free_block(pos, L // 16), PM.resolve(target, key, counter),
                      PM.FILLS[(ti // 3) % 3], random.Random(ti))
        _pp_roundtrip(pp_engine, key, counter, ct, f"len {L}, {PM.label(target)}, solved block {pos}")


@pytest.mark.parametrize("L", [48, 1424])
def test_per_packet_server_takes_the_select(pp_engine, L):
    """Cases whose accumulator, as mac_tag's lanes form it (poly_edge_model.pp_prefinish), enters poly_finish at
    residue + p: a select that keeps h, or a g with a wrong carry, gives another tag."""
    cases = PM.pp_select_cases(L)
    assert len(cases) >= 4
    for key, counter, ct, H in cases:
        _pp_roundtrip(pp_engine, key, counter, ct, f"len {L}, residue {H} entering poly_finish as p + {H}")


# ---- the general AEAD: aad blocks in front, an explicit nonce -----------------------------------------------------------

AEAD_TARGETS = [("H", 0), ("H", 4), ("H", PM.P - 1), ("H", 1 << 128), ("H", 1 << 129), ("T", bytes(16), 0),
                ("T", bytes(16), 3), ("T", b"\xff" * 16, 1)]


def test_general_aead_seal_and_open():
    """Engine.aead in WG_MODE_SEAL / WG_MODE_OPEN (k_tile with AAD): eight 64-B packets with a 12-byte AAD."""
    W = wg()
    torch, dev = _dev()
    n, L, A = len(AEAD_TARGETS), 64, 12
    aad = splitmix_np(0xAAD, 16 * n)
    d_seal, d_open = np.zeros(n, W.engine.WG_AEAD_DTYPE), np.zeros(n, W.engine.WG_AEAD_DTYPE)
    pt_buf = np.full(96 * n, SENT, np.uint8)
    ct_buf = np.full(96 * n, SENT, np.uint8)
    for i, target in enumerate(AEAD_TARGETS):
        key = KEYS[32 * (i % KEY_SLOTS):32 * (i % KEY_SLOTS) + 32].tobytes()
        nonce = splitmix_bytes(0x0E0 + i, 12)
        a = aad[16 * i:16 * i + A].tobytes()
        ct = PM.steer(key, 0, L, i % 4, PM.resolve(target, key, 0, nonce), PM.FILLS[i % 3], random.Random(i), aad=a,
                      nonce=nonce)
        sealed = ct + PM.tag_of(key, 0, ct, a, nonce)
        pt = O.py_aead_open(key, nonce, sealed, a)
        assert pt is not None and O.py_aead_seal(key, nonce, pt, a) == sealed
        pt_buf[96 * i:96 * i + L] = np.frombuffer(pt, np.uint8)
        ct_buf[96 * i:96 * i + L + 16] = np.frombuffer(sealed, np.uint8)
        for d in (d_seal, d_open):
            d["in_off"][i] = d["out_off"][i] = 96 * i
            d["aad_off"][i], d["len"][i], d["aad_len"][i], d["key_slot"][i] = 16 * i, L, A, i % KEY_SLOTS
            d["nonce"][i] = np.frombuffer(nonce, "<u4")
    engine = _engine()
    try:
        def dev_of(a):
            return torch.from_numpy(a).to(dev)
        d_aad = dev_of(aad)
        out = dev_of(np.full(96 * n, SENT, np.uint8))
        engine.aead(W._lib.WG_MODE_SEAL, dev_of(W.desc_as_int64(d_seal)), dev_of(pt_buf), d_aad, out, None, L)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ct_buf)
        forged, exp, exp_st = ct_buf.copy(), pt_buf.copy(), [OK] * n
        for i in (1, 5, 6):
            forged[96 * i + L + 15] ^= 0x80
            exp[96 * i:96 * i + L] = 0
            exp_st[i] = BADTAG
        for wire, want, want_st in ((ct_buf, pt_buf, [OK] * n), (forged, exp, exp_st)):
            back = dev_of(np.full(96 * n, SENT, np.uint8))
            st = dev_of(np.full(n, 9, np.int32))
            engine.aead(W._lib.WG_MODE_OPEN, dev_of(W.desc_as_int64(d_open)), dev_of(wire), d_aad, back, st, L)
            torch.cuda.synchronize()
            assert st.cpu().numpy().tolist() == want_st
            assert np.array_equal(back.cpu().numpy(), want)
    finally:
        engine.close()


# ---- the handshake chains' poly_tag -------------------------------------------------------------------------------------

def test_initiations_with_a_steered_encrypted_static():
    """wg_hs_open's AEAD over encrypted_static (32 B of ciphertext, the chain hash as AAD). The hash covers only
    what precedes encrypted_static and the key comes from the ephemeral, so the ciphertext can be steered: the
    device must accept all eight (the static they decrypt to belongs to no peer: NEWPEER, with that static in the
    entry) and reject each with its tag's last byte changed. poly_tag's Horner loop is the serial form that
    poly_edge_model restates: the residues 0 .. 4 are asserted to enter poly_finish at residue + p."""
    local_private = bytes(splitmix_np(0x6E00, 32))
    local_public = XM.public_key(local_private)
    targets = [("H", v) for v in range(5)] + [("H", PM.P - 1), ("T", bytes(16), 0), ("T", b"\xff" * 16, 2)]
    engine = wg().Engine(0, key_slots=KEY_SLOTS)
    try:
        assert engine.hs_static_set(local_private) == local_public
        for i, target in enumerate(targets):
            eph_private = bytes(splitmix_np(0x6E10 + i, 32))
            eph = XM.public_key(eph_private)
            ss = OM.x25519(local_private, eph)
            h = OM.blake2s(OM.blake2s(OM.INITIAL_HASH, local_public), eph)
            ck = OM.derive_key(OM.INITIAL_CHAIN_KEY, eph)
            key = OM.derive_key(ck, ss, 2)
            H = PM.resolve(target, key, 0, OM.ZERO_NONCE)
            ct = PM.steer(key, 0, 32, i % 2, H, "rand", random.Random(i), aad=h, nonce=OM.ZERO_NONCE)
            otk = PM.one_time_key(key, 0, OM.ZERO_NONCE)
            if H < 5:
                _, took, v = PM.finish(PM.serial_prefinish(otk, PM.mac_input(ct, h)), PM.r_s(otk)[1])
                assert took and v == PM.P + H
            enc_static = ct + PM.tag_of(key, 0, ct, h, OM.ZERO_NONCE)
            enc_ts = bytes(splitmix_np(0x6E20 + i, 28))
            want_st, want = OM.open_one(local_private, local_public, eph, enc_static, enc_ts, ss, [])
            assert want_st == OM.OPEN_NEWPEER
            st, entry = engine.hs_open_host(eph, enc_static, enc_ts)
            assert st == OM.OPEN_NEWPEER, PM.label(target)
            for f in ("remote_static", "hash", "chain_key"):
                assert entry[f].tobytes() == want[f], (PM.label(target), f)
            st, entry = engine.hs_open_host(eph, enc_static[:-1] + bytes([enc_static[-1] ^ 0x80]), enc_ts)
            assert (st, entry) == (OM.OPEN_BADAUTH, None), PM.label(target)
    finally:
        engine.close()


# ---- raw one-time keys on k_tile ----------------------------------------------------------------------------------------

def test_raw_mac_extremes(engine):
    """WG_MODE_MAC with chosen r and s: the largest clamped r under all-ones messages across the 63 / 64 block
    boundary and with every partial last block, r = 0, r = 1, sums that land on p, p - 1, 2^130 and 2 p, and tags
    whose carry runs through every word. Expected tags: the oracle's big-integer Poly1305."""
    W = wg()
    cases = PM.raw_mac_cases()
    descs, msgs, at = [], bytearray(), 0
    for i, (_, _, msg, _) in enumerate(cases):
        d = W._lib.WgAeadDesc()
        d.in_off, d.out_off, d.len, d.key_slot = at, 16 * i, len(msg), i
        descs.append(d)
        msgs += msg + bytes(-len(msg) % 16)
        at = len(msgs)
    out, _ = engine.aead_host(W._lib.WG_MODE_MAC, descs, b"".join(c[1] for c in cases), bytes(msgs), b"", 16 * len(cases))
    for i, (name, otk, msg, _) in enumerate(cases):
        assert out[16 * i:16 * i + 16] == O.py_poly1305(otk, msg), name
