"""The CPU model of wg_hs_open (tests/hs_open_model.py) against the standard library and against itself, and
the binding's layouts against include/wgaead.h. No GPU."""
import ctypes
import hashlib
import hmac as std_hmac
import os
import subprocess

import numpy as np
import pytest

import hs_model as HM
import hs_open_model as OM
import x25519_model as XM
from wgtest import ROOT, noise, splitmix_bytes, wg

RESPONDER = splitmix_bytes(0x4100, 32)
INITIATOR = splitmix_bytes(0x4101, 32)
EPHEMERAL = splitmix_bytes(0x4102, 32)
TIMESTAMP = splitmix_bytes(0x4103, 12)


@pytest.fixture(scope="module")
def hello():
    """One genuine initiation from INITIATOR to RESPONDER, and what the responder's DH gives for it."""
    pub = XM.public_key(RESPONDER)
    init = OM.initiate(INITIATOR, pub, EPHEMERAL, TIMESTAMP)
    ss = XM.x25519(RESPONDER, init["ephemeral"])
    return pub, init, ss


def _open(hello, peers, **edit):
    pub, init, ss = hello
    f = dict(init, **edit)
    return OM.open_one(RESPONDER, pub, f["ephemeral"], f["encrypted_static"], f["encrypted_timestamp"], edit.get("ss", ss), peers)


def test_constants():
    """The values the issue of this stage states, which the kernel holds as literals."""
    assert OM.INITIAL_CHAIN_KEY.hex().startswith("60e26dae") and OM.INITIAL_CHAIN_KEY.hex().endswith("8b78cd36")
    assert OM.INITIAL_HASH.hex().startswith("2211b361") and OM.INITIAL_HASH.hex().endswith("ba079ef3")


def test_hmac_is_the_standard_one():
    for seed, klen, mlen in [(1, 32, 32), (2, 32, 1), (3, 32, 33), (4, 0, 0), (5, 64, 100), (6, 65, 7), (7, 200, 64)]:
        key, msg = splitmix_bytes(0x4200 + seed, klen), splitmix_bytes(0x4300 + seed, mlen)
        assert OM.hmac(key, msg) == std_hmac.new(key, msg, "blake2s").digest()
        assert OM.hmac(key, msg[:3], msg[3:]) == OM.hmac(key, msg)


def test_derive_key_is_rfc5869():
    def hkdf(salt, ikm, n):  # RFC 5869 2.2 / 2.3 with an empty info
        prk = std_hmac.new(salt, ikm, "blake2s").digest()
        t, out = b"", []
        for i in range(1, n + 1):
            t = std_hmac.new(prk, t + bytes([i]), "blake2s").digest()
            out.append(t)
        return out

    for seed in range(4):
        salt, ikm = splitmix_bytes(0x4400 + seed, 32), splitmix_bytes(0x4500 + seed, 32 if seed else 0)
        want = hkdf(salt, ikm, 3)
        assert [OM.derive_key(salt, ikm, n) for n in (1, 2, 3)] == want
        assert OM.derive_key(salt, ikm) == want[0]


def test_initiator_and_responder_agree(hello):
    pub, init, _ = hello
    ipub = XM.public_key(INITIATOR)
    st, res = _open(hello, [splitmix_bytes(9, 32), ipub])
    assert st == OM.OPEN_OK and res["peer"] == 1 and res["remote_static"] == ipub
    assert res["hash"] == init["hash"] and res["chain_key"] == init["chain_key"]
    # a key that no peer holds: the same hash, the chain key one KDF1 short of the initiator's
    st, new = _open(hello, [])
    assert st == OM.OPEN_NEWPEER and new["peer"] == OM.NOPEER and new["remote_static"] == ipub
    assert new["hash"] == init["hash"] and new["chain_key"] != init["chain_key"]
    assert OM.derive_key(new["chain_key"], XM.x25519(RESPONDER, ipub)) == init["chain_key"]


def test_every_bit_of_ephemeral_and_encrypted_static_is_authenticated(hello):
    """One flipped bit in E (the responder's DH then gives another secret: both the right and the unchanged
    secret are tried) or in any of the 48 bytes of encrypted_static: BADAUTH."""
    pub, init, ss = hello
    for byte in range(32):
        for bit in range(8):
            e = bytearray(init["ephemeral"])
            e[byte] ^= 1 << bit
            assert _open(hello, [], ephemeral=bytes(e))[0] == OM.OPEN_BADAUTH  # (the old secret: the hash alone differs)
    e = bytearray(init["ephemeral"])
    e[5] ^= 0x10
    assert _open(hello, [], ephemeral=bytes(e), ss=XM.x25519(RESPONDER, bytes(e)))[0] == OM.OPEN_BADAUTH
    for byte in range(48):
        for bit in range(8):
            c = bytearray(init["encrypted_static"])
            c[byte] ^= 1 << bit
            assert _open(hello, [], encrypted_static=bytes(c))[0] == OM.OPEN_BADAUTH
    assert _open(hello, [], ss=bytes(32))[0] == OM.OPEN_BADAUTH


def test_the_timestamp_is_only_mixed_into_the_hash(hello):
    pub, init, _ = hello
    peers = [XM.public_key(INITIATOR)]
    for byte in (0, 11, 12, 27):
        t = bytearray(init["encrypted_timestamp"])
        t[byte] ^= 0x80
        st, res = _open(hello, peers, encrypted_timestamp=bytes(t))
        assert st == OM.OPEN_OK and res["hash"] != init["hash"] and res["chain_key"] == init["chain_key"]


def test_low_order_ephemeral_sealed_under_the_zero_secret(hello):
    pub = hello[0]
    low = (1).to_bytes(32, "little")
    assert XM.x25519(RESPONDER, low) == bytes(32)
    init = OM.initiate(INITIATOR, pub, None, TIMESTAMP, ephemeral_public=low, es_secret=bytes(32))
    st, res = OM.open_one(RESPONDER, pub, low, init["encrypted_static"], init["encrypted_timestamp"], bytes(32), [])
    assert st == OM.OPEN_NEWPEER and res["remote_static"] == XM.public_key(INITIATOR) and res["hash"] == init["hash"]


def test_open_batch_states_the_contract(hello):
    pub, init, ss = hello
    ipub = XM.public_key(INITIATOR)
    good = HM.message(1, OM.body(0xA1B2C3D4, init), pub)
    forged = good[:60] + bytes([good[60] ^ 1]) + good[61:]
    rec = np.zeros(6, HM.HS_RECORD)
    for k, (m, ln) in enumerate([(good, 148), (HM.message(2, b"", pub), 92), (forged, 148), (good, 100), (good, 148), (good, 148)]):
        rec[k] = (10 + k, ln, np.frombuffer(m.ljust(148, b"\0"), np.uint8), 0)
    shared = (ss + bytes(32) + ss + ss + ss + ss)
    dh = [XM.X_OK, XM.X_SKIPPED, XM.X_OK, XM.X_BADDESC, XM.X_SKIPPED, XM.X_BADDESC]
    st, inits, sm = OM.open_batch(rec, 6, 6, shared, dh, RESPONDER, [ipub], [9] * 7, b"\x7e" * (144 * 7), [7] * 4)
    assert st == [OM.OPEN_OK, OM.OPEN_SKIPPED, OM.OPEN_BADAUTH, OM.OPEN_BADDESC, OM.OPEN_SKIPPED, OM.OPEN_BADDESC, 9]
    assert sm == [1, 1, 1, 2] and inits[144:] == b"\x7e" * (144 * 6)
    e = np.frombuffer(inits[:144], OM.HS_INIT)[0]
    assert (e["index"], e["record"], e["sender_index"], e["peer"]) == (10, 0, 0xA1B2C3D4, 0)
    assert e["remote_ephemeral"].tobytes() == init["ephemeral"] and e["remote_static"].tobytes() == ipub
    assert e["hash"].tobytes() == init["hash"] and e["chain_key"].tobytes() == init["chain_key"]
    # n_records cuts the batch; an empty table makes the authentic record a NEWPEER
    st, inits, sm = OM.open_batch(rec, 1, 6, shared, dh, RESPONDER, [], [9] * 7, b"\x7e" * (144 * 7), [7] * 4)
    assert st == [OM.OPEN_NEWPEER] + [9] * 6 and sm == [1, 0, 0, 0]
    assert np.frombuffer(inits[:144], OM.HS_INIT)[0]["peer"] == OM.NOPEER
    assert OM.open_batch(rec, None, 0, shared, dh, RESPONDER, [], [9], b"", [7] * 4) == ([9], b"", [7] * 4)


# ---- layouts -----------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    fields = [("wg_hs_init", "WgHsInit", ["index", "record", "sender_index", "peer", "remote_ephemeral", "remote_static",
                                          "hash", "chain_key"]),
              ("wg_hs_open_summary", "WgHsOpenSummary", ["n_emitted", "n_known", "n_badauth", "n_skipped"]),
              ("wg_hs_open_batch", "WgHsOpenBatch", ["records", "n_records", "shared", "dh_status", "open_status", "inits",
                                                     "summary", "n", "_reserved"])]
    consts = ["WG_HS_OPEN_OK", "WG_HS_OPEN_NEWPEER", "WG_HS_OPEN_BADAUTH", "WG_HS_OPEN_SKIPPED", "WG_HS_OPEN_BADDESC",
              "WG_HS_NOPEER"]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += "".join(f'printf("%u\\n", {c});' for c in consts)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\nint main(void){' + body + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    W = wg()
    L = W._lib
    want = []
    for _, p, fs in fields:
        cls = getattr(L, p)
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    want += [getattr(L, c) for c in consts]
    assert got == want
    assert ctypes.sizeof(L.WgHsInit) == 144 and ctypes.sizeof(L.WgHsOpenSummary) == 16
    assert want[-6:] == [OM.OPEN_OK, OM.OPEN_NEWPEER, OM.OPEN_BADAUTH, OM.OPEN_SKIPPED, OM.OPEN_BADDESC, OM.NOPEER]
    assert W.WG_HS_INIT_DTYPE == OM.HS_INIT and W.WG_HS_INIT_DTYPE.itemsize == 144


def test_new_calls_are_bound():
    new = ("wg_hs_peers_set", "wg_hs_open")
    assert set(new) <= {name for name, _, _ in wg()._lib.SIGNATURES}
    lib = wg().lib()
    assert all(hasattr(lib, n) for n in new)
    N = noise()
    assert callable(N.Handshakes.decryptRemoteStatic) and callable(N.Crypto.deriveKey) and callable(N.Crypto.HMAC)
    assert hashlib.blake2s(b"").digest_size == 32
