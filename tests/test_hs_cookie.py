"""tests/hs_cookie_model.py pinned to the published vectors of draft-irtf-cfrg-xchacha-03, a model round trip of a
cookie reply, and the declarations of the new calls. No GPU, except the noise mirror's test: the mirror computes on
the device and carries the gpu mark itself."""
import ctypes
import os
import re

import numpy as np
import pytest

import hs_cookie_model as CM
import hs_model as HM
from wgtest import ROOT, noise, wg

PLAIN = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would "
         b"be it.")


def test_hchacha20_vector():
    """draft-irtf-cfrg-xchacha-03 2.2.1"""
    out = CM.hchacha20(bytes(range(32)), bytes.fromhex("000000090000004a0000000031415927"))
    assert out.hex() == "82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"


def test_xchacha20_poly1305_vector():
    """draft-irtf-cfrg-xchacha-03 A.3.1"""
    key, nonce = bytes(range(0x80, 0xA0)), bytes(range(0x40, 0x58))
    aad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    assert len(PLAIN) == 114
    sealed = CM.xaead_seal(key, nonce, PLAIN, aad)
    assert sealed[:16].hex() == "bd6d179d3e83d43b9576579493c0e939"
    assert sealed[-16:].hex() == "c0875924c1c7987947deafd8780acf49"
    assert CM.xaead_open(key, nonce, sealed, aad) == PLAIN
    assert CM.xaead_open(key, nonce, sealed[:-1] + bytes([sealed[-1] ^ 1]), aad) is None
    assert CM.xaead_open(key, nonce, sealed, aad[:-1] + b"\0") is None


def _src(addr: bytes, port: int, family: int):
    s = np.zeros(1, CM.HS_SRC)
    s["addr"][0, :len(addr)] = np.frombuffer(addr, np.uint8)
    s["port"][0] = [port >> 8, port & 0xFF]
    s["family"] = family
    return s


def test_cookie_takes_the_address_bytes_of_its_family():
    secret = bytes(range(32))
    v4 = _src(bytes([10, 0, 0, 7]) + b"\xAA" * 12, 51820, 4)[0]  # (bytes behind an IPv4 address are not hashed)
    assert CM.cookie_of_src(secret, v4) == HM.blake2s(bytes([10, 0, 0, 7, 0xCA, 0x6C]), secret, 16)
    v6 = _src(bytes(range(16)), 1, 6)[0]
    assert CM.cookie_of_src(secret, v6) == HM.blake2s(bytes(range(16)) + b"\0\1", secret, 16)


def test_model_round_trip_a_reply_opens_only_against_its_own_mac1():
    """admit's reply opens under cookie_open's rule with the mac1 of the message it answers and fails with another
    message's; the cookie it carries makes a mac2 that admit then accepts."""
    rng = np.random.default_rng(3100)
    b_pub, secret = rng.bytes(32), rng.bytes(32)
    m0 = HM.message(1, bytes(3) + (0x11223344).to_bytes(4, "little") + rng.bytes(108), b_pub)
    m1 = HM.message(1, bytes(3) + (0x55667788).to_bytes(4, "little") + rng.bytes(108), b_pub)
    ring = np.frombuffer(m0 + m1, np.uint8)
    off, lens = np.array([0, 148], np.uint64), np.array([148, 148], np.uint32)
    src = np.concatenate([_src(bytes([192, 0, 2, 1]), 7000, 4), _src(bytes(range(16)), 7001, 6)])
    nonces = rng.bytes(48)
    st, rec, s, reps, a, after = CM.admit(ring, off, lens, src, nonces, b_pub, secret)
    assert st == [CM.HS_NEEDCOOKIE] * 2 and len(rec) == 0 and s["n_rejected"] == 2
    assert a == dict(n_replies=2, n_mac2_ok=0, n_nononce=0, n_badsrc=0) and after == bytes(48)
    assert reps["index"].tolist() == [0, 1] and reps["len"].tolist() == [64, 64]
    # the initiator's side: one pending entry per message, both to peer 0 = B
    sent = np.zeros(2, HM.HS_RECORD)
    pend = np.zeros(2, CM.HS_PENDING)
    for k, m in enumerate((m0, m1)):
        sent[k]["len"] = 148
        sent[k]["msg"] = np.frombuffer(m, np.uint8)
        pend[k]["state"], pend[k]["local_index"] = 1, int.from_bytes(m[4:8], "little")
    wire = reps["msg"].tobytes()
    r_off, r_len = np.array([0, 64], np.uint64), np.array([64, 64], np.uint32)
    table = [(bytes(16), False)]
    cst, learned, cs, table2 = CM.cookie_open(wire, r_off, r_len, sent, pend, [b_pub], table)
    assert cst == [CM.CK_OK, CM.CK_OK] and cs["n_ok"] == 2
    assert table2[0] == (CM.cookie_of_src(secret, src[0]), True)  # the lowest batch index
    swapped = sent[::-1].copy()  # each reply against the other message's mac1
    cst, _, _, table3 = CM.cookie_open(wire, r_off, r_len, swapped, pend, [b_pub], table)
    assert cst == [CM.CK_BADAUTH, CM.CK_BADAUTH] and table3 == table
    # the retransmission with mac2 passes from the address the cookie was made for, and from no other
    again, mst, ms = CM.mac2_batch(sent[:1], [0], table2)
    assert mst == [CM.MAC2_OK] and again[0]["msg"].tobytes()[:132] == m0[:132]
    ring2 = np.frombuffer(again[0]["msg"].tobytes(), np.uint8)
    st, rec, s, reps, a, _ = CM.admit(ring2, off[:1], lens[:1], src[:1], bytes(24), b_pub, secret)
    assert st == [CM.HS_OK] and rec[0]["msg"].tobytes() == ring2.tobytes() and a["n_mac2_ok"] == 1
    st, _, _, _, a, _ = CM.admit(ring2, off[:1], lens[:1], src[1:], bytes(24), b_pub, secret)
    assert st == [CM.HS_NONONCE] and a["n_nononce"] == 1


@pytest.mark.gpu
def test_noise_mirror_equals_the_model():
    N = noise()
    rng = np.random.default_rng(3200)
    assert N.HChaCha20(bytes(range(32)), bytes.fromhex("000000090000004a0000000031415927")).hex() == \
        "82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"
    for ln, al in [(0, 0), (16, 16), (114, 12), (65, 33)]:
        key, nonce, pt, aad = rng.bytes(32), rng.bytes(24), rng.bytes(ln), rng.bytes(al)
        assert N.HChaCha20(key, nonce[:16]) == CM.hchacha20(key, nonce[:16])
        sealed = N.XChaCha20Poly1305.seal(key, nonce, pt, aad)
        assert sealed == CM.xaead_seal(key, nonce, pt, aad)
        assert N.XChaCha20Poly1305.open(key, nonce, sealed, aad) == pt
        with pytest.raises(N.AEADBadTagException):
            N.XChaCha20Poly1305.open(key, nonce, sealed[:-1] + bytes([sealed[-1] ^ 0x80]), aad)
    secret, head = rng.bytes(32), bytes([1]) + rng.bytes(131)
    assert N.calculate_cookie(secret, bytes([10, 1, 2, 3]), 51820) == CM.cookie(secret, bytes([10, 1, 2, 3]), b"\xCA\x6C")
    assert N.calculate_cookie(secret, bytes(range(16)), 258) == CM.cookie(secret, bytes(range(16)), b"\x01\x02")
    ck = rng.bytes(16)
    assert N.calculate_mac2(head, ck) == CM.mac2(ck, head)


def test_header_and_binding_declare_the_new_calls():
    L = wg()._lib
    src = open(os.path.join(ROOT, "include/wgaead.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    bound = {name for name, _, _ in L.SIGNATURES}
    for fn in ("wg_hs_cookie_secret_set", "wg_hs_admit", "wg_hs_cookie_open", "wg_hs_cookies_get", "wg_hs_cookies_set",
               "wg_hs_mac2"):
        assert re.search(r"^int " + fn + r"\(", code, re.M), fn
        assert fn in bound and hasattr(wg().lib(), fn), fn
    for name in ("WG_HS_BADSRC", "WG_HS_NONONCE", "WG_HS_NEEDCOOKIE", "WG_HS_COOKIE_SIZE", "WG_HS_CK_OK", "WG_HS_CK_NOPENDING",
                 "WG_HS_CK_BADAUTH", "WG_HS_CK_SKIPPED", "WG_HS_CK_BADLEN", "WG_HS_MAC2_OK", "WG_HS_MAC2_NONE",
                 "WG_HS_MAC2_BADDESC", "WG_HS_MAC2_BADPEER"):
        assert f"#define {name} {getattr(L, name)}u" in src, name
    assert getattr(L, "WG_HS_BADMAC2") == 4 and CM.HS_NEEDCOOKIE == L.WG_HS_NEEDCOOKIE and CM.CK_BADLEN == L.WG_HS_CK_BADLEN
    W = wg()
    assert W.WG_HS_SRC_DTYPE == CM.HS_SRC and W.WG_HS_COOKIE_REPLY_DTYPE == CM.HS_COOKIE_REPLY
    assert W.WG_HS_LEARNED_DTYPE == CM.HS_LEARNED
    assert (ctypes.sizeof(L.WgHsSrc), ctypes.sizeof(L.WgHsCookieReply), ctypes.sizeof(L.WgHsLearned)) == (24, 80, 16)
    assert L.WgHsSrc.port.offset == 16 and L.WgHsSrc.family.offset == 18 and L.WgHsCookieReply.msg.offset == 8
    assert L.WgHsAdmitBatch.src.offset == ctypes.sizeof(L.WgHsBatch) == 80
