"""The CPU model of wg_hs_respond (tests/hs_respond_model.py) against the initiator's side of the handshake, the
standard library and itself, and the binding's layouts against include/wgaead.h. No GPU."""
import ctypes
import hmac as std_hmac
import os
import subprocess

import numpy as np
import pytest

import hs_model as HM
import hs_open_model as OM
import hs_respond_model as RM
import x25519_model as XM
from wgtest import ROOT, noise, oracle, splitmix_bytes, wg

RESPONDER = splitmix_bytes(0x6100, 32)
INITIATORS = [splitmix_bytes(0x6110 + j, 32) for j in range(2)]
EPHEMERALS = [splitmix_bytes(0x6120 + j, 32) for j in range(2)]     # the initiators'
RESP_EPH = [splitmix_bytes(0x6130 + j, 32) for j in range(2)]        # the responder's
TIMESTAMP = splitmix_bytes(0x6140, 12)


def _handshake(i, e, local_index=0x01020304, sender_index=0xA1B2C3D4):
    """Initiator i's initiation with ephemeral e, opened by the responder (initiator 0 is a peer), and answered
    with responder ephemeral e. Returns (init, opened entry fields, response dict)."""
    pub = XM.public_key(RESPONDER)
    init = OM.initiate(INITIATORS[i], pub, EPHEMERALS[e], TIMESTAMP)
    ss = XM.x25519(RESPONDER, init["ephemeral"])
    st, res = OM.open_one(RESPONDER, pub, init["ephemeral"], init["encrypted_static"], init["encrypted_timestamp"], ss,
                          [XM.public_key(INITIATORS[0])])
    assert st == (OM.OPEN_OK if i == 0 else OM.OPEN_NEWPEER)
    if st == OM.OPEN_NEWPEER:  # the host finishes the chain key (Handshakes.java:232-233)
        res = dict(res, chain_key=OM.derive_key(res["chain_key"], XM.x25519(RESPONDER, res["remote_static"])))
    r = RM.respond_one(res["hash"], res["chain_key"], init["ephemeral"], res["remote_static"], RESP_EPH[e], local_index,
                       sender_index)
    return init, res, r


@pytest.fixture(scope="module")
def shakes():
    return {(i, e): _handshake(i, e) for i in range(2) for e in range(2)}


def _consume(i, e, init, response):
    return RM.consume_response(INITIATORS[i], EPHEMERALS[e], init["hash"], init["chain_key"], response[12:44], response[44:60])


def test_initiator_and_responder_agree(shakes):
    O = oracle()
    for (i, e), (init, res, r) in shakes.items():
        assert res["chain_key"] == init["chain_key"] and res["hash"] == init["hash"]
        resp = r["response"]
        assert resp[:4] == bytes([2, 0, 0, 0]) and resp[4:8] == bytes([4, 3, 2, 1]) and resp[8:12] == bytes.fromhex("d4c3b2a1")
        assert resp[12:44] == r["ephemeral_public"] == XM.public_key(RESP_EPH[e]) and resp[44:60] == r["encrypted_empty"]
        assert resp[76:] == bytes(16) and len(resp) == 92
        keys = _consume(i, e, init, resp)
        assert keys is not None
        assert keys["recv_key"] == r["send_key"] and keys["send_key"] == r["recv_key"] and r["send_key"] != r["recv_key"]
        # a transport packet each way
        nonce = O.transport_nonce(0)
        assert O.py_aead_open(keys["recv_key"], nonce, O.py_aead_seal(r["send_key"], nonce, b"ping")) == b"ping"
        assert O.py_aead_open(r["recv_key"], nonce, O.py_aead_seal(keys["send_key"], nonce, b"pong")) == b"pong"
    assert len({r["send_key"] for _, _, r in shakes.values()}) == 4


def test_empty_message_kdf_is_rfc5869():
    """derive_key(ck, b"", n): the extract's message is empty, so the inner hash is the key block alone."""
    for seed in range(3):
        ck = splitmix_bytes(0x6200 + seed, 32)
        prk = std_hmac.new(ck, b"", "blake2s").digest()
        t1 = std_hmac.new(prk, b"\x01", "blake2s").digest()
        t2 = std_hmac.new(prk, t1 + b"\x02", "blake2s").digest()
        t3 = std_hmac.new(prk, t2 + b"\x03", "blake2s").digest()
        assert [OM.derive_key(ck, b"", n) for n in (1, 2, 3)] == [t1, t2, t3]
        assert OM.hmac(ck) == prk


def test_every_byte_of_epub_and_encrypted_empty_is_authenticated(shakes):
    """One flipped bit in each of the 32 bytes of Epub and the 16 bytes of encrypted_empty (the bit walks with the
    byte): the initiator rejects."""
    init, _, r = shakes[(0, 0)]
    resp = r["response"]
    assert _consume(0, 0, init, resp) is not None
    for byte in range(12, 60):
        bad = bytearray(resp)
        bad[byte] ^= 1 << (byte % 8)
        assert _consume(0, 0, init, bytes(bad)) is None, byte
    # another initiator's state does not take it either
    other = shakes[(1, 0)][0]
    assert _consume(1, 0, other, resp) is None


def test_mac1_is_under_the_initiators_key(shakes):
    for (i, e), (init, res, r) in shakes.items():
        ipub = XM.public_key(INITIATORS[i])
        wire = r["response"]
        st, msg = HM.check_one(wire, len(wire), [0], [92], 1, 0, HM.mac1_key(ipub))
        assert st == HM.HS_OK and msg == wire and msg[0] == 2
        assert HM.check_one(wire, len(wire), [0], [92], 1, 0, HM.mac1_key(XM.public_key(RESPONDER)))[0] == HM.HS_BADMAC1


def _entries(shakes, peers):
    """HS_INIT entries of the four handshakes; peers[k]: entry k's peer field."""
    ent = np.zeros(4, OM.HS_INIT)
    for k, ((i, e), (init, res, _)) in enumerate(shakes.items()):
        ent[k]["index"], ent[k]["record"], ent[k]["sender_index"], ent[k]["peer"] = 50 + k, k, 0x70000000 + k, peers[k]
        ent[k]["remote_ephemeral"] = np.frombuffer(init["ephemeral"], np.uint8)
        for f in ("remote_static", "hash", "chain_key"):
            ent[k][f] = np.frombuffer(res[f], np.uint8)
    return ent


def test_respond_batch_states_the_contract(shakes):
    ent = _entries(shakes, [0, RM.NOPEER, 0, RM.NOPEER])
    late = bytes([7]) + bytes(31)  # the all-zero scalar only after clamping: not NOEPH
    assert XM.clamp(late) == XM.clamp(bytes(32)) and late != bytes(32)
    eph = RESP_EPH[0] + RESP_EPH[1] + bytes(32) + bytes(32)
    li = [0x100, 0x101, 0x102, 0x103]
    guard = (b"\x7e" * (176 * 5), [9] * 5, [7] * 4)
    # SKIP_NEWPEER: NOPEER comes before NOEPH (entry 3 has both), entry 2 is NOEPH
    e2, st, out, sm = RM.respond_batch(ent, 4, 4, eph, li, RM.SKIP_NEWPEER, guard[1], guard[0], guard[2])
    assert st == [RM.RESP_OK, RM.RESP_NOPEER, RM.RESP_NOEPH, RM.RESP_NOPEER, 9] and sm == [1, 2, 1, 0]
    assert e2 == bytes(32) + RESP_EPH[1] + bytes(64)  # consumed: zeroed; a non-OK entry's: untouched
    assert out[176:] == b"\x7e" * (176 * 4)
    s = np.frombuffer(out[:176], RM.HS_SESSION)[0]
    want = RM.respond_one(ent[0]["hash"].tobytes(), ent[0]["chain_key"].tobytes(), ent[0]["remote_ephemeral"].tobytes(),
                          ent[0]["remote_static"].tobytes(), RESP_EPH[0], 0x100, 0x70000000)
    assert (s["index"], s["init"], s["peer"], s["local_index"], s["remote_index"]) == (50, 0, 0, 0x100, 0x70000000)
    assert s["response"].tobytes() == want["response"] and s["send_key"].tobytes() == want["send_key"]
    assert s["recv_key"].tobytes() == want["recv_key"]
    # without the flag the peer is only copied through; the clamped-to-zero ephemeral is answered
    eph = RESP_EPH[0] + RESP_EPH[1] + late + bytes(32)
    e2, st, out, sm = RM.respond_batch(ent, None, 4, eph, li, 0, guard[1], guard[0], guard[2])
    assert st == [RM.RESP_OK, RM.RESP_OK, RM.RESP_OK, RM.RESP_NOEPH, 9] and sm == [3, 0, 1, 0] and e2 == bytes(128)
    ss = np.frombuffer(out[:176 * 3], RM.HS_SESSION)
    assert ss["init"].tolist() == [0, 1, 2] and ss["peer"].tolist() == [0, RM.NOPEER, 0] and out[176 * 3:] == b"\x7e" * (176 * 2)
    assert ss[2]["response"][12:44].tobytes() == XM.public_key(late) == XM.public_key(bytes(32))
    one = RM.respond_batch(ent[:1], None, 1, bytes([8]) + bytes(31), li, RM.SKIP_NEWPEER, [9], b"\x7e" * 176, [7] * 4)
    assert one[1] == [RM.RESP_OK] and one[3] == [1, 0, 0, 0] and one[0] == bytes(32)  # 08 00 .. 00 is a key like any other
    # n_inits cuts the batch, and above n it is n; n = 0 touches nothing
    e2, st, out, sm = RM.respond_batch(ent, 1, 4, eph, li, 0, guard[1], guard[0], guard[2])
    assert st == [RM.RESP_OK, 9, 9, 9, 9] and sm == [1, 0, 0, 0] and e2 == bytes(32) + eph[32:] and out[176:] == b"\x7e" * (176 * 4)
    assert RM.respond_batch(ent, 9, 4, eph, li, 0, guard[1], guard[0], guard[2])[3] == [3, 0, 1, 0]
    assert RM.respond_batch(ent, None, 0, eph, li, 0, [9], b"", [7] * 4) == (eph, [9], b"", [7] * 4)


# ---- layouts -----------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    fields = [("wg_hs_session", "WgHsSession", ["index", "init", "peer", "local_index", "response", "remote_index", "send_key",
                                                "recv_key"]),
              ("wg_hs_respond_summary", "WgHsRespondSummary", ["n_ok", "n_nopeer", "n_noeph", "_zero"]),
              ("wg_hs_respond_batch", "WgHsRespondBatch", ["inits", "n_inits", "ephemerals", "local_index", "resp_status",
                                                           "sessions", "summary", "n", "flags"])]
    consts = ["WG_HS_RESP_OK", "WG_HS_RESP_NOPEER", "WG_HS_RESP_NOEPH", "WG_HS_RESP_SKIP_NEWPEER"]
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
    assert ctypes.sizeof(L.WgHsSession) == 176 and ctypes.sizeof(L.WgHsRespondSummary) == 16
    assert want[-4:] == [RM.RESP_OK, RM.RESP_NOPEER, RM.RESP_NOEPH, RM.SKIP_NEWPEER]
    assert W.WG_HS_SESSION_DTYPE == RM.HS_SESSION and W.WG_HS_SESSION_DTYPE.itemsize == 176
    assert [W.WG_HS_SESSION_DTYPE.fields[f][1] for f in fields[0][2]] == [getattr(L.WgHsSession, f).offset for f in fields[0][2]]


def test_new_calls_are_bound():
    assert "wg_hs_respond" in {name for name, _, _ in wg()._lib.SIGNATURES}
    assert hasattr(wg().lib(), "wg_hs_respond")
    N = noise()
    assert callable(N.Handshakes.responderHandshake) and callable(wg().Engine.hs_respond) and callable(wg().Engine.hs_respond_host)
    for m in ("getKeypair", "getRemotePublicKey", "getEncryptedEmpty", "getLocalEphemeral"):
        assert callable(getattr(N.ResponderHandshake, m))
