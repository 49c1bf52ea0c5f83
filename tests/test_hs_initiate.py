"""The initiator's side without a GPU: tests/hs_initiate_model.py's batch restatements against
hs_open_model.initiate and hs_respond_model.consume_response entry by entry; kInitProgram and kFinProgram
(wireguard-java_amd/csrc/wg_hs_chain.h) printed by a host compiler and interpreted through hs_chain_model.run,
with k_hs_init_chain's and k_hs_fin_chain's own operations restated here, against the models; the mirror's TAI64N."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hs_chain_model as CM
import hs_initiate_model as IM
import hs_model as HM
import hs_open_model as OM
import hs_respond_model as RM
import x25519_model as XM
from wgtest import ROOT, noise, oracle, splitmix_bytes, wg

NAMES = ["OP_PAD", "OP_IN32", "OP_OUT", "OP_T1", "OP_TN", "OP_H2", "OP_MAC1KEY", "OP_MAC1A", "OP_IH0", "OP_IES1", "OP_IES2",
         "OP_ITS", "OP_IMAC1B", "OP_IMAC1C", "SRC_ZERO", "SRC_CK", "SRC_X", "SRC_STATIC", "SRC_EPUB", "SRC_EE", "SRC_ES",
         "SRC_ER", "SRC_PSK", "PAD_IPAD", "PAD_OPAD", "PAD_LAST", "PAD_SEAL", "DST_NONE", "DST_H", "DST_X", "DST_CK", "DST_IST",
         "DST_OST", "kInitSteps", "kFinSteps", "kOpenSteps", "kRespSteps"]

INITIATOR = splitmix_bytes(0x6600, 32)
RESPONDERS = [splitmix_bytes(0x6610 + j, 32) for j in range(2)]
EPHEMERALS = [splitmix_bytes(0x6620 + j, 32) for j in range(2)]
RESP_EPH = splitmix_bytes(0x6630, 32)
TIMESTAMP = splitmix_bytes(0x6640, 12)
PSK = splitmix_bytes(0x6650, 32)
LADDER = XM.x25519


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """(E, initiate program, finish program): the header's enums and constants by name, and the two tables."""
    d = tmp_path_factory.mktemp("hs_initiate")
    body = "".join(f'printf("{n} %u\\n", (unsigned)wghc::{n});' for n in NAMES)
    for name, prog in (("init", "kInitProgram"), ("fin", "kFinProgram")):
        body += (f'for (const wghc::Step& s : wghc::{prog}) printf("{name} %u %u %u %u\\n", (unsigned)s.op, (unsigned)s.arg, '
                 "(unsigned)s.imm, (unsigned)s.dst);")
    src = d / "tables.cpp"
    src.write_text('#include <stdio.h>\n#include "wg_hs_chain.h"\nint main(){' + body + " return 0;}\n")
    exe = d / "tables"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "wireguard-java_amd", "csrc"), "-o", str(exe), str(src)])
    E, progs = SimpleNamespace(), {"init": [], "fin": []}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        f = line.split()
        if f[0] in progs:
            progs[f[0]].append(tuple(int(x) for x in f[1:]))
        else:
            setattr(E, f[0], int(f[1]))
    return E, progs["init"], progs["fin"]


@pytest.fixture(scope="module")
def ladder():
    memo = {}

    def x25519(scalar, point):
        key = (bytes(scalar), bytes(point))
        if key not in memo:
            memo[key] = LADDER(*key)
        return memo[key]
    return x25519


def _ck0_states():
    ipad = CM.compress(CM.init(32), CM.words(bytes(b ^ 0x36 for b in CM.CK0) + b"\x36" * 32, 16), 64, False)
    opad = CM.compress(CM.init(32), CM.words(bytes(b ^ 0x5C for b in CM.CK0) + b"\x5c" * 32, 16), 64, False)
    return ipad, opad


def run_init(E, program, local_private, remote_public, ephemeral, timestamp, local_index, x25519):
    """k_hs_init_dh's two ladders and k_hs_init_chain's lane: (the 148-byte message, hash, chain_key)."""
    O = oracle()
    epub = x25519(ephemeral, XM.BASE_POINT)
    spub = x25519(local_private, XM.BASE_POINT)
    c = CM.new_chain()
    c.ist, c.ost = _ck0_states()
    lane = SimpleNamespace(es=bytes(48), ets=bytes(28))
    head = bytes([1, 0, 0, 0]) + int(local_index).to_bytes(4, "little") + epub

    def op_ih0(c, s):
        c.m, c.st, c.t, c.last = CM.words(CM.H0 + bytes(remote_public), 16), CM.init(32), 64, True

    def op_ies1(c, s):
        lane.es = O.py_aead_seal(CM.octets(c.st), CM.ZERO_NONCE, spub, CM.octets(c.hh))
        c.m, c.st, c.t, c.last = list(c.hh) + CM.words(lane.es[:32], 8), CM.init(32), 64, False

    def op_ies2(c, s):
        c.m, c.t, c.last = CM.words(lane.es[32:48], 16), 80, True

    def op_its(c, s):
        lane.ets = O.py_aead_seal(CM.octets(c.st), CM.ZERO_NONCE, bytes(timestamp), CM.octets(c.hh))
        c.m, c.st, c.t, c.last = list(c.hh) + CM.words(lane.ets, 8), CM.init(32), 60, True

    def op_mac1key(c, s):
        c.m, c.st, c.t, c.last = CM.words(b"mac1----" + bytes(remote_public), 16), CM.init(32), 40, True

    def op_mac1a(c, s):
        c.m, c.st, c.t, c.last = list(c.ist) + [0] * 8, CM.init(16, 32), 64, False

    def op_imac1b(c, s):
        c.m, c.t, c.last = CM.words(head + lane.es[:24], 16), 128, False

    def op_imac1c(c, s):
        c.m, c.t, c.last = CM.words(lane.es[24:] + lane.ets, 16), 180, True

    CM.run(E, program, c, {E.SRC_EPUB: epub, E.SRC_ES: x25519(ephemeral, remote_public),
                           E.SRC_STATIC: x25519(local_private, remote_public)},
           {E.OP_IH0: op_ih0, E.OP_IES1: op_ies1, E.OP_IES2: op_ies2, E.OP_ITS: op_its, E.OP_MAC1KEY: op_mac1key,
            E.OP_MAC1A: op_mac1a, E.OP_IMAC1B: op_imac1b, E.OP_IMAC1C: op_imac1c})
    assert len(lane.es) == 48 and len(lane.ets) == 28
    return head + lane.es + lane.ets + CM.octets(c.st)[:16] + bytes(16), CM.octets(c.hh), CM.octets(c.ck)


def run_fin(E, program, local_private, ephemeral, hash_, chain_key, remote_ephemeral, encrypted_empty, psk, x25519):
    """k_hs_fin_dh's two ladders and k_hs_fin_chain's lane: None, or dict(send_key, recv_key)."""
    O = oracle()
    c = CM.new_chain()
    c.hh, c.ck = CM.words(hash_, 8), CM.words(chain_key, 8)
    lane = SimpleNamespace(tag=None)

    def seal(c):
        lane.tag = O.py_aead_seal(CM.octets(c.x), CM.ZERO_NONCE, b"", CM.octets(c.hh))

    CM.run(E, program, c, {E.SRC_ER: remote_ephemeral, E.SRC_EE: x25519(ephemeral, remote_ephemeral),
                           E.SRC_ES: x25519(local_private, remote_ephemeral), E.SRC_PSK: psk}, {"seal": seal})
    if lane.tag != bytes(encrypted_empty):
        return None
    return dict(send_key=CM.octets(c.ck), recv_key=CM.octets(c.x))


def test_tables_have_the_kernels_lengths(tables):
    E, init_prog, fin_prog = tables
    assert (len(init_prog), len(fin_prog)) == (E.kInitSteps, E.kFinSteps) == (35, 47)
    assert (E.kOpenSteps, E.kRespSteps) == (28, 50)  # the earlier programs keep theirs
    assert [bool(s[2] & E.PAD_SEAL) and s[0] == E.OP_PAD for s in fin_prog].count(True) == 1
    assert [s[1] for s in fin_prog].count(E.SRC_PSK) == 1
    assert [s[0] for s in init_prog].count(E.OP_IES1) == 1 and [s[0] for s in init_prog].count(E.OP_ITS) == 1


@pytest.mark.parametrize("j", [0, 1])
def test_init_program_is_initiator_stage_one(tables, ladder, monkeypatch, j):
    E, init_prog, _ = tables
    monkeypatch.setattr(XM, "x25519", ladder)
    remote = XM.public_key(RESPONDERS[j])
    want = IM.initiate_one(INITIATOR, remote, EPHEMERALS[j], TIMESTAMP, 0x0A0B0C0D + j)
    msg, h, ck = run_init(E, init_prog, INITIATOR, remote, EPHEMERALS[j], TIMESTAMP, 0x0A0B0C0D + j, ladder)
    assert msg == want["message"] and h == want["hash"] and ck == want["chain_key"]
    # ... and it is an initiation the responder admits and opens
    assert HM.check_one(msg, 148, [0], [148], 1, 0, HM.mac1_key(remote))[0] == HM.HS_OK
    st, res = OM.open_one(RESPONDERS[j], remote, msg[8:40], msg[40:88], msg[88:116], ladder(RESPONDERS[j], msg[8:40]),
                          [XM.public_key(INITIATOR)])
    assert st == OM.OPEN_OK and res["hash"] == h and res["chain_key"] == ck


@pytest.mark.parametrize("case", ["authentic", "flipped_tag_bit", "psk"])
def test_fin_program_is_consume_message_response(tables, ladder, monkeypatch, case):
    E, _, fin_prog = tables
    monkeypatch.setattr(XM, "x25519", ladder)
    psk = PSK if case == "psk" else bytes(32)
    remote = XM.public_key(RESPONDERS[0])
    one = IM.initiate_one(INITIATOR, remote, EPHEMERALS[0], TIMESTAMP, 77)
    ans = IM.answer(RESPONDERS[0], XM.public_key(INITIATOR), one["message"], RESP_EPH, 88, psk)
    resp = bytearray(ans["response"])
    if case == "flipped_tag_bit":
        resp[59] ^= 0x80
    args = (INITIATOR, EPHEMERALS[0], one["hash"], one["chain_key"], bytes(resp[12:44]), bytes(resp[44:60]), psk)
    want = RM.consume_response(*args)
    got = run_fin(E, fin_prog, *args, ladder)
    if case == "flipped_tag_bit":
        assert want is None and got is None
    else:
        assert got == want and got["send_key"] == ans["recv_key"] and got["recv_key"] == ans["send_key"]
    if case == "psk":  # the psk matters: under the zero psk this response is a forgery
        assert RM.consume_response(*args[:-1]) is None and run_fin(E, fin_prog, *args[:-1], bytes(32), ladder) is None
    if case == "authentic":  # the zero-psk model responder is hs_respond_model's
        st, res = OM.open_one(RESPONDERS[0], remote, one["message"][8:40], one["message"][40:88], one["message"][88:116],
                              ladder(RESPONDERS[0], one["message"][8:40]), [XM.public_key(INITIATOR)])
        ref = RM.respond_one(res["hash"], res["chain_key"], one["message"][8:40], res["remote_static"], RESP_EPH, 88, 77)
        assert ref["response"] == ans["response"] and ref["send_key"] == ans["send_key"] and ref["recv_key"] == ans["recv_key"]


def test_batch_models_agree_with_the_single_models(ladder, monkeypatch):
    monkeypatch.setattr(XM, "x25519", ladder)
    peers = [XM.public_key(k) for k in RESPONDERS]
    psks = [bytes(32), PSK]
    n = 6
    peer = [1, 0, 2, 0, 1, 0]                          # 2: past the table
    eph = b"".join([EPHEMERALS[0], EPHEMERALS[1], EPHEMERALS[0], bytes(32), bytes([7]) + bytes(31), EPHEMERALS[0]])
    ts = b"".join(splitmix_bytes(0x6660 + k, 12) for k in range(n))
    li = [0x100 + k for k in range(n)]
    e2, st, rec, pend, sm = IM.initiate_batch(INITIATOR, peers, peer, eph + b"\xee" * 32, ts, li, n, [9] * (n + 1),
                                              b"\x7e" * (160 * (n + 1)), b"\x7e" * (112 * (n + 1)), [9] * 4)
    assert st == [0, 0, IM.INIT_BADPEER, IM.INIT_NOEPH, 0, 0, 9] and sm == [4, 1, 1, 0]
    assert rec[160 * n:] == b"\x7e" * 160 and pend[112 * n:] == b"\x7e" * 112 and e2[32 * n:] == b"\xee" * 32
    R = np.frombuffer(rec[:160 * n], HM.HS_RECORD)
    P = np.frombuffer(pend[:112 * n], IM.HS_PENDING)
    for k in range(n):
        if st[k] != IM.INIT_OK:
            assert rec[160 * k:160 * k + 160] == bytes(160) and pend[112 * k:112 * k + 112] == bytes(112)
            assert e2[32 * k:32 * k + 32] == eph[32 * k:32 * k + 32]
            continue
        init = OM.initiate(INITIATOR, peers[peer[k]], eph[32 * k:32 * k + 32], ts[12 * k:12 * k + 12])
        msg = R[k]["msg"].tobytes()
        assert (int(R[k]["index"]), int(R[k]["len"]), int(R[k]["_pad"])) == (k, 148, 0)
        assert msg[:8] == bytes([1, 0, 0, 0]) + li[k].to_bytes(4, "little")
        assert (msg[8:40], msg[40:88], msg[88:116]) == (init["ephemeral"], init["encrypted_static"], init["encrypted_timestamp"])
        assert msg[116:132] == HM.mac1(msg[:116], peers[peer[k]]) and msg[132:] == bytes(16)
        assert (int(P[k]["state"]), int(P[k]["peer"]), int(P[k]["local_index"]), int(P[k]["_zero"])) == (1, peer[k], li[k], 0)
        assert P[k]["ephemeral"].tobytes() == eph[32 * k:32 * k + 32] and P[k]["hash"].tobytes() == init["hash"]
        assert P[k]["chain_key"].tobytes() == init["chain_key"] and e2[32 * k:32 * k + 32] == bytes(32)
    # responses to entries 1 (peer 0), 4 (peer 1, its psk) and 5; a forgery against 0; an unknown index; an initiation
    me = XM.public_key(INITIATOR)
    resp = {k: IM.answer(RESPONDERS[peer[k]], me, R[k]["msg"].tobytes(), RESP_EPH, 0x900 + k, psks[peer[k]]) for k in (0, 1, 4, 5)}
    forged = bytearray(resp[0]["response"])
    forged[44] ^= 1
    unknown = bytearray(resp[5]["response"])
    unknown[8:12] = (0x7777).to_bytes(4, "little")
    msgs = [resp[4]["response"], bytes(forged), R[1]["msg"].tobytes(), resp[1]["response"], bytes(unknown), resp[5]["response"],
            resp[1]["response"]]
    recs = np.zeros(len(msgs), HM.HS_RECORD)
    for j, m in enumerate(msgs):
        recs[j]["index"], recs[j]["len"] = 10 + j, len(m)
        recs[j]["msg"][:len(m)] = np.frombuffer(m, np.uint8)
    m = len(msgs)
    p2, fs, est, fsum = IM.finish_batch(INITIATOR, len(peers), psks, recs, m - 1, m, pend, n, [9] * m, b"\x7e" * (96 * m), [9] * 4)
    assert fs == [IM.FIN_OK, IM.FIN_BADAUTH, IM.FIN_SKIPPED, IM.FIN_OK, IM.FIN_NOPENDING, IM.FIN_OK, 9] and fsum == [3, 1, 1, 1]
    S = np.frombuffer(est[:96 * 3], IM.HS_ESTABLISHED)
    assert est[96 * 3:] == b"\x7e" * (96 * (m - 3))
    for s, (j, k) in zip(S, [(0, 4), (3, 1), (5, 5)]):
        keys = RM.consume_response(INITIATOR, eph[32 * k:32 * k + 32], P[k]["hash"].tobytes(), P[k]["chain_key"].tobytes(),
                                   msgs[j][12:44], msgs[j][44:60], psks[peer[k]])
        assert (int(s["index"]), int(s["record"]), int(s["pending"]), int(s["peer"])) == (10 + j, j, k, peer[k])
        assert (int(s["local_index"]), int(s["remote_index"])) == (li[k], 0x900 + k) and not s["_zero"].any()
        assert s["send_key"].tobytes() == keys["send_key"] == resp[k]["recv_key"]
        assert s["recv_key"].tobytes() == keys["recv_key"] == resp[k]["send_key"]
    for k in range(n):  # the OK ones are consumed, the forgery's target is as it was
        assert p2[112 * k:112 * k + 112] == (bytes(112) if k in (1, 4, 5) else pend[112 * k:112 * k + 112])
    assert p2[112 * n:] == pend[112 * n:]
    # a second call over the same records: nothing is pending for them any more
    _, fs2, _, fsum2 = IM.finish_batch(INITIATOR, len(peers), psks, recs, None, m, p2, n, [9] * m, b"\x7e" * (96 * m), [9] * 4)
    assert fs2 == [IM.FIN_NOPENDING, IM.FIN_BADAUTH, IM.FIN_SKIPPED, IM.FIN_NOPENDING, IM.FIN_NOPENDING, IM.FIN_NOPENDING,
                   IM.FIN_NOPENDING] and fsum2 == [0, 5, 1, 1]


def test_tai64n_layout():
    """Crypto.java:19-27: four zero bytes, then the long millis * 1000 + 2^62 + 10 big-endian."""
    T = noise().Crypto.TAI64N
    assert T(0) == bytes(4) + bytes.fromhex("400000000000000a")
    assert T(1_700_000_000_123) == bytes(4) + (1_700_000_000_123_000 + (1 << 62) + 10).to_bytes(8, "big")
    now = T()
    assert len(now) == 12 and now[:4] == bytes(4) and now[4] == 0x40
    assert T(1) > T(0)  # later is larger, as a responder's replay check needs


def test_header_layouts_and_bindings(tmp_path):
    """include/wgaead.h's new structs and constants as a C compiler lays them out, against _lib.py, engine.py's dtypes
    and the model's."""
    fields = [("wg_hs_pending", "WgHsPending", ["state", "peer", "local_index", "_zero", "ephemeral", "hash", "chain_key"]),
              ("wg_hs_established", "WgHsEstablished", ["index", "record", "pending", "peer", "local_index", "remote_index", "_zero",
                                                        "send_key", "recv_key"]),
              ("wg_hs_initiate_batch", "WgHsInitiateBatch", ["peer", "ephemerals", "timestamps", "local_index", "status", "records",
                                                             "pending", "summary", "n", "_reserved"]),
              ("wg_hs_finish_batch", "WgHsFinishBatch", ["records", "n_records", "pending", "fin_status", "established", "summary",
                                                         "n", "n_pending"])]
    consts = ["WG_HS_INIT_OK", "WG_HS_INIT_BADPEER", "WG_HS_INIT_NOEPH", "WG_HS_FIN_OK", "WG_HS_FIN_NOPENDING", "WG_HS_FIN_BADAUTH",
              "WG_HS_FIN_SKIPPED", "WG_HS_FIN_BADDESC"]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += "".join(f'printf("%u\\n", {c});' for c in consts)
    body += 'printf("%zu\\n", sizeof(wg_hs_initiate_summary)); printf("%zu\\n", sizeof(wg_hs_finish_summary));'
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
    want += [getattr(L, c) for c in consts] + [16, 16]
    assert got == want
    assert ctypes.sizeof(L.WgHsPending) == 112 and ctypes.sizeof(L.WgHsEstablished) == 96
    assert want[-10:-2] == [IM.INIT_OK, IM.INIT_BADPEER, IM.INIT_NOEPH, IM.FIN_OK, IM.FIN_NOPENDING, IM.FIN_BADAUTH, IM.FIN_SKIPPED,
                            IM.FIN_BADDESC]
    assert W.WG_HS_PENDING_DTYPE == IM.HS_PENDING and W.WG_HS_ESTABLISHED_DTYPE == IM.HS_ESTABLISHED
    names = {name for name, _, _ in L.SIGNATURES}
    N = noise()
    for f in ("wg_hs_psks_set", "wg_hs_initiate", "wg_hs_finish"):
        assert f in names and hasattr(W.lib(), f)
    for m in ("hs_psks_set", "hs_initiate", "hs_finish", "hs_initiate_host", "hs_finish_host"):
        assert callable(getattr(W.Engine, m))
    for m in ("getLocalEphemeral", "getEncryptedStatic", "getEncryptedTimestamp", "initiation", "consumeMessageResponse"):
        assert callable(getattr(N.InitiatorStageOne, m))
    assert callable(N.Handshakes.initiateHandshake) and N.NoisePresharedKey.zero().data() == bytes(32)
    with pytest.raises(ValueError):
        N.NoisePresharedKey(bytes(31))
