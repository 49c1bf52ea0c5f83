"""The step programs of k_hs_open and k_hs_resp_chain (wireguard-java_amd/csrc/wg_hs_chain.h) as data: a host
compiler prints both tables, tests/hs_chain_model.py interprets them, and the results must equal
hs_open_model.open_one and hs_respond_model.respond_one. No GPU."""
import os
import subprocess
from types import SimpleNamespace

import pytest

import hs_chain_model as CM
import hs_open_model as OM
import hs_respond_model as RM
import x25519_model as XM
from wgtest import ROOT, splitmix_bytes

NAMES = ["OP_PAD", "OP_IN32", "OP_OUT", "OP_T1", "OP_TN", "OP_H2", "OP_H0", "OP_ES1", "OP_ES2", "OP_TS", "OP_MAC1KEY", "OP_MAC1A",
         "OP_MAC1B", "SRC_ZERO", "SRC_CK", "SRC_X", "SRC_E", "SRC_SS", "SRC_STATIC", "SRC_EPUB", "SRC_EE", "SRC_ES", "PAD_IPAD",
         "PAD_OPAD", "PAD_LAST", "PAD_SEAL", "DST_NONE", "DST_H", "DST_X", "DST_CK", "DST_IST", "DST_OST", "DST_CK_IF_PEER",
         "kOpenSteps", "kRespSteps", "kOpenStaticBegin", "kOpenStaticEnd"]

RESPONDER = splitmix_bytes(0x6500, 32)
INITIATORS = [splitmix_bytes(0x6510 + j, 32) for j in range(2)]  # initiator 0 is a peer, initiator 1 is not
EPHEMERALS = [splitmix_bytes(0x6520 + j, 32) for j in range(2)]
RESP_EPH = [splitmix_bytes(0x6530 + j, 32) for j in range(2)]
TIMESTAMP = splitmix_bytes(0x6540, 12)
LADDER = XM.x25519  # (the tests put a memo in its place)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """(E, open program, respond program): the header's enums and constants by name, and its two tables."""
    d = tmp_path_factory.mktemp("hs_chain")
    body = "".join(f'printf("{n} %u\\n", (unsigned)wghc::{n});' for n in NAMES)
    for name, prog in (("open", "kOpenProgram"), ("resp", "kRespProgram")):
        body += (f'for (const wghc::Step& s : wghc::{prog}) printf("{name} %u %u %u %u\\n", (unsigned)s.op, (unsigned)s.arg, '
                 "(unsigned)s.imm, (unsigned)s.dst);")
    src = d / "tables.cpp"
    src.write_text('#include <stdio.h>\n#include "wg_hs_chain.h"\nint main(){' + body + " return 0;}\n")
    exe = d / "tables"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "wireguard-java_amd", "csrc"), "-o", str(exe), str(src)])
    E, progs = SimpleNamespace(), {"open": [], "resp": []}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        f = line.split()
        if f[0] in progs:
            progs[f[0]].append(tuple(int(x) for x in f[1:]))
        else:
            setattr(E, f[0], int(f[1]))
    return E, progs["open"], progs["resp"]


@pytest.fixture(scope="module")
def ladder():
    """x25519_model's ladder, each result computed once for the model and the interpreter."""
    memo = {}

    def x25519(scalar, point):
        key = (bytes(scalar), bytes(point))
        if key not in memo:
            memo[key] = LADDER(*key)
        return memo[key]
    return x25519


def test_tables_have_the_kernels_lengths(tables):
    E, open_prog, resp_prog = tables
    assert (len(open_prog), len(resp_prog)) == (E.kOpenSteps, E.kRespSteps) == (28, 50)
    # the static-static KDF: an extract and an expand between H(h || encrypted_static) and H(h || encrypted_timestamp)
    assert E.kOpenStaticEnd - E.kOpenStaticBegin == 8
    assert open_prog[E.kOpenStaticBegin - 1][0] == E.OP_ES2 and open_prog[E.kOpenStaticEnd][0] == E.OP_TS
    assert [s[3] for s in open_prog].count(E.DST_CK_IF_PEER) == 1 and open_prog[E.kOpenStaticEnd - 1][3] == E.DST_CK_IF_PEER
    assert [bool(s[2] & E.PAD_SEAL) and s[0] == E.OP_PAD for s in resp_prog].count(True) == 1


def _initiation(i, e, monkey_ladder):
    pub = XM.public_key(RESPONDER)
    init = OM.initiate(INITIATORS[i], pub, EPHEMERALS[e], TIMESTAMP)
    return pub, init, monkey_ladder(RESPONDER, init["ephemeral"])


@pytest.mark.parametrize("case", ["known", "unknown", "unknown_in_a_wave_with_a_known_peer", "flipped_tag_bit"])
def test_open_program_is_decrypt_remote_static(tables, ladder, monkeypatch, case):
    E, open_prog, _ = tables
    monkeypatch.setattr(XM, "x25519", ladder)  # (hs_open_model calls the ladder through the module)
    i = 0 if case == "known" else 1
    pub, init, ss = _initiation(i, 0, ladder)
    es = bytearray(init["encrypted_static"])
    if case == "flipped_tag_bit":
        es[40] ^= 0x10
    peers = [splitmix_bytes(0x6550, 32), XM.public_key(INITIATORS[0])]
    want = OM.open_one(RESPONDER, pub, init["ephemeral"], bytes(es), init["encrypted_timestamp"], ss, peers)
    got = CM.open_one(E, open_prog, (E.kOpenStaticBegin, E.kOpenStaticEnd), RESPONDER, pub, init["ephemeral"], bytes(es),
                      init["encrypted_timestamp"], ss, peers, ladder,
                      wave_known=True if case == "unknown_in_a_wave_with_a_known_peer" else None)
    assert want[0] == {"known": OM.OPEN_OK, "flipped_tag_bit": OM.OPEN_BADAUTH}.get(case, OM.OPEN_NEWPEER)
    assert got[0] == want[0]
    if want[1] is None:
        assert got[1] is None
    else:
        for f in ("remote_static", "hash", "chain_key", "peer"):
            assert got[1][f] == want[1][f], f
        assert (want[1]["peer"] == 1) == (case == "known")


@pytest.mark.parametrize("j", [0, 1])
def test_respond_program_is_derive_keypair(tables, ladder, monkeypatch, j):
    E, _, resp_prog = tables
    monkeypatch.setattr(XM, "x25519", ladder)
    pub, init, ss = _initiation(0, j, ladder)
    st, res = OM.open_one(RESPONDER, pub, init["ephemeral"], init["encrypted_static"], init["encrypted_timestamp"], ss,
                          [XM.public_key(INITIATORS[0])])
    assert st == OM.OPEN_OK
    args = (res["hash"], res["chain_key"], init["ephemeral"], res["remote_static"], RESP_EPH[j], 0x01020304 + j, 0xA1B2C3D4 - j)
    want = RM.respond_one(*args)
    got = CM.respond_one(E, resp_prog, *args, ladder, XM.public_key)
    assert len(got["response"]) == 92
    for f in ("response", "send_key", "recv_key"):
        assert got[f] == want[f], f
