"""wg_hs_stamp without a GPU: tests/hs_stamp_model.py opens what hs_open_model.initiate and hs_initiate_model (the
restatement of the initiator mirror's message) sealed; its rule against a brute-force restatement of the header's six
steps and against WireGuard's one-by-one walk; kStampProgram, printed from wg_hs_chain.h by a host compiler and
interpreted, against the model; the binding's layouts against include/wgaead.h."""
import ctypes
import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hs_initiate_model as IM
import hs_open_model as OM
import hs_stamp_model as SM
import x25519_model as XM
from wgtest import ROOT, oracle, splitmix_bytes, wg

RESPONDER = splitmix_bytes(0x7500, 32)
TRIPLES = [(splitmix_bytes(0x7510 + j, 32), splitmix_bytes(0x7520 + j, 32), splitmix_bytes(0x7530 + j, 12)) for j in range(8)]
ladder = functools.lru_cache(maxsize=None)(XM.x25519)


@pytest.fixture(autouse=True)
def memoised_ladder(monkeypatch):
    monkeypatch.setattr(XM, "x25519", ladder)  # (the models call the ladder through the module)


def _message(j, sealer):
    """Triple j's 148-byte initiation to RESPONDER, and the two secrets the responder has for it."""
    initiator, eph, ts = TRIPLES[j]
    pub = XM.public_key(RESPONDER)
    if sealer == "open_model":
        msg = (bytes([1]) + OM.body(0x100 + j, OM.initiate(initiator, pub, eph, ts))).ljust(148, b"\0")
    else:
        msg = IM.initiate_one(initiator, pub, eph, ts, 0x100 + j)["message"]
    return pub, msg, ladder(RESPONDER, msg[8:40]), ladder(RESPONDER, XM.public_key(initiator))


@pytest.mark.parametrize("sealer", ["open_model", "initiate_model"])
def test_round_trip(sealer):
    for j, (_, _, ts) in enumerate(TRIPLES):
        pub, msg, ss, ss_p = _message(j, sealer)
        assert SM.open_timestamp(pub, msg, ss, ss_p) == ts
        for at in (88, 88 + (5 * j + 1) % 28, 99, 100, 115):  # anywhere in ets: ciphertext and tag
            bad = msg[:at] + bytes([msg[at] ^ (1 << (j % 8))]) + msg[at + 1:]
            assert SM.open_timestamp(pub, bad, ss, ss_p) is None
        # the key is NOT wg_hs_init's chain_key, nor anything derived from it: the chain must be walked again
        st, res = OM.open_one(RESPONDER, pub, msg[8:40], msg[40:88], msg[88:116], ss, [XM.public_key(TRIPLES[j][0])])
        assert st == OM.OPEN_OK
        k, h = SM.timestamp_key(pub, msg[8:40], msg[40:88], ss, ss_p)
        O = oracle()
        assert O.py_aead_open(k, OM.ZERO_NONCE, msg[88:116], h) == ts
        for wrong_key in (OM.derive_key(res["chain_key"], ss_p, 2), OM.derive_key(res["chain_key"], ss, 2), res["chain_key"]):
            for aad in (h, res["hash"]):
                assert O.py_aead_open(wrong_key, OM.ZERO_NONCE, msg[88:116], aad) is None
        assert O.py_aead_open(k, OM.ZERO_NONCE, msg[88:116], res["hash"]) is None  # nor is the aad the final hash


def brute(entries, stored):
    """Steps 1-6 as the header words them, every test a search through the call's entries."""
    out = []
    for j, (pre, p, t) in enumerate(entries):
        if pre is not None:  # 1-3
            out.append(pre)
        elif t <= stored.get(p, SM.ZERO_TS):  # 4: not greater than the value at the start of the call
            out.append(SM.TS_REPLAY)
        elif any(pre2 is None and p2 == p and (t2 > t or (t2 == t and k < j)) for k, (pre2, p2, t2) in enumerate(entries) if k != j):
            out.append(SM.TS_SUPERSEDED)  # 5
        else:
            out.append(SM.TS_OK)  # 6
    return out


def test_rule_against_brute_force_and_the_one_by_one_walk():
    values = [bytes(12), bytes(11) + b"\x01", bytes(8) + b"\x00\x00\x01\x00", bytes(7) + b"\x01" + bytes(4),
              b"\x01" + bytes(11), b"\xff" * 12]
    seen = {s: 0 for s in range(6)}
    ties = 0
    for seed in range(300):
        rng = np.random.default_rng(0x7540 + seed)
        n, n_peers = int(rng.integers(0, 65)), int(rng.integers(1, 6))
        stored = {p: values[int(rng.integers(0, 6))] for p in range(n_peers) if rng.random() < 0.5}
        entries = []
        for _ in range(n):
            q = rng.random()
            pre = SM.TS_NOPEER if q < 0.08 else SM.TS_BADDESC if q < 0.14 else SM.TS_BADAUTH if q < 0.25 else None
            entries.append((pre, SM.NOPEER if pre == SM.TS_NOPEER else int(rng.integers(0, n_peers)),
                            values[int(rng.integers(0, 6))]))  # (a refused entry's would-be T must not count)
        got, after = SM.rule(entries, stored)
        assert got == brute(entries, stored)
        # WireGuard's rule, one entry at a time in arrival order
        walk, last = dict(stored), {}
        for j, (pre, p, t) in enumerate(entries):
            if pre is None and t > walk.get(p, SM.ZERO_TS):
                walk[p], last[p] = t, j
        assert after == walk
        # our OK entry of each peer is the entry that walk accepts last (the first that carries the final value: a
        # later equal one is not greater)
        assert {p: j for j, (pre, p, t) in enumerate(entries) if got[j] == SM.TS_OK} == last
        for s in got:
            seen[s] += 1
        ties += sum(got[j] == SM.TS_SUPERSEDED and entries[j][2] == after[entries[j][1]] for j in range(n))
    assert all(v > 50 for v in seen.values()) and ties > 20, (seen, ties)


NAMES = ["OP_PAD", "OP_IN32", "OP_OUT", "OP_T1", "OP_TN", "OP_H2", "OP_H0", "OP_ES2", "OP_SES1", "OP_STS", "SRC_ZERO", "SRC_CK",
         "SRC_X", "SRC_E", "SRC_SS", "SRC_STATIC", "PAD_IPAD", "PAD_OPAD", "PAD_LAST", "PAD_SEAL", "DST_NONE", "DST_H", "DST_X",
         "DST_CK", "DST_IST", "DST_OST", "kStampSteps", "kOpenSteps"]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(E, stamp program): the header's enums and constants by name, and kStampProgram."""
    d = tmp_path_factory.mktemp("hs_stamp")
    body = "".join(f'printf("{n} %u\\n", (unsigned)wghc::{n});' for n in NAMES)
    body += ('for (const wghc::Step& s : wghc::kStampProgram) printf("stamp %u %u %u %u\\n", (unsigned)s.op, (unsigned)s.arg, '
             "(unsigned)s.imm, (unsigned)s.dst);")
    src = d / "table.cpp"
    src.write_text('#include <stdio.h>\n#include "wg_hs_chain.h"\nint main(){' + body + " return 0;}\n")
    exe = d / "table"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "wireguard-java_amd", "csrc"), "-o", str(exe), str(src)])
    E, prog = SimpleNamespace(), []
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        f = line.split()
        if f[0] == "stamp":
            prog.append(tuple(int(x) for x in f[1:]))
        else:
            setattr(E, f[0], int(f[1]))
    return E, prog


def test_stamp_program_opens_the_timestamp(table):
    E, prog = table
    assert len(prog) == E.kStampSteps == 28 == E.kOpenSteps  # the recomputation costs what the open cost
    assert [s[0] for s in prog].count(E.OP_STS) == 1 and prog[-1][0] == E.OP_STS
    assert prog[-2][3] == E.DST_NONE  # T2, the key, stays in the state for the open
    for j in range(5):
        pub, msg, ss, ss_p = _message(j, "initiate_model")
        if j == 4:
            msg = msg[:100] + bytes([msg[100] ^ 0x40]) + msg[101:]  # the tag's first byte
        ts, h, ck = SM.stamp_one(E, prog, pub, msg, ss, ss_p)
        assert ts == SM.open_timestamp(pub, msg, ss, ss_p) == (None if j == 4 else TRIPLES[j][2])
        # the program's h and ck end where wg_hs_open's do
        st, res = OM.open_one(RESPONDER, pub, msg[8:40], msg[40:88], msg[88:116], ss, [XM.public_key(TRIPLES[j][0])])
        assert st == OM.OPEN_OK and (h, ck) == (res["hash"], res["chain_key"])


def test_header_layouts_and_bindings(tmp_path):
    """include/wgaead.h's new structs and constants as a C compiler lays them out, against _lib.py and the model."""
    fields = [("wg_hs_stamp_summary", "WgHsStampSummary", ["n_ok", "n_stale", "n_badauth", "n_skipped"]),
              ("wg_hs_stamp_batch", "WgHsStampBatch", ["inits", "n_inits", "records", "shared", "ts_status", "opened", "fresh",
                                                       "summary", "n", "n_rec", "flags", "_reserved"]),
              ("wg_hs_init", "WgHsInit", ["record", "peer", "remote_ephemeral", "hash", "chain_key"])]
    consts = ["WG_HS_TS_OK", "WG_HS_TS_REPLAY", "WG_HS_TS_SUPERSEDED", "WG_HS_TS_BADAUTH", "WG_HS_TS_NOPEER", "WG_HS_TS_BADDESC"]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += "".join(f'printf("%u\\n", {c});' for c in consts)
    # n_ok, which wg_hs_respond reads as the entry count, is the first word, as n_emitted is in wg_hs_open's summary
    body += 'printf("%zu\\n", offsetof(wg_hs_stamp_summary, n_ok)); printf("%zu\\n", offsetof(wg_hs_open_summary, n_emitted));'
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\n'
    src = tmp_path / "layout.c"
    src.write_text(head + "int main(void){" + body + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    proto = tmp_path / "proto.c"  # the prototypes, as the header declares them (compiled only)
    proto.write_text(head + "int (*a)(wg_ctx*, const wg_hs_stamp_batch*, void*) = wg_hs_stamp;\n"
                     "int (*b)(wg_ctx*, uint32_t, uint32_t, const uint8_t*) = wg_hs_stamps_set;\n"
                     "int (*c)(wg_ctx*, uint32_t, uint32_t, uint8_t*) = wg_hs_stamps_get;\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"),
                           str(proto)])
    W = wg()
    L = W._lib
    want = []
    for _, p, fs in fields:
        cls = getattr(L, p)
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    want += [getattr(L, c) for c in consts] + [0, 0]
    assert got == want
    assert ctypes.sizeof(L.WgHsStampBatch) == 80 and ctypes.sizeof(L.WgHsStampSummary) == 16
    assert want[-8:-2] == [SM.TS_OK, SM.TS_REPLAY, SM.TS_SUPERSEDED, SM.TS_BADAUTH, SM.TS_NOPEER, SM.TS_BADDESC]
    names = {name for name, _, _ in L.SIGNATURES}
    for f in ("wg_hs_stamp", "wg_hs_stamps_set", "wg_hs_stamps_get"):
        assert f in names and hasattr(W.lib(), f)
    for m in ("hs_stamp", "hs_stamps_set", "hs_stamps_get", "hs_stamp_host"):
        assert callable(getattr(W.Engine, m))
