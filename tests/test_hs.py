"""tests/hs_model.py, the CPU model of wg_blake2s_batch / wg_hs_check, against known answers; the order of
the six check steps; the compaction; the ctypes layouts against the header; the Blake2s mirror's
argument errors. No GPU compute here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hs_model as M
from wgtest import ROOT, noise, wg

PUB = bytes(range(100, 132))


# ---- known answers ---------------------------------------------------------------------------------
def test_model_rfc7693_appendix_b():
    assert M.blake2s(b"abc").hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"


def test_model_keyed_kat_empty_input():
    assert M.blake2s(b"", bytes(range(32))).hex() == "48a8997da407876b3d79c0d92325ad3b89cbb754d86ab71aee047ad345fd2c49"


def test_model_mac1_of_zeros():
    assert M.mac1(bytes(116), bytes(32)).hex() == "a27f47acf041191bf95a6748dc26d89e"


def test_model_batch_descriptors():
    inp = bytes(range(200))
    d = np.zeros(6, M.B2S_DESC)
    d[0] = (3, 1, 0, 50, 32, 0, (0, 0))      # unkeyed
    d[1] = (3, 40, 101, 50, 16, 32, (0, 0))  # keyed
    d[2] = (0, 80, 0, 1, 0, 0, (0, 0))       # outlen 0
    d[3] = (0, 80, 0, 1, 33, 0, (0, 0))      # outlen 33
    d[4] = (151, 80, 0, 50, 8, 0, (0, 0))    # input one byte past the buffer
    d[5] = (0, 93, 0, 1, 8, 0, (0, 0))       # output one byte past the buffer
    out, st = M.b2s_batch(d, inp, b"\x5a" * 100)
    assert st == [0, 0, 1, 1, 1, 1]
    assert out[1:33] == M.blake2s(inp[3:53]) and out[40:56] == M.blake2s(inp[3:53], inp[101:133], 16)
    assert out[0:1] + out[33:40] + out[56:] == b"\x5a" * (1 + 7 + 44)


# ---- the six steps, in order -------------------------------------------------------------------------
def _ring(msgs):
    buf, off, lens = bytearray(b"\xee"), [], []
    for m, wl in msgs:
        off.append(len(buf))
        lens.append(len(m) if wl is None else wl)
        buf += m + b"\xee\xee\xee"
    return bytes(buf), off, lens


def test_steps_in_order():
    init = M.message(1, bytes(range(1, 116)), PUB)
    resp = M.message(2, bytes(range(1, 60)), PUB)
    assert len(init) == 148 and len(resp) == 92

    def flip(m, at):
        return m[:at] + bytes([m[at] ^ 0x10]) + m[at + 1:]

    bad_both = flip(flip(init, 120), 140)  # mac1 and mac2 wrong: mac1 is found first
    type3_len91 = bytes([3]) + resp[1:91]  # type and length wrong: the type is found first
    msgs = [(init, None), (resp, None),
            (flip(init, 50), None), (flip(init, 116), None), (flip(init, 147), None), (bad_both, None),
            (flip(resp, 59), None), (flip(resp, 75), None), (flip(resp, 76), None),
            (init, 147), (init + b"\0", 149), (resp, 91), (resp + b"\0", 93), (init, 0),
            (type3_len91, None), (bytes([4]) + init[1:], None), (bytes([0]) + init[1:], None),
            (init[:92], 92), (resp + bytes(56), 148)]  # a type-1 message of a response's size and the reverse
    wire, off, lens = _ring(msgs)
    off += [len(wire) - 147, len(wire), len(wire) + 1, (1 << 64) - 10]
    lens += [148, 148, 148, 148]
    st, rec, s = M.check(wire, off, lens, PUB)
    assert st == [0, 0, 3, 3, 4, 3, 3, 3, 4, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1]
    assert s == dict(n_valid=2, n_init=1, n_resp=1, n_rejected=21)
    assert rec["index"].tolist() == [0, 1] and rec["len"].tolist() == [148, 92]
    assert rec[0]["msg"].tobytes() == init and rec[1]["msg"].tobytes() == resp + bytes(56)
    # another public key: nothing passes mac1
    st2, rec2, s2 = M.check(wire, off, lens, bytes(32))
    assert st2[:2] == [3, 3] and s2["n_valid"] == 0 and len(rec2) == 0
    # the ring's stated size decides, not the buffer's
    st3, _, _ = M.check(wire, off, lens, PUB, wire_size=off[1] + 91)
    assert st3[:2] == [0, 1]


def test_list_compaction_and_summary():
    rng = np.random.default_rng(5)
    msgs = []
    for k in range(40):
        t = 1 + k % 2
        m = M.message(t, rng.bytes(120), PUB)
        if k % 3 == 0:
            m = m[:5] + bytes([m[5] ^ 1]) + m[6:]
        msgs.append((m, None))
    wire, off, lens = _ring(msgs)
    lst = [39, 2, 2, 40, 7, 0, 1, 1000, 38]  # any order, repeats, indices past the batch
    st, rec, s = M.check(wire, off, lens, PUB, lst=lst)
    assert st == [3, 0, 0, 1, 0, 3, 0, 1, 0]
    assert rec["index"].tolist() == [2, 2, 7, 1, 38] and rec["len"].tolist() == [148, 148, 92, 92, 148]
    assert s == dict(n_valid=5, n_init=3, n_resp=2, n_rejected=4)
    assert (rec["_pad"] == 0).all() and all(r["msg"][92:].sum() == 0 for r in rec if r["len"] == 92)
    st, rec, s = M.check(wire, off, lens, PUB, lst=[])
    assert st == [] and len(rec) == 0 and s == dict(n_valid=0, n_init=0, n_resp=0, n_rejected=0)
    assert len(M.check(wire, off, lens, PUB, lst=list(range(40)) * 2)[0]) == 40  # cut to n entries


# ---- layouts -----------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    fields = [("wg_b2s_desc", "WgB2sDesc", ["in_off", "out_off", "key_off", "len", "outlen", "keylen", "_pad"]),
              ("wg_hs_record", "WgHsRecord", ["index", "len", "msg", "_pad"]),
              ("wg_hs_summary", "WgHsSummary", ["n_valid", "n_init", "n_resp", "n_rejected"]),
              ("wg_hs_batch", "WgHsBatch", ["wire", "wire_size", "pkt_off", "pkt_len", "list", "n_list", "hs_status",
                                            "records", "summary", "n", "_reserved"])]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += 'printf("%u %u %u %u %u %u %u %u %u\\n", WG_B2S_OK, WG_B2S_BADDESC, WG_HS_OK, WG_HS_BADLEN, WG_HS_BADTYPE,' \
            ' WG_HS_BADMAC1, WG_HS_BADMAC2, WG_HS_INIT_SIZE, WG_HS_RESP_SIZE);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\nint main(void){' + body + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    L = wg()._lib
    want = []
    for _, p, fs in fields:
        cls = getattr(L, p)
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    want += [L.WG_B2S_OK, L.WG_B2S_BADDESC, L.WG_HS_OK, L.WG_HS_BADLEN, L.WG_HS_BADTYPE, L.WG_HS_BADMAC1,
             L.WG_HS_BADMAC2, L.WG_HS_INIT_SIZE, L.WG_HS_RESP_SIZE]
    assert got == want
    assert ctypes.sizeof(L.WgB2sDesc) == 32 and ctypes.sizeof(L.WgHsRecord) == 160
    W = wg()
    assert W.WG_B2S_DTYPE.itemsize == 32 and W.WG_HS_RECORD_DTYPE.itemsize == 160
    assert W.WG_B2S_DTYPE == M.B2S_DESC and W.WG_HS_RECORD_DTYPE == M.HS_RECORD
    assert [M.B2S_OK, M.B2S_BADDESC, M.HS_OK, M.HS_BADLEN, M.HS_BADTYPE, M.HS_BADMAC1, M.HS_BADMAC2] == want[-9:-2]
    d = W.pack_b2s_desc([1], [2], [3], [4], [5], [6])
    assert W.desc_as_int64(d).tolist() == [[1, 2, 3, 4 | 5 << 32 | 6 << 40]]


def test_new_calls_are_bound():
    names = {name for name, _, _ in wg()._lib.SIGNATURES}
    assert {"wg_blake2s_batch", "wg_hs_key_set", "wg_hs_reserve", "wg_hs_check"} <= names
    lib = wg().lib()
    assert all(hasattr(lib, n) for n in ("wg_blake2s_batch", "wg_hs_key_set", "wg_hs_reserve", "wg_hs_check"))


# ---- the mirror's argument errors (Blake2s.java:55-78, 111-114) -------------------------------------------
def test_blake2s_mirror_argument_errors():
    N = noise()
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="digestLength must be in"):
            N.Blake2s(bad)
    with pytest.raises(ValueError, match="key's length must be at most 32"):
        N.Blake2s(32, bytes(33))
    with pytest.raises(ValueError, match="key's length"):  # the key is looked at first (Blake2s.java:74-78)
        N.Blake2s(0, bytes(33))
    with pytest.raises(TypeError):
        N.Blake2s(32, None)
    h = N.Blake2s(16, bytes(32))
    assert h.digestLength == 16 and N.Blake2s.algorithm() == "BLAKE2s"
    for off, ln in ((-1, 1), (0, -1), (3, 2), (5, 0)):
        with pytest.raises(IndexError):
            h.update(b"abcd", off, ln)
    h.update(b"abcd", 1, 2)
    h.update(0x41)
    assert bytes(h._buf) == b"bcA"
