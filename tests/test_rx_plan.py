"""tests/rx_plan_model.py on hand-written cases (the model is what wg_rx_plan / wg_rx_deliver are compared
with on the GPU, tests/test_gpu_rx_plan.py), its agreement with oracle.parse_wire, the layout of the new
structs against the header, and the new status values. No GPU here."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np

import rx_plan_model as M
from wgtest import ROOT, oracle, wg

HDR = open(os.path.join(ROOT, "include", "wgaead.h")).read()


def _pkt(t, index=0, counter=0, payload=0, fill=0xAB):
    """A datagram of 16 + payload bytes: header {type, 0, 0, 0, LE32 index, LE64 counter}, then payload."""
    return struct.pack("<BxxxIQ", t, index, counter) + bytes([fill]) * payload


def _ring(pkts, gap=3):
    """Packets at unaligned offsets with `gap` bytes between them."""
    off, buf = [], bytearray(b"\x00" * 5)
    for p in pkts:
        off.append(len(buf))
        buf += p + b"\xEE" * gap
    return bytes(buf), off, [len(p) for p in pkts]


SESS = {7: 3, 0: 9, 0xFFFFFFFF: 1}


def test_each_status_in_check_order():
    pkts = [
        _pkt(4, 7, 0x1122334455667788, 16 + 40),   # 0: OK, len 40
        b"",                                       # 1: wl = 0 -> BADHDR
        bytes([1]),                                # 2: a one-byte type 1 is still a handshake
        _pkt(2, 99, 5, 76),                        # 3: response -> HANDSHAKE
        bytes([3]) + b"\0" * 60,                   # 4: type 3 -> BADHDR
        bytes([9]) + b"\0" * 60,                   # 5: type 9 -> BADHDR
        _pkt(4, 7, 1, 15),                         # 6: type 4, wl = 31 -> BADHDR (before the lookup)
        _pkt(4, 1234, 1, 16),                      # 7: unknown index -> NOSESSION (keepalive-sized)
        _pkt(4, 1234, 1, 16 + 500),                # 8: unknown index AND too long -> NOSESSION comes first
        _pkt(4, 0, 2, 16 + 101),                   # 9: len 101 > max_len 100 -> TOOLONG, key slot 9 kept
        _pkt(4, 0xFFFFFFFF, 3, 16),                # 10: keepalive, OK, len 0
        _pkt(4, 0, 4, 16 + 100),                   # 11: OK, len 100 = max_len
    ]
    wire, off, lens = _ring(pkts)
    wire += b"\0" * 200  # room for the plaintexts behind the packets (AFTER)
    d, st, host, s = M.plan(wire, off, lens, SESS, max_len=100, mode=M.PT_AFTER)
    assert st == [M.PKT_OK, M.PKT_BADHDR, M.PKT_HANDSHAKE, M.PKT_HANDSHAKE, M.PKT_BADHDR, M.PKT_BADHDR, M.PKT_BADHDR,
                  M.PKT_NOSESSION, M.PKT_NOSESSION, M.PKT_TOOLONG, M.PKT_OK, M.PKT_OK]
    assert host == [2, 3] and s == dict(pt_used=0, n_open=3, n_host=2)
    assert tuple(d[0]) == (off[0] + 16, off[0] + lens[0], 0x1122334455667788, 40, 3)
    assert tuple(d[10]) == (off[10] + 16, off[10] + 32, 3, 0, 1)
    for i in (1, 2, 3, 4, 5, 6, 7, 8):
        assert tuple(d[i]) == (off[i] + 16, off[i] + lens[i], 0, M.LEN_INVALID, 0), i
    assert tuple(d[9]) == (off[9] + 16, off[9] + lens[9], 0, M.LEN_INVALID, 9)
    # a packet that starts past the ring, one that ends past it, and one whose PLAINTEXT would (AFTER only)
    ws = len(wire)
    last = _pkt(4, 7, 8, 16 + 64)
    wire2 = wire + last
    off2, lens2 = [ws + len(last) + 1, ws, ws], [40, len(last) + 1, len(last)]
    d, st, host, s = M.plan(wire2, off2, lens2, SESS, max_len=100, mode=M.PT_AFTER)
    assert st == [M.PKT_BADHDR, M.PKT_BADHDR, M.PKT_BADHDR]
    assert [int(x) for x in d["key_slot"]] == [0, 0, 3]  # step 6 fails after the lookup succeeded
    d, st, host, s = M.plan(wire2, off2, lens2, SESS, max_len=100, mode=M.PT_PACKED, pt_base=32, pt_size=4096)
    assert st == [M.PKT_BADHDR, M.PKT_BADHDR, M.PKT_OK] and int(d[2]["out_off"]) == 32 and s["pt_used"] == 64
    assert [int(x) for x in d["out_off"][:2]] == [32, 32]
    # offsets near 2^64 wrap in the descriptor and are BADHDR
    d, st, _, _ = M.plan(wire, [M.MASK64 - 3], [40], SESS, max_len=100, mode=M.PT_AFTER)
    assert st == [M.PKT_BADHDR] and tuple(d[0]) == (12, 36, 0, M.LEN_INVALID, 0)


def test_packed_cursor_overflow_and_keepalive_after_it():
    lens_pt = [40, 0, 17, 100, 1, 0, 16]
    pkts = [_pkt(4, 7, k, 16 + L) for k, L in enumerate(lens_pt)]
    pkts.insert(3, _pkt(1, 0, 0, 132))       # a handshake in between takes no room
    pkts.insert(5, _pkt(4, 555, 0, 16 + 64))  # nor does an unknown session
    wire, off, lens = _ring(pkts)
    # C: 0 (40 -> 48), 48 (0), 48 (17 -> 32), -, 80 (100 -> 112), -, 192 (1 -> 16), 208 (0), 208 (16) -> 224
    d, st, host, s = M.plan(wire, off, lens, SESS, max_len=100, mode=M.PT_PACKED, pt_base=16, pt_size=16 + 224)
    assert [int(x) for x in d["out_off"]] == [16, 64, 64, 16, 96, 16, 208, 224, 224]
    assert st == [0, 0, 0, M.PKT_HANDSHAKE, 0, M.PKT_NOSESSION, 0, 0, 0] and s == dict(pt_used=224, n_open=7, n_host=1)
    # pt_size cuts inside the 100-B packet: it and everything after it is TOOLONG (the keepalives too, whose
    # offset lies past pt_size), yet the cursor runs on and pt_used is the full sum
    d, st, host, s = M.plan(wire, off, lens, SESS, max_len=100, mode=M.PT_PACKED, pt_base=16, pt_size=16 + 80 + 99)
    assert st == [0, 0, 0, M.PKT_HANDSHAKE, M.PKT_TOOLONG, M.PKT_NOSESSION, M.PKT_TOOLONG, M.PKT_TOOLONG,
                  M.PKT_TOOLONG]
    assert s == dict(pt_used=224, n_open=3, n_host=1)
    assert [int(x) for x in d["out_off"][4:]] == [16] * 5 and [int(x) for x in d["key_slot"][4:]] == [3, 0, 3, 3, 3]
    # one byte more and the 100-B packet fits exactly; a keepalive whose offset equals pt_size fits as well
    d, st, host, s = M.plan(wire, off, lens, SESS, max_len=100, mode=M.PT_PACKED, pt_base=0, pt_size=208)
    assert st[4] == M.PKT_OK and st[6] == M.PKT_OK and st[7] == M.PKT_OK and st[8] == M.PKT_TOOLONG
    # a pt_base past pt_size: nothing fits, not even a keepalive
    d, st, host, s = M.plan(wire, off, lens, SESS, max_len=100, mode=M.PT_PACKED, pt_base=300, pt_size=200)
    assert st.count(M.PKT_TOOLONG) == 7 and s["n_open"] == 0 and s["pt_used"] == 224


def test_host_list_is_ascending_batch_order():
    types = [4, 1, 2, 9, 1, 4, 2, 2, 4, 1]
    pkts = [_pkt(t, 7, k, 32) for k, t in enumerate(types)]
    wire, off, lens = _ring(pkts)
    _, st, host, s = M.plan(wire, off, lens, SESS, max_len=64, mode=M.PT_PACKED, pt_size=1 << 20)
    assert host == [1, 2, 4, 6, 7, 9] and s["n_host"] == 6
    assert [st[i] for i in host] == [M.PKT_HANDSHAKE] * 6


def test_deliver_merge_and_stable_order():
    d = np.zeros(8, M.WG_PKT)
    d["out_off"], d["len"], d["key_slot"] = np.arange(8) * 64 + 16, [10, 0, 30, 40, 50, 60, 70, 80], np.arange(8) + 100
    plan_st = [0, 0, M.PKT_HANDSHAKE, 0, M.PKT_NOSESSION, 0, 0, M.PKT_TOOLONG]
    open_st = [0, M.PKT_KEEPALIVE, M.PKT_BADTAG, M.PKT_BADTAG, M.PKT_BADTAG, M.PKT_REPLAY, 0, 0]
    final, items, idx, s = M.deliver(d, plan_st, open_st)
    # the plan's verdict wins wherever it is not OK: the open reports those packets as BADTAG (or anything)
    assert final == [0, M.PKT_KEEPALIVE, M.PKT_HANDSHAKE, M.PKT_BADTAG, M.PKT_NOSESSION, M.PKT_REPLAY, 0,
                     M.PKT_TOOLONG]
    assert idx == [0, 6] and s == dict(bytes=80, n_items=2, n_keepalive=1)
    assert [tuple(x) for x in items] == [(16, 10, 100), (6 * 64 + 16, 70, 106)]
    final, items, idx, s = M.deliver(d, [0] * 8, [0] * 8)
    assert idx == list(range(8)) and s == dict(bytes=340, n_items=8, n_keepalive=0)
    assert items["off"].tolist() == d["out_off"].tolist()
    final, items, idx, s = M.deliver(d, [M.PKT_BADHDR] * 8, [0] * 8)
    assert idx == [] and len(items) == 0 and s == dict(bytes=0, n_items=0, n_keepalive=0)


def test_model_agrees_with_the_parse_oracle_in_after_mode():
    """Type-4 packets of known sessions, AFTER mode: descriptors and statuses equal oracle.parse_wire's
    (fed the sessions' key slots), including short packets, wrong type bytes mapped to BADHDR and a
    plaintext that overruns the ring. parse_wire keeps the caller's key slot on a rejected packet, the
    plan writes 0 where it never reached the lookup, so key slots are compared on the accepted ones."""
    O = oracle()
    rng = np.random.default_rng(11)
    idx = [int(x) for x in rng.integers(0, 1 << 32, 20)]
    sess = {x: k + 5 for k, x in enumerate(idx)}
    pkts = []
    for k in range(300):
        wl = int(rng.choice([1, 15, 31, 32, 33, 48, 100, 180]))
        t = 4 if rng.random() < 0.9 else int(rng.choice([0, 3, 5, 9, 255]))
        p = bytearray(rng.bytes(max(wl, 16)))
        p[0:16] = struct.pack("<BxxxIQ", t, idx[k % 20], int(rng.integers(0, 1 << 63)))
        pkts.append(bytes(p[:wl]))
    wire, off, lens = _ring(pkts, gap=1)
    wire += b"\0" * 100  # the last packets' plaintexts overrun
    slots = [sess[idx[k % 20]] for k in range(300)]
    d, st, host, s = M.plan(wire, off, lens, sess, max_len=65535, mode=M.PT_AFTER)
    w = np.frombuffer(wire, np.uint8)
    od, ost = O.parse_wire(w, np.array(off, np.uint64), np.array(lens, np.uint32), np.array(slots, np.uint32))
    assert st == ost.tolist() and set(st) == {M.PKT_OK, M.PKT_BADHDR} and host == []
    ok = np.array(st) == M.PKT_OK
    assert 100 < ok.sum() < 300
    for f in ("in_off", "out_off", "counter", "len"):
        assert d[f].tolist() == od[f].tolist(), f
    assert d["key_slot"][ok].tolist() == od["key_slot"][ok].tolist()


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"wg_rx_batch": ["wire", "wire_size", "pkt_off", "pkt_len", "desc_out", "rx_status", "host_list",
                              "summary", "pt_base", "pt_size", "n", "max_len", "mode", "_reserved"],
              "wg_rx_summary": ["pt_used", "n_open", "n_host"],
              "wg_rx_item": ["off", "len", "key_slot"],
              "wg_rx_delivered": ["bytes", "n_items", "n_keepalive"],
              "wg_rx_deliver_batch": ["desc", "plan_status", "open_status", "final_status", "items", "index_out",
                                      "delivered", "n", "_reserved"]}
    L = wg()._lib
    py = {"wg_rx_batch": L.WgRxBatch, "wg_rx_summary": L.WgRxSummary, "wg_rx_item": L.WgRxItem,
          "wg_rx_delivered": L.WgRxDelivered, "wg_rx_deliver_batch": L.WgRxDeliverBatch}
    body = "".join(f'printf("%zu", sizeof({s})); ' + "".join(f'printf(" %zu", offsetof({s}, {f})); ' for f in fs) +
                   'printf("\\n"); ' for s, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\nint main(void){' + body +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rows = subprocess.check_output([str(exe)]).decode().splitlines()
    for (s, fs), row in zip(fields.items(), rows):
        got = [int(x) for x in row.split()]
        assert [n for n, _ in py[s]._fields_] == fs, s
        assert got == [ctypes.sizeof(py[s])] + [getattr(py[s], f).offset for f in fs], s
    assert M.WG_PKT.itemsize == 32 and M.RX_ITEM.itemsize == ctypes.sizeof(L.WgRxItem) == 16
    assert ctypes.sizeof(L.WgRxSummary) == ctypes.sizeof(L.WgRxDelivered) == 16


def test_new_status_values_in_the_header_and_bindings():
    def define(name):
        return int(re.search(rf"#define {name} (\d+)u", HDR).group(1))
    L = wg()._lib
    assert define("WG_PKT_NOSESSION") == 10 == L.WG_PKT_NOSESSION == M.PKT_NOSESSION
    assert define("WG_PKT_HANDSHAKE") == 11 == L.WG_PKT_HANDSHAKE == M.PKT_HANDSHAKE
    assert define("WG_PKT_BADHDR") == M.PKT_BADHDR and define("WG_PKT_TOOLONG") == M.PKT_TOOLONG == L.WG_PKT_TOOLONG
    assert define("WG_RX_PT_AFTER") == 0 == L.WG_RX_PT_AFTER == M.PT_AFTER
    assert define("WG_RX_PT_PACKED") == 1 == L.WG_RX_PT_PACKED == M.PT_PACKED
    # every other status keeps its value: the new ones collide with none
    vals = [int(v) for v in re.findall(r"#define WG_PKT_[A-Z]+ (\d+)u", HDR)]
    assert len(vals) == len(set(vals)) == 13
    for fn in ("wg_rx_sessions_set", "wg_rx_reserve", "wg_rx_plan", "wg_rx_deliver"):
        assert hasattr(wg().lib(), fn), fn
