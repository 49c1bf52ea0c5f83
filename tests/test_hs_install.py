"""wg_hs_install and the device-owned session table without a GPU: tests/hs_install_model.py's bucket-for-bucket table
against a plain dict over seeded random set / retire / install sequences at capacities 16 and 64 (chains that wrap the
table's end, retired entries inside chains, re-installed retired indices, the all-or-nothing FULL rule), its fmix32
inverse, and the binding's layouts against include/wgaead.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hs_install_model as IM
from wgtest import ROOT, splitmix_bytes, wg


def test_fmix32_inverse_and_buckets():
    for k in range(2000):
        x = int.from_bytes(splitmix_bytes(0x7700 + k, 4), "little")
        assert IM.fmix32_inv(IM.fmix32(x)) == x and IM.fmix32(IM.fmix32_inv(x)) == x
    for x in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert IM.fmix32_inv(IM.fmix32(x)) == x
    assert IM.fmix32(0) == 0 and IM.fmix32(1) == 0x514E28B7  # MurmurHash3's finaliser
    for cap in (16, 64, 1024):
        for b in (0, 1, cap - 2, cap - 1):
            got = {IM.index_in_bucket(b, cap, k) for k in range(5)}
            assert len(got) == 5 and all(IM.fmix32(i) & (cap - 1) == b for i in got)
    assert [IM.capacity_for(n) for n in (0, 4, 5, 16, 17, 65536)] == [16, 16, 32, 64, 128, 262144]


def brute_install(live, used, capacity, key_slots, entries, cover, send_slot, recv_slot, slot_first, slot_count, pos_field):
    """The five steps as the header words them, every test a search through the lower entries; `live` is a dict."""
    def step1(j):
        p = int(entries[j][pos_field])
        if p >= len(send_slot):
            return None
        s, r = int(send_slot[p]), int(recv_slot[p])
        ok = all(slot_first <= x < slot_first + slot_count and x < key_slots for x in (s, r)) and s != r
        return (s, r) if ok else None

    def step2(j):
        return step1(j) and not any(step1(k) and set(step1(k)) & set(step1(j)) for k in range(j))

    def step3(j):
        li = int(entries[j]["local_index"])
        return step2(j) and li not in live and not any(step2(k) and int(entries[k]["local_index"]) == li for k in range(j))

    cand = [j for j in range(cover) if step3(j)]
    full = used + len(cand) > capacity // 2
    status = []
    for j in range(cover):
        status.append(IM.INST_BADSLOT if not step1(j) else IM.INST_DUPSLOT if not step2(j) else IM.INST_DUPINDEX if not step3(j)
                      else IM.INST_FULL if full else IM.INST_OK)
    return status


def crowded_indices(cap, rng, n):
    """Indices that crowd a few buckets, the table's last two among them, so that chains form and wrap."""
    buckets = [cap - 1, cap - 2, int(rng.integers(0, cap)), int(rng.integers(0, cap))]
    return [IM.index_in_bucket(buckets[int(rng.integers(0, len(buckets)))], cap, int(rng.integers(0, 12))) for _ in range(n)]


@pytest.mark.parametrize("cap", [16, 64])
@pytest.mark.parametrize("source", [IM.SRC_SESSIONS, IM.SRC_ESTABLISHED])
def test_model_against_dict(cap, source):
    key_slots = 4 * cap
    seen = dict(wrap=0, retired_in_chain=0, reinstall=0, full=0, dupslot=0, dupindex=0, badslot=0, ok=0)
    for seed in range(40):
        rng = np.random.default_rng(1000 * cap + 10 * seed + source)
        T = IM.Table(capacity=cap)
        S = IM.State(key_slots)
        live, used, retired_ever = {}, 0, set()
        for step in range(30):
            op = int(rng.integers(0, 10))
            if op == 0:  # a rebuild on the host
                idx = list(dict.fromkeys(crowded_indices(cap, rng, int(rng.integers(0, cap // 4 + 1)))))
                slots = [int(rng.integers(0, key_slots)) for _ in idx]
                T.set(idx, slots)
                live, used = dict(zip(idx, slots)), len(idx)
                assert T.capacity == cap
            elif op <= 3:  # retire: live ones, unknown ones, repeats
                pool = list(live) + crowded_indices(cap, rng, 2)
                pick = [pool[int(rng.integers(0, len(pool)))] for _ in range(int(rng.integers(0, 5)))]
                want = len({i for i in pick if i in live})
                assert T.retire(pick) == want
                for i in pick:
                    if live.pop(i, None) is not None:
                        retired_ever.add(i)
            else:  # install
                n = int(rng.integers(1, max(9, cap // 4)))
                n_slots = n + int(rng.integers(0, 3))
                ent = np.zeros(n, IM.DTYPES[source])
                # mostly one position each; now and then a repeated one, or one past the slot arrays
                ent[IM.POSITION[source]] = np.where(rng.random(n) < 0.15, rng.integers(0, n_slots + 1, n), rng.permutation(n_slots)[:n])
                pool = crowded_indices(cap, rng, n) + list(live)[:2] + list(retired_ever)[:2]
                ent["local_index"] = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
                ent["remote_index"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
                ent["send_key"] = rng.integers(1, 256, (n, 32))
                ent["recv_key"] = rng.integers(1, 256, (n, 32))
                first, count = int(rng.integers(0, 8)), key_slots // 2
                pair = first + rng.permutation(count)[:2 * n_slots].reshape(2, n_slots)  # distinct slots, mostly
                send = np.where(rng.random(n_slots) < 0.1, rng.integers(first, first + count + 2, n_slots), pair[0])  # (or past the range)
                recv = np.where(rng.random(n_slots) < 0.05, send, pair[1])
                cover = None if rng.random() < 0.5 else int(rng.integers(0, n + 2))
                c = n if cover is None else min(cover, n)
                want = brute_install(live, used, cap, key_slots, ent, c, send, recv, first, count, IM.POSITION[source])
                before = ent.copy()
                got, summary = IM.install(T, S, ent, cover, send, recv, slot_first=first, slot_count=count, source=source)
                assert got == want
                assert summary == dict(n_ok=want.count(0), n_badslot=want.count(1), n_dup=want.count(2) + want.count(3),
                                       n_full=want.count(4))
                for j in range(n):
                    if j < c and want[j] == IM.INST_OK:
                        p = int(before[j][IM.POSITION[source]])
                        li = int(before[j]["local_index"])
                        seen["reinstall"] += li in retired_ever
                        live[li] = int(recv[p])
                        used += 1
                        assert S.keys[int(send[p])] == before[j]["send_key"].tobytes()
                        assert S.keys[int(recv[p])] == before[j]["recv_key"].tobytes()
                        assert S.receivers[int(send[p])] == int(before[j]["remote_index"])
                        assert not ent[j]["send_key"].any() and not ent[j]["recv_key"].any()
                    else:
                        assert ent[j] == before[j]  # a refused entry, or one behind the cover, keeps every byte
                for name, code in (("full", 4), ("dupslot", 2), ("dupindex", 3), ("badslot", 1), ("ok", 0)):
                    seen[name] += want.count(code)
            # the table against the dict, whatever the operation was
            assert T.live() == live and T.used == used and T.count() == (len(live), used - len(live))
            assert used <= cap // 2 or op == 0
            probe = list(live) + list(retired_ever) + crowded_indices(cap, rng, 4)
            for i in probe:
                assert T.lookup(i) == live.get(i)
            for i in live:  # what kinds of chains did this table hold?
                b0, k = IM.fmix32(i) & (cap - 1), T.chain(i)
                seen["wrap"] += b0 + k > cap
                seen["retired_in_chain"] += any(T.ent[(b0 + d) & (cap - 1)][1] == IM.RETIRED for d in range(k - 1))
    assert all(v > 0 for v in seen.values()), seen


def test_reserve_keeps_live_and_drops_retired():
    T = IM.Table(max_sessions=4)
    assert T.capacity == 16
    idx = [IM.index_in_bucket(15, 16, k) for k in range(4)]
    T.set(idx, [1, 2, 3, 4])
    assert T.retire([idx[1], idx[1], 12345]) == 1 and T.count() == (3, 1) and T.used == 4
    assert T.lookup(idx[1]) is None and T.lookup(idx[2]) == 3  # behind the retired entry, across the table's end
    T.reserve(40)
    assert T.capacity == 256 and T.count() == (3, 0) and T.live() == {idx[0]: 1, idx[2]: 3, idx[3]: 4}
    T.set(list(range(100)), list(range(100)))  # its own rule asks for more than the reserve
    assert T.capacity == 512


def test_header_layouts_and_bindings(tmp_path):
    """include/wgaead.h's new structs and constants as a C compiler lays them out, against _lib.py and the model."""
    fields = [("wg_hs_install_summary", "WgHsInstallSummary", ["n_ok", "n_badslot", "n_dup", "n_full"]),
              ("wg_hs_install_batch", "WgHsInstallBatch", ["entries", "n_entries", "send_slot", "recv_slot", "receivers",
                                                           "inst_status", "summary", "n", "n_slots", "slot_first", "slot_count",
                                                           "source", "flags"]),
              ("wg_hs_session", "WgHsSession", ["init", "local_index", "remote_index", "send_key", "recv_key"]),
              ("wg_hs_established", "WgHsEstablished", ["pending", "local_index", "remote_index", "send_key", "recv_key"])]
    consts = ["WG_HS_INST_OK", "WG_HS_INST_BADSLOT", "WG_HS_INST_DUPSLOT", "WG_HS_INST_DUPINDEX", "WG_HS_INST_FULL",
              "WG_HS_INSTALL_SESSIONS", "WG_HS_INSTALL_ESTABLISHED", "WG_HS_INSTALL_WIPE"]
    body = "".join(f'printf("%zu\\n", sizeof({c}));' + "".join(f'printf("%zu\\n", offsetof({c}, {f}));' for f in fs)
                   for c, _, fs in fields)
    body += "".join(f'printf("%u\\n", {c});' for c in consts)
    # n_ok, which the install reads as the entry count, is the first word of both summaries
    body += 'printf("%zu\\n", offsetof(wg_hs_respond_summary, n_ok)); printf("%zu\\n", offsetof(wg_hs_finish_summary, n_ok));'
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "wgaead.h"\n'
    src = tmp_path / "layout.c"
    src.write_text(head + "int main(void){" + body + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # the four prototypes, as the header declares them (compiled only: the pointer types must agree)
    proto = tmp_path / "proto.c"
    proto.write_text(head + "int (*a)(wg_ctx*, uint32_t) = wg_rx_sessions_reserve;\n"
                     "int (*b)(wg_ctx*, const uint32_t*, uint32_t, uint32_t*, void*) = wg_rx_sessions_retire;\n"
                     "int (*c)(wg_ctx*, uint32_t*, uint32_t*) = wg_rx_sessions_count;\n"
                     "int (*d)(wg_ctx*, const wg_hs_install_batch*, void*) = wg_hs_install;\n")
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
    assert ctypes.sizeof(L.WgHsInstallBatch) == 80 and ctypes.sizeof(L.WgHsInstallSummary) == 16
    assert want[-10:-2] == [IM.INST_OK, IM.INST_BADSLOT, IM.INST_DUPSLOT, IM.INST_DUPINDEX, IM.INST_FULL, IM.SRC_SESSIONS,
                         IM.SRC_ESTABLISHED, 1]
    assert W.WG_HS_SESSION_DTYPE == IM.HS_SESSION and W.WG_HS_ESTABLISHED_DTYPE == IM.HS_ESTABLISHED
    names = {name for name, _, _ in L.SIGNATURES}
    for f in ("wg_rx_sessions_reserve", "wg_rx_sessions_retire", "wg_rx_sessions_count", "wg_hs_install"):
        assert f in names and hasattr(W.lib(), f)
    for m in ("rx_sessions_reserve", "rx_sessions_retire", "rx_sessions_count", "hs_install"):
        assert callable(getattr(W.Engine, m))
