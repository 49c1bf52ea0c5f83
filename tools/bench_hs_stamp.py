"""Timing of wg_hs_stamp and of the chains around it on tools/bench_hs_open.py's two flood rings (65,536 type-1
datagrams of 148 B: `flood`, 1% genuine initiations, and `flood_all`, every one genuine; a pool of 24 (ephemeral,
initiator) pairs, four of the six initiators among 1,028 peers). Reports, after a 150-ms clock ramp, as the median
(min, max) of 20 calls after 5 warm-ups (HIP events on the launch stream), per ring:
  stamp_fresh_us            wg_hs_stamp alone over what plan + check + dh + open left, the stored stamps zeroed before
                            each call (outside the timed region): the newest initiation of each peer is OK
  stamp_replay_us           the same call again without the reset: every timestamp is stale
  plan_open_us              plan -> check -> dh -> open (the kernels the parent has: also measured with the parent's
                            library, WG_LIB_PATH, where the stamp rows are absent)
  plan_respond_us           plan -> ... -> open -> respond, the parent's responder: every known initiation is answered
                            every time (ephemerals refreshed before each call, outside the timed region)
  plan_stamp_respond_fresh_us / _replay_us
                            plan -> ... -> open -> stamp -> respond on a ring whose initiations are fresh (stamps zeroed
                            before each call) and on the same ring sent again
The pool has four known initiators, so a fresh ring has four OK entries: the stamp's cost is plan_stamp_respond minus
plan_respond's own parts, and what it saves on a replayed ring is the respond's ladders. Statuses, opened timestamps
and summaries are compared with the ring's make-up and tests/hs_stamp_model.py on a sample (`verified`). `--profile`
runs wg_hs_stamp on the flood_all ring 10 times (stamps zeroed in between) and nothing else, for a kernel-trace run
of its own; `--trace FILE.csv` turns that run's kernel trace into the median time per kernel. One JSON line each;
--out appends it to a file."""
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_hs_open as BO  # noqa: E402
from bench_tx import splitmix_np  # noqa: E402

KERNELS = ("k_hs_stamp_chain", "k_hs_stamp_hi", "k_hs_stamp_lo", "k_hs_stamp_j", "k_hs_stamp_commit", "k_hs_stamp_emit", "k_rx_scan")
PARENT_K_HS_OPEN_US = 84.9  # the parent's measured k_hs_open over 65,536 records: 28 compressions and one AEAD


def trace_summary(path):
    """Median / min per kernel over the last 10 calls of a rocprofv3 --kernel-trace CSV: the profile pass."""
    per = {}
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        k = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if k:
            per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v[-10:]), "median_us": round(float(np.median(v[-10:])), 2), "min_us": round(min(v[-10:]), 2)}
            for k, v in per.items()}


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        ks = trace_summary(p)
        out = {"kernel_trace": p.split("/")[-1], "kernels": ks}
        if "k_hs_stamp_chain" in ks:
            out["chain_over_parent_k_hs_open"] = round(ks["k_hs_stamp_chain"]["median_us"] / PARENT_K_HS_OPEN_US, 3)
        BO.emit(out)
        return
    import importlib
    import torch
    assert torch.cuda.is_available(), "bench_hs_stamp needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    probe = ctypes.CDLL(W._lib.LIB_PATH)
    have = hasattr(probe, "wg_hs_stamp")
    if not have:  # an earlier library (WG_LIB_PATH): bind what it exports, measure what it has
        W._lib.SIGNATURES[:] = [s for s in W._lib.SIGNATURES if hasattr(probe, s[0])]
    dev = torch.device("cuda", 0)
    n, K, max_len = 65536, 256, 1500
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    pub = eng.hs_static_set(BO.PRIVATE)
    bodies, ipubs = BO.pool(pub)
    peers = [bytes(splitmix_np(0x6300 + k, 32)) for k in range(BO.PEERS)] + ipubs[:4]
    eng.hs_peers_set(peers)
    eng.rx_reserve(n)
    if have:
        eng.hs_stamps_set(0, [])
    eng.hs_reserve(n)
    rings = {name: BO.flood(n, pub, bodies, every) for name, every in (("flood", False), ("flood_all", True))}
    dv = {name: (torch.from_numpy(r).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(ln).to(dev))
          for name, (r, o, ln, _) in rings.items()}
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st, d_st, o_st, s_st, p_st = (i32(n) for _ in range(7))
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_sum, o_sum, s_sum, p_sum = (i32(4) for _ in range(4))
    h_rec, shared, o_init, s_fresh, s_op, sess = u8(n, 160), u8(n, 32), u8(n, 144), u8(n, 144), u8(12 * n), u8(n, 176)
    eph0 = torch.from_numpy(splitmix_np(0x6400, 32 * n)).to(dev)
    eph = eph0.clone()
    li = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    zero_stamps = bytes(12 * len(peers))

    def plan_open(name):
        w, o, ln = dv[name]
        eng.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)
        eng.hs_dh(h_rec, h_sum, shared, d_st)
        eng.hs_open(h_rec, h_sum, shared, d_st, o_st, o_init, o_sum)

    def stamp():
        eng.hs_stamp(o_init, o_sum, h_rec, shared, s_st, s_op, s_fresh, s_sum)

    def plan_respond(name):
        plan_open(name)
        eng.hs_respond(o_init, o_sum, eph, li, p_st, sess, p_sum)

    def plan_stamp_respond(name):
        plan_open(name)
        stamp()
        eng.hs_respond(s_fresh, s_sum, eph, li, p_st, sess, p_sum)

    def fresh():
        eng.hs_stamps_set(0, zero_stamps)

    def new_eph():
        eph.copy_(eph0)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        plan_open("flood")
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        plan_open("flood_all")
        for _ in range(10):
            fresh()
            stamp()
            torch.cuda.synchronize()
        BO.emit({"profile_pass": 10, "n": n})
        eng.close()
        return

    def timed(f, before=None, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for k in range(warm + reps):
            if before:
                before()
                torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b) * 1e3)
        return [round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)]

    out = {"n": n, "peers": len(peers), "version": W.lib().wg_version().decode(), "lib": os.path.basename(W._lib.LIB_PATH),
           "has_stamp": have}
    verified = True
    pool_ts = [bytes(splitmix_np(0x6200 + k, 12)) for k in range(BO.POOL)]
    for name in ("flood", "flood_all"):
        res = {}
        res["plan_open_us"] = timed(lambda: plan_open(name))
        res["plan_respond_us"] = timed(lambda: plan_respond(name), before=new_eph)
        res["respond_n_ok"] = int(p_sum.cpu().numpy()[0])
        if have:
            plan_open(name)  # (leaves this ring's entries for the stamp alone)
            res["stamp_fresh_us"] = timed(stamp, before=fresh)
            torch.cuda.synchronize()
            sm = [int(x) for x in s_sum.cpu().numpy()]
            ne = int(o_sum.cpu().numpy()[0])
            st = s_st[:ne].cpu().numpy()
            ent = o_init[:ne].cpu().numpy().reshape(-1).view(W.WG_HS_INIT_DTYPE)
            opened = s_op[:12 * ne].cpu().numpy().reshape(ne, 12)
            known = ent["peer"] != W._lib.WG_HS_NOPEER
            # every entry's datagram names its pool entry; the four known initiators are peers 1,024 .. 1,027
            k_of = ent["index"] % BO.POOL
            verified &= sm == [4, int(known.sum()) - 4, 0, int((~known).sum())] and sm[0] + sm[1] + sm[3] == ne
            verified &= bool((st[~known] == W._lib.WG_HS_TS_NOPEER).all()) and not opened[~known].any()
            verified &= all(opened[j].tobytes() == pool_ts[int(k_of[j])] for j in np.nonzero(known)[0][:64])
            best = {}  # per peer: the greatest timestamp's first entry
            for j in np.nonzero(known)[0]:
                t, p = pool_ts[int(k_of[j])], int(ent["peer"][j])
                if p not in best or t > best[p][0]:
                    best[p] = (t, int(j))
            verified &= sorted(int(j) for j in np.nonzero(st == W._lib.WG_HS_TS_OK)[0]) == sorted(j for _, j in best.values())
            verified &= eng.hs_stamps_get(BO.PEERS, 4) == [best[BO.PEERS + i][0] for i in range(4)]
            res["stamp_summary_fresh"] = sm
            res["stamp_replay_us"] = timed(stamp)
            sm2 = [int(x) for x in s_sum.cpu().numpy()]
            verified &= sm2 == [0, sm[0] + sm[1], 0, sm[3]]
            res["plan_stamp_respond_fresh_us"] = timed(lambda: plan_stamp_respond(name), before=lambda: (fresh(), new_eph()))
            verified &= int(p_sum.cpu().numpy()[0]) == 4
            res["plan_stamp_respond_replay_us"] = timed(lambda: plan_stamp_respond(name), before=new_eph)
            verified &= int(p_sum.cpu().numpy()[0]) == 0 and bool((eph == eph0).all())
            res["stamp_over_parent_k_hs_open"] = round(res["stamp_fresh_us"][0] / PARENT_K_HS_OPEN_US, 3)
        out[name] = res
    out["verified"] = bool(verified)
    BO.emit(out)
    eng.close()


if __name__ == "__main__":
    main()
