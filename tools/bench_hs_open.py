"""Timing of wg_hs_open and of the plan -> check -> dh -> open chain (wg_rx_plan, wg_hs_check, wg_hs_dh,
wg_hs_open) on tools/bench_hs.py's flood ring (65,536 type-1 datagrams of 148 B), now made of genuine
initiations: `flood`, in which the 1% of datagrams with a correct mac1 are genuine (the rest never reach the
open), and `flood_all`, in which every datagram is. The genuine initiations repeat a pool of 24 (ephemeral,
initiator) pairs with their own sender indices: the device does the same work for each, and the host makes the
ring in a second. Four of the pool's six initiators are peers, among 1,024 random keys. Reports, after a 150-ms
clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch stream), per ring:
  open_us                   wg_hs_open alone over the records and secrets that plan + check + dh left
  plan_check_dh_us          the chain without the open, in one region
  plan_check_dh_open_us     the chain with it (no host read in between)
  d2h_bytes_device          16 + 144 n_emitted: what the host fetches after the open
  d2h_bytes_host            16 + (160 + 32 + 4) n_valid: records, secrets and statuses, which the host fetches
                            to run decryptRemoteStatic itself
Every timed output is compared with tests/hs_open_model.py on a sample of records, and the summary with the
ring's make-up (`verified`). `--profile` runs wg_hs_open on the flood_all ring 10 times and nothing else, for a
kernel-trace run of its own; `--trace FILE.csv` turns that run's kernel trace into the median time per kernel.
One JSON line each; --out appends it to a file."""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_hs  # noqa: E402
from bench_tx import splitmix_np  # noqa: E402

KERNELS = ("k_hs_open_emit", "k_hs_open", "k_rx_scan")
PRIVATE = bytes(splitmix_np(0x5853, 32))
POOL, INITIATORS, PEERS = 24, 6, 1024


def emit(out):
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")


def trace_summary(path):
    """Median / min per kernel over the last 10 calls of a rocprofv3 --kernel-trace CSV: the profile pass."""
    per = {}
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        k = next((k for k in KERNELS if k in r["Kernel_Name"]), None)  # (k_hs_open_emit before its prefix k_hs_open)
        if k:
            per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v[-10:]), "median_us": round(float(np.median(v[-10:])), 2), "min_us": round(min(v[-10:]), 2)}
            for k, v in per.items()}


def pool(pub):
    """The 24 genuine initiations to `pub` (msg[8 .. 116) each) and the initiators' public keys."""
    import hs_open_model as OM
    import x25519_model as M
    inits = [bytes(splitmix_np(0x6100 + j, 32)) for j in range(INITIATORS)]
    bodies = []
    for k in range(POOL):
        h = OM.initiate(inits[k % INITIATORS], pub, bytes(splitmix_np(0x6000 + k, 32)), bytes(splitmix_np(0x6200 + k, 12)))
        bodies.append(h["ephemeral"] + h["encrypted_static"] + h["encrypted_timestamp"])
    return bodies, [M.public_key(k) for k in inits]


def flood(n, pub, bodies, every):
    """bench_hs.flood_ring made for `pub`; the datagrams with a correct mac1 (every: all n) are genuine."""
    bench_hs.PUB = pub
    ring, off, lens, good = bench_hs.flood_ring(n)
    msgs = ring.reshape(n, 148)
    pick = range(n) if every else np.nonzero(splitmix_np(22, 4 * n).view("<u4") % 100 == 0)[0]
    for i in pick:
        msgs[i, 8:116] = np.frombuffer(bodies[i % POOL], np.uint8)
        msgs[i] = np.frombuffer(bench_hs.with_mac1(msgs[i, :116].tobytes()), np.uint8)
    return ring, off, lens, len(pick)


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return
    import importlib
    import torch
    import hs_open_model as OM
    assert torch.cuda.is_available(), "bench_hs_open needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, max_len = 65536, 256, 1500
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    pub = eng.hs_static_set(PRIVATE)
    bodies, ipubs = pool(pub)
    peers = [bytes(splitmix_np(0x6300 + k, 32)) for k in range(PEERS)] + ipubs[:4]
    eng.hs_peers_set(peers)
    eng.rx_reserve(n)
    eng.hs_reserve(n)
    rings = {name: flood(n, pub, bodies, every) for name, every in (("flood", False), ("flood_all", True))}
    dv = {name: (torch.from_numpy(r).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(ln).to(dev))
          for name, (r, o, ln, _) in rings.items()}
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st, d_st, o_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5))
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
    h_sum, o_sum = (torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(2))
    shared = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    o_init = torch.zeros((n, 144), dtype=torch.uint8, device=dev)

    def plan_check_dh(name):
        w, o, ln = dv[name]
        eng.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)
        eng.hs_dh(h_rec, h_sum, shared, d_st)

    def hs_open():
        eng.hs_open(h_rec, h_sum, shared, d_st, o_st, o_init, o_sum)

    def chain(name):
        plan_check_dh(name)
        hs_open()

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        chain("flood")
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        plan_check_dh("flood_all")
        for _ in range(10):
            hs_open()
            torch.cuda.synchronize()
        emit({"profile_pass": 10, "n": n})
        eng.close()
        return

    def timed(f, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for k in range(warm + reps):
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)

    out = {"n": n, "peers": len(peers), "version": W.lib().wg_version().decode()}
    verified = True
    for name in ("flood", "flood_all"):
        res = {}
        plan_check_dh(name)  # (leaves this ring's records and secrets for the open alone)
        res["open_us"], *res["open_spread_us"] = timed(hs_open)
        res["plan_check_dh_us"], *res["plan_check_dh_spread_us"] = timed(lambda: plan_check_dh(name))
        res["plan_check_dh_open_us"], *res["plan_check_dh_open_spread_us"] = timed(lambda: chain(name))
        torch.cuda.synchronize()
        nv = int(h_sum.cpu().numpy()[0])
        sm = [int(x) for x in o_sum.cpu().numpy()]
        res.update(n_valid=nv, n_emitted=sm[0], n_known=sm[1], n_badauth=sm[2], n_skipped=sm[3])
        res["open_fraction_of_chain"] = round(res["open_us"] / res["plan_check_dh_open_us"], 4)
        res["d2h_bytes_device"] = 16 + 144 * sm[0]
        res["d2h_bytes_host"] = 16 + (160 + 32 + 4) * nv
        genuine = rings[name][3]
        verified &= nv == genuine and sm[0] == genuine and sm[2] == 0 and sm[3] == 0
        rec, sh = h_rec[:nv].cpu().numpy(), shared[:nv].cpu().numpy()
        ent = o_init[:sm[0]].cpu().numpy().reshape(-1).view(W.WG_HS_INIT_DTYPE)
        index = np.ascontiguousarray(rec[:, :4]).view("<u4").reshape(-1)  # the datagram: its pool entry's initiator
        verified &= sm[1] == int((index % POOL % INITIATORS < 4).sum())
        for k in (0, nv // 2, nv - 1):
            m = rec[k, 8:156].tobytes()
            st, want = OM.open_one(PRIVATE, pub, m[8:40], m[40:88], m[88:116], sh[k].tobytes(), peers)
            e = ent[k]  # (every record is emitted: entry k is record k's)
            verified &= st in (OM.OPEN_OK, OM.OPEN_NEWPEER) and int(e["record"]) == k and int(e["peer"]) == want["peer"]
            verified &= all(e[f].tobytes() == want[f] for f in ("remote_static", "hash", "chain_key"))
        out[name] = res
    out["verified"] = bool(verified)
    emit(out)
    eng.close()


if __name__ == "__main__":
    main()
