"""Timing of wg_hs_respond and of the plan -> check -> dh -> open -> respond chain on tools/bench_hs_open.py's flood
rings (65,536 type-1 datagrams of 148 B): `flood`, in which the 616 datagrams with a correct mac1 are genuine
initiations, and `flood_all`, in which every datagram is. Here all six initiators of the pool are peers, so every
authentic initiation is answered. Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups
(HIP events on the launch stream; the ephemerals are refreshed from a device copy before each timed call, outside
the timed region), per ring:
  respond_us                  wg_hs_respond alone over the entries that plan + check + dh + open left
  dh_us                       wg_hs_dh alone over the same ring's records, in the same run: one ladder per record,
                              against the respond's three per entry
  plan_check_dh_open_us       the four earlier stages in one region
  chain5_us                   the five stages in one region (no host read in between)
  d2h_bytes_device            16 + 176 n_ok: what the host fetches after the respond
  d2h_bytes_host              16 + 144 n_emitted: the entries, which the host fetches to run deriveKeypair itself
Sessions are compared with tests/hs_respond_model.py on a sample, and the summary with the ring's make-up
(`verified`). `--ab OTHER_LIB` first times plan + check + dh + open in fresh child processes, alternately under
OTHER_LIB (the parent commit's library) and under this one, twice each: the earlier stages must cost what they did.
`--chain4` is that child's mode. `--profile` runs wg_hs_respond on the flood_all ring 10 times and nothing else, for
a kernel-trace run of its own; `--trace FILE.csv` turns that run's kernel trace into the median time per kernel.
One JSON line each; --out appends it to a file."""
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_hs_open as BO  # noqa: E402
from bench_tx import splitmix_np  # noqa: E402

KERNELS = ("k_hs_resp_dh", "k_hs_resp_chain", "k_hs_resp_emit", "k_rx_scan")


def emit(out):
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")


def trace_summary(path):
    """Median / min per kernel over the last 10 calls of a rocprofv3 --kernel-trace CSV: the profile pass."""
    per = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        k = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if k:
            per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v[-10:]), "median_us": round(float(np.median(v[-10:])), 2), "min_us": round(min(v[-10:]), 2)}
            for k, v in per.items()}


def ab(other):
    """plan + check + dh + open in fresh processes, other / this / other / this."""
    runs = []
    for k in range(4):
        env = dict(os.environ)
        if k % 2 == 0:
            env["WG_LIB_PATH"] = os.path.abspath(other)
        else:
            env.pop("WG_LIB_PATH", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--chain4"], env=env, stdout=subprocess.PIPE, timeout=240)
        if p.returncode != 0:
            raise SystemExit(f"--chain4 under {'the other' if k % 2 == 0 else 'this'} library ended with {p.returncode}")
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        r["library"] = "other" if k % 2 == 0 else "this"
        runs.append(r)
    return runs


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return
    ab_runs = ab(sys.argv[sys.argv.index("--ab") + 1]) if "--ab" in sys.argv else None  # (before this process opens the GPU)
    import importlib
    import torch
    assert torch.cuda.is_available(), "bench_hs_respond needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    if "--chain4" in sys.argv:  # the other library may lack this stage's symbol: bind what it has
        import ctypes
        have = ctypes.CDLL(W._lib.LIB_PATH)
        W._lib.SIGNATURES[:] = [sig for sig in W._lib.SIGNATURES if hasattr(have, sig[0])]
    dev = torch.device("cuda", 0)
    n, K, max_len = 65536, 256, 1500
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    pub = eng.hs_static_set(BO.PRIVATE)
    bodies, ipubs = BO.pool(pub)
    peers = [bytes(splitmix_np(0x6300 + k, 32)) for k in range(BO.PEERS)] + ipubs
    eng.hs_peers_set(peers)
    eng.rx_reserve(n)
    eng.hs_reserve(n)
    rings = {name: BO.flood(n, pub, bodies, every) for name, every in (("flood", False), ("flood_all", True))}
    dv = {name: (torch.from_numpy(r).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(ln).to(dev))
          for name, (r, o, ln, _) in rings.items()}
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st, d_st, o_st, s_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(6))
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
    h_sum, o_sum, s_sum = (torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(3))
    shared = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    o_init = torch.zeros((n, 144), dtype=torch.uint8, device=dev)

    def plan_check_dh(name):
        w, o, ln = dv[name]
        eng.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)
        eng.hs_dh(h_rec, h_sum, shared, d_st)

    def chain4(name):
        plan_check_dh(name)
        eng.hs_open(h_rec, h_sum, shared, d_st, o_st, o_init, o_sum)

    def timed(f, before=None, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for k in range(warm + reps):
            if before:
                before()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        chain4("flood")
        torch.cuda.synchronize()
    version = W.lib().wg_version().decode()
    if "--chain4" in sys.argv:
        out = {"chain4": True, "n": n, "version": version}
        for name in ("flood", "flood_all"):
            out[name + "_plan_check_dh_open_us"], *out[name + "_spread_us"] = timed(lambda: chain4(name))
        print(json.dumps(out))
        eng.close()
        return

    eph_host = splitmix_np(0x6400, 32 * n)
    eph_master = torch.from_numpy(eph_host).to(dev)
    eph = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    li_host = (np.arange(n, dtype=np.uint32) * np.uint32(40503) + np.uint32(0x01000000)).astype(np.uint32)
    li = torch.from_numpy(li_host.view(np.int32)).to(dev)
    sess = torch.zeros((n, 176), dtype=torch.uint8, device=dev)

    def refresh():
        eph.copy_(eph_master)

    def respond():
        eng.hs_respond(o_init, o_sum, eph, li, s_st, sess, s_sum, skip_newpeer=True)

    def chain5(name):
        chain4(name)
        respond()

    if "--profile" in sys.argv:
        chain4("flood_all")
        for _ in range(10):
            refresh()
            respond()
            torch.cuda.synchronize()
        emit({"profile_pass": 10, "n": n})
        eng.close()
        return

    import hs_respond_model as RM
    out = {"n": n, "peers": len(peers), "version": version}
    if ab_runs is not None:
        out["plan_check_dh_open_ab"] = ab_runs
    verified = True
    for name in ("flood", "flood_all"):
        res = {}
        chain4(name)  # (leaves this ring's entries for the respond alone)
        res["respond_us"], *res["respond_spread_us"] = timed(respond, refresh)
        res["dh_us"], *res["dh_spread_us"] = timed(lambda: eng.hs_dh(h_rec, h_sum, shared, d_st))
        res["plan_check_dh_open_us"], *res["plan_check_dh_open_spread_us"] = timed(lambda: chain4(name))
        res["chain5_us"], *res["chain5_spread_us"] = timed(lambda: chain5(name), refresh)
        torch.cuda.synchronize()
        om = [int(x) for x in o_sum.cpu().numpy()]
        sm = [int(x) for x in s_sum.cpu().numpy()]
        res.update(n_emitted=om[0], n_ok=sm[0], n_nopeer=sm[1], n_noeph=sm[2])
        res["respond_over_dh"] = round(res["respond_us"] / res["dh_us"], 3)
        res["d2h_bytes_device"] = 16 + 176 * sm[0]
        res["d2h_bytes_host"] = 16 + 144 * om[0]
        genuine = rings[name][3]
        verified &= om[0] == genuine and sm == [genuine, 0, 0, 0]
        verified &= not bool(eph[:32 * genuine].any().item()) and bool((eph[32 * genuine:] == eph_master[32 * genuine:]).all().item())
        ent = o_init[:om[0]].cpu().numpy().reshape(-1).view(W.WG_HS_INIT_DTYPE)
        got = sess[:sm[0]].cpu().numpy().reshape(-1).view(W.WG_HS_SESSION_DTYPE)
        for k in (0, genuine // 2, genuine - 1):
            e, s = ent[k], got[k]  # (every entry is answered: session k is entry k's)
            want = RM.respond_one(e["hash"].tobytes(), e["chain_key"].tobytes(), e["remote_ephemeral"].tobytes(),
                                  e["remote_static"].tobytes(), eph_host[32 * k:32 * k + 32].tobytes(), int(li_host[k]),
                                  int(e["sender_index"]))
            verified &= int(s["init"]) == k and int(s["index"]) == int(e["index"]) and int(s["local_index"]) == int(li_host[k])
            verified &= all(s[f].tobytes() == want[f] for f in ("response", "send_key", "recv_key"))
        out[name] = res
    out["verified"] = bool(verified)
    emit(out)
    eng.close()


if __name__ == "__main__":
    main()
