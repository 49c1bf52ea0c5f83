"""Timing of wg_x25519_batch and of the plan -> check -> dh chain (wg_rx_plan, wg_hs_check, wg_hs_dh).
Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch
stream):
  x25519_us[n]             wg_x25519_batch over n random (scalar, point) pairs, n = 256, 4,096, 65,536 (one
                           wave per SIMD of the MI355X) and 262,144 (four, what the kernel's registers allow)
  x25519_dh_per_s[n]       n over that time
  dh_flood_us              wg_hs_dh alone over the records of tools/bench_hs.py's flood ring (65,536 type-1
                           datagrams of 148 B, 1% with a correct mac1), made for the public key that
                           wg_hs_static_set returned
  plan_check_dh_flood_us   plan + check + dh in one region on that ring (no host read in between)
  dh_flood_all_us, plan_check_dh_flood_all_us
                           the same on a flood ring in which every datagram carries a correct mac1: what a
                           sender who knows the static public key can produce
Every timed output is compared with the big-integer model of tests/x25519_model.py on a sample of operands
(`verified`). `python_model_us_per_op` is that pure-Python model timed on 64 operands: a model, not a
baseline. `--profile` runs wg_x25519_batch at 65,536 and wg_hs_dh on the all-good flood ring 10 times each
and nothing else, for a kernel-trace or a counter run of its own; `--trace FILE.csv` turns that run's
kernel trace into the median time per kernel, `--counters FILE.csv` a counter run (SQ_WAVES SQ_INSTS_VALU)
into VALU instructions per wave. One JSON line each; --out appends it to a file."""
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

KERNELS = ("k_x25519", "k_hs_dh", "k_hs_check", "k_rx_scan", "k_hs_emit", "k_rx_plan")
PRIVATE = bytes(splitmix_np(0x5853, 32))


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
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v[-10:]), "median_us": round(float(np.median(v[-10:])), 2), "min_us": round(min(v[-10:]), 2)}
            for k, v in per.items()}


def counter_summary(path):
    """Per kernel, over its dispatches of the largest grid (the profile pass, not the clock ramp) in a
    rocprofv3 --pmc CSV: waves per dispatch and VALU instructions per wave (SQ_INSTS_VALU / SQ_WAVES)."""
    per = {}
    for r in csv.DictReader(open(path)):
        for k in ("k_x25519", "k_hs_dh"):
            if k in r["Kernel_Name"]:
                d = per.setdefault(k, {}).setdefault(r["Dispatch_Id"], {"grid": int(r["Grid_Size"])})
                d[r["Counter_Name"]] = float(r["Counter_Value"])
    out = {}
    for k, disp in per.items():
        grid = max(d["grid"] for d in disp.values())
        ds = [d for d in disp.values() if d["grid"] == grid]
        waves = sum(d.get("SQ_WAVES", 0.0) for d in ds)
        out[k] = {"grid": grid, "dispatches": len(ds), "waves_per_dispatch": round(waves / len(ds), 1),
                  "valu_per_wave": round(sum(d.get("SQ_INSTS_VALU", 0.0) for d in ds) / waves) if waves else None}
    return out


def flood(n, pub, every):
    """bench_hs.flood_ring made for `pub`; every: all n datagrams carry a correct mac1, not 1%."""
    bench_hs.PUB = pub
    ring, off, lens, good = bench_hs.flood_ring(n)
    if every:
        msgs = ring.reshape(n, 148)
        for i in range(n):
            msgs[i] = np.frombuffer(bench_hs.with_mac1(msgs[i, :116].tobytes()), np.uint8)
        good = n
    return ring, off, lens, good


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return
    if "--counters" in sys.argv:
        p = sys.argv[sys.argv.index("--counters") + 1]
        emit({"counters": p.split("/")[-1], "kernels": counter_summary(p)})
        return
    import importlib
    import torch
    import x25519_model as M
    assert torch.cuda.is_available(), "bench_x25519 needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, max_len = 65536, 256, 1500
    sizes, nx = (256, 4096, 65536, 262144), 262144
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    pub = eng.hs_static_set(PRIVATE)
    eng.rx_reserve(n)
    eng.hs_reserve(n)
    # wg_x25519_batch: random operands, scalar and point side by side
    x_host = splitmix_np(41, 64 * nx)
    x_in = torch.from_numpy(x_host).to(dev)
    at = 64 * np.arange(nx, dtype=np.uint64)
    x_desc = torch.from_numpy(W.desc_as_int64(W.pack_x25519_desc(at, at + np.uint64(32), at // np.uint64(2))).copy()).to(dev)
    x_out = torch.zeros(32 * nx, dtype=torch.uint8, device=dev)
    x_st = torch.zeros(nx, dtype=torch.int32, device=dev)
    rings = {name: flood(n, pub, every) for name, every in (("flood", False), ("flood_all", True))}
    dv = {name: (torch.from_numpy(r).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(ln).to(dev))
          for name, (r, o, ln, _) in rings.items()}
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st, d_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
    h_sum = torch.zeros(4, dtype=torch.int32, device=dev)
    shared = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

    def x25519(m):
        eng.x25519(x_desc[:m], x_in, x_out, x_st[:m])

    def plan_check(name):
        w, o, ln = dv[name]
        eng.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)

    def dh():
        eng.hs_dh(h_rec, h_sum, shared, d_st)

    def plan_check_dh(name):
        plan_check(name)
        dh()

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        x25519(4096)
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        plan_check("flood_all")
        for _ in range(10):
            x25519(n)
            dh()
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

    out = {"n": n, "version": W.lib().wg_version().decode(), "x25519_us": {}, "x25519_spread_us": {}, "x25519_dh_per_s": {}}
    verified = True
    for m in sizes:
        med, lo, hi = timed(lambda: x25519(m))
        out["x25519_us"][str(m)] = med
        out["x25519_spread_us"][str(m)] = [lo, hi]
        out["x25519_dh_per_s"][str(m)] = round(m / med * 1e6)
    got = x_out.cpu().numpy()
    for i in (0, 1, 255, 4095, 65535, 65536, nx - 1):
        want = M.x25519(x_host[64 * i:64 * i + 32].tobytes(), x_host[64 * i + 32:64 * i + 64].tobytes())
        verified &= got[32 * i:32 * i + 32].tobytes() == want
    verified &= int(x_st.abs().sum().item()) == 0
    for name in ("flood", "flood_all"):
        plan_check(name)  # (leaves this ring's records for the dh alone)
        out[f"dh_{name}_us"] = timed(dh)[0]
        out[f"plan_check_{name}_us"] = timed(lambda: plan_check(name))[0]
        out[f"plan_check_dh_{name}_us"] = timed(lambda: plan_check_dh(name))[0]
        torch.cuda.synchronize()
        nv = int(h_sum.cpu().numpy()[0])
        out[f"{name}_n_valid"] = nv
        verified &= nv == rings[name][3]
        rec, sh, st = h_rec[:nv].cpu().numpy(), shared[:nv].cpu().numpy(), d_st[:nv].cpu().numpy()
        for k in (0, nv // 2, nv - 1):
            verified &= sh[k].tobytes() == M.x25519(PRIVATE, rec[k, 16:48].tobytes()) and int(st[k]) == 0
        out[f"dh_{name}_per_s"] = round(nv / out[f"dh_{name}_us"] * 1e6)
    out["verified"] = bool(verified)
    ops = [(x_host[64 * i:64 * i + 32].tobytes(), x_host[64 * i + 32:64 * i + 64].tobytes()) for i in range(64)]
    t = time.perf_counter()
    for k, u in ops:
        M.x25519(k, u)
    out["python_model_us_per_op"] = round((time.perf_counter() - t) / 64 * 1e6, 1)
    emit(out)
    eng.close()


if __name__ == "__main__":
    main()
