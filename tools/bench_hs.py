"""Timing of the handshake admission check (wg_hs_check) and of wg_blake2s_batch on two rings:
  flood  65,536 type-1 datagrams of 148 B, back to back; 1% carry a correct mac1 (mac2 zero in all);
  mixed  the IMIX wire ring of tools/bench_rx_plan.py in shape (65,536 slots of 1,536 B, 40 / 576 / 1500 B
         at 7 : 4 : 1, 256 sessions) with 1.2% of the slots holding handshake messages (half of them with
         a correct mac1). The transport packets carry random bytes behind a valid header: the plan and
         the check read headers and handshake messages only.
Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch
stream):
  check_flood_us        wg_hs_check alone, identity list, flood ring
  check_mixed_us        wg_hs_check alone on the mixed ring, given the list a plan left
  plan_mixed_us         wg_rx_plan alone on the mixed ring
  plan_check_mixed_us   plan + check in one region (no host read in between)
  plan_check_flood_us   the same on the flood ring (the plan lists every datagram)
  b2s_us                wg_blake2s_batch, 65,536 x 116-B messages under one 32-B key, 16-B digests
and, as an alternating A/B of wall time (call to result on the host, median of 20 pairs, the order
swapped every pair), per ring:
  ab_device_wall_us  plan + check, the 16-B summary copied back, then 160 n_valid bytes of records
  ab_host_wall_us    the way without the check: plan, the plan's summary and host_list[0 .. n_host) copied
                     back, the listed datagrams fetched from the device ring (one copy of the whole ring
                     when the list covers more than an eighth of its bytes, else one copy per datagram),
                     then type, length, hashlib.blake2s mac1 and mac2 per message in a Python loop. This is a
                     stand-in for a per-packet host loop, not a tuned figure.
  d2h_bytes_device / d2h_bytes_host  what each way copies back
Both ways must accept the same datagrams (checked once). `--profile flood|mixed` runs the check 25 times
on that ring (and wg_blake2s_batch 25 times) and nothing else, for a kernel-trace run of its own;
`--trace FILE.csv` turns that run's kernel trace into the median time per kernel. One JSON line each;
--out appends it to a file."""
import csv
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tx import splitmix_np  # noqa: E402

PUB = bytes(splitmix_np(0x4853, 32))


def emit(out):
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")


def trace_summary(path):
    """Median / min per kernel over the last 25 calls of a rocprofv3 --kernel-trace CSV: the profile pass
    (the calls before it are the clock ramp on the mixed ring)."""
    per = {}
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        for k in ("k_hs_check", "k_rx_scan", "k_hs_emit", "k_b2s"):
            if k in name:
                per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v[-25:]), "median_us": round(float(np.median(v[-25:])), 2), "min_us": round(min(v[-25:]), 2)}
            for k, v in per.items()}


def mac1_key():
    return hashlib.blake2s(b"mac1----" + PUB).digest()


def with_mac1(head: bytes) -> bytes:
    return head + hashlib.blake2s(head, digest_size=16, key=mac1_key()).digest() + bytes(16)


def flood_ring(n):
    msgs = splitmix_np(21, n * 148).reshape(n, 148).copy()
    msgs[:, 0] = 1
    msgs[:, 132:] = 0
    good = np.nonzero(splitmix_np(22, 4 * n).view("<u4") % 100 == 0)[0]
    for i in good:
        msgs[i] = np.frombuffer(with_mac1(msgs[i, :116].tobytes()), np.uint8)
    return msgs.reshape(-1), np.arange(n, dtype=np.int64) * 148, np.full(n, 148, np.int32), len(good)


def mixed_ring(n, K, stride, receivers):
    u = splitmix_np(0x5EED2026, 4 * n).view("<u4") % 12
    lens = np.where(u < 7, 40, np.where(u < 11, 576, 1500)).astype(np.int64)
    ring = splitmix_np(23, n * stride)
    off = np.arange(n, dtype=np.int64) * stride
    slot = splitmix_np(11, n).astype(np.int64) % K
    ring[off] = 4
    for k in range(4):
        ring[off + 4 + k] = ((receivers[slot] >> (8 * k)) & 0xFF).astype(np.uint8)
    w_len = (lens + 32).astype(np.int32)
    pick = np.nonzero(splitmix_np(13, n) < 3)[0]  # about 1.2%
    n_good = 0
    for k, j in enumerate(pick):
        t = 1 + (k >> 1) % 2
        L = 148 if t == 1 else 92
        o = int(j) * stride
        ring[o] = t
        if k % 2 == 0:
            ring[o:o + L] = np.frombuffer(with_mac1(ring[o:o + L - 32].tobytes()), np.uint8)
            n_good += 1
        else:
            ring[o + L - 16:o + L] = 0
        w_len[j] = L
    return ring, off, w_len, len(pick), n_good


def main():
    if "--trace" in sys.argv:
        emit({"kernel_trace": sys.argv[sys.argv.index("--trace") + 1].split("/")[-1],
              "ring": sys.argv[sys.argv.index("--ring") + 1] if "--ring" in sys.argv else None,
              "kernels": trace_summary(sys.argv[sys.argv.index("--trace") + 1])})
        return
    import importlib
    import torch
    torch.cuda.is_available()
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, stride, max_len = 65536, 256, 1536, 1500
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    eng.hs_key_set(PUB)
    eng.rx_reserve(n)
    eng.hs_reserve(n)
    rings = {}
    f_ring, f_off, f_len, f_good = flood_ring(n)
    rings["flood"] = (f_ring, f_off, f_len)
    m_ring, m_off, m_len, m_hs, m_good = mixed_ring(n, K, stride, receivers)
    rings["mixed"] = (m_ring, m_off, m_len)
    dv = {name: (torch.from_numpy(r).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(ln).to(dev))
          for name, (r, o, ln) in rings.items()}
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
    h_sum = torch.zeros(4, dtype=torch.int32, device=dev)
    # wg_blake2s_batch: 65,536 x 116 B under one key
    b_in = torch.from_numpy(np.concatenate([splitmix_np(31, n * 116), np.frombuffer(mac1_key(), np.uint8)])).to(dev)
    b_desc = torch.from_numpy(W.desc_as_int64(W.pack_b2s_desc(np.arange(n, dtype=np.uint64) * 116,
                                                             np.arange(n, dtype=np.uint64) * 16,
                                                             np.full(n, n * 116, np.uint64), 116, 16, 32)).copy()).to(dev)
    b_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    b_st = torch.zeros(n, dtype=torch.int32, device=dev)

    def plan(name):
        w, o, ln = dv[name]
        eng.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)

    def check_list(name):
        w, o, ln = dv[name]
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)

    def check_identity(name):
        w, o, ln = dv[name]
        eng.hs_check(w, o, ln, h_st, h_rec, h_sum)

    def plan_check(name):
        plan(name)
        check_list(name)

    def b2s():
        eng.blake2s(b_desc, b_in, b_out, b_st)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        plan_check("mixed")
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        name = sys.argv[sys.argv.index("--profile") + 1]
        plan(name)
        for _ in range(25):
            check_list(name)
            b2s()
            torch.cuda.synchronize()
        emit({"profile_pass": 25, "ring": name})
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
        return round(float(np.median(ts)), 2)

    out = {"n": n, "flood_good": int(f_good), "mixed_handshakes": int(m_hs), "mixed_good": int(m_good),
           "mixed_stride": stride}
    out["check_flood_us"] = timed(lambda: check_identity("flood"))
    out["plan_mixed_us"] = timed(lambda: plan("mixed"))  # (leaves the mixed ring's list for the check below)
    out["check_mixed_us"] = timed(lambda: check_list("mixed"))
    out["plan_check_mixed_us"] = timed(lambda: plan_check("mixed"))
    out["plan_check_flood_us"] = timed(lambda: plan_check("flood"))
    out["b2s_us"] = timed(b2s)
    torch.cuda.synchronize()
    ref = hashlib.blake2s(b_in[:116].cpu().numpy().tobytes(), digest_size=16, key=mac1_key()).digest()
    out["b2s_verified"] = bool(b_out[:16].cpu().numpy().tobytes() == ref and int(b_st.sum()) == 0)
    out["b2s_gb_per_s"] = round(n * 116 / out["b2s_us"] / 1e3, 2)

    # ---- the two ways, wall time
    p_sum = torch.zeros(2, dtype=torch.int64).pin_memory()
    p_host = torch.zeros(n, dtype=torch.int32).pin_memory()
    p_hsum = torch.zeros(4, dtype=torch.int32).pin_memory()
    p_rec = torch.zeros((n, 160), dtype=torch.uint8).pin_memory()
    p_ring = {name: torch.zeros(len(rings[name][0]), dtype=torch.uint8).pin_memory() for name in rings}
    p_msg = torch.zeros(148, dtype=torch.uint8).pin_memory()
    key = mac1_key()
    res = {}

    def device_way(name):
        plan_check(name)
        p_hsum.copy_(h_sum, non_blocking=True)
        torch.cuda.synchronize()
        k = int(p_hsum[0])
        p_rec[:k].copy_(h_rec[:k], non_blocking=True)
        torch.cuda.synchronize()
        res["device"] = p_rec[:k, :4].numpy().copy().view("<u4").reshape(-1).tolist()
        res["d2h_device"] = 16 + 160 * k

    def host_way(name):
        w, o, ln = dv[name]
        h_off, h_len = rings[name][1], rings[name][2]
        plan(name)
        p_sum.copy_(r_sum, non_blocking=True)
        torch.cuda.synchronize()
        nh = int(p_sum.numpy()[1:2].view(np.uint32)[1])
        p_host[:nh].copy_(r_host[:nh], non_blocking=True)
        torch.cuda.synchronize()
        lst = p_host[:nh].numpy().tolist()
        listed = int(h_len[lst].sum()) if nh else 0
        whole = 8 * listed > w.numel()
        if whole:
            p_ring[name].copy_(w, non_blocking=True)
            torch.cuda.synchronize()
            buf = p_ring[name].numpy()
        ok = []
        for i in lst:
            a, wl = int(h_off[i]), int(h_len[i])
            if whole:
                msg = buf[a:a + wl].tobytes()
            else:
                p_msg[:wl].copy_(w[a:a + wl])
                msg = p_msg[:wl].numpy().tobytes()
            L = 148 if msg[0] == 1 else 92
            if wl != L:
                continue
            if hashlib.blake2s(msg[:L - 32], digest_size=16, key=key).digest() != msg[L - 32:L - 16]:
                continue
            if msg[L - 16:] != bytes(16):
                continue
            ok.append(i)
        res["host"] = ok
        res["d2h_host"] = 16 + 4 * nh + (int(w.numel()) if whole else listed)
        res["host_fetch"] = "whole ring" if whole else "per datagram"

    for name in ("flood", "mixed"):
        o2 = {"ring": name}
        device_way(name)
        host_way(name)
        o2["ways_agree"] = bool(res["device"] == res["host"])
        o2["n_valid"] = len(res["device"])
        wall = {"device": [], "host": []}
        variants = [("device", device_way), ("host", host_way)]
        for k in range(5 + 20):
            for nm, f in (variants if k % 2 == 0 else variants[::-1]):
                torch.cuda.synchronize()
                t = time.perf_counter()
                f(name)
                torch.cuda.synchronize()
                if k >= 5:
                    wall[nm].append((time.perf_counter() - t) * 1e6)
        o2["ab_device_wall_us"] = round(float(np.median(wall["device"])), 1)
        o2["ab_host_wall_us"] = round(float(np.median(wall["host"])), 1)
        o2["d2h_bytes_device"], o2["d2h_bytes_host"] = res["d2h_device"], res["d2h_host"]
        o2["host_fetch"] = res["host_fetch"]
        out[name] = o2
    emit(out)
    eng.close()


if __name__ == "__main__":
    main()
