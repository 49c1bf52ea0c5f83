"""Timing of the transmit planner (wg_tx_plan) on the IMIX mix: 65,536 tun packets of 40 / 576 / 1500 B
(7 : 4 : 1, bench.py's draw), 256 key slots, one /24 route per slot, wire slots of 1,536 B.
Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the
launch stream):
  route_plan_us       wg_tx_plan(WG_TX_ROUTE) alone
  broadcast_plan_us   wg_tx_plan(WG_TX_BROADCAST) alone, 4 peers x 16,384 packets (65,536 descriptors)
  seal_frame_us       wg_seal_batch(WG_F_FRAME) on the route plan's descriptors
  planned_us          plan + seal + frame in one region
and, as an alternating A/B of wall time (call to stream-synchronised, median of 20 pairs, the order
swapped every pair), what the plan replaces:
  ab_planned_wall_us  tx_seal (plan, seal, frame: nothing built or uploaded by the host)
  ab_host_wall_us     the same descriptors built on the host with numpy (destination byte -> slot,
                      per-slot stable rank -> counter), uploaded (32 B per packet) and sealed + framed
  host_build_us       the numpy build alone (part of ab_host_wall_us)
Both paths must produce the same ring (checked once). One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def splitmix_np(seed: int, n: int) -> np.ndarray:
    words = (n + 7) // 8
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.arange(1, words + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.astype("<u8").view(np.uint8)[:n].copy()


def main():
    import importlib
    import torch
    torch.cuda.is_available()
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, stride, max_len = 65536, 256, 1536, 1500
    u = splitmix_np(0x5EED2026, 4 * n).view("<u4") % 12
    lens = np.where(u < 7, 40, np.where(u < 11, 576, 1500)).astype(np.int64)
    sizes = (lens + 15) // 16 * 16
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    ring = splitmix_np(7, int(sizes.sum()))
    dst3 = (splitmix_np(11, n).astype(np.int64) % K).astype(np.uint8)  # 10.0.<slot>.x
    ring[off] = 0x45
    ring[off + 16], ring[off + 17], ring[off + 18] = 10, 0, dst3
    eng = W.Engine(0, key_slots=K)
    eng.set_keys(0, splitmix_np(3, 32 * K))
    eng.set_receivers(torch.arange(K, dtype=torch.int32, device=dev))
    eng.routes_set([(f"10.0.{k}.0", 24, k) for k in range(K)])
    eng.tx_peers_set([0, 1, 2, 3])
    eng.tx_reserve(n)
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    wire = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    out_size = wire.numel()
    nb = n // 4

    def route_plan():
        eng.tx_plan(d_ring, d_off, d_len, d_desc, d_st, stride, out_size, max_len, route=True)

    def broadcast_plan():
        eng.tx_plan(d_ring, d_off[:nb], d_len[:nb], d_desc, d_st, stride, out_size, max_len, route=False)

    def seal_frame():
        eng.seal(d_desc, d_ring, wire, max_len, frame=True)

    def planned():
        eng.tx_seal(d_ring, d_off, d_len, d_desc, d_st, wire, stride, max_len, route=True)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        planned()
        torch.cuda.synchronize()

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

    out = {"n": n, "key_slots": K, "mix": "imix 40/576/1500 at 7:4:1", "wire_stride": stride}
    out["broadcast_plan_us"] = timed(broadcast_plan)
    out["route_plan_us"] = timed(route_plan)
    out["tx_status_hist"] = np.bincount(d_st.cpu().numpy(), minlength=10).tolist()
    out["seal_frame_us"] = timed(seal_frame)  # on the descriptors of the last route plan
    out["planned_us"] = timed(planned)

    # what the plan replaces: the descriptors from the host
    h_desc = torch.zeros((n, 4), dtype=torch.int64).pin_memory()
    h_view = h_desc.numpy().view(W.WG_PKT_DTYPE).reshape(-1)
    host_send = np.zeros(K, np.uint64)
    build_ts = []

    def host_built():
        t = time.perf_counter()
        slot = ring[off + 18].astype(np.int64)
        order = np.argsort(slot, kind="stable")
        first = np.searchsorted(slot[order], np.arange(K))
        rank = np.empty(n, np.uint64)
        rank[order] = (np.arange(n) - first[slot[order]]).astype(np.uint64)
        h_view["in_off"], h_view["out_off"] = off, np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(16)
        h_view["counter"], h_view["len"], h_view["key_slot"] = host_send[slot] + rank, lens, slot
        host_send[:] += np.bincount(slot, minlength=K).astype(np.uint64)
        build_ts.append((time.perf_counter() - t) * 1e6)
        d_desc.copy_(h_desc, non_blocking=True)
        eng.seal(d_desc, d_ring, wire, max_len, frame=True)

    # same ring from both paths, from the same counters
    eng.tx_counters_set(0, np.zeros(K, np.uint64))
    planned()
    torch.cuda.synchronize()
    ring_planned = wire.clone()
    host_built()
    torch.cuda.synchronize()
    out["paths_agree"] = bool(torch.equal(ring_planned, wire))

    wall = {"planned": [], "host": []}
    variants = [("planned", planned), ("host", host_built)]
    for k in range(5 + 20):
        for name, f in (variants if k % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if k >= 5:
                wall[name].append((time.perf_counter() - t) * 1e6)
    out["ab_planned_wall_us"] = round(float(np.median(wall["planned"])), 1)
    out["ab_host_wall_us"] = round(float(np.median(wall["host"])), 1)
    out["host_build_us"] = round(float(np.median(build_ts[-20:])), 1)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
