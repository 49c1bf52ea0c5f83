"""Timing of the receive planner (wg_rx_plan / wg_rx_deliver) on the wire ring that tools/bench_tx.py's
route plan produces: 65,536 IMIX packets (40 / 576 / 1500 B at 7 : 4 : 1), 256 sessions, wire slots of
1,536 B; 1% of the ring is then edited (forged tags, type bytes 1 / 2 / 9, unknown receiver indices).
Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch
stream):
  plan_after_us / plan_packed_us   wg_rx_plan alone in each mode
  deliver_us                       wg_rx_deliver alone (on the statuses of the last planned run)
  parse_open_us                    wg_parse_open alone on the same ring (what the plan replaces on the device)
  open_us                          wg_open_batch(WG_F_RX_FILTER) alone on the packed plan's descriptors
  planned_us                       plan + open + deliver in one region (Engine.rx_open)
and, as an alternating A/B of wall time (call to synchronised with the result on the host, median of 20
pairs, the order swapped every pair), against the way without the planner on the same packets:
  ab_planned_wall_us  rx_open, then the 16-B totals and the n_items x 16-B delivery list copied back
  ab_host_wall_us     a numpy parse of type byte and receiver index from the host's copy of the ring, a dict
                      lookup per packet, the key-slot array uploaded (4 B per packet), wg_parse_open, the
                      same open, the statuses copied back (4 B per packet) and scanned with numpy
  host_parse_us / host_scan_us     the two host parts alone (inside ab_host_wall_us);
  host_parse_vectorised_us         the lookup done with numpy.searchsorted instead of the dict (a bound
                                   for a host that vectorises it; not part of the A/B)
wg_parse_open puts each plaintext behind its packet, so that path needs wire slots of 3,072 B (the ring
is copied into that layout once, outside the timing) and copies back a buffer of that size; the planned
path copies back pt_used bytes: d2h_bytes_host / d2h_bytes_planned. Both paths must deliver the same
packets (checked once). `--profile` runs the planned pipeline 25 times and nothing else, for a
kernel-trace run of its own. One JSON line; --out appends it to a file."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tx import splitmix_np  # noqa: E402


def main():
    import importlib
    import torch
    torch.cuda.is_available()
    W = importlib.import_module("wireguard-java_amd")
    L = W._lib
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
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.set_receivers(torch.from_numpy(receivers.view(np.int32)).to(dev))
    eng.routes_set([(f"10.0.{k}.0", 24, k) for k in range(K)])
    sessions = {int(receivers[k]): k for k in range(K)}
    eng.rx_sessions_set(list(sessions.keys()), list(sessions.values()))
    eng.tx_reserve(n)
    eng.rx_reserve(n)
    d_ring = torch.from_numpy(ring).to(dev)
    d_toff = torch.from_numpy(off).to(dev)
    d_tlen = torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    wire = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    eng.tx_seal(d_ring, d_toff, d_tlen, d_desc, d_st, wire, stride, max_len, route=True)
    torch.cuda.synchronize()
    assert int((d_st != 0).sum()) == 0
    # 1% of the ring edited, as a receiver sees it: forged tags, handshake and junk types, unknown indices
    h_wire = wire.cpu().numpy()
    pick = np.nonzero(splitmix_np(13, n) < 3)[0]  # about 1.2%
    for k, j in enumerate(pick):
        o = int(j) * stride
        if k % 4 == 0:
            h_wire[o + 16 + int(lens[j]) + 5] ^= 0x20
        elif k % 4 == 1:
            h_wire[o] = (1, 2, 9)[(k // 4) % 3]
        elif k % 4 == 2:
            h_wire[o + 4:o + 8] = (0xEE, 0xEE, 0xEE, 0xEE)
        else:
            h_wire[o + 40] ^= 1  # a ciphertext byte
    wire.copy_(torch.from_numpy(h_wire))
    w_off = np.arange(n, dtype=np.int64) * stride
    w_len = (lens + 32).astype(np.int32)
    d_woff = torch.from_numpy(w_off).to(dev)
    d_wlen = torch.from_numpy(w_len).to(dev)
    pt_size = int(sizes.sum())
    d_pt = torch.zeros(pt_size, dtype=torch.uint8, device=dev)
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, o_st, f_st, r_idx = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5))
    r_sum, r_del = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    r_items = torch.zeros((n, 2), dtype=torch.int64, device=dev)

    def plan_after():
        eng.rx_plan(wire, d_woff, d_wlen, r_desc, r_st, r_host, r_sum, max_len, packed=False)

    def plan_packed():
        eng.rx_plan(wire, d_woff, d_wlen, r_desc, r_st, r_host, r_sum, max_len, packed=True, pt_size=pt_size)

    def open_only():
        eng.open(r_desc, wire, d_pt, o_st, max_len, rx_filter=True)

    def deliver():
        eng.rx_deliver(r_desc, r_st, o_st, f_st, r_items, r_del, index_out=r_idx)

    d_zero_slot = torch.zeros(n, dtype=torch.int32, device=dev)
    p_desc0 = torch.zeros((n, 4), dtype=torch.int64, device=dev)

    def parse_only():  # the kernel the plan replaces, on the same ring (key slots given: no lookup)
        eng.parse_open(wire, d_woff, d_wlen, d_zero_slot, p_desc0, o_st)

    def planned():
        eng.rx_open(wire, d_woff, d_wlen, r_desc, r_st, r_host, r_sum, d_pt, o_st, f_st, r_items, r_del, max_len,
                    packed=True, index_out=r_idx)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        planned()
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        for _ in range(25):
            planned()
            parse_only()
            torch.cuda.synchronize()
        print(json.dumps({"profile_pass": 25}))
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

    out = {"n": n, "sessions": K, "mix": "imix 40/576/1500 at 7:4:1", "wire_stride": stride, "edited": int(len(pick))}
    out["parse_open_us"] = timed(parse_only)
    out["plan_after_us"] = timed(plan_after)
    out["plan_packed_us"] = timed(plan_packed)  # (leaves the packed descriptors for the open below)
    out["open_us"] = timed(open_only)
    out["deliver_us"] = timed(deliver)
    out["planned_us"] = timed(planned)
    torch.cuda.synchronize()
    h_sum, h_del = r_sum.cpu().numpy(), r_del.cpu().numpy()
    out["pt_used"] = int(h_sum[0])
    out["n_open"], out["n_host"] = (int(x) for x in h_sum[1:2].view(np.uint32))
    out["n_items"], out["n_keepalive"] = (int(x) for x in h_del[1:2].view(np.uint32))
    out["final_status_hist"] = np.bincount(f_st.cpu().numpy(), minlength=12).tolist()
    planned_idx = r_idx[:out["n_items"]].cpu().numpy()

    # ---- the way without the planner: plaintext behind each packet, so wire slots of 2 x 1,536 B
    stride2 = 2 * stride
    wire2 = torch.zeros(n * stride2, dtype=torch.uint8, device=dev)
    wire2.view(n, stride2)[:, :stride].copy_(wire.view(n, stride))
    h_wire2 = wire2.cpu().numpy()  # the host's copy of what it received
    w_off2 = np.arange(n, dtype=np.int64) * stride2
    d_woff2 = torch.from_numpy(w_off2).to(dev)
    h_slot = torch.zeros(n, dtype=torch.int32).pin_memory()
    d_slot = torch.zeros(n, dtype=torch.int32, device=dev)
    h_status = torch.zeros(n, dtype=torch.int32).pin_memory()
    p_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    p_st = torch.zeros(n, dtype=torch.int32, device=dev)
    o_st2 = torch.zeros(n, dtype=torch.int32, device=dev)
    parse_ts, scan_ts, res = [], [], {}
    index_at = (w_off2[:, None] + np.arange(4, 8)[None, :])

    def host_way():
        t = time.perf_counter()
        types = h_wire2[w_off2]
        index = h_wire2[index_at].copy().view("<u4").reshape(-1)
        slot = h_slot.numpy()
        slot[:] = [sessions.get(x, 0) for x in index.tolist()]
        known = np.fromiter((x in sessions for x in index.tolist()), bool, n)
        # what wg_parse_open cannot tell apart is told here: handshakes and unknown indices never reach the open
        lens_in = np.where((types == 4) & known, w_len, 0).astype(np.int32)
        parse_ts.append((time.perf_counter() - t) * 1e6)
        d_slot.copy_(h_slot, non_blocking=True)
        d_lens_in = torch.from_numpy(lens_in).to(dev, non_blocking=True)
        eng.parse_open(wire2, d_woff2, d_lens_in, d_slot, p_desc, p_st)
        eng.open(p_desc, wire2, wire2, o_st2, max_len, rx_filter=True)
        h_status.copy_(o_st2, non_blocking=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res["idx"] = np.nonzero(h_status.numpy() == 0)[0]
        scan_ts.append((time.perf_counter() - t) * 1e6)

    h_del2 = torch.zeros(2, dtype=torch.int64).pin_memory()
    h_items = torch.zeros((n, 2), dtype=torch.int64).pin_memory()

    def planned_way():
        planned()
        h_del2.copy_(r_del, non_blocking=True)
        torch.cuda.synchronize()
        k = int(h_del2.numpy()[1:2].view(np.uint32)[0])
        h_items[:k].copy_(r_items[:k], non_blocking=True)
        torch.cuda.synchronize()
        res["k"] = k

    host_way()
    out["paths_agree"] = bool(np.array_equal(res["idx"], planned_idx))
    wall = {"planned": [], "host": []}
    variants = [("planned", planned_way), ("host", host_way)]
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
    out["host_parse_us"] = round(float(np.median(parse_ts[-20:])), 1)
    out["host_scan_us"] = round(float(np.median(scan_ts[-20:])), 1)
    order = np.argsort(np.array(list(sessions.keys()), np.uint32))
    keys_sorted = np.array(list(sessions.keys()), np.uint32)[order]
    vals_sorted = np.array(list(sessions.values()), np.int32)[order]
    vec = []
    for _ in range(10):
        t = time.perf_counter()
        types = h_wire2[w_off2]
        index = h_wire2[index_at].copy().view("<u4").reshape(-1)
        pos = np.minimum(np.searchsorted(keys_sorted, index), K - 1)
        known = keys_sorted[pos] == index
        slot = np.where(known, vals_sorted[pos], 0)
        lens_in = np.where((types == 4) & known, w_len, 0).astype(np.int32)
        vec.append((time.perf_counter() - t) * 1e6)
    out["host_parse_vectorised_us"] = round(float(np.median(vec)), 1)
    out["d2h_bytes_host"] = int(wire2.numel())
    out["d2h_bytes_planned"] = int(min(out["pt_used"], pt_size))
    out["d2h_bytes_wire_ring"] = int(wire.numel())
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
