"""Timing of wg_tx_sendlist and wg_endpoints_learn against their yardsticks and the host's way of doing the same, on one
box in one run. Reports, after a 150-ms clock ramp, medians (min, max) of 10 calls after 3 warm-ups, HIP events on the
launch stream, for 616 and 65,536 descriptors:
  sendlist_us  wg_tx_sendlist over descriptors spread over as many peers as descriptors and all on one peer, the gate on
               and off (every peer has an endpoint, so the gate refuses nothing and the calls repeat), and wg_rx_deliver
               over the same n in the same process: the same three-launch skeleton, the yardstick.
  learn_us     wg_endpoints_learn spread and all on one peer (the sources alternate between two addresses from call to
               call, so every call roams), and wg_timers_mark (receive direction) over the same two batches; the two
               one-peer / spread ratios. A learn ratio well above mark's would say the wave election is missing.
  host_us      wall time, median of 5, of the host alternative each call replaces: descriptors and statuses copied back,
               the send list (or the peer -> address table) built with numpy. It is not the code under test.
`verified`: the summaries of every timed call are what the scenario says. One JSON line; --out appends it to a file."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_timers import load, timed, u32  # noqa: E402

T0 = 1_000_000


def addresses(W, n, port):
    v = np.zeros(n, W.WG_HS_SRC_DTYPE)
    v["addr"][:, 0] = 10
    v["addr"][:, 1:4] = np.stack([(np.arange(n) >> s) & 255 for s in (16, 8, 0)], axis=1)
    v["port"][:] = (port >> 8, port & 255)
    v["family"] = 4
    return v


def summary64(t):
    h = t.cpu().numpy()
    return int(h[0]), int(h[1]) & 0xFFFFFFFF, (int(h[1]) >> 32) & 0xFFFFFFFF


def bench(W, torch, n):
    dev = torch.device("cuda", 0)
    out, ok = {}, True
    eng = W.Engine(0, key_slots=n)
    eng.endpoints_reserve(n)
    eng.timers_reserve(n)
    eng.endpoints_set(0, addresses(W, n, 1000))
    eng.endpoint_slots_set(0, np.arange(n, dtype=np.uint32))
    # every key slot a RECV record, so that wg_timers_mark (receive direction) marks it
    ent = np.zeros(n // 2, W.WG_HS_ESTABLISHED_DTYPE)
    ent["pending"] = ent["peer"] = np.arange(n // 2)
    now = torch.full((1,), T0, dtype=torch.int64, device=dev)
    eng.timers_start(torch.from_numpy(ent.view(np.uint8).reshape(n // 2, 96).copy()).to(dev), None,
                     torch.zeros(n // 2, dtype=torch.int32, device=dev), u32(torch, dev, 2 * np.arange(n // 2)),
                     u32(torch, dev, 2 * np.arange(n // 2) + 1), now, W._lib.WG_HS_INSTALL_ESTABLISHED)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    items = torch.zeros((n, 48), dtype=torch.uint8, device=dev)
    s64 = torch.zeros(2, dtype=torch.int64, device=dev)
    s32 = torch.zeros(4, dtype=torch.int32, device=dev)
    msum = torch.zeros(2, dtype=torch.int32, device=dev)
    roam = torch.zeros(n, dtype=torch.int32, device=dev)
    rx_items, deliv = torch.zeros((n, 2), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    fst = torch.zeros(n, dtype=torch.int32, device=dev)
    srcs = [torch.from_numpy(addresses(W, n, p).view(np.uint8).reshape(n, 24).copy()).to(dev) for p in (2000, 3000)]
    flip = [0]
    tick = [T0]

    def advance():
        flip[0] ^= 1
        tick[0] += 1
        now.fill_(tick[0])

    descs = {}
    for name, slots in (("spread", np.arange(n)), ("one_peer", np.full(n, 1))):
        d = W.pack_desc(np.zeros(n, np.uint64), 16 + 96 * np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64), 64, slots)
        d_desc = descs[name] = torch.from_numpy(W.desc_as_int64(d)).to(dev)
        for gate in (False, True):
            out[f"sendlist_{name}{'_gated' if gate else ''}"] = timed(torch, lambda: eng.tx_sendlist(d_desc, st, items, s64, gate=gate))
            torch.cuda.synchronize()
            ok &= summary64(s64) == (96 * n, n, 0) and not st.cpu().numpy().any()
        out[f"learn_{name}"] = timed(torch, lambda: eng.endpoints_learn(d_desc, st, srcs[flip[0]], roam, s32), before=advance)
        torch.cuda.synchronize()
        ok &= s32.cpu().numpy().tolist() == ([n, n, n, 0] if name == "spread" else [n, 1, 1, 0])
        out[f"mark_{name}"] = timed(torch, lambda: eng.timers_mark(d_desc, st, now, msum), before=advance)
        torch.cuda.synchronize()
        ok &= msum.cpu().numpy().tolist() == ([n // 2, 0] if name == "spread" else [n, 0])
    out["rx_deliver"] = timed(torch, lambda: eng.rx_deliver(descs["spread"], st, st, fst, rx_items, deliv))
    for call in ("learn", "mark"):
        out[f"{call}_one_peer_over_spread"] = round(out[f"{call}_one_peer"]["median_us"] / out[f"{call}_spread"]["median_us"], 2)
    # the host alternative: descriptors and statuses back, the list / the table with numpy
    h_ep = addresses(W, n, 1000)
    h_map = np.arange(n, dtype=np.uint32)
    walls = {"sendlist": [], "learn": []}
    for r in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        h_st = st.cpu().numpy()
        h_d = np.ascontiguousarray(descs["spread"].cpu().numpy()).view(W.WG_PKT_DTYPE).reshape(-1)
        live = np.nonzero((h_st == 0) & (h_d["len"] != 0xFFFFFFFF))[0]
        peer = h_map[h_d["key_slot"][live]]
        lst = np.zeros(len(live), W.WG_TX_ITEM_DTYPE)
        lst["off"], lst["len"], lst["key_slot"] = h_d["out_off"][live] - 16, h_d["len"][live] + 32, h_d["key_slot"][live]
        lst["peer"], lst["index"], lst["dst"] = peer, live, h_ep[peer]
        walls["sendlist"].append((time.perf_counter() - t) * 1e6)
        torch.cuda.synchronize()
        t = time.perf_counter()
        h_st = st.cpu().numpy()
        h_d = np.ascontiguousarray(descs["spread"].cpu().numpy()).view(W.WG_PKT_DTYPE).reshape(-1)
        h_src = srcs[r & 1].cpu().numpy().reshape(-1).view(W.WG_HS_SRC_DTYPE)
        q = np.nonzero((h_st == 0) | (h_st == 3))[0]
        last = np.full(n, -1, np.int64)
        np.maximum.at(last, h_map[h_d["key_slot"][q]], q)
        seen = np.nonzero(last >= 0)[0]
        moved = seen[(h_ep[seen] != h_src[last[seen]])]
        h_ep[moved] = h_src[last[moved]]
        walls["learn"].append((time.perf_counter() - t) * 1e6)
    for k, w in walls.items():
        out[f"host_{k}"] = {"median_us": round(float(np.median(w)), 1), "min_us": round(min(w), 1), "max_us": round(max(w), 1)}
    eng.close()
    return out, ok


def main():
    W, torch = load()
    dev = torch.device("cuda", 0)
    x = torch.ones(1 << 24, device=dev)
    t = time.time()
    while time.time() - t < 0.15:  # clock ramp
        x.mul_(1.0001)
    torch.cuda.synchronize()
    out = {"tool": "bench_endpoints", "device": torch.cuda.get_device_name(0)}
    ok = True
    for n in (616, 65536):
        out[f"n_{n}"], k = bench(W, torch, n)
        ok &= k
    out["verified"] = bool(ok)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    return 0 if out["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
