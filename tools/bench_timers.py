"""Timing of wg_timers_sweep and wg_timers_mark against the host's way of running the same timers, on one box in one
run. Reports, after a 150-ms clock ramp, medians (min, max) of 10 calls after 3 warm-ups, HIP events on the launch stream:
  sweep_us   at 616 and 65,536 sessions (send slot k, recv slot n + k, peer k): nothing due; every keepalive due (interval
             1, the clock advanced by one tick per call); everything expired with WG_TIMERS_RETIRE (the sessions are
             started again and the table rebuilt before each call, outside the timed region)
  mark_us    a 65,536-descriptor batch spread over 1, 256 and 65,536 slots, both directions, the transmit one gated and not.
             The one-slot batch is 65,536 raises of one word, the case a per-lane atomic serialises on; WG_LIB_PATH
             names another build of the library to run the same figures against.
  host_us    wall time, median of 5, of the host alternative over the same 65,536 descriptors and sessions: statuses and
             descriptors copied back, numpy arrays of the same records updated (np.maximum.at), the three lists built with
             numpy, copied up. It is not the code under test.
`verified`: the summaries of every timed call are what the scenario says. One JSON line; --out appends it to a file."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
T0 = 1_000_000


def load():
    import importlib

    import torch
    return importlib.import_module("wireguard-java_amd"), torch


def timed(torch, fn, reps=10, warm=3, before=None):
    out = []
    for r in range(warm + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(float(np.median(out)), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def u32(torch, dev, v):
    return torch.from_numpy(np.asarray(v, np.uint32).view(np.int32).copy()).to(dev)


class Node:
    def __init__(self, W, torch, n, interval):
        dev = torch.device("cuda", 0)
        self.W, self.torch, self.dev, self.n = W, torch, dev, n
        L = W._lib
        self.eng = W.Engine(0, key_slots=2 * n)
        self.eng.timers_reserve(n)
        self.eng.rx_sessions_reserve(n)
        self.eng.timers_peers_set(0, [(interval, True)] * n)
        ent = np.zeros(n, W.WG_HS_ESTABLISHED_DTYPE)
        ent["pending"] = ent["peer"] = np.arange(n)
        ent["local_index"] = 0x10000 + 3 * np.arange(n)
        self.index = ent["local_index"].copy()
        self.ent = torch.from_numpy(ent.view(np.uint8).reshape(n, 96).copy()).to(dev)
        self.ok = torch.zeros(n, dtype=torch.int32, device=dev)
        self.send, self.recv = u32(torch, dev, np.arange(n)), u32(torch, dev, n + np.arange(n))
        self.now = torch.zeros(1, dtype=torch.int64, device=dev)
        self.exp = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self.init = torch.zeros(n, dtype=torch.int32, device=dev)
        self.keep = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        self.sum = torch.zeros(8, dtype=torch.int32, device=dev)
        self.src = L.WG_HS_INSTALL_ESTABLISHED

    def restart(self, t):
        self.eng.rx_sessions_set(self.index, self.n + np.arange(self.n))
        self.now.fill_(t)
        self.eng.timers_start(self.ent, None, self.ok, self.send, self.recv, self.now, self.src)

    def sweep(self, retire=False):
        self.eng.timers_sweep(self.now, self.exp, self.init, self.keep, self.sum, wire_stride=32, out_size=32 * self.n, retire=retire)

    def summary(self):
        self.torch.cuda.synchronize()
        return self.sum.cpu().numpy().tolist()


def bench_sweep(W, torch, n):
    out, ok = {}, True
    cfg = W.TimersConfig(reject_after_time=1000, rekey_after_time=900)
    nd = Node(W, torch, n, 0)
    nd.eng.timers_config_set(cfg)
    nd.restart(T0)
    nd.now.fill_(T0 + 1)
    out["none_due"] = timed(torch, nd.sweep)
    ok &= nd.summary() == [0, 0, 0, 0, 0, 0, n, 0]
    nd.eng.close()
    nd = Node(W, torch, n, 1)
    nd.eng.timers_config_set(cfg)
    nd.restart(T0)
    tick = [T0]

    def advance():
        tick[0] += 1
        nd.now.fill_(tick[0])
    out["keepalives_due"] = timed(torch, nd.sweep, before=advance)
    ok &= nd.summary() == [0, 0, 0, 0, n, n, n, 0]

    def again():
        nd.restart(T0)
        nd.now.fill_(T0 + 1000)
    out["expired_retire"] = timed(torch, lambda: nd.sweep(retire=True), before=again)
    ok &= nd.summary() == [n, n, n, n, 0, 0, 0, 0] and nd.eng.rx_sessions_count() == (0, n)
    nd.eng.close()
    return out, ok


def bench_mark(W, torch):
    dev = torch.device("cuda", 0)
    out, ok = {}, True
    nd = Node(W, torch, N, 0)
    nd.eng.timers_config_set(W.TimersConfig(reject_after_time=1 << 40, reject_after_messages=1 << 60))
    nd.restart(T0)
    msum = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.zeros(N, dtype=torch.int32, device=dev)
    tick = [T0]

    def advance():
        tick[0] += 1
        nd.now.fill_(tick[0])
    descs = {}
    for slots in (1, 256, N):
        for tx in (False, True):
            d = W.pack_desc(np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.arange(N, dtype=np.uint64), 64,
                            (np.arange(N) % slots) + (0 if tx else N))
            d_desc = torch.from_numpy(W.desc_as_int64(d)).to(dev)
            descs[(slots, tx)] = d_desc
            for gate in ((False, True) if tx else (False,)):
                name = f"{'tx' if tx else 'rx'}{'_gated' if gate else ''}_{slots}_slots"
                out[name] = timed(torch, lambda: nd.eng.timers_mark(d_desc, st, nd.now, msum, tx=tx, gate=gate, slot_first=0,
                                                                    slot_count=2 * N), before=advance)
                torch.cuda.synchronize()
                ok &= msum.cpu().numpy().tolist() == [N, 0] and not st.cpu().numpy().any()
    # the host alternative: statuses and descriptors back, numpy records, the three lists, copied up
    last, last_data = np.zeros(2 * N, np.uint64), np.zeros(2 * N, np.uint64)
    born = np.full(N, T0, np.uint64)
    walls = []
    d_desc = descs[(N, False)]
    for r in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        h_st = st.cpu().numpy()
        h_d = np.ascontiguousarray(d_desc.cpu().numpy()).view(W.WG_PKT_DTYPE).reshape(-1)
        now = np.uint64(tick[0] + r)
        okm = h_st == 0
        np.maximum.at(last, h_d["key_slot"][okm | (h_st == 3)], now)
        np.maximum.at(last_data, h_d["key_slot"][okm], now)
        age = now - born
        expired = np.nonzero(age >= 1 << 40)[0].astype(np.uint32)
        rekey = np.nonzero(age >= 1 << 39)[0].astype(np.uint32)
        keep = np.nonzero((last_data[N:] > last[:N]) & (now - last_data[N:] >= 10))[0].astype(np.uint32)
        for lst in (expired, rekey, keep):
            torch.from_numpy(np.concatenate([lst, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e6)
    out["host_us"] = {"median_us": round(float(np.median(walls)), 1), "min_us": round(min(walls), 1), "max_us": round(max(walls), 1)}
    nd.eng.close()
    return out, ok


def main():
    W, torch = load()
    dev = torch.device("cuda", 0)
    x = torch.ones(1 << 24, device=dev)
    t = time.time()
    while time.time() - t < 0.15:  # clock ramp
        x.mul_(1.0001)
    torch.cuda.synchronize()
    out = {"tool": "bench_timers", "device": torch.cuda.get_device_name(0)}
    ok = True
    for n in (616, N):
        out[f"sweep_{n}"], k = bench_sweep(W, torch, n)
        ok &= k
    out["mark_65536"], k = bench_mark(W, torch)
    out["verified"] = bool(ok and k)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    return 0 if out["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
