"""Timing of wg_hs_ratelimit, in one process with wg_hs_admit as the yardstick, on rings of valid-mac1, valid-mac2
initiations with random bodies (tools/bench_hs_cookie.py's flood ring (b), every datagram valid):
  spread  65,536 datagrams from as many sources (and its first 616)
  16src   65,536 datagrams from 16 sources
  1src    65,536 datagrams from one source
Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch stream; `now`
advances by `cost` before each call, outside the timed region; WireGuard's config at 1000 ticks per second):
  rl_<N>_<ring>_us        wg_hs_ratelimit on admit's records with every source in the table
  rl_<N>_spread_new_us    the same into an empty table (every record claims a bucket; the load is outside the timing)
  admit_<N>_spread_us     wg_hs_admit on the same ring
  chain_norl_us, chain_rl_us   plan -> admit -> [ratelimit] -> dh -> open -> stamp -> respond on the 16src ring, and
                          chain_*_ladders, the records that reached wg_hs_dh
One JSON line; --out appends it to a file; --table also prints the rows of DESIGN.md's table. --shape <ring> runs 30
plain calls on one ring and exits (for a kernel trace)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_hs  # noqa: E402
from bench_hs_cookie import SECRET, cookie, mac, sources  # noqa: E402
from bench_tx import splitmix_np  # noqa: E402


def valid_ring(n, src):
    """n initiations with random bodies, a correct mac1 and the mac2 of their source"""
    body = splitmix_np(0x524C, n * 116).reshape(n, 116).copy()
    body[:, 0] = 1
    body[:, 1:4] = 0
    msgs = np.zeros((n, 148), np.uint8)
    for i in range(n):
        m = bench_hs.with_mac1(body[i].tobytes())[:132]
        msgs[i] = np.frombuffer(m + mac(cookie(src[i]), m), np.uint8)
    return msgs.reshape(-1), np.arange(n, dtype=np.int64) * 148, np.full(n, 148, np.int32)


def main():
    import torch
    torch.cuda.is_available()
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, max_len, small = 65536, 256, 1500, 616
    B = W.Engine(0, key_slots=K)
    b_pub = B.hs_static_set(bytes(splitmix_np(0x4242, 32)))
    bench_hs.PUB = b_pub
    B.hs_peers_set([bytes(splitmix_np(0x4141, 32))])
    B.hs_cookie_secret_set(SECRET)
    B.set_keys(0, splitmix_np(3, 32 * K))
    B.rx_sessions_set([1 + k for k in range(K)], list(range(K)))
    B.rx_reserve(n)
    B.hs_reserve(n)
    B.hs_stamps_set(0, [])
    B.hs_rl_reserve(n)
    cfg = W.RateLimitConfig.wireguard(1000)
    B.hs_rl_config_set(cfg)
    spread = sources(n)
    srcs = {"spread": spread, "16src": spread[np.arange(n) % 16].copy(), "1src": spread[np.zeros(n, np.int64)].copy()}
    for name in ("16src", "1src"):  # (the ports stay each datagram's own: not part of the key)
        srcs[name][:, 16:18] = spread[:, 16:18]
    t8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    t32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    fresh_nonces = torch.from_numpy(splitmix_np(0x4E4F, 24 * n).reshape(n, 24) | 1).to(dev)
    d_non = t8(n, 24)
    d_now = torch.full((1,), 1_000_000, dtype=torch.int64, device=dev)
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st = t32(n), t32(n), t32(n)
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec, h_sum, h_rep, h_asum = t8(n, 160), t32(4), t8(n, 80), t32(4)
    l_st, l_rec, l_sum = t32(n), t8(n, 160), t32(4)
    d_sh, d_dh, d_ost, d_init, d_osum = t8(n, 32), t32(n), t32(n), t8(n, 144), t32(4)
    s_st, s_open, s_fresh, s_sum = t32(n), t8(n, 12), t8(n, 144), t32(4)
    r_eph, r_li, r_rst, r_sess, r_rsum = torch.from_numpy(splitmix_np(0x4550, 32 * n) | 1).to(dev), t32(n), t32(n), t8(n, 176), t32(4)

    def tick():
        d_non.copy_(fresh_nonces)
        d_now.add_(cfg.cost)

    def timed(f, pre=tick, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for k in range(warm + reps):
            pre()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(ts)), 2)

    ring, off, lens = valid_ring(n, spread)
    w, o, ln = torch.from_numpy(ring).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    d_src = {k: torch.from_numpy(v).to(dev) for k, v in srcs.items()}

    def admit(N=n, src="spread", **lst):
        B.hs_admit(w[:148 * N], o[:N], ln[:N], d_src[src][:N], d_non[:N], h_st[:N], h_rec[:N], h_sum, h_rep[:N], h_asum, **lst)

    def limit(N=n, src="spread"):  # (the records' mac2 is not read: one set of records serves every src array)
        B.hs_ratelimit(h_rec[:N], None, d_src[src][:N], d_now, l_st[:N], l_rec[:N], l_sum)

    tick()
    admit()
    torch.cuda.synchronize()
    assert int(h_sum.cpu().numpy()[0]) == n, "every datagram of the spread ring is admitted"
    if "--shape" in sys.argv:
        shape = sys.argv[sys.argv.index("--shape") + 1]
        for _ in range(30):
            tick()
            limit(n, shape)
        torch.cuda.synchronize()
        B.close()
        return
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        tick()
        limit()
        torch.cuda.synchronize()
    out = {"n": n, "cost": cfg.cost, "burst": cfg.burst}
    empty = np.zeros(0, W.WG_HS_RL_ENTRY_DTYPE)

    def cold():
        B.hs_rl_load(empty)
        tick()

    for N in (small, n):
        out[f"rl_{N}_spread_new_us"] = timed(lambda: limit(N), pre=cold)
        out[f"rl_{N}_spread_new_counts"] = l_sum.cpu().numpy().tolist()
        out[f"rl_{N}_spread_us"] = timed(lambda: limit(N))
        out[f"rl_{N}_spread_counts"] = l_sum.cpu().numpy().tolist()
        out[f"admit_{N}_spread_us"] = timed(lambda: admit(N))
    for src in ("16src", "1src"):
        B.hs_rl_load(empty)
        out[f"rl_{n}_{src}_us"] = timed(lambda: limit(n, src))
        out[f"rl_{n}_{src}_counts"] = l_sum.cpu().numpy().tolist()
    out["table_entries"] = B.hs_rl_count()[0]
    # ---- the chain on the 16-source ring (its mac2 is for these sources)
    ring, off, lens = valid_ring(n, srcs["16src"])
    w = torch.from_numpy(ring).to(dev)

    def tail(rec, sm):
        B.hs_dh(rec, sm, d_sh, d_dh)
        B.hs_open(rec, sm, d_sh, d_dh, d_ost, d_init, d_osum)
        B.hs_stamp(d_init, d_osum, rec, d_sh, s_st, s_open, s_fresh, s_sum)
        B.hs_respond(s_fresh, s_sum, r_eph, r_li, r_rst, r_sess, r_rsum)

    def chain(rl):
        B.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
        admit(n, "16src", host_list=r_host, rx_summary=r_sum)
        if rl:
            B.hs_ratelimit(h_rec, h_sum, d_src["16src"], d_now, l_st, l_rec, l_sum)
            tail(l_rec, l_sum)
        else:
            tail(h_rec, h_sum)

    out["chain_norl_us"] = timed(lambda: chain(False))
    out["chain_norl_ladders"] = int(h_sum.cpu().numpy()[0])
    out["chain_rl_us"] = timed(lambda: chain(True))
    out["chain_rl_ladders"] = int(l_sum.cpu().numpy()[0])
    out["chain_rl_admitted"] = int(h_sum.cpu().numpy()[0])
    bench_hs.emit(out)
    if "--table" in sys.argv:
        print("| measurement | µs |\n|---|---|")
        for k, v in out.items():
            if k.endswith("_us"):
                print(f"| {k[:-3]} | {v} |")
    B.close()


if __name__ == "__main__":
    main()
