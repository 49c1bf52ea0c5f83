"""Timing of the end of a session on the device: wg_rx_sessions_compact, wg_timers_sweep with WG_TIMERS_WIPE, and
wg_rx_plan on a half-retired table before and after the compaction. Reports, after a 150-ms clock ramp, medians (min,
max) of 10 calls after 3 warm-ups, HIP events on the launch stream:
  compact_us        wg_rx_sessions_compact at 65,536 live + 65,536 retired entries in C = 262,144 (the table is brought
                    back to that state before each call, outside the timed region: wg_rx_sessions_set of the 65,536 old
                    indices, their retirement, wg_hs_install of the 65,536 new ones)
  compact_noop_us   the same call on the compacted table (nothing retired: the spare is cleared, nothing else)
  host_rebuild_us   wall time, median of 5, of the only way to reclaim without it: wg_rx_sessions_set of the live lists
                    the host holds. It is not the code under test.
  plan_us           wg_rx_plan over 65,536 transport headers carrying the live indices, 20 calls after 5 warm-ups, on
                    the half-retired table and on the compacted one
  sweep_us          wg_timers_sweep over 65,536 sessions, all expiring, with WG_TIMERS_RETIRE and with RETIRE | WIPE
                    (tools/bench_timers.py's scenario: the sessions are started again before each call)
`verified`: the summaries, the table's counts, lookups of a sample of live, retired and unknown indices through wg_rx_plan,
and after the wiping sweep the key table through a seal of a sample of slots against the oracle under zero keys.
`--ab OTHER_LIB` first runs, in fresh child processes, tools/bench_timers.py's sweep figures alternately under OTHER_LIB
(the parent commit's library) and this one, twice each (`--timers` is that child's mode): the sweep's placing kernel gained
a pointer and a branch, and WG_TIMERS_RETIRE alone must cost what it did, within that tool's own run-to-run spread.
`--profile` runs the compaction and the wiping sweep 10 times each and nothing else, for a kernel-trace run of its own;
`--trace FILE.csv` turns that run's kernel trace into the median time per kernel. One JSON line each; --out appends it to
a file."""
import csv
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tx import splitmix_np  # noqa: E402

KERNELS = ("k_rx_compact_clear", "k_rx_compact_rehash", "k_rx_compact_flip", "k_tm_sweep_judge", "k_tm_sweep_place")
N = 65536
T0 = 1_000_000


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


def load():
    """The package, bound to what the library in use exports (the parent's lacks this commit's symbol). The package
    binds its SIGNATURES list lazily, at the first W.lib() / Engine(): this must run before either."""
    import ctypes
    import importlib
    import torch
    assert torch.cuda.is_available(), "bench_session_end needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    have = ctypes.CDLL(W._lib.LIB_PATH)
    W._lib.SIGNATURES[:] = [sig for sig in W._lib.SIGNATURES if hasattr(have, sig[0])]
    return W, torch, torch.device("cuda", 0)


def child(other):
    env = dict(os.environ)
    if other:
        env["WG_LIB_PATH"] = os.path.abspath(other)
    else:
        env.pop("WG_LIB_PATH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--timers"], env=env, stdout=subprocess.PIPE, timeout=400)
    if p.returncode != 0:
        raise SystemExit(f"--timers under {'the other' if other else 'this'} library ended with {p.returncode}")
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    r["library"] = "other" if other else "this"
    return r


def ramp(torch, dev):
    x = torch.ones(1 << 24, device=dev)
    t = time.time()
    while time.time() - t < 0.15:
        x.mul_(1.0001)
    torch.cuda.synchronize()


def timers_mode():
    """tools/bench_timers.py's sweep figures at 65,536 sessions, under whichever library is loaded."""
    W, torch, dev = load()
    import bench_timers
    ramp(torch, dev)
    out, ok = bench_timers.bench_sweep(W, torch, N)
    print(json.dumps({"sweep_65536": out, "verified": bool(ok), "version": W.lib().wg_version().decode()}))


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


class Table:
    """65,536 live + 65,536 retired entries in C = 262,144, and wg_rx_plan over the live indices."""

    def __init__(self, W, torch, dev):
        self.W, self.torch, self.dev = W, torch, dev
        L = W._lib
        K = 2 * N
        self.eng = W.Engine(0, key_slots=K)
        self.eng.rx_sessions_reserve(N)
        self.eng.rx_reserve(N)
        self.old = (np.arange(N, dtype=np.uint32) * np.uint32(40503) + np.uint32(0x01000000)).astype(np.uint32)
        self.new = (np.arange(N, dtype=np.uint32) * np.uint32(40503) + np.uint32(0x41000000)).astype(np.uint32)
        self.new_slots = np.arange(1, K, 2, dtype=np.uint32)
        ent = np.frombuffer(splitmix_np(0x5E0D, 176 * N).tobytes(), W.WG_HS_SESSION_DTYPE).copy()
        ent["init"] = np.arange(N, dtype=np.uint32)
        ent["local_index"] = self.new
        self.master = torch.from_numpy(ent.view(np.uint8).reshape(N, 176)).to(dev)
        self.d_sess = torch.zeros_like(self.master)
        self.d_old = torch.from_numpy(self.old.view(np.int32).copy()).to(dev)
        self.send = torch.arange(0, K, 2, dtype=torch.int32, device=dev)
        self.recv = torch.arange(1, K, 2, dtype=torch.int32, device=dev)
        self.st, self.sm = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        self.csum = torch.zeros(4, dtype=torch.int32, device=dev)
        self.src = L.WG_HS_INSTALL_SESSIONS
        # one 32-byte transport header (a keepalive) per live index
        wire = np.zeros((N, 32), np.uint8)
        wire[:, 0] = 4
        wire[:, 4:8] = self.new.view(np.uint8).reshape(N, 4)
        self.wire = torch.from_numpy(wire.reshape(-1)).to(dev)
        self.w_off = torch.arange(0, 32 * N, 32, dtype=torch.int64, device=dev)
        self.w_len = torch.full((N,), 32, dtype=torch.int32, device=dev)
        self.r_desc = torch.zeros((N, 4), dtype=torch.int64, device=dev)
        self.r_st, self.r_host = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        self.r_sum = torch.zeros(2, dtype=torch.int64, device=dev)

    def half_retired(self):
        self.eng.rx_sessions_set(self.old, np.arange(0, 2 * N, 2, dtype=np.uint32))
        self.eng.rx_sessions_retire(self.d_old)
        self.d_sess.copy_(self.master)
        self.eng.hs_install(self.d_sess, None, self.send, self.recv, self.st, self.sm, 0, 2 * N, self.src)

    def compact(self):
        self.eng.rx_sessions_compact(1, self.csum)

    def plan(self):
        self.eng.rx_plan(self.wire, self.w_off, self.w_len, self.r_desc, self.r_st, self.r_host, self.r_sum, 0)

    def plan_finds_every_live_index(self):
        self.plan()
        self.torch.cuda.synchronize()
        return not bool(self.r_st.any().item()) and (self.r_desc.cpu().numpy()[:, 3] >> 32).astype(np.uint32).tolist() == self.new_slots.tolist()

    def lookup(self, indices):
        torch, dev = self.torch, self.dev
        m = len(indices)
        wire = b"".join(struct.pack("<BxxxIQ", 4, int(i), 0) + bytes(16) for i in indices)
        desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        st, host = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        sm = torch.zeros(2, dtype=torch.int64, device=dev)
        self.eng.rx_plan(torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to(dev), torch.arange(0, 32 * m, 32, dtype=torch.int64, device=dev),
                         torch.full((m,), 32, dtype=torch.int32, device=dev), desc, st, host, sm, 0)
        torch.cuda.synchronize()
        return [int(s) if v == 0 else None for v, s in zip(st.cpu().numpy().tolist(), (desc.cpu().numpy()[:, 3] >> 32).tolist())]


def bench_table(W, torch, dev, profile):
    t = Table(W, torch, dev)
    out, ok = {}, True
    pick = [0, 1, 255, 256, 4097, N // 2, N - 1]
    if profile:
        for _ in range(10):
            t.half_retired()
            t.compact()
            torch.cuda.synchronize()
        t.eng.close()
        return out, ok
    t.half_retired()
    ok &= t.eng.rx_sessions_count() == (N, N) and t.plan_finds_every_live_index()
    out["plan_half_retired"] = timed(torch, t.plan, reps=20, warm=5)
    out["compact"] = timed(torch, t.compact, before=t.half_retired)
    ok &= t.csum.cpu().numpy().tolist() == [N, N, 1, 0] and t.eng.rx_sessions_count() == (N, 0)
    ok &= t.lookup([int(t.new[p]) for p in pick] + [int(t.old[p]) for p in pick] + [5]) == [2 * p + 1 for p in pick] + [None] * (len(pick) + 1)
    ok &= t.plan_finds_every_live_index()
    out["plan_compacted"] = timed(torch, t.plan, reps=20, warm=5)
    out["compact_noop"] = timed(torch, t.compact)
    ok &= t.csum.cpu().numpy().tolist() == [N, 0, 0, 0] and t.eng.rx_sessions_count() == (N, 0)
    walls = []
    for _ in range(6):  # the parent's only way: a rebuild on the host from the lists it holds
        t.half_retired()
        torch.cuda.synchronize()
        w = time.perf_counter()
        t.eng.rx_sessions_set(t.new, t.new_slots)
        walls.append((time.perf_counter() - w) * 1e6)
    ok &= t.eng.rx_sessions_count() == (N, 0)
    out["host_rebuild"] = {"median_us": round(float(np.median(walls[1:])), 1), "min_us": round(min(walls[1:]), 1), "max_us": round(max(walls[1:]), 1)}
    t.eng.close()
    return out, ok


def bench_sweep(W, torch, dev, profile):
    import bench_timers
    out, ok = {}, True
    nd = bench_timers.Node(W, torch, N, 0)
    nd.eng.timers_config_set(W.TimersConfig(reject_after_time=1000, rekey_after_time=900))
    keys = splitmix_np(0x5E0E, 32 * 2 * N)

    def again():
        nd.restart(T0)
        nd.now.fill_(T0 + 1000)

    def again_keyed():  # (wg_keys_set also fills the host's mirror, which the wipe leaves alone: the device table is timed and checked)
        nd.eng.set_keys(0, keys)
        again()

    def sweep(wipe):
        nd.eng.timers_sweep(nd.now, nd.exp, nd.init, nd.keep, nd.sum, wire_stride=32, out_size=32 * N, retire=True, wipe=wipe)

    if profile:
        for _ in range(10):
            again()
            sweep(True)
            torch.cuda.synchronize()
        nd.eng.close()
        return out, ok
    out["retire"] = timed(torch, lambda: sweep(False), before=again)
    ok &= nd.summary() == [N, N, N, N, 0, 0, 0, 0] and nd.eng.rx_sessions_count() == (0, N)
    out["retire_wipe"] = timed(torch, lambda: sweep(True), before=again_keyed)
    ok &= nd.summary() == [N, N, N, N, 0, 0, 0, 0] and nd.eng.rx_sessions_count() == (0, N)
    # every slot was a session's: a sample of the key table through a seal against the oracle under zero keys
    from oracle import oracle as O
    slots = np.array([0, 1, 255, 256, N - 1, N, N + 1, 2 * N - 1], np.uint32)
    desc = W.pack_desc(np.zeros(len(slots), np.uint64), 48 * np.arange(len(slots), dtype=np.uint64), slots.astype(np.uint64), 32, slots)
    pt = splitmix_np(0x5E0F, 32)
    d_ct = torch.zeros(48 * len(slots), dtype=torch.uint8, device=dev)
    nd.eng.seal(torch.from_numpy(W.desc_as_int64(desc)).to(dev), torch.from_numpy(pt).to(dev), d_ct, 32)
    torch.cuda.synchronize()
    ref = np.zeros(48 * len(slots), np.uint8)
    O.seal_batch(desc, pt, ref, np.zeros(32 * 2 * N, np.uint8), threads=1)
    ok &= d_ct.cpu().numpy().tobytes() == ref.tobytes()
    nd.eng.close()
    return out, ok


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"tool": "bench_session_end", "kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return 0
    if "--timers" in sys.argv:
        timers_mode()
        return 0
    ab = None
    if "--ab" in sys.argv:  # (before this process opens the GPU)
        other = sys.argv[sys.argv.index("--ab") + 1]
        ab = [child(other if k % 2 == 0 else None) for k in range(4)]
    W, torch, dev = load()
    profile = "--profile" in sys.argv
    ramp(torch, dev)
    out = {"tool": "bench_session_end", "device": torch.cuda.get_device_name(0), "n": N, "capacity": 4 * N,
           "version": W.lib().wg_version().decode()}
    tab, ok1 = bench_table(W, torch, dev, profile)
    swp, ok2 = bench_sweep(W, torch, dev, profile)
    if profile:
        emit({"tool": "bench_session_end", "profile_pass": 10, "n": N})
        return 0
    out.update({f"{k}_us": v for k, v in tab.items()})
    out.update({f"sweep_{k}_us": v for k, v in swp.items()})
    out["host_rebuild_over_compact"] = round(tab["host_rebuild"]["median_us"] / tab["compact"]["median_us"], 1)
    out["verified"] = bool(ok1 and ok2)
    if ab is not None:
        out["timers_sweep_ab"] = [{"library": r["library"], "verified": r["verified"], "version": r["version"],
                                   "expired_retire_us": r["sweep_65536"]["expired_retire"],
                                   "none_due_us": r["sweep_65536"]["none_due"]} for r in ab]
        out["verified"] = bool(out["verified"] and all(r["verified"] for r in ab))
    emit(out)
    return 0 if out["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
