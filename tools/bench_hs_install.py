"""Timing of wg_hs_install over 65,536 sessions (wg_hs_session entries with splitmix keys, one position, one
local_index and two key slots each; the table reserved for them, C = 262,144), against the way without it over the
same sessions, and wg_hs_respond's own time over as many entries as the scale. Reports, after a 150-ms clock ramp:
  install_us        wg_hs_install alone, median (min, max) of 10 calls after 3 warm-ups, HIP events on the launch
                    stream; the table is emptied (wg_rx_sessions_set of nothing) and the entries are restored from a
                    device copy before each call, outside the timed region
  host_path_us      wall time, median of 5: the sessions copied to the host, wg_keys_set of the one run of 2 n slots,
                    wg_rx_sessions_set of the n indices (what a host does after wg_hs_respond without the install);
                    host_d2h_us / host_keys_set_us / host_sessions_set_us are its parts, host_bytes_d2h / _h2d the
                    bytes that cross PCIe (keys twice)
  respond_us        wg_hs_respond over 65,536 entries, median of 5 (the scale: the install follows one respond)
`verified`: every status OK, the summary, the table's count, and on a sample the table through wg_rx_plan and the key
table through a seal against the oracle. `--ab OTHER_LIB` first runs, in fresh child processes, `--host` (the host path
and the respond) under OTHER_LIB (the parent commit's library), and tools/bench_rx_plan.py's plan times alternately
under OTHER_LIB and this library, twice each (`--plan` is that child's mode): rx_session() gained a compare, and the
plan must cost what it did, within that tool's own run-to-run spread. `--profile` runs the install 10 times and nothing
else, for a kernel-trace run of its own; `--trace FILE.csv` turns that run's kernel trace into the median time per
kernel. One JSON line each; --out appends it to a file."""
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

KERNELS = ("k_inst_fill", "k_inst_claim", "k_inst_insert", "k_inst_count", "k_inst_commit")
N = 65536


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


def child(mode, other):
    env = dict(os.environ)
    if other:
        env["WG_LIB_PATH"] = os.path.abspath(other)
    else:
        env.pop("WG_LIB_PATH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, stdout=subprocess.PIPE, timeout=400)
    if p.returncode != 0:
        raise SystemExit(f"{mode} under {'the other' if other else 'this'} library ended with {p.returncode}")
    r = json.loads(p.stdout.decode().strip().splitlines()[-1])
    r["library"] = "other" if other else "this"
    return r


def load():
    """The package, bound to what the library in use exports (the parent's lacks this commit's symbols)."""
    import ctypes
    import importlib
    import torch
    assert torch.cuda.is_available(), "bench_hs_install needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    have = ctypes.CDLL(W._lib.LIB_PATH)
    W._lib.SIGNATURES[:] = [sig for sig in W._lib.SIGNATURES if hasattr(have, sig[0])]
    return W, torch, torch.device("cuda", 0)


def sessions(W):
    """65,536 wg_hs_session entries: position p at entry p, keys and every other byte from splitmix."""
    ent = np.frombuffer(splitmix_np(0x1A57, 176 * N).tobytes(), W.WG_HS_SESSION_DTYPE).copy()
    ent["init"] = np.arange(N, dtype=np.uint32)
    ent["local_index"] = (np.arange(N, dtype=np.uint32) * np.uint32(40503) + np.uint32(0x01000000)).astype(np.uint32)
    return ent


def host_mode():
    """The host path and the respond, under whichever library is loaded."""
    W, torch, dev = load()
    eng = W.Engine(0, key_slots=2 * N)
    ent = sessions(W)
    d_sess = torch.from_numpy(ent.view(np.uint8).reshape(N, 176)).to(dev)
    eng.rx_sessions_set([1], [0])
    torch.cuda.synchronize()
    parts = []
    for _ in range(6):
        t0 = time.perf_counter()
        h = d_sess.cpu().numpy().reshape(-1).view(W.WG_HS_SESSION_DTYPE)
        t1 = time.perf_counter()
        keys = np.ascontiguousarray(np.stack([h["send_key"], h["recv_key"]], axis=1)).reshape(-1)  # slots 2 p, 2 p + 1
        eng.set_keys(0, keys)
        t2 = time.perf_counter()
        eng.rx_sessions_set(h["local_index"], np.arange(1, 2 * N, 2, dtype=np.uint32))
        t3 = time.perf_counter()
        parts.append([(t3 - t0) * 1e6, (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6])
    med = np.median(np.array(parts[1:]), axis=0)
    out = {"host": True, "n": N, "version": W.lib().wg_version().decode(), "host_path_us": round(float(med[0]), 1),
           "host_d2h_us": round(float(med[1]), 1), "host_keys_set_us": round(float(med[2]), 1),
           "host_sessions_set_us": round(float(med[3]), 1), "host_bytes_d2h": 176 * N, "host_bytes_h2d": 64 * N + 8 * 4 * N}
    # the scale: one wg_hs_respond over as many entries (the caller vouches for them: every one is answered)
    eng.hs_static_set(bytes(splitmix_np(0x1A58, 32)))
    eng.hs_peers_set([bytes(splitmix_np(0x1A59, 32))])
    inits = np.frombuffer(splitmix_np(0x1A5A, 144 * N).tobytes(), W.WG_HS_INIT_DTYPE).copy()
    inits["peer"] = 0
    d_init = torch.from_numpy(inits.view(np.uint8).reshape(N, 144)).to(dev)
    eph_master = torch.from_numpy(splitmix_np(0x1A5B, 32 * N)).to(dev)
    eph = torch.zeros(32 * N, dtype=torch.uint8, device=dev)
    li = torch.from_numpy(ent["local_index"].view(np.int32).copy()).to(dev)
    st, sm = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for k in range(7):
        eph.copy_(eph_master)
        a.record()
        eng.hs_respond(d_init, None, eph, li, st, d_sess, sm, skip_newpeer=False)
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(a.elapsed_time(b) * 1e3)
    out["respond_us"], out["respond_n_ok"] = round(float(np.median(ts)), 1), int(sm.cpu().numpy()[0])
    print(json.dumps(out))
    eng.close()


def plan_mode():
    """tools/bench_rx_plan.py as it stands, under whichever library is loaded; its plan times."""
    load()
    import contextlib
    import io
    import bench_rx_plan
    sys.argv = [sys.argv[0]]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench_rx_plan.main()
    r = json.loads(buf.getvalue().strip().splitlines()[-1])
    print(json.dumps({k: r[k] for k in r if k.startswith("plan_") or k in ("deliver_us", "planned_us", "version")}))


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return
    if "--host" in sys.argv:
        return host_mode()
    if "--plan" in sys.argv:
        return plan_mode()
    ab = None
    if "--ab" in sys.argv:  # (before this process opens the GPU)
        other = sys.argv[sys.argv.index("--ab") + 1]
        ab = {"parent": child("--host", other), "rx_plan": [child("--plan", other if k % 2 == 0 else None) for k in range(4)]}
    W, torch, dev = load()
    L = W._lib
    K = 2 * N
    eng = W.Engine(0, key_slots=K)
    eng.replay_enable(2048)
    eng.tx_counters_set(0, [0])  # the transmit state exists: its counters are reset too
    eng.rx_sessions_reserve(N)
    eng.rx_reserve(4096)
    ent = sessions(W)
    master = torch.from_numpy(ent.view(np.uint8).reshape(N, 176)).to(dev)
    d_sess = torch.zeros_like(master)
    send = torch.arange(0, K, 2, dtype=torch.int32, device=dev)
    recv = torch.arange(1, K, 2, dtype=torch.int32, device=dev)
    receivers = torch.zeros(K, dtype=torch.int32, device=dev)
    st, sm = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)

    def refresh():
        eng.rx_sessions_set([], [])
        d_sess.copy_(master)

    def install():
        eng.hs_install(d_sess, None, send, recv, st, sm, 0, K, L.WG_HS_INSTALL_SESSIONS, receivers=receivers)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        refresh()
        install()
        torch.cuda.synchronize()
    if "--profile" in sys.argv:
        for _ in range(10):
            refresh()
            install()
            torch.cuda.synchronize()
        emit({"profile_pass": 10, "n": N})
        eng.close()
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for k in range(13):
        refresh()
        a.record()
        install()
        b.record()
        torch.cuda.synchronize()
        if k >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    out = {"n": N, "capacity": 4 * N, "version": W.lib().wg_version().decode(), "install_us": round(float(np.median(ts)), 2),
           "install_spread_us": [round(float(min(ts)), 2), round(float(max(ts)), 2)], "bytes_over_pcie": 0}
    # verified
    ok = not bool(st.any().item()) and sm.cpu().numpy().tolist() == [N, 0, 0, 0] and eng.rx_sessions_count() == (N, 0)
    ok &= not bool(d_sess[:, 112:].any().item()) and bool((d_sess[:, :112] == master[:, :112]).all().item())
    ok &= bool((receivers[0::2].cpu().numpy().view(np.uint32) == ent["remote_index"]).all())
    pick = [0, 1, 255, 256, 4097, N // 2, N - 1]
    wire = b"".join(struct.pack("<BxxxIQ", 4, int(ent["local_index"][p]), 0) + bytes(16) for p in pick) + struct.pack("<BxxxIQ", 4, 5, 0) + bytes(16)
    m = len(pick) + 1
    r_desc = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    r_st, r_host = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.rx_plan(torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to(dev), torch.arange(0, 32 * m, 32, dtype=torch.int64, device=dev),
                torch.full((m,), 32, dtype=torch.int32, device=dev), r_desc, r_st, r_host, r_sum, 0)
    torch.cuda.synchronize()
    ok &= r_st.cpu().numpy().tolist() == [0] * len(pick) + [L.WG_PKT_NOSESSION]
    ok &= (r_desc.cpu().numpy()[:len(pick), 3] >> 32).tolist() == [2 * p + 1 for p in pick]
    from oracle import oracle as O
    slots = np.array([s for p in pick for s in (2 * p, 2 * p + 1)], np.uint32)
    table = np.zeros(32 * K, np.uint8)
    for p in pick:
        table[64 * p:64 * p + 32], table[64 * p + 32:64 * p + 64] = ent["send_key"][p], ent["recv_key"][p]
    desc = W.pack_desc(np.zeros(len(slots), np.uint64), 48 * np.arange(len(slots), dtype=np.uint64), slots.astype(np.uint64), 32, slots)
    pt = splitmix_np(0x1A5C, 32)
    d_ct = torch.zeros(48 * len(slots), dtype=torch.uint8, device=dev)
    eng.seal(torch.from_numpy(W.desc_as_int64(desc)).to(dev), torch.from_numpy(pt).to(dev), d_ct, 32)
    torch.cuda.synchronize()
    ref = np.zeros(48 * len(slots), np.uint8)
    O.seal_batch(desc, pt, ref, table, threads=1)
    ok &= d_ct.cpu().numpy().tobytes() == ref.tobytes()
    out["verified"] = bool(ok)
    if ab is not None:
        out["parent"] = ab["parent"]
        out["rx_plan_ab"] = ab["rx_plan"]
        out["host_over_install"] = round(ab["parent"]["host_path_us"] / out["install_us"], 1)
        out["install_over_respond"] = round(out["install_us"] / ab["parent"]["respond_us"], 4)
    emit(out)
    eng.close()


if __name__ == "__main__":
    main()
