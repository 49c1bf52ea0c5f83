"""Timing of wg_hs_initiate and of check + wg_hs_finish, with wg_hs_respond on the same box in the same run for
comparison, at 616 and 65,536 entries. Two contexts on one device: A initiates to its peer B, B answers A's records
laid out as a ring (check -> dh -> open -> respond), A checks and finishes B's responses. Reports, after a 150-ms
clock ramp, as the median of 20 calls after 5 warm-ups (HIP events on the launch stream; ephemerals and pending
entries are refreshed from device copies before each timed call, outside the timed region), per size:
  initiate_us        wg_hs_initiate alone: two ladders and a 35-compression chain per entry
  respond_us         wg_hs_respond alone over the same entries: three ladders and 50 compressions
  check_finish_us    wg_hs_check + wg_hs_finish over B's responses: the table, two ladders, 47 compressions
  finish_us          wg_hs_finish alone
A sample of the records, pending entries and established entries is compared with tests/hs_initiate_model.py and
tests/hs_respond_model.py, and the summaries with the batch's make-up (`verified`). `--profile` runs initiate and
check + finish at 65,536 entries 10 times and nothing else, for a kernel-trace run of its own; `--trace FILE.csv`
turns that run's kernel trace into the median time per kernel. One JSON line each; --out appends it to a file."""
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

from bench_tx import splitmix_np  # noqa: E402

KERNELS = ("k_hs_init_dh", "k_hs_init_chain", "k_hs_fin_fill", "k_hs_fin_insert", "k_hs_fin_dh", "k_hs_fin_chain",
           "k_hs_fin_emit", "k_hs_check", "k_hs_emit", "k_rx_scan")
A_PRIV, B_PRIV = bytes(splitmix_np(0x6B00, 32)), bytes(splitmix_np(0x6B01, 32))


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


def main():
    if "--trace" in sys.argv:
        p = sys.argv[sys.argv.index("--trace") + 1]
        emit({"kernel_trace": p.split("/")[-1], "kernels": trace_summary(p)})
        return
    import importlib
    import torch
    assert torch.cuda.is_available(), "bench_hs_initiate needs the MI355X"
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    N = 65536
    A, B = W.Engine(0, key_slots=16), W.Engine(0, key_slots=16)
    a_pub, b_pub = A.hs_static_set(A_PRIV), B.hs_static_set(B_PRIV)
    others = [bytes(splitmix_np(0x6B10 + k, 32)) for k in range(3)]
    A.hs_peers_set(others + [b_pub])  # B is peer 3
    B.hs_peers_set([a_pub])
    A.hs_reserve(N)
    B.hs_reserve(N)
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    eph_host, beph_host = splitmix_np(0x6B20, 32 * N), splitmix_np(0x6B21, 32 * N)
    ts_host = splitmix_np(0x6B22, 12 * N)
    li_host = (np.arange(N, dtype=np.uint32) * np.uint32(40503) + np.uint32(0x01000000)).astype(np.uint32)
    eph_master, beph_master = torch.from_numpy(eph_host).to(dev), torch.from_numpy(beph_host).to(dev)
    ts = torch.from_numpy(ts_host).to(dev)
    li = torch.from_numpy(li_host.view(np.int32)).to(dev)
    bli = torch.from_numpy((li_host + np.uint32(0x40000000)).view(np.int32)).to(dev)
    peer = torch.full((N,), 3, dtype=torch.int32, device=dev)
    version = W.lib().wg_version().decode()

    def timed(f, before=None, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for k in range(warm + reps):
            if before:
                before()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                out.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(out)), 2), round(float(min(out)), 2), round(float(max(out)), 2)

    def rig(n):
        """The buffers and the calls of one size."""
        r = type("R", (), {})()
        r.eph, r.beph = z8(32 * n), z8(32 * n)
        r.st, r.sum, r.rec, r.pend, r.pend_master = z32(n), z32(4), z8(n, 160), z8(n, 112), z8(n, 112)
        r.off148 = torch.arange(0, 148 * n, 148, dtype=torch.int64, device=dev)
        r.len148 = torch.full((n,), 148, dtype=torch.int32, device=dev)
        r.b_hst, r.b_hsum, r.b_rec = z32(n), z32(4), z8(n, 160)
        r.b_sh, r.b_dh, r.b_ost, r.b_init, r.b_osum = z8(n, 32), z32(n), z32(n), z8(n, 144), z32(4)
        r.b_rst, r.b_sess, r.b_rsum = z32(n), z8(n, 176), z32(4)
        r.ring92 = z8(92 * n)
        r.off92 = torch.arange(0, 92 * n, 92, dtype=torch.int64, device=dev)
        r.len92 = torch.full((n,), 92, dtype=torch.int32, device=dev)
        r.f_hst, r.f_hsum, r.f_rec, r.f_st, r.f_est, r.f_sum = z32(n), z32(4), z8(n, 160), z32(n), z8(n, 96), z32(4)
        r.refresh = lambda: r.eph.copy_(eph_master[:32 * n])
        r.initiate = lambda: A.hs_initiate(peer[:n], r.eph, ts[:12 * n], li[:n], r.st, r.rec, r.pend, r.sum)
        r.brefresh = lambda: r.beph.copy_(beph_master[:32 * n])
        r.respond = lambda: B.hs_respond(r.b_init, r.b_osum, r.beph, bli[:n], r.b_rst, r.b_sess, r.b_rsum)
        r.prefresh = lambda: r.pend.copy_(r.pend_master)
        r.check = lambda: A.hs_check(r.ring92, r.off92, r.len92, r.f_hst, r.f_rec, r.f_hsum)
        r.finish = lambda: A.hs_finish(r.f_rec, r.f_hsum, r.pend, r.f_st, r.f_est, r.f_sum)

        def prepare():  # A's initiations, B's entries for them, B's responses as a ring
            r.refresh()
            r.initiate()
            r.pend_master.copy_(r.pend)
            ring = r.rec[:, 8:156].contiguous().reshape(-1)
            B.hs_check(ring, r.off148, r.len148, r.b_hst, r.b_rec, r.b_hsum)
            B.hs_dh(r.b_rec, r.b_hsum, r.b_sh, r.b_dh)
            B.hs_open(r.b_rec, r.b_hsum, r.b_sh, r.b_dh, r.b_ost, r.b_init, r.b_osum)
            r.brefresh()
            r.respond()
            r.ring92.copy_(r.b_sess[:, 16:108].contiguous().reshape(-1))
            torch.cuda.synchronize()
        r.prepare = prepare
        return r

    small = rig(616)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:  # clock ramp
        small.refresh()
        small.initiate()
        torch.cuda.synchronize()

    if "--profile" in sys.argv:
        r = rig(N)
        r.prepare()
        for _ in range(10):
            r.refresh()
            r.initiate()
            r.prefresh()
            r.check()
            r.finish()
            torch.cuda.synchronize()
        emit({"profile_pass": 10, "n": N})
        A.close()
        B.close()
        return

    import hs_initiate_model as IM
    import hs_respond_model as RM
    out = {"version": version, "peers": 4}
    verified = True
    for n in (616, N):
        r = small if n == 616 else rig(n)
        r.prepare()
        res = {}
        res["initiate_us"], *res["initiate_spread_us"] = timed(r.initiate, r.refresh)
        res["respond_us"], *res["respond_spread_us"] = timed(r.respond, r.brefresh)

        def check_finish():
            r.check()
            r.finish()
        res["check_finish_us"], *res["check_finish_spread_us"] = timed(check_finish, r.prefresh)
        r.check()
        res["finish_us"], *res["finish_spread_us"] = timed(r.finish, r.prefresh)
        torch.cuda.synchronize()
        res["initiate_over_respond"] = round(res["initiate_us"] / res["respond_us"], 3)
        res["finish_over_respond"] = round(res["finish_us"] / res["respond_us"], 3)
        verified &= [int(x) for x in r.sum.cpu().numpy()] == [n, 0, 0, 0] and [int(x) for x in r.f_sum.cpu().numpy()] == [n, 0, 0, 0]
        verified &= [int(x) for x in r.b_rsum.cpu().numpy()] == [n, 0, 0, 0] and not bool(r.eph.any().item())
        verified &= not bool(r.pend.any().item())
        rec = r.rec.cpu().numpy().reshape(-1).view(W.WG_HS_RECORD_DTYPE)
        pend = r.pend_master.cpu().numpy().reshape(-1).view(W.WG_HS_PENDING_DTYPE)
        est = r.f_est.cpu().numpy().reshape(-1).view(W.WG_HS_ESTABLISHED_DTYPE)
        sess = r.b_sess.cpu().numpy().reshape(-1).view(W.WG_HS_SESSION_DTYPE)
        for k in (0, n // 2, n - 1):
            e = eph_host[32 * k:32 * k + 32].tobytes()
            want = IM.initiate_one(A_PRIV, b_pub, e, ts_host[12 * k:12 * k + 12].tobytes(), int(li_host[k]))
            verified &= rec[k]["msg"].tobytes() == want["message"] and int(rec[k]["index"]) == k and int(rec[k]["len"]) == 148
            verified &= pend[k]["hash"].tobytes() == want["hash"] and pend[k]["chain_key"].tobytes() == want["chain_key"]
            verified &= pend[k]["ephemeral"].tobytes() == e and int(pend[k]["local_index"]) == int(li_host[k])
            resp = sess[k]["response"].tobytes()
            keys = RM.consume_response(A_PRIV, e, want["hash"], want["chain_key"], resp[12:44], resp[44:60])
            verified &= keys is not None and est[k]["send_key"].tobytes() == keys["send_key"] == sess[k]["recv_key"].tobytes()
            verified &= keys is not None and est[k]["recv_key"].tobytes() == keys["recv_key"] == sess[k]["send_key"].tobytes()
            verified &= int(est[k]["record"]) == k == int(est[k]["pending"]) and int(est[k]["peer"]) == 3
        out[str(n)] = res
    out["verified"] = bool(verified)
    emit(out)
    A.close()
    B.close()


if __name__ == "__main__":
    main()
