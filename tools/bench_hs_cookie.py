"""Timing of the cookie calls (wg_hs_admit, wg_hs_cookie_open, wg_hs_mac2) on the two rings of tools/bench_hs.py:
  flood  65,536 type-1 datagrams of 148 B, back to back; 1% carry a correct mac1;
  mixed  the IMIX wire ring (65,536 slots of 1,536 B) with 1.2% of the slots holding handshake messages, half of them
         with a correct mac1.
Each ring three ways: (a) as it is, no datagram carries a cookie; (b) every valid-mac1 datagram carries a valid mac2
for its source address; (c) every handshake datagram carries a valid mac1 and no cookie (on the flood ring: 65,536
replies, the worst case). Reports, after a 150-ms clock ramp, as the median of 20 calls after 5 warm-ups (HIP events
on the launch stream; the nonces are refilled before each call, outside the timed region):
  admit_<ring>_<a|b|c>_us, check_<ring>_<a|b|c>_us   wg_hs_admit and wg_hs_check on the same ring in the same process
                                                     (flood: identity list; mixed: the list a plan left)
  chain_admit_c_us, chain_check_c_us   plan -> admit | check -> dh -> open -> stamp -> respond on flood ring (c), whose
                                       bodies are random: what a spoofed flood costs either way
  cookie_open_<N>_us, mac2_<N>_us      for N = 616 and 65,536 entries (the replies come from a second context's admit
                                       of the first one's initiations)
One JSON line; --out appends it to a file."""
import hashlib
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_hs  # noqa: E402
from bench_tx import splitmix_np  # noqa: E402

SECRET = bytes(splitmix_np(0x434B, 32))


def mac(key, data):
    return hashlib.blake2s(data, digest_size=16, key=key).digest()


def sources(n):
    """wg_hs_src per datagram: IPv4 and IPv6 alternate, random addresses and ports"""
    s = splitmix_np(0x5243, 24 * n).reshape(n, 24).copy()
    s[:, 18] = np.where(np.arange(n) % 2 == 0, 4, 6)
    return s


def cookie(s):
    return mac(SECRET, s[:4].tobytes() + s[16:18].tobytes() if s[18] == 4 else s[:18].tobytes())


def variants(ring, off, lens, src, hs):
    """(a), (b), (c) of a ring: hs = the indices of its handshake datagrams with a correct mac1 (a, b) / of all its
    handshake datagrams (c)"""
    good, every = hs
    out = {"a": ring}
    b = ring.copy()
    for i in good:
        o, L = int(off[i]), int(lens[i])
        b[o + L - 16:o + L] = np.frombuffer(mac(cookie(src[i]), b[o:o + L - 16].tobytes()), np.uint8)
    out["b"] = b
    c = ring.copy()
    for i in every:
        o, L = int(off[i]), int(lens[i])
        c[o:o + L] = np.frombuffer(bench_hs.with_mac1(c[o:o + L - 32].tobytes()), np.uint8)
    out["c"] = c
    return out


def main():
    import torch
    torch.cuda.is_available()
    W = importlib.import_module("wireguard-java_amd")
    dev = torch.device("cuda", 0)
    n, K, stride, max_len = 65536, 256, 1536, 1500
    B = W.Engine(0, key_slots=K)
    A = W.Engine(0, key_slots=4)
    b_pub = B.hs_static_set(bytes(splitmix_np(0x4242, 32)))
    a_pub = A.hs_static_set(bytes(splitmix_np(0x4141, 32)))
    bench_hs.PUB = b_pub  # the rings' mac1 is for B
    B.hs_peers_set([a_pub])
    A.hs_peers_set([b_pub])
    B.hs_cookie_secret_set(SECRET)
    B.set_keys(0, splitmix_np(3, 32 * K))
    receivers = (np.arange(K, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    B.rx_sessions_set([int(x) for x in receivers], list(range(K)))
    B.rx_reserve(n)
    B.hs_reserve(n)
    B.hs_stamps_set(0, [])
    A.hs_reserve(n)
    src = sources(n)
    f_ring, f_off, f_len, f_good = bench_hs.flood_ring(n)
    good = np.nonzero(splitmix_np(22, 4 * n).view("<u4") % 100 == 0)[0]
    assert len(good) == f_good
    m_ring, m_off, m_len, m_hs, m_good = bench_hs.mixed_ring(n, K, stride, receivers)
    pick = np.nonzero(splitmix_np(13, n) < 3)[0]
    rings = {"flood": (variants(f_ring, f_off, f_len, src, (good, np.arange(n))), f_off, f_len),
             "mixed": (variants(m_ring, m_off, m_len, src, (pick[::2], pick)), m_off, m_len)}
    t8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    t32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    d_src = torch.from_numpy(src).to(dev)
    fresh_nonces = torch.from_numpy(splitmix_np(0x4E4F, 24 * n).reshape(n, 24) | 1).to(dev)
    d_non = t8(n, 24)
    r_desc = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    r_st, r_host, h_st = t32(n), t32(n), t32(n)
    r_sum = torch.zeros(2, dtype=torch.int64, device=dev)
    h_rec, h_sum, h_rep, h_asum = t8(n, 160), t32(4), t8(n, 80), t32(4)
    d_sh, d_dh, d_ost, d_init, d_osum = t8(n, 32), t32(n), t32(n), t8(n, 144), t32(4)
    s_st, s_open, s_fresh, s_sum = t32(n), t8(n, 12), t8(n, 144), t32(4)
    r_eph, r_li, r_rst, r_sess, r_rsum = torch.from_numpy(splitmix_np(0x4550, 32 * n) | 1).to(dev), t32(n), t32(n), t8(n, 176), t32(4)

    def refill():
        d_non.copy_(fresh_nonces)

    def timed(f, pre=None, reps=20, warm=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for k in range(warm + reps):
            if pre:
                pre()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(ts)), 2)

    out = {"n": n, "flood_good": int(f_good), "mixed_handshakes": int(m_hs), "mixed_good": int(m_good)}
    first = True
    for name, (vs, off, lens) in rings.items():
        o, ln = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
        for v, ring in vs.items():
            w = torch.from_numpy(ring).to(dev)
            lst = {}
            if name == "mixed":
                B.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
                lst = dict(host_list=r_host, rx_summary=r_sum)

            def admit():
                B.hs_admit(w, o, ln, d_src, d_non, h_st, h_rec, h_sum, h_rep, h_asum, **lst)

            def check():
                B.hs_check(w, o, ln, h_st, h_rec, h_sum, **lst)

            if first:  # clock ramp
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.15:
                    refill()
                    admit()
                    torch.cuda.synchronize()
                first = False
            out[f"admit_{name}_{v}_us"] = timed(admit, refill)
            out[f"admit_{name}_{v}_counts"] = h_sum.cpu().numpy().tolist() + h_asum.cpu().numpy().tolist()
            out[f"check_{name}_{v}_us"] = timed(check)
            out[f"check_{name}_{v}_valid"] = int(h_sum.cpu().numpy()[0])
            if name == "flood" and v == "c":
                def tail():
                    B.hs_dh(h_rec, h_sum, d_sh, d_dh)
                    B.hs_open(h_rec, h_sum, d_sh, d_dh, d_ost, d_init, d_osum)
                    B.hs_stamp(d_init, d_osum, h_rec, d_sh, s_st, s_open, s_fresh, s_sum)
                    B.hs_respond(s_fresh, s_sum, r_eph, r_li, r_rst, r_sess, r_rsum)

                def chain_admit():
                    B.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
                    B.hs_admit(w, o, ln, d_src, d_non, h_st, h_rec, h_sum, h_rep, h_asum, host_list=r_host, rx_summary=r_sum)
                    tail()

                def chain_check():
                    B.rx_plan(w, o, ln, r_desc, r_st, r_host, r_sum, max_len, packed=False)
                    B.hs_check(w, o, ln, h_st, h_rec, h_sum, host_list=r_host, rx_summary=r_sum)
                    tail()

                out["chain_admit_c_us"] = timed(chain_admit, refill)
                out["chain_admit_c_ladders"] = int(h_sum.cpu().numpy()[0])
                out["chain_check_c_us"] = timed(chain_check)
                out["chain_check_c_ladders"] = int(h_sum.cpu().numpy()[0])
    # ---- the initiator's side: A initiates N entries to B, B's admit makes the replies
    for N in (int(f_good), n):
        peer, li = t32(N), torch.arange(1, N + 1, dtype=torch.int32, device=dev)
        eph = torch.from_numpy(splitmix_np(0x4549, 32 * N) | 1).to(dev)
        a_st, a_rec, a_pend, a_sum = t32(N), t8(N, 160), t8(N, 112), t32(4)
        A.hs_cookies_set(0, [bytes(16)], [False])
        A.hs_initiate(peer, eph, t8(12 * N), li, a_st, a_rec, a_pend, a_sum)
        w = a_rec[:, 8:156].contiguous().reshape(-1)
        o = torch.arange(0, 148 * N, 148, dtype=torch.int64, device=dev)
        ln = torch.full((N,), 148, dtype=torch.int32, device=dev)
        refill()
        B.hs_admit(w, o, ln, d_src[:N], d_non[:N], h_st[:N], h_rec[:N], h_sum, h_rep[:N], h_asum)
        w64 = h_rep[:N, 8:72].contiguous().reshape(-1)
        o64 = torch.arange(0, 64 * N, 64, dtype=torch.int64, device=dev)
        l64 = torch.full((N,), 64, dtype=torch.int32, device=dev)
        c_st, c_lrn, c_sum, m_st, m_sum = t32(N), t8(N, 16), t32(4), t32(N), t32(4)
        out[f"cookie_open_{N}_us"] = timed(lambda: A.hs_cookie_open(w64, o64, l64, a_rec, a_pend, c_st, c_lrn, c_sum))
        out[f"mac2_{N}_us"] = timed(lambda: A.hs_mac2(a_rec, peer, m_st, m_sum))
        out[f"verified_{N}"] = bool(int(c_sum.cpu().numpy()[0]) == N and int(m_sum.cpu().numpy()[0]) == N and
                                    int(h_asum.cpu().numpy()[0]) == N)
    bench_hs.emit(out)
    A.close()
    B.close()


if __name__ == "__main__":
    main()
