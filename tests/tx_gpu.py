"""What the transmit-plan GPU modules share (tests/test_gpu_tx.py, tests/test_gpu_tx_edges.py): an engine
of their own with one key and one receiver index per slot, a tun ring from a packet list, wg_tx_plan with
guard records behind its outputs, the seal into a wire ring and the frozen oracle's ring for the model's
descriptors."""
import ipaddress

import numpy as np

import tx_model as M
from wgtest import oracle, splitmix_np, wg

KEY_SLOTS = 4096
FILL = 0x5A  # wire rings start as this byte: an untouched slot must still hold it
GUARD = 0x7E


def open_rig(key_seed=0x7C5):
    """A module's own engine (its send counters, peers and routes must not leak into other files'
    tests), one key per slot and a receiver index per slot. Close rig.eng when done."""
    import torch
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    W = wg()
    eng = W.Engine(0, key_slots=KEY_SLOTS)
    keys = splitmix_np(key_seed, 32 * KEY_SLOTS)
    eng.set_keys(0, keys)
    receivers = (np.arange(KEY_SLOTS, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17)).astype(np.uint32)
    eng.set_receivers(torch.from_numpy(receivers.view(np.int32)).to(dev))
    return type("Rig", (), dict(eng=eng, keys=keys, receivers=receivers, torch=torch, dev=dev, W=W))


def ring_of(pkts):
    """Tun ring with the packets 16-byte aligned; returns (ring, offsets, lengths)."""
    lens = np.array([len(p) for p in pkts], np.int64)
    sizes = ((lens + 15) // 16) * 16
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(pkts) else np.zeros(0, np.int64)
    ring = np.zeros(int(sizes.sum()) + 16, np.uint8)
    for o, p in zip(off, pkts):
        ring[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    return ring, off, lens


def plan(rig, ring, off, lens, n_desc, *, route, stride, out_size, max_len, wire_base=0, stream=None):
    """Runs wg_tx_plan; returns (desc as WG_PKT array, status list, device desc tensor). The output
    arrays carry guard records after n_desc entries, which must stay intact."""
    torch, dev = rig.torch, rig.dev
    d_ring = torch.from_numpy(ring).to(dev)
    d_off = torch.from_numpy(np.asarray(off, np.int64)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int64).astype(np.uint32).view(np.int32)).to(dev)
    d_desc = torch.full((n_desc + 2, 4), -0x0101010101010102, dtype=torch.int64, device=dev)
    d_st = torch.full((n_desc + 4,), GUARD, dtype=torch.int32, device=dev)
    rig.eng.tx_plan(d_ring, d_off, d_len, d_desc[:n_desc], d_st[:n_desc], stride, out_size, max_len, route=route,
                    wire_base=wire_base, stream=stream)
    torch.cuda.synchronize()
    h_desc, h_st = d_desc.cpu().numpy(), d_st.cpu().numpy()
    assert (h_desc[n_desc:] == -0x0101010101010102).all(), "descriptor guard overwritten"
    assert (h_st[n_desc:] == GUARD).all(), "status guard overwritten"
    desc = np.ascontiguousarray(h_desc[:n_desc]).view(M.WG_PKT).reshape(-1)
    return desc, h_st[:n_desc].tolist(), (d_ring, d_desc[:n_desc])


def oracle_ring(rig, model_desc, ring, out_size, max_len):
    O = oracle()
    ref = np.full(out_size, FILL, np.uint8)
    ok = np.ascontiguousarray(model_desc[model_desc["len"] != M.LEN_INVALID])
    if len(ok):
        O.seal_batch(ok, ring, ref, rig.keys, threads=4)
        O.frame_headers(ok, rig.receivers, ref, KEY_SLOTS, len(ring), max_len)
    return ref


def seal(rig, d_desc, d_ring, out_size, max_len, uniform=False):
    out = rig.torch.full((out_size,), FILL, dtype=rig.torch.uint8, device=rig.dev)
    rig.eng.seal(d_desc, d_ring, out, max_len, uniform=uniform, frame=True)
    rig.torch.cuda.synchronize()
    return out.cpu().numpy()


def same_desc(got, want):
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]][:5]


def ipv4(dst, total, rng):
    p = bytearray(rng.bytes(max(total, 20)))
    p[0] = 0x45
    p[16:20] = ipaddress.ip_address(dst).packed
    return bytes(p[:total])


def ipv6(dst, total, rng):
    p = bytearray(rng.bytes(max(total, 40)))
    p[0] = 0x60 | (p[0] & 0x0F)
    p[24:40] = ipaddress.ip_address(dst).packed
    return bytes(p[:total])


def counters(rig, slots):
    return {int(s): int(rig.eng.tx_counters_get(int(s), 1)[0]) for s in slots}
