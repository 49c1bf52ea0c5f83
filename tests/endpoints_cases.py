"""Seeded inputs for the endpoint tests (tests/test_endpoints.py on the model, tests/test_gpu_endpoints.py on the
device): a key table of K slots of which some have no peer, peers at and past max_peers, peers without an endpoint, both
address families, and descriptor rings that hit every one of them."""
import numpy as np

import endpoints_model as EM
from wgtest import splitmix_np

K, P = 150, 70  # key slots, max_peers: 70 peers are more than one wave of them


def _r32(seed, n):
    return np.frombuffer(splitmix_np(seed, 4 * max(n, 1)).tobytes(), "<u4")[:n].astype(np.int64)


def address(p, port=None, v6=None):
    """Peer p's configured endpoint: IPv4 for even p, IPv6 for odd."""
    v6 = bool(p & 1) if v6 is None else v6
    addr = bytes([0x20, 0x01, 0x0D, 0xB8] + [0] * 10 + [p >> 8, p & 255]) if v6 else bytes([10, 9, p >> 8, p & 255])
    return EM.src(addr, 51820 + p if port is None else port)


def slot_map():
    """Slots 0 .. 139 belong to peer s % 75 (70 .. 74: at and past max_peers), 140 .. 149 to none."""
    return [s % 75 if s < 140 else EM.NOPEER for s in range(K)]


def endpoints():
    """Every seventh peer (3, 10, ...) has no endpoint."""
    return [bytes(24) if p % 7 == 3 else address(p) for p in range(P)]


def state():
    m = EM.Endpoints(K, P)
    m.slots_set(0, slot_map())
    m.endpoints_set(0, endpoints())
    return m


def descriptors(n, seed, one_peer=None, sweep_style=False):
    """n wg_pkt descriptors and statuses as wg_tx_plan leaves them: every status code 0 .. 11 (half of them OK),
    WG_LEN_INVALID, keepalives, slots past the key table. sweep_style: a keepalive list padded as wg_timers_sweep pads."""
    r = _r32(seed, 3 * n)
    d = np.zeros(n, EM.PKT_DTYPE)
    status = []
    for j in range(n):
        a, b, c = int(r[3 * j]), int(r[3 * j + 1]), int(r[3 * j + 2])
        slot = a % (K + 10) if one_peer is None else one_peer
        ln = EM.LEN_INVALID if b % 8 == 0 else 0 if b % 8 == 1 else 1 + (b >> 3) % 1400
        st = 0 if c % 2 else (c >> 1) % 12
        if sweep_style:
            live = j < (2 * n) // 3
            d[j] = (0, 48 + 32 * j + 16 if live else 0, j if live else 0, 0 if live else EM.LEN_INVALID, slot if live else 0)
        else:
            d[j] = (128 * j, 64 + 1536 * j + 16, (seed << 8) + j, ln, slot)
        status.append(st)
    return d, (None if sweep_style else status)


def sources(n, seed, spread=True):
    """n datagram sources by batch index, each distinct: both families, a family-0 and a family-9 source, IPv4 sources
    with garbage behind the address and in _pad."""
    r = _r32(seed, n)
    out = []
    for i in range(n):
        a = int(r[i])
        if i % 41 == 7:
            out.append(EM.src(bytes([1, 2, 3, 4]), 7, family=0))
        elif i % 41 == 19:
            out.append(EM.src(bytes([1, 2, 3, 4]), 7, family=9))
        elif a % 3 == 0:
            out.append(EM.src(bytes([0xFD, 0] + [i >> 8, i & 255] * 7), 1024 + i))
        elif a % 3 == 1:
            out.append(EM.src(bytes([172, 16, i >> 8, i & 255]), 1024 + i))
        else:  # the same host as a clean source would be, with garbage where the stored form has zeros
            out.append(EM.src(bytes([172, 16, i >> 8, i & 255]) + bytes([0xA5] * 12), 1024 + i, family=4, pad=bytes([0x5A] * 5)))
    return np.frombuffer(b"".join(out), EM.SRC_DTYPE).copy()


def learn_batch(n, seed, peers):
    """n received descriptors: one in three unauthenticated (every status but OK and KEEPALIVE), the others on slots of
    `peers` peers (1: all on slot 5), some past the key table or on slots without a usable peer."""
    r = _r32(seed, 2 * n)
    d = np.zeros(n, EM.PKT_DTYPE)
    status = []
    bad = [1, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    for i in range(n):
        a, b = int(r[2 * i]), int(r[2 * i + 1])
        slot = 5 if peers == 1 else a % (K + 10)
        d[i] = (0, 0, i, 40, slot)
        status.append(bad[b % 10] if i % 3 == 1 else (EM.PKT_KEEPALIVE if b % 5 == 0 else EM.PKT_OK))
    return d, status
