"""A Python interpreter of the step programs in wireguard-java_amd/csrc/wg_hs_chain.h: what k_hs_open and
k_hs_resp_chain do with kOpenProgram and kRespProgram, one lane at a time. The programs and the enums' values come
from the header itself (tests/test_hs_chain.py compiles a program that prints them); the operations are restated
here over the BLAKE2s compression function of RFC 7693 3.2, written out without hashlib, and the two AEAD hooks use
the oracle's Python ChaCha20-Poly1305. A wrong table therefore fails against hs_open_model / hs_respond_model on
any machine; a wrong build of a right table fails only in the GPU tests.
"""
from __future__ import annotations

import struct
from types import SimpleNamespace

from wgtest import oracle

M32 = 0xFFFFFFFF
IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
         (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
         (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
         (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
         (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
ZERO_NONCE = bytes(12)
NOPEER = 0xFFFFFFFF
OPEN_OK, OPEN_NEWPEER, OPEN_BADAUTH = 0, 1, 2


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(h, m, t, last):
    """RFC 7693 3.2: F(h, m, t, f), on lists of 32-bit words."""
    v = list(h) + list(IV)
    v[12] ^= t & M32
    v[13] ^= (t >> 32) & M32
    if last:
        v[14] ^= M32

    def g(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & M32
        v[d] = _rotr(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & M32
        v[b] = _rotr(v[b] ^ v[c], 12)
        v[a] = (v[a] + v[b] + y) & M32
        v[d] = _rotr(v[d] ^ v[a], 8)
        v[c] = (v[c] + v[d]) & M32
        v[b] = _rotr(v[b] ^ v[c], 7)

    for s in SIGMA:
        g(0, 4, 8, 12, m[s[0]], m[s[1]])
        g(1, 5, 9, 13, m[s[2]], m[s[3]])
        g(2, 6, 10, 14, m[s[4]], m[s[5]])
        g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]])
        g(1, 6, 11, 12, m[s[10]], m[s[11]])
        g(2, 7, 8, 13, m[s[12]], m[s[13]])
        g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[k] ^ v[k] ^ v[k + 8] for k in range(8)]


def init(outlen, keylen=0):
    """RFC 7693 2.5: the state before the first block."""
    return [IV[0] ^ (outlen | (keylen << 8) | 0x01010000)] + list(IV[1:])


def words(b: bytes, n: int):
    """b as n little-endian words, zeros behind it."""
    return list(struct.unpack(f"<{n}I", bytes(b).ljust(4 * n, b"\0")))


def octets(w) -> bytes:
    return struct.pack(f"<{len(w)}I", *w)


def blake2s(data: bytes):
    """BLAKE2s-256 of a non-empty message, as a state: only for the constants below."""
    h, n = init(32), len(data)
    for off in range(0, n, 64):
        h = compress(h, words(data[off:off + 64], 16), min(off + 64, n), off + 64 >= n)
    return h


CK0 = octets(blake2s(b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s"))
H0 = octets(blake2s(CK0 + b"WireGuard v1 zx2c4 Jason@zx2c4.com"))


def new_chain():
    z = [0] * 8
    return SimpleNamespace(hh=list(z), ck=list(z), x=list(z), ist=list(z), ost=list(z), st=list(z), m=[0] * 16, t=0, last=True)


def prepare(E, c, op, imm, src):
    """wghc::prepare: the generic operations."""
    if op == E.OP_PAD:
        pad = 0x5C5C5C5C if imm & E.PAD_OPAD else 0x36363636
        c.m, c.st, c.t, c.last = [w ^ pad for w in src] + [pad] * 8, init(32), 64, bool(imm & E.PAD_LAST)
    elif op == E.OP_IN32:
        c.m, c.st, c.t, c.last = list(src) + [0] * 8, list(c.ist), 96, True
    elif op == E.OP_OUT:
        c.m, c.st, c.t, c.last = list(c.st) + [0] * 8, list(c.ost), 96, True
    elif op == E.OP_T1:
        c.m, c.st, c.t, c.last = [1] + [0] * 15, list(c.ist), 65, True
    elif op == E.OP_TN:
        c.m, c.st, c.t, c.last = list(src) + [imm] + [0] * 7, list(c.ist), 97, True
    elif op == E.OP_H2:
        c.m, c.st, c.t, c.last = list(c.hh) + list(src), init(32), 64, True
    else:
        raise AssertionError(f"no operation {op}")


def run(E, program, c, sources, own_ops, own_dst=None, jump=None):
    """The kernels' loop. sources: {SRC_*: 32 bytes or a callable giving them} for the kernel's own sources;
    own_ops: {OP_*: f(c, step)} for its own operations (they set m, st, t, last; they may return nothing);
    own_dst: {DST_*: f(c)}; jump(step) -> step: open's skip. A source that nobody supplies is 32 zero bytes."""
    step = 0
    while step < len(program):
        if jump:
            step = jump(step)
        op, arg, imm, dst = program[step]
        if arg == E.SRC_CK:
            src = list(c.ck)
        elif arg == E.SRC_X:
            src = list(c.x)
        else:
            s = sources.get(arg, bytes(32))
            src = words(s() if callable(s) else s, 8)
        if op in own_ops:
            own_ops[op](c, (op, arg, imm, dst))
        else:
            if op == E.OP_PAD and imm & E.PAD_SEAL:
                own_ops["seal"](c)
            prepare(E, c, op, imm, src)
        c.st = compress(c.st, c.m, c.t, c.last)
        if own_dst and dst in own_dst:
            own_dst[dst](c)
        elif dst != E.DST_NONE:
            name = {E.DST_H: "hh", E.DST_X: "x", E.DST_CK: "ck", E.DST_IST: "ist", E.DST_OST: "ost"}[dst]
            setattr(c, name, list(c.st))
        step += 1
    return c


def open_one(E, program, skip, local_private, local_public, ephemeral, enc_static, enc_ts, ss, peers, x25519, wave_known=None):
    """k_hs_open's lane, in hs_open_model.open_one's terms. skip = (kOpenStaticBegin, kOpenStaticEnd). wave_known:
    whether some lane of the wave has a known peer (None: this lane alone decides); a lane without a peer in such
    a wave runs the static-static KDF over zeros and drops its result."""
    O = oracle()
    peers = [bytes(p) for p in peers]
    c = new_chain()
    c.ist = compress(init(32), words(bytes(b ^ 0x36 for b in CK0) + b"\x36" * 32, 16), 64, False)  # kCk0Ipad
    c.ost = compress(init(32), words(bytes(b ^ 0x5C for b in CK0) + b"\x5c" * 32, 16), 64, False)  # kCk0Opad
    hs0 = octets(blake2s(H0 + bytes(local_public)))
    lane = SimpleNamespace(auth=False, peer=0, rs=None, any_known=False)

    def op_h0(c, s):
        c.m, c.st, c.t, c.last = words(hs0 + bytes(ephemeral), 16), init(32), 64, True

    def op_es1(c, s):
        lane.rs = O.py_aead_open(octets(c.st), ZERO_NONCE, bytes(enc_static), octets(c.hh))
        lane.auth = lane.rs is not None
        if lane.auth and lane.rs in peers:
            lane.peer = peers.index(lane.rs) + 1
        lane.any_known = bool(lane.peer) if wave_known is None else wave_known
        c.m, c.st, c.t, c.last = list(c.hh) + words(enc_static[:32], 8), init(32), 64, False

    def op_es2(c, s):
        c.m, c.t, c.last = words(enc_static[32:48], 16), 80, True

    def op_ts(c, s):
        c.m, c.st, c.t, c.last = list(c.hh) + words(enc_ts, 8), init(32), 60, True

    def ck_if_peer(c):
        if lane.peer:
            c.ck = list(c.st)

    def jump(step):
        return skip[1] if step == skip[0] and not lane.any_known else step

    run(E, program, c, {E.SRC_E: ephemeral, E.SRC_SS: ss,
                        E.SRC_STATIC: lambda: x25519(local_private, lane.rs) if lane.peer else bytes(32)},
        {E.OP_H0: op_h0, E.OP_ES1: op_es1, E.OP_ES2: op_es2, E.OP_TS: op_ts}, {E.DST_CK_IF_PEER: ck_if_peer}, jump)
    if not lane.auth:
        return OPEN_BADAUTH, None
    return (OPEN_OK if lane.peer else OPEN_NEWPEER), dict(remote_static=lane.rs, hash=octets(c.hh), chain_key=octets(c.ck),
                                                           peer=lane.peer - 1 if lane.peer else NOPEER)


def respond_one(E, program, hash_, chain_key, remote_ephemeral, remote_static, ephemeral, local_index, sender_index, x25519,
                public_key):
    """k_hs_resp_dh's three ladders and k_hs_resp_chain's lane, in hs_respond_model.respond_one's terms."""
    O = oracle()
    epub = public_key(ephemeral)
    c = new_chain()
    c.hh, c.ck = words(hash_, 8), words(chain_key, 8)
    lane = SimpleNamespace(tag=bytes(16))
    head = bytes([2, 0, 0, 0]) + int(local_index).to_bytes(4, "little") + int(sender_index).to_bytes(4, "little") + epub

    def seal(c):
        lane.tag = O.py_aead_seal(octets(c.x), ZERO_NONCE, b"", octets(c.hh))
        assert len(lane.tag) == 16

    def op_mac1key(c, s):
        c.m, c.st, c.t, c.last = words(b"mac1----" + bytes(remote_static), 16), init(32), 40, True

    def op_mac1a(c, s):
        c.m, c.st, c.t, c.last = list(c.ist) + [0] * 8, init(16, 32), 64, False

    def op_mac1b(c, s):
        c.m, c.t, c.last = words(head + lane.tag, 16), 124, True

    run(E, program, c, {E.SRC_EPUB: epub, E.SRC_EE: x25519(ephemeral, remote_ephemeral), E.SRC_ES: x25519(ephemeral, remote_static)},
        {E.OP_MAC1KEY: op_mac1key, E.OP_MAC1A: op_mac1a, E.OP_MAC1B: op_mac1b, "seal": seal})
    response = head + lane.tag + octets(c.st)[:16] + bytes(16)
    return dict(response=response, send_key=octets(c.x), recv_key=octets(c.ck))
