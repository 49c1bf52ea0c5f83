"""ax.xz.wireguard.noise.crypto mirror: ChaCha20, Poly1305, ChaCha20Poly1305, Crypto.

Every arithmetic call goes to the device (libwgaead); nothing is computed on the
host. "MemorySegment" arguments are Python buffers: bytes for inputs, and
writable buffers (bytearray, memoryview, numpy uint8) for outputs, which are
filled in place exactly like the Java code fills its output segments.
"""
from __future__ import annotations

import struct

import numpy as np

from .. import _lib as L
from ..engine import default_engine


class BadPaddingException(Exception):
    """javax.crypto.BadPaddingException"""


class AEADBadTagException(BadPaddingException):
    """javax.crypto.AEADBadTagException (thrown by ChaCha20Poly1305.java:51-53)"""


class IllegalStateException(Exception):
    """java.lang.IllegalStateException (Poly1305.java:114-119, 138-143)"""


class Crypto:
    """Constants of Crypto.java:8-14."""
    POLY1305_TAG_SIZE = 16
    ChaChaPoly1305NonceSize = 12
    ChaChaPoly1305Overhead = 16
    BLAKE2S_BLOCKBYTES = 64

    @staticmethod
    def TAI64N(millis: int | None = None) -> bytes:
        """Crypto.TAI64N (Crypto.java:19-27): the long currentTimeMillis() * 1000 + 4611686018427387914 written
        big-endian into the last 8 of 12 bytes; the first 4 stay zero (the long is positive, so its arithmetic
        shifts bring in zeros). millis: the clock's value, None for now."""
        if millis is None:
            import time
            millis = time.time_ns() // 1_000_000
        return bytes(4) + ((millis * 1000 + 4611686018427387914) & 0x7FFFFFFFFFFFFFFF).to_bytes(8, "big")

    @staticmethod
    def HMAC(sum, key, *messages) -> None:
        """Crypto.HMAC (Crypto.java:39-71): sum = HMAC-BLAKE2s(key, messages...) over the 64-byte block, the two
        hashes on the device (wg_blake2s_batch). A key longer than a block is hashed first; the digest is
        cut to sum's size, as digest(sum, 0, sum.length) cuts it."""
        k = _bytes(key)
        if len(k) > Crypto.BLAKE2S_BLOCKBYTES:
            k = BLAKE2s256(k)
        padded = k + bytes(Crypto.BLAKE2S_BLOCKBYTES - len(k))
        inner = BLAKE2s256(bytes(b ^ 0x36 for b in padded), *messages)
        _write(sum, BLAKE2s256(bytes(b ^ 0x5C for b in padded), inner)[:_size(sum)])

    @staticmethod
    def deriveKey(salt, IKM, n: int = 1) -> bytes:
        """Crypto.deriveKey (Crypto.java:74-99): T(n) of HKDF(salt, IKM) with empty info."""
        if n < 1:
            raise IndexError("n")  # T[n - 1] of an empty array
        prk = bytearray(32)
        Crypto.HMAC(prk, salt, IKM)
        t = bytearray(32)
        for i in range(1, n + 1):
            Crypto.HMAC(t, prk, bytes(t) if i > 1 else b"", b"", bytes([i]))
        return bytes(t)


def _bytes(seg) -> bytes:
    if seg is None:
        return b""
    if isinstance(seg, np.ndarray):
        return seg.astype(np.uint8, copy=False).tobytes()
    return bytes(seg)


def _write(dst, data: bytes) -> None:
    """Copy `data` into the leading bytes of the writable buffer `dst`."""
    if isinstance(dst, np.ndarray):
        dst.reshape(-1).view(np.uint8)[: len(data)] = np.frombuffer(data, np.uint8)
        return
    mv = memoryview(dst).cast("B")
    mv[: len(data)] = data


def _size(seg) -> int:
    if isinstance(seg, np.ndarray):
        return seg.nbytes
    return memoryview(seg).nbytes


def _nonce_words(nonce: bytes) -> list[int]:
    return list(struct.unpack("<3I", nonce))


class ChaCha20:
    """ChaCha20.java: state layout helpers + the chacha_cipher downcalls, on the device."""

    @staticmethod
    def initializeState(key, nonce, state, counter: int) -> None:
        """ChaCha20.java:55-74 (state = constants || key || counter || nonce, LE words)."""
        if _size(state) != 64:
            raise ValueError(f"State size must be 64 bytes (is {_size(state)})")
        words = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", _bytes(key)))
        words += [counter & 0xFFFFFFFF] + _nonce_words(_bytes(nonce))
        _write(state, struct.pack("<16I", *words))

    @staticmethod
    def _cipher(key: bytes, nonce: bytes, data: bytes, counter: int) -> bytes:
        d = L.WgAeadDesc()
        d.len = len(data)
        d.ctr0 = counter & 0xFFFFFFFF
        d.nonce[:] = _nonce_words(nonce)
        out, _ = default_engine().aead_host(L.WG_MODE_CIPHER, [d], key, data, b"", len(data))
        return out

    @staticmethod
    def chacha20Block(state, output, counter: int) -> None:
        """ChaCha20.java:85-104: sets word 12 = counter and writes one 64-byte keystream block."""
        st = bytearray(_bytes(state))
        st[48:52] = struct.pack("<I", counter & 0xFFFFFFFF)
        _write(state, bytes(st))
        ks = ChaCha20._cipher(bytes(st[16:48]), bytes(st[52:64]), bytes(64), counter)
        _write(output, ks)

    @staticmethod
    def chacha20(key, nonce, input, output, counter: int) -> None:
        """ChaCha20.java:116-131: output = input ^ keystream(counter, counter+1, ...)."""
        data = _bytes(input)
        if _size(output) < len(data):
            raise ValueError("Output buffer must be at least as large as input buffer")
        _write(output, ChaCha20._cipher(_bytes(key), _bytes(nonce), data, counter))


class Poly1305:
    """Poly1305.java: init / update / finish. Updates are buffered and the MAC is
    evaluated on the device at finish (one-shot, same result as donna streaming)."""

    def __init__(self, context=None):
        self._key: bytes | None = None
        self._buf = bytearray()
        self.initialised = False
        self.finished = False

    def init(self, key) -> None:
        self._key = _bytes(key)[:32]
        self._buf = bytearray()
        self.initialised = True
        self.finished = False

    def update(self, message) -> None:
        if self.finished:
            raise IllegalStateException("Poly1305 context has already been finished")
        if not self.initialised:
            raise IllegalStateException("Poly1305 context has not been initialised")
        self._buf += _bytes(message)

    def finish(self, mac=None):
        if self.finished:
            raise IllegalStateException("Poly1305 context has already been finished")
        if not self.initialised:
            raise IllegalStateException("Poly1305 context has not been initialised")
        d = L.WgAeadDesc()
        d.len = len(self._buf)
        tag, _ = default_engine().aead_host(L.WG_MODE_MAC, [d], self._key, bytes(self._buf), b"", 16)
        self.finished = True
        self._key = None
        if mac is None:
            return tag
        _write(mac, tag)
        return None


class ChaCha20Poly1305:
    """ChaCha20Poly1305.java:10-98 (RFC 8439 AEAD) on the device."""

    @staticmethod
    def poly1305ChaChaKeyGen(*args):
        """(key, nonce) -> bytes[32], or (stateBuffer, key, nonce, output) (ChaCha20Poly1305.java:11-29)."""
        if len(args) == 2:
            key, nonce = args
            ks = ChaCha20._cipher(_bytes(key), _bytes(nonce), bytes(64), 0)
            return ks[:32]
        state, key, nonce, output = args
        ChaCha20.initializeState(key, nonce, state, 0)
        ChaCha20.chacha20Block(state, output, 0)
        return None

    @staticmethod
    def poly1305AeadEncrypt(*args) -> None:
        """([aad,] key, nonce, plaintext, ciphertext, tag) (ChaCha20Poly1305.java:31-38)."""
        aad, key, nonce, pt, ct, tag = args if len(args) == 6 else (None, *args)
        p = _bytes(pt)
        d = L.WgAeadDesc()
        d.len = len(p)
        a = _bytes(aad)
        d.aad_len = len(a)
        d.nonce[:] = _nonce_words(_bytes(nonce))
        out, _ = default_engine().aead_host(L.WG_MODE_SEAL, [d], _bytes(key), p, a, len(p) + 16)
        _write(ct, out[: len(p)])
        _write(tag, out[len(p):])

    @staticmethod
    def poly1305AeadDecrypt(*args) -> None:
        """([aad,] key, nonce, ciphertext, plaintext, tag); raises AEADBadTagException and leaves
        plaintext untouched on a mismatch (ChaCha20Poly1305.java:40-60)."""
        aad, key, nonce, ct, pt, tag = args if len(args) == 6 else (None, *args)
        c = _bytes(ct)
        t = _bytes(tag)[:16]
        d = L.WgAeadDesc()
        d.len = len(c)
        a = _bytes(aad)
        d.aad_len = len(a)
        d.nonce[:] = _nonce_words(_bytes(nonce))
        out, status = default_engine().aead_host(L.WG_MODE_OPEN, [d], _bytes(key), c + t, a, len(c))
        if status[0] != L.WG_PKT_OK:
            raise AEADBadTagException(f"Invalid tag (got {list(t)})")
        _write(pt, out)


class Blake2s:
    """Blake2s.java: BLAKE2s (RFC 7693) with the reference's constructor, update and digest. Updates
    are buffered and the hash is evaluated on the device at digest (wg_blake2s_batch); the instance
    is reset afterwards, as engineDigest does (Blake2s.java:129-142)."""

    BLOCK_LENGTH = 64

    def __init__(self, digestLength: int, key=b""):
        key = _bytes(key) if key is not None else None
        if key is None:
            raise TypeError("key is null")  # NullPointerException
        if not len(key) <= 32:
            raise ValueError("key's length must be at most 32")  # Blake2s.java:74-75
        if not 1 <= digestLength <= 32:
            raise ValueError("digestLength must be in [1, 32]")  # Blake2s.java:77-78
        self.digestLength = digestLength
        self._key = key
        self._buf = bytearray()

    @staticmethod
    def algorithm() -> str:
        return "BLAKE2s"

    def reset(self) -> None:
        self._buf = bytearray()

    def update(self, input, off: int | None = None, len_: int | None = None) -> None:
        """update(byte), update(bytes) or update(bytes, off, len) (Blake2s.java:104-127)."""
        if isinstance(input, int):
            self._buf.append(input & 0xFF)
            return
        data = _bytes(input)
        if off is not None or len_ is not None:
            off, len_ = off or 0, len(data) - (off or 0) if len_ is None else len_
            if len_ < 0 or off < 0 or off + len_ > len(data):
                raise IndexError("off or len out of bounds")  # Blake2s.java:112-114
            data = data[off:off + len_]
        self._buf += data

    def digest(self, *data) -> bytes:
        for d in data:
            self.update(d)
        out = default_engine().blake2s_host([(bytes(self._buf), self._key, self.digestLength)])[0]
        self.reset()
        return out


def BLAKE2s256(*data) -> bytes:
    """Crypto.BLAKE2s256: the unkeyed 32-byte digest of the concatenated arguments."""
    return default_engine().blake2s_host([(b"".join(_bytes(d) for d in data), b"", 32)])[0]


def calculate_mac1(message_without_macs, public_key) -> bytes:
    """InitiationPacket.calculateMac1 (InitiationPacket.java:110-120; ResponsePacket.java:107-117):
    BLAKE2s-128 of the message without its two MACs under BLAKE2s-256("mac1----" || the receiver's
    static public key), for the outgoing side."""
    key = BLAKE2s256(b"mac1----", _bytes(public_key))
    return default_engine().blake2s_host([(_bytes(message_without_macs), key, 16)])[0]


def HChaCha20(key, nonce16) -> bytes:
    """HChaCha20 (draft-irtf-cfrg-xchacha-03 2.2): the 20 ChaCha rounds over {constants, key, nonce16} without the
    final addition; state words 0-3 and 12-15. The rounds run on the device: a keystream block is the rounds' output
    plus the input state, so the input words are taken off again."""
    k, n = _bytes(key), _bytes(nonce16)
    if len(k) != 32 or len(n) != 16:
        raise ValueError("HChaCha20 takes a 32-byte key and a 16-byte nonce")
    ks = struct.unpack("<16I", ChaCha20._cipher(k, n[4:], bytes(64), struct.unpack("<I", n[:4])[0]))
    st = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574) + struct.unpack("<8I", k) + struct.unpack("<4I", n)
    return struct.pack("<8I", *[(ks[j] - st[j]) & 0xFFFFFFFF for j in (0, 1, 2, 3, 12, 13, 14, 15)])


class XChaCha20Poly1305:
    """XChaCha20-Poly1305 (draft-irtf-cfrg-xchacha-03): HChaCha20, then ChaCha20Poly1305 under the subkey with the
    nonce 0^4 || nonce24[16 .. 24). What a cookie reply is sealed with."""

    @staticmethod
    def _sub(key, nonce24):
        n = _bytes(nonce24)
        if len(n) != 24:
            raise ValueError("an XChaCha20 nonce is 24 bytes")
        return HChaCha20(key, n[:16]), bytes(4) + n[16:]

    @staticmethod
    def seal(key, nonce24, plaintext, aad=b"") -> bytes:
        """ciphertext || tag"""
        sub, n12 = XChaCha20Poly1305._sub(key, nonce24)
        p = _bytes(plaintext)
        ct, tag = bytearray(len(p)), bytearray(16)
        ChaCha20Poly1305.poly1305AeadEncrypt(_bytes(aad), sub, n12, p, ct, tag)
        return bytes(ct) + bytes(tag)

    @staticmethod
    def open(key, nonce24, sealed, aad=b"") -> bytes:
        """the plaintext of ciphertext || tag; raises AEADBadTagException"""
        sub, n12 = XChaCha20Poly1305._sub(key, nonce24)
        c = _bytes(sealed)
        if len(c) < 16:
            raise AEADBadTagException("shorter than a tag")
        pt = bytearray(len(c) - 16)
        ChaCha20Poly1305.poly1305AeadDecrypt(_bytes(aad), sub, n12, c[:-16], pt, c[-16:])
        return bytes(pt)


def calculate_cookie(secret, addr, port: int) -> bytes:
    """cookie(src) = BLAKE2s-128 keyed with the responder's secret over addr || port: addr is the 4 or 16 address
    bytes, the port goes in network order."""
    a = _bytes(addr)
    if len(a) not in (4, 16):
        raise ValueError("an address is 4 or 16 bytes")
    return default_engine().blake2s_host([(a + struct.pack(">H", port), _bytes(secret), 16)])[0]


def calculate_mac2(message_without_mac2, cookie) -> bytes:
    """mac2 = BLAKE2s-128 keyed with the 16-byte cookie over the message up to its mac2 field."""
    return default_engine().blake2s_host([(_bytes(message_without_mac2), _bytes(cookie), 16)])[0]
