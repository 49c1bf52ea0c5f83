"""Mirror of ax.xz.wireguard.noise.crypto.internal.X25519 and ax.xz.wireguard.noise.keys.NoisePrivateKey /
NoisePublicKey: the same names, argument order and return values, with every scalar multiplication on the
device (wg_x25519_batch, one descriptor per call). A data path with many operands batches them itself
(Engine.x25519 / Engine.hs_dh)."""
from __future__ import annotations

import base64
import os

from .. import _lib as L
from ..engine import default_engine
from .crypto import _write


class X25519:
    """X25519.java:13-14, 24-28, 62-79, 96-155, 157-160."""
    POINT_SIZE = 32
    SCALAR_SIZE = 32

    @staticmethod
    def _mult(k, kOff: int, point):
        scalar = bytes(k[kOff:kOff + 32])
        if len(scalar) != 32 or (point is not None and len(point) != 32):
            raise IndexError("X25519 operands are 32 bytes")
        return default_engine().x25519_host([(scalar, point)])[0]

    @staticmethod
    def scalarMult(k, kOff: int, u, uOff: int, r, rOff: int) -> None:
        """r[rOff .. rOff + 32) = X25519(k[kOff ..), u[uOff ..)); the scalar is clamped as decodeScalar does."""
        out, _ = X25519._mult(k, kOff, bytes(u[uOff:uOff + 32]))
        _write(memoryview(r)[rOff:], out)

    @staticmethod
    def scalarMultBase(k, kOff: int, r, rOff: int) -> None:
        """The base point u = 9 (the reference goes through Ed25519 tables to the same value)."""
        out, _ = X25519._mult(k, kOff, None)
        _write(memoryview(r)[rOff:], out)

    @staticmethod
    def generatePublicKey(k, kOff: int, r, rOff: int) -> None:
        X25519.scalarMultBase(k, kOff, r, rOff)

    @staticmethod
    def calculateAgreement(k, kOff: int, u, uOff: int, r, rOff: int) -> bool:
        """scalarMult, then whether r is not all zero (X25519.java:24-28); r is written either way."""
        out, status = X25519._mult(k, kOff, bytes(u[uOff:uOff + 32]))
        _write(memoryview(r)[rOff:], out)
        return status != L.WG_X25519_ZERO

    @staticmethod
    def generatePrivateKey(random, k) -> None:
        """k = 32 random bytes, clamped (X25519.java:62-74). random: an object with nextBytes(buffer), or a
        callable n -> bytes such as os.urandom."""
        if len(k) != X25519.SCALAR_SIZE:
            raise ValueError("k")
        if hasattr(random, "nextBytes"):
            random.nextBytes(k)
        else:
            _write(k, bytes(random(X25519.SCALAR_SIZE)))
        k[0] &= 0xF8
        k[X25519.SCALAR_SIZE - 1] &= 0x7F
        k[X25519.SCALAR_SIZE - 1] |= 0x40


class NoisePublicKey:
    """NoisePublicKey.java: 32 bytes."""
    LENGTH = 32

    def __init__(self, data):
        data = bytes(data)
        if len(data) != self.LENGTH:
            raise ValueError("NoisePublicKey must be 32 bytes")
        self._data = data

    def data(self) -> bytes:
        return self._data

    def __eq__(self, other):
        return isinstance(other, NoisePublicKey) and self._data == other._data

    def __hash__(self):
        return hash(self._data)


class NoisePresharedKey:
    """NoisePresharedKey.java: 32 bytes."""
    LENGTH = 32

    def __init__(self, data):
        if data is None:
            raise TypeError("data")
        data = bytes(data)
        if len(data) != self.LENGTH:
            raise ValueError("NoisePublicKey must be 32 bytes")  # (the reference's message)
        self._data = data

    def data(self) -> bytes:
        return self._data

    @staticmethod
    def fromBase64(text: str) -> "NoisePresharedKey":
        return NoisePresharedKey(base64.b64decode(text))

    @staticmethod
    def zero() -> "NoisePresharedKey":
        return NoisePresharedKey(bytes(NoisePresharedKey.LENGTH))

    def __eq__(self, other):
        return isinstance(other, NoisePresharedKey) and self._data == other._data

    def __hash__(self):
        return hash(self._data)


class NoisePrivateKey:
    """NoisePrivateKey.java:12-56: the public key is derived when the key is made; sharedSecret ignores
    calculateAgreement's result, so a low-order public key yields 32 zero bytes."""
    LENGTH = 32

    def __init__(self, data, publicKey: NoisePublicKey | None = None):
        if data is None:
            raise TypeError("data")
        self._data = bytearray(data)
        if len(self._data) != self.LENGTH:
            raise ValueError("NoisePrivateKey must be 32 bytes")
        if publicKey is None:
            pub = bytearray(NoisePublicKey.LENGTH)
            X25519.generatePublicKey(self._data, 0, pub, 0)
            publicKey = NoisePublicKey(pub)
        self._public = publicKey

    def data(self) -> bytearray:
        return self._data

    def publicKey(self) -> NoisePublicKey:
        return self._public

    @staticmethod
    def newPrivateKey() -> "NoisePrivateKey":
        pk = bytearray(NoisePrivateKey.LENGTH)
        X25519.generatePrivateKey(os.urandom, pk)
        return NoisePrivateKey(pk)

    def sharedSecret(self, publicKey: NoisePublicKey) -> NoisePublicKey:
        shared = bytearray(NoisePublicKey.LENGTH)
        X25519.calculateAgreement(self._data, 0, publicKey.data(), 0, shared, 0)
        return NoisePublicKey(shared)

    @staticmethod
    def fromBase64(text: str) -> "NoisePrivateKey":
        return NoisePrivateKey(base64.b64decode(text))
