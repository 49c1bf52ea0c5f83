"""Mirror of the reference module ax.xz.wireguard.noise (crypto + handshake
packages) whose ChaCha20-Poly1305 arithmetic runs on the MI355X through
libwgaead. Same class and method names, argument meaning and exceptions as the
Java sources, so the reference's own tests read the same against it."""
from .crypto import (AEADBadTagException, BadPaddingException, Blake2s, BLAKE2s256, ChaCha20,  # noqa: F401
                     ChaCha20Poly1305, Crypto, HChaCha20, IllegalStateException, Poly1305, XChaCha20Poly1305,
                     calculate_cookie, calculate_mac1, calculate_mac2)
from .handshake import Handshakes, InitiatorStageOne, ResponderHandshake, SymmetricKeypair  # noqa: F401
from .ratelimit import RateLimiter, ratelimit_key  # noqa: F401
from .keys import NoisePresharedKey, NoisePrivateKey, NoisePublicKey, X25519  # noqa: F401
