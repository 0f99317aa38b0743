"""KeccakHash<N> -- mirror of plonky2/src/hash/keccak.rs:104-127 (and hash_or_noop, plonk/config.rs:63-74), batched on the
device through p2hot_keccak256_dev.

A digest is N bytes (1..32).  On the device, and in every array this package returns for a tree, it occupies the 32-byte slot of a
Poseidon digest ([4] words, bytes N..32 zero); `to_bytes` / `from_bytes` convert between the slot words and BytesHash<N>.
Pass a KeccakHash as `hasher=` to MerkleTree.new and PolynomialBatch.from_values / from_coeffs.
"""
import numpy as np

from ..engine import default_engine

P = 0xFFFFFFFF00000001
KECCAK_DOMAIN = 0x01  # keccak_hash::keccak (the original Keccak padding)
SHA3_DOMAIN = 0x06    # FIPS 202 SHA3-256


def keccak256(msgs, domain=KECCAK_DOMAIN, engine=None):
    """Keccak-256 (domain 0x01) or SHA3-256 (0x06) of one bytes object -> 32 bytes, or of equal-length messages uint8
    [count][L] -> uint8 [count][32]"""
    eng = engine or default_engine()
    if isinstance(msgs, (bytes, bytearray)):
        return bytes(eng.keccak256(np.frombuffer(bytes(msgs), dtype=np.uint8)[None, :], domain)[0])
    return eng.keccak256(msgs, domain)


def to_bytes(slots, n):
    """slot words [..][4] -> digests uint8 [..][n]"""
    w = np.ascontiguousarray(np.asarray(slots, dtype=np.uint64).reshape(-1, 4).astype("<u8"))
    return w.view(np.uint8).reshape(-1, 32)[:, :n]


def from_bytes(digests):
    """digests uint8 [..][n] -> slot words [..][4] (bytes n..32 zero)"""
    d = np.asarray(digests, dtype=np.uint8)
    d = d.reshape(-1, d.shape[-1])
    out = np.zeros((d.shape[0], 32), dtype=np.uint8)
    out[:, :d.shape[1]] = d
    return out.view("<u8").astype(np.uint64).reshape(-1, 4)


def _field_bytes(elems):
    e = np.asarray(elems, dtype=np.uint64)
    e = np.where(e >= np.uint64(P), e - np.uint64(P), e)  # to_canonical_u64
    return np.ascontiguousarray(e.astype("<u8")).view(np.uint8).reshape(e.shape[0], -1)


class KeccakHash:
    """KeccakHash<n>.  Every method is batched: elements [count][W] (uint64), digests uint8 [count][n]."""

    def __init__(self, n, engine=None):
        if not 1 <= n <= 32:
            raise ValueError("KeccakHash<N>: N is 1..32 bytes (the reference slices hash_bytes[..N] of 32)")
        self.n = n
        self._engine = engine

    def __repr__(self):
        return "KeccakHash(%d)" % self.n

    @property
    def engine(self):
        return self._engine or default_engine()

    def hash_no_pad(self, elems):  # keccak.rs:110-116
        return self.engine.keccak256(_field_bytes(elems), KECCAK_DOMAIN)[:, :self.n]

    def two_to_one(self, left, right):  # keccak.rs:118-125
        msgs = np.concatenate([np.asarray(left, dtype=np.uint8), np.asarray(right, dtype=np.uint8)], axis=1)
        return self.engine.keccak256(msgs, KECCAK_DOMAIN)[:, :self.n]

    def hash_or_noop(self, elems):  # plonk/config.rs:63-74
        e = np.asarray(elems, dtype=np.uint64)
        if 8 * e.shape[1] <= self.n:
            out = np.zeros((e.shape[0], self.n), dtype=np.uint8)
            out[:, :8 * e.shape[1]] = _field_bytes(e)
            return out
        return self.hash_no_pad(e)


def hash_size(hasher):
    """the library's hasher code: 0 for Poseidon (None), N for KeccakHash<N>"""
    if hasher is None:
        return 0
    if isinstance(hasher, KeccakHash):
        return hasher.n
    raise TypeError("unsupported hasher %r (PoseidonHash = None, or KeccakHash(N))" % (hasher,))
