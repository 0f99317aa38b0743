"""Keccak-f[1600] restated from FIPS 202 (sections 3.2, 5.1, B.2), vectorised over messages with numpy, and on top of it
KeccakHash<N> (plonky2/src/hash/keccak.rs:104-127), hash_or_noop (plonk/config.rs:63-74) and the reference-layout Merkle tree
(hash/merkle_tree.rs:86-149).  Independent of the library: the test-suite pins it to hashlib.sha3_256 and to the public
Keccak-256 vectors, then pins the library to it."""
import numpy as np

P = 0xFFFFFFFF00000001
RATE = 136  # bytes, Keccak-256 / SHA3-256

# rho offsets r[x][y] (FIPS 202 Table 2)
_R = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]


def _rc():
    """iota constants from the LFSR rc(t) (FIPS 202 Algorithm 5), not from a table"""
    out = []
    r = 1
    bits = []
    for _ in range(255):
        bits.append(r & 1)
        r <<= 1
        if r & 0x100:
            r ^= 0x171
    for ir in range(24):
        v = 0
        for j in range(7):
            if bits[(j + 7 * ir) % 255]:
                v |= 1 << ((1 << j) - 1)
        out.append(v)
    return out


_RC = [np.uint64(v) for v in _rc()]


def _rotl(a, n):
    n %= 64
    if n == 0:
        return a
    return (a << np.uint64(n)) | (a >> np.uint64(64 - n))


def keccak_f(A):
    """A: uint64 [count][5][5] indexed [.., x, y]; returns the permuted state"""
    A = A.copy()
    for ir in range(24):
        C = A[:, :, 0] ^ A[:, :, 1] ^ A[:, :, 2] ^ A[:, :, 3] ^ A[:, :, 4]
        D = np.stack([C[:, (x - 1) % 5] ^ _rotl(C[:, (x + 1) % 5], 1) for x in range(5)], axis=1)
        A ^= D[:, :, None]
        B = np.empty_like(A)
        for x in range(5):
            for y in range(5):
                B[:, y, (2 * x + 3 * y) % 5] = _rotl(A[:, x, y], _R[x][y])
        for x in range(5):
            for y in range(5):
                A[:, x, y] = B[:, x, y] ^ (~B[:, (x + 1) % 5, y] & B[:, (x + 2) % 5, y])
        A[:, 0, 0] ^= _RC[ir]
    return A


def sponge(msgs, domain=0x01):
    """msgs: uint8 [count][L] (equal lengths) -> uint8 [count][32]: rate 136, pad10*1 with the given domain byte
    (0x01 Keccak-256, 0x06 SHA3-256)"""
    msgs = np.asarray(msgs, dtype=np.uint8)
    count, L = msgs.shape
    padded_len = (L // RATE + 1) * RATE
    buf = np.zeros((count, padded_len), dtype=np.uint8)
    buf[:, :L] = msgs
    buf[:, L] ^= domain
    buf[:, -1] ^= 0x80
    lanes = buf.view("<u8").astype(np.uint64)  # [count][padded_len / 8]
    A = np.zeros((count, 5, 5), dtype=np.uint64)
    for b in range(padded_len // RATE):
        blk = lanes[:, b * 17:(b + 1) * 17]
        for i in range(17):
            A[:, i % 5, i // 5] ^= blk[:, i]
        A = keccak_f(A)
    out = np.stack([A[:, i % 5, i // 5] for i in range(4)], axis=1).astype("<u8")
    return out.view(np.uint8).reshape(count, 32)


def keccak256(msgs):
    return sponge(msgs, 0x01)


def field_bytes(elems):
    """write_field_vec (util/serialization/mod.rs:1254-1260): canonical u64s, little-endian; [count][W] -> uint8 [count][8W]"""
    e = np.asarray(elems, dtype=np.uint64)
    e = np.where(e >= np.uint64(P), e - np.uint64(P), e)
    return np.ascontiguousarray(e.astype("<u8")).view(np.uint8).reshape(e.shape[0], -1)


class KeccakHash:
    """KeccakHash<N>; digests are uint8 [count][N]"""

    def __init__(self, n):
        self.n = n

    def hash_no_pad(self, elems):
        return keccak256(field_bytes(elems))[:, :self.n]

    def hash_or_noop(self, elems):
        e = np.asarray(elems, dtype=np.uint64)
        if 8 * e.shape[1] <= self.n:
            out = np.zeros((e.shape[0], self.n), dtype=np.uint8)
            out[:, :8 * e.shape[1]] = field_bytes(e)
            return out
        return self.hash_no_pad(e)

    def two_to_one(self, left, right):
        return keccak256(np.concatenate([np.asarray(left, np.uint8), np.asarray(right, np.uint8)], axis=1))[:, :self.n]


def to_slots(d):
    """N-byte digests [count][N] -> the 32-byte slots the library stores ([count][4] words, bytes N..32 zero)"""
    d = np.asarray(d, dtype=np.uint8)
    out = np.zeros((d.shape[0], 32), dtype=np.uint8)
    out[:, :d.shape[1]] = d
    return out.view("<u8").astype(np.uint64).reshape(-1, 4)


def from_slots(words, n):
    return np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1, 4).astype("<u8")).view(np.uint8).reshape(-1, 32)[:, :n]


def merkle_tree(leaves, cap_height, hasher):
    """MerkleTree::new (merkle_tree.rs:193-224, fill_digests_buf :115-149, fill_subtree :86-113): (digests, cap) as uint8
    [2 (n - 2^cap_height)][N] and [2^cap_height][N], level by level over all subtrees at once"""
    leaves = np.asarray(leaves, dtype=np.uint64)
    n = leaves.shape[0]
    log_n = n.bit_length() - 1
    h = log_n - cap_height
    N = hasher.n
    level = hasher.hash_or_noop(leaves)  # [n][N], leaf order
    sub = 1 << h
    sub_digests = 2 * (sub - 1)
    digests = np.zeros((max(sub_digests << cap_height, 0), N), dtype=np.uint8)
    for lv in range(h + 1):
        if lv > 0:
            level = hasher.two_to_one(level[0::2], level[1::2])
        if lv == h:
            break
        for j in range(level.shape[0]):  # node j of level lv: merkle.hpp node_slot (the closed form of fill_subtree's layout)
            s, jl = j >> (h - lv), j & ((1 << (h - lv)) - 1)
            idx = 2 * (((jl >> 1) << (lv + 1)) + (1 << lv) - 1) + (jl & 1)
            digests[s * sub_digests + idx] = level[j]
    return digests, level


def prove(digests, leaf_index, n_leaves, cap_height):
    """merkle_tree_prove (merkle_tree.rs:151-190) over uint8 [..][N] digests"""
    num_layers = n_leaves.bit_length() - 1 - cap_height
    tree_len = digests.shape[0] >> cap_height
    tree = digests[tree_len * (leaf_index >> num_layers):]
    pair = leaf_index & ((1 << num_layers) - 1)
    out = []
    for i in range(num_layers):
        parity = pair & 1
        pair >>= 1
        sib = (pair << (i + 1)) + (1 << i) - 1
        out.append(tree[2 * sib + (1 - parity)])
    return out


def verify(leaf_digest, leaf_index, path, cap, cap_height, hasher):
    """verify_merkle_proof_to_cap (merkle_proofs.rs): fold the path with two_to_one, compare with the cap entry"""
    cur = np.asarray(leaf_digest, dtype=np.uint8)[None]
    idx = leaf_index
    for sib in path:
        s = np.asarray(sib, dtype=np.uint8)[None]
        cur = hasher.two_to_one(s, cur) if idx & 1 else hasher.two_to_one(cur, s)
        idx >>= 1
    return bool((cur[0] == np.asarray(cap)[idx]).all())
