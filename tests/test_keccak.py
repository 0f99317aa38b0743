"""KeccakHash<N> Merkle commitments (KeccakGoldilocksConfig, plonk/config.rs:118-126): the numpy restatement of Keccak
(tests/keccak_ref.py) pinned to hashlib and the public Keccak-256 vectors, then the library pinned to it -- the primitive, the
trees, the commitments and the ABI boundaries -- on the emulator (CPU tier) and on the MI355X (-m gpu)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from plonky2_amd import _lib
from tests import keccak_ref as kr
from tests.conftest import P, rand_field


def _khash(eng, n):
    from plonky2_amd.hash.keccak import KeccakHash
    return KeccakHash(n, engine=eng)


# ---------------------------------------------------------------- the reference itself
def test_reference_equals_hashlib_sha3_at_every_length():
    rng = np.random.default_rng(1)
    for L in list(range(0, 301)) + [1080]:
        m = rng.integers(0, 256, size=(2, L), dtype=np.uint8)
        got = kr.sponge(m, 0x06)
        for i in range(2):
            assert bytes(got[i]) == hashlib.sha3_256(bytes(m[i])).digest(), L


def test_reference_gives_the_public_keccak256_vectors():
    empty = kr.keccak256(np.zeros((1, 0), dtype=np.uint8))[0]
    abc = kr.keccak256(np.frombuffer(b"abc", dtype=np.uint8)[None, :])[0]
    assert bytes(empty).hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert bytes(abc).hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_reference_hash_or_noop_and_tree_layout():
    h = kr.KeccakHash(25)
    e = np.array([[1, 2, 3]], dtype=np.uint64)
    assert bytes(h.hash_or_noop(e)[0]) == b"".join(int(x).to_bytes(8, "little") for x in (1, 2, 3)) + b"\0"
    e4 = np.array([[1, 2, 3, P + 4]], dtype=np.uint64)  # 32 bytes > 25: hashed, canonical bytes
    assert bytes(h.hash_or_noop(e4)[0]) == bytes(kr.keccak256(kr.field_bytes(np.array([[1, 2, 3, 4]], np.uint64)))[0][:25])
    # fill_subtree on 4 leaves, cap height 0: [d(l0), d(l1), d(l2), d(l3)... ] in the reference order
    leaves = np.arange(4 * 5, dtype=np.uint64).reshape(4, 5)
    d, cap = kr.merkle_tree(leaves, 0, h)
    l = h.hash_or_noop(leaves)
    n01, n23 = h.two_to_one(l[0:1], l[1:2]), h.two_to_one(l[2:3], l[3:4])
    # layout: left recursive (l0, l1) || left child || right child || right recursive (l2, l3)
    assert (d[0] == l[0]).all() and (d[1] == l[1]).all() and (d[2] == n01[0]).all() and (d[3] == n23[0]).all()
    assert (d[4] == l[2]).all() and (d[5] == l[3]).all() and (cap[0] == h.two_to_one(n01, n23)[0]).all()


# ---------------------------------------------------------------- the primitive
@pytest.mark.parametrize("L", [0, 1, 8, 50, 135, 136, 137, 1080, 1112])
def test_keccak256_primitive(eng, L):
    from plonky2_amd.hash.keccak import SHA3_DOMAIN, keccak256
    rng = np.random.default_rng(L)
    count = 67  # not a multiple of 64
    m = rng.integers(0, 256, size=(count, L), dtype=np.uint8)
    sha3 = keccak256(m, SHA3_DOMAIN, engine=eng)
    kec = keccak256(m, engine=eng)
    assert sha3.shape == (count, 32)
    for i in range(count):
        assert bytes(sha3[i]) == hashlib.sha3_256(bytes(m[i])).digest(), (L, i)
    assert (kec == kr.keccak256(m)).all()
    if L == 0:
        assert keccak256(b"", engine=eng).hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    if L == 1:
        assert keccak256(b"abc", engine=eng).hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_keccak_hash_mirror(eng):
    rng = np.random.default_rng(3)
    for n in (25, 32, 20, 1):
        h, ref = _khash(eng, n), kr.KeccakHash(n)
        for W in (1, 2, 3, 4, 5, 17, 18):
            e = rand_field(rng, 9, W, noncanonical=True)
            assert (h.hash_or_noop(e) == ref.hash_or_noop(e)).all(), (n, W)
            assert (h.hash_no_pad(e) == ref.hash_no_pad(e)).all(), (n, W)
        a = rng.integers(0, 256, size=(5, n), dtype=np.uint8)
        b = rng.integers(0, 256, size=(5, n), dtype=np.uint8)
        assert (h.two_to_one(a, b) == ref.two_to_one(a, b)).all()


# ---------------------------------------------------------------- trees
def _check_tree(digests, cap, slots_d, slots_c, n_leaves, cap_height, n, paths=None):
    """library slots (words) vs the reference's N-byte digests (to_slots: bytes N..32 of every slot zero); paths: {leaf: path}"""
    sd = np.asarray(slots_d, dtype=np.uint64).reshape(-1, 4)
    assert sd.shape[0] == len(digests) and (sd == kr.to_slots(digests)).all()
    assert (np.asarray(slots_c, dtype=np.uint64).reshape(-1, 4) == kr.to_slots(cap)).all()
    for i, p in (paths or {}).items():
        want = np.array(kr.prove(digests, i, n_leaves, cap_height), dtype=np.uint8).reshape(-1, n)
        assert (np.asarray(p, dtype=np.uint64).reshape(-1, 4) == kr.to_slots(want)).all(), i


@pytest.mark.parametrize("n", [25, 32, 20])
def test_keccak_merkle_trees_equal_the_reference(eng, n):
    from plonky2_amd.hash.merkle_tree import MerkleTree
    rng = np.random.default_rng(n)
    ref = kr.KeccakHash(n)
    log_leaves = 6
    L = 1 << log_leaves
    for k, W in enumerate((1, 2, 3, 4, 5, 16, 17, 18, 34, 135)):
        cap_height = (0, 3, log_leaves)[k % 3]
        leaves = rand_field(rng, L, W, noncanonical=True)
        d_ref, c_ref = kr.merkle_tree(leaves, cap_height, ref)
        # row-major leaves through the mirror
        t = MerkleTree.new(leaves, cap_height, engine=eng, hasher=_khash(eng, n))
        idx = [0, 5, L - 1]
        paths = {i: p for i, p in zip(idx, t.prove_many(idx))}  # gathered on the device (p2hot_merkle_paths_dev)
        _check_tree(d_ref, c_ref, t.digests, t.cap.entries, L, cap_height, n, paths)
        assert t.cap.to_bytes(n) == [bytes(c) for c in c_ref]
        raw = np.ascontiguousarray(np.asarray(t.digests, dtype=np.uint64).reshape(-1, 4)).view(np.uint8).reshape(-1, 32)
        assert not raw[:, n:].any() and not t.cap.entries.view(np.uint8).reshape(-1, 32)[:, n:].any()
        # column-major leaves through the device entry point
        dig, cap = eng.merkle(eng.dev(np.ascontiguousarray(leaves.T)), 0, W, log_leaves, cap_height, hash_size=n)
        _check_tree(d_ref, c_ref, eng.host(dig), eng.host(cap), L, cap_height, n)


def test_keccak_merkle_leaf_ranges(eng):
    """a range of whole cap subtrees writes only its own slots (p2hot_keccak_merkle_dev leaf_begin / leaf_count)"""
    rng = np.random.default_rng(5)
    n, W, log_leaves, cap_height = 25, 19, 5, 2
    leaves = rand_field(rng, 1 << log_leaves, W)
    d_ref, c_ref = kr.merkle_tree(leaves, cap_height, kr.KeccakHash(n))
    nd = eng.num_digests(log_leaves, cap_height)
    dig, cap = eng.mem.zeros(nd, 4), eng.mem.zeros(1 << cap_height, 4)
    sub = 1 << (log_leaves - cap_height)
    for s in (2, 0, 3, 1):
        part = eng.dev(np.ascontiguousarray(leaves[s * sub:(s + 1) * sub]))
        eng.merkle(part, 1, W, log_leaves, cap_height, leaf_begin=s * sub, leaf_count=sub, digests=dig, cap=cap, hash_size=n)
    _check_tree(d_ref, c_ref, eng.host(dig), eng.host(cap), 1 << log_leaves, cap_height, n)


# ---------------------------------------------------------------- commitments
def _commit_host(eng, cols, rb, cap, is_values, flags, salts=None, leaves=False, handle=False):
    W, n = cols.shape
    log_n = n.bit_length() - 1
    N = n << rb
    S = 0 if salts is None else salts.shape[0]
    ptrs = (C.c_void_p * W)(*[cols[c].ctypes.data for c in range(W)])
    nd = eng.num_digests(log_n + rb, cap)
    out = {"coeffs": np.zeros((W, n), dtype=np.uint64), "digests": np.zeros((max(nd, 1), 4), dtype=np.uint64),
           "cap": np.zeros((1 << cap, 4), dtype=np.uint64)}
    if leaves:
        out["leaves"] = np.zeros((N, W + S), dtype=np.uint64)
    h = C.c_void_p()
    common = (out["coeffs"].ctypes.data, out["leaves"].ctypes.data if leaves else None, out["digests"].ctypes.data,
              out["cap"].ctypes.data, C.byref(h) if handle else None)
    if S:
        sptrs = (C.c_void_p * S)(*[salts[j].ctypes.data for j in range(S)])
        rc = eng.lib.p2hot_commit_salted(eng.ctx, ptrs, W, log_n, rb, cap, 1 if is_values else 0, flags, sptrs, S, *common)
    else:
        rc = eng.lib.p2hot_commit(eng.ctx, ptrs, W, log_n, rb, cap, 1 if is_values else 0, flags, *common)
    eng.check(rc)
    out["digests"] = out["digests"][:nd]
    out["handle"] = h
    return out


@pytest.mark.parametrize("W,n_hash,blinded", [(3, 25, False), (13, 25, False), (17, 32, True), (40, 25, False), (21, 20, True)])
def test_keccak_commitments_equal_the_reference(eng, ora, W, n_hash, blinded):
    from plonky2_amd.fri.oracle import PolynomialBatch
    rng = np.random.default_rng(W)
    log_n, rb, cap = 6, 2, 2
    N = 1 << (log_n + rb)
    hasher, ref = _khash(eng, n_hash), kr.KeccakHash(n_hash)
    vals = rand_field(rng, W, 1 << log_n, noncanonical=True)
    salts = rand_field(rng, 4, N) if blinded else None
    for is_values in (True, False):
        o = (ora.commit_salted(vals, salts, rb, cap, is_values) if blinded else ora.commit(vals, rb, cap, is_values))
        build = PolynomialBatch.from_values if is_values else PolynomialBatch.from_coeffs
        b = build(vals, rb, blinded, cap, engine=eng, salts=salts, hasher=hasher)
        assert b.hasher is hasher
        # the LDE does not depend on the hasher
        coeffs = o["coeffs"] % np.uint64(P)  # (from_coeffs: the oracle hands the input back as it came)
        assert (b.polynomials == coeffs).all()
        leaves = b.merkle_tree.leaves
        assert (leaves == o["leaves"]).all()
        d_ref, c_ref = kr.merkle_tree(leaves, cap, ref)
        _check_tree(d_ref, c_ref, b.merkle_tree.digests, b.merkle_tree.cap.entries, N, cap, n_hash)
        # batch paths verify to the cap
        for i in (0, 77, N - 1):
            path = kr.from_slots(b.merkle_tree.prove(i), n_hash)
            assert kr.verify(ref.hash_or_noop(leaves[i:i + 1])[0], i, path, c_ref, cap, ref)
        # the host flag variants give the same bytes
        flags = _lib.HASH_KECCAK(n_hash)
        base = _commit_host(eng, vals, rb, cap, is_values, flags, salts, leaves=True)
        asy = _commit_host(eng, vals, rb, cap, is_values, flags | _lib.LEAVES_ASYNC | _lib.LEAVES_NATURAL, salts, leaves=True,
                           handle=True)
        eng.check(eng.lib.p2hot_batch_leaves_wait(asy["handle"], 0, N))
        kv = _commit_host(eng, vals, rb, cap, is_values, flags | _lib.KEEP_VALUES, salts, handle=True)
        for r in (base, asy, kv):
            assert (r["cap"] == kr.to_slots(c_ref)).all() and (r["digests"] == kr.to_slots(d_ref)).all()
            assert (r["coeffs"] == coeffs).all()
        assert (base["leaves"] == o["leaves"]).all()
        rev = [int(format(i, "0%db" % (log_n + rb))[::-1], 2) for i in range(N)]
        assert (asy["leaves"] == o["leaves"][rev]).all()
        eng.lib.p2hot_batch_free(asy["handle"])
        eng.lib.p2hot_batch_free(kv["handle"])
    # a Poseidon commitment on the same context afterwards is still oracle-exact
    p = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng)
    assert (p.merkle_tree.cap.entries == ora.commit(vals, rb, cap, True)["cap"]).all()


def test_keccak_commit_from_device_columns_and_buffers(eng, ora):
    """p2hot_commit_cols with the hasher flag, and p2hot_commit_keccak_dev on device buffers"""
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    rng = np.random.default_rng(11)
    W, log_n, rb, cap, n = 9, 5, 3, 1, 25
    vals = rand_field(rng, W, 1 << log_n)
    o = ora.commit(vals, rb, cap, True)
    d_ref, c_ref = kr.merkle_tree(o["leaves"], cap, kr.KeccakHash(n))
    dc = DeviceColumns.upload(vals, eng)
    b = PolynomialBatch.from_values(dc, rb, False, cap, engine=eng, hasher=_khash(eng, n))
    assert dc._h is None
    _check_tree(d_ref, c_ref, b.merkle_tree.digests, b.merkle_tree.cap.entries, 1 << (log_n + rb), cap, n)
    r = eng.commit(eng.dev(vals), log_n, rb, cap, True, want_leaves=True, hash_size=n)
    assert (eng.host(r["coeffs"]) == o["coeffs"]).all() and (eng.host(r["leaves"]) == o["leaves"]).all()
    _check_tree(d_ref, c_ref, eng.host(r["digests"]), eng.host(r["cap"]), 1 << (log_n + rb), cap, n)
    with pytest.raises(ValueError):
        PolynomialBatch.from_values(eng.dev(vals), rb, False, cap, engine=eng, hasher=_khash(eng, n))


# ---------------------------------------------------------------- boundaries
def test_keccak_boundaries(eng):
    from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, eval_openings, prove_openings
    from plonky2_amd.iop.challenger import Challenger
    rng = np.random.default_rng(2)
    W, log_n, rb, cap = 6, 5, 2, 1
    vals = rand_field(rng, W, 1 << log_n)
    leaves = eng.dev(rand_field(rng, 16, 5))
    dig, capb = eng.mem.zeros(eng.num_digests(4, 0), 4), eng.mem.zeros(1, 4)
    msgs = eng.dev(np.zeros(4, dtype=np.uint64))
    out = eng.mem.zeros(1, 4)
    for bad in [0] + list(range(33, 64)):
        assert eng.lib.p2hot_keccak_merkle_dev(eng.ctx, eng.ptr(leaves), 1, 0, 5, 4, 0, 0, 16, eng.ptr(dig), eng.ptr(capb),
                                               bad) == _lib.EINVAL
        d = eng.mem.empty(W, 1 << log_n)
        lde = eng.mem.empty(W, 1 << (log_n + rb))
        cols = eng.dev(vals)
        assert eng.lib.p2hot_commit_keccak_dev(eng.ctx, eng.ptr(cols), 1 << log_n, W, log_n, rb, cap, 1, 0, 1 << (log_n + rb),
                                               eng.ptr(d), 1 << log_n, eng.ptr(lde), 1 << (log_n + rb), None, eng.ptr(dig),
                                               eng.ptr(capb), bad) == _lib.EINVAL
        if bad:
            with pytest.raises(_lib.P2HotError) as e:
                _commit_host(eng, vals, rb, cap, True, _lib.HASH_KECCAK(bad))
            assert e.value.code == _lib.EINVAL
    assert eng.lib.p2hot_keccak256_dev(eng.ctx, eng.ptr(msgs), 8, 1, 0x100, eng.ptr(out)) == _lib.EINVAL
    # the existing unknown flag bits stay EINVAL, with or without the hasher field
    for flags in (0xF0, 0xF0 | _lib.HASH_KECCAK(25), 0x10000 | _lib.HASH_KECCAK(25)):
        with pytest.raises(_lib.P2HotError) as e:
            _commit_host(eng, vals, rb, cap, True, flags)
        assert e.value.code == _lib.EINVAL
    # a Keccak batch: prove_openings is refused, eval_openings equals the Poseidon batch's
    kb = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng, hasher=_khash(eng, 25))
    pb = PolynomialBatch.from_values(vals, rb, False, cap, engine=eng)
    with pytest.raises(_lib.P2HotError) as e:
        prove_openings([FriBatchInfo([1, 2], [(0, 0)])], [kb], Challenger(eng), rb, cap, [1], 0, 2, engine=eng)
    assert e.value.code == _lib.EUNSUPPORTED and "Keccak" in str(e.value)
    pts = rand_field(rng, 3, 2)
    assert all((a == b).all() for a, b in zip(eval_openings([kb], pts, engine=eng), eval_openings([pb], pts, engine=eng)))
    assert (kb.merkle_tree.leaves == pb.merkle_tree.leaves).all() and (kb.polynomials == pb.polynomials).all()


# ---------------------------------------------------------------- full size
@pytest.mark.gpu
def test_c3_wires_keccak_commit_full_size(gpu):
    """the C3 wires shape (2^23 leaves of 135 words) with KeccakHash<25>: rows equal the Poseidon batch's (whose cap is the
    golden one), level-0 digests equal the reference, and the paths verify to the Keccak cap"""
    import json
    import os
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.util.synthetic import splitmix_columns_numpy
    from tests.conftest import ROOT
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "commit_caps.json")))["c3_wires"]
    W, log_n, rb, cap = g["W"], g["log_n"], g["rate_bits"], g["cap_height"]
    N = 1 << (log_n + rb)
    cols = splitmix_columns_numpy(0, W, 1 << log_n)
    ref = kr.KeccakHash(25)
    pb = PolynomialBatch.from_values(cols, rb, False, cap, engine=gpu)
    assert pb.merkle_tree.cap.entries.tolist() == g["cap"]
    rng = np.random.default_rng(23)
    idx = np.unique(rng.integers(0, N, size=4096)).astype(np.uint64)
    prow = pb.merkle_tree._getter(idx)
    del pb
    kb = PolynomialBatch.from_values(cols, rb, False, cap, engine=gpu, hasher=_khash(gpu, 25))
    krow = kb.merkle_tree._getter(idx)
    assert (krow == prow).all()
    lvl0 = ref.hash_or_noop(krow)
    # the level-0 digest of leaf i is the first sibling on the path of leaf i ^ 1
    sib = kb._owner.paths(idx ^ np.uint64(1))[:, 0]
    assert (kr.from_slots(sib, 25) == lvl0).all() and (sib == kr.to_slots(lvl0)).all()
    paths = kb._owner.paths(idx)
    capb = kr.from_slots(kb.merkle_tree.cap.entries, 25)
    for q, i in enumerate(int(x) for x in idx):
        assert kr.verify(lvl0[q], i, kr.from_slots(paths[q], 25), capb, cap, ref), i
    gpu.check(gpu.lib.p2hot_ctx_trim(gpu.ctx))
