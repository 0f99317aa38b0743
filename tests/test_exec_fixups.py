"""The S-box multiply streams whose carry is added under a lane mask and whose borrow sits behind a scalar branch
(gl_mul3.hpp mul3cx / mul1cx; flag 2048 of the field self-test), and the kernels that run them.

The reduction's tail is u + (c - b)(2^32 - 1) with two per-lane flags: c, the carry of u = t + T.lo (2^32 - 1), set in about half
the lanes, and b, the borrow of t = lo - T.hi - cm, set with probability 2^-32 on random operands.  The streams treat the two
differently, so the inputs here are built to reach every combination, in every one of the three stream positions, next to lanes
that take another path, and in waves that are not full (the masks are cut to the lanes still running).  The flags are restated
below with Python integers and the test asserts that its own operands reach what it claims.

The emulator runs the C forms of these functions (its instruction interpreter knows neither scalar instructions nor EXEC); the
CPU tier therefore checks the self-test's new entry and the operands, the GPU tier (-m gpu) the streams themselves.
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import P, ROOT

M32 = 2**32 - 1
M64 = 2**64 - 1
E32 = 2**32
Z = 0x9E3779B97F4A7C15


def stream_flags(a, b):
    """(borrow b, carry c, result) of one product as the streams compute it (gl_mul3.hpp, mul3cg's chained partial products)"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p = a0 * b0
    m = a1 * b0 + (p >> 32)
    n = a0 * b1 + m
    cm, n = n >> 64, n & M64
    t_hi = a1 * b1 + (n >> 32)  # the high 64 bits without cm
    lo = (p & M32) | ((n & M32) << 32)
    t = lo - (t_hi >> 32) - cm
    bor, t = int(t < 0), t & M64
    u = t + (t_hi & M32) * M32
    car, u = u >> 64, u & M64
    r = u + (car - bor) * M32
    assert 0 <= r < 2**64 and r % P == a * b % P
    return bor, car, r


# (x, y) pairs by the flags of x * y: e = +1, e = -1, e = 0 with both flags, e = 0 with neither
CASES = {
    (0, 1): (0xFFFFFFFF, 2**64 - 1),
    (1, 0): (2**48, 0xFFFF * 2**48),  # low 64 bits 0, T.lo = 0, T.hi = 0xFFFF
    (1, 1): (P - 1, P - 1),
    (0, 0): (1, 1),
}
# one more borrow case whose neighbours in the same call carry no borrow: the three streams' borrow pairs are ORed for one branch
LONE_BORROW = (2**40, 2**57 + 2**24)  # x * y = 2^97 + 2^64: low 64 bits 0, T.hi = 2


def constructed():
    """192 pairs = three waves in which consecutive lanes take different paths"""
    order = [CASES[(0, 1)], CASES[(1, 0)], CASES[(1, 1)], CASES[(0, 0)], LONE_BORROW, CASES[(0, 1)]]
    return [order[i % 6] for i in range(192)]


def test_constructed_operands_reach_every_flag_combination():
    for want, (x, y) in CASES.items():
        assert stream_flags(x, y)[:2] == want, (want, hex(x), hex(y))
    # the self-test kernel runs x * y in stream position 0, 2 and 1 of its three calls (operand rows {x, y, z}, {y, z, x}, {z, x, y}
    # against {y, y, x}, {y, x, y}, {x, y, y}; z = x ^ Z), with y * y and z * x in the other two positions
    x, y = LONE_BORROW
    z = x ^ Z
    assert stream_flags(x, y)[0] == 1 and stream_flags(y, y)[0] == 0 and stream_flags(z, x)[0] == 0
    # and the other products of the constructed lanes show both values of c, so a wave mixes masked and unmasked lanes in every position
    cs = {stream_flags(y, y)[1] for x, y in CASES.values()} | {stream_flags(x ^ Z, x)[1] for x, y in CASES.values()}
    assert cs == {0, 1}
    pairs = constructed()
    assert len(pairs) % 64 == 0 and len(set(pairs[:6])) == 5


def operands():
    rng = np.random.default_rng(2048)
    edge = [0, 1, 2, 3, E32 - 2, E32 - 1, E32, E32 + 1, 2**63 - 1, 2**63, 2**63 + 1, P - E32, P - 2, P - 1, P, P + 1,
            P + E32 - 2, 2**64 - E32, 2**64 - 2, 2**64 - 1, 0xFFFFFFFF_00000000, 0x00000000_FFFFFFFF,
            0xFFFFFFFE_FFFFFFFF, 0x80000000_80000000]  # the reference's grid (field/src/prime_field_testing.rs:8-17)
    a = [x for x, _ in constructed()] + [x for x in edge for _ in edge] + [int(v) for v in rng.integers(0, 2**64, 4096, dtype=np.uint64)]
    b = [y for _, y in constructed()] + [y for _ in edge for y in edge] + [int(v) for v in rng.integers(0, 2**64, 4096, dtype=np.uint64)]
    assert len(a) % 256 == 0
    return a, b


def run_selftest(eng, a, b):
    n = len(a)
    da, db = eng.dev(np.array(a, dtype=np.uint64)), eng.dev(np.array(b, dtype=np.uint64))
    out = eng.mem.zeros(6, n)
    eng.check(eng.lib.p2hot_field_selftest_dev(eng.ctx, eng.ptr(da), eng.ptr(db), n, eng.ptr(out)))
    return eng.host(out)


def check_streams(eng):
    a, b = operands()
    for count in (len(a), 229, 37):  # whole waves; three waves and one of 37 lanes; one wave of 37 lanes
        o = run_selftest(eng, a[:count], b[:count])
        assert (o[5] == 0).all(), (count, np.flatnonzero(o[5])[:8], o[5][o[5] != 0][:8])
        assert (o[0] == np.array([x * y % P for x, y in zip(a[:count], b[:count])], dtype=np.uint64)).all()


def test_stream_selftest_on_the_emulator(emu):
    check_streams(emu)


@pytest.mark.gpu
def test_stream_selftest_on_the_gpu(gpu):
    check_streams(gpu)


@pytest.fixture
def lane_kernels(gpu):
    """Every launch through the one-permutation-per-lane kernels (poseidon.hpp: permute_batch_kernel, hash_leaves_kernel,
    merkle_level_kernel), which are the ones that run mul3cx / mul1cx.  By default launches of at most 2^13 permutations go to the
    word-per-lane kernels and of at most 2^15 to the quad kernels, both of which keep mul3cg / mul1cg, and the shapes below are far
    smaller than either threshold."""
    gpu.check(gpu.lib.p2hot_tune_quad(gpu.ctx, 0))
    gpu.check(gpu.lib.p2hot_tune_row(gpu.ctx, 0))
    try:
        yield gpu
    finally:
        gpu.check(gpu.lib.p2hot_tune_quad(gpu.ctx, 1 << 15))
        gpu.check(gpu.lib.p2hot_tune_row(gpu.ctx, 1 << 13))


@pytest.mark.gpu
def test_permutation_batch_on_the_gpu(lane_kernels, ora, kats):
    """100 states through the one-permutation-per-lane kernel (poseidon.hpp): the reference KAT inputs, edge states, random states"""
    from plonky2_amd.hash.poseidon import poseidon
    gpu = lane_kernels
    rng = np.random.default_rng(100)
    edge = [0, 1, E32 - 1, E32, E32 + 1, P - 1, P, P + 1, 2**63, 2**64 - E32, 2**64 - 1, 2**48, 0xFFFF * 2**48]
    states = [list(k["input"]) for k in kats["poseidon12"]]
    assert len(states) == 4
    states += [[v] * 12 for v in edge] + [[v if i == 0 else 0 for i in range(12)] for v in edge]
    states += [[edge[int(k)] for k in rng.integers(0, len(edge), 12)] for _ in range(30)]
    states += [[int(v) for v in rng.integers(0, 2**64, 12, dtype=np.uint64)] for _ in range(100 - len(states))]
    s = np.array(states, dtype=np.uint64)
    assert s.shape == (100, 12)
    got = poseidon(s.copy(), gpu)
    assert (got == np.stack([ora.poseidon(x) for x in s])).all()
    exp = np.array([k["output"] for k in kats["poseidon12"]], dtype=np.uint64)
    assert (got[:4] == exp).all()


@pytest.mark.gpu
def test_commit_parity_on_the_gpu(lane_kernels, ora):
    """W = 135 at 2^7 rows against the golden cap; W = 9 at 2^5 rows (the last absorb takes one word) against the oracle; leaves and
    every Merkle level through the one-permutation-per-lane kernels"""
    from plonky2_amd.fri.oracle import PolynomialBatch
    gpu = lane_kernels
    from plonky2_amd.util.synthetic import splitmix_columns_numpy
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "commit_caps.json")))["tiny_wires"]
    assert (g["W"], g["log_n"]) == (135, 7)
    b = PolynomialBatch.from_values(splitmix_columns_numpy(0, g["W"], 1 << g["log_n"]), g["rate_bits"], False, g["cap_height"], engine=gpu)
    assert b.merkle_tree.cap.entries.tolist() == g["cap"]
    rng = np.random.default_rng(9)
    vals = rng.integers(0, P, size=(9, 1 << 5), dtype=np.uint64)
    b = PolynomialBatch.from_values(vals, 3, False, 4, engine=gpu)
    ref = ora.commit(vals, 3, 4, True)
    assert (b.merkle_tree.cap.entries == ref["cap"]).all()
    assert (b.merkle_tree.digests == ref["digests"]).all()
