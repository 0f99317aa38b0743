"""The gate kernels of the quotient (gates::cheap_gates_kernel, gates::poseidon_gate_kernel, the launches of gates_launch in
csrc/host_plonk.hpp) at the edges tests/test_gates.py leaves out: more cheap descriptors than one launch carries, operands from
the field's edge grid, alphas handed over as alpha + P, a quotient step above 1, a blinded and a Keccak-hashed commitment.  Every
comparison is bit for bit with tests/gates_ref.py over tests/vanishing_ref.py's LDE rows; the helpers are tests/test_gates.py's."""
import numpy as np
import pytest

from tests import gates_ref as gr
from tests import test_gates as tg
from tests import vanishing_ref as vr
from tests.conftest import P

W = tg.W


# ------------------------------------------------------------------ more than gates::MAX_CHEAP (32) cheap descriptors
def _many_cheap(count):
    """`count` descriptors of the cheap kinds with small parameters, three Noops and one Poseidon among the first 32 of them (the
    cheap count runs behind the descriptor index from index 3 on), rows = indices, selector groups of eight"""
    cycle = [(gr.CONSTANT, 1, 0), (gr.ARITHMETIC, 1, 0), (gr.PUBLIC_INPUT, 0, 0), (gr.MUL_EXT, 2, 0), (gr.BASE_SUM, 3, 2),
             (gr.ARITHMETIC_EXT, 1, 0), (gr.CONSTANT, 2, 0), (gr.ARITHMETIC, 4, 0), (gr.MUL_EXT, 1, 0), (gr.ARITHMETIC_EXT, 3, 0),
             (gr.BASE_SUM, 2, 4), (gr.ARITHMETIC, 2, 0), (gr.MUL_EXT, 4, 0), (gr.ARITHMETIC_EXT, 2, 0), (gr.ARITHMETIC, 3, 0),
             (gr.MUL_EXT, 3, 0), (gr.ARITHMETIC_EXT, 4, 0)]
    kinds = [cycle[k % len(cycle)] for k in range(count)]
    for at, kind in ((3, gr.NOOP), (10, gr.POSEIDON), (17, gr.NOOP), (29, gr.NOOP)):
        kinds.insert(at, (kind, 0, 0))
    ns = -(-len(kinds) // 8)
    gates = [gr.Gate(kind, row, row // 8, (row // 8 * 8, min(row // 8 * 8 + 8, len(kinds))), p0, p1) for row, (kind, p0, p1) in enumerate(kinds)]
    return gates, ns


@pytest.mark.parametrize("count", [31, 32, 33, 64, 65])
def test_gate_sums_split_over_several_launches(eng, count):
    """exactly MAX_CHEAP - 1, MAX_CHEAP, MAX_CHEAP + 1, 2 MAX_CHEAP and 2 MAX_CHEAP + 1 cheap descriptors: one launch that is not
    full, one that is and nothing behind it, a second launch of one descriptor, ...; 5 to 9 selector polynomials.  A descriptor
    launched twice or not at all changes every point: the points are nonzero and equal the restatement's"""
    gates, ns = _many_cheap(count)
    cheap = [g for g in gates if g.kind not in (gr.NOOP, gr.POSEIDON)]
    assert len(cheap) == count and len(gates) == count + 4 and ns == -(-(count + 4) // 8)
    assert sum(g.kind not in (gr.NOOP, gr.POSEIDON) for g in gates[:32]) == 28          # cheap count != descriptor index
    assert {g.kind for g in gates} == set(range(8))
    q = tg._instance(900 + count, gates, ns, 3, nc=2)
    exp = tg._ref_sums(q, tg._ldes(q))
    got = tg._device_sums(eng, q, tg._commit(eng, q), 2)
    assert got.shape == exp.shape == (2, 64)
    assert (got == exp).all() and exp.all()


# ------------------------------------------------------------------ edge operands
GRID = [0, 1, 2, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, P - 2**32, P - 2, P - 1]     # canonical: the LDE canonicalises
FILLS = ["seed0", "seed1", "seed2", "seed3", "zeros", "p_minus_1"]


def _constant_instance(fill, name):
    """every committed column is a constant (so is its LDE at every coset point): the wires the gate reads and the gate constants
    c0, c1 from GRID, the one selector polynomial = the gate's row index 1"""
    kind, p0, p1 = tg.ALONE[name]
    gates = tg._alone(kind, p0, p1, row=1, group=(0, 3))
    nw = max(gr.num_wires(gates[0]), 1)
    if fill.startswith("seed"):
        rng = np.random.default_rng(1000 * int(fill[4:]) + 10 * kind + p0)
        w, c, pih = ([GRID[k] for k in rng.integers(0, len(GRID), size=cnt)] for cnt in (nw, 2, 4))
    else:
        v = 0 if fill == "zeros" else P - 1
        w, c, pih = [v] * nw, [v] * 2, [v] * 4
    rng = np.random.default_rng(5)
    n = 8
    q = dict(gates=gates, ns=1, nls=0, log_n=3, n=n, qdf=8, pih=pih, sigmas_first=3, alphas=[int(v) for v in tg._rand(rng, 2)],
             wires=np.repeat(np.asarray(w, dtype=np.uint64)[:, None], n, axis=1),
             cs=np.repeat(np.asarray([1] + c + [7], dtype=np.uint64)[:, None], n, axis=1))     # [selector, c0, c1, one "sigma"]
    return q, w, [1] + c + [7]


@pytest.mark.parametrize("name", sorted(tg.ALONE))
def test_gate_sums_on_edge_operands(eng, name):
    """0, 1, 2, 2^32 -+ 1, 2^63, P - 2^32, P - 1 ... meet in ext_mul + mul_add, the BaseSum range product, Poseidon's add_canon
    chains and S-boxes and the filter: constant columns put them into the kernels at every point.  (No "every term nonzero" here:
    it does not hold for these inputs)"""
    for fill in FILLS:
        q, w, c = _constant_instance(fill, name)
        ldes = tg._ldes(q)
        for L in (0, 37):        # the restatement's LDE of a constant column is that constant
            assert ldes["wires"].row(L) == w and ldes["cs"].row(L) == c
        exp = gr.reduced_sums(vr.BASE, q["gates"], 1, 0, w, c, q["pih"], q["alphas"])
        got = tg._device_sums(eng, q, tg._commit(eng, q), 2)
        assert got.shape == (2, 64)
        assert (got == np.asarray(exp, dtype=np.uint64)[:, None]).all(), fill


# ------------------------------------------------------------------ alphas in [P, 2^64)
def test_gate_sums_noncanonical_alphas(eng):
    """the caller's alphas are raw GoldilocksField(u64) words: alpha + P gives the sums of alpha (the full set: both kernels read
    the alpha-power table; three challenges)"""
    gates, ns = tg._full_set()
    q = tg._instance(70, gates, ns, 3, nc=3)
    q["alphas"] = [2**32 - 2, 3, q["alphas"][2]]
    exp = tg._ref_sums(q, tg._ldes(q))
    b = tg._commit(eng, q)
    shifted = [q["alphas"][0] + P, q["alphas"][1] + P, q["alphas"][2]]
    assert max(shifted) < 1 << 64
    got = tg._device_sums(eng, q, b, 3)
    assert (got == exp).all() and exp.all()
    assert tg._device_sums(eng, q, b, 3, alphas=shifted).tobytes() == got.tobytes()


# ------------------------------------------------------------------ a quotient step above 1, other commitments
def _factor4_set():
    """the eight kinds as a factor-4 circuit groups them (group size + largest degree <= 5; degrees 0 1 1 2 3 3 3): three, two, two;
    Poseidon (degree 7: no such circuit holds it -- gate_sums needs values only) alone in a fourth group"""
    kinds = [(gr.NOOP, 0, 0), (gr.CONSTANT, 2, 0), (gr.PUBLIC_INPUT, 0, 0), (gr.BASE_SUM, 63, 2), (gr.ARITHMETIC, 20, 0),
             (gr.ARITHMETIC_EXT, 10, 0), (gr.MUL_EXT, 13, 0), (gr.POSEIDON, 0, 0)]
    groups = [(0, 3), (3, 5), (5, 7), (7, 8)]
    return [gr.Gate(kind, row, next(k for k, (a, b) in enumerate(groups) if a <= row < b),
                    next(g for g in groups if g[0] <= row < g[1]), p0, p1) for row, (kind, p0, p1) in enumerate(kinds)], len(groups)


@pytest.mark.parametrize("rate_bits,qdf", [(3, 4), (4, 8)])
def test_gate_sums_read_every_second_lde_row(eng, rate_bits, qdf):
    """qbits = rate_bits - 1: point i is LDE row bitrev(2 i), the kernels' lanes cover the first half of the committed matrix"""
    gates, ns = _factor4_set() if qdf == 4 else tg._full_set()
    q = tg._instance(80 + qdf, gates, ns, 4, nc=2, qdf=qdf)
    assert vr.quotient_rows(1, 4, rate_bits, vr.log2_ceil(qdf))[0] == (1, 2)
    exp = tg._ref_sums(q, tg._ldes(q, rate_bits=rate_bits))
    got = tg._device_sums(eng, q, tg._commit(eng, q, rate_bits=rate_bits), 2)
    assert got.shape == exp.shape == (2, 16 * (1 << rate_bits) // 2)
    assert (got == exp).all() and exp.all()


_F8 = {}


def _factor8():
    """the full set at factor 8, rate 3, 2^4 rows, with the restatement's sums: shared by the two tests below"""
    if not _F8:
        gates, ns = tg._full_set()
        q = tg._instance(90, gates, ns, 4, nc=2)
        _F8["v"] = (q, tg._ref_sums(q, tg._ldes(q)))
    return _F8["v"]


def test_gate_sums_of_a_blinded_wires_commitment(eng):
    """four salt columns behind the 135 wires (oracle.rs:133-137): the gates read the wire columns of THAT LDE matrix.  The
    reference rows are the library's own committed leaves without their salt words, not a second interpolation"""
    from plonky2_amd.fri.oracle import PolynomialBatch
    q, plain = _factor8()
    N = 16 << tg.RATE_BITS
    salts = tg._rand(np.random.default_rng(91), 4, N)
    b = tg._commit(eng, q, ("cs",))
    b["wires"] = PolynomialBatch.from_values(q["wires"], tg.RATE_BITS, True, 0, engine=eng, salts=salts)
    leaves = b["wires"].merkle_tree.leaves
    assert leaves.shape == (N, W + 4) and leaves[:, W:].all() and b["wires"].salt_size == 4
    ldes = {"wires": vr.Leaves(leaves[:, :W], 4, tg.RATE_BITS), "cs": tg._ldes(q, ("cs",))["cs"]}
    exp = tg._ref_sums(q, ldes)
    got = tg._device_sums(eng, q, b, 2)
    assert (got == exp).all() and exp.all()
    assert (exp == plain).all()          # (salting adds leaf words and leaves the polynomials alone)


def test_gate_sums_of_keccak_hashed_commitments(eng):
    """p2hot_gate_sums takes commitments of any hasher: KeccakHash<25> trees over the same LDE matrices, the same sums"""
    from plonky2_amd.hash.keccak import KeccakHash
    q, exp = _factor8()
    keccak = tg._commit(eng, q, hasher=KeccakHash(25))
    poseidon = tg._commit(eng, q)
    assert (keccak["wires"].merkle_tree.cap.entries != poseidon["wires"].merkle_tree.cap.entries).any()
    got = tg._device_sums(eng, q, keccak, 2)
    assert got.tobytes() == tg._device_sums(eng, q, poseidon, 2).tobytes() and (got == exp).all()
