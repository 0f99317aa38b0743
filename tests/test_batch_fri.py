"""Batch FRI (plonky2/src/batch_fri/{oracle,prover}.rs over hash/batch_merkle_tree.rs) on the device against tests/batch_fri_ref.py,
the restatement that runs the commit phase literally (coset_fft, f * beta + v, coset_ifft).  Every comparison is exact."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import batch_fri_ref as ref
from tests.conftest import P, rand_field


def is_gpu(eng):
    return not bool(eng.lib.p2hot_is_emulated())


def _mats(rng, shape):
    return [rand_field(rng, 1 << h, w) for h, w in shape]


def _indices(h0):
    n = 1 << h0
    return sorted({0, n - 1, n // 2, max(n // 4 - 1, 0)})


# ------------------------------------------------------------------ 1. the restatement, by the reference alone (CPU)
def test_restated_tree_commit_single_and_mixed(ora):
    """the reference's commit_single and commit_mixed (hash/batch_merkle_tree.rs:185-294)"""
    mat_1 = [[0, 1], [2, 1], [2, 2], [0, 0]]
    fmt = ref.BatchMerkleTree([mat_1], 0)
    h1 = [ora.hash_or_noop(r) for r in mat_1]
    assert (fmt.digests[0:2] == h1[0:2]).all() and (fmt.digests[4:6] == h1[2:4]).all()
    layer_1 = [ora.two_to_one(h1[0], h1[1]), ora.two_to_one(h1[2], h1[3])]
    assert (fmt.digests[2:4] == layer_1).all()
    assert (fmt.cap.reshape(-1) == ora.two_to_one(layer_1[0], layer_1[1])).all()
    assert (fmt.open_batch(2) == [h1[3], layer_1[0]]).all()
    assert [v.tolist() for v in fmt.values(2)] == [[2, 2]]
    ref.verify_batch_merkle_proof_to_cap(fmt.values(2), fmt.leaf_heights, 2, fmt.cap, fmt.open_batch(2))

    mat_2 = [[1, 2, 1], [0, 2, 2]]
    fmt = ref.BatchMerkleTree([mat_1, mat_2], 0)
    assert (fmt.digests[0:4] == h1).all()
    new_leaves = [np.concatenate([layer_1[k], np.array(mat_2[k], dtype=np.uint64)]) for k in range(2)]
    l1 = [ora.hash_or_noop(new_leaves[0]), ora.hash_or_noop(new_leaves[1])]
    assert (fmt.digests[4:] == l1).all()
    assert (fmt.cap.reshape(-1) == ora.two_to_one(l1[0], l1[1])).all()
    assert (fmt.open_batch(1) == [h1[0], l1[1]]).all()
    assert [v.tolist() for v in fmt.values(1)] == [[2, 1], [1, 2, 1]]
    ref.verify_batch_merkle_proof_to_cap(fmt.values(1), fmt.leaf_heights, 1, fmt.cap, fmt.open_batch(1))


def test_restated_tree_verifies_and_rejects(ora):
    """test_batch_merkle_trees and _cap_at_leaves_height (:296-337); a one-group tree is the plain MerkleTree; one changed word fails"""
    from oracle import fri_verifier as fv
    rng = np.random.default_rng(11)
    fmt = ref.BatchMerkleTree(_mats(rng, [(10, 7), (6, 3), (5, 100)]), 3)
    assert len(fmt.digests) == 2 * (1024 - 8) and fmt.open_batch(0).shape == (7, 4)
    for index in (0, 1023, 512, 255):
        ref.verify_batch_merkle_proof_to_cap(fmt.values(index), fmt.leaf_heights, index, fmt.cap, fmt.open_batch(index))
    vals, sib = fmt.values(255), fmt.open_batch(255)
    bad = [v.copy() for v in vals]
    bad[2][99] ^= np.uint64(1)                      # a word of a lower group's row
    with pytest.raises(fv.VerificationError):
        ref.verify_batch_merkle_proof_to_cap(bad, fmt.leaf_heights, 255, fmt.cap, sib)
    bad_sib = sib.copy()
    bad_sib[4][0] ^= np.uint64(1)                   # layers 0..3 are segment 0 (1024 -> 64), layer 4 is the second segment's (64 -> 32)
    with pytest.raises(fv.VerificationError):
        ref.verify_batch_merkle_proof_to_cap(vals, fmt.leaf_heights, 255, fmt.cap, bad_sib)
    one = _mats(rng, [(4, 7)])
    fmt = ref.BatchMerkleTree(one, 4)
    assert len(fmt.digests) == 0
    for index in range(16):
        assert fmt.open_batch(index).shape == (0, 4)
        ref.verify_batch_merkle_proof_to_cap(fmt.values(index), fmt.leaf_heights, index, fmt.cap, fmt.open_batch(index))
    for cap_height in (0, 2, 4):
        fmt = ref.BatchMerkleTree(one, cap_height)
        digests, cap = ora.merkle_tree(one[0], cap_height)
        assert (fmt.digests == digests).all() and (fmt.cap == cap).all()


# ------------------------------------------------------------------ 2. the tree on the device
TREE_SHAPES = [([(10, 7), (6, 3), (5, 100)], 3), ([(4, 7)], 4), ([(6, 2), (5, 1), (3, 4), (2, 5)], 2), ([(7, 3), (6, 12), (5, 13)], 0)]
_tree_refs = {}


def _tree_case(k):
    if k not in _tree_refs:
        shape, cap_height = TREE_SHAPES[k]
        mats = _mats(np.random.default_rng(100 + k), shape)
        _tree_refs[k] = (mats, ref.BatchMerkleTree(mats, cap_height))
    return _tree_refs[k]


def _check_tree(got, exp, h0):
    assert (got.digests == exp.digests).all()
    assert (got.cap.entries == exp.cap).all()
    assert got.leaf_heights == exp.leaf_heights
    idx = _indices(h0)
    rows, paths = got.values_many(idx), got.open_batch_many(idx)
    for q, i in enumerate(idx):
        assert (rows[q] == np.concatenate(exp.values(i))).all(), i
        assert (paths[q] == exp.open_batch(i)).all(), i


@pytest.mark.parametrize("mapping", ["default", "row=0", "row=quad=0"])
@pytest.mark.parametrize("k", range(len(TREE_SHAPES)))
def test_batch_merkle_tree_on_the_device(eng, k, mapping):
    """digests, cap, values and open_batch under every leaf mapping: the word-per-lane, the quad and the lane-per-leaf kernels"""
    from plonky2_amd.hash.batch_merkle_tree import BatchMerkleTree
    from tests.emu_backend import EMU_TUNE_QUAD, EMU_TUNE_ROW
    mats, exp = _tree_case(k)
    quad, row = ((1 << 15), (1 << 13)) if is_gpu(eng) else (EMU_TUNE_QUAD, EMU_TUNE_ROW)
    try:
        if mapping != "default":
            eng.check(eng.lib.p2hot_tune_row(eng.ctx, 0))
        if mapping == "row=quad=0":
            eng.check(eng.lib.p2hot_tune_quad(eng.ctx, 0))
        got = BatchMerkleTree.new(mats, TREE_SHAPES[k][1], engine=eng)
        _check_tree(got, exp, TREE_SHAPES[k][0][0][0])
    finally:
        eng.check(eng.lib.p2hot_tune_quad(eng.ctx, quad))
        eng.check(eng.lib.p2hot_tune_row(eng.ctx, row))


def test_batch_tree_gathers_flag_an_index_out_of_range(eng):
    """the contract of p2hot_gather_rows_dev: a device-resident index past the tallest group zeroes its output and the next
    synchronisation returns EINVAL; the context works afterwards"""
    from plonky2_amd import _lib
    from plonky2_amd.hash.batch_merkle_tree import BatchMerkleTree, _tables
    mats, exp = _tree_case(2)
    tree = BatchMerkleTree.new(mats, 2, engine=eng)
    ptrs, strides, widths, logs = _tables(eng, tree._groups)
    d_idx = eng.dev(np.array([5, 64], dtype=np.uint64))
    out = eng.mem.zeros(2, 12)
    eng.check(eng.lib.p2hot_batch_merkle_rows_dev(eng.ctx, ptrs, strides, widths, logs, 4, eng.ptr(d_idx), 2, eng.ptr(out)))
    assert eng.lib.p2hot_ctx_sync(eng.ctx) == _lib.EINVAL
    got = eng.host(out)
    assert (got[0] == np.concatenate(exp.values(5))).all() and not got[1].any()
    paths = eng.mem.zeros(2, 4, 4)
    eng.check(eng.lib.p2hot_batch_merkle_paths_dev(eng.ctx, eng.ptr(tree._digests_dev), logs, 4, 2, eng.ptr(d_idx), 2, eng.ptr(paths)))
    assert eng.lib.p2hot_ctx_sync(eng.ctx) == _lib.EINVAL
    got = eng.host(paths)
    assert (got[0] == exp.open_batch(5)).all() and not got[1].any()
    eng.sync()
    assert (tree.values_many([63])[0] == np.concatenate(exp.values(63))).all()


# ------------------------------------------------------------------ 3. commit
def test_batch_oracle_commit(eng, ora):
    from plonky2_amd.batch_fri import BatchFriOracle
    from plonky2_amd.fri.oracle import PolynomialBatch
    rng = np.random.default_rng(3)
    degrees, rate_bits, cap_height = [9, 8, 8, 6], 1, 5
    values = [rand_field(rng, 1 << d, noncanonical=True) for d in degrees]
    got = BatchFriOracle.from_values(values, rate_bits, False, cap_height, engine=eng)
    coeffs = [ora.ifft(v % np.uint64(P)) for v in values]
    polys = got.polynomials
    assert all((a == b).all() for a, b in zip(polys, coeffs))
    exp = ref.BatchFriOracle(coeffs, rate_bits, cap_height)
    assert got.degree_bits == exp.degree_bits == [9, 8, 6]
    assert got.batch_merkle_tree.leaf_heights == [10, 9, 7] and got.batch_merkle_tree._widths == [1, 2, 1]

    def same_tree(o):
        t, e = o.batch_merkle_tree, exp.batch_merkle_tree
        assert (t.cap.entries == e.cap).all() and (t.digests == e.digests).all()
        idx = _indices(10)
        rows, paths = t.values_many(idx), t.open_batch_many(idx)
        for q, i in enumerate(idx):
            assert (rows[q] == np.concatenate(e.values(i))).all() and (paths[q] == e.open_batch(i)).all()
        assert [v.tolist() for v in t.values(777)] == [v.tolist() for v in e.values(777)]
        assert (t.open_batch(777) == e.open_batch(777)).all()

    same_tree(got)
    again = BatchFriOracle.from_coeffs(coeffs, rate_bits, False, cap_height, engine=eng)
    assert all((a == b).all() for a, b in zip(again.polynomials, coeffs))
    same_tree(again)
    # one degree: the plain PolynomialBatch
    cols = rand_field(rng, 5, 1 << 7)
    single = BatchFriOracle.from_values(list(cols), 2, False, 3, engine=eng)
    plain = PolynomialBatch.from_values(cols, 2, False, 3, engine=eng)
    assert (single.batch_merkle_tree.cap.entries == plain.merkle_tree.cap.entries).all()
    assert (single.batch_merkle_tree.digests == plain.merkle_tree.digests).all()
    assert (single.batch_merkle_tree.values_many([0, 511]) == plain.merkle_tree._getter(np.array([0, 511], dtype=np.uint64))).all()


# ------------------------------------------------------------------ 4. the commit phase
COMMIT_CASES = [([9, 8, 6], [1, 2, 1], 1, 5), ([7, 5], [2], 1, 2), ([10, 6], [4, 1], 3, 2), ([8], [2, 1], 1, 3)]


_commit_refs = {}


def _commit_ref(degrees, arity, rate_bits, cap_height):
    """the literal commit phase of one case, computed once: (coeffs, pre, trees, final, betas, the challenges drawn afterwards)"""
    from oracle import p2oracle as ora
    key = (tuple(degrees), tuple(arity), rate_bits, cap_height)
    if key not in _commit_refs:
        rng = np.random.default_rng(5)
        coeffs = [rand_field(rng, 1 << d, 2) for d in degrees]
        pre = rand_field(rng, 5)
        oc = ora.Challenger()
        oc.observe_elements(pre)
        lde, values = [], []
        for co in coeffs:
            pad = np.zeros((len(co) << rate_bits, 2), dtype=np.uint64)
            pad[:len(co)] = co
            lde.append(pad)
            values.append(ref.ext_coset_fft(pad, ref.G))
        etrees, efinal, ebetas = ref.batch_fri_committed_trees(lde[0], values, oc, rate_bits, cap_height, arity)
        _commit_refs[key] = (coeffs, pre, etrees, efinal, ebetas, oc.get_n_challenges(3))
    return _commit_refs[key]


def _commit_phase(eng, degrees, arity, rate_bits, cap_height):
    from plonky2_amd.batch_fri import batch_fri_committed_trees
    from plonky2_amd.iop.challenger import Challenger
    coeffs, pre, etrees, efinal, ebetas, after = _commit_ref(degrees, arity, rate_bits, cap_height)
    c = Challenger(eng)
    c.observe_elements(pre)
    trees, final, betas = batch_fri_committed_trees(coeffs, c, rate_bits, cap_height, arity, engine=eng)
    assert (final == efinal).all()
    assert [tuple(int(x) for x in b) for b in betas] == [tuple(b) for b in ebetas]
    for t, e in zip(trees, etrees):
        assert (t.cap.entries == e["cap"]).all()
        assert (np.asarray(t.digests).reshape(-1, 4) == e["digests"]).all()
        assert (t.leaves == e["leaves"]).all()
    assert c.get_n_challenges(3) == after   # the challenger's state afterwards
    return coeffs, pre, final, betas, trees


@pytest.mark.parametrize("degrees,arity,rate_bits,cap_height", COMMIT_CASES)
def test_batch_commit_phase_equals_the_literal_algorithm(eng, degrees, arity, rate_bits, cap_height):
    """joins after rounds 0 and 1 (the second sees shift' = g^8); a join in the last round; rate 3; a single instance, which must
    also equal p2hot_fri_commit_dev on the same input"""
    coeffs, pre, final, betas, trees = _commit_phase(eng, degrees, arity, rate_bits, cap_height)
    if len(degrees) == 1:
        from plonky2_amd.fri.prover import fri_committed_trees_device
        from plonky2_amd.iop.challenger import Challenger
        c = Challenger(eng)
        c.observe_elements(pre)
        ptrees, pfinal, pbetas = fri_committed_trees_device(eng.dev(np.ascontiguousarray(coeffs[0].T)), degrees[0], c, rate_bits, cap_height,
                                                            arity, engine=eng)
        assert (pfinal == final).all() and (pbetas == betas).all()
        for a, b in zip(ptrees, trees):
            assert (a.cap.entries == b.cap.entries).all() and (a.digests == b.digests).all() and (a.leaves == b.leaves).all()


# ------------------------------------------------------------------ 5. the whole proof
def _scenario(eng, ora, kind):
    """-> (degree_bits, polys per oracle, instances [(point, [(oi, pi)])], num_polys[i][o], fri parameters, rng)"""
    rng = np.random.default_rng({"multiple_polynomials": 21, "two_oracles": 22, "plain": 23, "default_thresholds": 24}[kind])
    if kind == "multiple_polynomials":   # batch_fri/prover.rs:342-478, with a grind
        degree_bits, widths = [9, 8, 6], [[1, 1, 1]]
        params = dict(rate_bits=1, cap_height=5, arity=[1, 2, 1], pow_bits=3, nq=10)
    elif kind == "two_oracles":          # widths 3 + 2 at degree 9, 2 + 1 at degree 7; two opening points
        degree_bits, widths = [9, 7], [[3, 2], [2, 1]]
        params = dict(rate_bits=1, cap_height=3, arity=[2, 2], pow_bits=2, nq=4)
    elif kind == "plain":                # one instance, one group
        degree_bits, widths = [7], [[4]]
        params = dict(rate_bits=2, cap_height=2, arity=[2, 1], pow_bits=2, nq=3)
    else:                                # the lane-per-leaf and quad mappings without tuning
        degree_bits, widths = [16, 14, 12], [[3, 2, 2]]
        params = dict(rate_bits=1, cap_height=4, arity=[2, 2, 4, 4], pow_bits=4, nq=6)
    polys = [[rand_field(rng, 1 << d) for d, w in zip(degree_bits, ws) for _ in range(w)] for ws in widths]
    return degree_bits, widths, polys, params, rng


def _prove_both(eng, ora, kind):
    from plonky2_amd.batch_fri import BatchFriOracle, FriInstanceInfo
    from plonky2_amd.iop.challenger import Challenger
    degree_bits, widths, polys, pr, rng = _scenario(eng, ora, kind)
    oracles = [BatchFriOracle.from_coeffs(ps, pr["rate_bits"], False, pr["cap_height"], engine=eng) for ps in polys]
    eoracles = [ref.BatchFriOracle(ps, pr["rate_bits"], pr["cap_height"]) for ps in polys]
    for o, e in zip(oracles, eoracles):
        assert (o.batch_merkle_tree.cap.entries == e.batch_merkle_tree.cap).all()
    c, oc = Challenger(eng), ora.Challenger()
    for ch in (c, oc):
        for e in eoracles:
            ch.observe_cap(e.batch_merkle_tree.cap)
    zeta = [int(x) for x in oc.get_extension_challenge()]
    assert list(c.get_extension_challenge()) == zeta
    instances, num_polys, openings = [], [], []
    for i, d in enumerate(degree_bits):
        first = [sum(ws[:i]) for ws in widths]                         # the instance's first polynomial in every oracle
        every = [(o, first[o] + p) for o, ws in enumerate(widths) for p in range(ws[i])]
        batches = [(zeta, every)]
        if kind == "two_oracles":                                      # g * zeta, the subgroup generator of THIS instance's degree
            g = ora.root_of_unity(d)
            batches.append(([zeta[0] * g % P, zeta[1] * g % P], [(0, first[0] + p) for p in range(widths[0][i])][:2] + [(1, first[1])]))
        instances.append(batches)
        num_polys.append([ws[i] for ws in widths])
        openings.append([[ora.eval_polys_ext(np.stack([polys[o][p]]), np.array(pt, dtype=np.uint64))[0] for (o, p) in ps] for pt, ps in batches])
    for ch in (c, oc):
        for opn in openings:
            for vals in opn:
                ch.observe_elements(np.asarray(vals, dtype=np.uint64).reshape(-1))
    vc = oc.clone()
    proof = BatchFriOracle.prove_openings(degree_bits, [FriInstanceInfo(b) for b in instances], oracles, c, pr["rate_bits"], pr["cap_height"],
                                          pr["arity"], pr["pow_bits"], pr["nq"], engine=eng)
    exp = ref.prove_openings(degree_bits, instances, eoracles, oc, pr["rate_bits"], pr["cap_height"], pr["arity"], pr["pow_bits"], pr["nq"])
    assert c.get_n_challenges(2) == oc.get_n_challenges(2)
    caps = [e.batch_merkle_tree.cap for e in eoracles]
    return proof, exp, (degree_bits, instances, num_polys, openings, caps, pr, vc)


def _assert_same_proof(proof, exp):
    from tests.wire_format import write_fri_proof
    assert proof["pow_witness"] == exp["pow_witness"] and proof["query_indices"] == exp["query_indices"]
    assert (proof["final_poly"] == exp["final_poly"]).all()
    assert len(proof["commit_phase_merkle_caps"]) == len(exp["commit_phase_merkle_caps"])
    for a, b in zip(proof["commit_phase_merkle_caps"], exp["commit_phase_merkle_caps"]):
        assert (a == b).all()
    for qa, qb in zip(proof["query_round_proofs"], exp["query_round_proofs"]):
        for (la, sa), (lb, sb) in zip(qa["initial_trees_proof"] + qa["steps"], qb["initial_trees_proof"] + qb["steps"]):
            assert (np.asarray(la) == lb).all() and (np.asarray(sa) == sb).all()
    assert write_fri_proof(proof) == write_fri_proof(exp)   # the FriProof's bytes (serialization/mod.rs:1595-1611)


def _verify(pf, ctx):
    from oracle import fri_verifier as fv
    degree_bits, instances, num_polys, openings, caps, pr, vc = ctx
    chal = fv.fri_challenges(vc.clone(), pf["commit_phase_merkle_caps"], pf["final_poly"], pf["pow_witness"], degree_bits[0], pr["rate_bits"],
                             pr["cap_height"], pr["nq"])
    ref.verify_batch_fri_proof(degree_bits, instances, num_polys, openings, chal, caps, pf, pr["rate_bits"], pr["arity"], pr["pow_bits"],
                               pr["nq"])


def _bump(a, *at):
    a = np.array(a, dtype=np.uint64)
    a[at] = (int(a[at]) + 1) % P
    return a


@pytest.mark.parametrize("kind", ["multiple_polynomials", "two_oracles"])
def test_batch_proof_equals_the_restated_prover_and_verifies(eng, ora, kind):
    from oracle import fri_verifier as fv
    proof, exp, ctx = _prove_both(eng, ora, kind)
    _assert_same_proof(proof, exp)
    _verify(proof, ctx)
    degree_bits, pr = ctx[0], ctx[5]
    seg0_layers = degree_bits[0] - degree_bits[1]   # the layers of an initial path that belong to the first segment

    def tampered(edit):
        bad = copy.deepcopy(proof)
        edit(bad)
        with pytest.raises(fv.VerificationError):
            _verify(bad, ctx)

    def lower_row(bad):      # a word of a lower group's opened row: the last word of oracle 0's leaf
        leaf, sib = bad["query_round_proofs"][0]["initial_trees_proof"][0]
        bad["query_round_proofs"][0]["initial_trees_proof"][0] = (_bump(leaf, len(leaf) - 1), sib)

    def second_segment_sibling(bad):
        leaf, sib = bad["query_round_proofs"][1]["initial_trees_proof"][0]
        bad["query_round_proofs"][1]["initial_trees_proof"][0] = (leaf, _bump(sib, seg0_layers, 2))

    def step_eval(bad):
        evals, sib = bad["query_round_proofs"][-1]["steps"][1]
        bad["query_round_proofs"][-1]["steps"][1] = (_bump(evals, 1, 0), sib)

    def step_path(bad):
        evals, sib = bad["query_round_proofs"][0]["steps"][0]
        bad["query_round_proofs"][0]["steps"][0] = (evals, _bump(sib, 0, 3))

    def final_coeff(bad):
        bad["final_poly"] = _bump(bad["final_poly"], 1, 1)

    for edit in (lower_row, second_segment_sibling, step_eval, step_path, final_coeff):
        tampered(edit)
    # the witness: another one is almost surely invalid, and it moves the query indices
    for step in range(1, 6):
        bad = copy.deepcopy(proof)
        bad["pow_witness"] = int(bad["pow_witness"]) + step
        try:
            _verify(bad, ctx)
        except fv.VerificationError:
            break
    else:
        raise AssertionError("five consecutive PoW witnesses verify")


def test_one_instance_one_group_equals_prove_openings(eng, ora):
    """the batch path over a single degree is the plain path, byte for byte"""
    from plonky2_amd.fri.oracle import FriBatchInfo, PolynomialBatch, prove_openings
    from plonky2_amd.iop.challenger import Challenger
    from tests.wire_format import write_fri_proof
    proof, exp, ctx = _prove_both(eng, ora, "plain")
    _assert_same_proof(proof, exp)
    degree_bits, widths, polys, pr, _ = _scenario(eng, ora, "plain")
    plain = PolynomialBatch.from_coeffs(np.stack(polys[0]), pr["rate_bits"], False, pr["cap_height"], engine=eng)
    c = Challenger(eng)
    c.observe_cap(plain.merkle_tree.cap.entries)
    zeta = c.get_extension_challenge()
    for vals in ctx[3][0]:
        c.observe_elements(np.asarray(vals, dtype=np.uint64).reshape(-1))
    pp = prove_openings([FriBatchInfo(zeta, [(0, p) for p in range(4)])], [plain], c, pr["rate_bits"], pr["cap_height"], pr["arity"],
                        pr["pow_bits"], pr["nq"], engine=eng)
    assert write_fri_proof(pp) == write_fri_proof(proof)


def test_batch_pow_witness_outside_the_first_search_range(eng, ora, monkeypatch):
    """The batch path shares the opening-proof core with p2hot_prove_openings, and with it the rewind of the transcript when the
    range searched on the device holds no witness (tests/test_prove_openings.py, test_pow_witness_outside_the_first_search_range).
    Forced here by shrinking the range to 2^3 candidates (P2HOT_POW_RANGE_LOG) over the accepted proof of
    test_batch_prove_openings_validation: the proof's bytes and the transcript afterwards are unchanged, and equal the restated prover's."""
    from plonky2_amd.batch_fri import BatchFriOracle, FriInstanceInfo
    from plonky2_amd.iop.challenger import Challenger
    from tests.wire_format import write_fri_proof
    rng = np.random.default_rng(8)
    degree_bits, rate_bits, cap_height, arity, pow_bits, nq, z = [7, 5], 1, 2, [2], 9, 3, [3, 4]
    polys = [rand_field(rng, 1 << 7), rand_field(rng, 1 << 5)]
    instances = [[(z, [(0, 0)])], [(z, [(0, 1)])]]
    oracle = BatchFriOracle.from_coeffs(polys, rate_bits, False, cap_height, engine=eng)
    runs = []
    for rng_log in (None, "-6"):
        if rng_log is None:
            monkeypatch.delenv("P2HOT_POW_RANGE_LOG", raising=False)
        else:
            monkeypatch.setenv("P2HOT_POW_RANGE_LOG", rng_log)
        c = Challenger(eng)
        c.observe_elements(np.arange(5, dtype=np.uint64))
        proof = BatchFriOracle.prove_openings(degree_bits, [FriInstanceInfo(b) for b in instances], [oracle], c, rate_bits, cap_height, arity,
                                              pow_bits, nq, engine=eng)
        runs.append((proof, c.get_n_challenges(3)))
    (p0, t0), (p1, t1) = runs
    assert p0["pow_witness"] >= 8            # the forced run did leave its first range (the seed was picked for this)
    assert write_fri_proof(p0) == write_fri_proof(p1) and p0["query_indices"] == p1["query_indices"] and t0 == t1
    oc = ora.Challenger()
    oc.observe_elements(np.arange(5, dtype=np.uint64))
    exp = ref.prove_openings(degree_bits, instances, [ref.BatchFriOracle(polys, rate_bits, cap_height)], oc, rate_bits, cap_height, arity,
                             pow_bits, nq)
    _assert_same_proof(p1, exp)
    assert oc.get_n_challenges(3) == t1


# ------------------------------------------------------------------ 6. validation
def _commit_raw(eng, degrees, rate_bits, cap_height, flags=0, seed=1):
    rng = np.random.default_rng(seed)
    host = [rand_field(rng, 1 << d) for d in degrees]
    W = len(host)
    ptrs = (C.c_void_p * max(W, 1))(*[c.ctypes.data for c in host])
    log_n = (C.c_uint * max(W, 1))(*degrees)
    h = C.c_void_p()
    rc = eng.lib.p2hot_batch_oracle_commit(eng.ctx, ptrs, log_n, W, rate_bits, cap_height, 0, flags, None, None, None, C.byref(h))
    return rc, h


COMMIT_ERRORS = [([], 0, 0, "EINVAL", "W = 0"), ([5, 6], 0, 0, "EINVAL", "log_n"), ([6, 4], 6, 0, "EINVAL", "cap_height"),
                 ([6, 4], 2, 25 << 8, "EUNSUPPORTED", "Poseidon-only")]


@pytest.mark.parametrize("degrees,cap_height,flags,code,word", COMMIT_ERRORS)
def test_batch_oracle_commit_validation(eng, degrees, cap_height, flags, code, word):
    from plonky2_amd import _lib
    rc, h = _commit_raw(eng, degrees, 1, cap_height, flags)
    text = eng.lib.p2hot_last_error(eng.ctx).decode()
    assert rc == getattr(_lib, code) and not h.value and word in text, (rc, text)
    _commit_phase(eng, *COMMIT_CASES[0])   # the context still runs the first commit-phase shape


# keyword overrides of a proof over degrees 7 / 5 (rate 1, cap 2, arity [2]) that is accepted as it stands
PROVE_ERRORS = [
    (dict(degree_bits=(), instances=()), "EINVAL", "n_instances"),
    (dict(degree_bits=(5, 7), instances="reversed"), "EINVAL", "degree_bits"),
    (dict(degree_bits=(8, 5), arity=(3,)), "EINVAL", "oracle 0"),          # the tallest group is 2^(7 + 1) rows
    (dict(instances="wrong degree"), "EINVAL", "polynomial (0, 0)"),       # a polynomial of degree 2^7 in instance 1
    (dict(arity=(1, 2)), "EINVAL", "instance 1"),                          # 7 -> 6 -> 4: the length 2^5 is never reached
    (dict(arity=(2, 6)), "EINVAL", "arity"),                               # round 1 does not divide the degree bound
    (dict(arity=(2, 3, 2)), "EINVAL", "cap"),                              # 2^8 -> 2^6 -> 2^3 -> 2 leaves under a 2^2 cap
    (dict(max_num_query_steps=3), "EINVAL", "max_num_query_steps"),
    (dict(final_poly_coeff_len=64), "EINVAL", "final_poly_coeff_len"),
    (dict(oracles="other rate"), "EINVAL", "oracle 0"),
    (dict(oracles="other context"), "EINVAL", "another context"),
    (dict(challenger="keccak"), "EUNSUPPORTED", "Poseidon-only"),
]


@pytest.mark.parametrize("case", range(len(PROVE_ERRORS)))
def test_batch_prove_openings_validation(eng, case):
    from plonky2_amd import Engine, _lib
    from plonky2_amd.batch_fri import BatchFriOracle, FriInstanceInfo
    from plonky2_amd.hash.keccak import KeccakHash
    from plonky2_amd.iop.challenger import Challenger
    rng = np.random.default_rng(8)
    rate_bits, cap_height, z = 1, 2, [3, 4]
    polys = [rand_field(rng, 1 << 7), rand_field(rng, 1 << 5)]
    oracle = BatchFriOracle.from_coeffs(polys, rate_bits, False, cap_height, engine=eng)
    inst = [FriInstanceInfo([(z, [(0, 0)])]), FriInstanceInfo([(z, [(0, 1)])])]

    def prove(degree_bits=(7, 5), instances=inst, oracles=(oracle,), challenger=None, arity=(2,), **kw):
        try:
            BatchFriOracle.prove_openings(list(degree_bits), list(instances), list(oracles), challenger or Challenger(eng), rate_bits,
                                          cap_height, list(arity), 1, 2, engine=eng, **kw)
        except _lib.P2HotError as e:
            return e.code, str(e)
        return _lib.OK, ""

    kw, code, word = PROVE_ERRORS[case]
    kw = dict(kw)
    if case == 0:
        assert prove()[0] == _lib.OK
    if kw.get("instances") == "reversed":
        kw["instances"] = inst[::-1]
    elif kw.get("instances") == "wrong degree":
        kw["instances"] = [inst[0], FriInstanceInfo([(z, [(0, 0)])])]
    if kw.get("oracles") == "other rate":
        kw["oracles"] = (BatchFriOracle.from_coeffs(polys, 2, False, cap_height, engine=eng),)
    elif kw.get("oracles") == "other context":
        if is_gpu(eng):
            eng2 = Engine(0)
        else:
            from tests.emu_backend import emu_engine
            eng2 = emu_engine()
        kw["oracles"] = (BatchFriOracle.from_coeffs(polys, rate_bits, False, cap_height, engine=eng2),)
    if kw.get("challenger") == "keccak":
        kw["challenger"] = Challenger(eng, hasher=KeccakHash(25))
    rc, text = prove(**kw)
    assert rc == getattr(_lib, code) and word in text, (kw, rc, text)
    _commit_phase(eng, *COMMIT_CASES[0])   # the context still runs the first commit-phase shape


def test_batch_dev_entry_points_validate(eng):
    """the device-pointer commit phase checks its own schedule and hasher, and a tree its heights"""
    from plonky2_amd import _lib
    from plonky2_amd.hash.batch_merkle_tree import BatchMerkleTree
    from plonky2_amd.hash.keccak import KeccakHash
    from plonky2_amd.iop.challenger import Challenger
    lib = eng.lib
    c, kc = Challenger(eng), Challenger(eng, hasher=KeccakHash(25))
    planes = [eng.mem.zeros(2, 1 << 7), eng.mem.zeros(2, 1 << 5)]
    ptrs = (C.c_void_p * 2)(*[eng.mem.ptr(p) for p in planes])
    ab = (C.c_uint * 2)(1, 2)
    rc = lib.p2hot_batch_fri_commit_dev(eng.ctx, ptrs, (C.c_uint * 2)(7, 5), 2, 1, 2, ab, 2, c._h, None, None, 0, None, None, None)
    assert rc == _lib.EINVAL and "instance 1" in lib.p2hot_last_error(eng.ctx).decode()
    rc = lib.p2hot_batch_fri_commit_dev(eng.ctx, ptrs, (C.c_uint * 2)(7, 5), 2, 1, 2, ab, 2, kc._h, None, None, 0, None, None, None)
    assert rc == _lib.EUNSUPPORTED and "Poseidon-only" in lib.p2hot_last_error(eng.ctx).decode()
    with pytest.raises(_lib.P2HotError, match="decrease strictly"):
        BatchMerkleTree.new([np.zeros((4, 1), np.uint64), np.zeros((4, 2), np.uint64)], 0, engine=eng)
    with pytest.raises(_lib.P2HotError, match="cap_height"):
        BatchMerkleTree.new([np.zeros((8, 1), np.uint64), np.zeros((2, 2), np.uint64)], 2, engine=eng)
    _commit_phase(eng, *COMMIT_CASES[0])


# ------------------------------------------------------------------ 7. at the default thresholds (MI355X only)
@pytest.mark.gpu
def test_batch_tree_at_default_thresholds(gpu):
    from plonky2_amd.hash.batch_merkle_tree import BatchMerkleTree
    shape, cap_height = [(17, 20), (15, 8), (13, 4)], 4   # 2^17 leaves: lane per leaf; 2^15: quad; 2^13: word per lane
    mats = _mats(np.random.default_rng(7), shape)
    _check_tree(BatchMerkleTree.new(mats, cap_height, engine=gpu), ref.BatchMerkleTree(mats, cap_height), 17)


@pytest.mark.gpu
def test_batch_proof_at_default_thresholds(gpu, ora):
    proof, exp, ctx = _prove_both(gpu, ora, "default_thresholds")
    _assert_same_proof(proof, exp)
    _verify(proof, ctx)
