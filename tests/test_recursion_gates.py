"""The recursion gates' constraints on the device -- PoseidonMds, Reducing, ReducingExtension, RandomAccess, Exponentiation and
CosetInterpolation (gates::recursion_gates_kernel, gates::mds_gate_kernel of csrc/gates_recursion.hpp) through p2hot_gate_sums,
p2hot_quotient_polys_gates and p2hot_quotient_polys_lookup_gates -- against tests/recursion_gates_ref.py, a big-integer restatement
that shares no code with the library (its barycentric weights are the definition's; the library's are x_k / N), and the quotient the
device produced put through the verifier's identity (plonk/verifier.rs:83-98) with the gates evaluated over the extension field.

Shapes are tests/test_gates.py's, and so are the helpers that do not depend on the gate kinds: 135 wires (80 routed), rate_bits 3,
quotient degree factor 8; 2^4 rows (128 points: one partly filled workgroup) for one gate, 2^6 rows (512 points) for sets.  At
factor 8 nothing is trimmed, so a broken witness shows as a failed identity there and as "Quotient has failed" at factor 7."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import gates_ref as gr
from tests import recursion_gates_ref as rr
from tests import test_gates as tg
from tests import vanishing_ref as vr
from tests.conftest import P, ROOT
from tests.pyref import G

W, NUM_ROUTED, RATE_BITS, QDF, NUM_GATE_CONSTS = tg.W, tg.NUM_ROUTED, tg.RATE_BITS, tg.QDF, tg.NUM_GATE_CONSTS

# name -> (kind, param0, param1); RandomAccess as (copies, bits, extra), CosetInterpolation as (subgroup_bits, degree)
ALONE = {"poseidon_mds": (rr.POSEIDON_MDS, 0, 0)}
ALONE.update({"reducing_%d" % n: (rr.REDUCING, n, 0) for n in (43, 1, 2)})
ALONE.update({"reducing_ext_%d" % n: (rr.REDUCING_EXT, n, 0) for n in (32, 1)})
ALONE.update({"exponentiation_%d" % n: (rr.EXPONENTIATION, n, 0) for n in (66, 1, 2)})
ALONE.update({"random_access_%d_%d_%d" % t: (rr.RANDOM_ACCESS, t[0], rr.ra_param1(t[1], t[2])) for t in ((4, 4, 2), (1, 1, 0), (1, 6, 0), (2, 5, 2))})
ALONE.update({"coset_interpolation_%d_%d" % t: (rr.COSET_INTERPOLATION, t[0], t[1]) for t in ((4, 6), (4, 5), (3, 8), (3, 2), (1, 2), (5, 8))})
# (wires, constraints) by the table of include/p2hot.h, worked out by hand
TABLE = {"poseidon_mds": (48, 24), "reducing_43": (133, 86), "reducing_1": (7, 2), "reducing_2": (10, 4), "reducing_ext_32": (132, 64),
         "reducing_ext_1": (8, 2), "exponentiation_66": (134, 67), "exponentiation_1": (4, 2), "exponentiation_2": (6, 3),
         "random_access_4_4_2": (90, 26), "random_access_1_1_0": (5, 3), "random_access_1_6_0": (72, 8), "random_access_2_5_2": (80, 16),
         "coset_interpolation_4_6": (47, 12), "coset_interpolation_4_5": (51, 16), "coset_interpolation_3_8": (23, 4),
         "coset_interpolation_3_2": (47, 28), "coset_interpolation_1_2": (11, 4), "coset_interpolation_5_8": (87, 20)}


def _groups(gates_by_degree, qdf):
    """selector_polynomials (gates/selectors.rs:101-160) on gates sorted by degree, max_degree = factor + 1: one group if
    largest degree + count - 1 <= max_degree, else greedily while size + the next gate's degree < max_degree -- every group then has
    size + largest degree <= factor + 1"""
    degs, max_degree = [rr.degree(g) for g in gates_by_degree], qdf + 1
    assert degs == sorted(degs) and degs[-1] < max_degree
    if degs[-1] + len(degs) - 1 <= max_degree:
        return [(0, len(degs))]
    groups, start = [], 0
    while start < len(degs):
        size = 0
        while start + size < len(degs) and size + degs[start + size] < max_degree:
            size += 1
        groups.append((start, start + size))
        start += size
    return groups


def _set(kinds, qdf):
    protos = [gr.Gate(kind, 0, 0, (0, 1), p0, p1) for kind, p0, p1 in kinds]
    groups = _groups(protos, qdf)
    assert all(b - a + max(rr.degree(p) for p in protos[a:b]) <= qdf + 1 for a, b in groups)
    out = []
    for row, (kind, p0, p1) in enumerate(kinds):
        s = next(k for k, (a, b) in enumerate(groups) if a <= row < b)
        out.append(gr.Gate(kind, row, s, groups[s], p0, p1))
    return out, len(groups)


RECURSION_KINDS = [(gr.NOOP, 0, 0), (gr.CONSTANT, 2, 0), (gr.PUBLIC_INPUT, 0, 0), (rr.POSEIDON_MDS, 0, 0), (rr.REDUCING, 43, 0),
                   (rr.REDUCING_EXT, 32, 0), (gr.BASE_SUM, 63, 2), (gr.ARITHMETIC, 20, 0), (gr.ARITHMETIC_EXT, 10, 0), (gr.MUL_EXT, 13, 0),
                   (rr.EXPONENTIATION, 66, 0), (rr.RANDOM_ACCESS, 4, rr.ra_param1(4, 2)), (rr.COSET_INTERPOLATION, 4, 6), (gr.POSEIDON, 0, 0)]
ROW_RANDOM_ACCESS, ROW_COSET = 11, 12


def _recursion_set(qdf=QDF):
    """the fourteen gates of a recursion circuit under standard_recursion_config in the builder's order (by degree); at factor 7
    without Poseidon, whose degree 7 no group of such a circuit holds"""
    return _set(RECURSION_KINDS if qdf >= 8 else RECURSION_KINDS[:-1], qdf)


def test_recursion_set_groups():
    gates, ns = _recursion_set()
    assert ns == 4 and sorted({g.group for g in gates}) == [(0, 7), (7, 11), (11, 13), (13, 14)]
    gates, ns = _recursion_set(7)
    assert ns == 4 and sorted({g.group for g in gates}) == [(0, 6), (6, 10), (10, 12), (12, 13)]


def _instance(seed, gates, num_selectors, log_n, nls=0, satisfied=False, nc=4, qdf=QDF):
    """tests/test_gates.py's _instance with the witness filler of all fourteen kinds"""
    if not satisfied:
        return tg._instance(seed, gates, num_selectors, log_n, nls=nls, nc=nc, qdf=qdf)
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    row_gate = [i % len(gates) for i in range(n)]
    sel = tg._selectors(gates, num_selectors, row_gate)
    consts = tg._rand(rng, NUM_GATE_CONSTS, n)
    pih = [int(v) for v in tg._rand(rng, 4)]
    k_is = [pow(G, j, P) for j in range(NUM_ROUTED)]
    sub = vr.subgroup(log_n)
    perm = np.arange(NUM_ROUTED * n)
    w = [[int(v) for v in col] for col in tg._rand(rng, W, n)]
    free = [(j, i) for i in range(n) for j in range(NUM_ROUTED) if j not in set(rr.determined_wires(gates[row_gate[i]]))]
    picks = [free[t] for t in rng.choice(len(free), size=min(60, len(free) // 3 * 3), replace=False)]
    for c in range(0, len(picks), 3):
        cyc = picks[c:c + 3]
        for t, (j, i) in enumerate(cyc):
            w[j][i] = w[cyc[0][0]][cyc[0][1]]
            nj, ni = cyc[(t + 1) % 3]
            perm[j * n + i] = nj * n + ni
    for i in range(n):
        row = [w[j][i] for j in range(W)]
        rr.fill_witness(rng, gates[row_gate[i]], row, [int(consts[0][i]), int(consts[1][i])], pih)
        for j in range(W):
            w[j][i] = row[j]
    wires = np.asarray(w, dtype=np.uint64)
    sigmas = np.asarray([[k_is[p // n] * sub[p % n] % P for p in perm[j * n:(j + 1) * n]] for j in range(NUM_ROUTED)], dtype=np.uint64)
    cs = np.concatenate([sel, tg._rand(rng, nls, n), consts, sigmas])
    betas, gammas, alphas = ([int(v) for v in tg._rand(rng, nc)] for _ in range(3))
    q = dict(gates=gates, ns=num_selectors, nls=nls, log_n=log_n, n=n, qdf=qdf, pih=pih, k_is=k_is, wires=wires, cs=cs,
             sigmas_first=num_selectors + nls + NUM_GATE_CONSTS, betas=betas, gammas=gammas, alphas=alphas, row_gate=row_gate)
    q["zs"] = np.asarray(vr.zs_partial_products_batch(wires[:NUM_ROUTED], sigmas, k_is, betas, gammas, qdf), dtype=np.uint64)
    return q


def _ref_sums(q, ldes, gates=None, alphas=None):
    """the restatement at every point of the quotient coset: [len(alphas)][n << qbits]"""
    qbits = vr.log2_ceil(q["qdf"])
    m = q["n"] << qbits
    alphas = q["alphas"] if alphas is None else alphas
    out = np.zeros((len(alphas), m), dtype=np.uint64)
    for i in range(m):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], ldes["wires"].rate_bits, qbits)
        out[:, i] = rr.reduced_sums(vr.BASE, q["gates"] if gates is None else gates, q["ns"], q["nls"], vr.get_lde_values(ldes["wires"], li, step),
                                    vr.get_lde_values(ldes["cs"], li, step), q["pih"], alphas)
    return out


# ------------------------------------------------------------------ 1. the restatement on its own
def _sensitive_wires(g):
    """wires whose change (+1) must break a constraint whatever the random row holds"""
    nw = rr.num_wires(g)
    if g.kind == rr.EXPONENTIATION:      # (the base is not read when every power bit is 0; a bit 0 -> 1 or 1 -> 2 changes the factor)
        return [1, 1 + g.param0, nw - 1]
    return [0, nw - 1]


@pytest.mark.parametrize("name", sorted(ALONE))
def test_ref_constraints_vanish_on_the_filled_witness(name):
    """every constraint is zero on the filler's row, one changed wire of the gate breaks at least one, and the counts are the
    header's table"""
    kind, p0, p1 = ALONE[name]
    g = gr.Gate(kind, 0, 0, (0, 1), p0, p1)
    assert (rr.num_wires(g), rr.num_constraints(g)) == TABLE[name]
    rng = np.random.default_rng(kind * 1000 + p0 * 10 + p1 % 7)
    for _ in range(2):
        w, c, pih = ([int(v) for v in tg._rand(rng, k)] for k in (W, NUM_GATE_CONSTS, 4))
        rr.fill_witness(rng, g, w, c, pih)
        cons = rr.eval_unfiltered(vr.BASE, g, w, c, pih)
        assert len(cons) == rr.num_constraints(g) and not any(cons)
        assert max(rr.determined_wires(g)) < rr.num_wires(g)
        for j in _sensitive_wires(g):
            bad = list(w)
            bad[j] = (bad[j] + 1) % P
            assert any(rr.eval_unfiltered(vr.BASE, g, bad, c, pih)), j
        # a wire past the gate's is not read
        if rr.num_wires(g) < W:
            more = list(w)
            more[rr.num_wires(g)] = (more[rr.num_wires(g)] + 1) % P
            assert not any(rr.eval_unfiltered(vr.BASE, g, more, c, pih))


def test_ref_coset_interpolation_witness_interpolates():
    """the filled evaluation value is the interpolant of the values on shift * H at the evaluation point, by Lagrange's formula"""
    g = gr.Gate(rr.COSET_INTERPOLATION, 0, 0, (0, 1), 3, 4)
    rng = np.random.default_rng(3)
    w = [int(v) for v in tg._rand(rng, W)]
    rr.fill_witness(rng, g, w, [], [0] * 4)
    F, n = vr.EXT, 8
    xs = [(x * w[0] % P, 0) for x in rr.two_adic_subgroup(3)]
    z = (w[1 + 2 * n], w[2 + 2 * n])
    acc = F.zero
    for k in range(n):
        term = (w[1 + 2 * k], w[2 + 2 * k])
        for j in range(n):
            if j != k:
                term = F.mul(term, F.mul(F.sub(z, xs[j]), F.inv(F.sub(xs[k], xs[j]))))
        acc = F.add(acc, term)
    assert acc == (w[1 + 2 * n + 2], w[1 + 2 * n + 3])


def test_ref_random_access_and_exponentiation_witnesses():
    rng = np.random.default_rng(4)
    g = gr.Gate(rr.RANDOM_ACCESS, 0, 0, (0, 1), 2, rr.ra_param1(3, 1))
    w = [int(v) for v in tg._rand(rng, W)]
    rr.fill_witness(rng, g, w, [77, 0], [0] * 4)
    for copy in range(2):
        assert w[10 * copy] < 8 and w[10 * copy + 1] == w[10 * copy + 2 + w[10 * copy]]
    assert w[20] == 77
    g = gr.Gate(rr.EXPONENTIATION, 0, 0, (0, 1), 9)
    rr.fill_witness(rng, g, w, [], [0] * 4)
    assert w[10] == pow(w[0], sum(b << k for k, b in enumerate(w[1:10])), P)


# ------------------------------------------------------------------ 2. p2hot_gate_sums, one gate
@pytest.mark.parametrize("name", sorted(ALONE))
def test_gate_sums_of_one_gate(eng, name):
    """one kind, one selector polynomial, random wires, every coset point, 1 to 4 challenges"""
    kind, p0, p1 = ALONE[name]
    gates = tg._alone(kind, p0, p1, row=1, group=(0, 3))        # (two more gates in the group: the filter has two factors)
    q = _instance(kind * 1000 + p0 * 10 + p1 % 7, gates, 1, 4, nc=4)
    exp = _ref_sums(q, tg._ldes(q))
    assert exp.shape == (4, 16 << 3) and exp.all()
    b = tg._commit(eng, q)
    for nc in (1, 2, 3, 4):
        got = tg._device_sums(eng, q, b, nc)
        assert got.shape == (nc, 128) and (got < P).all()
        assert (got == exp[:nc]).all(), nc


# ------------------------------------------------------------------ 3. the recursion set
_FULL = {}


def _full(satisfied, qdf=QDF, log_n=6):
    key = (satisfied, qdf, log_n)
    if key not in _FULL:
        gates, ns = _recursion_set(qdf)
        q = _instance(17 + satisfied, gates, ns, log_n, satisfied=satisfied, qdf=qdf, nc=2 if satisfied else 4)
        ldes = tg._ldes(q)
        _FULL[key] = (q, ldes, _ref_sums(q, ldes))
    return _FULL[key]


@pytest.mark.parametrize("nc", [1, 2, 3, 4])
def test_gate_sums_of_the_recursion_set(eng, nc):
    """all fourteen kinds in four selector groups, 512 points (two workgroups)"""
    q, _, exp = _full(False)
    assert q["ns"] == 4 and (q["cs"][:q["ns"]] == gr.UNUSED_SELECTOR).any()
    got = tg._device_sums(eng, q, tg._commit(eng, q), nc)
    assert (got == exp[:nc]).all() and exp.all()


def test_recursion_set_split_between_device_and_host_residual(eng):
    """the quotient values with all fourteen on the device, with only the six new kinds described and the old eight as the host
    residual, and the other way round: the residual is still added"""
    from plonky2_amd.plonk.prover import compute_quotient_polys
    nc = 2
    q, ldes, exp = _full(False)
    q = dict(q, zs=tg._rand(np.random.default_rng(5), nc * (1 + vr.num_partial_products(NUM_ROUTED, QDF)), q["n"]))
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    _, vals = compute_quotient_polys(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], QDF, q["betas"][:nc], q["gammas"][:nc],
                                     q["alphas"][:nc], gate_sums=exp[:nc], want_values=True, engine=eng)
    new = [g for g in q["gates"] if g.kind in rr.NEW_KINDS]
    old = [g for g in q["gates"] if g.kind not in rr.NEW_KINDS]
    assert len(new) == 6 and len(old) == 8 and vals.any()
    _, got = tg._quotients(eng, q, b, nc, None, None)
    assert (got == vals).all()
    for device, host in ((new, old), (old, new)):
        rest = _ref_sums(q, ldes, gates=host, alphas=q["alphas"][:nc])
        _, got = tg._quotients(eng, q, b, nc, device, rest)
        assert (got == vals).all()
        _, alone = tg._quotients(eng, q, b, nc, device, None)
        assert (alone != vals).any()


def _many_new(count):
    """`count` descriptors of the descriptor-loop kinds with small parameters, a PoseidonMds, a Poseidon and cheap kinds among them
    (so the new-kind count runs behind the descriptor index), rows = indices, selector groups of eight"""
    cycle = [(rr.REDUCING, 2, 0), (rr.EXPONENTIATION, 3, 0), (rr.RANDOM_ACCESS, 2, rr.ra_param1(2, 1)), (rr.COSET_INTERPOLATION, 2, 3),
             (rr.REDUCING_EXT, 3, 0), (rr.RANDOM_ACCESS, 1, rr.ra_param1(3, 0)), (rr.COSET_INTERPOLATION, 3, 4), (rr.EXPONENTIATION, 1, 0),
             (rr.REDUCING, 5, 0), (rr.COSET_INTERPOLATION, 1, 2), (rr.REDUCING_EXT, 1, 0)]
    kinds = [cycle[k % len(cycle)] for k in range(count)]
    for at, kind in ((2, (rr.POSEIDON_MDS, 0, 0)), (9, (gr.ARITHMETIC, 3, 0)), (20, (gr.POSEIDON, 0, 0)), (30, (gr.NOOP, 0, 0))):
        kinds.insert(at, kind)
    gates = [gr.Gate(kind, row, row // 8, (row // 8 * 8, min(row // 8 * 8 + 8, len(kinds))), p0, p1) for row, (kind, p0, p1) in enumerate(kinds)]
    return gates, -(-len(kinds) // 8)


@pytest.mark.parametrize("count", [32, 33, 65])
def test_gate_sums_split_over_several_launches(eng, count):
    """gates::MAX_CHEAP = 32 descriptors per launch of the descriptor loop: one full launch, a second of one descriptor, a third.  A
    descriptor launched twice or not at all changes every point"""
    gates, ns = _many_new(count)
    assert sum(g.kind in rr.NEW_KINDS and g.kind != rr.POSEIDON_MDS for g in gates) == count
    q = _instance(700 + count, gates, ns, 3, nc=2)
    exp = _ref_sums(q, tg._ldes(q))
    got = tg._device_sums(eng, q, tg._commit(eng, q), 2)
    assert got.shape == exp.shape == (2, 64)
    assert (got == exp).all() and exp.all()


# ------------------------------------------------------------------ 4. a satisfied instance: the quotient and the verifier's identity
def _ref_chunks(q, nc):
    """compute_quotient_polys (prover.rs:609-815) by the restatements alone: the vanishing polynomial with the gate constraints at
    every point of the quotient coset over Z_H, then coset_ifft, trim, chunks"""
    ldes = tg._ldes(q, ("wires", "cs", "zs"))
    qdf, log_n, sf = q["qdf"], q["log_n"], q["sigmas_first"]
    qbits = vr.log2_ceil(qdf)
    num_prods = vr.num_partial_products(NUM_ROUTED, qdf)
    vals = []
    for i in range(q["n"] << qbits):
        (li, step), (nxt, _) = vr.quotient_rows(i, log_n, RATE_BITS, qbits)
        x = vr.quotient_point(i, log_n, qbits)
        lw, lcs, lz, nz = (vr.get_lde_values(ldes[name], at, step) for name, at in (("wires", li), ("cs", li), ("zs", li), ("zs", nxt)))
        cons = rr.evaluate_gate_constraints(vr.BASE, q["gates"], q["ns"], q["nls"], lw, lcs, q["pih"])
        v = vr.eval_vanishing_poly(vr.BASE, q["n"], x, lw, lz[:nc], nz[:nc], lz[nc:nc + nc * num_prods], lcs[sf:sf + NUM_ROUTED], q["k_is"],
                                   q["betas"][:nc], q["gammas"][:nc], q["alphas"][:nc], qdf, cons)
        zh_inv = vr.BASE.inv(vr.eval_zero_poly(vr.BASE, q["n"], x))
        vals.append([a * zh_inv % P for a in v])
    return np.asarray(vr.quotient_chunks([[c[a] for c in vals] for a in range(nc)], log_n, qdf), dtype=np.uint64)


def _identity_holds(eng, q, b, chunks, nc, seed):
    """tests/test_gates.py's _identity_holds with the gate constraints of all fourteen kinds over the extension"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    b_q = PolynomialBatch.from_coeffs(chunks, RATE_BITS, False, 0, engine=eng)
    rng = np.random.default_rng(seed)
    zeta = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(q["log_n"]))
    cs_z, w_z, zs_z, q_z = [tg._pairs(e[0]) for e in eval_openings([b["cs"], b["wires"], b["zs"], b_q], [zeta], eng)]
    zs_gz = tg._pairs(eval_openings([b["zs"]], [gz], eng)[0][0])
    cons = rr.evaluate_gate_constraints(vr.EXT, q["gates"], q["ns"], q["nls"], w_z, cs_z, q["pih"])
    sf = q["sigmas_first"]
    van = vr.eval_vanishing_poly(vr.EXT, q["n"], zeta, w_z, zs_z[:nc], zs_gz[:nc], zs_z[nc:], cs_z[sf:sf + NUM_ROUTED], q["k_is"], q["betas"][:nc],
                                 q["gammas"][:nc], q["alphas"][:nc], q["qdf"], cons)
    return vr.verifier_check(vr.EXT, zeta, q["n"], van, q_z, q["qdf"])


def _break(q, what):
    """one non-routed wire of one row (the permutation argument stays satisfied): bit 1 of copy 2 of a RandomAccess row, or word 1 of
    the second intermediate product of a CosetInterpolation row"""
    q = dict(q)
    wires = q["wires"].copy()
    if what == "random_access_bit":
        row, wire = q["row_gate"].index(ROW_RANDOM_ACCESS), 18 * 4 + 2 + 2 * 4 + 1
    else:
        row, wire = q["row_gate"].index(ROW_COSET), 1 + 32 + 4 + 2 * 2 + 2 + 1
    assert wire >= NUM_ROUTED if what == "random_access_bit" else wire in rr.determined_wires(q["gates"][ROW_COSET])
    wires[wire][row] = (int(wires[wire][row]) + 1) % P
    q["wires"] = wires
    return q


@pytest.mark.parametrize("log_n", [4, 6])
def test_quotient_of_a_satisfied_recursion_circuit(eng, log_n):
    """every row satisfies its gate, the routed wires a real permutation, NULL host residual: the chunks are the restatement's byte
    for byte and pass the verifier's identity at an extension point"""
    nc = 2
    q, _, _ = _full(True, log_n=log_n)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = tg._quotients(eng, q, b, nc, None, None)
    exp = _ref_chunks(q, nc)
    assert chunks.shape == exp.shape == (nc * QDF, q["n"]) and exp.any()
    assert (chunks == exp).all()
    assert _identity_holds(eng, q, b, chunks, nc, 1) == [True] * nc


@pytest.mark.parametrize("what", ["random_access_bit", "coset_intermediate"])
def test_broken_wire_fails_the_identity_and_the_quotient(eng, what):
    """factor 8 keeps every coefficient, so the verifier's identity is what fails; at factor 7 (the thirteen gates without Poseidon,
    7 n of 8 n coefficients kept) the trim sees a quotient that is no polynomial and the call returns the error"""
    nc = 2
    q, _, _ = _full(True, log_n=4)
    bad = _break(q, what)
    b = tg._commit(eng, q, ("cs", "zs"))
    b["wires"] = tg._commit(eng, bad, ("wires",))["wires"]
    chunks, _ = tg._quotients(eng, bad, b, nc, None, None)
    assert _identity_holds(eng, bad, b, chunks, nc, 1) == [False] * nc
    q, _, _ = _full(True, qdf=7, log_n=4)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = tg._quotients(eng, q, b, nc, None, None)
    assert chunks.shape == (nc * 7, 16) and _identity_holds(eng, q, b, chunks, nc, 2) == [True] * nc
    bad = _break(q, what)
    b["wires"] = tg._commit(eng, bad, ("wires",))["wires"]
    with pytest.raises(ValueError, match="Quotient has failed"):
        tg._quotients(eng, bad, b, nc, None, None)
    h = C.c_void_p(1)
    vals = np.zeros((nc, 16 << 3), dtype=np.uint64)
    rc = eng.lib.p2hot_quotient_polys_gates(eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b["zs"]._h, tg._u64(q["k_is"]), NUM_ROUTED, 7,
                                            tg._u64(q["betas"]), tg._u64(q["gammas"]), tg._u64(q["alphas"]), nc, None, tg._gate_set(q).ptr,
                                            vals.ctypes.data_as(C.c_void_p), C.byref(h))
    assert rc == 1 and not h.value and b"Quotient has failed" in eng.lib.p2hot_last_error(eng.ctx)
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


# ------------------------------------------------------------------ 5. the lookup variant
def test_lookup_quotient_with_recursion_gates(eng):
    """p2hot_quotient_polys_lookup_gates on the (unsatisfied: values only) lookup instance of tests/test_gates.py's lookup case --
    15 wires, two selector polynomials, no gate constants -- with PublicInput, Reducing(3), CosetInterpolation(1, 2) in one group
    and RandomAccess(1 copy, 2 bits) in the other, as factor 4 groups them: against p2hot_quotient_polys_lookup (tests/test_lookup.py
    pins it to tests/lookup_ref.py) fed the restated sums"""
    from tests import test_lookup as tl
    nc, num_routed, qdf = 2, 12, 4
    q = tl._instance(np.random.default_rng(23), nc, qdf, num_routed, 3, 4, satisfied=False)
    nls = 4 + len(q["luts"])
    assert q["sigmas_first"] == tl.SEL_FIRST + nls
    gates, ns = _set([(gr.PUBLIC_INPUT, 0, 0), (rr.REDUCING, 3, 0), (rr.COSET_INTERPOLATION, 1, 2), (rr.RANDOM_ACCESS, 1, rr.ra_param1(2, 0))], qdf)
    assert ns == 2 and max(rr.num_wires(g) for g in gates) <= 15
    gq = dict(gates=gates, ns=2, nls=nls, log_n=4, n=16, qdf=qdf, pih=[5, 6, 7, 8], alphas=q["alphas"])
    ldes = {name: vr.Lde(vr.interpolate_columns(q[name]), 4, 3) for name in ("wires", "cs")}
    exp = _ref_sums(gq, ldes)
    b = tl._commit(eng, q)
    vals, got, got2 = (np.zeros((nc, 16 << 2), dtype=np.uint64) for _ in range(3))
    common = (eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b["zs"]._h, tg._u64(q["k_is"]), num_routed, qdf, tg._u64(q["betas"]),
              tg._u64(q["gammas"]), tg._u64(q["alphas"]), nc)
    lk = (q["lu_slots"], q["lut_slots"], len(q["luts"]), tl.SEL_FIRST, tg._u64(q["deltas"]), tg._u64(q["evals"]))
    assert eng.lib.p2hot_quotient_polys_lookup(*common, tl._ptrs(exp), *lk, vals.ctypes.data_as(C.c_void_p), None) == 0
    assert eng.lib.p2hot_quotient_polys_lookup_gates(*common, None, *lk, tg._gate_set(gq).ptr, got.ctypes.data_as(C.c_void_p), None) == 0, \
        eng.lib.p2hot_last_error(eng.ctx)
    assert exp.all() and vals.any() and (got == vals).all()
    # the new kinds on the device, PublicInput as the host residual
    rest = _ref_sums(gq, ldes, gates=gates[:1])
    assert eng.lib.p2hot_quotient_polys_lookup_gates(*common, tl._ptrs(rest), *lk, tg._gate_set(gq, gates[1:]).ptr, got2.ctypes.data_as(C.c_void_p), None) == 0
    assert (got2 == vals).all()


# ------------------------------------------------------------------ 6. any hasher
def test_gate_sums_of_keccak_hashed_commitments(eng):
    """p2hot_gate_sums takes commitments of any hasher: KeccakHash<25> trees over the same LDE matrices, the same sums"""
    from plonky2_amd.hash.keccak import KeccakHash
    gates, ns = _recursion_set()
    q = _instance(31, gates, ns, 4, nc=2)
    exp = _ref_sums(q, tg._ldes(q))
    keccak = tg._commit(eng, q, hasher=KeccakHash(25))
    assert (keccak["wires"].merkle_tree.cap.entries != tg._commit(eng, q, ("wires",))["wires"].merkle_tree.cap.entries).any()
    assert (tg._device_sums(eng, q, keccak, 2) == exp).all() and exp.all()


# ------------------------------------------------------------------ 7. errors
def test_errors_come_before_any_work(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.plonk.prover import GateSet
    q, _, _ = _full(True, qdf=7, log_n=4)
    b = tg._commit(eng, q, ("wires", "cs"))
    # (wide enough for the permutation argument at every factor from 2 up: nc (1 + 39) polynomials)
    b["zs"] = PolynomialBatch.from_values(tg._rand(np.random.default_rng(8), 80, 16), RATE_BITS, False, 0, engine=eng)
    nc, sf = 2, q["sigmas_first"]
    assert sf == 4 + NUM_GATE_CONSTS
    out = np.zeros((nc, 16 << 3), dtype=np.uint64)

    def sums(gs, qdf=8, wires=None):
        return eng.lib.p2hot_gate_sums(eng.ctx, (wires or b["wires"])._h, b["cs"]._h, sf, gs.ptr, qdf, tg._u64(q["alphas"]), nc, out.ctypes.data_as(C.c_void_p))

    def quot(gs, qdf=8, wires=None):
        h = C.c_void_p(1)
        rc = eng.lib.p2hot_quotient_polys_gates(eng.ctx, (wires or b["wires"])._h, b["cs"]._h, sf, b["zs"]._h, tg._u64(q["k_is"]), NUM_ROUTED, qdf,
                                                tg._u64(q["betas"]), tg._u64(q["gammas"]), tg._u64(q["alphas"]), nc, None, gs.ptr, None, C.byref(h))
        assert rc == _lib.OK or not h.value          # chunks_out is null after every failure
        if rc == _lib.OK:
            eng.lib.p2hot_cols_free(h)
        return rc

    def one(kind, p0=0, p1=0, ns=4):
        return GateSet([(kind, 0, 0, 0, 1, p0, p1)], ns, 0)

    def refused(gs, code, qdf=8, words=(), wires=None):
        for call in (sums, quot):
            out[:] = 0
            assert call(gs, qdf=qdf, wires=wires) == code, (gs.gates, qdf)
            msg = eng.lib.p2hot_last_error(eng.ctx)
            assert msg and all(word in msg for word in words), msg
            assert not out.any()

    def accepted(gs, qdf=8):
        assert sums(gs, qdf=qdf) == _lib.OK, (gs.gates, qdf, eng.lib.p2hot_last_error(eng.ctx))
        # (below factor 8 the trim of this unsatisfied instance fails AFTER the work; the descriptor itself is taken)
        assert quot(gs, qdf=qdf) == _lib.OK or (qdf < 8 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng.ctx))

    ra = rr.ra_param1
    for kind in (8, 15, 22):
        refused(one(kind), _lib.EUNSUPPORTED, words=(b"unknown kind %d" % kind,))
    # a parameter of 0
    for kind, p1 in ((rr.REDUCING, 0), (rr.REDUCING_EXT, 0), (rr.EXPONENTIATION, 0), (rr.RANDOM_ACCESS, ra(1, 0))):
        refused(one(kind, 0, p1), _lib.EINVAL)
        accepted(one(kind, 1, p1))
    # RandomAccess bits 1..6 (bits 6 has degree 7: a factor of at least 7)
    refused(one(rr.RANDOM_ACCESS, 1, ra(0, 0)), _lib.EINVAL, words=(b"RandomAccess",))
    refused(one(rr.RANDOM_ACCESS, 1, ra(7, 0)), _lib.EINVAL, words=(b"RandomAccess",))
    accepted(one(rr.RANDOM_ACCESS, 1, ra(6, 0)))
    accepted(one(rr.RANDOM_ACCESS, 1, ra(6, 0)), qdf=7)
    refused(one(rr.RANDOM_ACCESS, 1, ra(6, 0)), _lib.EINVAL, qdf=6, words=(b"RandomAccess", b"factor 6"))
    # CosetInterpolation subgroup_bits 1..5, 2 <= d <= N, d <= factor
    refused(one(rr.COSET_INTERPOLATION, 0, 2), _lib.EINVAL, words=(b"CosetInterpolation",))
    refused(one(rr.COSET_INTERPOLATION, 6, 8), _lib.EINVAL, words=(b"CosetInterpolation",))
    accepted(one(rr.COSET_INTERPOLATION, 5, 8))
    refused(one(rr.COSET_INTERPOLATION, 2, 1), _lib.EINVAL, words=(b"CosetInterpolation",))
    refused(one(rr.COSET_INTERPOLATION, 2, 5), _lib.EINVAL, words=(b"CosetInterpolation",))      # d = N + 1
    accepted(one(rr.COSET_INTERPOLATION, 2, 4))                                                  # d = N
    refused(one(rr.COSET_INTERPOLATION, 1, 3), _lib.EINVAL, words=(b"CosetInterpolation",))
    accepted(one(rr.COSET_INTERPOLATION, 1, 2))
    accepted(one(rr.COSET_INTERPOLATION, 3, 8))
    refused(one(rr.COSET_INTERPOLATION, 3, 8), _lib.EINVAL, qdf=7, words=(b"CosetInterpolation", b"factor 7"))
    refused(one(rr.COSET_INTERPOLATION, 4, 9), _lib.EINVAL, words=(b"CosetInterpolation", b"factor 8"))
    # Exponentiation has degree 4
    accepted(one(rr.EXPONENTIATION, 3), qdf=4)
    refused(one(rr.EXPONENTIATION, 3), _lib.EINVAL, qdf=3, words=(b"Exponentiation", b"factor 3"))
    # Reducing / ReducingExtension have degree 2: the smallest factor the entry points take
    accepted(one(rr.REDUCING, 2), qdf=2)
    accepted(one(rr.REDUCING_EXT, 2), qdf=2)
    # wires beyond the commitment
    refused(one(rr.REDUCING, 44), _lib.EINVAL, words=(b"136 wires",))
    accepted(one(rr.REDUCING, 43))
    refused(one(rr.REDUCING_EXT, 33), _lib.EINVAL, words=(b"136 wires",))
    refused(one(rr.EXPONENTIATION, 67), _lib.EINVAL, words=(b"136 wires",))
    refused(one(rr.RANDOM_ACCESS, 2, ra(6, 0)), _lib.EINVAL, words=(b"144 wires",))
    narrow = PolynomialBatch.from_values(q["wires"][:86], RATE_BITS, False, 0, engine=eng)
    refused(one(rr.COSET_INTERPOLATION, 5, 8), _lib.EINVAL, words=(b"87 wires",), wires=narrow)
    narrow = PolynomialBatch.from_values(q["wires"][:47], RATE_BITS, False, 0, engine=eng)
    assert sums(one(rr.POSEIDON_MDS), wires=narrow) == _lib.EINVAL and sums(one(rr.POSEIDON_MDS)) == _lib.OK
    # RandomAccess' extra constants past sigmas_first_col = 4 selectors + 2 constants
    refused(one(rr.RANDOM_ACCESS, 1, ra(2, 3)), _lib.EINVAL, words=(b"sigmas_first_col",))
    accepted(one(rr.RANDOM_ACCESS, 1, ra(2, 2)))
    refused(one(rr.RANDOM_ACCESS, 1, ra(2, 2), ns=5), _lib.EINVAL, words=(b"sigmas_first_col",))
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0
    good = tg._gate_set(q)
    b["zs"] = tg._commit(eng, q, ("zs",))["zs"]
    assert sums(good, qdf=7) == _lib.OK and quot(good, qdf=7) == _lib.OK and out.any()


# ------------------------------------------------------------------ 8. code objects, the Rust constants
NEW_NAMES = ("POSEIDON_MDS", "REDUCING", "REDUCING_EXT", "RANDOM_ACCESS", "EXPONENTIATION", "COSET_INTERPOLATION")


def test_new_gate_kernels_use_no_scratch_and_spill_nothing():
    so = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")
    if not os.path.exists(so):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    md = codeobj.kernel_metadata(so)
    for kernel in ("recursion_gates_kernel", "mds_gate_kernel"):
        names = [n for n in md if "5gates" in n and kernel in n]
        assert len(names) == 4, (kernel, names)
        for n in names:
            assert "cheap_gates_kernel" not in n and "poseidon_gate_kernel" not in n
            k = md[n]
            assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
            assert k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, n


def test_recursion_kinds_are_numbered_alike_everywhere():
    """the header's second enum starts at 16; integration/p2hot.rs, the Python mirror and the restatement carry the same values"""
    from plonky2_amd.plonk import prover
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2hot.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "p2hot.rs")).read()
    enums = re.findall(r"enum \{(.*?)\}", h, flags=re.S)
    assert len(enums) >= 2
    items = [x.strip() for x in enums[1].split(",")]
    assert items[0].replace(" ", "") == "P2HOT_GATE_POSEIDON_MDS=16"
    assert [items[0].split("=")[0].strip()] + items[1:] == ["P2HOT_GATE_" + n for n in NEW_NAMES]
    for k, name in enumerate(NEW_NAMES, 16):
        assert re.search(r"pub const P2HOT_GATE_%s: u32 = %d;" % (name, k), rs), name
        assert getattr(prover, "GATE_" + name) == k == getattr(rr, name)
