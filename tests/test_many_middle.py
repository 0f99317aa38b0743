"""The middle of a proof for M witnesses of ONE circuit (include/p2hot.h, the *_many section): p2hot_partial_products_many,
p2hot_commit_cols_many, p2hot_quotient_polys_gates_many, p2hot_eval_openings_many.

The yardstick is the single-proof path, which tests/test_vanishing_identity.py, test_gates.py and test_recursion_gates.py pin to the
restatements (vanishing_ref.py, gates_ref.py, recursion_gates_ref.py): every result of an M-form must equal M single-proof calls word
for word.  Sizes: 2^5 rows (one scan chunk per proof) and 2^7 (two), rate 3, cap 2; nc 2 with degree 8 (the pipelined quotient
instantiation) and nc 3 with degree 4 (the generic one); the recursion gate set needs factor 8 (and 7 for a quotient whose trim
can fail), so the gate cases run nc 2 and nc 3 at those.  nc 1 and nc 4 at 2^5 rows and M = 2 run the remaining instantiations of
the quotient and gate M-forms and the partial products' pairing rule with a lone challenge and with two pairs."""
import ctypes as C

import numpy as np
import pytest

from tests import recursion_gates_ref as rr
from tests import test_gates as tg
from tests import test_recursion_gates as trg
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import G

W, NUM_ROUTED, RATE_BITS, CAP = tg.W, tg.NUM_ROUTED, tg.RATE_BITS, 2


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _handles(batches):
    return (C.c_void_p * max(len(batches), 1))(*[b._h if b is not None else None for b in batches])


def _err(eng):
    return eng.lib.p2hot_last_error(eng.ctx).decode()


def _commit_wires(eng, wires, shared, rate_bits=RATE_BITS):
    """the M wires commitments: shares of ONE p2hot_commit_many block (interleaved columns, strides M * n), or separately committed
    batches (plain strides)"""
    from plonky2_amd.fri.oracle import PolynomialBatch
    if shared:
        return PolynomialBatch.from_values_many(wires, rate_bits, CAP, engine=eng)
    return [PolynomialBatch.from_values(w, rate_bits, False, CAP, engine=eng) for w in wires]


# ------------------------------------------------------------------ 1. partial products and Zs
PP_CASES = [(5, 2, 8, 1, True), (5, 2, 8, 2, False), (5, 2, 8, 8, True), (5, 3, 4, 1, False), (5, 3, 4, 2, True), (5, 3, 4, 8, False),
            (7, 2, 8, 2, True), (7, 2, 8, 8, False), (7, 3, 4, 2, False), (7, 3, 4, 8, True), (5, 1, 4, 2, True), (5, 4, 4, 2, False)]


@pytest.mark.parametrize("log_n,nc,degree,M,shared", PP_CASES)
def test_partial_products_many_equals_single_calls(eng, log_n, nc, degree, M, shared):
    """different wires and different (beta, gamma) per proof, one sigma set: out_host and the downloaded interleaved out_cols
    equal M p2hot_partial_products calls word for word, for handles that share one block and for separately committed ones"""
    from plonky2_amd.fri.oracle import DeviceColumns
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products, all_wires_permutation_partial_products_many
    rng = np.random.default_rng(1000 * log_n + 100 * nc + 10 * M + shared)
    n, R = 1 << log_n, 21  # 21 routed wires: a ragged last chunk at degree 8 and at degree 4
    wires = tg._rand(rng, M, R + 2, n)
    sigmas = DeviceColumns.upload(tg._rand(rng, R, n), eng)
    k_is = [pow(G, j, P) for j in range(R)]
    betas, gammas = tg._rand(rng, M, nc), tg._rand(rng, M, nc)
    bw = _commit_wires(eng, wires, shared)
    cols, host = all_wires_permutation_partial_products_many(bw, sigmas, k_is, degree, betas, gammas, want_host=True, engine=eng)
    rows = nc * (-(-R // degree))
    assert host.shape == (M, rows, n) and cols.width == rows * M
    inter = cols.host().reshape(rows, M, n)
    for m in range(M):
        one = all_wires_permutation_partial_products(DeviceColumns.upload(wires[m][:R], eng), sigmas, k_is, degree, betas[m], gammas[m], eng).host()
        assert one.any() and (host[m] == one).all(), m
        assert (inter[:, m] == one).all(), m


def test_partial_products_many_names_the_proof_with_a_zero_denominator(eng):
    """wire + beta * sigma + gamma = 0 at one row of proof 2 only"""
    from plonky2_amd.fri.oracle import DeviceColumns
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products_many
    rng = np.random.default_rng(5)
    n, R, M, nc = 32, 9, 4, 2
    wires, sig = tg._rand(rng, M, R, n), tg._rand(rng, R, n)
    betas, gammas = tg._rand(rng, M, nc), tg._rand(rng, M, nc)
    wires[2][4][7] = (P - (int(betas[2][1]) * int(sig[4][7]) + int(gammas[2][1])) % P) % P
    with pytest.raises(ValueError, match="proof 2: tried to invert zero"):
        all_wires_permutation_partial_products_many(_commit_wires(eng, wires, True), DeviceColumns.upload(sig, eng), [pow(G, j, P) for j in range(R)],
                                                    4, betas, gammas, engine=eng)


# ------------------------------------------------------------------ 2. the commitment of an interleaved column set
@pytest.mark.parametrize("is_values", [1, 0])
def test_commit_cols_many_equals_commit_cols_per_proof(eng, is_values):
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    from plonky2_amd.plonk.prover import commit_columns_many
    rng = np.random.default_rng(20 + is_values)
    M, Wd, log_n = 4, 5, 5
    N = 1 << (log_n + RATE_BITS)
    inter = tg._rand(rng, Wd * M, 1 << log_n)  # column e of proof m is column e * M + m
    dc = DeviceColumns.upload(inter, eng)
    many = commit_columns_many(dc, M, RATE_BITS, CAP, is_values, engine=eng)
    assert dc._h is None and len(many) == M  # the set is consumed
    for m, b in enumerate(many):
        one = PolynomialBatch._build(DeviceColumns.upload(inter[m::M], eng), RATE_BITS, False, CAP, bool(is_values), eng, False)
        assert (b.merkle_tree.cap.entries == one.merkle_tree.cap.entries).all(), m
        assert (b.merkle_tree.digests == one.merkle_tree.digests).all(), m
        assert (b.polynomials == one.polynomials).all(), m
        assert (b._owner.rows(np.arange(N)) == one._owner.rows(np.arange(N))).all(), m


def test_commit_cols_many_leaves_the_set_with_the_caller_after_einval(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    rng = np.random.default_rng(23)
    vals = tg._rand(rng, 12, 32)
    dc = DeviceColumns.upload(vals, eng)
    hs = (C.c_void_p * 8)()  # (the call clears M entries first)
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, dc._h, 3, RATE_BITS, CAP, 1, None, hs) == _lib.EINVAL
    assert "the number of proofs (3) must be a power of two" in _err(eng)
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, None, 4, RATE_BITS, CAP, 1, None, hs) == _lib.EINVAL and "null column set" in _err(eng)
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, dc._h, 8, RATE_BITS, CAP, 1, None, hs) == _lib.EINVAL and "not an interleaved set" in _err(eng)
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, dc._h, 4, RATE_BITS, 99, 1, None, hs) == _lib.EINVAL and "cap_height" in _err(eng)
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, dc._h, 0, RATE_BITS, CAP, 1, None, hs) == _lib.OK  # nothing done
    kept = PolynomialBatch.from_values(vals, RATE_BITS, False, CAP, engine=eng, keep_values=True)
    view = kept.values()
    assert eng.lib.p2hot_commit_cols_many(eng.ctx, view._h, 4, RATE_BITS, CAP, 1, None, hs) == _lib.EINVAL and "borrowed view" in _err(eng)
    assert not any(hs) and (dc.host() == vals).all() and (view.host() == vals).all()  # both still belong to the caller


# ------------------------------------------------------------------ M witnesses of one recursion circuit
def _circuit(seed, log_n, qdf):
    """one circuit: the recursion gate set, its selectors and constants, copy cycles between free routed positions and their sigmas"""
    gates, ns = trg._recursion_set(qdf)
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    row_gate = [i % len(gates) for i in range(n)]
    sel = tg._selectors(gates, ns, row_gate)
    consts = tg._rand(rng, tg.NUM_GATE_CONSTS, n)
    k_is = [pow(G, j, P) for j in range(NUM_ROUTED)]
    sub = vr.subgroup(log_n)
    perm = np.arange(NUM_ROUTED * n)
    free = [(j, i) for i in range(n) for j in range(NUM_ROUTED) if j not in set(rr.determined_wires(gates[row_gate[i]]))]
    picks = [free[t] for t in rng.choice(len(free), size=min(60, len(free) // 3 * 3), replace=False)]
    cycles = [picks[c:c + 3] for c in range(0, len(picks), 3)]
    for cyc in cycles:
        for t, (j, i) in enumerate(cyc):
            nj, ni = cyc[(t + 1) % 3]
            perm[j * n + i] = nj * n + ni
    sigmas = np.asarray([[k_is[p // n] * sub[p % n] % P for p in perm[j * n:(j + 1) * n]] for j in range(NUM_ROUTED)], dtype=np.uint64)
    return dict(gates=gates, ns=ns, nls=0, log_n=log_n, n=n, qdf=qdf, k_is=k_is, cs=np.concatenate([sel, consts, sigmas]), consts=consts,
                sigmas=sigmas, sigmas_first=ns + tg.NUM_GATE_CONSTS, row_gate=row_gate, cycles=cycles)


def _witness(circ, seed):
    """a satisfied witness of the circuit with its own public-inputs hash: (wires [135][n], pih)"""
    rng = np.random.default_rng(seed)
    n = circ["n"]
    pih = [int(v) for v in tg._rand(rng, 4)]
    w = [[int(v) for v in col] for col in tg._rand(rng, W, n)]
    for cyc in circ["cycles"]:
        for j, i in cyc:
            w[j][i] = w[cyc[0][0]][cyc[0][1]]
    for i in range(n):
        row = [w[j][i] for j in range(W)]
        rr.fill_witness(rng, circ["gates"][circ["row_gate"][i]], row, [int(circ["consts"][0][i]), int(circ["consts"][1][i])], pih)
        for j in range(W):
            w[j][i] = row[j]
    return np.asarray(w, dtype=np.uint64), pih


_PROOFS = {}


def _proofs(log_n, qdf, M):
    """the circuit and M witnesses, computed once per shape and left unchanged"""
    key = (log_n, qdf, M)
    if key not in _PROOFS:
        circ = _circuit(7 * log_n + qdf, log_n, qdf)
        ws = [_witness(circ, 100 * log_n + 10 * qdf + m) for m in range(M)]
        _PROOFS[key] = (circ, np.stack([w for w, _ in ws]), _u64([p for _, p in ws]))
    return _PROOFS[key]


def _challenges(seed, M, nc):
    rng = np.random.default_rng(seed)
    return tg._rand(rng, M, nc), tg._rand(rng, M, nc), tg._rand(rng, M, nc)


def _setup(eng, log_n, qdf, M, nc, seed, shared=True):
    """(circuit, wires, hashes, challenges, the wires / constants_sigmas / Zs commitments) with the Zs from the single-proof calls"""
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products
    circ, wires, pihs = _proofs(log_n, qdf, M)
    betas, gammas, alphas = _challenges(seed, M, nc)
    bw = _commit_wires(eng, wires, shared)
    bcs = PolynomialBatch.from_values(circ["cs"], RATE_BITS, False, CAP, engine=eng)
    ds = DeviceColumns.upload(circ["sigmas"], eng)
    bz = [PolynomialBatch.from_values(all_wires_permutation_partial_products(DeviceColumns.upload(wires[m][:NUM_ROUTED], eng), ds, circ["k_is"], qdf,
                                                                              betas[m], gammas[m], eng), RATE_BITS, False, CAP, engine=eng) for m in range(M)]
    return circ, wires, pihs, (betas, gammas, alphas), bw, bcs, bz


def _gate_set(circ, pih):
    q = dict(circ, pih=[int(v) for v in pih])
    return tg._gate_set(q)


def _single_quotient(eng, circ, bw, bcs, bz, ch, m, pih, gates=True):
    from plonky2_amd.plonk.prover import compute_quotient_polys, compute_quotient_polys_gates
    betas, gammas, alphas = ch
    if not gates:
        cols, vals = compute_quotient_polys(bw, bcs, circ["sigmas_first"], bz, circ["k_is"], circ["qdf"], betas[m], gammas[m], alphas[m], None, True, eng)
    else:
        cols, vals = compute_quotient_polys_gates(bw, bcs, circ["sigmas_first"], bz, circ["k_is"], circ["qdf"], betas[m], gammas[m], alphas[m],
                                                  _gate_set(circ, pih), None, True, eng)
    return cols.host(), vals


# ------------------------------------------------------------------ 3. the quotient with the recursion gate set
@pytest.mark.parametrize("log_n,nc,M,shared", [(5, 2, 2, True), (5, 3, 2, False), (7, 2, 2, False), (5, 2, 8, True), (5, 2, 1, False),
                                                 (5, 1, 2, False), (5, 4, 2, True)])
def test_quotient_polys_gates_many_equals_single_calls(eng, log_n, nc, M, shared):
    """satisfied witnesses, per-proof challenges and public-inputs hashes: values and interleaved chunks equal M
    p2hot_quotient_polys_gates calls bit for bit; one proof's chunks pass the verifier's identity at an extension point"""
    from plonky2_amd.plonk.prover import compute_quotient_polys_gates_many
    qdf = 8
    circ, wires, pihs, ch, bw, bcs, bz = _setup(eng, log_n, qdf, M, nc, 31 * log_n + nc + M, shared)
    gs = _gate_set(circ, [0, 0, 0, 0])  # the set's own hash is replaced per proof
    cols, vals = compute_quotient_polys_gates_many(bw, bcs, circ["sigmas_first"], bz, circ["k_is"], qdf, *ch, gate_set=gs, public_inputs_hashes=pihs,
                                                   want_values=True, engine=eng)
    n = circ["n"]
    assert vals.shape == (M, nc, n << 3) and cols.width == nc * qdf * M
    inter = cols.host().reshape(nc * qdf, M, n)
    for m in range(M):
        chunks, v = _single_quotient(eng, circ, bw[m], bcs, bz[m], ch, m, pihs[m])
        assert v.any() and (vals[m] == v).all(), m
        assert (inter[:, m] == chunks).all(), m
    m = M - 1
    q = dict(circ, pih=[int(v) for v in pihs[m]], betas=[int(v) for v in ch[0][m]], gammas=[int(v) for v in ch[1][m]], alphas=[int(v) for v in ch[2][m]])
    assert trg._identity_holds(eng, q, {"cs": bcs, "wires": bw[m], "zs": bz[m]}, inter[:, m], nc, 3) == [True] * nc


@pytest.mark.parametrize("log_n,nc,qdf", [(5, 3, 4), (7, 2, 8), (5, 1, 4), (5, 4, 4)])
def test_quotient_many_without_gates_equals_quotient_polys(eng, log_n, nc, qdf):
    """gates = NULL: the permutation terms only, p2hot_quotient_polys with no gate sums (random columns: the quotient need not be a
    polynomial where the factor keeps every coefficient)"""
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.plonk.prover import compute_quotient_polys, compute_quotient_polys_gates_many
    rng = np.random.default_rng(40 + log_n)
    n, M, R = 1 << log_n, 2, 21
    num_prods = -(-R // qdf) - 1
    bw = _commit_wires(eng, tg._rand(rng, M, R + 3, n), log_n == 5)
    bcs = PolynomialBatch.from_values(tg._rand(rng, 2 + R, n), RATE_BITS, False, CAP, engine=eng)
    bz = [PolynomialBatch.from_values(tg._rand(rng, nc * (1 + num_prods), n), RATE_BITS, False, CAP, engine=eng) for _ in range(M)]
    k_is = [pow(G, j, P) for j in range(R)]
    ch = _challenges(41, M, nc)
    cols, vals = compute_quotient_polys_gates_many(bw, bcs, 2, bz, k_is, qdf, *ch, want_values=True, engine=eng)
    inter = cols.host().reshape(nc * qdf, M, n)
    for m in range(M):
        one, v = compute_quotient_polys(bw[m], bcs, 2, bz[m], k_is, qdf, ch[0][m], ch[1][m], ch[2][m], None, True, eng)
        assert v.any() and (vals[m] == v).all() and (inter[:, m] == one.host()).all(), m


# ------------------------------------------------------------------ 4. a broken wire in one proof
def test_broken_wire_names_the_proof_and_leaves_the_others_alone(eng):
    """factor 7 keeps 7 n of 8 n coefficients, so the trim sees that proof 2's quotient is no polynomial; with values_out only
    nothing is trimmed and the other proofs' values are their single calls'"""
    from plonky2_amd.plonk.prover import compute_quotient_polys_gates_many
    log_n, qdf, M, nc, j = 4, 7, 4, 2, 2
    circ, wires, pihs, ch, bw, bcs, bz = _setup(eng, log_n, qdf, M, nc, 50)
    gs = _gate_set(circ, [0, 0, 0, 0])
    args = (bcs, circ["sigmas_first"], bz, circ["k_is"], qdf) + ch
    good = compute_quotient_polys_gates_many(bw, *args, gate_set=gs, public_inputs_hashes=pihs, engine=eng)
    assert good.width == nc * qdf * M
    bad = trg._break(dict(circ, wires=wires[j]), "random_access_bit")["wires"]
    broken = list(bw)
    broken[j] = _commit_wires(eng, [bad], False)[0]
    with pytest.raises(ValueError, match=r"Quotient has failed.*\(proof 2\)"):
        compute_quotient_polys_gates_many(broken, *args, gate_set=gs, public_inputs_hashes=pihs, engine=eng)
    vals = compute_quotient_polys_gates_many(broken, *args, gate_set=gs, public_inputs_hashes=pihs, want_values=True, want_chunks=False, engine=eng)
    for m in range(M):
        if m != j:
            assert (vals[m] == _single_quotient(eng, circ, bw[m], bcs, bz[m], ch, m, pihs[m])[1]).all(), m


# ------------------------------------------------------------------ 5. the OpeningSet
@pytest.mark.parametrize("log_n,M", [(5, 3), (7, 2)])
def test_eval_openings_many_equals_single_calls(eng, log_n, M):
    """M proofs, 2 points each, the constants_sigmas handle repeated for every proof; any M is accepted"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings, eval_openings_many
    rng = np.random.default_rng(60 + log_n)
    n = 1 << log_n
    bcs = PolynomialBatch.from_values(tg._rand(rng, 7, n), RATE_BITS, False, CAP, engine=eng)
    shared = PolynomialBatch.from_values_many(tg._rand(rng, 4, 5, n), RATE_BITS, CAP, engine=eng)
    oracles = [[bcs, shared[m], PolynomialBatch.from_coeffs(tg._rand(rng, 3, n), RATE_BITS, False, CAP, engine=eng)] for m in range(M)]
    points = tg._rand(rng, M, 2, 2)
    got = eval_openings_many(oracles, points, eng)
    for m in range(M):
        exp = eval_openings(oracles[m], points[m], eng)
        assert len(got[m]) == 3 and all(e.any() and (g == e).all() for g, e in zip(got[m], exp)), m


# ------------------------------------------------------------------ 6. the chain
def test_the_whole_middle_for_four_proofs_equals_the_chain_of_single_calls(eng):
    """from_values_many (wires) -> partial_products_many -> commit_cols_many -> quotient_polys_gates_many -> commit_cols_many ->
    eval_openings_many -> p2hot_prove_openings_many: every proof's bytes equal the same chain made of single calls.  The challenges
    are fixed here, not drawn from the results under test."""
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch, eval_openings, eval_openings_many
    from plonky2_amd.iop.challenger import Challenger
    from plonky2_amd.plonk import prover as pv
    log_n, qdf, M, nc = 5, 8, 4, 2
    circ, wires, pihs = _proofs(log_n, qdf, M)
    betas, gammas, alphas = _challenges(70, M, nc)
    rng = np.random.default_rng(71)
    zetas = tg._rand(rng, M, 2)
    gen = vr.root_of_unity(log_n)
    points = _u64([[z, [int(z[0]) * gen % P, int(z[1]) * gen % P]] for z in zetas])  # zeta and g * zeta
    bcs = PolynomialBatch.from_values(circ["cs"], RATE_BITS, False, CAP, engine=eng)
    ds = bcs.subgroup_values(circ["sigmas_first"], NUM_ROUTED)
    k_is, sf = circ["k_is"], circ["sigmas_first"]
    gs0 = _gate_set(circ, [0, 0, 0, 0])
    # the M-form chain
    bw = PolynomialBatch.from_values_many(wires, RATE_BITS, CAP, engine=eng)
    bz = pv.commit_columns_many(pv.all_wires_permutation_partial_products_many(bw, ds, k_is, qdf, betas, gammas, engine=eng), M, RATE_BITS, CAP, 1, eng)
    chunks = pv.compute_quotient_polys_gates_many(bw, bcs, sf, bz, k_is, qdf, betas, gammas, alphas, gate_set=gs0, public_inputs_hashes=pihs, engine=eng)
    bq = pv.commit_columns_many(chunks, M, RATE_BITS, CAP, 0, eng)
    many = [[bcs, bw[m], bz[m], bq[m]] for m in range(M)]
    opened = eval_openings_many(many, points, eng)
    # the same chain of single calls
    single = []
    for m in range(M):
        w1 = PolynomialBatch.from_values(wires[m], RATE_BITS, False, CAP, engine=eng)
        z1 = PolynomialBatch.from_values(pv.all_wires_permutation_partial_products(DeviceColumns.upload(wires[m][:NUM_ROUTED], eng), ds, k_is, qdf, betas[m],
                                                                                    gammas[m], eng), RATE_BITS, False, CAP, engine=eng)
        q1 = PolynomialBatch.from_coeffs(pv.compute_quotient_polys_gates(w1, bcs, sf, z1, k_is, qdf, betas[m], gammas[m], alphas[m], _gate_set(circ, pihs[m]),
                                                                         engine=eng), RATE_BITS, False, CAP, engine=eng)
        single.append([bcs, w1, z1, q1])
        for a, b in zip(many[m], single[m]):
            assert (a.merkle_tree.cap.entries == b.merkle_tree.cap.entries).all() and (a.polynomials == b.polynomials).all(), m
        for g, e in zip(opened[m], eval_openings(single[m], points[m], eng)):
            assert (g == e).all(), m
    # the opening proofs of both chains: all four oracles at zeta, the Zs at g * zeta as well
    widths = [o._W for o in many[0]]
    at_zeta = [(oi, pi) for oi, w in enumerate(widths) for pi in range(w)]
    at_gz = [(2, pi) for pi in range(widths[2])]
    arity, Q = [1, 1], 3
    ab = (C.c_uint * len(arity))(*arity)
    fp = _lib.FriParams(RATE_BITS, CAP, 2, Q, ab, len(arity), 0, 0, 0)
    lay = _lib.FriProofLayout()
    assert eng.lib.p2hot_fri_proof_sizes(_handles(many[0]), 4, C.byref(fp), C.byref(lay)) == _lib.OK
    names = ("caps", "final_poly", "initial_leaves", "initial_paths", "step_evals", "step_paths")
    keep = []

    def infos_of(m):
        inf = (_lib.FriBatchInfo * 2)()
        for k, polys in enumerate((at_zeta, at_gz)):
            oi = (C.c_uint32 * len(polys))(*[o for o, _ in polys])
            pi = (C.c_uint32 * len(polys))(*[p for _, p in polys])
            keep.extend([oi, pi])
            inf[k].point[0], inf[k].point[1] = int(points[m][k][0]), int(points[m][k][1])
            inf[k].oracle_index, inf[k].poly_index, inf[k].n_polys = oi, pi, len(polys)
        return inf

    def run(oracles, together):
        chs = [Challenger(eng) for _ in range(M)]
        for m, c in enumerate(chs):
            c.observe_elements(np.arange(m, m + 5, dtype=np.uint64))
        bufs = [{k: np.zeros(max(1, getattr(lay, k + "_words")), dtype=np.uint64) for k in names} for _ in range(M)]
        qidx = [np.zeros(Q, dtype=np.uint64) for _ in range(M)]
        infos = [infos_of(m) for m in range(M)]
        proofs = (_lib.FriProof * M)()
        for m, b in enumerate(bufs):
            proofs[m] = _lib.FriProof(b["caps"].ctypes.data, b["final_poly"].ctypes.data, 0, qidx[m].ctypes.data, b["initial_leaves"].ctypes.data,
                                      b["initial_paths"].ctypes.data, b["step_evals"].ctypes.data, b["step_paths"].ctypes.data)
        if together:
            bp = (C.POINTER(_lib.FriBatchInfo) * M)(*[C.cast(inf, C.POINTER(_lib.FriBatchInfo)) for inf in infos])
            nb = (C.c_size_t * M)(*([2] * M))
            cp = (C.c_void_p * M)(*[c._h for c in chs])
            eng.check(eng.lib.p2hot_prove_openings_many(eng.ctx, M, bp, nb, _handles([o for row in oracles for o in row]), 4, cp, C.byref(fp), proofs))
        else:
            for m in range(M):
                eng.check(eng.lib.p2hot_prove_openings(eng.ctx, infos[m], 2, _handles(oracles[m]), 4, chs[m]._h, C.byref(fp), C.byref(proofs[m])))
        return [b"".join(b[k].tobytes() for k in names) + qidx[m].tobytes() + int(proofs[m].pow_witness).to_bytes(8, "little") for m, b in enumerate(bufs)]

    a, b = run(single, False), run(many, True)
    assert a == b and len(set(b)) == M


# ------------------------------------------------------------------ 7. argument errors, each before any work
def test_argument_errors_come_before_any_work(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    rng = np.random.default_rng(80)
    n, R, M, nc, qdf = 32, 9, 2, 2, 4
    num_prods = -(-R // qdf) - 1
    lib, ctx = eng.lib, eng.ctx
    bw = _commit_wires(eng, tg._rand(rng, M, R, n), False)
    ds = DeviceColumns.upload(tg._rand(rng, R, n), eng)
    bcs = PolynomialBatch.from_values(tg._rand(rng, 2 + R, n), RATE_BITS, False, CAP, engine=eng)
    bz = [PolynomialBatch.from_values(tg._rand(rng, nc * (1 + num_prods), n), RATE_BITS, False, CAP, engine=eng) for _ in range(M)]
    other_degree = PolynomialBatch.from_values(tg._rand(rng, R, 2 * n), RATE_BITS, False, CAP, engine=eng)
    other_rate = PolynomialBatch.from_values(tg._rand(rng, R, n), RATE_BITS - 1, False, CAP, engine=eng)
    k = _u64([pow(G, j, P) for j in range(R)])
    ch = [_u64(c) for c in _challenges(81, M, nc)]
    h = C.c_void_p(1)

    def pp(M_, wires, sig=ds, kk=k, be=ch[0]):
        return lib.p2hot_partial_products_many(ctx, M_, wires, 0, sig._h if sig is not None else None, 0, _ptr(kk) if kk is not None else None, R, qdf,
                                               _ptr(be) if be is not None else None, _ptr(ch[1]), nc, None, C.byref(h))

    def quot(M_, wires, zs, cs=bcs, al=ch[2], vals=None, out=h):
        return lib.p2hot_quotient_polys_gates_many(ctx, M_, wires, cs._h if cs is not None else None, 2, zs, _ptr(k), R, qdf, _ptr(ch[0]), _ptr(ch[1]),
                                                   _ptr(al) if al is not None else None, nc, None, None, vals, C.byref(out) if out is not None else None)

    # M = 0: P2HOT_OK, nothing done, whatever else is passed
    assert pp(0, None, None, None, None) == _lib.OK and not h.value
    assert quot(0, None, None, None, None) == _lib.OK and not h.value
    assert lib.p2hot_eval_openings_many(ctx, 0, None, 1, None, 1, None) == _lib.OK
    # null tables
    assert pp(M, None) == _lib.EINVAL and "null argument" in _err(eng)
    assert pp(M, _handles(bw), None) == _lib.EINVAL and pp(M, _handles(bw), ds, None) == _lib.EINVAL and pp(M, _handles(bw), ds, k, None) == _lib.EINVAL
    assert quot(M, None, _handles(bz)) == _lib.EINVAL and quot(M, _handles(bw), None) == _lib.EINVAL and "null argument" in _err(eng)
    assert quot(M, _handles(bw), _handles(bz), None) == _lib.EINVAL and quot(M, _handles(bw), _handles(bz), bcs, None) == _lib.EINVAL
    assert quot(M, _handles(bw), _handles(bz), out=None) == _lib.EINVAL and "nothing asked for" in _err(eng)
    pts, out = tg._rand(rng, M, 1, 2), np.zeros(2 * M * 2 * R, dtype=np.uint64)
    assert lib.p2hot_eval_openings_many(ctx, M, None, 1, _ptr(pts), 1, _ptr(out)) == _lib.EINVAL
    assert lib.p2hot_eval_openings_many(ctx, M, _handles(bw), 1, None, 1, _ptr(out)) == _lib.EINVAL
    assert lib.p2hot_eval_openings_many(ctx, M, _handles(bw), 1, _ptr(pts), 1, None) == _lib.EINVAL and "null argument" in _err(eng)
    # a null entry: the message names the proof
    assert pp(M, _handles([bw[0], None])) == _lib.EINVAL and "proof 1: the wires commitment is null" in _err(eng)
    assert quot(M, _handles([bw[0], None]), _handles(bz)) == _lib.EINVAL and "proof 1: the wires commitment is null" in _err(eng)
    assert quot(M, _handles(bw), _handles([None, bz[1]])) == _lib.EINVAL and "proof 0: the zs_partial_products commitment is null" in _err(eng)
    assert lib.p2hot_eval_openings_many(ctx, M, _handles([bw[0], None]), 1, _ptr(pts), 1, _ptr(out)) == _lib.EINVAL and "proof 1: oracle 0 is null" in _err(eng)
    # proofs of different degree or rate
    assert pp(M, _handles([bw[0], other_degree])) == _lib.EINVAL and "proof 1: the wires commitment differs in degree or rate" in _err(eng)
    assert pp(M, _handles([bw[0], other_rate])) == _lib.EINVAL and "proof 1: the wires commitment differs in degree or rate" in _err(eng)
    assert quot(M, _handles([bw[0], other_rate]), _handles(bz)) == _lib.EINVAL and "proof 1: the wires commitment differs in degree or rate" in _err(eng)
    assert quot(M, _handles(bw), _handles([bz[0], other_degree])) == _lib.EINVAL and "proof 1: the zs_partial_products commitment differs" in _err(eng)
    assert lib.p2hot_eval_openings_many(ctx, M, _handles([bw[0], other_degree]), 1, _ptr(pts), 1, _ptr(out)) == _lib.EINVAL and "proof 1:" in _err(eng)
    # too narrow, too many
    narrow = PolynomialBatch.from_values(tg._rand(rng, 2, n), RATE_BITS, False, CAP, engine=eng)
    assert quot(M, _handles(bw), _handles([bz[0], narrow])) == _lib.EINVAL and "proof 1: the zs_partial_products commitment has 2 polynomials" in _err(eng)
    big = 65535 // R + 1
    assert pp(big, _handles([bw[0]] * big)) == _lib.EINVAL and "exceed one launch (65535)" in _err(eng)
    bigq = 65535 // (nc * qdf) + 1
    assert quot(bigq, _handles([bw[0]] * bigq), _handles([bz[0]] * bigq), al=_u64(np.ones((bigq, nc))), vals=None) == _lib.EINVAL
    assert "exceed one launch (65535)" in _err(eng)
    wide = C.c_void_p()  # W * M = 65536 one-row columns
    col = np.zeros(1, dtype=np.uint64)
    ptrs = (C.c_void_p * 65536)(*([col.ctypes.data] * 65536))
    assert lib.p2hot_cols_upload(ctx, ptrs, 65536, 0, C.byref(wide)) == _lib.OK
    hs = (C.c_void_p * 2)()
    assert lib.p2hot_commit_cols_many(ctx, wide, 2, RATE_BITS, 0, 1, None, hs) == _lib.EINVAL
    assert "W * M = 65536 polynomials exceed one launch (65535)" in _err(eng) and not any(hs)
    lib.p2hot_cols_free(wide)  # not consumed
    assert h.value in (None, 0)  # every refused call cleared its output
    assert lib.p2hot_ctx_trim(ctx) == _lib.OK


def test_errors_commitment_of_another_context(emu):
    """(emulator only: a second context on the same device costs nothing there)"""
    from plonky2_amd import _lib
    from plonky2_amd.engine import Engine
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    from tests.emu_backend import HostMemory, emu_lib
    rng = np.random.default_rng(90)
    n, R, M, nc, qdf = 32, 9, 2, 2, 4
    other = Engine(0, lib=emu_lib(), memory=HostMemory())
    bw = _commit_wires(emu, tg._rand(rng, M, R, n), False)
    fw = PolynomialBatch.from_values(tg._rand(rng, R, n), RATE_BITS, False, CAP, engine=other)
    ds = DeviceColumns.upload(tg._rand(rng, R, n), emu)
    bcs = PolynomialBatch.from_values(tg._rand(rng, 2 + R, n), RATE_BITS, False, CAP, engine=emu)
    bz = [PolynomialBatch.from_values(tg._rand(rng, nc * 3, n), RATE_BITS, False, CAP, engine=emu) for _ in range(M)]
    k = _u64([pow(G, j, P) for j in range(R)])
    ch = [_u64(c) for c in _challenges(91, M, nc)]
    h, lib, ctx = C.c_void_p(), emu.lib, emu.ctx
    mixed = _handles([bw[0], fw])
    assert lib.p2hot_partial_products_many(ctx, M, mixed, 0, ds._h, 0, _ptr(k), R, qdf, _ptr(ch[0]), _ptr(ch[1]), nc, None, C.byref(h)) == _lib.EINVAL
    assert "proof 1: the wires commitment belongs to another context" in _err(emu)
    assert lib.p2hot_quotient_polys_gates_many(ctx, M, mixed, bcs._h, 2, _handles(bz), _ptr(k), R, qdf, _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), nc, None,
                                               None, None, C.byref(h)) == _lib.EINVAL
    assert "proof 1: the wires commitment belongs to another context" in _err(emu)
    pts, out = tg._rand(rng, M, 1, 2), np.zeros(2 * M * R, dtype=np.uint64)
    assert lib.p2hot_eval_openings_many(ctx, M, mixed, 1, _ptr(pts), 1, _ptr(out)) == _lib.EINVAL and "proof 1: oracle 0" in _err(emu)
    hs = (C.c_void_p * 1)()
    assert other.lib.p2hot_commit_cols_many(other.ctx, ds._h, 1, RATE_BITS, CAP, 1, None, hs) == _lib.EINVAL
    assert "another context" in other.lib.p2hot_last_error(other.ctx).decode() and (ds.host() != 0).any()
