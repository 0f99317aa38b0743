"""The standard gates' constraints on the device -- p2hot_gate_sums, p2hot_quotient_polys_gates, p2hot_quotient_polys_lookup_gates
(gates::cheap_gates_kernel, gates::poseidon_gate_kernel in front of the unchanged lookup and permutation kernels) -- against
tests/gates_ref.py, a big-integer restatement of the eight gates, the filter and the reduction that shares no code with the library;
and the quotient the device produced put through the verifier's identity (plonk/verifier.rs:83-98) with the gate constraints
evaluated over the extension field by the restatement.

Shapes: 135 wires (80 routed), rate_bits 3, quotient degree factor 8; 2^4 rows for one gate, 2^6 rows (512 points, two workgroups)
for the full set.  With a quotient degree factor of 8 the quotient's 8 n values hold 8 n coefficients and trim_to_len drops nothing,
so neither the reference nor the library can report "Quotient has failed" there: the broken-witness case checks at factor 8 that the
verifier's identity fails, and at factor 7 (same rate, 7 n of 8 n coefficients kept) that the call returns the error."""
import ctypes as C

import numpy as np
import pytest

from tests import gates_ref as gr
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import G, poseidon_naive

W, NUM_ROUTED, RATE_BITS, QDF = 135, 80, 3, 8
NUM_GATE_CONSTS = 2


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _full_set():
    """common_data.gates as the builder sorts them (by degree), in three selector groups as selector_polynomials forms them
    (gates/selectors.rs:101-160: group size + the largest degree in the group <= quotient degree factor + 1)"""
    kinds = [(gr.NOOP, 0, 0), (gr.CONSTANT, 2, 0), (gr.PUBLIC_INPUT, 0, 0), (gr.BASE_SUM, 63, 2), (gr.ARITHMETIC, 20, 0),
             (gr.ARITHMETIC_EXT, 10, 0), (gr.MUL_EXT, 13, 0), (gr.POSEIDON, 0, 0)]
    groups = [(0, 4), (4, 7), (7, 8)]
    out = []
    for row, (kind, p0, p1) in enumerate(kinds):
        s = next(k for k, (a, b) in enumerate(groups) if a <= row < b)
        out.append(gr.Gate(kind, row, s, groups[s], p0, p1))
    return out, len(groups)


def _alone(kind, p0=0, p1=0, row=0, group=(0, 1)):
    return [gr.Gate(kind, row, 0, group, p0, p1)]


def _selectors(gates, num_selectors, row_gate):
    """selector_polynomials: column k holds the index of the row's gate when that gate is of group k, else UNUSED_SELECTOR"""
    sel = np.full((num_selectors, len(row_gate)), gr.UNUSED_SELECTOR, dtype=np.uint64)
    for i, g in enumerate(row_gate):
        sel[gates[g].selector_index][i] = gates[g].row
    return sel


def _instance(seed, gates, num_selectors, log_n, nls=0, satisfied=False, nc=4, qdf=QDF, pih=None):
    """values on H of the committed batches: wires [135][n]; constants_sigmas = [selectors, nls lookup-selector columns, c0, c1,
    sigmas].  satisfied: every row satisfies the gate its selectors name, the routed wires carry copy cycles between free positions
    and the sigmas are that permutation's; the Zs / partial products come from the restatement."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    row_gate = [i % len(gates) for i in range(n)]
    sel = _selectors(gates, num_selectors, row_gate)
    consts = _rand(rng, NUM_GATE_CONSTS, n)
    pih = pih or [int(v) for v in _rand(rng, 4)]
    k_is = [pow(G, j, P) for j in range(NUM_ROUTED)]
    sub = vr.subgroup(log_n)
    perm = np.arange(NUM_ROUTED * n)
    wires = _rand(rng, W, n)
    if satisfied:
        w = [[int(v) for v in col] for col in wires]
        free = [(j, i) for i in range(n) for j in range(NUM_ROUTED) if j not in set(gr.determined_wires(gates[row_gate[i]]))]
        picks = [free[t] for t in rng.choice(len(free), size=min(60, len(free) // 3 * 3), replace=False)]
        for c in range(0, len(picks), 3):
            cyc = picks[c:c + 3]
            for t, (j, i) in enumerate(cyc):
                w[j][i] = w[cyc[0][0]][cyc[0][1]]
                nj, ni = cyc[(t + 1) % 3]
                perm[j * n + i] = nj * n + ni
        for i in range(n):
            row = [w[j][i] for j in range(W)]
            gr.fill_witness(rng, gates[row_gate[i]], row, [int(consts[0][i]), int(consts[1][i])], pih)
            for j in range(W):
                w[j][i] = row[j]
        wires = np.asarray(w, dtype=np.uint64)
    sigmas = np.asarray([[k_is[p // n] * sub[p % n] % P for p in perm[j * n:(j + 1) * n]] for j in range(NUM_ROUTED)], dtype=np.uint64)
    cs = np.concatenate([sel, _rand(rng, nls, n), consts, sigmas])
    betas, gammas, alphas = ([int(v) for v in _rand(rng, nc)] for _ in range(3))
    q = dict(gates=gates, ns=num_selectors, nls=nls, log_n=log_n, n=n, qdf=qdf, pih=pih, k_is=k_is, wires=wires, cs=cs,
             sigmas_first=num_selectors + nls + NUM_GATE_CONSTS, betas=betas, gammas=gammas, alphas=alphas, row_gate=row_gate)
    if satisfied:
        q["zs"] = np.asarray(vr.zs_partial_products_batch(wires[:NUM_ROUTED], sigmas, k_is, betas, gammas, qdf), dtype=np.uint64)
    return q


def _ldes(q, names=("wires", "cs"), rate_bits=RATE_BITS):
    return {name: vr.Lde(vr.interpolate_columns(q[name]), q["log_n"], rate_bits) for name in names}


def _ref_sums(q, ldes, gates=None, alphas=None):
    """the restatement at every point of the quotient coset: [len(alphas)][n << qbits]; the rate is the LDEs' own"""
    qbits = vr.log2_ceil(q["qdf"])
    m = q["n"] << qbits
    alphas = q["alphas"] if alphas is None else alphas
    out = np.zeros((len(alphas), m), dtype=np.uint64)
    for i in range(m):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], ldes["wires"].rate_bits, qbits)
        out[:, i] = gr.reduced_sums(vr.BASE, q["gates"] if gates is None else gates, q["ns"], q["nls"], vr.get_lde_values(ldes["wires"], li, step),
                                    vr.get_lde_values(ldes["cs"], li, step), q["pih"], alphas)
    return out


def _commit(eng, q, names=("wires", "cs"), rate_bits=RATE_BITS, hasher=None):
    from plonky2_amd.fri.oracle import PolynomialBatch
    return {name: PolynomialBatch.from_values(q[name], rate_bits, False, 0, engine=eng, hasher=hasher) for name in names}


def _gate_set(q, gates=None, pih=None):
    from plonky2_amd.plonk.prover import GateSet
    return GateSet([g.descriptor() for g in (q["gates"] if gates is None else gates)], q["ns"], q["nls"], pih or q["pih"])


def _device_sums(eng, q, b, nc, gates=None, pih=None, alphas=None):
    from plonky2_amd.plonk.prover import gate_sums
    return gate_sums(b["wires"], b["cs"], q["sigmas_first"], _gate_set(q, gates, pih), q["qdf"], (alphas or q["alphas"])[:nc], engine=eng)


# ------------------------------------------------------------------ the restatement on its own
ALONE = {"noop": (gr.NOOP, 0, 0), "constant1": (gr.CONSTANT, 1, 0), "constant2": (gr.CONSTANT, 2, 0), "public_input": (gr.PUBLIC_INPUT, 0, 0),
         "arithmetic": (gr.ARITHMETIC, 20, 0), "arithmetic_ext": (gr.ARITHMETIC_EXT, 10, 0), "mul_ext": (gr.MUL_EXT, 13, 0),
         "base_sum_2_63": (gr.BASE_SUM, 63, 2), "base_sum_4_31": (gr.BASE_SUM, 31, 4), "poseidon": (gr.POSEIDON, 0, 0)}


@pytest.mark.parametrize("name", sorted(ALONE))
def test_ref_constraints_vanish_on_the_filled_witness(name):
    """every constraint is zero on the filler's row, and one changed wire of the gate breaks at least one"""
    kind, p0, p1 = ALONE[name]
    g = gr.Gate(kind, 0, 0, (0, 1), p0, p1)
    rng = np.random.default_rng(kind * 100 + p0)
    for trial in range(2):
        w, c, pih = ([int(v) for v in _rand(rng, k)] for k in (W, NUM_GATE_CONSTS, 4))
        gr.fill_witness(rng, g, w, c, pih, swap=trial)
        cons = gr.eval_unfiltered(vr.BASE, g, w, c, pih)
        assert len(cons) == gr.num_constraints(g) and not any(cons)
        for j in ([0, gr.num_wires(g) - 1] + ([gr.START_PARTIAL + 7, gr.WIRE_SWAP] if kind == gr.POSEIDON else [])) if gr.num_wires(g) else []:
            bad = list(w)
            bad[j] = (bad[j] + 1) % P
            assert any(gr.eval_unfiltered(vr.BASE, g, bad, c, pih)), j


@pytest.mark.parametrize("swap", [0, 1])
def test_ref_poseidon_witness_is_the_permutation(swap):
    """the fast partial rounds of the gate and the defining 30-round form agree: the output wires are poseidon_naive(inputs)"""
    rng = np.random.default_rng(swap)
    w = [int(v) for v in _rand(rng, W)]
    gr.fill_witness(rng, gr.Gate(gr.POSEIDON, 0, 0, (0, 1)), w, [], [0] * 4, swap=swap)
    inputs = w[4:8] + w[0:4] + w[8:12] if swap else w[0:12]
    assert w[12:24] == poseidon_naive(inputs)


def test_ref_filter_selects_its_own_gate():
    gates, ns = _full_set()
    for g in gates:
        for other in gates:
            s = [gr.UNUSED_SELECTOR] * ns
            s[other.selector_index] = other.row
            f = gr.compute_filter(vr.BASE, g.row, g.group, s[g.selector_index], True)
            assert (f != 0) == (other is g), (g.row, other.row)
    assert gr.compute_filter(vr.BASE, 1, (0, 3), 1, False) == (0 - 1) * (2 - 1) % P


# ------------------------------------------------------------------ p2hot_gate_sums vs the restatement
@pytest.mark.parametrize("name", sorted(ALONE))
def test_gate_sums_of_one_gate(eng, name):
    """one kind, one selector polynomial, random wires: every term of every point is a nonzero value"""
    kind, p0, p1 = ALONE[name]
    gates = _alone(kind, p0, p1, row=1, group=(0, 3))        # (two more gates in the group: the filter has two factors)
    q = _instance(kind * 10 + p0, gates, 1, 4, nc=2)
    exp = _ref_sums(q, _ldes(q))
    got = _device_sums(eng, q, _commit(eng, q), 2)
    assert got.shape == exp.shape == (2, 16 << 3) and (got < P).all()
    assert (got == exp).all()
    assert exp.all() or kind == gr.NOOP


@pytest.mark.parametrize("nls", [0, 5])
def test_gate_sums_lookup_selectors_shift_the_constants(eng, nls):
    gates = [gr.Gate(gr.CONSTANT, 0, 0, (0, 2), 2), gr.Gate(gr.ARITHMETIC_EXT, 1, 0, (0, 2), 10)]
    q = _instance(40 + nls, gates, 1, 4, nls=nls, nc=2)
    assert (_device_sums(eng, q, _commit(eng, q), 2) == _ref_sums(q, _ldes(q))).all()


def test_gate_sums_noncanonical_public_inputs_hash(eng):
    q = _instance(50, _alone(gr.PUBLIC_INPUT), 1, 4, nc=1, pih=[3, P - 1, 0, 12345])
    b = _commit(eng, q)
    exp = _ref_sums(q, _ldes(q))
    shifted = [3 + P, P - 1, P, 12345 + P]                   # the same elements, representatives in [P, 2^64)
    assert max(shifted) < 1 << 64
    assert (_device_sums(eng, q, b, 1, pih=shifted) == exp).all() and (_device_sums(eng, q, b, 1) == exp).all()


_FULL = {}


def _full(satisfied, qdf=QDF, log_n=6):
    key = (satisfied, qdf, log_n)
    if key not in _FULL:
        gates, ns = _full_set()
        q = _instance(7 + satisfied, gates, ns, log_n, satisfied=satisfied, qdf=qdf, nc=2 if satisfied else 4)   # (the Zs batch is per nc)
        ldes = _ldes(q)
        _FULL[key] = (q, ldes, _ref_sums(q, ldes))
    return _FULL[key]


@pytest.mark.parametrize("nc", [1, 2, 3, 4])
def test_gate_sums_of_the_full_set(eng, nc):
    """all eight kinds in three selector groups (the UNUSED_SELECTOR factor; rows whose selector is 0xFFFFFFFF in two groups),
    512 points"""
    q, _, exp = _full(False)
    assert (q["cs"][:q["ns"]] == gr.UNUSED_SELECTOR).any()
    got = _device_sums(eng, q, _commit(eng, q), nc)
    assert (got == exp[:nc]).all() and exp.all()


# ------------------------------------------------------------------ the quotient
_KEEP = []


def _u64(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.uint64))
    _KEEP.append(a)
    return a.ctypes.data_as(C.c_void_p)


def _quotients(eng, q, b, nc, device_gates, host_sums):
    """(chunks, values) of p2hot_quotient_polys_gates with `device_gates` on the device and `host_sums` as the residual"""
    from plonky2_amd.plonk.prover import compute_quotient_polys_gates
    cols, vals = compute_quotient_polys_gates(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], q["qdf"], q["betas"][:nc], q["gammas"][:nc],
                                              q["alphas"][:nc], _gate_set(q, device_gates), gate_sums=host_sums, want_values=True, engine=eng)
    return cols.host(), vals


def test_quotient_equals_the_host_gate_sums_path(eng):
    """byte for byte: the device-evaluated gates against p2hot_quotient_polys fed the restated sums, with all gates on the device
    and with half of them as the host residual"""
    from plonky2_amd.plonk.prover import compute_quotient_polys
    nc = 2
    q, ldes, exp = _full(True)
    b = _commit(eng, q, ("wires", "cs", "zs"))
    cols, vals = compute_quotient_polys(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], q["qdf"], q["betas"][:nc], q["gammas"][:nc],
                                        q["alphas"][:nc], gate_sums=exp[:nc], want_values=True, engine=eng)
    chunks = cols.host()
    assert chunks.shape == (nc * QDF, q["n"]) and chunks.any()
    got_chunks, got_vals = _quotients(eng, q, b, nc, None, None)
    assert (got_vals == vals).all() and (got_chunks == chunks).all()
    half = q["gates"][0::2]
    rest = _ref_sums(q, ldes, gates=q["gates"][1::2], alphas=q["alphas"][:nc])
    got_chunks, got_vals = _quotients(eng, q, b, nc, half, rest)
    assert (got_vals == vals).all() and (got_chunks == chunks).all()


def test_lookup_quotient_equals_the_host_gate_sums_path(eng):
    """the lookup variant on an (unsatisfied: values only) lookup instance of tests/test_lookup.py -- 15 wires, constants_sigmas =
    [c0, c1, 6 lookup selectors, sigmas] read as two selector polynomials and the lookup selectors, which leaves room for gates
    without constants: PublicInput and BaseSum<2> with 10 limbs in two groups"""
    from tests import test_lookup as tl
    nc, num_routed, qdf = 2, 12, 4
    q = tl._instance(np.random.default_rng(21), nc, qdf, num_routed, 3, 4, satisfied=False)
    nls = 4 + len(q["luts"])
    assert q["sigmas_first"] == tl.SEL_FIRST + nls
    gates = [gr.Gate(gr.PUBLIC_INPUT, 0, 0, (0, 1)), gr.Gate(gr.BASE_SUM, 1, 1, (1, 3), 10, 2)]
    gq = dict(gates=gates, ns=2, nls=nls, log_n=4, n=16, qdf=qdf, pih=[5, 6, 7, 8], alphas=q["alphas"])
    ldes = {name: vr.Lde(vr.interpolate_columns(q[name]), 4, 3) for name in ("wires", "cs")}
    exp = _ref_sums(gq, ldes)
    b = tl._commit(eng, q)
    vals, got, got2 = (np.zeros((nc, 16 << 2), dtype=np.uint64) for _ in range(3))
    common = (eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b["zs"]._h, _u64(q["k_is"]), num_routed, qdf, _u64(q["betas"]), _u64(q["gammas"]),
              _u64(q["alphas"]), nc)
    lk = (q["lu_slots"], q["lut_slots"], len(q["luts"]), tl.SEL_FIRST, _u64(q["deltas"]), _u64(q["evals"]))
    assert eng.lib.p2hot_quotient_polys_lookup(*common, tl._ptrs(exp), *lk, vals.ctypes.data_as(C.c_void_p), None) == 0
    assert eng.lib.p2hot_quotient_polys_lookup_gates(*common, None, *lk, _gate_set(gq).ptr, got.ctypes.data_as(C.c_void_p), None) == 0, \
        eng.lib.p2hot_last_error(eng.ctx)
    assert exp.all() and vals.any() and (got == vals).all()
    # one gate on the device, the other as the host residual
    rest = _ref_sums(gq, ldes, gates=gates[1:])
    assert eng.lib.p2hot_quotient_polys_lookup_gates(*common, tl._ptrs(rest), *lk, _gate_set(gq, gates[:1]).ptr, got2.ctypes.data_as(C.c_void_p), None) == 0
    assert (got2 == vals).all()
    # the Python mirror makes the same call
    from plonky2_amd.plonk.prover import compute_quotient_polys_lookup_gates
    _, got3 = compute_quotient_polys_lookup_gates(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], qdf, q["betas"], q["gammas"], q["alphas"],
                                                  q["lu_slots"], q["lut_slots"], tl.SEL_FIRST, q["deltas"], q["evals"], _gate_set(gq), want_values=True,
                                                  engine=eng)
    assert (got3 == vals).all()


def _pairs(a):
    return [(int(v[0]), int(v[1])) for v in a]


def _identity_holds(eng, q, b, chunks, nc, seed):
    """vanishing(zeta) == Z_H(zeta) sum_j chunk_j(zeta) zeta^(n j) per challenge, from the library's openings and the restated gates"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    b_q = PolynomialBatch.from_coeffs(chunks, RATE_BITS, False, 0, engine=eng)
    rng = np.random.default_rng(seed)
    zeta = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(q["log_n"]))
    cs_z, w_z, zs_z, q_z = [_pairs(e[0]) for e in eval_openings([b["cs"], b["wires"], b["zs"], b_q], [zeta], eng)]
    zs_gz = _pairs(eval_openings([b["zs"]], [gz], eng)[0][0])
    cons = gr.evaluate_gate_constraints(vr.EXT, q["gates"], q["ns"], q["nls"], w_z, cs_z, q["pih"])
    sf = q["sigmas_first"]
    van = vr.eval_vanishing_poly(vr.EXT, q["n"], zeta, w_z, zs_z[:nc], zs_gz[:nc], zs_z[nc:], cs_z[sf:sf + NUM_ROUTED], q["k_is"], q["betas"][:nc],
                                 q["gammas"][:nc], q["alphas"][:nc], q["qdf"], cons)
    return vr.verifier_check(vr.EXT, zeta, q["n"], van, q_z, q["qdf"])


def _break_poseidon(q):
    """one S-box input wire of the second full rounds (not routed: the permutation argument stays satisfied) of a PoseidonGate row"""
    q = dict(q)
    wires = q["wires"].copy()
    row = q["row_gate"].index(7)
    wires[gr.START_FULL_1 + 3][row] = (int(wires[gr.START_FULL_1 + 3][row]) + 1) % P
    q["wires"] = wires
    return q


def test_verifier_identity_of_a_satisfied_circuit(eng):
    """every row satisfies its gate, the routed wires a real permutation: the device's chunks and openings satisfy the verifier's
    identity at an extension point; with one Poseidon S-box wire changed they do not (factor 8 keeps every coefficient: no trim)"""
    nc = 2
    q, _, _ = _full(True)
    b = _commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = _quotients(eng, q, b, nc, None, None)
    assert _identity_holds(eng, q, b, chunks, nc, 1) == [True] * nc
    bad = _break_poseidon(q)
    b["wires"] = _commit(eng, bad, ("wires",))["wires"]
    chunks, _ = _quotients(eng, bad, b, nc, None, None)
    assert _identity_holds(eng, bad, b, chunks, nc, 1) == [False] * nc


def test_broken_poseidon_wire_fails_the_quotient(eng):
    """quotient degree factor 7 at the same rate: 7 n of the 8 n coefficients are kept, the trim sees a quotient that is no
    polynomial.  The intact instance passes first (the three groups fit factor 7: group size + largest degree <= 8)"""
    nc = 2
    q, _, _ = _full(True, qdf=7, log_n=4)
    b = _commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = _quotients(eng, q, b, nc, None, None)
    assert chunks.shape == (nc * 7, 16) and _identity_holds(eng, q, b, chunks, nc, 2) == [True] * nc
    bad = _break_poseidon(q)
    b["wires"] = _commit(eng, bad, ("wires",))["wires"]
    with pytest.raises(ValueError, match="Quotient has failed"):
        _quotients(eng, bad, b, nc, None, None)
    h = C.c_void_p(1)
    vals = np.zeros((nc, 16 << 3), dtype=np.uint64)
    rc = eng.lib.p2hot_quotient_polys_gates(eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b["zs"]._h, _u64(q["k_is"]), NUM_ROUTED, 7,
                                            _u64(q["betas"]), _u64(q["gammas"]), _u64(q["alphas"]), nc, None, _gate_set(q).ptr,
                                            vals.ctypes.data_as(C.c_void_p), C.byref(h))
    assert rc == 1 and not h.value and b"Quotient has failed" in eng.lib.p2hot_last_error(eng.ctx)
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


# ------------------------------------------------------------------ errors
def test_errors_come_before_any_work(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.plonk.prover import GateSet
    q, _, _ = _full(True, qdf=7, log_n=4)
    b = _commit(eng, q, ("wires", "cs", "zs"))
    nc, sf = 2, q["sigmas_first"]
    out = np.zeros((nc, 16 << 3), dtype=np.uint64)

    def sums(gs, wires=None, cs=None, sigmas_first=sf, qdf=7):
        return eng.lib.p2hot_gate_sums(eng.ctx, (wires or b["wires"])._h, (cs or b["cs"])._h, sigmas_first, gs.ptr if gs else None, qdf,
                                       _u64(q["alphas"]), nc, out.ctypes.data_as(C.c_void_p))

    def quot(gs, wires=None, qdf=7):
        h = C.c_void_p(1)
        rc = eng.lib.p2hot_quotient_polys_gates(eng.ctx, (wires or b["wires"])._h, b["cs"]._h, sf, b["zs"]._h, _u64(q["k_is"]), NUM_ROUTED, qdf,
                                                _u64(q["betas"]), _u64(q["gammas"]), _u64(q["alphas"]), nc, None, gs.ptr if gs else None, None,
                                                C.byref(h))
        assert rc == _lib.OK or not h.value          # chunks_out is null after every failure
        if rc == _lib.OK:
            eng.lib.p2hot_cols_free(h)
        return rc

    def one(kind, row=0, sel=0, group=(0, 1), p0=0, p1=0, ns=3, nls=0):
        return GateSet([(kind, row, sel, group[0], group[1], p0, p1)], ns, nls)
    good = _gate_set(q)
    assert sums(good) == _lib.OK and quot(good) == _lib.OK
    cases = [
        (one(8), _lib.EUNSUPPORTED), (one(1000), _lib.EUNSUPPORTED),
        (one(gr.NOOP, row=1, group=(0, 1)), _lib.EINVAL), (one(gr.NOOP, row=0, group=(1, 3)), _lib.EINVAL),
        (one(gr.NOOP, sel=3), _lib.EINVAL),
        (one(gr.CONSTANT, p0=3), _lib.EINVAL),                       # 3 selectors + 3 constants > sigmas_first_col = 5
        (one(gr.ARITHMETIC, p0=1, nls=1), _lib.EINVAL),              # 3 + 1 + 2 constants
        (one(gr.MUL_EXT, p0=1, ns=5), _lib.EINVAL),                  # 5 selectors + 1 constant
        (one(gr.ARITHMETIC, p0=34), _lib.EINVAL),                    # 136 wires
        (one(gr.ARITHMETIC_EXT, p0=17), _lib.EINVAL), (one(gr.MUL_EXT, p0=23), _lib.EINVAL),
        (one(gr.BASE_SUM, p0=4, p1=1), _lib.EINVAL), (one(gr.BASE_SUM, p0=4, p1=0), _lib.EINVAL), (one(gr.BASE_SUM, p0=64, p1=2), _lib.EINVAL),
    ]
    for gs, code in cases:
        assert sums(gs) == code and quot(gs) == code, gs.gates
        assert eng.lib.p2hot_last_error(eng.ctx)
    # a BaseSum base above the quotient degree factor: its range constraint has degree B, and the kernel's loop is B - 1 long.
    # (factor + 1 and no larger base: before the bound a large one WAS the long-running kernel)
    # (accepted at factor 8 only: there the trim drops nothing, and this instance does not satisfy a BaseSum row)
    for base, qdf, code in ((9, 8, _lib.EINVAL), (8, 7, _lib.EINVAL), (8, 8, _lib.OK)):
        gs = one(gr.BASE_SUM, p0=4, p1=base)
        assert sums(gs, qdf=qdf) == code and quot(gs, qdf=qdf) == code, (base, qdf)
        if code != _lib.OK:
            msg = eng.lib.p2hot_last_error(eng.ctx)
            assert b"BaseSum base %d" % base in msg and b"factor %d" % qdf in msg, msg
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0
    _base_sum_bound_of_the_lookup_variant(eng)
    narrow = PolynomialBatch.from_values(q["wires"][:134], RATE_BITS, False, 0, engine=eng)
    assert sums(one(gr.POSEIDON), wires=narrow) == _lib.EINVAL and sums(one(gr.POSEIDON)) == _lib.OK
    null_gates = GateSet([], 3)
    null_gates._set.num_gates = 2
    null_gates._set.gates = None
    assert sums(null_gates) == _lib.EINVAL and quot(null_gates) == _lib.EINVAL
    assert sums(None) == _lib.EINVAL and quot(None) == _lib.EINVAL
    # commitments of another degree, another rate
    small = PolynomialBatch.from_values(q["wires"][:, :8], RATE_BITS, False, 0, engine=eng)
    rate2 = PolynomialBatch.from_values(q["wires"], 2, False, 0, engine=eng)
    for other in (small, rate2):
        assert sums(good, wires=other) == _lib.EINVAL and quot(good, wires=other) == _lib.EINVAL
    assert sums(good) == _lib.OK and quot(good) == _lib.OK and out.any()


def _base_sum_bound_of_the_lookup_variant(eng):
    """p2hot_quotient_polys_lookup_gates on the lookup instance of test_lookup_quotient_equals_the_host_gate_sums_path (factor 4):
    base 5 is refused before anything is enqueued, base 4 runs"""
    from plonky2_amd import _lib
    from tests import test_lookup as tl
    nc, num_routed, qdf = 2, 12, 4
    q = tl._instance(np.random.default_rng(22), nc, qdf, num_routed, 3, 4, satisfied=False)
    nls = 4 + len(q["luts"])
    b = tl._commit(eng, q)
    vals = np.zeros((nc, 16 << 2), dtype=np.uint64)
    from plonky2_amd.plonk.prover import GateSet
    for base, code in ((5, _lib.EINVAL), (4, _lib.OK)):
        gs = GateSet([(gr.BASE_SUM, 0, 0, 0, 1, 6, base)], 2, nls)
        vals[:] = 0
        rc = eng.lib.p2hot_quotient_polys_lookup_gates(
            eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b["zs"]._h, _u64(q["k_is"]), num_routed, qdf, _u64(q["betas"]), _u64(q["gammas"]),
            _u64(q["alphas"]), nc, None, q["lu_slots"], q["lut_slots"], len(q["luts"]), tl.SEL_FIRST, _u64(q["deltas"]), _u64(q["evals"]), gs.ptr,
            vals.ctypes.data_as(C.c_void_p), None)
        msg = eng.lib.p2hot_last_error(eng.ctx)
        assert rc == code, (base, msg)
        assert vals.any() if code == _lib.OK else not vals.any() and b"BaseSum base 5" in msg and b"factor 4" in msg, msg
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


def test_base_sum_base_equal_to_the_factor(eng):
    """the largest base the bound admits: BaseSum<8> alone in its group at factor 8 (group size 1 + degree 8 = factor + 1)"""
    q = _instance(61, _alone(gr.BASE_SUM, 5, 8), 1, 4, nc=2)
    exp = _ref_sums(q, _ldes(q))
    assert (_device_sums(eng, q, _commit(eng, q), 2) == exp).all() and exp.all()


def test_errors_commitment_of_another_context(emu):
    """(emulator only: a second context on the same device costs nothing there)"""
    from plonky2_amd import _lib
    from plonky2_amd.engine import Engine
    from tests.emu_backend import HostMemory, emu_lib
    q = _instance(3, _alone(gr.NOOP), 1, 4, nc=1)
    b = _commit(emu, q)
    other = Engine(0, lib=emu_lib(), memory=HostMemory())
    out = np.zeros((1, 16 << 3), dtype=np.uint64)
    rc = other.lib.p2hot_gate_sums(other.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], _gate_set(q).ptr, QDF, _u64(q["alphas"]), 1,
                                   out.ctypes.data_as(C.c_void_p))
    assert rc == _lib.EINVAL and b"another context" in other.lib.p2hot_last_error(other.ctx)
