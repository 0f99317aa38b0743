"""The quotient's permutation terms (p2hot_quotient_polys -> plonk::quotient_perm_kernel) and the partial products / Zs
(p2hot_partial_products) against tests/vanishing_ref.py, a big-integer restatement of the reference that shares no code with
the library or the CPU oracle -- and the quotient the device produced put through the reference verifier's identity
(plonk/verifier.rs:83-98): vanishing(zeta) == Z_H(zeta) * sum_j chunk_j(zeta) zeta^(n j) at an extension point zeta, from
the library's own openings.  The divisibility property tests/test_permutation.py pins the oracle with cannot see a wrong
alpha power, a wrong alpha, a missing 1/n in L_0 or gate terms behind the wrong power; the identity can
(test_sensitivity_variants_pass_trim_and_fail_the_identity records which)."""
import hashlib

import numpy as np
import pytest

from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import G

SIGMAS_FIRST = 2   # constants_sigmas: [c0, c1, sigma_0 ...]


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _permutation(rng, num_routed, log_n):
    """routed wires constant on the cycles of a random permutation of the (wire, row) positions, and sigma_j(w^i) = k_j' w^i'
    for the position (j', i') that (j, i) maps to (circuit_builder.rs sigma_vecs, permutation_argument.rs)"""
    n = 1 << log_n
    m = num_routed * n
    perm = rng.permutation(m)
    label = np.arange(m)
    for s in range(m):      # cycle label = its smallest member
        if label[s] != s:
            continue
        t = perm[s]
        while t != s:
            label[t] = s
            t = perm[t]
    routed = _rand(rng, m)[label].reshape(num_routed, n)
    k_is = [pow(G, j, P) for j in range(num_routed)]           # get_unique_coset_shifts (field/src/cosets.rs:9-24)
    sub = np.asarray(vr.subgroup(log_n), dtype=object)
    kk = np.asarray(k_is, dtype=object)
    sig = (kk[perm // n] * sub[perm % n] % P).astype(np.uint64).reshape(num_routed, n)
    return routed, sig, k_is


def _instance(rng, nc, qdf, num_routed, rate_bits, log_n, satisfied=True, challenges=None):
    """values on H of the three committed batches.  wires = [routed..., one free wire, e, f] with e = w0 w1 and f = w0 + w1 on H
    (vr.gate_constraints); constants_sigmas = [c0, c1, sigmas...]; Zs + partial products from the restatement.  An unsatisfied
    instance has random wires (copy constraints and gate both broken): only the quotient's values are defined then."""
    n = 1 << log_n
    routed, sigmas, k_is = _permutation(rng, num_routed, log_n)
    if not satisfied:
        routed = _rand(rng, num_routed, n)
    free = _rand(rng, 1, n)
    w = np.concatenate([routed, free])
    w0, w1 = [int(v) for v in w[0]], [int(v) for v in w[1]]
    e = [a * b % P for a, b in zip(w0, w1)]
    f = [(a + b) % P for a, b in zip(w0, w1)]
    wires = np.concatenate([w, np.asarray([e, f], dtype=np.uint64)])
    if not satisfied:
        wires[-2:] = _rand(rng, 2, n)
    cs = np.concatenate([_rand(rng, SIGMAS_FIRST, n), sigmas])
    betas, gammas, alphas = challenges or ([int(v) for v in _rand(rng, nc)] for _ in range(3))
    zs = np.asarray(vr.zs_partial_products_batch(routed, sigmas, k_is, betas, gammas, qdf), dtype=np.uint64)
    return dict(nc=nc, qdf=qdf, num_routed=num_routed, rate_bits=rate_bits, log_n=log_n, n=n, k_is=k_is, betas=list(betas),
                gammas=list(gammas), alphas=list(alphas), wires=wires, cs=cs, zs=zs, routed=routed, sigmas=sigmas)


def _ref_ldes(q):
    """the restatement's own LDEs: coefficients by its naive interpolation, rows by evaluation"""
    return {name: vr.Lde(vr.interpolate_columns(q[name]), q["log_n"], q["rate_bits"]) for name in ("wires", "cs", "zs")}


def _ref_quotient(q, ldes, with_gates, variant=None):
    return vr.quotient_values(ldes["wires"], ldes["cs"], ldes["zs"], SIGMAS_FIRST, q["k_is"], q["qdf"], q["betas"], q["gammas"],
                              q["alphas"], with_gates=with_gates, variant=variant)


def _gate_sums(q, lde_w, lde_cs):
    """the caller's share of compute_quotient_polys: per challenge a and point i (natural order) reduce_with_powers of the gate
    constraints at x_i with alpha_a -- what the library places behind alpha_a^K"""
    qbits = vr.log2_ceil(q["qdf"])
    m = q["n"] << qbits
    out = np.zeros((q["nc"], m), dtype=np.uint64)
    for i in range(m):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], q["rate_bits"], qbits)
        t = vr.gate_constraints(vr.BASE, vr.get_lde_values(lde_w, li, step), vr.get_lde_values(lde_cs, li, step))
        for a in range(q["nc"]):
            out[a, i] = vr.reduce_with_powers(vr.BASE, t, q["alphas"][a])
    return out


def _zeta(rng):
    return (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))


def _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz, with_gates, variant=None):
    nc, nr = q["nc"], q["num_routed"]
    cons = vr.gate_constraints(vr.EXT, w_z, cs_z) if with_gates else []
    return vr.eval_vanishing_poly(vr.EXT, q["n"], zeta, w_z, zs_z[:nc], zs_gz[:nc], zs_z[nc:], cs_z[SIGMAS_FIRST:SIGMAS_FIRST + nr],
                                  q["k_is"], q["betas"], q["gammas"], q["alphas"], q["qdf"], cons, variant)


def _pairs(a):
    return [(int(v[0]), int(v[1])) for v in a]


# ------------------------------------------------------------------ the restatement on its own
def test_ref_l0_is_the_indicator_of_one_on_h():
    for log_n in (0, 1, 3, 5):
        n = 1 << log_n
        for i, x in enumerate(vr.subgroup(log_n)):
            assert vr.eval_l_0(vr.BASE, n, x) == (1 if i == 0 else 0)
        x = G * 5 % P     # off H: (x^n - 1) / (n (x - 1)) = (1 + x + ... + x^(n-1)) / n
        assert vr.eval_l_0(vr.BASE, n, x) == sum(pow(x, k, P) for k in range(n)) * pow(n, P - 2, P) % P
        z = (3, 11)
        lz = vr.eval_l_0(vr.EXT, n, z)
        s = (0, 0)
        for k in range(n):
            s = vr.EXT.add(s, vr.fpow(vr.EXT, z, k))
        assert lz == vr.EXT.scalar_mul(s, pow(n, P - 2, P))


def test_ref_reduce_with_powers_multi_is_the_direct_sum():
    rng = np.random.default_rng(3)
    terms = [int(v) for v in _rand(rng, 9)]
    alphas = [0, 1, P - 1, int(_rand(rng, 1)[0])]
    got = vr.reduce_with_powers_multi(vr.BASE, terms, alphas)
    for a, g in zip(alphas, got):
        assert g == sum(t * pow(a, k, P) for k, t in enumerate(terms)) % P == vr.reduce_with_powers(vr.BASE, terms, a)
    et = [(int(a), int(b)) for a, b in _rand(rng, 5, 2)]
    direct = (0, 0)
    for k, t in enumerate(et):
        direct = vr.EXT.add(direct, vr.EXT.scalar_mul(t, pow(alphas[3], k, P)))
    assert vr.reduce_with_powers_multi(vr.EXT, et, [(alphas[3], 0)]) == [direct]


def test_ref_partial_products_vanish_on_h_and_z_closes():
    rng = np.random.default_rng(5)
    for num_routed, qdf, log_n in ((12, 4, 4), (7, 3, 3), (3, 8, 2)):
        n = 1 << log_n
        routed, sigmas, k_is = _permutation(rng, num_routed, log_n)
        beta, gamma = [int(v) for v in _rand(rng, 2)]
        cols = vr.wires_permutation_partial_products_and_zs(routed, sigmas, k_is, beta, gamma, qdf)
        num_prods = vr.num_partial_products(num_routed, qdf)
        assert len(cols) == num_prods + 1
        z = cols[num_prods]
        assert z[0] == 1
        sub = vr.subgroup(log_n)
        for i in range(n):
            num = [(int(routed[j][i]) + beta * k_is[j] * sub[i] + gamma) % P for j in range(num_routed)]
            den = [(int(routed[j][i]) + beta * int(sigmas[j][i]) + gamma) % P for j in range(num_routed)]
            # Z closes: the last row's Z(g x) wraps to Z(1) = 1
            checks = vr.check_partial_products(vr.BASE, num, den, [c[i] for c in cols[:num_prods]], z[i], z[(i + 1) % n], qdf)
            assert not any(checks), (num_routed, i)
            # the same rows from the per-row functions: chunk products of num / den, running products from Z(x)
            ratios = [a * pow(b, P - 2, P) % P for a, b in zip(num, den)]
            row = vr.partial_products_and_z_gx(vr.BASE, z[i], vr.quotient_chunk_products(vr.BASE, ratios, qdf))
            assert row == [c[i] for c in cols[:num_prods]] + [z[(i + 1) % n]]
        routed[0][1] = (int(routed[0][1]) + 1) % P      # one broken copy constraint: Z no longer closes
        z_bad = vr.wires_permutation_partial_products_and_zs(routed, sigmas, k_is, beta, gamma, qdf)[num_prods]
        i = n - 1
        num = [(int(routed[j][i]) + beta * k_is[j] * sub[i] + gamma) % P for j in range(num_routed)]
        den = [(int(routed[j][i]) + beta * int(sigmas[j][i]) + gamma) % P for j in range(num_routed)]
        pp = vr.wires_permutation_partial_products_and_zs(routed, sigmas, k_is, beta, gamma, qdf)
        assert any(vr.check_partial_products(vr.BASE, num, den, [c[i] for c in pp[:num_prods]], z_bad[i], z_bad[0], qdf))


@pytest.mark.parametrize("nc,qdf,num_routed,rate_bits,log_n", [(2, 3, 5, 2, 3), (1, 5, 6, 3, 2), (3, 7, 2, 3, 1)])
def test_ref_quotient_satisfies_the_verifier_identity(nc, qdf, num_routed, rate_bits, log_n):
    """values / Z_H on the quotient coset, interpolated naively, trimmed (divisible), and verifier.rs:83-98 at a random zeta --
    the restatement alone, against its own evaluations"""
    rng = np.random.default_rng(nc * 100 + qdf)
    q = _instance(rng, nc, qdf, num_routed, rate_bits, log_n)
    ldes = _ref_ldes(q)
    chunks = vr.quotient_chunks(_ref_quotient(q, ldes, True), log_n, qdf)
    zeta = _zeta(rng)
    ev = {k: [vr.eval_ext(c, zeta) for c in ldes[k].coeffs] for k in ldes}
    gz = vr.EXT.scalar_mul(zeta, vr.subgroup(log_n)[1 % q["n"]])
    zs_gz = [vr.eval_ext(c, gz) for c in ldes["zs"].coeffs]
    van = _vanishing_at(q, zeta, ev["wires"], ev["cs"], ev["zs"], zs_gz, True)
    assert all(vr.verifier_check(vr.EXT, zeta, q["n"], van, [vr.eval_ext(c, zeta) for c in chunks], qdf))
    # barycentric evaluation from the values on H agrees with the interpolated polynomials
    assert vr.barycentric_ext(q["wires"], zeta, log_n) == ev["wires"]


# ------------------------------------------------------------------ (a) partial products and Zs
@pytest.mark.parametrize("nc,qdf,num_routed,log_n", [(1, 2, 3, 3), (2, 8, 80, 4), (3, 4, 9, 5), (4, 3, 7, 2), (4, 8, 17, 1), (2, 5, 11, 0)])
def test_partial_products_vs_restatement(eng, nc, qdf, num_routed, log_n):
    """p2hot_partial_products: [Z_0 .. Z_{nc-1}, partial products of challenge 0, 1, ...] = the restatement of prover.rs:392-449
    and :224-229; nc = 3 runs the paired kernel and one single challenge, nc = 4 two pairs"""
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products
    rng = np.random.default_rng(nc * 1000 + num_routed * 10 + log_n)
    routed, sigmas, k_is = _permutation(rng, num_routed, log_n)
    betas, gammas = [int(v) for v in _rand(rng, nc)], [int(v) for v in _rand(rng, nc)]
    if nc >= 3:
        betas[0], gammas[1], betas[2] = 0, P - 1, 1
    got = eng.host(all_wires_permutation_partial_products(routed, sigmas, k_is, qdf, betas, gammas, eng))
    exp = np.asarray(vr.zs_partial_products_batch(routed, sigmas, k_is, betas, gammas, qdf), dtype=np.uint64)
    assert got.shape == exp.shape and (got == exp).all()
    assert (got[:nc, 0] == 1).all()


# ------------------------------------------------------------------ (b) + (c): the library's quotient, pointwise and at zeta
EDGE2 = ([1, P - 1], [0, P - 1], [0, P - 1])
EDGE3 = ([0, 1, P - 1], [P - 1, 0, 1], [1, P - 1, 0])
QUOTIENT_SHAPES = [
    # nc, qdf, num_routed, rate_bits, log_n, gates, challenges
    (1, 2, 1, 1, 3, True, None),        # qbits 1 = rate: step 1; one routed wire
    (2, 3, 2, 2, 3, True, None),        # num_routed = qdf - 1, generic <2, 0>
    (3, 4, 4, 3, 1, True, EDGE3),       # num_routed = qdf, step 2, challenges 0 / 1 / P - 1
    (4, 5, 6, 3, 3, True, None),        # <4, 0>, num_routed = qdf + 1
    (2, 7, 14, 3, 5, True, None),       # num_routed = 2 qdf
    (1, 3, 80, 4, 3, False, None),      # 80 routed wires, step 4
    (3, 5, 80, 4, 1, True, None),
    (4, 2, 3, 3, 5, True, None),        # step 4, nc 4
    (2, 4, 8, 2, 3, False, EDGE2),
    (2, 8, 1, 3, 1, True, None),        # the pipelined <2, 8>: its preload clamps the column below 8 routed wires
    (2, 8, 7, 3, 3, True, None),
    (2, 8, 8, 3, 1, True, EDGE2),
    (2, 8, 9, 4, 3, True, None),
    (2, 8, 16, 3, 1, False, None),
    (2, 8, 17, 3, 3, True, None),
    (2, 8, 80, 3, 3, True, None),
]


def _library_quotient(eng, q, gate_sums):
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.plonk.prover import compute_quotient_polys
    b = {name: PolynomialBatch.from_values(q[name], q["rate_bits"], False, 0, engine=eng) for name in ("wires", "cs", "zs")}
    cols, vals = compute_quotient_polys(b["wires"], b["cs"], SIGMAS_FIRST, b["zs"], q["k_is"], q["qdf"], q["betas"], q["gammas"],
                                        q["alphas"], gate_sums=gate_sums, want_values=True, engine=eng)
    return b, cols, vals


@pytest.mark.parametrize("nc,qdf,num_routed,rate_bits,log_n,gates,challenges", QUOTIENT_SHAPES)
def test_quotient_values_and_verifier_identity(eng, nc, qdf, num_routed, rate_bits, log_n, gates, challenges):
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    rng = np.random.default_rng(nc * 7919 + qdf * 101 + num_routed * 13 + log_n)
    q = _instance(rng, nc, qdf, num_routed, rate_bits, log_n, challenges=challenges)
    ldes = _ref_ldes(q)
    gs = _gate_sums(q, ldes["wires"], ldes["cs"]) if gates else None
    b, cols, vals = _library_quotient(eng, q, gs)
    # (b) every point of the quotient coset
    exp = _ref_quotient(q, ldes, gates)
    assert (vals == np.asarray(exp, dtype=np.uint64)).all()
    chunks = vr.quotient_chunks(exp, log_n, qdf)
    got_chunks = cols.host()
    assert got_chunks.shape == (nc * qdf, q["n"]) and (got_chunks == np.asarray(chunks, dtype=np.uint64)).all()
    # (c) verifier.rs:83-98 on the library's openings (OpeningSet::new: every batch at zeta, the Zs batch at g zeta)
    b_q = PolynomialBatch.from_coeffs(got_chunks, rate_bits, False, 0, engine=eng)
    zeta = _zeta(rng)
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(log_n))
    ev = [_pairs(e[0]) for e in eval_openings([b["cs"], b["wires"], b["zs"], b_q], [zeta], eng)]
    zs_gz = _pairs(eval_openings([b["zs"]], [gz], eng)[0][0])
    cs_z, w_z, zs_z, q_z = ev
    for got, lde in ((cs_z, ldes["cs"]), (w_z, ldes["wires"]), (zs_z, ldes["zs"])):
        assert got == [vr.eval_ext(c, zeta) for c in lde.coeffs]
    assert zs_gz == [vr.eval_ext(c, gz) for c in ldes["zs"].coeffs]
    assert q_z == [vr.eval_ext(c, zeta) for c in chunks]
    van = _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz, gates)
    assert vr.verifier_check(vr.EXT, zeta, q["n"], van, q_z, qdf) == [True] * nc


@pytest.mark.parametrize("nc,qdf,num_routed,rate_bits,log_n", [(1, 2, 5, 2, 3), (2, 8, 9, 3, 2), (3, 4, 4, 2, 3), (4, 8, 12, 3, 1),
                                                                (2, 4, 80, 3, 1)])
def test_quotient_values_of_unsatisfied_witnesses(eng, nc, qdf, num_routed, rate_bits, log_n):
    """random wires (copy constraints and gate broken): the quotient is no polynomial, its values are still defined.  Power-of-two
    factors only, where nothing is trimmed"""
    rng = np.random.default_rng(nc * 31 + num_routed)
    q = _instance(rng, nc, qdf, num_routed, rate_bits, log_n, satisfied=False)
    ldes = _ref_ldes(q)
    gs = _gate_sums(q, ldes["wires"], ldes["cs"])
    _, _, vals = _library_quotient(eng, q, gs)
    assert (vals == np.asarray(_ref_quotient(q, ldes, True), dtype=np.uint64)).all()


# ------------------------------------------------------------------ (d) the CPU oracle's restatement
@pytest.mark.parametrize("nc,qdf,num_routed,rate_bits,log_n,gates,challenges", [s for s in QUOTIENT_SHAPES if s[2] <= 16 and s[4] <= 3])
def test_oracle_quotient_permutation_vs_restatement(ora, nc, qdf, num_routed, rate_bits, log_n, gates, challenges):
    rng = np.random.default_rng(nc * 7919 + qdf * 101 + num_routed * 13 + log_n)
    q = _instance(rng, nc, qdf, num_routed, rate_bits, log_n, challenges=challenges)
    ldes = _ref_ldes(q)
    gs = _gate_sums(q, ldes["wires"], ldes["cs"]) if gates else None
    lv = {name: ora.commit(q[name], rate_bits, 0, True)["leaves"] for name in ("wires", "cs", "zs")}
    got = ora.quotient_permutation(lv["wires"], lv["cs"], SIGMAS_FIRST, lv["zs"], log_n, rate_bits, q["k_is"], qdf, q["betas"],
                                   q["gammas"], q["alphas"], gs)
    assert (got == np.asarray(_ref_quotient(q, ldes, gates), dtype=np.uint64)).all()


def test_oracle_quotient_of_the_k12_path_instance_vs_restatement(ora):
    """the instance behind the committed per_proof_path records (plonky2_amd/util/synthetic.py): the oracle's Zs = the restatement's,
    the oracle's quotient values hash to the record, and at 64 sampled points of the quotient coset the restatement -- owning the
    row choice and the formula -- reproduces them from the rows of the oracle's commitments"""
    from plonky2_amd.util.proof_path import golden
    from plonky2_amd.util.synthetic import path_instance, splitmix_columns_numpy
    inst = path_instance("per_proof_path_k12")
    log_n, rb, nr, qdf = inst["log_n"], inst["rate_bits"], inst["num_routed"], inst["quotient_degree_factor"]
    n, f = 1 << log_n, inst["num_constants"]
    wires = splitmix_columns_numpy(inst["wires_seed"], inst["wires_width"], n)
    cs = splitmix_columns_numpy(inst["cs_seed"], inst["cs_width"], n)
    zs = np.asarray(vr.zs_partial_products_batch(wires[:nr], cs[f:f + nr], inst["k_is"], inst["betas"], inst["gammas"], qdf), dtype=np.uint64)
    num_prods = vr.num_partial_products(nr, qdf)
    for c in range(2):
        pp = ora.partial_products(wires[:nr], cs[f:f + nr], inst["k_is"], qdf, inst["betas"][c], inst["gammas"][c])
        assert (pp[num_prods] == zs[c]).all() and (pp[:num_prods] == zs[2 + c * num_prods:2 + (c + 1) * num_prods]).all()
    lv = {name: ora.commit(cols, rb, 0, True)["leaves"] for name, cols in (("wires", wires), ("cs", cs), ("zs", zs))}
    vals = ora.quotient_permutation(lv["wires"], lv["cs"], f, lv["zs"], log_n, rb, inst["k_is"], qdf, inst["betas"], inst["gammas"],
                                    inst["alphas"])
    rec = golden("per_proof_path_k12")
    assert hashlib.sha256(vals.astype("<u8").tobytes()).hexdigest() == rec["quotient_values_sha256"]
    L = {name: vr.Leaves(lv[name], log_n, rb) for name in lv}
    m = n << vr.log2_ceil(qdf)
    idx = [0, 1, 7, 8, m - 8, m - 1] + [int(i) for i in np.random.default_rng(12).choice(m, 58, replace=False)]
    for i in idx:
        exp = vr.quotient_value_at(i, L["wires"], L["cs"], L["zs"], f, inst["k_is"], qdf, inst["betas"], inst["gammas"], inst["alphas"])
        assert [int(vals[a, i]) for a in range(2)] == exp, i


# ------------------------------------------------------------------ (e) what the divisibility property cannot see
@pytest.mark.parametrize("variant", [v for v in vr.VARIANTS if v])
def test_sensitivity_variants_pass_trim_and_fail_the_identity(variant):
    """each deliberate mistake keeps every vanishing term zero on H, so its quotient is still a polynomial of degree below
    qdf * n (trim_to_len, the property tests/test_permutation.py pins the oracle with) -- and the verifier's identity at zeta
    rejects it"""
    rng = np.random.default_rng(2024)
    q = _instance(rng, 2, 3, 5, 2, 3)
    ldes = _ref_ldes(q)
    zeta = _zeta(rng)
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(q["log_n"]))
    ev = {k: [vr.eval_ext(c, zeta) for c in ldes[k].coeffs] for k in ldes}
    zs_gz = [vr.eval_ext(c, gz) for c in ldes["zs"].coeffs]
    van = _vanishing_at(q, zeta, ev["wires"], ev["cs"], ev["zs"], zs_gz, True)
    good = vr.quotient_chunks(_ref_quotient(q, ldes, True), q["log_n"], q["qdf"])
    assert vr.verifier_check(vr.EXT, zeta, q["n"], van, [vr.eval_ext(c, zeta) for c in good], q["qdf"]) == [True, True]
    bad_vals = _ref_quotient(q, ldes, True, variant=variant)
    assert bad_vals != _ref_quotient(q, ldes, True)
    bad = vr.quotient_chunks(bad_vals, q["log_n"], q["qdf"])          # trim_to_len still passes: no "Quotient has failed"
    assert vr.verifier_check(vr.EXT, zeta, q["n"], van, [vr.eval_ext(c, zeta) for c in bad], q["qdf"]) == [False, False]


# ------------------------------------------------------------------ full-size shapes on the MI355X
def _check_large(eng, q, samples, seed):
    """(a) in full, (c) in full with every opening of wires / constants_sigmas / Zs against the barycentric evaluation of the
    values on H, (b) at `samples` points from the library's committed rows (their LDE spot-checked against barycentric too)"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products
    rng = np.random.default_rng(seed)
    nc, qdf, log_n, rb = q["nc"], q["qdf"], q["log_n"], q["rate_bits"]
    n = q["n"]
    zs = eng.host(all_wires_permutation_partial_products(q["routed"], q["sigmas"], q["k_is"], qdf, q["betas"], q["gammas"], eng))
    assert (zs == q["zs"]).all()
    b = {name: PolynomialBatch.from_values(q[name], rb, False, 4, engine=eng) for name in ("wires", "cs", "zs")}
    qbits = vr.log2_ceil(qdf)
    m = n << qbits
    lv = {name: b[name].merkle_tree.leaves for name in ("wires", "cs")}
    step = 1 << (rb - qbits)
    rows = [vr.bitrev(i * step, log_n + rb) for i in range(m)]
    W = lv["wires"][rows].astype(object)
    C = lv["cs"][rows].astype(object)
    t0 = (W[:, 0] * W[:, 1] - W[:, -2]) % P                 # vr.gate_constraints, vectorised over the points
    t1 = C[:, 0] * ((W[:, 0] + W[:, 1] - W[:, -1]) % P) % P
    gs = np.stack([((t0 + t1 * a) % P).astype(np.uint64) for a in q["alphas"]])
    from plonky2_amd.plonk.prover import compute_quotient_polys
    cols, vals = compute_quotient_polys(b["wires"], b["cs"], SIGMAS_FIRST, b["zs"], q["k_is"], qdf, q["betas"], q["gammas"], q["alphas"],
                                        gate_sums=gs, want_values=True, engine=eng)
    chunks = cols.host()
    b_q = PolynomialBatch.from_coeffs(chunks, rb, False, 4, engine=eng)
    zeta = _zeta(rng)
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(log_n))
    cs_z, w_z, zs_z, q_z = [_pairs(e[0]) for e in eval_openings([b["cs"], b["wires"], b["zs"], b_q], [zeta], eng)]
    zs_gz = _pairs(eval_openings([b["zs"]], [gz], eng)[0][0])
    assert w_z == vr.barycentric_ext(q["wires"], zeta, log_n)
    assert cs_z == vr.barycentric_ext(q["cs"], zeta, log_n)
    assert zs_z == vr.barycentric_ext(q["zs"], zeta, log_n)
    assert zs_gz == vr.barycentric_ext(q["zs"], gz, log_n)
    for j in (0, nc * qdf - 1):
        assert q_z[j] == vr.eval_ext([int(c) for c in chunks[j]], zeta)
    van = _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz, True)
    assert vr.verifier_check(vr.EXT, zeta, n, van, q_z, qdf) == [True] * nc
    # (b) sampled points, the rows read off the library's commitments by the restatement's own row choice
    L = {name: vr.Leaves(lv[name], log_n, rb) for name in lv}
    L["zs"] = vr.Leaves(b["zs"].merkle_tree.leaves, log_n, rb)
    idx = [0, 1, m - 1] + [int(i) for i in rng.choice(m, samples, replace=False)]
    for i in idx:
        exp = vr.quotient_value_at(i, L["wires"], L["cs"], L["zs"], SIGMAS_FIRST, q["k_is"], qdf, q["betas"], q["gammas"], q["alphas"],
                                   with_gates=True)
        assert [int(vals[a, i]) for a in range(nc)] == exp, i
    for i in idx[:3]:        # the LDE those rows come from
        x = vr.quotient_point(i, log_n, qbits)
        r = vr.bitrev(i * step, log_n + rb)
        assert [(int(v), 0) for v in lv["wires"][r]] == vr.barycentric_ext(q["wires"], (x, 0), log_n)


@pytest.mark.gpu
@pytest.mark.parametrize("nc,qdf,num_routed,rate_bits,log_n,samples", [(2, 8, 80, 3, 13, 300), (4, 5, 80, 3, 12, 200)])
def test_full_size_quotient_identity(gpu, nc, qdf, num_routed, rate_bits, log_n, samples):
    """standard_recursion_config's shape (80 routed wires, 2 challenges, degree 8, rate 1/8: the pipelined <2, 8> kernel) at 2^13
    rows, and the generic <4, 0> kernel at nc = 4 / qdf = 5 over many workgroups"""
    rng = np.random.default_rng(log_n * 10 + nc)
    q = _instance(rng, nc, qdf, num_routed, rate_bits, log_n)
    _check_large(gpu, q, samples, log_n)
