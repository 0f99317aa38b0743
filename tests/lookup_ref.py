"""The lookup argument restated with Python integers from the reference alone (plonky2/src/plonk/prover.rs:451-605,
plonk/vanishing_poly.rs:30-52, :57-164, :343-512, gates/selectors.rs:34-99, gates/lookup.rs, gates/lookup_table.rs).  Independent of
the library and of the CPU oracle: nothing here imports either.  The field classes, the LDE, the row choice of the quotient loop,
the permutation argument's vanishing terms and the verifier's check come from tests/vanishing_ref.py.

The leave-one-out products of check_lookup_constraints are restated literally (a product over j != i per i, O(d^2)), and the
polynomials walk their rows one by one with one inverse per slot, so the library's streamed sums, grouped inversions and scans are
checked against the plain forms."""
from tests import vanishing_ref as vr
from tests.pyref import P

A, B, ALPHA, DELTA = 0, 1, 2, 3                                  # LookupChallenges (plonk/circuit_builder.rs:68-73)
TRANS_SRE, TRANS_LDC, INIT_SRE, LAST_LDC, START_END = 0, 1, 2, 3, 4   # LookupSelectors (gates/selectors.rs:34-40)


def num_lu_slots(num_routed):
    """LookupGate::num_slots (gates/lookup.rs:58-61); looking inp / out of slot i on wires 2i, 2i + 1 (:63-69)"""
    return num_routed // 2


def num_lut_slots(num_routed):
    """LookupTableGate::num_slots (gates/lookup_table.rs:64-67); looked inp / out / multiplicity of slot i on wires 3i, 3i+1, 3i+2"""
    return num_routed // 3


def div_ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ gates/selectors.rs:51-99
def selectors_lookup(n, lookup_rows):
    sel = [[0] * n for _ in range(START_END)]
    for last_lu_row, last_lut_row, first_lut_row in lookup_rows:
        for row in range(last_lut_row, first_lut_row + 1):
            sel[TRANS_SRE][row] = 1
        for row in range(last_lu_row, last_lut_row):
            sel[TRANS_LDC][row] = 1
        sel[INIT_SRE][first_lut_row + 1] = 1
        sel[LAST_LDC][last_lu_row] = 1
    return sel


def selector_ends_lookups(n, lookup_rows):
    out = []
    for _, last_lut_row, _ in lookup_rows:
        e = [0] * n
        e[last_lut_row] = 1
        out.append(e)
    return out


# ------------------------------------------------------------------ plonk/vanishing_poly.rs:30-52
def get_lut_poly(lut, nb_slots, deltas, degree):
    """coefficients, lowest first, of the polynomial whose value at delta is RE at the LUT's last row"""
    b = deltas[B]
    n = len(lut)
    nb_padded_elts = (nb_slots - n % nb_slots) % nb_slots
    padding_inp, padding_out = lut[0]
    coeffs = [(inp + b * out) % P for inp, out in lut]
    coeffs += [(padding_inp + b * padding_out) % P] * nb_padded_elts
    coeffs += [0] * (degree - (n + nb_padded_elts))
    coeffs.reverse()
    return coeffs


def lut_re_poly_eval(lut, nb_slots, deltas):
    """prover.rs:652-680 / vanishing_poly.rs:410-421: get_lut_poly(.., num_lut_slots * lut_row_number).eval(delta)"""
    lut_row_number = div_ceil(len(lut), nb_slots)
    return vr.eval_base(get_lut_poly(lut, nb_slots, deltas, nb_slots * lut_row_number), deltas[DELTA])


# ------------------------------------------------------------------ plonk/prover.rs:458-605
def compute_lookup_polys(wires, deltas, lookup_rows, num_routed, max_quotient_degree_factor):
    """prover.rs:458-574 for one challenge.  wires[col][row]; returns [RE, SLDC_0 .. SLDC_{S-1}] as lists of n values"""
    degree = len(wires[0])
    lu_slots, lut_slots = num_lu_slots(num_routed), num_lut_slots(num_routed)
    max_lookup_degree = max_quotient_degree_factor - 1
    num_partial_lookups = div_ceil(lu_slots, max_lookup_degree)
    max_lookup_table_degree = div_ceil(lut_slots, num_partial_lookups)
    w = lambda row, col: int(wires[col][row]) % P
    final = [[0] * degree for _ in range(num_partial_lookups + 1)]
    for last_lu_row, last_lut_row, first_lut_row in lookup_rows:
        for row in range(first_lut_row, last_lut_row - 1, -1):
            looked_combos = [(w(row, 3 * s) + deltas[A] * w(row, 3 * s + 1)) % P for s in range(lut_slots)]
            inverses = [vr.BASE.inv((deltas[ALPHA] - c) % P) for c in looked_combos]
            lookup_combos = [(w(row, 3 * s) + deltas[B] * w(row, 3 * s + 1)) % P for s in range(lut_slots)]
            new_re = final[0][row + 1]
            for elt in lookup_combos:
                new_re = (new_re * deltas[DELTA] + elt) % P
            final[0][row] = new_re
            for slot in range(num_partial_lookups):
                prev = final[slot][row] if slot != 0 else final[num_partial_lookups][row + 1]
                acc = prev
                for s in range(slot * max_lookup_table_degree, min((slot + 1) * max_lookup_table_degree, lut_slots)):
                    acc = (acc + w(row, 3 * s + 2) * inverses[s]) % P
                final[slot + 1][row] = acc
        for row in range(last_lut_row - 1, last_lu_row - 1, -1):
            looking_combos = [(w(row, 2 * s) + deltas[A] * w(row, 2 * s + 1)) % P for s in range(lu_slots)]
            inverses = [vr.BASE.inv((deltas[ALPHA] - c) % P) for c in looking_combos]
            for slot in range(num_partial_lookups):
                prev = final[num_partial_lookups][row + 1] if slot == 0 else final[slot][row]
                acc = 0
                for s in range(slot * max_lookup_degree, min((slot + 1) * max_lookup_degree, lu_slots)):
                    acc = (acc + inverses[s]) % P
                final[slot + 1][row] = (prev - acc) % P
    return final


def compute_all_lookup_polys(wires, deltas, lookup_rows, num_routed, max_quotient_degree_factor):
    """prover.rs:577-605: deltas [nc][4]; the challenges' polynomials concatenated"""
    out = []
    for d in deltas:
        out.extend(compute_lookup_polys(wires, [int(v) % P for v in d], lookup_rows, num_routed, max_quotient_degree_factor))
    return out


# ------------------------------------------------------------------ plonk/vanishing_poly.rs:343-512
def check_lookup_constraints(F, local_wires, local_lookup_zs, next_lookup_zs, lookup_selectors, deltas, luts, num_routed,
                             quotient_degree_factor):
    """one challenge's lookup terms at a point (BASE: the batch form :515-664 with its precomputed lut_re_poly_evals is the same
    arithmetic).  local_lookup_zs / next_lookup_zs: [RE, SLDC_0 ..]; lookup_selectors: the 4 + len(luts) columns' values"""
    lu_slots, lut_slots = num_lu_slots(num_routed), num_lut_slots(num_routed)
    lu_degree = quotient_degree_factor - 1
    num_sldc_polys = len(local_lookup_zs) - 1
    lut_degree = div_ceil(lut_slots, num_sldc_polys)
    constraints = []
    z_re, next_z_re = local_lookup_zs[0], next_lookup_zs[0]
    z_x = local_lookup_zs[1:num_sldc_polys + 1]
    z_gx = next_lookup_zs[1:num_sldc_polys + 1]
    alpha = F.lift(deltas[ALPHA])
    combo = lambda i_w, o_w, ch: F.add(local_wires[i_w], F.scalar_mul(local_wires[o_w], deltas[ch]))
    looked = [combo(3 * s, 3 * s + 1, A) for s in range(lut_slots)]
    looking = [combo(2 * s, 2 * s + 1, A) for s in range(lu_slots)]
    lookup_combos = [combo(3 * s, 3 * s + 1, B) for s in range(lut_slots)]
    constraints.append(F.mul(lookup_selectors[LAST_LDC], z_x[num_sldc_polys - 1]))
    constraints.append(F.mul(lookup_selectors[INIT_SRE], z_x[0]))
    constraints.append(F.mul(lookup_selectors[INIT_SRE], z_re))
    for r in range(START_END, START_END + len(luts)):
        ev = lut_re_poly_eval(luts[r - START_END], lut_slots, deltas)
        constraints.append(F.mul(lookup_selectors[r], F.sub(z_re, F.lift(ev))))
    cur_sum = next_z_re
    for elt in lookup_combos:
        cur_sum = F.add(F.scalar_mul(cur_sum, deltas[DELTA]), elt)
    constraints.append(F.mul(lookup_selectors[TRANS_SRE], F.sub(z_re, cur_sum)))

    def product(vals):
        p = F.one
        for v in vals:
            p = F.mul(p, v)
        return p

    for poly in range(num_sldc_polys):
        lut_range = range(poly * lut_degree, min((poly + 1) * lut_degree, lut_slots))
        lu_range = range(poly * lu_degree, min((poly + 1) * lu_degree, lu_slots))
        lut_prod = product(F.sub(alpha, looked[i]) for i in lut_range)
        lu_prod = product(F.sub(alpha, looking[i]) for i in lu_range)
        lut_prod_i = lambda i: product(F.sub(alpha, looked[j]) if j != i else F.one for j in lut_range)
        lu_prod_i = lambda i: product(F.sub(alpha, looking[j]) if j != i else F.one for j in lu_range)
        lu_sum_prods = F.zero
        for i in lu_range:
            lu_sum_prods = F.add(lu_sum_prods, lu_prod_i(i))
        lut_sum_prods_with_mul = F.zero
        for i in lut_range:
            lut_sum_prods_with_mul = F.add(lut_sum_prods_with_mul, F.mul(local_wires[3 * i + 2], lut_prod_i(i)))
        prev = z_gx[num_sldc_polys - 1] if poly == 0 else z_x[poly - 1]
        diff = F.sub(z_x[poly], prev)
        constraints.append(F.mul(lookup_selectors[TRANS_SRE], F.sub(F.mul(lut_prod, diff), lut_sum_prods_with_mul)))
        constraints.append(F.mul(lookup_selectors[TRANS_LDC], F.add(F.mul(lu_prod, diff), lu_sum_prods)))
    return constraints


VARIANTS = (None, "lookups_behind_gates", "lookup_challenges_interleaved")


def all_lookup_terms(F, local_wires, local_lookup_zs, next_lookup_zs, lookup_selectors, deltas, luts, num_routed,
                     quotient_degree_factor, variant=None):
    """vanishing_poly.rs:104-121: challenge 0's terms, then challenge 1's, ...  (`variant`: a deliberate mistake)"""
    nc = len(deltas)
    npolys = len(local_lookup_zs) // nc
    per = [check_lookup_constraints(F, local_wires, local_lookup_zs[c * npolys:(c + 1) * npolys],
                                    next_lookup_zs[c * npolys:(c + 1) * npolys], lookup_selectors, [int(v) % P for v in deltas[c]],
                                    luts, num_routed, quotient_degree_factor) for c in range(nc)]
    if variant == "lookup_challenges_interleaved":
        return [per[c][t] for t in range(len(per[0])) for c in range(nc)]
    return [t for p in per for t in p]


def eval_vanishing_poly(F, n, x, local_wires, local_zs, next_zs, partial_products, local_lookup_zs, next_lookup_zs, s_sigmas,
                        lookup_selectors, k_is, betas, gammas, alphas, deltas, luts, max_degree, constraint_terms, variant=None):
    """vanishing_poly.rs:57-164 with lookups: the term list is Z_1 terms, partial-product terms, lookup terms, gate terms
    (:154-160) -- vr.eval_vanishing_poly with the lookup terms in front of the gate terms"""
    assert variant in VARIANTS
    lk = all_lookup_terms(F, local_wires, local_lookup_zs, next_lookup_zs, lookup_selectors, deltas, luts, len(k_is), max_degree,
                          variant)
    tail = list(constraint_terms) + lk if variant == "lookups_behind_gates" else lk + list(constraint_terms)
    return vr.eval_vanishing_poly(F, n, x, local_wires, local_zs, next_zs, partial_products, s_sigmas, k_is, betas, gammas, alphas,
                                  max_degree, tail)


# ------------------------------------------------------------------ plonk/prover.rs:609-815 (the quotient loop, with lookups)
def quotient_value_at(i, wires, cs, zs, selectors_first, num_luts, sigmas_first, k_is, max_degree, betas, gammas, alphas, deltas,
                      luts, with_gates=False, variant=None):
    """one point of the loop (prover.rs:700-803): zs holds the Zs, the partial products, then the lookup polynomials"""
    degree_bits, rate_bits = wires.degree_bits, wires.rate_bits
    qbits = vr.log2_ceil(max_degree)
    nc, num_routed = len(betas), len(k_is)
    num_prods = vr.num_partial_products(num_routed, max_degree)
    (li, step), (ni, _) = vr.quotient_rows(i, degree_bits, rate_bits, qbits)
    x = vr.quotient_point(i, degree_bits, qbits)
    local_wires = vr.get_lde_values(wires, li, step)
    local_cs = vr.get_lde_values(cs, li, step)
    local_z = vr.get_lde_values(zs, li, step)
    next_z = vr.get_lde_values(zs, ni, step)
    base = nc * (1 + num_prods)
    constraints = vr.gate_constraints(vr.BASE, local_wires, local_cs) if with_gates else []
    v = eval_vanishing_poly(vr.BASE, 1 << degree_bits, x, local_wires, local_z[:nc], next_z[:nc], local_z[nc:base], local_z[base:],
                            next_z[base:], local_cs[sigmas_first:sigmas_first + num_routed],
                            local_cs[selectors_first:selectors_first + 4 + num_luts], k_is, betas, gammas, alphas, deltas, luts,
                            max_degree, constraints, variant)
    zh_inv = vr.BASE.inv(vr.eval_zero_poly(vr.BASE, 1 << degree_bits, x))
    return [a * zh_inv % P for a in v]


def quotient_values(wires, cs, zs, selectors_first, num_luts, sigmas_first, k_is, max_degree, betas, gammas, alphas, deltas, luts,
                    with_gates=False, variant=None):
    m = (1 << wires.degree_bits) << vr.log2_ceil(max_degree)
    cols = [quotient_value_at(i, wires, cs, zs, selectors_first, num_luts, sigmas_first, k_is, max_degree, betas, gammas, alphas,
                              deltas, luts, with_gates, variant) for i in range(m)]
    return [[c[a] for c in cols] for a in range(len(betas))]
