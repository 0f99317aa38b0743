"""The permutation argument's vanishing polynomial, its quotient and the verifier's check of it, restated with Python integers
from the reference alone (plonky2/src/plonk/plonk_common.rs, util/partial_products.rs, plonk/prover.rs,
plonk/vanishing_poly.rs, plonk/verifier.rs; no lookups).  Independent of the library and of the CPU oracle: nothing here
imports either.  Small instances only, except where a function says it is vectorised over rows (numpy object arrays of
Python integers, the same arithmetic per row).

Field elements are Python ints (BASE) or pairs (a0, a1) = a0 + a1 X of GF(p^2) = GF(p)[X] / (X^2 - 7) (EXT,
field/src/goldilocks_extensions.rs:14-17: W = 7), so eval_vanishing_poly runs at a coset point of the prover as well as at the
verifier's zeta."""
import numpy as np

from tests.pyref import G, P, bitrev, ext_add, ext_inv, ext_mul, root_of_unity


class BASE:
    zero, one = 0, 1

    @staticmethod
    def lift(a):
        return int(a) % P

    @staticmethod
    def add(a, b):
        return (a + b) % P

    @staticmethod
    def sub(a, b):
        return (a - b) % P

    @staticmethod
    def mul(a, b):
        return a * b % P

    @staticmethod
    def scalar_mul(a, s):
        return a * (int(s) % P) % P

    @staticmethod
    def inv(a):
        assert a % P, "Tried to invert zero"
        return pow(a, P - 2, P)


class EXT:
    zero, one = (0, 0), (1, 0)

    @staticmethod
    def lift(a):
        return (int(a[0]) % P, int(a[1]) % P) if isinstance(a, (tuple, list, np.ndarray)) else (int(a) % P, 0)

    @staticmethod
    def add(a, b):
        return ext_add(a, b)

    @staticmethod
    def sub(a, b):
        return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)

    @staticmethod
    def mul(a, b):
        return ext_mul(a, b)

    @staticmethod
    def scalar_mul(a, s):
        s = int(s) % P
        return (a[0] * s % P, a[1] * s % P)

    @staticmethod
    def inv(a):
        assert a[0] % P or a[1] % P, "Tried to invert zero"
        return ext_inv(a)


def fpow(F, x, e):
    r = F.one
    while e:
        if e & 1:
            r = F.mul(r, x)
        x = F.mul(x, x)
        e >>= 1
    return r


# ------------------------------------------------------------------ plonk_common.rs:52-130
def eval_zero_poly(F, n, x):
    """plonk_common.rs:52-56: Z_H(x) = x^n - 1"""
    return F.sub(fpow(F, x, n), F.one)


def eval_l_0(F, n, x, inv_n=True):
    """plonk_common.rs:59-71: L_0(x) = Z_H(x) / (n (x - 1)), and 1 at x = 1.  inv_n=False drops the 1/n (a sensitivity
    variant, not the reference)"""
    if x == F.one:
        return F.one
    den = F.sub(x, F.one)
    if inv_n:
        den = F.scalar_mul(den, n)
    return F.mul(eval_zero_poly(F, n, x), F.inv(den))


def reduce_with_powers(F, terms, alpha):
    """plonk_common.rs:117-130: sum_t terms[t] alpha^t by Horner from the last term"""
    s = F.zero
    for t in reversed(terms):
        s = F.add(F.mul(s, alpha), t)
    return s


def reduce_with_powers_multi(F, terms, alphas):
    """plonk_common.rs:99-115: one reduction per alpha; term.multiply_accumulate(c, alpha) = term + c * alpha"""
    cumul = [F.zero] * len(alphas)
    for t in reversed(terms):
        cumul = [F.add(t, F.mul(c, a)) for c, a in zip(cumul, alphas)]
    return cumul


# ------------------------------------------------------------------ util/partial_products.rs
def num_partial_products(n, max_degree):
    """partial_products.rs:38-47"""
    return -(-n // max_degree) - 1


def quotient_chunk_products(F, quotient_values, max_degree):
    """partial_products.rs:11-23: the product of every chunk of max_degree values"""
    assert max_degree > 1 and quotient_values
    out = []
    for c in range(0, len(quotient_values), max_degree):
        p = F.one
        for v in quotient_values[c:c + max_degree]:
            p = F.mul(p, v)
        out.append(p)
    return out


def partial_products_and_z_gx(F, z_x, chunk_products):
    """partial_products.rs:25-36: z_x times the running products; the last one is Z(g x)"""
    assert chunk_products
    res, acc = [], z_x
    for c in chunk_products:
        acc = F.mul(acc, c)
        res.append(acc)
    return res


def check_partial_products(F, numerators, denominators, partials, z_x, z_gx, max_degree):
    """partial_products.rs:49-79: the accumulators run z_x, partials..., z_gx; per chunk prev * prod(num) - next * prod(den)"""
    accs = [z_x] + list(partials) + [z_gx]
    nch = -(-len(numerators) // max_degree)
    assert len(accs) == nch + 1 and len(denominators) == len(numerators)   # zip_eq
    out = []
    for c in range(nch):
        pn = pd = F.one
        for j in range(c * max_degree, min((c + 1) * max_degree, len(numerators))):
            pn = F.mul(pn, numerators[j])
            pd = F.mul(pd, denominators[j])
        out.append(F.sub(F.mul(accs[c], pn), F.mul(accs[c + 1], pd)))
    return out


# ------------------------------------------------------------------ plonk/prover.rs:224-229, :392-449
def subgroup(log_n):
    w = root_of_unity(log_n)
    out, x = [], 1
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % P
    return out


def wires_permutation_partial_products_and_zs(wires, sigmas, k_is, beta, gamma, degree):
    """prover.rs:392-449 for one (beta, gamma): per row i of H (x = w^i) the quotients
    (wire_j + beta k_j x + gamma) / (wire_j + beta sigma_j + gamma) of the routed wires, their chunk products, the running
    product from Z(x) = 1 at row 0; the last running product is Z(g x), swapped with Z(x) so that Z ends the row.  Returns the
    transpose: [num_prods + 1][n] columns, Z last.

    Vectorised over the rows: wires and sigmas are [num_routed][n], every step below is the reference's per-row arithmetic on
    all rows at once.  The chunk product of the quotients is taken as (product of numerators) / (product of denominators),
    the same field element as the product of num_j * den_j^-1 (prover.rs:430-436)."""
    wires = np.asarray(wires, dtype=object) % P
    sigmas = np.asarray(sigmas, dtype=object) % P
    r, n = wires.shape
    xs = np.asarray(subgroup(n.bit_length() - 1), dtype=object)
    beta, gamma = int(beta) % P, int(gamma) % P
    num_prods = num_partial_products(r, degree)
    chunks = []
    for c in range(0, r, degree):
        pn = np.ones(n, dtype=object)
        pd = np.ones(n, dtype=object)
        for j in range(c, min(c + degree, r)):
            pn = pn * ((wires[j] + beta * (int(k_is[j]) * xs % P) + gamma) % P) % P
            pd = pd * ((wires[j] + beta * sigmas[j] + gamma) % P) % P
        assert all(pd), "Tried to invert zero"     # batch_multiplicative_inverse
        chunks.append([int(a) * pow(int(b), P - 2, P) % P for a, b in zip(pn, pd)])
    assert len(chunks) == num_prods + 1
    cols = [[0] * n for _ in range(num_prods + 1)]
    z_x = 1
    for i in range(n):
        row = partial_products_and_z_gx(BASE, z_x, [ch[i] for ch in chunks])
        z_x, row[num_prods] = row[num_prods], z_x    # prover.rs:441-444
        for p in range(num_prods + 1):
            cols[p][i] = row[p]
    return cols


def zs_partial_products_batch(wires, sigmas, k_is, betas, gammas, degree):
    """prover.rs:219-229: every challenge's [partial products..., Z], then the batch layout of the commitment: the Z of every
    challenge first, then the partial products of challenge 0, 1, ... (zs_range / partial_products_range)"""
    per = [wires_permutation_partial_products_and_zs(wires, sigmas, k_is, b, g, degree) for b, g in zip(betas, gammas)]
    return [pp[-1] for pp in per] + [col for pp in per for col in pp[:-1]]


# ------------------------------------------------------------------ plonk/vanishing_poly.rs:57-164 (no lookups)
VARIANTS = (None, "alpha_powers_reversed", "alphas_rotated", "l0_without_inv_n", "gates_behind_alpha_k_minus_1")


def eval_vanishing_poly(F, n, x, local_wires, local_zs, next_zs, partial_products, s_sigmas, k_is, betas, gammas, alphas,
                        max_degree, constraint_terms, variant=None):
    """vanishing_poly.rs:57-164 at one point x (BASE or EXT).  local_wires: at least the routed wires; constraint_terms: the gate
    constraints' values at x (evaluate_gate_constraints); partial_products: [nc * num_prods] in the commitment's order.
    Returns one value per alpha.  `variant` names a deliberate mistake for the suite's sensitivity test; None is the reference."""
    assert variant in VARIANTS
    nc, num_routed = len(betas), len(k_is)
    num_prods = num_partial_products(num_routed, max_degree)
    l_0_x = eval_l_0(F, n, x, inv_n=variant != "l0_without_inv_n")
    z_1_terms, pp_terms = [], []
    for i in range(nc):
        z_x, z_gx = local_zs[i], next_zs[i]
        z_1_terms.append(F.mul(l_0_x, F.sub(z_x, F.one)))
        gamma = F.lift(gammas[i])
        numerators = [F.add(F.add(local_wires[j], F.scalar_mul(F.scalar_mul(x, k_is[j]), betas[i])), gamma) for j in range(num_routed)]
        denominators = [F.add(F.add(local_wires[j], F.scalar_mul(s_sigmas[j], betas[i])), gamma) for j in range(num_routed)]
        current = partial_products[i * num_prods:(i + 1) * num_prods]
        pp_terms.extend(check_partial_products(F, numerators, denominators, current, z_x, z_gx, max_degree))
    al = [F.lift(a) for a in alphas]
    if variant == "alphas_rotated":
        al = al[1:] + al[:1]
    if variant == "gates_behind_alpha_k_minus_1":
        perm = reduce_with_powers_multi(F, z_1_terms + pp_terms, al)
        K = len(z_1_terms) + len(pp_terms)
        return [F.add(p, F.mul(fpow(F, a, K - 1), reduce_with_powers(F, constraint_terms, a))) for p, a in zip(perm, al)]
    terms = z_1_terms + pp_terms + list(constraint_terms)        # vanishing_poly.rs:151-157
    if variant == "alpha_powers_reversed":
        terms = terms[::-1]
    return reduce_with_powers_multi(F, terms, al)


# ------------------------------------------------------------------ the test circuit's gate
def gate_constraints(F, wires, constants):
    """The suite's synthetic gate (not a reference gate): with the last two wire columns e, f set on H to w0 * w1 and w0 + w1,
    both constraints vanish on H.  [w0 w1 - w_e,  c0 (w0 + w1 - w_f)]"""
    w0, w1, we, wf = wires[0], wires[1], wires[-2], wires[-1]
    return [F.sub(F.mul(w0, w1), we), F.mul(constants[0], F.sub(F.add(w0, w1), wf))]


# ------------------------------------------------------------------ polynomials on H and on the cosets
def _powers(x, count):
    out, acc = [], 1
    for _ in range(count):
        out.append(acc)
        acc = acc * x % P
    return out


_IDFT = {}


def interpolate_columns(columns):
    """values on H (natural order) -> coefficients, per column: c_k = (1/n) sum_i v_i w^(-ik) (naive inverse DFT, O(n^2))"""
    V = np.asarray(columns, dtype=object).reshape(len(columns), -1) % P
    n = V.shape[1]
    if n not in _IDFT:
        w_inv = pow(root_of_unity(n.bit_length() - 1), P - 2, P)
        _IDFT[n] = np.asarray([_powers(pow(w_inv, k, P), n) for k in range(n)], dtype=object).T   # [i][k] = w^(-ik)
    n_inv = pow(n, P - 2, P)
    return [[int(c) * n_inv % P for c in row] for row in V.dot(_IDFT[n]) % P]


def interpolate(values):
    return interpolate_columns([values])[0]


def coset_interpolate(values, shift=G):
    """values at shift * w^i (natural order) -> coefficients (coset_ifft, naive)"""
    c = interpolate(values)
    return [a * s % P for a, s in zip(c, _powers(pow(shift, P - 2, P), len(c)))]


def eval_base(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def eval_ext(coeffs, x):
    acc = (0, 0)
    for c in reversed(coeffs):
        acc = ext_add(ext_mul(acc, x), (int(c) % P, 0))
    return acc


def barycentric_ext(columns, zeta, log_n):
    """p(zeta) for polynomials of degree < n given by their values on H: p(zeta) = (zeta^n - 1) / n * sum_i v_i w^i / (zeta - w^i)
    (zeta outside H).  O(n) per column; vectorised over the columns."""
    n = 1 << log_n
    xs = subgroup(log_n)
    c0, c1 = [], []
    for x in xs:
        d = ext_inv(((zeta[0] - x) % P, zeta[1] % P))
        c0.append(d[0] * x % P)
        c1.append(d[1] * x % P)
    V = np.asarray(columns, dtype=object) % P
    s0, s1 = V.dot(np.asarray(c0, dtype=object)) % P, V.dot(np.asarray(c1, dtype=object)) % P
    zh = EXT.sub(fpow(EXT, (zeta[0] % P, zeta[1] % P), n), EXT.one)
    f = EXT.scalar_mul(zh, pow(n, P - 2, P))
    return [ext_mul(f, (int(a), int(b))) for a, b in zip(s0, s1)]


class Lde:
    """a batch's LDE matrix in the committed order (fri/oracle.rs:57-112, :142-147): row L holds every polynomial at
    g * w_N^bitrev(L), N = n << rate_bits.  Rows are evaluated from the coefficients when asked for (small instances)"""

    def __init__(self, coeffs, degree_bits, rate_bits):
        self.coeffs = np.asarray(coeffs, dtype=object).reshape(len(coeffs), -1) % P
        self.degree_bits, self.rate_bits = degree_bits, rate_bits
        self._rows = {}

    def point(self, L):
        bits = self.degree_bits + self.rate_bits
        return G * pow(root_of_unity(bits), bitrev(L, bits), P) % P

    def row(self, L):
        if L not in self._rows:
            x, n = self.point(L), 1 << self.degree_bits
            xp = np.asarray(_powers(x, n), dtype=object)
            self._rows[L] = [int(v) for v in self.coeffs.dot(xp) % P]
        return self._rows[L]


class Leaves:
    """the same interface over a given leaf matrix [N][W] (committed order)"""

    def __init__(self, leaves, degree_bits, rate_bits):
        self.leaves, self.degree_bits, self.rate_bits = leaves, degree_bits, rate_bits

    def row(self, L):
        return [int(v) % P for v in self.leaves[L]]


def get_lde_values(lde, index, step):
    """fri/oracle.rs:142-147: the row reverse_bits(index * step, degree_log + rate_bits)"""
    return lde.row(bitrev(index * step, lde.degree_bits + lde.rate_bits))


# ------------------------------------------------------------------ plonk/prover.rs:609-815 (the quotient loop)
def log2_ceil(v):
    return (v - 1).bit_length()


def quotient_point(i, degree_bits, quotient_degree_bits):
    """prover.rs:645, :707: x = coset_shift * two_adic_subgroup(degree_bits + quotient_degree_bits)[i]"""
    return G * pow(root_of_unity(degree_bits + quotient_degree_bits), i, P) % P


def quotient_rows(i, degree_bits, rate_bits, quotient_degree_bits):
    """prover.rs:639-643, :708-718 as indices: (index, step) of get_lde_values for the point i and for its "next" point"""
    step = 1 << (rate_bits - quotient_degree_bits)
    next_step = 1 << quotient_degree_bits
    lde_size = 1 << (degree_bits + quotient_degree_bits)
    return (i, step), ((i + next_step) % lde_size, step)


def quotient_value_at(i, wires, cs, zs, sigmas_first, k_is, max_degree, betas, gammas, alphas, num_gate_wires=None,
                      with_gates=False, variant=None):
    """one point of compute_quotient_polys' loop (prover.rs:700-803): the rows of the three commitments, eval_vanishing_poly at
    x_i, times 1 / Z_H(x_i).  Returns one value per challenge."""
    degree_bits, rate_bits = wires.degree_bits, wires.rate_bits
    qbits = log2_ceil(max_degree)
    assert qbits <= rate_bits, "Having constraints of degree higher than the rate is not supported yet."
    nc, num_routed = len(betas), len(k_is)
    num_prods = num_partial_products(num_routed, max_degree)
    (li, step), (ni, _) = quotient_rows(i, degree_bits, rate_bits, qbits)
    x = quotient_point(i, degree_bits, qbits)
    local_wires = get_lde_values(wires, li, step)
    local_cs = get_lde_values(cs, li, step)
    local_z = get_lde_values(zs, li, step)
    next_z = get_lde_values(zs, ni, step)
    s_sigmas = local_cs[sigmas_first:sigmas_first + num_routed]
    constraints = gate_constraints(BASE, local_wires, local_cs) if with_gates else []
    v = eval_vanishing_poly(BASE, 1 << degree_bits, x, local_wires, local_z[:nc], next_z[:nc], local_z[nc:nc + nc * num_prods],
                            s_sigmas, k_is, betas, gammas, alphas, max_degree, constraints, variant)
    zh_inv = BASE.inv(eval_zero_poly(BASE, 1 << degree_bits, x))    # ZeroPolyOnCoset (zero_poly_coset.rs:21-50)
    return [a * zh_inv % P for a in v]


def quotient_values(wires, cs, zs, sigmas_first, k_is, max_degree, betas, gammas, alphas, with_gates=False, variant=None):
    """every point of the quotient coset, [nc][n << log2_ceil(max_degree)] natural order (prover.rs:805-807: transposed)"""
    m = (1 << wires.degree_bits) << log2_ceil(max_degree)
    cols = [quotient_value_at(i, wires, cs, zs, sigmas_first, k_is, max_degree, betas, gammas, alphas, with_gates=with_gates,
                              variant=variant) for i in range(m)]
    return [[c[a] for c in cols] for a in range(len(betas))]


def quotient_chunks(values, degree_bits, max_degree):
    """prover.rs:274-289: coset_ifft, trim_to_len(quotient_degree_factor * n) (panics unless the tail is zero), chunks of n"""
    n = 1 << degree_bits
    out = []
    for v in values:
        co = coset_interpolate(v)
        if any(co[max_degree * n:]):
            raise ValueError("Quotient has failed, the vanishing polynomial is not divisible by Z_H")
        out.extend(co[c * n:(c + 1) * n] for c in range(max_degree))
    return out


def verifier_check(F, zeta, n, vanishing_zeta, quotient_zeta, max_degree):
    """verifier.rs:83-98: vanishing(zeta) == Z_H(zeta) * reduce_with_powers(chunk, zeta^n) for every challenge"""
    zeta_pow_deg = fpow(F, zeta, n)
    z_h_zeta = F.sub(zeta_pow_deg, F.one)
    ok = []
    for i in range(len(vanishing_zeta)):
        chunk = quotient_zeta[i * max_degree:(i + 1) * max_degree]
        ok.append(vanishing_zeta[i] == F.mul(z_h_zeta, reduce_with_powers(F, chunk, zeta_pow_deg)))
    return ok
