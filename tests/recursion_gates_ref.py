"""The constraints of the six gates a recursive verifier circuit adds under standard_recursion_config, restated with Python integers
from the reference alone (plonky2/src/gates/{poseidon_mds,reducing,reducing_extension,random_access,exponentiation,
coset_interpolation}.rs, field/src/interpolation.rs:53-65), in the style of tests/gates_ref.py and next to it: eval_unfiltered here
takes the eight kinds of gates_ref to gates_ref and the six new ones to itself, so mixed sets work.  Generic over
vanishing_ref.BASE / EXT: over EXT an "extension element on wires c, c + 1" is an element of the extension ALGEBRA, a pair (a0, a1)
of field elements with (a0, a1)(b0, b1) = (a0 b0 + 7 a1 b1, a0 b1 + a1 b0).  Nothing here imports the library or the CPU oracle.
The barycentric weights are the definition's, 1 / prod_{j != k} (x_k - x_j), not a closed form.  A witness filler per gate makes
satisfied rows."""
from tests import gates_ref as gr
from tests.gates_ref import Gate  # noqa: F401  (the descriptor class is shared)
from tests.pyref import P, root_of_unity
from tests.vanishing_ref import BASE, reduce_with_powers

POSEIDON_MDS, REDUCING, REDUCING_EXT, RANDOM_ACCESS, EXPONENTIATION, COSET_INTERPOLATION = range(16, 22)
NEW_KINDS = tuple(range(16, 22))


def ra_param1(bits, num_extra_constants):
    return bits | num_extra_constants << 8


def _ra(g):
    """(copies, bits, extra) of a RandomAccess descriptor"""
    return g.param0, g.param1 & 0xFF, g.param1 >> 8


def _ci(g):
    """(num_points, degree, num_intermediates) of a CosetInterpolation descriptor (coset_interpolation.rs:98-100, :146-148)"""
    n = 1 << g.param0
    return n, g.param1, (n - 2) // (g.param1 - 1)


def num_wires(g):
    k = g.kind
    if k not in NEW_KINDS:
        return gr.num_wires(g)
    if k == POSEIDON_MDS:
        return 48
    if k == REDUCING:
        return 3 * g.param0 + 4
    if k == REDUCING_EXT:
        return 4 * g.param0 + 4
    if k == EXPONENTIATION:
        return 2 + 2 * g.param0
    if k == RANDOM_ACCESS:
        copies, bits, extra = _ra(g)
        return (2 + (1 << bits) + bits) * copies + extra
    n, _, ni = _ci(g)
    return 1 + 2 * n + 4 + 2 * (2 * ni + 1)


def num_constants(g):
    return _ra(g)[2] if g.kind == RANDOM_ACCESS else 0 if g.kind in NEW_KINDS else gr.num_constants(g)


def num_constraints(g):
    k = g.kind
    if k not in NEW_KINDS:
        return gr.num_constraints(g)
    if k == POSEIDON_MDS:
        return 24
    if k in (REDUCING, REDUCING_EXT):
        return 2 * g.param0
    if k == EXPONENTIATION:
        return g.param0 + 1
    if k == RANDOM_ACCESS:
        copies, bits, extra = _ra(g)
        return copies * (bits + 2) + extra
    return 4 + 4 * _ci(g)[2]


def degree(g):
    """Gate::degree of every kind (the selector groups are formed from it)"""
    k = g.kind
    return {gr.NOOP: 0, gr.CONSTANT: 1, gr.PUBLIC_INPUT: 1, gr.ARITHMETIC: 3, gr.ARITHMETIC_EXT: 3, gr.MUL_EXT: 3, gr.BASE_SUM: g.param1,
            gr.POSEIDON: 7, POSEIDON_MDS: 1, REDUCING: 2, REDUCING_EXT: 2, RANDOM_ACCESS: (g.param1 & 0xFF) + 1, EXPONENTIATION: 4,
            COSET_INTERPOLATION: g.param1}[k]


# ------------------------------------------------------------------ the extension algebra over F
def _alg(w, c):
    return (w[c], w[c + 1])


def _alg_add(F, a, b):
    return (F.add(a[0], b[0]), F.add(a[1], b[1]))


def _alg_sub(F, a, b):
    return (F.sub(a[0], b[0]), F.sub(a[1], b[1]))


# ------------------------------------------------------------------ the two-adic subgroup and its barycentric weights
def two_adic_subgroup(bits):
    g, out, x = root_of_unity(bits), [], 1
    for _ in range(1 << bits):
        out.append(x)
        x = x * g % P
    return out


def barycentric_weights(points):
    """field/src/interpolation.rs:53-65: w_k = 1 / prod_{j != k} (x_k - x_j)"""
    out = []
    for k, xk in enumerate(points):
        d = 1
        for j, xj in enumerate(points):
            if j != k:
                d = d * (xk - xj) % P
        out.append(pow(d, P - 2, P))
    return out


def _partial_interpolate(F, domain, values, weights, x, ev, prod):
    """coset_interpolation.rs:553-580 over the algebra: eval <- eval (x - x_k) + (w_k v_k) prod, prod <- prod (x - x_k)"""
    for xk, v, wk in zip(domain, values, weights):
        term = (F.sub(x[0], F.lift(xk)), x[1])
        val = (F.scalar_mul(v[0], wk), F.scalar_mul(v[1], wk))
        ev, prod = _alg_add(F, gr._alg_mul(F, ev, term), gr._alg_mul(F, val, prod)), gr._alg_mul(F, prod, term)
    return ev, prod


def _ci_wires(g):
    n, d, ni = _ci(g)
    start = 1 + 2 * n + 4
    return dict(n=n, d=d, ni=ni, point=1 + 2 * n, value=1 + 2 * n + 2, evals=start, prods=start + 2 * ni, shifted=start + 4 * ni)


def _ci_walk(F, g, w, on_intermediate):
    """the chunks of coset_interpolation.rs:263-294; on_intermediate(i, eval, prod) returns the pair the walk continues from"""
    L = _ci_wires(g)
    n, d = L["n"], L["d"]
    domain = two_adic_subgroup(g.param0)
    weights = barycentric_weights(domain)
    values = [_alg(w, 1 + 2 * i) for i in range(n)]
    x = _alg(w, L["shifted"])
    ev, prod = _partial_interpolate(F, domain[:d], values[:d], weights[:d], x, (F.zero, F.zero), (F.one, F.zero))
    for i in range(L["ni"]):
        ev, prod = on_intermediate(i, ev, prod)
        s = 1 + (d - 1) * (i + 1)
        e = min(s + d - 1, n)
        ev, prod = _partial_interpolate(F, domain[s:e], values[s:e], weights[s:e], x, ev, prod)
    return ev


# ------------------------------------------------------------------ eval_unfiltered
def eval_unfiltered(F, g, w, c, pih):
    """as gates_ref.eval_unfiltered, for all fourteen kinds"""
    k = g.kind
    if k not in NEW_KINDS:
        return gr.eval_unfiltered(F, g, w, c, pih)
    out = []
    if k == POSEIDON_MDS:                               # poseidon_mds.rs:140-175: base-field MDS entries, so per component
        comp = [gr._mds_layer(F, [w[2 * i + t] for i in range(12)]) for t in (0, 1)]
        for i in range(12):
            out += [F.sub(w[24 + 2 * i], comp[0][i]), F.sub(w[24 + 2 * i + 1], comp[1][i])]
    elif k in (REDUCING, REDUCING_EXT):                 # reducing.rs:83-127, reducing_extension.rs:85-128
        nc = g.param0
        alpha, acc = _alg(w, 2), _alg(w, 4)
        start_accs = 6 + (nc if k == REDUCING else 2 * nc)
        for i in range(nc):
            coeff = (w[6 + i], F.zero) if k == REDUCING else _alg(w, 6 + 2 * i)
            acc_i = _alg(w, 0) if i == nc - 1 else _alg(w, start_accs + 2 * i)
            out += list(_alg_sub(F, _alg_add(F, gr._alg_mul(F, acc, alpha), coeff), acc_i))
            acc = acc_i
    elif k == EXPONENTIATION:                           # exponentiation.rs:210-243
        n = g.param0
        base, bits, inter = w[0], w[1:1 + n], w[2 + n:2 + 2 * n]
        for i in range(n):
            prev = F.one if i == 0 else F.mul(inter[i - 1], inter[i - 1])
            bit = bits[n - 1 - i]
            out.append(F.sub(F.mul(prev, F.add(F.mul(bit, base), F.sub(F.one, bit))), inter[i]))
        out.append(F.sub(w[1 + n], inter[n - 1]))
    elif k == RANDOM_ACCESS:                            # random_access.rs:144-175, :302-343
        copies, nbits, extra = _ra(g)
        vec = 1 << nbits
        stride = 2 + vec
        for copy in range(copies):
            items = [w[stride * copy + 2 + i] for i in range(vec)]
            bits = [w[stride * copies + extra + copy * nbits + i] for i in range(nbits)]
            out += [F.mul(b, F.sub(b, F.one)) for b in bits]
            acc = F.zero
            for b in reversed(bits):
                acc = F.add(F.add(acc, acc), b)
            out.append(F.sub(acc, w[stride * copy]))
            for b in bits:
                items = [F.add(x, F.mul(b, F.sub(y, x))) for x, y in zip(items[0::2], items[1::2])]
            assert len(items) == 1
            out.append(F.sub(items[0], w[stride * copy + 1]))
        out += [F.sub(c[i], w[stride * copies + i]) for i in range(extra)]
    else:                                               # coset_interpolation.rs:201-298
        L = _ci_wires(g)
        shifted = _alg(w, L["shifted"])
        out += list(_alg_sub(F, _alg(w, L["point"]), (F.mul(shifted[0], w[0]), F.mul(shifted[1], w[0]))))

        def inter(i, ev, prod):
            ie, ip = _alg(w, L["evals"] + 2 * i), _alg(w, L["prods"] + 2 * i)
            out.extend(_alg_sub(F, ie, ev) + _alg_sub(F, ip, prod))
            return ie, ip
        ev = _ci_walk(F, g, w, inter)
        out += list(_alg_sub(F, _alg(w, L["value"]), ev))
    assert len(out) == num_constraints(g)
    return out


def evaluate_gate_constraints(F, gates, num_selectors, num_lookup_selectors, w, constants, pih):
    """vanishing_poly.rs:702-728 with eval_filtered (gate.rs:158-185), as gates_ref's, over all fourteen kinds"""
    out = []
    for g in gates:
        f = gr.compute_filter(F, g.row, g.group, constants[g.selector_index], num_selectors > 1)
        cons = eval_unfiltered(F, g, w, constants[num_selectors + num_lookup_selectors:], pih)
        out += [F.zero] * (len(cons) - len(out))
        for j, v in enumerate(cons):
            out[j] = F.add(out[j], F.mul(f, v))
    return out


def reduced_sums(F, gates, num_selectors, num_lookup_selectors, w, constants, pih, alphas):
    cons = evaluate_gate_constraints(F, gates, num_selectors, num_lookup_selectors, w, constants, pih)
    return [reduce_with_powers(F, cons, F.lift(a)) for a in alphas]


# ------------------------------------------------------------------ witnesses (base field)
def determined_wires(g):
    """the wires fill_witness writes; every other wire of the row is free"""
    k = g.kind
    if k not in NEW_KINDS:
        return gr.determined_wires(g)
    if k == POSEIDON_MDS:
        return list(range(24, 48))
    if k in (REDUCING, REDUCING_EXT):
        nc = g.param0
        return [0, 1] + list(range(6 + (nc if k == REDUCING else 2 * nc), num_wires(g)))
    if k == EXPONENTIATION:
        return list(range(1, num_wires(g)))
    if k == RANDOM_ACCESS:
        copies, nbits, extra = _ra(g)
        stride = 2 + (1 << nbits)
        return [stride * c + t for c in range(copies) for t in (0, 1)] + list(range(stride * copies, num_wires(g)))
    L = _ci_wires(g)
    return [L["point"], L["point"] + 1, L["value"], L["value"] + 1] + list(range(L["evals"], L["shifted"]))


def fill_witness(rng, g, w, c, pih, swap=None):
    """as gates_ref.fill_witness, for all fourteen kinds"""
    F, k = BASE, g.kind
    if k not in NEW_KINDS:
        return gr.fill_witness(rng, g, w, c, pih, swap)
    if k == POSEIDON_MDS:
        for t in (0, 1):
            for i, v in enumerate(gr._mds_layer(F, [w[2 * i + t] for i in range(12)])):
                w[24 + 2 * i + t] = v
    elif k in (REDUCING, REDUCING_EXT):
        nc = g.param0
        alpha, acc = _alg(w, 2), _alg(w, 4)
        start_accs = 6 + (nc if k == REDUCING else 2 * nc)
        for i in range(nc):
            coeff = (w[6 + i], 0) if k == REDUCING else _alg(w, 6 + 2 * i)
            acc = _alg_add(F, gr._alg_mul(F, acc, alpha), coeff)
            at = 0 if i == nc - 1 else start_accs + 2 * i
            w[at], w[at + 1] = acc
    elif k == EXPONENTIATION:
        n = g.param0
        bits = [int(v) for v in rng.integers(0, 2, size=n)]
        w[1:1 + n] = bits
        cur = 1
        for i in range(n):
            cur = cur * cur % P * (w[0] if bits[n - 1 - i] else 1) % P
            w[2 + n + i] = cur
        w[1 + n] = cur
    elif k == RANDOM_ACCESS:
        copies, nbits, extra = _ra(g)
        stride = 2 + (1 << nbits)
        for copy in range(copies):
            index = int(rng.integers(0, 1 << nbits))
            w[stride * copy], w[stride * copy + 1] = index, w[stride * copy + 2 + index]
            for i in range(nbits):
                w[stride * copies + extra + copy * nbits + i] = index >> i & 1
        for i in range(extra):
            w[stride * copies + i] = int(c[i]) % P
    else:
        L = _ci_wires(g)
        shifted = _alg(w, L["shifted"])
        w[L["point"]], w[L["point"] + 1] = shifted[0] * w[0] % P, shifted[1] * w[0] % P

        def inter(i, ev, prod):
            w[L["evals"] + 2 * i], w[L["evals"] + 2 * i + 1] = ev
            w[L["prods"] + 2 * i], w[L["prods"] + 2 * i + 1] = prod
            return ev, prod
        w[L["value"]], w[L["value"] + 1] = _ci_walk(F, g, w, inter)
