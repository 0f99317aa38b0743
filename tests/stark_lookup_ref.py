"""starky's logUp lookups and cross-table lookups restated with Python integers from the reference alone (starky/src/lookup.rs,
cross_table_lookup.rs, constraint_consumer.rs, vanishing_poly.rs, prover.rs::compute_quotient_polys).  Independent of the library:
nothing here imports it.  Generic over vanishing_ref.BASE / vanishing_ref.EXT where the reference is generic over the field (the
constraint side), plain integers where it is not (the generation side).  Small instances only."""
from tests import vanishing_ref as vr
from tests.pyref import G, P, root_of_unity


# ------------------------------------------------------------------ Column / Filter (lookup.rs:37-130, :137-343)
class Column:
    def __init__(self, lin=(), nxt=(), const=0):
        self.lin, self.nxt, self.const = [(c, f % P) for c, f in lin], [(c, f % P) for c, f in nxt], const % P


def col_eval(F, col, v):
    """Column::eval (lookup.rs:293-303): the current-row terms and the constant -- no next-row terms"""
    acc = F.zero
    for c, f in col.lin:
        acc = F.add(acc, F.scalar_mul(v[c], f))
    return F.add(acc, F.lift(col.const))


def col_eval_with_next(F, col, v, next_v):
    """Column::eval_with_next (lookup.rs:306-321)"""
    acc = F.zero
    for c, f in col.lin:
        acc = F.add(acc, F.scalar_mul(v[c], f))
    for c, f in col.nxt:
        acc = F.add(acc, F.scalar_mul(next_v[c], f))
    return F.add(acc, F.lift(col.const))


def col_eval_table(col, table, row):
    """Column::eval_table (lookup.rs:324-335): table[col][row], the next row wraps"""
    acc = sum(int(table[c][row]) * f for c, f in col.lin)
    acc += sum(int(table[c][(row + 1) % len(table[c])]) * f for c, f in col.nxt)
    return (acc + col.const) % P


class Filter:
    def __init__(self, products=(), constants=()):
        self.products, self.constants = list(products), list(constants)


def default_filter():
    """lookup.rs:43-50"""
    return Filter([], [Column(const=1)])


def filter_eval(F, flt, v, next_v):
    """Filter::eval_filter (lookup.rs:70-84)"""
    acc = F.zero
    for a, b in flt.products:
        acc = F.add(acc, F.mul(col_eval_with_next(F, a, v, next_v), col_eval_with_next(F, b, v, next_v)))
    for c in flt.constants:
        acc = F.add(acc, col_eval_with_next(F, c, v, next_v))
    return acc


def filter_eval_table(flt, table, row):
    """Filter::eval_table (lookup.rs:119-129)"""
    acc = sum(col_eval_table(a, table, row) * col_eval_table(b, table, row) for a, b in flt.products)
    return (acc + sum(col_eval_table(c, table, row) for c in flt.constants)) % P


class Lookup:
    def __init__(self, columns, table_column, frequencies_column, filter_columns):
        self.columns, self.table_column, self.frequencies_column, self.filter_columns = columns, table_column, frequencies_column, filter_columns


def chunk_size(constraint_degree):
    """constraint_degree.checked_sub(1).unwrap_or(1)"""
    return constraint_degree - 1 if constraint_degree >= 1 else 1


def div_ceil(a, b):
    return -(-a // b)


def num_helper_columns(lookup, constraint_degree):
    """Lookup::num_helper_columns (lookup.rs:433-441)"""
    return div_ceil(len(lookup.columns), chunk_size(constraint_degree)) + 1


def combine(F, beta, gamma, terms):
    """GrandProductChallenge::combine (lookup.rs:457-464): reduce_with_powers(terms, beta) + gamma"""
    acc = F.zero
    for t in reversed(list(terms)):
        acc = F.add(F.scalar_mul(acc, beta), t)
    return F.add(acc, F.lift(gamma))


def inv(a):
    assert a % P, "Tried to invert zero"
    return pow(a, P - 2, P)


def batch_inv(values):
    """F::batch_multiplicative_inverse: one inversion for the lot (prefix products); a zero panics"""
    pre, acc = [], 1
    for v in values:
        assert v % P, "Tried to invert zero"
        pre.append(acc)
        acc = acc * v % P
    acc = inv(acc)
    out = [0] * len(values)
    for k in reversed(range(len(values))):
        out[k] = acc * pre[k] % P
        acc = acc * values[k] % P
    return out


# ------------------------------------------------------------------ generation (lookup.rs:579-652, :746-789; cross_table_lookup.rs:383-414)
def get_helper_cols(trace, degree, columns_filters, beta, gamma, constraint_degree):
    """lookup.rs:746-789: per chunk of (columns, filter) pairs, sum of filter / combine(columns) over the rows"""
    cs = chunk_size(constraint_degree)
    out = []
    for k in range(0, len(columns_filters), cs):
        acc = [0] * degree
        for cols, flt in columns_filters[k:k + cs]:
            combined = batch_inv([combine(vr.BASE, beta, gamma, [col_eval_table(c, trace, d) for c in cols]) for d in range(degree)])
            for d in range(degree):
                acc[d] = (acc[d] + combined[d] * filter_eval_table(flt, trace, d)) % P
        out.append(acc)
    assert len(out) == div_ceil(len(columns_filters), cs)
    return out


def lookup_helper_columns(lookup, trace, challenge, constraint_degree):
    """lookup.rs:579-652: the helper columns, then Z (1 / (table + challenge) is not a column)"""
    n = len(trace[0])
    nh = num_helper_columns(lookup, constraint_degree)
    cols = get_helper_cols(trace, n, [([c], f) for c, f in zip(lookup.columns, lookup.filter_columns)], 1, challenge, constraint_degree)
    table_inv = batch_inv([(challenge + col_eval_table(lookup.table_column, trace, i)) % P for i in range(n)])
    freq = [col_eval_table(lookup.frequencies_column, trace, i) for i in range(n)]
    z = [0]
    for i in range(n - 1):
        x = (sum(c[i] for c in cols[:nh - 1]) - freq[i] * table_inv[i]) % P
        z.append((z[i] + x) % P)
    return cols + [z]


def lookup_last_increment(lookup, trace, challenge, constraint_degree, cols):
    """(sum h - m g)[n - 1]: what Z would gain on the last row (the argument closes iff Z[n-1] + this = 0)"""
    n = len(trace[0])
    g = inv((challenge + col_eval_table(lookup.table_column, trace, n - 1)) % P)
    return (sum(c[n - 1] for c in cols[:-1]) - col_eval_table(lookup.frequencies_column, trace, n - 1) * g) % P


def all_lookup_helper_columns(lookups, trace, challenges, constraint_degree):
    """prover.rs:177-195: per lookup, per challenge"""
    out = []
    for lk in lookups:
        for ch in challenges:
            out.extend(lookup_helper_columns(lk, trace, ch, constraint_degree))
    return out


def partial_sums(trace, columns_filters, beta, gamma, constraint_degree):
    """cross_table_lookup.rs:383-414: the helpers and the upside-down running sum; one pair: the sum alone"""
    degree = len(trace[0])
    helpers = get_helper_cols(trace, degree, columns_filters, beta, gamma, constraint_degree)
    z = [sum(c[degree - 1] for c in helpers) % P]
    for i in reversed(range(degree - 1)):
        z.append((z[-1] + sum(c[i] for c in helpers)) % P)
    z.reverse()
    return helpers + [z] if len(columns_filters) > 1 else [z]


class CtlZ:
    """CtlZData (cross_table_lookup.rs:155-167) before / after partial_sums"""

    def __init__(self, columns, filters, beta, gamma):
        self.columns, self.filters, self.beta, self.gamma = columns, filters, beta % P, gamma % P
        self.helper_columns, self.z = [], None


def ctl_data_for_table(trace, zs, constraint_degree):
    for z in zs:
        ps = partial_sums(trace, list(zip(z.columns, z.filters)), z.beta, z.gamma, constraint_degree)
        z.helper_columns, z.z = ps[:-1], ps[-1]
    return zs


def get_ctl_auxiliary_polys(zs):
    """cross_table_lookup.rs:253-261: ctl_helper_polys, then ctl_z_polys"""
    out = []
    for z in zs:
        out.extend(z.helper_columns)
    return out + [z.z for z in zs]


# ------------------------------------------------------------------ the constraint side
class ConstraintConsumer:
    """constraint_consumer.rs:14-88; `accs`: where the accumulators stand when the lookup terms begin (the STARK's own
    constraints come first, vanishing_poly.rs)"""

    def __init__(self, F, alphas, z_last, l_first, l_last, accs=None):
        self.F, self.alphas, self.z_last, self.l_first, self.l_last = F, [F.lift(a) for a in alphas], z_last, l_first, l_last
        self.accs = list(accs) if accs is not None else [F.zero] * len(alphas)
        self.terms = []  # every constraint as it came in (the reference keeps the accumulators only)

    def constraint(self, c):
        self.accs = [self.F.add(self.F.mul(acc, a), c) for acc, a in zip(self.accs, self.alphas)]
        self.terms.append(c)

    def constraint_transition(self, c):
        self.constraint(self.F.mul(c, self.z_last))

    def constraint_first_row(self, c):
        self.constraint(self.F.mul(c, self.l_first))

    def constraint_last_row(self, c):
        self.constraint(self.F.mul(c, self.l_last))


def eval_helper_columns(F, filters, columns, local, nxt, helpers, constraint_degree, beta, gamma, consumer):
    """lookup.rs:655-695; columns: per pair the evaluated columns"""
    if not helpers:
        return
    cs = chunk_size(constraint_degree)
    chunks = [(columns[k:k + cs], filters[k:k + cs]) for k in range(0, len(columns), cs)]
    for (chunk, fs), h in zip(chunks, helpers):
        if len(chunk) == 2:
            c0, c1 = combine(F, beta, gamma, chunk[0]), combine(F, beta, gamma, chunk[1])
            f0, f1 = filter_eval(F, fs[0], local, nxt), filter_eval(F, fs[1], local, nxt)
            consumer.constraint(F.sub(F.sub(F.mul(F.mul(c1, c0), h), F.mul(f0, c1)), F.mul(f1, c0)))
        elif len(chunk) == 1:
            c0 = combine(F, beta, gamma, chunk[0])
            consumer.constraint(F.sub(F.mul(c0, h), filter_eval(F, fs[0], local, nxt)))
        else:
            raise NotImplementedError("Allow other constraint degrees")


def eval_packed_lookups_generic(F, lookups, local, nxt, lookup_local, lookup_next, challenges, constraint_degree, consumer):
    """lookup.rs:804-863"""
    start = 0
    for lk in lookups:
        nh = num_helper_columns(lk, constraint_degree)
        for ch in challenges:
            cols = [[col_eval_with_next(F, c, local, nxt)] for c in lk.columns]
            helpers = lookup_local[start:start + nh - 1]
            eval_helper_columns(F, lk.filter_columns, cols, local, nxt, helpers, constraint_degree, 1, ch, consumer)
            z, next_z = lookup_local[start + nh - 1], lookup_next[start + nh - 1]
            twc = F.add(col_eval(F, lk.table_column, local), F.lift(ch))
            hs = F.zero
            for h in helpers:
                hs = F.add(hs, h)
            y = F.sub(F.mul(hs, twc), col_eval(F, lk.frequencies_column, local))
            consumer.constraint_first_row(z)
            consumer.constraint(F.sub(F.mul(F.sub(next_z, z), twc), y))
            start += nh


class CtlCheckVars:
    def __init__(self, helper_columns, local_z, next_z, beta, gamma, columns, filters):
        self.helper_columns, self.local_z, self.next_z, self.beta, self.gamma = helper_columns, local_z, next_z, beta, gamma
        self.columns, self.filters = columns, filters


def eval_cross_table_lookup_checks(F, local, nxt, ctl_vars, consumer, constraint_degree):
    """cross_table_lookup.rs:558-629"""
    for v in ctl_vars:
        evals = [[col_eval_with_next(F, c, local, nxt) for c in cols] for cols in v.columns]
        eval_helper_columns(F, v.filters, evals, local, nxt, v.helper_columns, constraint_degree, v.beta, v.gamma, consumer)
        if v.helper_columns:
            hs = F.zero
            for h in v.helper_columns:
                hs = F.add(hs, h)
            consumer.constraint_last_row(F.sub(v.local_z, hs))
            consumer.constraint_transition(F.sub(F.sub(v.local_z, v.next_z), hs))
        elif len(v.columns) > 1:
            c0, c1 = combine(F, v.beta, v.gamma, evals[0]), combine(F, v.beta, v.gamma, evals[1])
            f0, f1 = filter_eval(F, v.filters[0], local, nxt), filter_eval(F, v.filters[1], local, nxt)
            rest = F.add(F.mul(f0, c1), F.mul(f1, c0))
            consumer.constraint_last_row(F.sub(F.mul(F.mul(c0, c1), v.local_z), rest))
            consumer.constraint_transition(F.sub(F.mul(F.mul(c0, c1), F.sub(v.local_z, v.next_z)), rest))
        else:
            c0 = combine(F, v.beta, v.gamma, evals[0])
            f0 = filter_eval(F, v.filters[0], local, nxt)
            consumer.constraint_last_row(F.sub(F.mul(c0, v.local_z), f0))
            consumer.constraint_transition(F.sub(F.mul(c0, F.sub(v.local_z, v.next_z)), f0))


def ctl_check_vars(zs, num_helpers, aux_local, aux_next, num_lookup_columns):
    """prover.rs:596-633: the helper columns of Z i start behind those of the Zs before it; its Z is column
    num_lookup_columns + total helpers + i"""
    total, start, out = sum(num_helpers), 0, []
    for i, (z, nh) in enumerate(zip(zs, num_helpers)):
        at = num_lookup_columns + total + i
        out.append(CtlCheckVars(aux_local[num_lookup_columns + start:num_lookup_columns + start + nh], aux_local[at], aux_next[at], z.beta, z.gamma,
                                z.columns, z.filters))
        start += nh
    return out


def eval_vanishing_poly(F, local, nxt, lookups, lookup_challenges, zs, num_helpers, aux_local, aux_next, constraint_degree, consumer):
    """vanishing_poly.rs: (the STARK's own constraints -- already in the consumer), the lookups, the CTLs"""
    nlc = sum(len(lookup_challenges) * num_helper_columns(lk, constraint_degree) for lk in lookups)
    eval_packed_lookups_generic(F, lookups, local, nxt, aux_local[:nlc], aux_next[:nlc], lookup_challenges, constraint_degree, consumer)
    eval_cross_table_lookup_checks(F, local, nxt, ctl_check_vars(zs, num_helpers, aux_local, aux_next, nlc), consumer, constraint_degree)


def eval_l_0_and_l_last(F, log_n, x):
    """vanishing_poly.rs:99-106"""
    n, g = 1 << log_n, root_of_unity(log_n)
    z_x = F.sub(vr.fpow(F, x, n), F.one)
    d0 = F.scalar_mul(F.sub(x, F.one), n)
    d1 = F.scalar_mul(F.sub(F.scalar_mul(x, g), F.one), n)
    return F.mul(z_x, F.inv(d0)), F.mul(z_x, F.inv(d1))


# ------------------------------------------------------------------ compute_quotient_polys (prover.rs:488-671)
def quotient_degree_factor(constraint_degree):
    return max(1, constraint_degree - 1)


def selector_lde(n, row, qbits):
    """PolynomialValues::selector(n, row).lde_onto_coset(qbits) (prover.rs:526-529): values at g w^i, natural order"""
    log_n = n.bit_length() - 1
    coeffs = vr.interpolate([1 if i == row else 0 for i in range(n)])
    w = root_of_unity(log_n + qbits)
    return [vr.eval_base(coeffs, G * pow(w, i, P) % P) for i in range(n << qbits)]


def quotient_values(trace_lde, aux_lde, lookups, lookup_challenges, zs, num_helpers, alphas, constraint_degree, accs=None):
    """every point of the quotient coset: [nc][n << qbits], natural order.  trace_lde / aux_lde: vanishing_ref.Lde (aux_lde None
    without aux columns); accs: the caller's accumulators [nc][n << qbits] or None"""
    degree_bits, rate_bits = trace_lde.degree_bits, trace_lde.rate_bits
    n = 1 << degree_bits
    qbits = vr.log2_ceil(quotient_degree_factor(constraint_degree))
    assert qbits <= rate_bits, "Having constraints of degree higher than the rate is not supported yet."
    step, next_step, size = 1 << (rate_bits - qbits), 1 << qbits, n << qbits
    l_first, l_last = selector_lde(n, 0, qbits), selector_lde(n, n - 1, qbits)
    last = pow(root_of_unity(degree_bits), P - 2, P)
    w = root_of_unity(degree_bits + qbits)
    out = [[0] * size for _ in alphas]
    for i in range(size):
        i_next = (i + next_step) % size
        x = G * pow(w, i, P) % P
        consumer = ConstraintConsumer(vr.BASE, alphas, (x - last) % P, l_first[i], l_last[i],
                                      [int(a[i]) % P for a in accs] if accs is not None else None)
        local, nxt = vr.get_lde_values(trace_lde, i, step), vr.get_lde_values(trace_lde, i_next, step)
        aux_local = vr.get_lde_values(aux_lde, i, step) if aux_lde is not None else []
        aux_next = vr.get_lde_values(aux_lde, i_next, step) if aux_lde is not None else []
        eval_vanishing_poly(vr.BASE, local, nxt, lookups, lookup_challenges, zs, num_helpers, aux_local, aux_next, constraint_degree, consumer)
        zh_inv = vr.BASE.inv(vr.eval_zero_poly(vr.BASE, n, x))
        for a, acc in enumerate(consumer.accs):
            out[a][i] = acc * zh_inv % P
    return out


def num_terms(lookups, nc, zs, num_helpers, constraint_degree):
    return sum(nc * (num_helper_columns(lk, constraint_degree) + 1) for lk in lookups) + sum(nh + 2 for nh in num_helpers)
