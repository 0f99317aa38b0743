"""starky's lookup and cross-table-lookup stage on the device -- p2hot_stark_lookup_polys, p2hot_stark_ctl_polys (stark.hpp:
helper_rows_kernel, increments_kernel, the three scan kernels) and p2hot_stark_quotient_polys (stark::aux_terms_kernel) -- against
tests/stark_lookup_ref.py, a big-integer restatement of starky/src/lookup.rs, cross_table_lookup.rs, constraint_consumer.rs and
prover.rs::compute_quotient_polys that shares no code with the library; and the quotient the device produced put through the
verifier's identity (starky/src/verifier.rs:167-186)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import stark_lookup_ref as sr
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import root_of_unity


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _ints(rng, count):
    return [int(v) for v in _rand(rng, count)]


# ------------------------------------------------------------------ one description, two sets of objects
# a column is (lin, nxt, const); a filter is None (the default), or (products, constants) of columns
def _ref_col(c):
    return sr.Column(*c)


def _ref_filter(f):
    return sr.default_filter() if f is None else sr.Filter([(_ref_col(a), _ref_col(b)) for a, b in f[0]], [_ref_col(c) for c in f[1]])


def _lib_col(c):
    from plonky2_amd.starky.lookup import Column
    return Column(*c)


def _lib_filter(f):
    from plonky2_amd.starky.lookup import Filter
    return Filter() if f is None else Filter([(_lib_col(a), _lib_col(b)) for a, b in f[0]], [_lib_col(c) for c in f[1]])


def _ref_lookup(lk):
    return sr.Lookup([_ref_col(c) for c in lk["columns"]], _ref_col(lk["table"]), _ref_col(lk["freq"]), [_ref_filter(f) for f in lk["filters"]])


def _lib_lookup(lk):
    from plonky2_amd.starky.lookup import Lookup
    return Lookup([_lib_col(c) for c in lk["columns"]], _lib_col(lk["table"]), _lib_col(lk["freq"]), [_lib_filter(f) for f in lk["filters"]])


def _ref_z(z):
    return sr.CtlZ([[_ref_col(c) for c in cols] for cols in z["columns"]], [_ref_filter(f) for f in z["filters"]], z["beta"], z["gamma"])


def _lib_z(z):
    from plonky2_amd.starky.cross_table_lookup import CtlZData
    from plonky2_amd.starky.lookup import GrandProductChallenge
    return CtlZData(GrandProductChallenge(z["beta"], z["gamma"]), [[_lib_col(c) for c in cols] for cols in z["columns"]],
                    [_lib_filter(f) for f in z["filters"]])


def _single(c):
    return ([(c, 1)], [], 0)


# trace layout of the lookup instances: 0 table, 1 frequencies, then per looking column j its value column 2 + j, then three
# filter columns (A, B, C) shared by the filters
def _lookup_desc(num_looking, first=2, table=None, freq=None, filt_cols=None):
    """looking column j: single / 3 c + 5 / next-row / 7 c(cur) + 2 c'(next) + 1, filters: default / single column / products +
    constants, by j mod"""
    fa, fb, fc = filt_cols
    cols, filters = [], []
    for j in range(num_looking):
        c = first + j
        cols.append([_single(c), ([(c, 3)], [], 5), ([], [(c, 1)], 0), ([(c, 7)], [(fa, 2)], 1)][j % 4])
        filters.append([None, ([], [_single(fa)]), ([(_single(fb), ([(fc, 2)], [], 1))], [_single(fa), ([], [(fb, 1)], 0)])][j % 3])
    return {"columns": cols, "filters": filters, "table": table if table is not None else _single(0), "freq": freq if freq is not None else _single(1)}


def _satisfied_lookup_trace(rng, log_n, num_looking, desc=None):
    """a witness on which the logUp argument closes: the table holds n distinct values, every looking column (as its Column
    evaluates, next-row terms and the wrap at row n - 1 included) takes values of the table, and the frequency of a table entry is
    the sum of the FILTER values of the rows that look it up (the filters need not be 0 / 1)"""
    n = 1 << log_n
    W = 2 + num_looking + 3
    fa, fb, fc = W - 3, W - 2, W - 1
    desc = desc or _lookup_desc(num_looking, filt_cols=(fa, fb, fc))
    trace = [[0] * n for _ in range(W)]
    trace[0] = [int(v) for v in rng.choice(1 << 20, size=n, replace=False)]
    for c in (fa, fb, fc):
        trace[c] = [int(v) for v in rng.integers(0, 4, size=n)]
    index = {v: k for k, v in enumerate(trace[0])}
    for j, (lin, nxt, const) in enumerate(desc["columns"]):
        c = 2 + j
        target = [trace[0][int(k)] for k in rng.integers(0, n, size=n)]
        for i in range(n):
            # solve the column's own trace cell for the target: the term on column c is in lin (row i) or in nxt (row i + 1)
            rest = const + sum(trace[cc][i] * f for cc, f in lin if cc != c) + sum(trace[cc][(i + 1) % n] * f for cc, f in nxt if cc != c)
            own = [(f, i) for cc, f in lin if cc == c] + [(f, (i + 1) % n) for cc, f in nxt if cc == c]
            (f, row), = own
            trace[c][row] = (target[i] - rest) * pow(f, P - 2, P) % P
    ref = _ref_lookup(desc)
    freq = [0] * n
    for col, flt in zip(ref.columns, ref.filter_columns):
        for i in range(n):
            freq[index[sr.col_eval_table(col, trace, i)]] += sr.filter_eval_table(flt, trace, i)
    trace[1] = [f % P for f in freq]
    return trace, desc


def _ctl_instance(rng, log_n):
    """one trace that holds a looked table (columns 0, 1; filter column 2) and two looking ones (columns 3, 4 / 5, 6; filter columns
    7 / 8): the rows the looking filters select are, together, the rows the looked filter selects"""
    n = 1 << log_n
    trace = [_ints(rng, n) for _ in range(9)]
    sel = [int(v) for v in rng.integers(0, 2, size=n)]
    trace[2] = sel
    trace[7], trace[8] = [0] * n, [0] * n
    slots = list(rng.permutation(2 * n))
    for i in range(n):
        if sel[i]:
            s = int(slots.pop())
            who, row = s // n, s % n
            trace[3 + 2 * who][row], trace[4 + 2 * who][row] = trace[0][i], trace[1][i]
            trace[7 + who][row] = 1
    beta, gamma = _ints(rng, 2)
    looked = {"columns": [[_single(0), _single(1)]], "filters": [([], [_single(2)])], "beta": beta, "gamma": gamma}
    looking = {"columns": [[_single(3), _single(4)], [_single(5), _single(6)]], "filters": [([], [_single(7)]), ([], [_single(8)])], "beta": beta,
               "gamma": gamma}
    return trace, looking, looked


# ------------------------------------------------------------------ 1. (the restatement on its own: tests/test_stark_lookup_ref.py)
def test_mirror_column_constructors():
    from plonky2_amd.starky.lookup import Column, Filter
    assert (Column.single(3).linear_combination, Column.single(3).next_row_linear_combination) == ([(3, 1)], [])
    assert Column.single_next_row(2).next_row_linear_combination == [(2, 1)] and Column.single_next_row(2).linear_combination == []
    assert Column.constant(P + 5).constant_term == 5
    assert Column.le_bits([4, 5, 6]).linear_combination == [(4, 1), (5, 2), (6, 4)]
    assert Column.sum([1, 2]).linear_combination == [(1, 1), (2, 1)]
    c = Column.linear_combination_and_next_row_with_constant([(0, 2)], [(1, 3)], 4)
    assert (c.linear_combination, c.next_row_linear_combination, c.constant_term) == ([(0, 2)], [(1, 3)], 4)
    assert Column.linear_combination_with_constant([(0, 2)], 9).constant_term == 9
    with pytest.raises(ValueError):
        Column.linear_combination_with_constant([(0, 1), (0, 2)], 0)
    assert [x.constant_term for x in Filter().constants] == [1] and Filter().products == []


# ------------------------------------------------------------------ 2. the lookup polynomials
def _parity_lookups(num_looking, W):
    """two lookups in one call: the first with num_looking columns of every kind and a table column with a next-row term (generation
    evaluates it with eval_table), the second with two columns"""
    fc = (W - 3, W - 2, W - 1)
    a = _lookup_desc(num_looking, first=2, table=([(0, 1)], [(1, 5)], 3), freq=([(1, 2)], [(0, 1)], 0), filt_cols=fc)
    b = _lookup_desc(2, first=3, filt_cols=fc)
    return [a, b]


@functools.lru_cache(maxsize=None)
def _lookup_polys_case(log_n, num_looking, constraint_degree, nc):
    rng = np.random.default_rng(log_n * 1000 + num_looking * 100 + constraint_degree * 10 + nc)
    W = 2 + 5 + 3
    trace = _rand(rng, W, 1 << log_n)
    descs = _parity_lookups(num_looking, W)
    ch = _ints(rng, nc)
    exp = sr.all_lookup_helper_columns([_ref_lookup(d) for d in descs], [[int(v) for v in col] for col in trace], ch, constraint_degree)
    return trace, descs, ch, np.asarray(exp, dtype=np.uint64)


LOOKUP_CASES = [(log_n, k, cd, nc) for log_n in (3, 5) for k in (1, 2, 3, 5) for cd in (2, 3) for nc in (1, 2)] + \
    [(13, 5, 3, 2), (13, 3, 2, 1), (13, 2, 3, 1), (13, 1, 2, 2)]


@pytest.mark.parametrize("log_n,num_looking,constraint_degree,nc", LOOKUP_CASES)
def test_lookup_polys_vs_restatement(eng, log_n, num_looking, constraint_degree, nc):
    """2^13 rows is more scan chunks than the carries workgroup has threads, 2^3 fewer rows than a wave; the last chunk of looking
    columns is full or single; the wrap at row n - 1 reads row 0; both outputs"""
    from plonky2_amd.starky.lookup import lookup_helper_columns
    trace, descs, ch, exp = _lookup_polys_case(log_n, num_looking, constraint_degree, nc)
    cols, host = lookup_helper_columns(trace, [_lib_lookup(d) for d in descs], ch, constraint_degree, want_host=True, engine=eng)
    chunk = max(1, constraint_degree - 1)
    assert exp.shape == (nc * (-(-num_looking // chunk) + 1) + nc * (-(-2 // chunk) + 1), 1 << log_n) == host.shape
    assert (host == exp).all()
    assert (cols.host() == exp).all()


# ------------------------------------------------------------------ 3. the CTL polynomials
def _ctl_descs(rng, W):
    """Zs of one, two and three looking entries; entries of one and three columns (beta matters), columns with coefficients,
    constants and next-row terms, every kind of filter"""
    e1 = [_single(0)]
    e3 = [([(1, 3)], [], 5), ([], [(2, 1)], 0), ([(3, 7)], [(4, 2)], 1)]
    e3b = [_single(5), ([(6, 2)], [(6, 1)], 0), ([], [], 9)]
    f_single = ([], [_single(W - 1)])
    f_prod = ([(_single(W - 2), ([(W - 3, 2)], [], 1))], [_single(W - 1), ([], [(W - 2, 1)], 0)])
    b, g = _ints(rng, 3), _ints(rng, 3)
    return [{"columns": [e3], "filters": [f_prod], "beta": b[0], "gamma": g[0]},
            {"columns": [e1, e1], "filters": [None, f_single], "beta": b[1], "gamma": g[1]},
            {"columns": [e3, e3b, e3], "filters": [f_single, None, f_prod], "beta": b[2], "gamma": g[2]}]


@functools.lru_cache(maxsize=None)
def _ctl_polys_case(log_n, constraint_degree):
    rng = np.random.default_rng(log_n * 10 + constraint_degree)
    W = 10
    trace = _rand(rng, W, 1 << log_n)
    descs = _ctl_descs(rng, W)
    zs = sr.ctl_data_for_table([[int(v) for v in col] for col in trace], [_ref_z(d) for d in descs], constraint_degree)
    return trace, descs, [len(z.helper_columns) for z in zs], np.asarray(sr.get_ctl_auxiliary_polys(zs), dtype=np.uint64)


@pytest.mark.parametrize("constraint_degree", [2, 3])
@pytest.mark.parametrize("log_n", [3, 5, 13])
def test_ctl_polys_vs_restatement(eng, log_n, constraint_degree):
    """no helpers / one / two with the last of one entry (constraint_degree 3), none / two / three (2); the helpers of all Zs come
    before the Zs; zs_first is Z[0] of every Z"""
    from plonky2_amd.starky.cross_table_lookup import ctl_polys
    trace, descs, nh, exp = _ctl_polys_case(log_n, constraint_degree)
    assert nh == ([0, 1, 2] if constraint_degree == 3 else [0, 2, 3])
    zs = [_lib_z(d) for d in descs]
    assert [z.num_helpers(constraint_degree) for z in zs] == nh
    cols, firsts, host = ctl_polys(trace, zs, constraint_degree, want_host=True, engine=eng)
    assert host.shape == exp.shape == (sum(nh) + 3, 1 << log_n)
    assert (host == exp).all()
    assert (cols.host() == exp).all()
    assert [int(v) for v in firsts] == [int(exp[sum(nh) + k][0]) for k in range(3)]


def test_cross_table_lookup_data_groups_by_table(eng):
    """the Python mirror's bookkeeping: per CTL and challenge the looking tables by table index, then the looked table; one library
    call per table; the Zs' first values agree across the tables on a satisfied witness"""
    from plonky2_amd.starky.cross_table_lookup import CrossTableLookup, TableWithColumns, cross_table_lookup_data, get_ctl_auxiliary_polys
    from plonky2_amd.starky.lookup import GrandProductChallenge
    rng = np.random.default_rng(5)
    trace, looking, looked = _ctl_instance(rng, 4)
    t_looking = np.asarray([trace[c] for c in (3, 4, 5, 6, 7, 8)], dtype=np.uint64)     # table 0
    t_looked = np.asarray(trace[:3], dtype=np.uint64)                                     # table 1
    lc = lambda *cs: [_lib_col(_single(c)) for c in cs]  # noqa: E731
    ctl = CrossTableLookup([TableWithColumns(0, lc(0, 1), _lib_filter(([], [_single(4)]))), TableWithColumns(0, lc(2, 3), _lib_filter(([], [_single(5)])))],
                           TableWithColumns(1, lc(0, 1), _lib_filter(([], [_single(2)]))))
    chs = [GrandProductChallenge(*_ints(rng, 2)) for _ in range(2)]
    data = cross_table_lookup_data([t_looking, t_looked], [ctl], chs, 3, engine=eng)
    assert [len(d.zs_columns) for d in data] == [2, 2]
    assert data[0].num_ctl_helper_polys() == [1, 1] and data[1].num_ctl_helper_polys() == [0, 0]
    assert get_ctl_auxiliary_polys(data[0]).width == 4 and get_ctl_auxiliary_polys(data[1]).width == 2
    for k in range(2):
        assert data[0].zs_columns[k].z_first == data[1].zs_columns[k].z_first != 0
    z0 = sr.CtlZ([[sr.Column([(0, 1)]), sr.Column([(1, 1)])], [sr.Column([(2, 1)]), sr.Column([(3, 1)])]],
                 [sr.Filter([], [sr.Column([(4, 1)])]), sr.Filter([], [sr.Column([(5, 1)])])], chs[0].beta, chs[0].gamma)
    ref = sr.partial_sums([[int(v) for v in c] for c in t_looking], list(zip(z0.columns, z0.filters)), z0.beta, z0.gamma, 3)
    got = get_ctl_auxiliary_polys(data[0]).host()
    assert [int(v) for v in got[0]] == ref[0] and [int(v) for v in got[2]] == ref[1]


# ------------------------------------------------------------------ 4. the quotient, pointwise on the coset
def _commit(eng, cols, rate_bits):
    from plonky2_amd.fri.oracle import PolynomialBatch
    return PolynomialBatch.from_values(np.asarray(cols, dtype=np.uint64), rate_bits, False, 0, engine=eng)


def _lde(cols, log_n, rate_bits):
    return vr.Lde(vr.interpolate_columns([[int(v) for v in c] for c in cols]), log_n, rate_bits)


@functools.lru_cache(maxsize=None)
def _quotient_case(log_n, constraint_degree, rate_bits, kind, nc):
    """a random trace (the values of the quotient on the coset are defined for any witness), its aux polynomials by the restatement,
    and the restated quotient values without and with a random residual"""
    rng = np.random.default_rng(log_n * 1000 + constraint_degree * 100 + rate_bits * 10 + nc + len(kind))
    W, n = 10, 1 << log_n
    trace = [[int(v) for v in c] for c in _rand(rng, W, n)]
    lookups = [_lookup_desc(3, first=2, table=([(0, 1)], [(1, 5)], 3), freq=([(1, 2)], [(0, 1)], 0), filt_cols=(7, 8, 9))] if kind != "ctl" else []
    zd = _ctl_descs(rng, W)
    zdescs = [zd[0], zd[2] if constraint_degree == 3 else zd[1]] if kind != "lookup" else []
    ch, alphas = _ints(rng, nc), _ints(rng, nc)
    ref_lookups = [_ref_lookup(d) for d in lookups]
    zs = sr.ctl_data_for_table(trace, [_ref_z(d) for d in zdescs], constraint_degree)
    nh = [len(z.helper_columns) for z in zs]
    aux = sr.all_lookup_helper_columns(ref_lookups, trace, ch, constraint_degree) + sr.get_ctl_auxiliary_polys(zs)
    qbits = vr.log2_ceil(sr.quotient_degree_factor(constraint_degree))
    accs = _rand(rng, nc, n << qbits)
    t_lde, a_lde = _lde(trace, log_n, rate_bits), _lde(aux, log_n, rate_bits)
    exp = [np.asarray(sr.quotient_values(t_lde, a_lde, ref_lookups, ch, zs, nh, alphas, constraint_degree, r), dtype=np.uint64) for r in (None, accs)]
    assert sr.num_terms(ref_lookups, nc, zs, nh, constraint_degree) > 0
    return trace, aux, lookups, zdescs, ch, alphas, accs, exp


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("kind", ["both", "lookup", "ctl"])
@pytest.mark.parametrize("log_n,constraint_degree,rate_bits", [(4, 2, 1), (4, 3, 1), (4, 3, 2), (6, 2, 1), (6, 3, 1), (6, 3, 2), (4, 0, 0)])
def test_quotient_values_vs_restatement(eng, log_n, constraint_degree, rate_bits, kind, nc):
    """qbits 0 and 1, step 1 and 2 (and constraint_degree 0 at rate 1: chunks of one, qdf 1, the degree permutation_stark.rs declares); one lookup + two CTL Zs, lookups only, CTLs only (no lookup columns in front); the residual
    NULL and random: the random one pins alpha^K and the end of the Horner it sits at"""
    trace, aux, lookups, zdescs, ch, alphas, accs, exp = _quotient_case(log_n, constraint_degree, rate_bits, kind, nc)
    bt, ba = _commit(eng, trace, rate_bits), _commit(eng, aux, rate_bits)
    for r, want in zip((None, accs), exp):
        _, vals = _values_only(eng, bt, ba, ch, lookups, zdescs, alphas, constraint_degree, r)
        assert vals.shape == want.shape and want.any()
        assert (vals == want).all()
    assert (exp[0] != exp[1]).any()


def _values_only(eng, bt, ba, ch, lookups, zdescs, alphas, constraint_degree, accs, num_helpers=None):
    """p2hot_stark_quotient_polys for the VALUES on the coset alone (no chunks: nothing is trimmed, any witness has values)"""
    from plonky2_amd import _lib
    from plonky2_amd.starky.cross_table_lookup import marshal_ctl_zs
    from plonky2_amd.starky.lookup import DescriptorTables, marshal_lookups
    tables = DescriptorTables()
    lk = marshal_lookups(tables, [_lib_lookup(d) for d in lookups])
    cz = marshal_ctl_zs(tables, [_lib_z(d) for d in zdescs])
    nc = len(alphas)
    qbits = vr.log2_ceil(sr.quotient_degree_factor(constraint_degree))
    vals = np.zeros((nc, (1 << bt.degree_log) << qbits), dtype=np.uint64)
    a, c = np.asarray(alphas, dtype=np.uint64), np.asarray(ch, dtype=np.uint64)
    r = np.ascontiguousarray(accs) if accs is not None else None
    ptrs = (C.c_void_p * nc)(*[r[k].ctypes.data for k in range(nc)]) if r is not None else None
    nh = (C.c_uint * max(len(zdescs), 1))(*num_helpers) if num_helpers is not None else None
    t = tables.struct()
    rc = eng.lib.p2hot_stark_quotient_polys(eng.ctx, bt._h, ba._h if ba is not None else None, C.byref(t), lk, len(lookups), c.ctypes.data_as(C.c_void_p), cz,
                                            len(zdescs), nh, constraint_degree, a.ctypes.data_as(C.c_void_p), nc, ptrs, vals.ctypes.data_as(C.c_void_p), None)
    assert rc == _lib.OK, eng.lib.p2hot_last_error(eng.ctx)
    return None, vals


def test_quotient_ctl_branch_of_two_entries_without_helpers(eng):
    """cross_table_lookup.rs:610-621: two entries and NO helper column -- partial_sums never produces it, so the aux column (a Z
    alone) is hand made"""
    rng = np.random.default_rng(44)
    log_n, cd, rate_bits, W = 4, 3, 1, 10
    trace = [[int(v) for v in c] for c in _rand(rng, W, 1 << log_n)]
    zd = [_ctl_descs(rng, W)[1]]
    aux = [_ints(rng, 1 << log_n)]
    alphas = _ints(rng, 2)
    zs = [_ref_z(zd[0])]
    want = np.asarray(sr.quotient_values(_lde(trace, log_n, rate_bits), _lde(aux, log_n, rate_bits), [], [], zs, [0], alphas, cd), dtype=np.uint64)
    _, vals = _values_only(eng, _commit(eng, trace, rate_bits), _commit(eng, aux, rate_bits), [], [], zd, alphas, cd, None, num_helpers=[0])
    assert want.any() and (vals == want).all()


# ------------------------------------------------------------------ 5. divisibility
@functools.lru_cache(maxsize=None)
def _divisibility_case():
    rng = np.random.default_rng(55)
    log_n = 4
    trace, desc = _satisfied_lookup_trace(rng, log_n, 2)
    return log_n, trace, desc, _ints(rng, 2), _ints(rng, 2)


def _lookup_quotient(eng, log_n, trace, desc, ch, alphas, cd, rate_bits):
    from plonky2_amd.starky.lookup import lookup_helper_columns
    from plonky2_amd.starky.prover import compute_quotient_polys
    from plonky2_amd.fri.oracle import PolynomialBatch
    lookups = [_lib_lookup(desc)]
    t = np.asarray(trace, dtype=np.uint64)
    aux = lookup_helper_columns(t, lookups, ch, cd, engine=eng)
    ba = PolynomialBatch.from_values(aux, rate_bits, False, 0, engine=eng)
    return compute_quotient_polys(_commit(eng, t, rate_bits), ba, ch, lookups, None, alphas, cd, engine=eng)


def test_quotient_divisibility(eng):
    """constraint_degree 4 at rate 1/4 (qdf 3 on the coset of 4 n; chunks of three, two looking columns): a satisfied witness with
    a NULL residual returns chunks that are the restated quotient's; one changed frequency is "Quotient has failed" """
    log_n, trace, desc, ch, alphas = _divisibility_case()
    cd, rate_bits = 4, 2
    chunks = _lookup_quotient(eng, log_n, trace, desc, ch, alphas, cd, rate_bits).host()
    assert chunks.shape == (2 * 3, 1 << log_n)
    lk = _ref_lookup(desc)
    aux = sr.all_lookup_helper_columns([lk], trace, ch, cd)
    vals = sr.quotient_values(_lde(trace, log_n, rate_bits), _lde(aux, log_n, rate_bits), [lk], ch, [], [], alphas, cd)
    assert (chunks == np.asarray(vr.quotient_chunks(vals, log_n, 3), dtype=np.uint64)).all() and chunks.any()
    bad = [list(c) for c in trace]
    bad[1][5] = (bad[1][5] + 1) % P
    with pytest.raises(ValueError, match="Quotient has failed"):
        _lookup_quotient(eng, log_n, bad, desc, ch, alphas, cd, rate_bits)
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


# ------------------------------------------------------------------ 6. the verifier's identity
def _pairs(a):
    return [(int(v[0]), int(v[1])) for v in a]


def test_verifier_identity(eng):
    """permutation_stark.rs' trace (x0 + i, its rotation, frequency 1; one lookup, no constraints of its own) at constraint_degree 3,
    plus one CTL Z: the device's aux polynomials are committed, the device's quotient too, and the library's openings at zeta and
    g zeta satisfy vanishing(zeta) = Z_H(zeta) reduce_with_powers(chunks(zeta), zeta^n) (verifier.rs:167-186) with the restated
    vanishing polynomial, for every challenge; with the CTL terms in front of the lookup terms they do not"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    from plonky2_amd.plonk.prover import concat_columns
    from plonky2_amd.starky.cross_table_lookup import ctl_polys
    from plonky2_amd.starky.lookup import lookup_helper_columns
    from plonky2_amd.starky.prover import compute_quotient_polys
    rng = np.random.default_rng(66)
    log_n, cd, rate_bits, nc = 5, 3, 1, 2
    n, x0 = 1 << log_n, 12345
    trace = [[x0 + i for i in range(n)], [x0 + 1 + i for i in range(n - 1)] + [x0], [1] * n]
    ldesc = {"columns": [_single(0)], "filters": [None], "table": _single(1), "freq": _single(2)}
    zdesc = {"columns": [[_single(0), _single(1)]], "filters": [None], "beta": _ints(rng, 1)[0], "gamma": _ints(rng, 1)[0]}
    ch, alphas = _ints(rng, nc), _ints(rng, nc)
    t = np.asarray(trace, dtype=np.uint64)
    lookups, zs = [_lib_lookup(ldesc)], [_lib_z(zdesc)]
    lcols = lookup_helper_columns(t, lookups, ch, cd, engine=eng)
    ccols, firsts = ctl_polys(t, zs, cd, engine=eng)
    assert lcols.width == nc * 2 and ccols.width == 1
    bt = _commit(eng, t, rate_bits)
    ba = PolynomialBatch.from_values(concat_columns(lcols, ccols, eng), rate_bits, False, 0, engine=eng)
    chunks = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, engine=eng)
    qdf = 2
    assert chunks.width == nc * qdf
    bq = PolynomialBatch.from_coeffs(chunks, rate_bits, False, 0, engine=eng)
    zeta = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    gz = vr.EXT.scalar_mul(zeta, root_of_unity(log_n))
    t_z, a_z, q_z = [_pairs(e[0]) for e in eval_openings([bt, ba, bq], [zeta], eng)]
    t_gz, a_gz = [_pairs(e[0]) for e in eval_openings([bt, ba], [gz], eng)]
    ref_lk, ref_z = _ref_lookup(ldesc), _ref_z(zdesc)
    assert int(firsts[0]) == sr.partial_sums(trace, [(ref_z.columns[0], ref_z.filters[0])], ref_z.beta, ref_z.gamma, cd)[0][0]
    l0, ll = sr.eval_l_0_and_l_last(vr.EXT, log_n, zeta)
    z_last = vr.EXT.sub(zeta, vr.EXT.lift(pow(root_of_unity(log_n), P - 2, P)))

    def vanishing(ctl_first):
        cons = sr.ConstraintConsumer(vr.EXT, alphas, z_last, l0, ll)
        ctl = lambda: sr.eval_cross_table_lookup_checks(vr.EXT, t_z, t_gz, sr.ctl_check_vars([ref_z], [0], a_z, a_gz, nc * 2), cons, cd)  # noqa: E731
        if ctl_first:
            ctl()
        sr.eval_packed_lookups_generic(vr.EXT, [ref_lk], t_z, t_gz, a_z[:nc * 2], a_gz[:nc * 2], ch, cd, cons)
        if not ctl_first:
            ctl()
        return cons.accs
    assert vr.verifier_check(vr.EXT, zeta, n, vanishing(False), q_z, qdf) == [True] * nc
    assert vr.verifier_check(vr.EXT, zeta, n, vanishing(True), q_z, qdf) == [False] * nc


# ------------------------------------------------------------------ 7. errors
def _live_allocs(eng):
    """the emulated runtime counts live allocations; on the GPU the accounting is the trim's return code alone"""
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0
    if not eng.lib.p2hot_is_emulated():
        return None
    eng.lib.p2hot_emu_fault.argtypes = [C.c_char_p, C.c_int]
    eng.lib.p2hot_emu_fault.restype = C.c_int
    return eng.lib.p2hot_emu_fault(b"live_allocs", 0)


def test_errors_leave_nothing_allocated(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns
    from plonky2_amd.starky.cross_table_lookup import marshal_ctl_zs
    from plonky2_amd.starky.lookup import DescriptorTables, lookup_helper_columns, marshal_lookups
    rng = np.random.default_rng(77)
    log_n, W, rate_bits = 4, 10, 1
    n = 1 << log_n
    trace = _rand(rng, W, n)
    dt = DeviceColumns.upload(trace, eng)
    bt = _commit(eng, trace, rate_bits)
    ldesc = _lookup_desc(3, first=2, filt_cols=(7, 8, 9))
    zdesc = _ctl_descs(rng, W)
    ch, alphas = _ints(rng, 2), _ints(rng, 2)
    aux_ok = sr.all_lookup_helper_columns([_ref_lookup(ldesc)], [[int(v) for v in c] for c in trace], ch, 3)
    zs_ref = sr.ctl_data_for_table([[int(v) for v in c] for c in trace], [_ref_z(d) for d in zdesc], 3)
    ba = _commit(eng, aux_ok + sr.get_ctl_auxiliary_polys(zs_ref), rate_bits)
    ba_lookup_only = _commit(eng, aux_ok, rate_bits)
    bt_rate0 = _commit(eng, trace, 0)
    ba_rate0 = _commit(eng, aux_ok + sr.get_ctl_auxiliary_polys(zs_ref), 0)
    keep = []

    def call(which, cd=3, nc=2, mutate=None, lookups=(ldesc,), zds=tuple(zdesc), aux=ba, tr=bt, challenges=ch):
        """which: 'lookup' / 'ctl' / 'quotient'; mutate(tables, lk, cz) edits the marshalled descriptors"""
        tables = DescriptorTables()
        lk = marshal_lookups(tables, [_lib_lookup(d) for d in lookups])
        cz = marshal_ctl_zs(tables, [_lib_z(d) for d in zds])
        if mutate:
            mutate(tables, lk, cz)
        t = tables.struct()
        c, a = np.asarray(challenges, dtype=np.uint64), np.asarray((alphas * 3)[:max(nc, 1)], dtype=np.uint64)
        keep.extend([tables, t, c, a])
        h = C.c_void_p()
        if which == "lookup":
            rc = eng.lib.p2hot_stark_lookup_polys(eng.ctx, dt._h, C.byref(t), lk, len(lookups), c.ctypes.data_as(C.c_void_p), nc, cd, None, C.byref(h))
        elif which == "ctl":
            rc = eng.lib.p2hot_stark_ctl_polys(eng.ctx, dt._h, C.byref(t), cz, len(zds), cd, None, C.byref(h), None)
        else:
            rc = eng.lib.p2hot_stark_quotient_polys(eng.ctx, tr._h, aux._h if aux is not None else None, C.byref(t), lk, len(lookups),
                                                    c.ctypes.data_as(C.c_void_p), cz, len(zds), None, cd, a.ctypes.data_as(C.c_void_p), nc, None, None,
                                                    C.byref(h))
        if rc == _lib.OK:
            eng.lib.p2hot_cols_free(h)
        else:
            assert not h.value and eng.lib.p2hot_last_error(eng.ctx)
        return rc
    assert call("lookup") == _lib.OK and call("ctl") == _lib.OK
    # (qdf = 2 = 2^qbits: all of the coset's coefficients are kept, so even a random witness has chunks)
    assert call("quotient") == _lib.OK
    base = _live_allocs(eng)
    everywhere = ("lookup", "ctl", "quotient")
    # a chunk of three columns: constraint_degree 4 with three looking columns / three looking entries
    for which in everywhere:
        assert call(which, cd=4) == _lib.EUNSUPPORTED, which
    assert call("lookup", cd=4, lookups=(_lookup_desc(2, first=2, filt_cols=(7, 8, 9)),)) == _lib.OK
    # constraint_degree 1: chunks of zero columns
    for which in everywhere:
        assert call(which, cd=1) == _lib.EINVAL, which

    def term_col(tables, lk, cz):
        tables.terms[0] = (W, 0, 1)

    def column_terms(tables, lk, cz):
        tables.columns[0] = (len(tables.terms), 1, 0)

    def filter_constants(tables, lk, cz):
        tables.filters[0] = (0, 0, len(tables.constants), 1)

    def filter_product_id(tables, lk, cz):
        tables.products[0] = (len(tables.columns), 0)

    for which in everywhere:
        for m in (term_col, column_terms, filter_constants, filter_product_id):
            assert call(which, mutate=m) == _lib.EINVAL, (which, m.__name__)

    def lookup_columns(tables, lk, cz):
        lk[0].first_column = len(tables.columns)

    def lookup_no_columns(tables, lk, cz):
        lk[0].num_columns = 0

    def lookup_table_id(tables, lk, cz):
        lk[0].table_column = len(tables.columns)

    def lookup_filter_id(tables, lk, cz):
        lk[0].first_filter = len(tables.filters) - 1

    for which in ("lookup", "quotient"):
        for m in (lookup_columns, lookup_no_columns, lookup_table_id, lookup_filter_id):
            assert call(which, mutate=m) == _lib.EINVAL, (which, m.__name__)
        assert call(which, nc=0) == _lib.EINVAL and call(which, nc=5, challenges=ch * 3) == _lib.EINVAL, which

    def z_looking(tables, lk, cz):
        cz[0].first_looking = len(tables.looking)

    def z_no_looking(tables, lk, cz):
        cz[1].num_looking = 0

    def looking_filter(tables, lk, cz):
        tables.looking[0] = (tables.looking[0][0], tables.looking[0][1], len(tables.filters))

    def looking_columns(tables, lk, cz):
        tables.looking[0] = (len(tables.columns), 1, 0)

    for which in ("ctl", "quotient"):
        for m in (z_looking, z_no_looking, looking_filter, looking_columns):
            assert call(which, mutate=m) == _lib.EINVAL, (which, m.__name__)
    # the quotient alone: the rate, the aux commitment's width
    assert call("quotient", tr=bt_rate0, aux=ba_rate0) == _lib.EINVAL and b"above the rate" in eng.lib.p2hot_last_error(eng.ctx)
    assert call("quotient", aux=ba_lookup_only) == _lib.EINVAL and b"aux commitment" in eng.lib.p2hot_last_error(eng.ctx)
    assert call("quotient", aux=None) == _lib.EINVAL
    assert call("quotient", aux=ba, zds=()) == _lib.EINVAL
    assert call("quotient", aux=ba_rate0) == _lib.EINVAL                                     # another rate
    # a zero denominator: the challenge is -col[0] of a looking column / -(table[0]); gamma = -v of a CTL entry
    tr = [[int(v) for v in c] for c in trace]
    lk_ref = _ref_lookup(ldesc)
    for zero_ch in ((-sr.col_eval_table(lk_ref.columns[1], tr, 0)) % P, (-sr.col_eval_table(lk_ref.table_column, tr, 0)) % P):
        assert call("lookup", challenges=[ch[0], zero_ch]) == _lib.EINVAL
        assert b"Tried to invert zero" in eng.lib.p2hot_last_error(eng.ctx)
    with pytest.raises(ValueError, match="Tried to invert zero"):
        lookup_helper_columns(dt, [_lib_lookup(ldesc)], [(-sr.col_eval_table(lk_ref.columns[0], tr, n - 1)) % P], 3, engine=eng)
    z_ref = _ref_z(zdesc[0])
    v = sr.combine(vr.BASE, z_ref.beta, 0, [sr.col_eval_table(c, tr, 2) for c in z_ref.columns[0]])
    assert call("ctl", zds=(dict(zdesc[0], gamma=(-v) % P),)) == _lib.EINVAL
    assert b"Tried to invert zero" in eng.lib.p2hot_last_error(eng.ctx)
    # a Keccak commitment
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.hash.keccak import KeccakHash
    bk = PolynomialBatch.from_values(trace, rate_bits, False, 0, engine=eng, hasher=KeccakHash(25))
    assert call("quotient", tr=bk) == _lib.EUNSUPPORTED
    del bk
    assert _live_allocs(eng) == base
    assert call("lookup") == _lib.OK and call("ctl") == _lib.OK
