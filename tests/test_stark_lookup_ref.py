"""tests/stark_lookup_ref.py on its own: the restatement of starky's lookup.rs / cross_table_lookup.rs has the properties the
reference's arguments rest on -- a satisfied lookup closes, the looking and looked CTL sums agree, every constraint vanishes on H,
and the streamed leave-one-out sum the kernels use is the plain one.  Nothing here touches the library."""
import numpy as np
import pytest

from tests import stark_lookup_ref as sr
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import root_of_unity
from tests.test_stark_lookup import _ctl_instance, _ints, _ref_lookup, _ref_z, _satisfied_lookup_trace


@pytest.mark.parametrize("num_looking,constraint_degree", [(1, 2), (2, 3), (3, 3), (5, 2)])
def test_ref_lookup_closes_and_vanishes_on_h(num_looking, constraint_degree):
    """on a satisfied witness Z[n-1] + (sum h - m g)[n-1] = 0, every lookup constraint vanishes on every row of H (L_first / L_last
    the indicators of row 0 / n - 1, z_last = w^i - w^(n-1)); one wrong frequency breaks the first"""
    rng = np.random.default_rng(100 + num_looking)
    log_n = 4
    n = 1 << log_n
    trace, desc = _satisfied_lookup_trace(rng, log_n, num_looking)
    lk, ch = _ref_lookup(desc), _ints(rng, 2)
    cols = sr.all_lookup_helper_columns([lk], trace, ch, constraint_degree)
    nh = sr.num_helper_columns(lk, constraint_degree)
    assert len(cols) == 2 * nh
    for k, x in enumerate(ch):
        mine = cols[k * nh:(k + 1) * nh]
        assert mine[-1][0] == 0
        assert (mine[-1][n - 1] + sr.lookup_last_increment(lk, trace, x, constraint_degree, mine)) % P == 0
    w = root_of_unity(log_n)
    for i in range(n):
        local, nxt = [t[i] for t in trace], [t[(i + 1) % n] for t in trace]
        cons = sr.ConstraintConsumer(vr.BASE, [3], (pow(w, i, P) - pow(w, n - 1, P)) % P, int(i == 0), int(i == n - 1))
        sr.eval_packed_lookups_generic(vr.BASE, [lk], local, nxt, [c[i] for c in cols], [c[(i + 1) % n] for c in cols], ch, constraint_degree, cons)
        assert len(cons.terms) == 2 * (nh + 1) and not any(cons.terms), i
    trace[1][3] = (trace[1][3] + 1) % P
    bad = sr.lookup_helper_columns(lk, trace, ch[0], constraint_degree)
    assert (bad[-1][n - 1] + sr.lookup_last_increment(lk, trace, ch[0], constraint_degree, bad)) % P != 0


@pytest.mark.parametrize("constraint_degree", [2, 3])
def test_ref_ctl_sums_agree_and_vanish_on_h(constraint_degree):
    """the looking Zs' Z[0] sum to the looked table's Z[0] (verify_cross_table_lookups); every CTL constraint vanishes on H"""
    rng = np.random.default_rng(7)
    log_n = 4
    n = 1 << log_n
    trace, looking, looked = _ctl_instance(rng, log_n)
    zs = sr.ctl_data_for_table(trace, [_ref_z(looking), _ref_z(looked)], constraint_degree)
    assert len(zs[0].helper_columns) == (2 if constraint_degree == 2 else 1) and zs[1].helper_columns == []
    assert zs[0].z[0] == zs[1].z[0] != 0
    aux = sr.get_ctl_auxiliary_polys(zs)
    nh = [len(z.helper_columns) for z in zs]
    w = root_of_unity(log_n)
    for i in range(n):
        local, nxt = [t[i] for t in trace], [t[(i + 1) % n] for t in trace]
        cons = sr.ConstraintConsumer(vr.BASE, [3], (pow(w, i, P) - pow(w, n - 1, P)) % P, int(i == 0), int(i == n - 1))
        sr.eval_cross_table_lookup_checks(vr.BASE, local, nxt, sr.ctl_check_vars(zs, nh, [c[i] for c in aux], [c[(i + 1) % n] for c in aux], 0), cons,
                                          constraint_degree)
        assert len(cons.terms) == sum(nh) + 4 and not any(cons.terms), i


def test_ref_leave_one_out_sum_is_the_streamed_one():
    """sum_i f_i / d_i = (sum_i f_i prod_{j != i} d_j) / prod_j d_j with the numerator by S <- S d + f P, P <- P d (the kernels)"""
    rng = np.random.default_rng(1)
    for cnt in (1, 2, 5):
        d, f = _ints(rng, cnt), _ints(rng, cnt)
        plain = sum(fi * sr.inv(di) for fi, di in zip(f, d)) % P
        prod, s = 1, 0
        for di, fi in zip(d, f):
            s, prod = (s * di + fi * prod) % P, prod * di % P
        assert s * sr.inv(prod) % P == plain
