"""Host-side mirror of compute_quotient_polys (starky/src/prover.rs:488-671) for the lookup and cross-table-lookup terms: one
p2hot_stark_quotient_polys call.  The STARK's own constraints (Stark::eval_packed_generic, user code) enter as the caller's
consumer accumulators."""
import ctypes as C

import numpy as np

from .cross_table_lookup import marshal_ctl_zs
from .lookup import P, DescriptorTables, marshal_lookups, raise_reference_panics


def quotient_degree_factor(constraint_degree):
    """starky/src/stark.rs: 1.max(constraint_degree - 1)"""
    return max(1, constraint_degree - 1)


def compute_quotient_polys(trace_commitment, auxiliary_polys_commitment, lookup_challenges, lookups, ctl_zs_columns, alphas,
                           constraint_degree, constraint_accs=None, num_ctl_helper_polys=None, want_values=False, engine=None):
    """trace_commitment / auxiliary_polys_commitment: PolynomialBatches of one engine with the same degree and rate; the second
    (None without lookups and CTLs) holds the lookup columns, the CTL helpers, the CTL Zs.  lookups: [Lookup]; ctl_zs_columns:
    [CtlZData] of this table (or None); num_ctl_helper_polys: CtlData.num_ctl_helper_polys() when it is not what partial_sums
    yields; constraint_accs: [num_challenges][n << qbits] -- ConstraintConsumer::accumulators() after the STARK's own
    constraints -- or None.  Returns DeviceColumns [num_challenges * quotient_degree_factor][n] for PolynomialBatch.from_coeffs
    (and the quotient values [num_challenges][n << qbits] when want_values)."""
    from ..fri.oracle import DeviceColumns
    eng = engine or trace_commitment.engine
    zs = list(ctl_zs_columns or [])
    a = np.ascontiguousarray(np.asarray([int(v) % P for v in alphas], dtype=np.uint64))
    ch = np.ascontiguousarray(np.asarray([int(v) % P for v in (lookup_challenges if lookup_challenges is not None else [])], dtype=np.uint64))
    nc = len(a)
    if lookups and len(ch) != nc:
        raise ValueError("one lookup challenge per alpha (StarkConfig::num_challenges)")
    tables = DescriptorTables()
    lk = marshal_lookups(tables, lookups)
    cz = marshal_ctl_zs(tables, zs)
    nh = None
    if num_ctl_helper_polys is not None:
        nh = (C.c_uint * max(len(zs), 1))(*[int(v) for v in num_ctl_helper_polys])
    qb = max(0, (quotient_degree_factor(constraint_degree) - 1).bit_length())
    m = (1 << trace_commitment.degree_log) << qb
    accs = aptrs = None
    if constraint_accs is not None:
        accs = np.ascontiguousarray(np.asarray(constraint_accs, dtype=np.uint64))
        if accs.shape != (nc, m):
            raise ValueError("constraint_accs must be [num_challenges][n << log2_ceil(quotient_degree_factor)]")
        aptrs = (C.c_void_p * max(nc, 1))(*[accs[c].ctypes.data for c in range(nc)])
    vals = np.zeros((nc, m), dtype=np.uint64) if want_values else None
    h = C.c_void_p()
    t = tables.struct()
    rc = eng.lib.p2hot_stark_quotient_polys(
        eng.ctx, trace_commitment._h, auxiliary_polys_commitment._h if auxiliary_polys_commitment is not None else None, C.byref(t), lk,
        len(lookups), ch.ctypes.data_as(C.c_void_p) if len(ch) else None, cz, len(zs), nh, constraint_degree, a.ctypes.data_as(C.c_void_p), nc,
        aptrs, vals.ctypes.data_as(C.c_void_p) if want_values else None, C.byref(h))
    raise_reference_panics(eng, rc)
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols
