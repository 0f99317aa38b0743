"""Host-side mirror of compute_quotient_polys (starky/src/prover.rs:488-671) for the lookup and cross-table-lookup terms: one
p2hot_stark_quotient_polys call.  The STARK's own constraints (Stark::eval_packed_generic, user code) enter as a constraint
program (starky/air.py; one p2hot_stark_quotient_polys_air call, nothing of the trace crosses to the host) or as the caller's
consumer accumulators."""
import ctypes as C

import numpy as np

from .cross_table_lookup import marshal_ctl_zs
from .lookup import P, DescriptorTables, marshal_lookups, raise_reference_panics


def quotient_degree_factor(constraint_degree):
    """starky/src/stark.rs: 1.max(constraint_degree - 1)"""
    return max(1, constraint_degree - 1)


def _program(air):
    """an air.Program, or an AirBuilder that is built here"""
    return air.build() if hasattr(air, "build") else air


def _publics(prog, public_inputs):
    pub = np.ascontiguousarray(np.asarray([int(v) % P for v in (public_inputs if public_inputs is not None else [])], dtype=np.uint64))
    if len(pub) != prog.num_publics:
        raise ValueError("the program names %d public inputs, %d given" % (prog.num_publics, len(pub)))
    return pub


def constraint_accs(trace_commitment, air, public_inputs, alphas, constraint_degree, engine=None):
    """ConstraintConsumer::accumulators() after the STARK's own constraints (`air`: an air.Program or AirBuilder) at every point
    of the quotient coset: [num_challenges][n << qbits], natural order -- one p2hot_stark_constraint_accs call"""
    eng = engine or trace_commitment.engine
    prog = _program(air)
    pub = _publics(prog, public_inputs)
    a = np.ascontiguousarray(np.asarray([int(v) % P for v in alphas], dtype=np.uint64))
    qb = max(0, (quotient_degree_factor(constraint_degree) - 1).bit_length())
    out = np.zeros((len(a), (1 << trace_commitment.degree_log) << qb), dtype=np.uint64)
    ps = prog.struct()
    rc = eng.lib.p2hot_stark_constraint_accs(eng.ctx, trace_commitment._h, C.byref(ps), pub.ctypes.data_as(C.c_void_p) if len(pub) else None,
                                             constraint_degree, a.ctypes.data_as(C.c_void_p), len(a), out.ctypes.data_as(C.c_void_p))
    eng.check(rc)
    return out


def compute_quotient_polys(trace_commitment, auxiliary_polys_commitment, lookup_challenges, lookups, ctl_zs_columns, alphas,
                           constraint_degree, constraint_accs=None, num_ctl_helper_polys=None, want_values=False, engine=None,
                           air=None, public_inputs=None):
    """trace_commitment / auxiliary_polys_commitment: PolynomialBatches of one engine with the same degree and rate; the second
    (None without lookups and CTLs) holds the lookup columns, the CTL helpers, the CTL Zs.  lookups: [Lookup]; ctl_zs_columns:
    [CtlZData] of this table (or None); num_ctl_helper_polys: CtlData.num_ctl_helper_polys() when it is not what partial_sums
    yields; constraint_accs: [num_challenges][n << qbits] -- ConstraintConsumer::accumulators() after the STARK's own
    constraints -- or None; air: the same constraints as an air.Program or AirBuilder, with their public_inputs (not both: a
    ValueError).  Returns DeviceColumns [num_challenges * quotient_degree_factor][n] for PolynomialBatch.from_coeffs
    (and the quotient values [num_challenges][n << qbits] when want_values)."""
    from ..fri.oracle import DeviceColumns
    eng = engine or trace_commitment.engine
    if air is not None and constraint_accs is not None:
        raise ValueError("the STARK's constraints come as a program (air) or as accumulators (constraint_accs), not both")
    if air is None and public_inputs is not None:
        raise ValueError("public_inputs belong to a constraint program (air)")
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
    common = (eng.ctx, trace_commitment._h, auxiliary_polys_commitment._h if auxiliary_polys_commitment is not None else None, C.byref(t), lk,
              len(lookups), ch.ctypes.data_as(C.c_void_p) if len(ch) else None, cz, len(zs), nh, constraint_degree, a.ctypes.data_as(C.c_void_p), nc)
    out = (vals.ctypes.data_as(C.c_void_p) if want_values else None, C.byref(h))
    if air is not None:
        prog = _program(air)
        pub = _publics(prog, public_inputs)
        ps = prog.struct()
        rc = eng.lib.p2hot_stark_quotient_polys_air(*common, C.byref(ps), pub.ctypes.data_as(C.c_void_p) if len(pub) else None, *out)
    else:
        rc = eng.lib.p2hot_stark_quotient_polys(*common, aptrs, *out)
    raise_reference_panics(eng, rc)
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols
