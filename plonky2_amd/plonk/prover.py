"""Host-side mirror of the gate-independent pieces of plonky2/src/plonk/prover.rs that sit next to the commit path
(SURVEY 8f-3): the permutation argument's partial products / Z polynomials, computed on the GPU from device-resident
wire and sigma columns and handed straight to PolynomialBatch.from_values."""
import ctypes as C

import numpy as np

from ..engine import default_engine


def num_partial_products(n, max_degree):
    """plonky2/src/util/partial_products.rs:40-47"""
    return -(-n // max_degree) - 1


def all_wires_permutation_partial_products(wires, sigmas, k_is, quotient_degree_factor, betas, gammas, engine=None):
    """all_wires_permutation_partial_products (prover.rs:356-390) followed by the batch ordering of prover.rs:224-229.

    wires, sigmas: [num_routed][n] column-major -- MatrixWitness.wire_values[col][row] and the sigma polynomials' values
    on the subgroup -- as host ndarrays / DeviceColumns (the host-pointer entry point p2hot_partial_products, what the
    Rust shim calls; returns DeviceColumns) or as device buffers (p2hot_partial_products_dev; returns a device buffer).
    Result [nc * (num_prods + 1)][n]: the Z of every challenge first, then the partial products of challenge 0, 1, ...
    (`zs_partial_products`)."""
    from ..fri.oracle import DeviceColumns
    eng = engine or default_engine()
    if not (eng.mem.is_buffer(wires) and eng.mem.is_buffer(sigmas)):
        for x in (wires, sigmas):
            if not isinstance(x, DeviceColumns) and (np.ndim(x) != 2 or np.shape(x)[1] & (np.shape(x)[1] - 1)):
                raise ValueError("wires and sigmas must be [num_routed][n] with n a power of two")
        dw = wires if isinstance(wires, DeviceColumns) else DeviceColumns.upload(eng.host(wires), eng)
        ds = sigmas if isinstance(sigmas, DeviceColumns) else DeviceColumns.upload(eng.host(sigmas), eng)
        k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
        if dw.degree_log != ds.degree_log or dw.width < len(k) or ds.width < len(k):
            raise ValueError("wires and sigmas must both be [num_routed][n]")
        if not quotient_degree_factor < len(k):  # prover.rs:215-218
            raise ValueError("quotient_degree_factor must be smaller than the number of routed wires")
        b = np.ascontiguousarray(np.asarray(betas, dtype=np.uint64))
        g = np.ascontiguousarray(np.asarray(gammas, dtype=np.uint64))
        if b.shape != g.shape or b.ndim != 1:
            raise ValueError("betas and gammas must be equally long vectors")
        h = C.c_void_p()
        eng.check(eng.lib.p2hot_partial_products(eng.ctx, dw._h, 0, ds._h, 0, k.ctypes.data_as(C.c_void_p), len(k),
                                                 quotient_degree_factor, b.ctypes.data_as(C.c_void_p),
                                                 g.ctypes.data_as(C.c_void_p), len(b), None, C.byref(h)))
        return DeviceColumns(eng, h)
    d_w, d_s = eng.dev(wires), eng.dev(sigmas)
    if d_w.ndim != 2 or d_s.shape != d_w.shape:
        raise ValueError("wires and sigmas must both be [num_routed][n]")
    r, n = d_w.shape
    log_n = int(n).bit_length() - 1
    if n != 1 << log_n:
        raise ValueError("row count must be a power of two")
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    if k.shape != (r,):
        raise ValueError("k_is must have one shift per routed wire")
    b = np.ascontiguousarray(np.asarray(betas, dtype=np.uint64))
    g = np.ascontiguousarray(np.asarray(gammas, dtype=np.uint64))
    if b.shape != g.shape or b.ndim != 1:
        raise ValueError("betas and gammas must be equally long vectors")
    nc = b.shape[0]
    # prover.rs:215-218: "When the number of routed wires is smaller that the degree, we should change the logic"
    if not quotient_degree_factor < r:
        raise ValueError("quotient_degree_factor must be smaller than the number of routed wires")
    num_prods = num_partial_products(r, quotient_degree_factor)
    out = eng.mem.empty(nc * (num_prods + 1), n)
    eng.check(eng.lib.p2hot_partial_products_dev(eng.ctx, eng.ptr(d_w), n, eng.ptr(d_s), n, k.ctypes.data_as(C.c_void_p), r,
                                                 log_n, quotient_degree_factor, b.ctypes.data_as(C.c_void_p),
                                                 g.ctypes.data_as(C.c_void_p), nc, eng.ptr(out), n))
    return out


def partial_products_and_zs_commitment(wires, sigmas, k_is, quotient_degree_factor, betas, gammas, rate_bits, cap_height,
                                       engine=None):
    """prover.rs:219-247 without lookups: compute partial products + Zs and commit to them (from_values, no blinding)."""
    from ..fri.oracle import PolynomialBatch
    eng = engine or default_engine()
    zs_pp = all_wires_permutation_partial_products(wires, sigmas, k_is, quotient_degree_factor, betas, gammas, eng)
    return PolynomialBatch.from_values(zs_pp, rate_bits, False, cap_height, engine=eng)


def quotient_poly_chunks(quotient_values, degree_bits, quotient_degree_factor, engine=None):
    """The gate-independent tail of the quotient computation (prover.rs:274-289, :810-815): the quotient polynomials
    arrive as values on the coset g*H of size n << ceil(log2(quotient_degree_factor)) (one row per challenge, natural
    order), are interpolated with coset_ifft, trimmed to quotient_degree_factor * n coefficients (the reference panics
    with "Quotient has failed, the vanishing polynomial is not divisible by Z_H" if the tail is not zero) and split
    into quotient_degree_factor chunks of n coefficients.  Returns DeviceColumns
    [num_challenges * quotient_degree_factor][n] ready for PolynomialBatch.from_coeffs."""
    from ..fri.oracle import DeviceColumns
    eng = engine or default_engine()
    # one p2hot_quotient_chunks call (the Rust shim's path: compute_quotient_polys leaves host Vecs)
    q = np.ascontiguousarray(eng.host(quotient_values))
    if q.ndim != 2:
        raise ValueError("expected [num_challenges][n << quotient_degree_bits]")
    qb = max(0, (quotient_degree_factor - 1).bit_length())
    if q.shape[1] != (1 << degree_bits) << qb:
        raise ValueError("quotient values must live on the coset of size n << ceil(log2(quotient_degree_factor))")
    ptrs = (C.c_void_p * max(q.shape[0], 1))(*[q[c].ctypes.data for c in range(q.shape[0])])
    h = C.c_void_p()
    rc = eng.lib.p2hot_quotient_chunks(eng.ctx, ptrs, q.shape[0], degree_bits, quotient_degree_factor, C.byref(h))
    if rc == 1 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (polynomial/mod.rs:164-178)
    eng.check(rc)
    return DeviceColumns(eng, h)


def compute_quotient_polys(wires_commitment, constants_sigmas_commitment, sigmas_first_col, zs_partial_products_commitment, k_is,
                           quotient_degree_factor, betas, gammas, alphas, gate_sums=None, want_values=False, engine=None):
    """compute_quotient_polys (prover.rs:609-815) without its gate evaluation -- one p2hot_quotient_polys call: the permutation
    argument's vanishing terms (vanishing_poly.rs:167-330) on the quotient coset from the three commitments' device-resident LDE
    matrices, plus `gate_sums` (the caller's reduce_with_powers of the gate constraint terms, [num_challenges][n << qbits], or
    None), over Z_H, then coset_ifft / trim / chunks.  Returns DeviceColumns [num_challenges * quotient_degree_factor][n] for
    PolynomialBatch.from_coeffs (and the quotient values [num_challenges][n << qbits] when want_values)."""
    from ..fri.oracle import DeviceColumns
    eng = engine or wires_commitment.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g, a = (np.ascontiguousarray(np.asarray(v, dtype=np.uint64)) for v in (betas, gammas, alphas))
    if not (b.shape == g.shape == a.shape and b.ndim == 1):
        raise ValueError("betas, gammas and alphas must be equally long vectors")
    nc = len(b)
    qb = max(0, (quotient_degree_factor - 1).bit_length())
    m = (1 << wires_commitment.degree_log) << qb
    gs = None
    if gate_sums is not None:
        gs = np.ascontiguousarray(np.asarray(gate_sums, dtype=np.uint64))
        if gs.shape != (nc, m):
            raise ValueError("gate_sums must be [num_challenges][n << ceil(log2(quotient_degree_factor))]")
    gptrs = (C.c_void_p * nc)(*[gs[c].ctypes.data for c in range(nc)]) if gs is not None else None
    vals = np.zeros((nc, m), dtype=np.uint64) if want_values else None
    h = C.c_void_p()
    rc = eng.lib.p2hot_quotient_polys(eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col,
                                      zs_partial_products_commitment._h, k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor,
                                      b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), nc, gptrs,
                                      vals.ctypes.data_as(C.c_void_p) if want_values else None, C.byref(h))
    if rc == 1 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (polynomial/mod.rs:164-178)
    eng.check(rc)
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols


# ------------------------------------------------------------------ the lookup argument
def num_sldc_polys(num_lu_slots, lookup_degree):
    """prover.rs:471 / vanishing_poly.rs:527: the partial SLDC polynomials of one challenge"""
    return -(-num_lu_slots // lookup_degree)


def concat_columns(a, b, engine=None):
    """p2hot_cols_concat: a's columns then b's as new DeviceColumns (the Zs / partial products ++ the lookup polynomials of
    prover.rs:237-241, for one PolynomialBatch.from_values); a and b stay valid"""
    from ..fri.oracle import DeviceColumns
    eng = engine or a.engine
    h = C.c_void_p()
    eng.check(eng.lib.p2hot_cols_concat(eng.ctx, a._h, b._h, C.byref(h)))
    return DeviceColumns(eng, h)


def all_lookup_polys(wires, lookup_rows, deltas, num_lu_slots, num_lut_slots, lookup_degree, want_host=False, engine=None):
    """compute_all_lookup_polys (prover.rs:451-605) -- one p2hot_lookup_polys call.

    wires: [>= max(2 num_lu_slots, 3 num_lut_slots)][n] wire columns (host ndarray or DeviceColumns); lookup_rows: per LUT
    (last_lu_gate, last_lut_gate, first_lut_gate) in prover_data.lookup_rows order; deltas: [num_challenges][4] = A, B, Alpha,
    Delta; lookup_degree = max_quotient_degree_factor - 1.  Returns DeviceColumns [num_challenges * (S + 1)][n]: RE and the S
    partial SLDC polynomials of challenge 0, 1, ... (and the same as a host array when want_host).  A zero alpha - combination
    raises ValueError("Tried to invert zero"), where the reference panics."""
    from ..fri.oracle import DeviceColumns
    eng = engine or default_engine()
    dw = wires if isinstance(wires, DeviceColumns) else DeviceColumns.upload(eng.host(wires), eng)
    rows = np.ascontiguousarray(np.asarray(lookup_rows, dtype=np.uint64).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(deltas, dtype=np.uint64))
    if d.ndim != 2 or d.shape[1] != 4:
        raise ValueError("deltas must be [num_challenges][4]")
    nc = d.shape[0]
    out = None
    if want_host and lookup_degree > 0 and 1 <= nc <= 4:
        out = np.zeros((nc * (num_sldc_polys(num_lu_slots, lookup_degree) + 1), 1 << dw.degree_log), dtype=np.uint64)
    h = C.c_void_p()
    rc = eng.lib.p2hot_lookup_polys(eng.ctx, dw._h, 0, num_lu_slots, num_lut_slots, lookup_degree, rows.ctypes.data_as(C.c_void_p),
                                    len(rows), d.ctypes.data_as(C.c_void_p), nc, out.ctypes.data_as(C.c_void_p) if out is not None else None,
                                    C.byref(h))
    if rc == 1 and b"Tried to invert zero" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (field/src/types.rs:133)
    eng.check(rc)
    cols = DeviceColumns(eng, h)
    return (cols, out) if want_host else cols


def compute_quotient_polys_lookup(wires_commitment, constants_sigmas_commitment, sigmas_first_col, zs_partial_products_lookups_commitment,
                                  k_is, quotient_degree_factor, betas, gammas, alphas, num_lu_slots, num_lut_slots,
                                  lookup_selectors_first_col, deltas, lut_re_poly_evals, gate_sums=None, want_values=False, engine=None):
    """compute_quotient_polys (prover.rs:609-815) of a circuit with lookup tables -- one p2hot_quotient_polys_lookup call:
    compute_quotient_polys above plus the terms of check_lookup_constraints_batch (vanishing_poly.rs:515-664) between the
    partial-product terms and the gate terms.  The third commitment holds the Zs, the partial products and the lookup polynomials
    (all_lookup_polys' order); the 4 + num_luts lookup selectors are columns lookup_selectors_first_col .. of constants_sigmas;
    deltas [num_challenges][4]; lut_re_poly_evals [num_challenges][num_luts] = get_lut_poly(..).eval(delta).  Returns as
    compute_quotient_polys does."""
    from ..fri.oracle import DeviceColumns
    eng = engine or wires_commitment.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g, a = (np.ascontiguousarray(np.asarray(v, dtype=np.uint64)) for v in (betas, gammas, alphas))
    if not (b.shape == g.shape == a.shape and b.ndim == 1):
        raise ValueError("betas, gammas and alphas must be equally long vectors")
    nc = len(b)
    d = np.ascontiguousarray(np.asarray(deltas, dtype=np.uint64))
    ev = np.ascontiguousarray(np.asarray(lut_re_poly_evals, dtype=np.uint64).reshape(nc, -1))
    if d.shape != (nc, 4):
        raise ValueError("deltas must be [num_challenges][4]")
    qb = max(0, (quotient_degree_factor - 1).bit_length())
    m = (1 << wires_commitment.degree_log) << qb
    gs = None
    if gate_sums is not None:
        gs = np.ascontiguousarray(np.asarray(gate_sums, dtype=np.uint64))
        if gs.shape != (nc, m):
            raise ValueError("gate_sums must be [num_challenges][n << ceil(log2(quotient_degree_factor))]")
    gptrs = (C.c_void_p * max(nc, 1))(*[gs[c].ctypes.data for c in range(nc)]) if gs is not None else None
    vals = np.zeros((nc, m), dtype=np.uint64) if want_values else None
    h = C.c_void_p()
    rc = eng.lib.p2hot_quotient_polys_lookup(
        eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, zs_partial_products_lookups_commitment._h,
        k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
        a.ctypes.data_as(C.c_void_p), nc, gptrs, num_lu_slots, num_lut_slots, ev.shape[1], lookup_selectors_first_col,
        d.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p) if want_values else None, C.byref(h))
    if rc == 1 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (polynomial/mod.rs:164-178)
    eng.check(rc)
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols


# ------------------------------------------------------------------ the standard gates' constraints
GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_ARITHMETIC_EXT, GATE_MUL_EXT, GATE_BASE_SUM, GATE_POSEIDON = range(8)
# the gates a recursive verifier circuit adds (the header's second enum)
GATE_POSEIDON_MDS, GATE_REDUCING, GATE_REDUCING_EXT, GATE_RANDOM_ACCESS, GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION = range(16, 22)


class _P2hotGate(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("kind", "row", "selector_index", "group_first", "group_end", "param0", "param1")]


class _P2hotGateSet(C.Structure):
    _fields_ = [("gates", C.POINTER(_P2hotGate)), ("num_gates", C.c_uint32), ("num_selectors", C.c_uint32),
                ("num_lookup_selectors", C.c_uint32), ("public_inputs_hash", C.c_uint64 * 4)]


class GateSet:
    """p2hot_gate_set (include/p2hot.h): the gates of common_data.gates the library evaluates on the device.

    gates: (kind, row, selector_index, group_first, group_end, param0, param1) per gate -- row = the gate's index in
    common_data.gates, [group_first, group_end) = selectors_info.groups[selector_index], param0 = num_consts / num_ops /
    num_limbs, param1 = BaseSum's base.  The recursion kinds: Reducing / ReducingExtension param0 = num_coeffs; Exponentiation
    param0 = num_power_bits; RandomAccess param0 = num_copies, param1 = bits | num_extra_constants << 8; CosetInterpolation
    param0 = subgroup_bits, param1 = degree; PoseidonMds takes none.  num_selectors = selectors_info.num_selectors(); num_lookup_selectors = 4 + num_luts of
    a circuit with lookup tables, else 0; public_inputs_hash: four field elements."""

    def __init__(self, gates, num_selectors, num_lookup_selectors=0, public_inputs_hash=(0, 0, 0, 0)):
        gates = [tuple(int(v) for v in g) for g in gates]
        if any(len(g) != 7 for g in gates) or len(public_inputs_hash) != 4:
            raise ValueError("a gate is (kind, row, selector_index, group_first, group_end, param0, param1); the hash has 4 words")
        self._array = (_P2hotGate * max(len(gates), 1))(*[_P2hotGate(*g) for g in gates])
        self._set = _P2hotGateSet(C.cast(self._array, C.POINTER(_P2hotGate)), len(gates), num_selectors, num_lookup_selectors,
                                  (C.c_uint64 * 4)(*[int(v) for v in public_inputs_hash]))
        self.gates = gates

    @property
    def ptr(self):
        return C.cast(C.pointer(self._set), C.c_void_p)


def gate_sums(wires_commitment, constants_sigmas_commitment, sigmas_first_col, gate_set, quotient_degree_factor, alphas, engine=None,
              programs=None):
    """evaluate_gate_constraints_base_batch (vanishing_poly.rs:702-728) for the gates of `gate_set` on the quotient coset, reduced
    by the powers of every alpha -- one p2hot_gate_sums call.  Returns [num_challenges][n << qbits], natural order, canonical.
    `programs`: a list of gate_program.GateProgram, the user-defined gates of the circuit (one p2hot_gate_sums_programs call)."""
    eng = engine or wires_commitment.engine
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.uint64))
    qb = max(0, (quotient_degree_factor - 1).bit_length())
    out = np.zeros((len(a), (1 << wires_commitment.degree_log) << qb), dtype=np.uint64)
    if programs is not None:
        from .gate_program import marshal
        parr, pn, _keep = marshal(programs)
        eng.check(eng.lib.p2hot_gate_sums_programs(eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, gate_set.ptr,
                                                   quotient_degree_factor, a.ctypes.data_as(C.c_void_p), len(a), out.ctypes.data_as(C.c_void_p),
                                                   parr, pn))
        return out
    eng.check(eng.lib.p2hot_gate_sums(eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, gate_set.ptr,
                                      quotient_degree_factor, a.ctypes.data_as(C.c_void_p), len(a), out.ctypes.data_as(C.c_void_p)))
    return out


def _quotient_call(eng, call, nc, m, want_values):
    vals = np.zeros((nc, m), dtype=np.uint64) if want_values else None
    h = C.c_void_p()
    rc = call(vals.ctypes.data_as(C.c_void_p) if want_values else None, C.byref(h))
    if rc == 1 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (polynomial/mod.rs:164-178)
    eng.check(rc)
    from ..fri.oracle import DeviceColumns
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols


def _host_gate_sums(gate_sums, nc, m):
    if gate_sums is None:
        return None, None
    gs = np.ascontiguousarray(np.asarray(gate_sums, dtype=np.uint64))
    if gs.shape != (nc, m):
        raise ValueError("gate_sums must be [num_challenges][n << ceil(log2(quotient_degree_factor))]")
    return gs, (C.c_void_p * max(nc, 1))(*[gs[c].ctypes.data for c in range(nc)])


def compute_quotient_polys_gates(wires_commitment, constants_sigmas_commitment, sigmas_first_col, zs_partial_products_commitment, k_is,
                                 quotient_degree_factor, betas, gammas, alphas, gate_set, gate_sums=None, want_values=False, engine=None,
                                 programs=None):
    """compute_quotient_polys above with the gates of `gate_set` evaluated on the device (one p2hot_quotient_polys_gates call);
    `gate_sums`, if given, is the caller's residual of the other gates and is added to the device's sums.  `programs`: a list of
    gate_program.GateProgram evaluated on the device beside the set (one p2hot_quotient_polys_gate_programs call)."""
    eng = engine or wires_commitment.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g, a = (np.ascontiguousarray(np.asarray(v, dtype=np.uint64)) for v in (betas, gammas, alphas))
    if not (b.shape == g.shape == a.shape and b.ndim == 1):
        raise ValueError("betas, gammas and alphas must be equally long vectors")
    nc = len(b)
    m = (1 << wires_commitment.degree_log) << max(0, (quotient_degree_factor - 1).bit_length())
    gs, gptrs = _host_gate_sums(gate_sums, nc, m)
    if programs is not None:
        from .gate_program import marshal
        parr, pn, _keep = marshal(programs)
        return _quotient_call(eng, lambda vals, h: eng.lib.p2hot_quotient_polys_gate_programs(
            eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, zs_partial_products_commitment._h,
            k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
            a.ctypes.data_as(C.c_void_p), nc, gptrs, gate_set.ptr, vals, h, parr, pn), nc, m, want_values)
    return _quotient_call(eng, lambda vals, h: eng.lib.p2hot_quotient_polys_gates(
        eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, zs_partial_products_commitment._h,
        k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
        a.ctypes.data_as(C.c_void_p), nc, gptrs, gate_set.ptr, vals, h), nc, m, want_values)


# ------------------------------------------------------------------ M witnesses of one circuit (include/p2hot.h, the *_many section)
def _per_proof(v, M, what):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.uint64))
    if a.ndim != 2 or a.shape[0] != M:
        raise ValueError("%s must be [M][num_challenges]" % what)
    return a


def all_wires_permutation_partial_products_many(wires_commitments, sigmas, k_is, quotient_degree_factor, betas, gammas, want_host=False,
                                                engine=None):
    """all_wires_permutation_partial_products for M witnesses of one circuit -- one p2hot_partial_products_many call.
    wires_commitments: the M wires batches (their routed columns are the first len(k_is)); sigmas: DeviceColumns shared by all
    proofs; betas / gammas [M][num_challenges].  Returns DeviceColumns of rows * M interleaved columns (column e of proof m is
    column e * M + m) for commit_columns_many, and with want_host also the host array [M][rows][n].  A zero denominator raises
    ValueError naming the proof."""
    from ..fri.oracle import DeviceColumns, _handles
    M = len(wires_commitments)
    eng = engine or sigmas.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g = _per_proof(betas, M, "betas"), _per_proof(gammas, M, "gammas")
    if b.shape != g.shape:
        raise ValueError("betas and gammas must have one shape")
    nc = b.shape[1]
    out = None
    if want_host and M:
        rows = nc * (num_partial_products(len(k), quotient_degree_factor) + 1)
        out = np.zeros((M, rows, 1 << sigmas.degree_log), dtype=np.uint64)
    h = C.c_void_p()
    rc = eng.lib.p2hot_partial_products_many(eng.ctx, M, _handles(wires_commitments), 0, sigmas._h, 0, k.ctypes.data_as(C.c_void_p), len(k),
                                             quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), nc,
                                             out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(h))
    if rc == 1 and b"tried to invert zero" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (field/src/types.rs:133)
    eng.check(rc)
    cols = DeviceColumns(eng, h)
    return (cols, out) if want_host else cols


def commit_columns_many(cols, M, rate_bits, cap_height, is_values, engine=None):
    """p2hot_commit_cols_many: the interleaved DeviceColumns of a *_many call -> M PolynomialBatch sharing their blocks"""
    from ..fri.oracle import PolynomialBatch
    return PolynomialBatch.from_device_columns_many(cols, M, rate_bits, cap_height, is_values, engine=engine)


def compute_quotient_polys_gates_many(wires_commitments, constants_sigmas_commitment, sigmas_first_col, zs_partial_products_commitments,
                                      k_is, quotient_degree_factor, betas, gammas, alphas, gate_set=None, public_inputs_hashes=None,
                                      want_values=False, want_chunks=True, engine=None):
    """compute_quotient_polys_gates for M witnesses of one circuit -- one p2hot_quotient_polys_gates_many call.  betas / gammas /
    alphas [M][num_challenges]; public_inputs_hashes [M][4] or None (the set's for every proof); gate_set None: permutation terms
    only.  Returns the chunks as interleaved DeviceColumns (nc * quotient_degree_factor * M columns) for commit_columns_many, the
    values [M][nc][n << qbits] with want_values (alone with want_chunks=False).  "Quotient has failed" raises ValueError naming
    the proof."""
    from ..fri.oracle import DeviceColumns, _handles
    M = len(wires_commitments)
    eng = engine or constants_sigmas_commitment.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g, a = _per_proof(betas, M, "betas"), _per_proof(gammas, M, "gammas"), _per_proof(alphas, M, "alphas")
    if not b.shape == g.shape == a.shape:
        raise ValueError("betas, gammas and alphas must have one shape")
    nc = b.shape[1]
    pih = None
    if public_inputs_hashes is not None:
        pih = np.ascontiguousarray(np.asarray(public_inputs_hashes, dtype=np.uint64))
        if pih.shape != (M, 4):
            raise ValueError("public_inputs_hashes must be [M][4]")
    m = (1 << constants_sigmas_commitment.degree_log) << max(0, (quotient_degree_factor - 1).bit_length())
    vals = np.zeros((M, nc, m), dtype=np.uint64) if want_values else None
    h = C.c_void_p()
    rc = eng.lib.p2hot_quotient_polys_gates_many(
        eng.ctx, M, _handles(wires_commitments), constants_sigmas_commitment._h, sigmas_first_col, _handles(zs_partial_products_commitments),
        k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
        a.ctypes.data_as(C.c_void_p), nc, gate_set.ptr if gate_set is not None else None,
        pih.ctypes.data_as(C.c_void_p) if pih is not None else None, vals.ctypes.data_as(C.c_void_p) if want_values else None,
        C.byref(h) if want_chunks else None)
    if rc == 1 and b"Quotient has failed" in eng.lib.p2hot_last_error(eng._ctx):
        raise ValueError(eng.lib.p2hot_last_error(eng._ctx).decode())  # the reference panics (polynomial/mod.rs:164-178)
    eng.check(rc)
    if not want_chunks:
        return vals
    cols = DeviceColumns(eng, h)
    return (cols, vals) if want_values else cols


def compute_quotient_polys_lookup_gates(wires_commitment, constants_sigmas_commitment, sigmas_first_col,
                                        zs_partial_products_lookups_commitment, k_is, quotient_degree_factor, betas, gammas, alphas,
                                        num_lu_slots, num_lut_slots, lookup_selectors_first_col, deltas, lut_re_poly_evals, gate_set,
                                        gate_sums=None, want_values=False, engine=None, programs=None):
    """compute_quotient_polys_lookup above with the gates of `gate_set` evaluated on the device (one
    p2hot_quotient_polys_lookup_gates call); `gate_sums` is the caller's residual of the other gates.  `programs`: a list of
    gate_program.GateProgram evaluated beside the set (one p2hot_quotient_polys_lookup_gate_programs call)."""
    eng = engine or wires_commitment.engine
    k = np.ascontiguousarray(np.asarray(k_is, dtype=np.uint64))
    b, g, a = (np.ascontiguousarray(np.asarray(v, dtype=np.uint64)) for v in (betas, gammas, alphas))
    if not (b.shape == g.shape == a.shape and b.ndim == 1):
        raise ValueError("betas, gammas and alphas must be equally long vectors")
    nc = len(b)
    d = np.ascontiguousarray(np.asarray(deltas, dtype=np.uint64))
    ev = np.ascontiguousarray(np.asarray(lut_re_poly_evals, dtype=np.uint64).reshape(nc, -1))
    if d.shape != (nc, 4):
        raise ValueError("deltas must be [num_challenges][4]")
    m = (1 << wires_commitment.degree_log) << max(0, (quotient_degree_factor - 1).bit_length())
    gs, gptrs = _host_gate_sums(gate_sums, nc, m)
    if programs is not None:
        from .gate_program import marshal
        parr, pn, _keep = marshal(programs)
        return _quotient_call(eng, lambda vals, h: eng.lib.p2hot_quotient_polys_lookup_gate_programs(
            eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, zs_partial_products_lookups_commitment._h,
            k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
            a.ctypes.data_as(C.c_void_p), nc, gptrs, num_lu_slots, num_lut_slots, ev.shape[1], lookup_selectors_first_col,
            d.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), gate_set.ptr, vals, h, parr, pn), nc, m, want_values)
    return _quotient_call(eng, lambda vals, h: eng.lib.p2hot_quotient_polys_lookup_gates(
        eng.ctx, wires_commitment._h, constants_sigmas_commitment._h, sigmas_first_col, zs_partial_products_lookups_commitment._h,
        k.ctypes.data_as(C.c_void_p), len(k), quotient_degree_factor, b.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
        a.ctypes.data_as(C.c_void_p), nc, gptrs, num_lu_slots, num_lut_slots, ev.shape[1], lookup_selectors_first_col,
        d.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), gate_set.ptr, vals, h), nc, m, want_values)
