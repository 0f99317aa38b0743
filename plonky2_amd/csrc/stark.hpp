// stark.hpp -- starky's logUp lookups and cross-table lookups on the device: the auxiliary polynomials and their terms of the quotient.
//
// (a) lookup_helper_columns (starky/src/lookup.rs:579-652) and partial_sums (starky/src/cross_table_lookup.rs:383-414).  Both are
// get_helper_cols (lookup.rs:746-789) followed by a running sum, so both are described by the same ZDesc: `num_entries` looking
// entries (columns, filter) under one GrandProductChallenge (a Lookup's column j is the entry ([column j], filter j) with beta = 1,
// gamma = x, lookup.rs:592-607), helper k = sum over the entries of chunk k of filter_e / v_e, v_e = sum_j col_{e,j} beta^j + gamma.
//   helper_rows_kernel   lane = row, blockIdx.y = output helper column: ONE inversion per helper and row, the chunk's sum of
//                        fractions taken as (sum_i f_i prod_{j != i} v_j) / prod_j v_j by lookup.hpp's streamed recurrence
//   increments_kernel    lane = row, blockIdx.y = Z: the row's increment sum_k h_k[i] (a lookup: - freq(i) / (table(i) + x))
//   scan_*_kernel        chunk totals -> carries in one workgroup -> replay (the shape of lookup.hpp's SLDC scan): an exclusive
//                        prefix sum for a lookup's Z (Z[0] = 0, lookup.rs:639-648), an inclusive suffix sum for a CTL's
//                        (cross_table_lookup.rs:395-406)
// Columns and filters are evaluated with eval_table (lookup.rs:119-129, :324-335): the next row of row n - 1 is row 0.
//
// (b) eval_packed_lookups_generic (lookup.rs:804-863) and eval_cross_table_lookup_checks (cross_table_lookup.rs:558-629) on the
// quotient coset of compute_quotient_polys (starky/src/prover.rs:488-671): aux_terms_kernel, below.
#pragma once
#include "../../include/p2hot.h"
#include "gl.hpp"
#include "lookup.hpp"
#include "ntt.hpp"

namespace stark {
using gl::u32;
using gl::u64;

constexpr unsigned SCAN_CHUNK = 4;  // rows per lane of the scan kernels (lookup.hpp's; not measured against other sizes)

// one lookup under one challenge, or one CTL Z.  Column indices are relative to the output / aux matrix the kernel is given
struct ZDesc {
    u32 first_entry, num_entries;  // entries[first_entry ..): the looking (columns, filter) pairs
    u32 num_helpers, helper_col;   // helper columns [helper_col, + num_helpers)
    u32 z_col;
    u32 kind;                      // 0: a lookup (table / frequencies, exclusive prefix), 1: a CTL Z (inclusive suffix)
    u32 table_column, frequencies_column;
    u64 beta, gamma;
};
// output helper column -> (its Z, its chunk).  A CTL Z of one entry has no helper column: its single fraction goes to the Z column
struct HelperMap {
    u32 z, first_entry, num_entries, out_col;
};
// the caller's descriptor arrays (include/p2hot.h) as they lie in one device block, plus what the host derived from them
struct Tables {
    const p2hot_stark_term *terms;
    const p2hot_stark_column *columns;
    const u32 *products, *constants;
    const p2hot_stark_filter *filters;
    const p2hot_stark_looking *entries;
    const ZDesc *zs;
    const HelperMap *hmap;
};

// Column::eval_with_next (lookup.rs:306-321) on a column-major matrix: current-row terms read row `cur`, next-row terms row `nxt`;
// with_next = false is Column::eval (:293-303), which has no next-row terms
__device__ __forceinline__ u64 eval_column(const Tables &t, u32 id, const u64 *m, size_t stride, size_t cur, size_t nxt, bool with_next = true) {
    const p2hot_stark_column c = t.columns[id];
    u64 acc = c.constant;
    for (u32 k = 0; k < c.num_terms; ++k) {
        const p2hot_stark_term tm = t.terms[c.first_term + k];
        if (tm.next && !with_next) continue;
        acc = gl::mul_add(m[(size_t)tm.col * stride + (tm.next ? nxt : cur)], tm.coeff, acc);
    }
    return acc;
}

// Filter::eval_filter (lookup.rs:70-84)
__device__ __forceinline__ u64 eval_filter(const Tables &t, u32 id, const u64 *m, size_t stride, size_t cur, size_t nxt) {
    const p2hot_stark_filter f = t.filters[id];
    u64 acc = 0;
    for (u32 p = 0; p < f.num_products; ++p) {
        const u32 a = t.products[2 * (f.first_product + p)], b = t.products[2 * (f.first_product + p) + 1];
        acc = gl::mul_add(eval_column(t, a, m, stride, cur, nxt), eval_column(t, b, m, stride, cur, nxt), acc);
    }
    for (u32 k = 0; k < f.num_constants; ++k) acc = gl::add(acc, eval_column(t, t.constants[f.first_constant + k], m, stride, cur, nxt));
    return acc;
}

// GrandProductChallenge::combine (lookup.rs:457-464) of an entry's columns: reduce_with_powers(evals, beta) + gamma, Horner from
// the last column
__device__ __forceinline__ u64 combine_entry(const Tables &t, const p2hot_stark_looking e, u64 beta, u64 gamma, const u64 *m, size_t stride,
                                             size_t cur, size_t nxt) {
    u64 acc = 0;
    for (u32 j = e.num_columns; j-- > 0;) acc = gl::mul_add(acc, beta, eval_column(t, e.first_column + j, m, stride, cur, nxt));
    return gl::add(acc, gamma);
}

struct PolyArgs {
    Tables t;
    const u64 *trace;  // [W][n] column-major
    u64 *out;          // [num_out][n]
    size_t n;
    unsigned num_z;
    size_t n_chunks;   // ceil(n / SCAN_CHUNK)
    u64 *csum, *carry; // scratch [num_z][n_chunks]
    unsigned *zero_flag;
};

// lane = row, blockIdx.y = output helper column
__global__ void __launch_bounds__(256) helper_rows_kernel(PolyArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const HelperMap h = a.t.hmap[blockIdx.y];
    const ZDesc z = a.t.zs[h.z];
    const size_t nxt = (i + 1) & (a.n - 1);
    u64 prod = 1, sum = 0;
    for (u32 e = 0; e < h.num_entries; ++e) {
        const p2hot_stark_looking en = a.t.entries[h.first_entry + e];
        const u64 v = combine_entry(a.t, en, z.beta, z.gamma, a.trace, a.n, i, nxt);
        lookup::loo_step(prod, sum, v, eval_filter(a.t, en.filter, a.trace, a.n, i, nxt));
    }
    if (gl::canon(prod) == 0) atomicOr(a.zero_flag, 1u);
    a.out[(size_t)h.out_col * a.n + i] = gl::canon(gl::mul(sum, gl::inv(prod)));
}

// lane = row, blockIdx.y = Z: the Z column receives the row's increment (a CTL Z of one entry holds it already)
__global__ void __launch_bounds__(256) increments_kernel(PolyArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const ZDesc z = a.t.zs[blockIdx.y];
    if (z.num_helpers == 0) return;
    u64 inc = 0;
    for (u32 k = 0; k < z.num_helpers; ++k) inc = gl::add(inc, a.out[(size_t)(z.helper_col + k) * a.n + i]);
    if (z.kind == 0) {
        const size_t nxt = (i + 1) & (a.n - 1);
        const u64 tb = gl::add(eval_column(a.t, z.table_column, a.trace, a.n, i, nxt), z.gamma);
        if (gl::canon(tb) == 0) atomicOr(a.zero_flag, 1u);
        inc = gl::sub(inc, gl::mul(eval_column(a.t, z.frequencies_column, a.trace, a.n, i, nxt), gl::inv(tb)));
    }
    a.out[(size_t)z.z_col * a.n + i] = inc;
}

// the scan runs over positions t = 0 .. n-1: row t of a lookup's Z, row n - 1 - t of a CTL's
__device__ __forceinline__ size_t scan_row(const ZDesc &z, size_t n, size_t t) { return z.kind ? n - 1 - t : t; }

// lane = chunk of SCAN_CHUNK positions, blockIdx.y = Z: the chunk's total
__global__ void __launch_bounds__(64) scan_totals_kernel(PolyArgs a) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_chunks) return;
    const ZDesc z = a.t.zs[blockIdx.y];
    const u64 *col = a.out + (size_t)z.z_col * a.n;
    const size_t t1 = (m + 1) * SCAN_CHUNK < a.n ? (m + 1) * SCAN_CHUNK : a.n;
    u64 sum = 0;
    for (size_t t = m * SCAN_CHUNK; t < t1; ++t) sum = gl::add(sum, col[scan_row(z, a.n, t)]);
    a.csum[(size_t)blockIdx.y * a.n_chunks + m] = sum;
}

// one 1024-thread block per Z, `per` consecutive chunks per thread, Hillis-Steele over the threads: what enters every chunk
__global__ void __launch_bounds__(1024) scan_carries_kernel(PolyArgs a, size_t per) {
    __shared__ u64 ss[1024];
    const unsigned tid = threadIdx.x;
    const u64 *csum = a.csum + (size_t)blockIdx.x * a.n_chunks;
    u64 *carry = a.carry + (size_t)blockIdx.x * a.n_chunks;
    const size_t lo = (size_t)tid * per < a.n_chunks ? (size_t)tid * per : a.n_chunks, hi = lo + per < a.n_chunks ? lo + per : a.n_chunks;
    u64 ls = 0;
    for (size_t m = lo; m < hi; ++m) ls = gl::add(ls, csum[m]);
    ss[tid] = ls;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const u64 f = tid >= d ? ss[tid - d] : 0;
        __syncthreads();
        ss[tid] = gl::add(ss[tid], f);
        __syncthreads();
    }
    u64 c = tid ? ss[tid - 1] : 0;
    for (size_t m = lo; m < hi; ++m) {
        carry[m] = c;
        c = gl::add(c, csum[m]);
    }
}

// lane = chunk, blockIdx.y = Z: the Z values of its positions from the chunk's carry
__global__ void __launch_bounds__(64) scan_emit_kernel(PolyArgs a) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_chunks) return;
    const ZDesc z = a.t.zs[blockIdx.y];
    u64 *col = a.out + (size_t)z.z_col * a.n;
    const size_t t1 = (m + 1) * SCAN_CHUNK < a.n ? (m + 1) * SCAN_CHUNK : a.n;
    u64 acc = a.carry[(size_t)blockIdx.y * a.n_chunks + m];
    for (size_t t = m * SCAN_CHUNK; t < t1; ++t) {
        u64 *q = col + scan_row(z, a.n, t);
        const u64 inc = *q;
        if (z.kind) {
            acc = gl::add(acc, inc);
            *q = gl::canon(acc);
        } else {
            *q = gl::canon(acc);
            acc = gl::add(acc, inc);
        }
    }
}

// ------------------------------------------------------------------ the arguments' share of the quotient
// ConstraintConsumer::constraint is acc <- acc alpha + c (starky/src/constraint_consumer.rs:68-74) and eval_vanishing_poly feeds
// it the STARK's own constraints first, then the lookups', then the CTLs' (starky/src/vanishing_poly.rs): with K library terms
//   value_a(x) = (accs[a][i] alpha_a^K + sum_t c_t alpha_a^(K-1-t)) / Z_H(x)
// where accs is the caller's consumer after Stark::eval_packed_generic alone.  The terms, per ZDesc in order:
//   kind 0 (lookup.rs:835-859)  the helper checks; L_first z; (next_z - z)(t + x) - ((sum h)(t + x) - m), t and m by Column::eval
//   kind 1 (cross_table_lookup.rs:593-627)  the helper checks, then with helpers  L_last (z - sum h), z_last (z - next_z - sum h);
//          without, two entries  L_last (v0 v1 z - f0 v1 - f1 v0), z_last (v0 v1 (z - next_z) - f0 v1 - f1 v0);
//          without, one entry    L_last (v0 z - f0), z_last (v0 (z - next_z) - f0)
//   helper check (lookup.rs:671-692), chunk of two: v1 v0 h - f0 v1 - f1 v0; of one: v0 h - f0
// z_last = x - w_n^-1; L_first(x) = Z_H(x) / (n (x - 1)) and L_last(x) = Z_H(x) / (n (w_n x - 1)): the values of the selector LDEs
// of prover.rs:526-529.  w_n x is the coset's point i + 2^qbits, so both come from the one table quotient_perm_kernel uses.
// lane = row L of the LDE matrices, indexed as plonk::quotient_perm_kernel does (i = bitrev(L), next row bitrev(i + 2^qbits mod Nq)).
struct TermArgs {
    Tables t;
    const u64 *trace, *aux;  // LDE matrices, element (col, L) at col * stride + L
    size_t trace_stride, aux_stride;
    const u64 *apow;       // device [nc][K + 1]: alpha_a^(K-1-t) at t < K, alpha_a^K at K (wave-uniform)
    const u64 *zh;         // device [2 << qbits]: Z_H(g w^i) for i mod 2^qbits, then their inverses
    const u64 *inv_nx1;    // device [Nq], committed order: 1 / (n (x_L - 1))  (plonk::quot_inv_kernel)
    const u64 *accs;       // device [nc][Nq] natural order, or null
    u64 *out;              // device [nc][Nq] natural order
    unsigned num_z, K, chunk, log_nq, qbits;
    u64 last;              // w_n^-1
    ntt::RootTable roots;
};

template <int NC>
__global__ void __launch_bounds__(256) aux_terms_kernel(TermArgs q) {
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const size_t i_next = (i + ((size_t)1 << q.qbits)) & (nq - 1);
    const size_t L_next = q.log_nq ? (size_t)(__brevll((unsigned long long)i_next) >> (64 - q.log_nq)) : 0;
    const u64 x = gl::mul(gl::COSET_SHIFT, q.log_nq ? ntt::root_pow(q.roots, (u32)(i << (32 - q.log_nq))) : (u64)1);
    const size_t r = i & (((size_t)1 << q.qbits) - 1);
    const u64 l_first = gl::mul(q.zh[r], q.inv_nx1[L]), l_last = gl::mul(q.zh[r], q.inv_nx1[L_next]), z_last = gl::sub(x, q.last);
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    unsigned t = 0;
    auto put = [&](u64 term) {
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(term, q.apow[(size_t)a * (q.K + 1) + t], res[a]);
        ++t;
    };
    auto entry = [&](const ZDesc &z, u32 e, u64 &v, u64 &f) {
        const p2hot_stark_looking en = q.t.entries[z.first_entry + e];
        v = combine_entry(q.t, en, z.beta, z.gamma, q.trace, q.trace_stride, L, L_next);
        f = eval_filter(q.t, en.filter, q.trace, q.trace_stride, L, L_next);
    };
    for (unsigned zi = 0; zi < q.num_z; ++zi) {
        const ZDesc z = q.t.zs[zi];
        u64 hsum = 0;
        for (u32 k = 0; k < z.num_helpers; ++k) {
            const u64 h = q.aux[(size_t)(z.helper_col + k) * q.aux_stride + L];
            hsum = gl::add(hsum, h);
            u64 v0, f0;
            entry(z, k * q.chunk, v0, f0);
            if (k * q.chunk + 1 < z.num_entries && q.chunk > 1) {
                u64 v1, f1;
                entry(z, k * q.chunk + 1, v1, f1);
                put(gl::sub(gl::sub(gl::mul(gl::mul(v1, v0), h), gl::mul(f0, v1)), gl::mul(f1, v0)));
            } else {
                put(gl::sub(gl::mul(v0, h), f0));
            }
        }
        const u64 zl = q.aux[(size_t)z.z_col * q.aux_stride + L], zn = q.aux[(size_t)z.z_col * q.aux_stride + L_next];
        if (z.kind == 0) {
            const u64 tb = gl::add(eval_column(q.t, z.table_column, q.trace, q.trace_stride, L, L_next, false), z.gamma);
            const u64 y = gl::sub(gl::mul(hsum, tb), eval_column(q.t, z.frequencies_column, q.trace, q.trace_stride, L, L_next, false));
            put(gl::mul(zl, l_first));
            put(gl::sub(gl::mul(gl::sub(zn, zl), tb), y));
        } else if (z.num_helpers) {
            put(gl::mul(gl::sub(zl, hsum), l_last));
            put(gl::mul(gl::sub(gl::sub(zl, zn), hsum), z_last));
        } else if (z.num_entries > 1) {
            u64 v0, f0, v1, f1;
            entry(z, 0, v0, f0);
            entry(z, 1, v1, f1);
            const u64 vv = gl::mul(v0, v1), ff = gl::mul_add(f1, v0, gl::mul(f0, v1));
            put(gl::mul(gl::sub(gl::mul(vv, zl), ff), l_last));
            put(gl::mul(gl::sub(gl::mul(vv, gl::sub(zl, zn)), ff), z_last));
        } else {
            u64 v0, f0;
            entry(z, 0, v0, f0);
            put(gl::mul(gl::sub(gl::mul(v0, zl), f0), l_last));
            put(gl::mul(gl::sub(gl::mul(v0, gl::sub(zl, zn)), f0), z_last));
        }
    }
    const u64 zinv = q.zh[((size_t)1 << q.qbits) + r];
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 s = res[a];
        if (q.accs) s = gl::mul_add(q.apow[(size_t)a * (q.K + 1) + q.K], q.accs[(size_t)a * nq + i], s);
        q.out[(size_t)a * nq + i] = gl::canon(gl::mul(s, zinv));
    }
}

}  // namespace stark
