// lookup.hpp -- the lookup argument on the device: the RE / partial SLDC polynomials and the lookup terms of the quotient.
//
// (a) compute_lookup_polys (plonky2/src/plonk/prover.rs:458-574).  Per LUT the reference walks [last_lu_row, first_lut_row]
// from the top row down.  With, on a LookupTableGate row, combo_X(s) = inp_s + X * out_s (wires 3s, 3s+1; multiplicity 3s+2) and,
// on a LookupGate row, combo_A(s) = inp_s + A * out_s (wires 2s, 2s+1):
//   RE[row]        = RE[row+1] * delta^num_lut_slots + horner_delta(combo_B(0..))               (LUT rows only)
//   SLDC_p[row]    = SLDC_last[row+1] + sum_{k <= p} group_k(row),
//   group_k(row)   = + sum_{s in LUT group k} mult_s / (alpha - combo_A(s))   on LUT rows (groups of lut_degree slots)
//                    - sum_{s in LU group k}  1 / (alpha - combo_A(s))        on LU rows  (groups of lookup_degree slots)
// so the row walk is an affine suffix scan (RE) and a suffix sum (SLDC) over per-row quantities: lane = row computes them
// (lookup_rows_kernel), then chunk totals -> carries in one workgroup -> replay, the shape of plonk.hpp's partial products.
// A group's sum of inverses is taken as  (sum_i m_i prod_{j != i} d_j) / prod_j d_j  with ONE inversion per group; the
// numerator streams:  S <- S d + m P,  P <- P d  (P the prefix product: O(d), no per-slot storage).  Field arithmetic is exact, so
// the values equal the reference's batch_multiplicative_inverse route bit for bit once canonical.  A zero alpha - combo makes the
// reference panic ("Tried to invert zero"); here it raises a flag -> P2HOT_EINVAL.
//
// (b) check_lookup_constraints_batch (plonk/vanishing_poly.rs:515-664) on the quotient coset: lookup_terms_kernel, below.
#pragma once
#include "gl.hpp"
#include "ntt.hpp"

namespace lookup {
using gl::u32;
using gl::u64;

constexpr unsigned SCAN_CHUNK = 4;  // rows per lane of the scan kernels

// one (d, m) factor of a group: S <- S d + m P, P <- P d
__device__ __forceinline__ void loo_step(u64 &prod, u64 &sum, u64 d, u64 m) {
    sum = gl::mul_add(m, prod, gl::mul(sum, d));
    prod = gl::mul(prod, d);
}
// ... with m = 1 (the LDC side)
__device__ __forceinline__ void loo_step1(u64 &prod, u64 &sum, u64 d) {
    sum = gl::mul_add(sum, d, prod);
    prod = gl::mul(prod, d);
}

struct PolyArgs {
    const u64 *wires;  // [>= max(2 num_lu_slots, 3 num_lut_slots)][n] column-major
    size_t wires_stride;
    u64 *out;          // [nc][S + 1][n]: RE, SLDC_0 .. SLDC_{S-1} of challenge 0, 1, ...
    size_t out_stride;
    unsigned num_lu_slots, num_lut_slots, lu_degree, lut_degree, S;
    size_t last_lu, last_lut, first_lut;  // one LUT's rows (LookupWire, plonk/circuit_data.rs)
    u64 deltas[4][4];   // per challenge: A, B, Alpha, Delta (canonical)
    u64 delta_pow[4];   // Delta^num_lut_slots
    size_t n_chunks;    // ceil(len / SCAN_CHUNK), len = first_lut - last_lu + 1
    u64 *csum, *cmul, *cadd;      // scratch [nc][n_chunks]: chunk totals (SLDC sum; RE as x -> x * cmul + cadd)
    u64 *carry_s, *carry_re;      // scratch [nc][n_chunks]
    unsigned *zero_flag;
};

// lane = row of the region (t = first_lut - row), blockIdx.y = challenge: out[1 + p][row] = sum_{k <= p} group_k(row),
// out[0][row] = horner_delta(combo_B) on LUT rows (both without what the rows above carry in)
__global__ void __launch_bounds__(256) lookup_rows_kernel(PolyArgs a) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t len = a.first_lut - a.last_lu + 1;
    if (t >= len) return;
    const unsigned c = blockIdx.y;
    const size_t row = a.first_lut - t;
    const u64 dA = a.deltas[c][0], dB = a.deltas[c][1], alpha = a.deltas[c][2], delta = a.deltas[c][3];
    u64 *out = a.out + (size_t)c * (a.S + 1) * a.out_stride + row;
    const u64 *w = a.wires + row;
    u64 acc = 0;
    bool zero = false;
    if (row >= a.last_lut) {
        u64 h = 0;
        for (unsigned p = 0; p < a.S; ++p) {
            const unsigned s0 = p * a.lut_degree, s1 = s0 + a.lut_degree < a.num_lut_slots ? s0 + a.lut_degree : a.num_lut_slots;
            u64 prod = 1, sum = 0;
            for (unsigned s = s0; s < s1; ++s) {
                const u64 inp = w[(size_t)(3 * s) * a.wires_stride], ou = w[(size_t)(3 * s + 1) * a.wires_stride];
                const u64 m = w[(size_t)(3 * s + 2) * a.wires_stride];
                h = gl::add(gl::mul(h, delta), gl::mul_add(dB, ou, inp));
                loo_step(prod, sum, gl::sub(alpha, gl::mul_add(dA, ou, inp)), m);
            }
            if (s0 < s1) {
                if (gl::canon(prod) == 0) zero = true;
                acc = gl::mul_add(sum, gl::inv(prod), acc);
            }
            out[(size_t)(1 + p) * a.out_stride] = acc;
        }
        out[0] = h;
    } else {
        for (unsigned p = 0; p < a.S; ++p) {
            const unsigned s0 = p * a.lu_degree, s1 = s0 + a.lu_degree < a.num_lu_slots ? s0 + a.lu_degree : a.num_lu_slots;
            u64 prod = 1, sum = 0;
            for (unsigned s = s0; s < s1; ++s) {
                const u64 inp = w[(size_t)(2 * s) * a.wires_stride], ou = w[(size_t)(2 * s + 1) * a.wires_stride];
                loo_step1(prod, sum, gl::sub(alpha, gl::mul_add(dA, ou, inp)));
            }
            if (s0 < s1) {
                if (gl::canon(prod) == 0) zero = true;
                acc = gl::sub(acc, gl::mul(sum, gl::inv(prod)));
            }
            out[(size_t)(1 + p) * a.out_stride] = acc;
        }
    }
    if (zero) atomicOr(a.zero_flag, 1u);
}

// lane = chunk of SCAN_CHUNK rows (walking down from first_lut): the sum of its rows' totals, and its RE rows as one affine map
__global__ void __launch_bounds__(64) lookup_chunk_totals_kernel(PolyArgs a) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_chunks) return;
    const unsigned c = blockIdx.y;
    const size_t len = a.first_lut - a.last_lu + 1, len_lut = a.first_lut - a.last_lut + 1;
    const u64 *out = a.out + (size_t)c * (a.S + 1) * a.out_stride;
    const u64 D = a.delta_pow[c];
    u64 sum = 0, mu = 1, ad = 0;
    const size_t t1 = (m + 1) * SCAN_CHUNK < len ? (m + 1) * SCAN_CHUNK : len;
    for (size_t t = m * SCAN_CHUNK; t < t1; ++t) {
        const size_t row = a.first_lut - t;
        sum = gl::add(sum, out[(size_t)a.S * a.out_stride + row]);
        if (t < len_lut) {
            ad = gl::mul_add(ad, D, out[row]);
            mu = gl::mul(mu, D);
        }
    }
    a.csum[(size_t)c * a.n_chunks + m] = sum;
    a.cmul[(size_t)c * a.n_chunks + m] = mu;
    a.cadd[(size_t)c * a.n_chunks + m] = ad;
}

// what enters every chunk: the reference reads values[row + 1] AS IT IS when the region is processed (prover.rs:517, :528, :561),
// so the seeds are the buffer's row first_lut + 1 -- zero, or what an earlier region left there.  One 1024-thread block per
// challenge, `per` consecutive chunks per thread, Hillis-Steele over the threads (sums; affine maps composed left to right)
__global__ void __launch_bounds__(1024) lookup_carries_kernel(PolyArgs a, size_t per) {
    __shared__ u64 ss[1024], sm[1024], sa[1024];
    const unsigned tid = threadIdx.x, c = blockIdx.x;
    const u64 *out = a.out + (size_t)c * (a.S + 1) * a.out_stride;
    const u64 *csum = a.csum + (size_t)c * a.n_chunks, *cmul = a.cmul + (size_t)c * a.n_chunks, *cadd = a.cadd + (size_t)c * a.n_chunks;
    const size_t lo = (size_t)tid * per < a.n_chunks ? (size_t)tid * per : a.n_chunks, hi = lo + per < a.n_chunks ? lo + per : a.n_chunks;
    u64 ls = 0, lm = 1, la = 0;
    for (size_t m = lo; m < hi; ++m) {
        ls = gl::add(ls, csum[m]);
        la = gl::mul_add(la, cmul[m], cadd[m]);
        lm = gl::mul(lm, cmul[m]);
    }
    ss[tid] = ls, sm[tid] = lm, sa[tid] = la;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        u64 fs = 0, fm = 1, fa = 0;
        if (tid >= d) fs = ss[tid - d], fm = sm[tid - d], fa = sa[tid - d];
        __syncthreads();
        // (earlier threads first): x -> (x fm + fa) sm + sa
        const u64 ns = gl::add(ss[tid], fs), na = gl::mul_add(fa, sm[tid], sa[tid]), nm = gl::mul(fm, sm[tid]);
        ss[tid] = ns, sm[tid] = nm, sa[tid] = na;
        __syncthreads();
    }
    const u64 seed_s = out[(size_t)a.S * a.out_stride + a.first_lut + 1], seed_re = out[a.first_lut + 1];
    u64 cs = tid ? gl::add(seed_s, ss[tid - 1]) : seed_s;
    u64 cr = tid ? gl::mul_add(seed_re, sm[tid - 1], sa[tid - 1]) : seed_re;
    for (size_t m = lo; m < hi; ++m) {
        a.carry_s[(size_t)c * a.n_chunks + m] = cs;
        a.carry_re[(size_t)c * a.n_chunks + m] = cr;
        cs = gl::add(cs, csum[m]);
        cr = gl::mul_add(cr, cmul[m], cadd[m]);
    }
}

// lane = chunk: the polynomials' values for its rows from the chunk's carries
__global__ void __launch_bounds__(64) lookup_emit_kernel(PolyArgs a) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_chunks) return;
    const unsigned c = blockIdx.y;
    const size_t len = a.first_lut - a.last_lu + 1, len_lut = a.first_lut - a.last_lut + 1;
    u64 *out = a.out + (size_t)c * (a.S + 1) * a.out_stride;
    const u64 D = a.delta_pow[c];
    u64 acc = a.carry_s[(size_t)c * a.n_chunks + m], re = a.carry_re[(size_t)c * a.n_chunks + m];
    const size_t t1 = (m + 1) * SCAN_CHUNK < len ? (m + 1) * SCAN_CHUNK : len;
    for (size_t t = m * SCAN_CHUNK; t < t1; ++t) {
        const size_t row = a.first_lut - t;
        u64 last = 0;
        for (unsigned p = 0; p < a.S; ++p) {
            u64 *q = out + (size_t)(1 + p) * a.out_stride + row;
            last = *q;
            *q = gl::canon(gl::add(last, acc));
        }
        acc = gl::add(acc, last);
        if (t < len_lut) {
            re = gl::mul_add(re, D, out[row]);
            out[row] = gl::canon(re);
        }
    }
}

// ------------------------------------------------------------------ the lookup argument's share of the quotient
// eval_vanishing_poly_base_batch puts check_lookup_constraints_batch's terms (vanishing_poly.rs:515-664) of challenge 0, 1, ...
// between the partial-product terms and the gate terms (vanishing_poly.rs:317-322).  Per challenge c, Kc = 4 + num_luts + 2 S terms:
//   0  LastLdc * sldc[S-1]      1  InitSre * sldc[0]      2  InitSre * z_re      3 + r  end_r * (z_re - lut_re_poly_evals[c][r])
//   3 + num_luts  TransSre * (z_re - horner(next_z_re, combo_B, delta))
//   4 + num_luts + 2 p      TransSre * (lut_prod_p (sldc[p] - prev_p) - sum_i mult_i prod_{j != i} (alpha - combo_A(j)))      (LUT group p)
//   4 + num_luts + 2 p + 1  TransLdc * (lu_prod_p  (sldc[p] - prev_p) + sum_i prod_{j != i} (alpha - combo_A(j)))             (LU group p)
// with prev_0 = next row's sldc[S-1], prev_p = sldc[p-1].  The leave-one-out sums stream as in loo_step (the reference's are
// O(d^2)).  This kernel writes  lookup_sums[a][i] = sum_t term_t alpha_a^t + alpha_a^(nc Kc) gate_sums[a][i]  (in place over
// gate_sums when given), which the unchanged quotient_perm_kernel takes as ITS gate_sums behind the permutation terms.
// lane = row L of the LDE matrices, indexed as quotient_perm_kernel does (i = bitrev(L), next row bitrev(i + 2^qbits mod Nq)).
struct TermArgs {
    const u64 *wires, *sel, *lz;  // LDE matrices, element (col, L) at col * stride + L; sel -> the TransSre column, lz -> challenge 0's RE
    size_t wires_stride, sel_stride, lz_stride;
    const u64 *apow;       // device [nc][nc * Kc + 1]: alpha_a^t (wave-uniform)
    const u64 *lut_evals;  // device [nc][num_luts]
    const u64 *gate_sums;  // device [nc][Nq] natural order, or null
    u64 *out;              // device [nc][Nq] natural order (may alias gate_sums)
    unsigned num_lu_slots, num_lut_slots, lu_degree, lut_degree, S, num_luts, log_nq, qbits;
    u64 deltas[4][4];
};

template <int NC>
__global__ void __launch_bounds__(256) lookup_terms_kernel(TermArgs q) {
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const size_t i_next = (i + ((size_t)1 << q.qbits)) & (nq - 1);
    const size_t L_next = q.log_nq ? (size_t)(__brevll((unsigned long long)i_next) >> (64 - q.log_nq)) : 0;
    const unsigned Kc = 4 + q.num_luts + 2 * q.S, K = NC * Kc, S = q.S;
    const u64 trans_sre = q.sel[L], trans_ldc = q.sel[q.sel_stride + L], init_sre = q.sel[2 * q.sel_stride + L], last_ldc = q.sel[3 * q.sel_stride + L];
    u64 res[NC], z_re[NC], cur[NC], prev[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    auto put = [&](unsigned t, u64 term) {  // term t of the whole list
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(term, q.apow[(size_t)a * (K + 1) + t], res[a]);
    };
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const u64 *lz = q.lz + (size_t)c * (S + 1) * q.lz_stride;
        z_re[c] = lz[L];
        cur[c] = lz[L_next];                              // next_z_re: the start of the RE transition's Horner
        prev[c] = lz[(size_t)S * q.lz_stride + L_next];   // the last SLDC of the next row
        const u64 sldc0 = lz[q.lz_stride + L], sldc_last = lz[(size_t)S * q.lz_stride + L];
        put(c * Kc, gl::mul(last_ldc, sldc_last));
        put(c * Kc + 1, gl::mul(init_sre, sldc0));
        put(c * Kc + 2, gl::mul(init_sre, z_re[c]));
        for (unsigned r = 0; r < q.num_luts; ++r)
            put(c * Kc + 3 + r, gl::mul(q.sel[(size_t)(4 + r) * q.sel_stride + L], gl::sub(z_re[c], q.lut_evals[(size_t)c * q.num_luts + r])));
    }
    for (unsigned p = 0; p < S; ++p) {
        u64 lup[NC], lus[NC], ltp[NC], lts[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) lup[c] = ltp[c] = 1, lus[c] = lts[c] = 0;
        const unsigned u0 = p * q.lu_degree, u1 = u0 + q.lu_degree < q.num_lu_slots ? u0 + q.lu_degree : q.num_lu_slots;
        for (unsigned s = u0; s < u1; ++s) {
            const u64 inp = q.wires[(size_t)(2 * s) * q.wires_stride + L], ou = q.wires[(size_t)(2 * s + 1) * q.wires_stride + L];
#pragma unroll
            for (int c = 0; c < NC; ++c) loo_step1(lup[c], lus[c], gl::sub(q.deltas[c][2], gl::mul_add(q.deltas[c][0], ou, inp)));
        }
        const unsigned t0 = p * q.lut_degree, t1 = t0 + q.lut_degree < q.num_lut_slots ? t0 + q.lut_degree : q.num_lut_slots;
        for (unsigned s = t0; s < t1; ++s) {
            const u64 inp = q.wires[(size_t)(3 * s) * q.wires_stride + L], ou = q.wires[(size_t)(3 * s + 1) * q.wires_stride + L];
            const u64 m = q.wires[(size_t)(3 * s + 2) * q.wires_stride + L];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                cur[c] = gl::add(gl::mul(cur[c], q.deltas[c][3]), gl::mul_add(q.deltas[c][1], ou, inp));
                loo_step(ltp[c], lts[c], gl::sub(q.deltas[c][2], gl::mul_add(q.deltas[c][0], ou, inp)), m);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const u64 z = q.lz[((size_t)c * (S + 1) + 1 + p) * q.lz_stride + L];
            const u64 diff = gl::sub(z, prev[c]);
            prev[c] = z;
            put(c * Kc + 4 + q.num_luts + 2 * p, gl::mul(trans_sre, gl::sub(gl::mul(ltp[c], diff), lts[c])));
            put(c * Kc + 4 + q.num_luts + 2 * p + 1, gl::mul(trans_ldc, gl::mul_add(lup[c], diff, lus[c])));
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) put(c * Kc + 3 + q.num_luts, gl::mul(trans_sre, gl::sub(z_re[c], cur[c])));
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 s = res[a];
        if (q.gate_sums) s = gl::mul_add(q.apow[(size_t)a * (K + 1) + K], q.gate_sums[(size_t)a * nq + i], s);
        q.out[(size_t)a * nq + i] = gl::canon(s);
    }
}

}  // namespace lookup
