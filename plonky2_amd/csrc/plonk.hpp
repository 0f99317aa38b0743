// plonk.hpp -- the permutation argument's partial products and Z polynomials on the device.
//
// Replaces wires_permutation_partial_products_and_zs (plonky2/src/plonk/prover.rs:392-449) with its helpers
// quotient_chunk_products / partial_products_and_z_gx (plonky2/src/util/partial_products.rs:13-39).  Per row i of
// the trace (x_i = w_n^i, prover_data.subgroup) and routed wire j the reference forms
//   num_j = wire + beta * k_j * x_i + gamma,   den_j = wire + beta * sigma_j(x_i) + gamma,
// multiplies num_j / den_j over chunks of `degree` wires, and walks the rows SEQUENTIALLY:
//   pp_p(x_i) = Z(x_i) * prod_{c <= p} chunk_c(i)   (p < num_prods),   Z(x_{i+1}) = Z(x_i) * prod_c chunk_c(i),  Z(x_0) = 1.
// Here the row walk is an exclusive prefix PRODUCT scan (chunk totals -> carries in one workgroup -> replay), and
// the per-row work is lane-parallel with one field inversion per row: with PN_c / PD_c the prefix products of the
// chunk numerators / denominators, prod_{k <= c} chunk_k = PN_c * PD_c^-1 and PD_{c-1}^-1 = PD_c^-1 * D_c
// (Montgomery's trick run backwards over the chunks).  Field arithmetic is exact, so the values equal the
// reference's element-wise batch_multiplicative_inverse route (field/src/types.rs:133) bit for bit once canonical.
// A zero denominator makes the reference panic ("Tried to invert zero"); here it raises a flag -> P2HOT_EINVAL.
#pragma once
#include "gl_mul3.hpp"
#include "gl.hpp"
#include "ntt.hpp"

namespace plonk {
using gl::u32;
using gl::u64;

struct PPArgs {
    const u64 *wires, *sigmas;  // [num_routed][n] column-major (element (j, i) at j * stride + i)
    size_t wires_stride, sigmas_stride;
    const u64 *k_is;            // device, [num_routed] coset shifts (common_data.k_is)
    unsigned num_routed, degree, num_chunks, log_n;
    u64 beta, gamma;
    ntt::RootTable roots;       // forward table: x_i = w_n^i
    u64 *pp;                    // [num_chunks - 1][n] (stride pp_stride): prefix quotients, later the partial products
    size_t pp_stride;
    u64 *dchunk;                // scratch [num_chunks][n]: chunk denominators
    u64 *total;                 // scratch [n]: T_i = prod over all chunks of row i
    unsigned *zero_flag;
};

// lane = row: prefix quotients Q_c(i) = prod_{k <= c} chunk_k(i) for c < num_chunks - 1, and T_i = Q_last(i)
__global__ void __launch_bounds__(256) pp_quotients_kernel(PPArgs a) {
#include "kbody_pp_quotients.hpp"
}

// Both challenges of a plonky2 config in ONE pass over the wires and sigmas, all multiplications as gl_mul3.hpp streams (the
// additions ride the multiply-adds), the two Fermat inversions as two interleaved streams: the same results as two
// pp_quotients_kernel launches at less than half their instructions (the compiler's 64-bit multiply-reduce costs ~34 here).
struct PPArgs2 {
    PPArgs c[2];  // wires / sigmas / k_is / sizes / roots are taken from c[0]
};
__global__ void __launch_bounds__(256) pp_quotients2_kernel(PPArgs2 aa) {
    const PPArgs &a = aa.c[0], &b = aa.c[1];
#include "kbody_pp_quotients2.hpp"
}

// ------------------------------------------------------------------ M witnesses of one circuit (p2hot_partial_products_many, p2hot_quotient_polys_gates_many)
// What differs between the proofs of one call, one entry per proof in device memory.  A kernel's M-form takes the shared arguments
// by value as its single-proof form does, runs one grid row (blockIdx.y) per proof and takes the per-proof fields from
// tab[blockIdx.y]: the index is wave-uniform and the table read-only, so these are scalar loads into SGPRs, where the single-proof
// form finds its kernel arguments.  Z_H and the 1 / (n (x - 1)) table depend on the sizes only and stay shared.
// The kernels' bodies are the kbody_*.hpp fragments, #included by both forms: the single-proof kernels keep their tokens and with
// them their code.
// (A pointer read from the table would have no known address space and cost flat loads: the table holds each block's OFFSET in
// words from proof 0's block, which the kernel has as an argument.)
struct ManyProof {
    ptrdiff_t wires_off, zs_off, coef_off;  // this proof's wires / Zs LDE matrices and wires coefficients, from proof 0's
    size_t wires_stride, zs_stride, coef_stride;
    u64 betas[4], gammas[4], alphas[4];          // as the single-proof arguments carry them (gammas canonical)
    u64 base[4][4], alpha_k[4];                  // QuotArgs' tables for this proof's alphas
};

// the routed wires' coefficients of every proof into one block [M][num_routed][n] (grid: rows, routed wire, proof), for one forward NTT
__global__ void __launch_bounds__(256) many_gather_coeffs_kernel(const u64 *coef0, const ManyProof *__restrict__ tab, size_t first_col, size_t n,
                                                                 u64 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ManyProof &t = tab[blockIdx.z];
    out[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * n + i] = (coef0 + t.coef_off)[(first_col + blockIdx.y) * t.coef_stride + i];
}

// pp_quotients_kernel / pp_quotients2_kernel for proof blockIdx.y: the shared PPArgs describe proof 0's blocks, proof y's lie
// `wires_step` (the gathered values), n (a column of the interleaved output; the row totals) and num_chunks * n (the chunk
// denominators) further per proof; challenge `ch` of the proof's own (beta, gamma); one zero-denominator flag word per proof
__device__ __forceinline__ void many_patch(PPArgs &a, const ManyProof &t, unsigned ch, size_t wires_step) {
    const size_t y = blockIdx.y, n = (size_t)1 << a.log_n;
    a.wires += y * wires_step;
    a.beta = t.betas[ch], a.gamma = t.gammas[ch];
    a.pp += y * n, a.dchunk += y * a.num_chunks * n, a.total += y * n, a.zero_flag += y;
}
__global__ void __launch_bounds__(256) pp_quotients_many_kernel(PPArgs a, const ManyProof *__restrict__ tab, unsigned ch, size_t wires_step) {
    many_patch(a, tab[blockIdx.y], ch, wires_step);
#include "kbody_pp_quotients.hpp"
}
__global__ void __launch_bounds__(256) pp_quotients2_many_kernel(PPArgs2 aa, const ManyProof *__restrict__ tab, unsigned ch, size_t wires_step) {
    PPArgs &a = aa.c[0], &b = aa.c[1];
    many_patch(a, tab[blockIdx.y], ch, wires_step);
    many_patch(b, tab[blockIdx.y], ch + 1, wires_step);
#include "kbody_pp_quotients2.hpp"
}

// lane = chunk of 2^chunk_log rows: its product
__global__ void pp_chunk_totals_kernel(const u64 *total, unsigned chunk_log, size_t n_chunks, u64 *prod) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    u64 acc = 1;
    const size_t base = m << chunk_log;
    for (size_t i = 0; i < ((size_t)1 << chunk_log); ++i) acc = gl::mul(acc, total[base + i]);
    prod[m] = acc;
}

// carry[m] = prod_{m' < m} P[m'] (exclusive prefix product); one 1024-thread block, `per` consecutive chunks per thread
__global__ void __launch_bounds__(1024) pp_carries_kernel(const u64 *prod, size_t n_chunks, size_t per, u64 *carry) {
#include "kbody_pp_carries.hpp"
}
// one scan per proof: workgroup y scans proof y's n_chunks chunk products.  (The chunk totals, the Z walk and the scaling need no
// M-form: with the proofs' rows back to back they are the single-proof kernels over M * n rows -- only the carries restart.)
__global__ void __launch_bounds__(1024) pp_carries_many_kernel(const u64 *prod, size_t n_chunks, size_t per, u64 *carry) {
    prod += (size_t)blockIdx.y * n_chunks, carry += (size_t)blockIdx.y * n_chunks;
#include "kbody_pp_carries.hpp"
}

// lane = chunk: Z(x_i) for its rows from the chunk's carry (Z(x_0) = 1)
__global__ void pp_emit_z_kernel(const u64 *total, unsigned chunk_log, size_t n_chunks, const u64 *carry, u64 *z) {
    const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    u64 acc = carry[m];
    const size_t base = m << chunk_log;
    for (size_t i = 0; i < ((size_t)1 << chunk_log); ++i) {
        z[base + i] = gl::canon(acc);
        acc = gl::mul(acc, total[base + i]);
    }
}

// lane = row: pp_p(x_i) = Z(x_i) * Q_p(i)
__global__ void pp_scale_kernel(u64 *pp, size_t pp_stride, unsigned num_prods, const u64 *z, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 zi = z[i];
    for (unsigned p = 0; p < num_prods; ++p) {
        u64 *q = pp + (size_t)p * pp_stride + i;
        *q = gl::canon(gl::mul(*q, zi));
    }
}

// trim_to_len's divisibility check (field/src/polynomial/mod.rs:164-178): raises *flag when any of v[0..count) is nonzero
__global__ void any_nonzero_kernel(const u64 *v, size_t count, unsigned *flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && gl::canon(v[i]) != 0) atomicOr(flag, 1u);
}

// the divisibility check for M proofs: polynomial (proof z, challenge y) is column z * nc + y of `v` (m coefficients each); a nonzero
// coefficient at or behind `keep` raises flags[z].  grid: (tail, challenge, proof)
__global__ void any_nonzero_many_kernel(const u64 *v, size_t m, size_t keep, unsigned *flags) {
    const size_t i = keep + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && gl::canon(v[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * m + i]) != 0) atomicOr(flags + blockIdx.z, 1u);
}
// trim_to_len + chunks(n) for M proofs into the interleaved layout of p2hot_commit_many_dev: chunk k of polynomial (proof z,
// challenge c) is column e = c * qdf + k of proof z, which is column e * M + z of the set.  grid: (rows, nc * qdf, M); canonical
__global__ void __launch_bounds__(256) chunks_interleave_kernel(const u64 *v, size_t m, size_t n, unsigned qdf, unsigned nc, u64 *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned e = blockIdx.y, c = e / qdf, k = e % qdf;
    out[((size_t)e * gridDim.z + blockIdx.z) * n + i] = gl::canon(v[((size_t)blockIdx.z * nc + c) * m + (size_t)k * n + i]);
}

// ------------------------------------------------------------------ the permutation argument's share of the quotient
// compute_quotient_polys (plonky2/src/plonk/prover.rs:609-815) evaluates, at every point x = g * w^i of the quotient coset
// (size Nq = n << qbits, qbits = log2_ceil(quotient_degree_factor)), eval_vanishing_poly_base_batch
// (plonk/vanishing_poly.rs:167-330): the terms  L_0(x) (Z_c(x) - 1)  and, per chunk of `degree` routed wires,
//   prev_acc * prod(wire_j + beta_c k_j x + gamma_c) - next_acc * prod(wire_j + beta_c sigma_j(x) + gamma_c)
// (check_partial_products, util/partial_products.rs:52-79: the accumulators run Z_c(x), the partial products, Z_c(g x)), then
// the gate constraint terms; reduces them with the powers of every alpha (plonk_common.rs:99-115) and multiplies by 1 / Z_H(x)
// (prover.rs:797-803).  Everything but the gate terms is circuit independent: this kernel computes it where the three
// commitments' LDE matrices already are.  The gate terms stay the caller's (out of scope): their own reduce_with_powers,
// `gate_sums[a][i]`, enters as alpha_a^K * gate_sums behind the K permutation terms.
// lane = row L of the LDE matrices (committed order).  The reference reads get_lde_values(i, step) = leaves[reverse_bits(i * step)]
// with step = 2^(rate_bits - qbits) (oracle.rs:142-147, prover.rs:640): those are exactly the rows L < Nq, i = bitrev_{log Nq}(L),
// so the column-major matrices are read coalesced; the "next" row is bitrev(i + 2^qbits mod Nq) (prover.rs:643, :708).
struct QuotArgs {
    const u64 *wires, *sigmas, *zs;  // column-major LDE matrices, element (col, L) at col * stride + L; sigmas points at sigma_0
    size_t wires_stride, sigmas_stride, zs_stride;
    const u64 *bk;         // device [nc][num_routed]: beta_c * k_j (wave-uniform)
    const u64 *zh;         // device [2 << qbits]: Z_H(g w^i) for i mod 2^qbits, then their inverses (field/src/zero_poly_coset.rs:21-34)
    const u64 *inv_nx1;    // device [Nq], committed order: 1 / (n (x_L - 1)), x_L = g w^bitrev(L)  (quot_inv_kernel; cached per size)
    const u64 *gate_sums;  // device [nc][Nq] natural order, or null
    u64 *out;              // device [nc][Nq] natural order (prover.rs:805-807: transpose(&quotient_values))
    unsigned num_routed, degree, num_chunks, log_nq, qbits;
    u64 betas[4], gammas[4], alphas[4];
    u64 base[4][4];        // base[a][c] = alpha_a^(nc + c * num_chunks): where challenge c's chunk terms start in the term list
    u64 alpha_k[4];        // alpha_a^K, K = nc + nc * num_chunks
    ntt::RootTable roots;  // forward table: w_Nq^i
};

// 1 / (n (x - 1)) on the quotient coset, in the committed (bit-reversed) order: the denominator of L_0 (zero_poly_coset.rs:58-61).
// Depends on the sizes only, so it is computed once per (log_nq, qbits) and kept by the context.
__global__ void __launch_bounds__(256) quot_inv_kernel(u64 *out, unsigned log_nq, u64 n_field, ntt::RootTable roots) {
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (L >> log_nq) return;
    const size_t i = log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - log_nq)) : 0;
    const u64 x = gl::mul(gl::COSET_SHIFT, log_nq ? ntt::root_pow(roots, (u32)(i << (32 - log_nq))) : (u64)1);
    out[L] = gl::canon(gl::inv(gl::mul(n_field, gl::sub(x, 1))));
}

// DEG > 0: quotient_degree_factor known at compile time (8 in every plonky2 config): the 2 * DEG loads of the NEXT chunk of routed
// wires are issued before the current chunk's 4 * NC * DEG multiplications, so the kernel streams its 13 GB instead of waiting
// for each pair of loads.  DEG == 0: any degree, plain loop.
template <int NC, int DEG>
__global__ void __launch_bounds__(256) quotient_perm_kernel(QuotArgs q) {
#include "kbody_quotient_perm.hpp"
}
// QuotArgs as proof blockIdx.y of M sees them: the member names of QuotArgs, the proof's matrices by their offsets in the table, its beta * k_j
// rows, gate sums and output NC * num_routed / NC * Nq words behind proof 0's, and the challenges and alpha tables as POINTERS into
// the table entry -- the body reads them where it uses them, as scalar loads, and nothing per proof sits in a VGPR array
struct QuotMany {
    const u64 *wires, *sigmas, *zs;
    size_t wires_stride, sigmas_stride, zs_stride;
    const u64 *bk, *zh, *inv_nx1, *gate_sums;
    u64 *out;
    unsigned num_routed, degree, num_chunks, log_nq, qbits;
    const u64 *betas, *gammas, *alphas;
    const u64 (*base)[4];
    const u64 *alpha_k;
    ntt::RootTable roots;
    __device__ QuotMany(const QuotArgs &s, const ManyProof &t, size_t nc)
        : wires(s.wires + t.wires_off), sigmas(s.sigmas), zs(s.zs + t.zs_off), wires_stride(t.wires_stride), sigmas_stride(s.sigmas_stride), zs_stride(t.zs_stride),
          bk(s.bk + blockIdx.y * nc * s.num_routed), zh(s.zh), inv_nx1(s.inv_nx1),
          gate_sums(s.gate_sums ? s.gate_sums + ((blockIdx.y * nc) << s.log_nq) : nullptr), out(s.out + ((blockIdx.y * nc) << s.log_nq)),
          num_routed(s.num_routed), degree(s.degree), num_chunks(s.num_chunks), log_nq(s.log_nq), qbits(s.qbits), betas(t.betas), gammas(t.gammas),
          alphas(t.alphas), base(t.base), alpha_k(t.alpha_k), roots(s.roots) {}
};
template <int NC, int DEG>
__global__ void __launch_bounds__(256) quotient_perm_many_kernel(QuotArgs shared, const ManyProof *__restrict__ tab) {
    const QuotMany q(shared, tab[blockIdx.y], NC);
#include "kbody_quotient_perm.hpp"
}

}  // namespace plonk
