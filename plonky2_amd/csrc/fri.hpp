// fri.hpp -- FRI commit-phase kernels: coefficient fold, the device-resident Fiat-Shamir sponge,
// proof-of-work grind, extension (de)interleave.
//
// Replaces the loop body of fri_committed_trees (plonky2/src/fri/prover.rs:84-150):
//   reduce_with_powers fold (plonk/plonk_common.rs:120-132) with F^2 arithmetic
//   (field/src/extension/quadratic.rs:180-194, W = 7), Challenger::observe_cap /
//   get_extension_challenge / duplexing (plonky2/src/iop/challenger.rs:39-48, :76-92, :109-116,
//   :129-144) and fri_proof_of_work (fri/prover.rs:153-202).
//
// MI355X-first: extension polynomials live as two base-field planes so the F^2 NTT is the batch-of-2
// base NTT (extension/mod.rs:75-78: the roots of unity are base-field), and the challenger state is
// a 232-byte device object advanced by a single-wave kernel (state over one quad of lanes, MDS through
// DPP quad rotations) -- every FRI round is enqueued without a host round trip; beta never leaves the GPU.
#pragma once
#include "poseidon.hpp"
#include "poseidon4.hpp"
#include "poseidon16.hpp"
#include "keccak.hpp"

namespace fri {
using gl::u32;
using gl::u64;

struct Challenger {  // mirrors challenger.rs:16-24
    u64 state[12];
    u64 in[8];
    u64 out[8];
    u32 n_in, n_out;
};

// observe n_obs elements, then squeeze n_get challenges (popped from the back, challenger.rs:82-92).
// Launch with exactly one 64-thread block.  The sponge state lives in the first 16-lane row of the wave, one word per
// lane (poseidon16.hpp: the lowest-latency mapping -- a proof is a chain of dependent permutations here); the other
// lanes run the same instruction stream on zeros and store nothing.
__global__ void __launch_bounds__(64) challenger_kernel(Challenger *ch, const u64 *obs, size_t n_obs, u64 *out,
                                                       size_t n_get) {
    __shared__ u64 inbuf[8];
    __shared__ u64 outbuf[8];
    const unsigned lane = threadIdx.x, r = lane & 15;
    const bool owner = lane < 12;
    u32 n_in = ch->n_in, n_out = ch->n_out;
    u64 w = owner ? ch->state[lane] : 0;
    if (lane < 8) {
        inbuf[lane] = ch->in[lane];
        outbuf[lane] = ch->out[lane];
    }
    __syncthreads();
    const poseidon16::RowConsts k = poseidon16::row_consts(r);
    // duplexing (challenger.rs:129-144): overwrite the first n_in words with the buffered inputs, permute,
    // refill the output buffer with the rate portion
    auto duplex = [&]() {
        if (owner && lane < n_in) w = inbuf[lane];
        poseidon16::permute_row(w, r, k);
        w = gl::canon(w);
        if (lane < 8) outbuf[lane] = w;
        n_in = 0;
        n_out = 8;
        __syncthreads();
    };
    for (size_t i = 0; i < n_obs; ++i) {
        n_out = 0;
        if (lane == 0) inbuf[n_in] = gl::canon(obs[i]);
        ++n_in;
        __syncthreads();
        if (n_in == 8) duplex();
    }
    for (size_t i = 0; i < n_get; ++i) {
        if (n_in != 0 || n_out == 0) duplex();
        --n_out;
        if (lane == 0) out[i] = outbuf[n_out];
    }
    __syncthreads();
    if (owner) ch->state[lane] = w;
    if (lane < 8) {
        ch->in[lane] = inbuf[lane];
        ch->out[lane] = outbuf[lane];
    }
    if (lane == 0) {
        ch->n_in = n_in;
        ch->n_out = n_out;
    }
}

// BytesHash<N>::to_vec (hash/hash_types.rs:184-194): element c of a digest is its bytes [7c, 7c + 7) zero-extended ("chunks of
// 7 bytes since 8 bytes would allow collisions"): ceil(N / 7) elements, 4 for N = 25 and 5 for N = 32.  slot: the digest's
// 32-byte slot; bytes N..32 are not trusted to be zero.
__device__ __forceinline__ unsigned digest_elems(unsigned N) { return (N + 6) / 7; }
__device__ __forceinline__ u64 digest_element(const u64 *slot, unsigned N, unsigned c) {
    const unsigned b0 = 7 * c, q = b0 >> 3, sh = 8 * (b0 & 7);
    u64 v = slot[q] >> sh;
    if (sh > 8 && q + 1 < 4) v |= slot[q + 1] << (64 - sh);  // the 7 bytes cross into the next word
    const unsigned nb = N - b0 < 7 ? N - b0 : 7;
    return v & ((1ull << (8 * nb)) - 1);
}

// The kernels of the Keccak config's FRI carry the suffix _k256 (Keccak-256): the transcript, the round trees' leaves, the grind.
//
// The same transcript for Challenger<F, KeccakHash<N>>: the generic duplex (challenger.rs:129-144) over
// keccak::keccak_permutation.  One lane: a duplex is a chain of three dependent Keccak-f (no lane of a wave could help the
// next), so the kernel is launched with ONE thread; the buffers sit in LDS because they are indexed by the running lengths.
// Every observed element passes through that lane: about 37 us per 8 elements on the MI355X (profiles/keccak_fri.json), so a
// long observation -- a final polynomial of 2^16 coefficients after few reduction rounds -- is a single-thread kernel of 0.6 s.
// digest_n != 0: obs holds digest slots and the n_obs observed elements are the to_vec elements of those BytesHash<digest_n>
// (observe_hash / observe_cap, challenger.rs:69-80), element e = chunk e % per of slot e / per.
__global__ void __launch_bounds__(1) challenger_kernel_k256(Challenger *ch, const u64 *obs, size_t n_obs, u64 *out,
                                                              size_t n_get, unsigned digest_n) {
    __shared__ u64 inbuf[8];
    __shared__ u64 outbuf[8];
    u32 n_in = ch->n_in, n_out = ch->n_out;
    u64 st[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) st[i] = ch->state[i];
    for (int i = 0; i < 8; ++i) {
        inbuf[i] = ch->in[i];
        outbuf[i] = ch->out[i];
    }
    auto duplex = [&]() {
#pragma unroll
        for (unsigned i = 0; i < 8; ++i)
            if (i < n_in) st[i] = inbuf[i];
        keccak::keccak_permutation(st);
#pragma unroll
        for (int i = 0; i < 8; ++i) outbuf[i] = st[i];
        n_in = 0;
        n_out = 8;
    };
    const unsigned per = digest_n ? digest_elems(digest_n) : 1;
    for (size_t i = 0; i < n_obs; ++i) {
        n_out = 0;
        inbuf[n_in] = digest_n ? digest_element(obs + 4 * (i / per), digest_n, (unsigned)(i % per)) : gl::canon(obs[i]);
        if (++n_in == 8) duplex();
    }
    for (size_t i = 0; i < n_get; ++i) {
        if (n_in != 0 || n_out == 0) duplex();
        out[i] = outbuf[--n_out];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) ch->state[i] = st[i];
    for (int i = 0; i < 8; ++i) {
        ch->in[i] = inbuf[i];
        ch->out[i] = outbuf[i];
    }
    ch->n_in = n_in;
    ch->n_out = n_out;
}

// coeffs'[j] = sum_{i < arity} beta^i * coeffs[arity*j + i]  (Horner from the top, plonk_common.rs:120-132)
__global__ void fold_kernel(const u64 *c0, const u64 *c1, unsigned arity_bits, const u64 *beta, size_t m_out,
                            u64 *o0, u64 *o1) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m_out) return;
    gl::ext2 b{beta[0], beta[1]};
    gl::ext2 acc{0, 0};
    const size_t base = j << arity_bits;
    for (unsigned i = 1u << arity_bits; i-- > 0;) {
        acc = gl::ext_mul(acc, b);
        acc.a0 = gl::add(acc.a0, c0[base + i]);
        acc.a1 = gl::add(acc.a1, c1[base + i]);
    }
    o0[j] = gl::canon(acc.a0);
    o1[j] = gl::canon(acc.a1);
}

// ---- prove_openings prelude: final_poly = sum_i alpha^(k_i) (F_i(X) - F_i(z_i)) / (X - z_i) ----
// ReducingFactor::reduce_polys_base (util/reducing.rs:83-95): o[t] = sum_j apow[j] * polys[j][t]
// (extension scalar times base coefficient = two base multiplies).  Lane = coefficient index, so
// every polynomial is streamed once with fully coalesced reads; apow / the pointer table are wave-uniform.
__global__ void __launch_bounds__(256) reduce_polys_base_kernel(const u64 *const *polys, size_t n_polys, const u64 *apow,
                                                               size_t n, u64 *o0, u64 *o1) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    u64 a0 = 0, a1 = 0;
    for (size_t j = 0; j < n_polys; ++j) {
        u64 p = polys[j][t];
        a0 = gl::add(a0, gl::mul(apow[2 * j], p));
        a1 = gl::add(a1, gl::mul(apow[2 * j + 1], p));
    }
    o0[t] = a0;
    o1[t] = a1;
}

// The same sum for short polynomials (recursion-size proofs: n = 2^12, ~170 polynomials): with one lane per coefficient the
// launch is 16 workgroups walking a chain of n_polys dependent multiply-adds.  Here a workgroup is 64 coefficients x 16
// polynomial groups (lane (t, g) sums the polynomials j = g mod 16) and the groups are folded through LDS in a fixed order,
// so the chain is n_polys / 16 long on 16x the lanes.  Field addition is exact: any order gives the same canonical value.
__global__ void __launch_bounds__(1024) reduce_polys_base_small_kernel(const u64 *const *polys, size_t n_polys, const u64 *apow,
                                                                      size_t n, u64 *o0, u64 *o1) {
    __shared__ u64 s0[16][64], s1[16][64];
    const unsigned lane = threadIdx.x & 63u, g = threadIdx.x >> 6;
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    u64 a0 = 0, a1 = 0;
    if (t < n)
        for (size_t j = g; j < n_polys; j += 16) {
            u64 p = polys[j][t];
            a0 = gl::add(a0, gl::mul(apow[2 * j], p));
            a1 = gl::add(a1, gl::mul(apow[2 * j + 1], p));
        }
    s0[g][lane] = a0;
    s1[g][lane] = a1;
    __syncthreads();
    for (unsigned d = 8; d; d >>= 1) {
        if (g < d) {
            s0[g][lane] = gl::add(s0[g][lane], s0[g + d][lane]);
            s1[g][lane] = gl::add(s1[g][lane], s1[g + d][lane]);
        }
        __syncthreads();
    }
    if (g == 0 && t < n) {
        o0[t] = s0[0][lane];
        o1[t] = s1[0][lane];
    }
}

// divide_by_linear (field/src/polynomial/division.rs:79-92) is the Horner suffix scan
//   b_k = b_{k+1} * z + c_k,  quotient[k-1] = b_k (k >= 1), padded with a zero.
// Three steps over chunks of 2^chunk_log coefficients: (1) chunk totals, (2) chunk carries by a
// suffix scan (one workgroup), (3) replay each chunk from its carry and emit
//   acc[k] = acc[k] * shift + quotient[k]     (ReducingFactor::shift_poly + `final_poly += quotient`, oracle.rs:210-212)
__global__ void horner_chunk_totals_kernel(const u64 *c0, const u64 *c1, unsigned chunk_log, size_t n_chunks, gl::ext2 z,
                                           u64 *p0, u64 *p1) {
    size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    gl::ext2 acc{0, 0};
    const size_t base = m << chunk_log;
    for (size_t i = (size_t)1 << chunk_log; i-- > 0;) {
        acc = gl::ext_mul(acc, z);
        acc.a0 = gl::add(acc.a0, c0[base + i]);
        acc.a1 = gl::add(acc.a1, c1[base + i]);
    }
    p0[m] = acc.a0;
    p1[m] = acc.a1;
}

// carry[m] = sum_{m' > m} P[m'] * zL^(m' - m - 1)  (zL = z^(chunk length)); one 1024-thread block.
// Each thread owns `per` consecutive chunks; block-level Hillis-Steele suffix scan through LDS.
__global__ void __launch_bounds__(1024) horner_carries_kernel(const u64 *p0, const u64 *p1, size_t n_chunks, size_t per,
                                                             gl::ext2 zL, u64 *t0, u64 *t1) {
    __shared__ u64 s0[1024], s1[1024];
    const unsigned tid = threadIdx.x;
    const size_t lo = (size_t)tid * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    // local total of my chunks: L = sum_{g} P[lo + g] * zL^g ; and zL^per
    gl::ext2 loc{0, 0};
    for (size_t m = hi; m-- > lo;) {
        loc = gl::ext_mul(loc, zL);
        loc.a0 = gl::add(loc.a0, p0[m]);
        loc.a1 = gl::add(loc.a1, p1[m]);
    }
    gl::ext2 zP{1, 0};  // zL^per
    for (size_t g = 0; g < per; ++g) zP = gl::ext_mul(zP, zL);
    s0[tid] = lo < n_chunks ? loc.a0 : 0;
    s1[tid] = lo < n_chunks ? loc.a1 : 0;
    __syncthreads();
    // inclusive suffix scan: S[t] = sum_{t' >= t} loc[t'] * zP^(t' - t)
    gl::ext2 f = zP;
    for (unsigned d = 1; d < 1024; d <<= 1) {
        gl::ext2 add{0, 0};
        if (tid + d < 1024) add = gl::ext_mul(gl::ext2{s0[tid + d], s1[tid + d]}, f);
        __syncthreads();
        s0[tid] = gl::add(s0[tid], add.a0);
        s1[tid] = gl::add(s1[tid], add.a1);
        __syncthreads();
        f = gl::ext_mul(f, f);
    }
    // carry into my last chunk = S[tid + 1]; walk my chunks backwards
    gl::ext2 carry{0, 0};
    if (tid + 1 < 1024) carry = gl::ext2{s0[tid + 1], s1[tid + 1]};
    for (size_t m = hi; m-- > lo;) {
        t0[m] = carry.a0;
        t1[m] = carry.a1;
        carry = gl::ext_mul(carry, zL);
        carry.a0 = gl::add(carry.a0, p0[m]);
        carry.a1 = gl::add(carry.a1, p1[m]);
    }
}

// The chunk carries of a long polynomial in two levels (2^22 coefficients = 65536 chunks: one block walking 64 chunks per
// thread took 319 us): groups of 2^group_log chunks get their totals from horner_chunk_totals_kernel (ratio zL), the group
// carries T come from horner_carries_kernel over the groups, and this kernel walks each group down from its carry:
//   t[last chunk of g] = T[g],  t[m] = t[m + 1] * zL + P[m + 1].
__global__ void horner_group_walk_kernel(const u64 *p0, const u64 *p1, unsigned group_log, size_t n_groups, gl::ext2 zL, const u64 *T0,
                                         const u64 *T1, u64 *t0, u64 *t1) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    gl::ext2 carry{T0[g], T1[g]};
    const size_t base = g << group_log;
    for (size_t i = (size_t)1 << group_log; i-- > 0;) {
        const size_t m = base + i;
        t0[m] = carry.a0;
        t1[m] = carry.a1;
        carry = gl::ext_mul(carry, zL);
        carry.a0 = gl::add(carry.a0, p0[m]);
        carry.a1 = gl::add(carry.a1, p1[m]);
    }
}

__global__ void horner_emit_kernel(const u64 *c0, const u64 *c1, unsigned chunk_log, size_t n_chunks, gl::ext2 z,
                                   const u64 *t0, const u64 *t1, const u64 *shift_ptr, int accumulate, u64 *a0, u64 *a1) {
    size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    const gl::ext2 shift{shift_ptr[0], shift_ptr[1]};  // alpha^(#polys of the batch), device-resident (alpha never visits the host)
    gl::ext2 acc{t0[m], t1[m]};
    const size_t base = m << chunk_log, n = n_chunks << chunk_log;
    for (size_t i = (size_t)1 << chunk_log; i-- > 0;) {
        const size_t k = base + i;
        if (k == n - 1) {  // the padding coefficient of the quotient ("pad back to power of two", oracle.rs:209)
            gl::ext2 prev = accumulate ? gl::ext_mul(gl::ext2{a0[k], a1[k]}, shift) : gl::ext2{0, 0};
            a0[k] = gl::canon(prev.a0);
            a1[k] = gl::canon(prev.a1);
        }
        acc = gl::ext_mul(acc, z);
        acc.a0 = gl::add(acc.a0, c0[k]);
        acc.a1 = gl::add(acc.a1, c1[k]);
        if (k >= 1) {  // quotient[k-1] = b_k
            gl::ext2 prev = accumulate ? gl::ext_mul(gl::ext2{a0[k - 1], a1[k - 1]}, shift) : gl::ext2{0, 0};
            a0[k - 1] = gl::canon(gl::add(prev.a0, acc.a0));
            a1[k - 1] = gl::canon(gl::add(prev.a1, acc.a1));
        }
    }
}

// [n_points][total][2] (how the evaluation kernels write) -> per oracle [n_points][W_o][2], oracles back to back (how the
// caller's OpeningSet buffers are laid out), so the results go back in one copy.  Up to 8 oracles, described by value.
struct OpeningLayout {
    unsigned n_oracles;
    unsigned width[8];   // W_o
    unsigned first[8];   // index of the oracle's first polynomial among the `total`
};
__global__ void reorder_openings_kernel(const u64 *res, size_t total, size_t n_points, OpeningLayout lay, u64 *out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one (point, polynomial) pair of the device layout
    if (t >= n_points * total) return;
    const size_t p = t / total, j = t % total;
    size_t out_off = 0;
    unsigned o = 0;
    while (o + 1 < lay.n_oracles && j >= lay.first[o] + lay.width[o]) {
        out_off += 2 * n_points * lay.width[o];
        ++o;
    }
    const size_t dst = out_off + 2 * (p * lay.width[o] + (j - lay.first[o]));
    out[dst] = res[2 * t];
    out[dst + 1] = res[2 * t + 1];
}

// OpeningSet::new (plonky2/src/plonk/proof.rs:314-327): out[j] = polys[j](z) for an extension point z.
// Stage 1 (eval_polys_dot_kernel): workgroup (j, s) evaluates segment s (seg = 2^seg_log coefficients) of polynomial
//   j at z as a dot product with the table z^u, u < seg -> part[j][s].
// Stage 2: workgroup j evaluates the extension polynomial sum_s part[j][s] * (z^seg)^s: lane t Horner-folds the
//   partials t, t+256, ... with (z^seg)^256, the 256 results are combined with weights (z^seg)^t through LDS.
__device__ __forceinline__ gl::ext2 block_weighted_sum(gl::ext2 acc, gl::ext2 z, u64 *s0, u64 *s1) {
    const unsigned tid = threadIdx.x;
    gl::ext2 w{1, 0}, b = z;  // weight z^tid
    for (unsigned e = tid; e; e >>= 1) {
        if (e & 1) w = gl::ext_mul(w, b);
        b = gl::ext_mul(b, b);
    }
    acc = gl::ext_mul(acc, w);
    s0[tid] = acc.a0;
    s1[tid] = acc.a1;
    __syncthreads();
    for (unsigned d = 128; d; d >>= 1) {
        if (tid < d) {
            s0[tid] = gl::add(s0[tid], s0[tid + d]);
            s1[tid] = gl::add(s1[tid], s1[tid + d]);
        }
        __syncthreads();
    }
    return gl::ext2{s0[0], s1[0]};
}

// out[j] = alpha^j as [2] words for j < count, alpha read from device memory: base.powers() of ReducingFactor
// (util/reducing.rs:88-89) and, at index J, the shift_poly factor alpha^J (reducing.rs:103-106)
__global__ void alpha_powers_kernel(const u64 *alpha, size_t count, u64 *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    gl::ext2 w{1, 0}, b{gl::canon(alpha[0]), gl::canon(alpha[1])};
    for (size_t e = j; e; e >>= 1) {
        if (e & 1) w = gl::ext_mul(w, b);
        b = gl::ext_mul(b, b);
    }
    out[2 * j] = gl::canon(w.a0);
    out[2 * j + 1] = gl::canon(w.a1);
}

// fri_prover_query_rounds (fri/prover.rs:215-220, :243-253): x_index = rand % N per query, then x_index >>= arity_bits per
// round.  idx[0][q] = x_index, idx[1 + r][q] = x_index after round r's shift; rand are the challenger's outputs on the device.
struct ArityBits {
    unsigned char b[32];
};
__global__ void query_indices_kernel(const u64 *rand, size_t n_queries, unsigned log_n_total, ArityBits ab, unsigned n_rounds, u64 *idx) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    u64 x = gl::canon(rand[q]) & ((((u64)1) << log_n_total) - 1);  // rand.to_canonical_u64() as usize % n, n = 2^log_n_total
    idx[q] = x;
    for (unsigned r = 0; r < n_rounds; ++r) {
        x >>= ab.b[r];
        idx[(1 + (size_t)r) * n_queries + q] = x;
    }
}

// w0[u] + X w1[u] = z^u for u < count (the power table of one segment, shared by every segment of every polynomial)
__device__ __forceinline__ void ext_powers_body(gl::ext2 z, unsigned count, u64 *w0, u64 *w1) {
    const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= count) return;
    gl::ext2 w{1, 0}, b = z;
    for (unsigned e = u; e; e >>= 1) {
        if (e & 1) w = gl::ext_mul(w, b);
        b = gl::ext_mul(b, b);
    }
    w0[u] = w.a0;
    w1[u] = w.a1;
}
__global__ void ext_powers_kernel(gl::ext2 z, unsigned count, u64 *w0, u64 *w1) { ext_powers_body(z, count, w0, w1); }
// one table per point of a point list (grid row y): pts [G][2] canonical, w [G][2][count]
__global__ void ext_powers_many_kernel(const u64 *__restrict__ pts, unsigned count, u64 *w) {
    u64 *w0 = w + (size_t)blockIdx.y * 2 * count;
    ext_powers_body(gl::ext2{pts[2 * blockIdx.y], pts[2 * blockIdx.y + 1]}, count, w0, w0 + count);
}

// Stage 1 as a dot product with the segment's power table: the coefficients are base-field elements, so a term is two
// base multiplications instead of the extension multiplication of a Horner step (about 40 instructions instead of 110).
__device__ __forceinline__ void eval_polys_dot_body(const u64 *const *polys, unsigned seg_log, const u64 *w0, const u64 *w1, u64 *part, u64 *s0,
                                                    u64 *s1) {
    const unsigned tid = threadIdx.x;
    const size_t seg = (size_t)1 << seg_log;
    const u64 *c = polys[blockIdx.x] + (size_t)blockIdx.y * seg;
    u64 a0 = 0, a1 = 0;
    for (size_t t = tid; t < seg; t += 256) {
        const u64 x = c[t];
        a0 = gl::add(a0, gl::mul1(x, w0[t]));
        a1 = gl::add(a1, gl::mul1(x, w1[t]));
    }
    s0[tid] = a0;
    s1[tid] = a1;
    __syncthreads();
    for (unsigned d = 128; d; d >>= 1) {
        if (tid < d) {
            s0[tid] = gl::add(s0[tid], s0[tid + d]);
            s1[tid] = gl::add(s1[tid], s1[tid + d]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        u64 *o = part + 2 * ((size_t)blockIdx.x * gridDim.y + blockIdx.y);
        o[0] = s0[0];
        o[1] = s1[0];
    }
}
__global__ void __launch_bounds__(256) eval_polys_dot_kernel(const u64 *const *polys, unsigned seg_log, const u64 *w0,
                                                            const u64 *w1, u64 *part /* [J][S][2] */) {
    __shared__ u64 s0[256], s1[256];
    eval_polys_dot_body(polys, seg_log, w0, w1, part, s0, s1);
}
// A point set per polynomial range (p2hot_eval_openings_many): polynomial j belongs to group grp[j] (a proof) and is evaluated at
// that group's P = gridDim.z points; point z of group g has the power table w[(g * P + z)] ([2][seg] words).  part [P][J][S][2]
__global__ void __launch_bounds__(256) eval_polys_dot_many_kernel(const u64 *const *polys, const unsigned *__restrict__ grp, unsigned seg_log,
                                                                 const u64 *w, u64 *part) {
    __shared__ u64 s0[256], s1[256];
    const size_t seg = (size_t)1 << seg_log;
    const u64 *w0 = w + ((size_t)grp[blockIdx.x] * gridDim.z + blockIdx.z) * 2 * seg;
    eval_polys_dot_body(polys, seg_log, w0, w0 + seg, part + 2 * (size_t)blockIdx.z * gridDim.x * gridDim.y, s0, s1);
}

__device__ __forceinline__ void eval_polys_stage2_body(const u64 *part, size_t n_seg, gl::ext2 zs, gl::ext2 zs256, u64 *out, u64 *s0, u64 *s1) {
    const unsigned tid = threadIdx.x;
    const u64 *c = part + 2 * (size_t)blockIdx.x * n_seg;
    gl::ext2 acc{0, 0};
    if (tid < n_seg) {
        size_t last = tid + ((n_seg - 1 - tid) / 256) * 256;
        for (size_t t = last;; t -= 256) {
            acc = gl::ext_mul(acc, zs256);
            acc.a0 = gl::add(acc.a0, c[2 * t]);
            acc.a1 = gl::add(acc.a1, c[2 * t + 1]);
            if (t < 256) break;
        }
    }
    gl::ext2 r = block_weighted_sum(acc, zs, s0, s1);
    if (tid == 0) {
        out[2 * blockIdx.x] = gl::canon(r.a0);
        out[2 * blockIdx.x + 1] = gl::canon(r.a1);
    }
}
__global__ void __launch_bounds__(256) eval_polys_stage2_kernel(const u64 *part, size_t n_seg, gl::ext2 zs, gl::ext2 zs256,
                                                               u64 *out /* [J][2] */) {
    __shared__ u64 s0[256], s1[256];
    eval_polys_stage2_body(part, n_seg, zs, zs256, out, s0, s1);
}
// grid (J, P): zsp [G * P][4] = (z^seg, (z^seg)^256) per point of every group, canonical; out [P][J][2]
__global__ void __launch_bounds__(256) eval_polys_stage2_many_kernel(const u64 *part, const unsigned *__restrict__ grp, size_t n_seg,
                                                                    const u64 *__restrict__ zsp, u64 *out) {
    __shared__ u64 s0[256], s1[256];
    const u64 *z = zsp + 4 * ((size_t)grp[blockIdx.x] * gridDim.y + blockIdx.y);
    const size_t pj = (size_t)blockIdx.y * gridDim.x;
    eval_polys_stage2_body(part + 2 * pj * n_seg, n_seg, gl::ext2{z[0], z[1]}, gl::ext2{z[2], z[3]}, out + 2 * pj, s0, s1);
}

// merkle_tree_prove (hash/merkle_tree.rs:151-190) for m leaf indices straight from the device-resident
// digest array: out[q][i] = sibling at layer i.  Lane = (query, layer).
// A leaf index >= 2^log_leaves (the reference panics) yields a zero path and raises *oob.
__global__ void merkle_paths_kernel(const u64 *digests, unsigned log_leaves, unsigned cap_height, const u64 *idx,
                                    size_t m, u64 *out, unsigned *oob) {
    const unsigned layers = log_leaves - cap_height;
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (layers == 0 || e >= m * layers) return;
    const size_t q = e / layers;
    const unsigned i = (unsigned)(e % layers);
    const size_t leaf = idx[q];
    if (leaf >> log_leaves) {
#pragma unroll
        for (int w = 0; w < 4; ++w) out[4 * e + w] = 0;
        if (i == 0) atomicOr(oob, 2u);
        return;
    }
    const size_t tree_len = 2 * (((size_t)1 << layers) - 1);
    const size_t pair = (leaf & (((size_t)1 << layers) - 1)) >> i;  // pair_index before this layer's shift
    const size_t parity = pair & 1;
    const size_t siblings_index = ((pair >> 1) << (i + 1)) + ((size_t)1 << i) - 1;
    const u64 *src = digests + 4 * (tree_len * (leaf >> layers) + 2 * siblings_index + (1 - parity));
#pragma unroll
    for (int w = 0; w < 4; ++w) out[4 * e + w] = src[w];
}

// rows of a row-major matrix (the FRI round trees' leaves, MerkleTree::get, merkle_tree.rs:227): out[q][0..w) = in[idx[q]][0..w)
__global__ void gather_rowmajor_kernel(const u64 *in, size_t w, size_t n_rows, const u64 *idx, size_t m, u64 *out, unsigned *oob) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * w) return;
    const size_t q = e / w, c = e % w;
    const u64 r = idx[q];
    if (r >= n_rows) {
        out[e] = 0;
        if (c == 0) atomicOr(oob, 1u);
        return;
    }
    out[e] = gl::canon(in[r * w + c]);
}

// [count][2] <-> two planes (flatten order extension/mod.rs:128-135)
__global__ void deinterleave_kernel(const u64 *in, size_t count, u64 *p0, u64 *p1) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    p0[i] = in[2 * i];
    p1[i] = in[2 * i + 1];
}
__global__ void interleave_kernel(const u64 *p0, const u64 *p1, size_t count, u64 *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[2 * i] = gl::canon(p0[i]);
    out[2 * i + 1] = gl::canon(p1[i]);
}

// fri_proof_of_work (fri/prover.rs:153-202): candidate w is valid when the permutation of the
// challenger's duplex state with w in the next input slot has >= pow_bits leading zeros in word 7.
// Deterministic: atomicMin over valid candidates in [start, start + count) -> the smallest witness.
__global__ void __launch_bounds__(256) pow_kernel(const Challenger *ch, unsigned pow_bits, u64 start, u64 count,
                                                 unsigned long long *best) {
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    // a witness below `start` was found by an earlier chunk: the chunks are enqueued back to back without host round
    // trips, the later ones retire here (kernel boundaries order this load after the earlier chunk's atomicMin)
    if (*best < (unsigned long long)start) return;
    u64 s[12];
    const u32 n_in = ch->n_in;
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = ((u32)i < n_in && i < 8) ? ch->in[i < 8 ? i : 0] : ch->state[i];
    const u64 cand = start + t;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if ((u32)i == n_in) s[i] = cand;
    poseidon::permute(s);
    u64 resp = gl::canon(s[7]);
    unsigned lz = resp ? (unsigned)__clzll((long long)resp) : 64u;
    if (lz >= pow_bits) atomicMin(best, (unsigned long long)cand);
}

// The leaves of a round tree under KeccakHash<N> (fri/prover.rs:99-104): hash_or_noop of 2 << arity_bits words each, which
// copies the leaf when 8 * W <= N (N = 32 at arity 2) -- the commitments' leaf sponge over the planar FRI layout
__global__ void __launch_bounds__(256) round_leaves_kernel_k256(merkle::FriPlanarReader rd, unsigned W, size_t leaf_offset,
                                                               size_t leaf_count, unsigned h, unsigned N, u64 *digests, u64 *cap) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= leaf_count) return;
    const size_t L = leaf_offset + t;
    keccak::leaf_digest(rd, W, L, N, merkle::node_slot(digests, cap, h, 0, L));
}

// The grind for Challenger<F, KeccakHash<N>> (fri/prover.rs:179-195): the same duplex intermediate state with the candidate
// at the next input slot, through keccak::keccak_permutation (three Keccak-f per candidate, more after a rejected word);
// the response is kept word 7.  One candidate per lane.
__global__ void __launch_bounds__(256) pow_kernel_k256(const Challenger *ch, unsigned pow_bits, u64 start, u64 count,
                                                        unsigned long long *best) {
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    if (*best < (unsigned long long)start) return;  // see pow_kernel
    // the duplex intermediate state: the sponge state, its first n_in words overwritten by the buffered inputs, the candidate next
    u64 s[12];
    const u32 n_in = ch->n_in;
    const u64 cand = start + t;
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = ch->state[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if ((u32)i < n_in) s[i] = ch->in[i];
        if ((u32)i == n_in) s[i] = cand;
    }
    keccak::keccak_permutation(s);
    const u64 resp = s[7];  // canonical: only words < p are kept
    unsigned lz = resp ? (unsigned)__clzll((long long)resp) : 64u;
    if (lz >= pow_bits) atomicMin(best, (unsigned long long)cand);
}

// ---- batch FRI (plonky2/src/batch_fri/prover.rs, hash/batch_merkle_tree.rs) ----
// fold_kernel for a round after which the next instance joins (batch_fri/prover.rs:115-136): the reference evaluates the folded
// coefficients f on shift' * H, adds the joining codeword (P's values on g * H) index by index, times beta for f, and interpolates
// on shift' * H again.  P(g w^i) = P'(shift' w^i) for P'(X) = P(X g / shift'), and both polynomials have fewer coefficients than
// the coset has points, so the interpolant is coefficient by coefficient
//   s_k = beta * f_k + p_k * c^k,   c = g / shift'  (a base-field constant of the round)
// c^k by square-and-multiply per lane: the base is wave-uniform, the exponent is the lane's coefficient index.
__global__ void __launch_bounds__(256) fold_join_kernel(const u64 *c0, const u64 *c1, unsigned arity_bits, const u64 *beta, size_t m_out,
                                                        const u64 *p0, const u64 *p1, u64 c, u64 *o0, u64 *o1) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m_out) return;
    gl::ext2 b{beta[0], beta[1]};
    gl::ext2 acc{0, 0};
    const size_t base = j << arity_bits;
    for (unsigned i = 1u << arity_bits; i-- > 0;) {
        acc = gl::ext_mul(acc, b);
        acc.a0 = gl::add(acc.a0, c0[base + i]);
        acc.a1 = gl::add(acc.a1, c1[base + i]);
    }
    acc = gl::ext_mul(acc, b);
    const u64 ck = gl::pow(c, (u64)j);
    o0[j] = gl::canon(gl::add(acc.a0, gl::mul(p0[j], ck)));
    o1[j] = gl::canon(gl::add(acc.a1, gl::mul(p1[j], ck)));
}

// A BatchMerkleTree as the query phase sees it, by value (at most 8 groups).  Group k: its column-major LDE matrix, the shift from
// a leaf index of the tallest group to its own row (h_0 - h_k), its first word inside values(i) flattened; segment k of the digest
// array: where it starts, its leaf and cap heights (h_k, h_{k+1} or the tree's cap height), its first layer inside open_batch(i).
struct BatchTreeTable {
    const u64 *lde[8];
    size_t stride[8];
    size_t dig_off[8];  // in digests
    unsigned w_off[8], shift[8], log_h[8], cap_h[8], layer_off[8];
    unsigned n_groups, total_w, layers;
};

// BatchMerkleTree::values (hash/batch_merkle_tree.rs:155-164) flattened, for m leaf indices of the tallest group:
// out[q][w_off[k] + c] = group k's element (idx[q] >> shift[k], c).  Lane = (query, word).  The group is picked by compares against
// constants of the table (no dynamically indexed array).  An index >= 2^log_h[0] zeroes its row and raises *oob like gather_rows_kernel.
__global__ void __launch_bounds__(256) batch_rows_kernel(BatchTreeTable t, const u64 *idx, size_t m, u64 *out, unsigned *oob) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * t.total_w) return;
    const size_t q = e / t.total_w;
    const unsigned c = (unsigned)(e % t.total_w);
    const u64 r = idx[q];
    if (r >> t.log_h[0]) {
        out[e] = 0;
        if (c == 0) atomicOr(oob, 1u);
        return;
    }
    const u64 *lde = t.lde[0];
    size_t stride = t.stride[0];
    unsigned w0 = 0, sh = 0;
#pragma unroll
    for (unsigned k = 1; k < 8; ++k)
        if (k < t.n_groups && c >= t.w_off[k]) {
            lde = t.lde[k];
            stride = t.stride[k];
            w0 = t.w_off[k];
            sh = t.shift[k];
        }
    out[e] = gl::canon(lde[(size_t)(c - w0) * stride + (size_t)(r >> sh)]);
}

// BatchMerkleTree::open_batch (hash/batch_merkle_tree.rs:133-153): the merkle_tree_prove paths of the segments, concatenated.
// out[q][i] = sibling at layer i of leaf idx[q]; layer i belongs to the last segment k with layer_off[k] <= i and is layer
// i - layer_off[k] of the tree (2^log_h[k] leaves, cap height cap_h[k]) at digests + 4 * dig_off[k], for leaf idx[q] >> shift[k].
// Lane = (query, layer), as merkle_paths_kernel.
__global__ void __launch_bounds__(256) batch_paths_kernel(const u64 *digests, BatchTreeTable t, const u64 *idx, size_t m, u64 *out,
                                                          unsigned *oob) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t.layers == 0 || e >= m * t.layers) return;
    const size_t q = e / t.layers;
    const unsigned i = (unsigned)(e % t.layers);
    const u64 r = idx[q];
    if (r >> t.log_h[0]) {
#pragma unroll
        for (int w = 0; w < 4; ++w) out[4 * e + w] = 0;
        if (i == 0) atomicOr(oob, 2u);
        return;
    }
    size_t dig_off = t.dig_off[0];
    unsigned l0 = 0, sh = 0, lh = t.log_h[0], ch = t.cap_h[0];
#pragma unroll
    for (unsigned k = 1; k < 8; ++k)
        if (k < t.n_groups && i >= t.layer_off[k]) {
            dig_off = t.dig_off[k];
            l0 = t.layer_off[k];
            sh = t.shift[k];
            lh = t.log_h[k];
            ch = t.cap_h[k];
        }
    const unsigned layers = lh - ch, il = i - l0;
    const size_t leaf = (size_t)(r >> sh);
    const size_t tree_len = 2 * (((size_t)1 << layers) - 1);
    const size_t pair = (leaf & (((size_t)1 << layers) - 1)) >> il;
    const size_t parity = pair & 1;
    const size_t siblings_index = ((pair >> 1) << (il + 1)) + ((size_t)1 << il) - 1;
    const u64 *src = digests + 4 * (dig_off + tree_len * (leaf >> layers) + 2 * siblings_index + (1 - parity));
#pragma unroll
    for (int w = 0; w < 4; ++w) out[4 * e + w] = src[w];
}

// ---- M proofs of one shape per launch (p2hot_fri_commit_many_dev, p2hot_fri_pow_many) ----
// The commit phase and the grind of a recursion-size proof are chains of launches that leave the chip idle; M proofs share
// nothing, so each kernel below is its single-proof kernel with the proof on a grid axis.  Coefficient planes are [2][M][len]
// (plane p of proof y at (p * M + y) * len, M = gridDim.y): the 2M columns of one LDE.  The single-proof kernels above are
// untouched; these repeat their arithmetic statement by statement, so every word equals the single call's.

// challenger_kernel for M transcripts: workgroup blockIdx.x advances chs[blockIdx.x], observes obs[blockIdx.x * obs_stride + i]
// (obs_stride = 0: every transcript observes the same words -- the zero caps and the zero padding of prover.rs:122-147) and
// writes its challenges to out[blockIdx.x * out_stride + i].  A Poseidon digest is its 4 words (challenger.rs:69-80), so a cap of
// c digests in their slots is observed as n_obs = 4 c.  n_in / n_out are per transcript: transcripts whose buffers are filled
// differently take different numbers of duplexes, which is per-workgroup control flow.  One transcript per wave, as above.
__global__ void __launch_bounds__(64) challenger_many_kernel(Challenger *const *__restrict__ chs, const u64 *obs, size_t obs_stride,
                                                            size_t n_obs, u64 *out, size_t out_stride, size_t n_get) {
    __shared__ u64 inbuf[8];
    __shared__ u64 outbuf[8];
    Challenger *ch = chs[blockIdx.x];
    obs += (size_t)blockIdx.x * obs_stride;
    out += (size_t)blockIdx.x * out_stride;
    const unsigned lane = threadIdx.x, r = lane & 15;
    const bool owner = lane < 12;
    u32 n_in = ch->n_in, n_out = ch->n_out;
    u64 w = owner ? ch->state[lane] : 0;
    if (lane < 8) {
        inbuf[lane] = ch->in[lane];
        outbuf[lane] = ch->out[lane];
    }
    __syncthreads();
    const poseidon16::RowConsts k = poseidon16::row_consts(r);
    auto duplex = [&]() {  // challenger.rs:129-144
        if (owner && lane < n_in) w = inbuf[lane];
        poseidon16::permute_row(w, r, k);
        w = gl::canon(w);
        if (lane < 8) outbuf[lane] = w;
        n_in = 0;
        n_out = 8;
        __syncthreads();
    };
    for (size_t i = 0; i < n_obs; ++i) {
        n_out = 0;
        if (lane == 0) inbuf[n_in] = gl::canon(obs[i]);
        ++n_in;
        __syncthreads();
        if (n_in == 8) duplex();
    }
    for (size_t i = 0; i < n_get; ++i) {
        if (n_in != 0 || n_out == 0) duplex();
        --n_out;
        if (lane == 0) out[i] = outbuf[n_out];
    }
    __syncthreads();
    if (owner) ch->state[lane] = w;
    if (lane < 8) {
        ch->in[lane] = inbuf[lane];
        ch->out[lane] = outbuf[lane];
    }
    if (lane == 0) {
        ch->n_in = n_in;
        ch->n_out = n_out;
    }
}

// fold_kernel for M proofs, grid (blocks, M): c [2][M][m_out << arity_bits] -> o [2][M][m_out], beta of proof y at beta[2 y]
__global__ void __launch_bounds__(256) fold_many_kernel(const u64 *c, unsigned arity_bits, const u64 *beta, size_t m_out, u64 *o) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m_out) return;
    const size_t y = blockIdx.y, M = gridDim.y, len = m_out << arity_bits;
    const u64 *c0 = c + y * len, *c1 = c + (M + y) * len;
    gl::ext2 b{beta[2 * y], beta[2 * y + 1]};
    gl::ext2 acc{0, 0};
    const size_t base = j << arity_bits;
    for (unsigned i = 1u << arity_bits; i-- > 0;) {
        acc = gl::ext_mul(acc, b);
        acc.a0 = gl::add(acc.a0, c0[base + i]);
        acc.a1 = gl::add(acc.a1, c1[base + i]);
    }
    o[y * m_out + j] = gl::canon(acc.a0);
    o[(M + y) * m_out + j] = gl::canon(acc.a1);
}

// interleave_kernel for M proofs, grid (blocks, M): planes p [2][M][count] -> proof y's [count][2] at out + y * out_stride
// (the round leaves of proof y inside its own leaf block; the final polynomials back to back)
__global__ void __launch_bounds__(256) interleave_many_kernel(const u64 *p, size_t count, u64 *out, size_t out_stride) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t y = blockIdx.y, M = gridDim.y;
    u64 *o = out + y * out_stride;
    o[2 * i] = gl::canon(p[y * count + i]);
    o[2 * i + 1] = gl::canon(p[(M + y) * count + i]);
}

// ---- the prelude of prove_openings for M proofs (final_poly_many_core): grid row y = proof, planes [2][M][len] ----
// What the single-proof launches take by value comes from device tables here: alpha of proof y from its two device words, the
// points from zt [M][n_batches][6] = z | z^L | z^G per batch (L = chunk length, G = L << group_log; canonical words, computed on
// the host as the single path computes its arguments).  `zt` points at the batch's entry of proof 0, zt_stride words further on
// is proof 1's; `which` picks z (0), z^L (1) or z^G (2).
__device__ __forceinline__ gl::ext2 many_point(const u64 *zt, size_t zt_stride, unsigned which) {
    const u64 *e = zt + (size_t)blockIdx.y * zt_stride + 2 * which;
    return gl::ext2{e[0], e[1]};
}

// alpha_powers_kernel: out [M][count][2], alpha of proof y at alpha[y * alpha_stride]
__global__ void __launch_bounds__(256) alpha_powers_many_kernel(const u64 *alpha, size_t alpha_stride, size_t count, u64 *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    alpha += (size_t)blockIdx.y * alpha_stride;
    out += 2 * (size_t)blockIdx.y * count;
    gl::ext2 w{1, 0}, b{gl::canon(alpha[0]), gl::canon(alpha[1])};
    for (size_t e = j; e; e >>= 1) {
        if (e & 1) w = gl::ext_mul(w, b);
        b = gl::ext_mul(b, b);
    }
    out[2 * j] = gl::canon(w.a0);
    out[2 * j + 1] = gl::canon(w.a1);
}

// reduce_polys_base_kernel: proof y's pointers at polys[y * table_stride ..], its alpha powers at apow[y * apow_stride ..]
__global__ void __launch_bounds__(256) reduce_polys_base_many_kernel(const u64 *const *polys, size_t table_stride, size_t n_polys,
                                                                    const u64 *apow, size_t apow_stride, size_t n, u64 *o) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const size_t y = blockIdx.y, M = gridDim.y;
    polys += y * table_stride;
    apow += y * apow_stride;
    u64 a0 = 0, a1 = 0;
    for (size_t j = 0; j < n_polys; ++j) {
        u64 p = polys[j][t];
        a0 = gl::add(a0, gl::mul(apow[2 * j], p));
        a1 = gl::add(a1, gl::mul(apow[2 * j + 1], p));
    }
    o[y * n + t] = a0;
    o[(M + y) * n + t] = a1;
}

// reduce_polys_base_small_kernel, the same way
__global__ void __launch_bounds__(1024) reduce_polys_base_small_many_kernel(const u64 *const *polys, size_t table_stride, size_t n_polys,
                                                                           const u64 *apow, size_t apow_stride, size_t n, u64 *o) {
    __shared__ u64 s0[16][64], s1[16][64];
    const unsigned lane = threadIdx.x & 63u, g = threadIdx.x >> 6;
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    const size_t y = blockIdx.y, M = gridDim.y;
    polys += y * table_stride;
    apow += y * apow_stride;
    u64 a0 = 0, a1 = 0;
    if (t < n)
        for (size_t j = g; j < n_polys; j += 16) {
            u64 p = polys[j][t];
            a0 = gl::add(a0, gl::mul(apow[2 * j], p));
            a1 = gl::add(a1, gl::mul(apow[2 * j + 1], p));
        }
    s0[g][lane] = a0;
    s1[g][lane] = a1;
    __syncthreads();
    for (unsigned d = 8; d; d >>= 1) {
        if (g < d) {
            s0[g][lane] = gl::add(s0[g][lane], s0[g + d][lane]);
            s1[g][lane] = gl::add(s1[g][lane], s1[g + d][lane]);
        }
        __syncthreads();
    }
    if (g == 0 && t < n) {
        o[y * n + t] = s0[0][lane];
        o[(M + y) * n + t] = s1[0][lane];
    }
}

// horner_chunk_totals_kernel: c [2][M][n_chunks << chunk_log] -> p [2][M][n_chunks]
__global__ void __launch_bounds__(256) horner_chunk_totals_many_kernel(const u64 *c, unsigned chunk_log, size_t n_chunks, const u64 *zt,
                                                                      size_t zt_stride, unsigned which, u64 *p) {
    size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    const size_t y = blockIdx.y, M = gridDim.y, len = n_chunks << chunk_log;
    const u64 *c0 = c + y * len, *c1 = c + (M + y) * len;
    const gl::ext2 z = many_point(zt, zt_stride, which);
    gl::ext2 acc{0, 0};
    const size_t base = m << chunk_log;
    for (size_t i = (size_t)1 << chunk_log; i-- > 0;) {
        acc = gl::ext_mul(acc, z);
        acc.a0 = gl::add(acc.a0, c0[base + i]);
        acc.a1 = gl::add(acc.a1, c1[base + i]);
    }
    p[y * n_chunks + m] = acc.a0;
    p[(M + y) * n_chunks + m] = acc.a1;
}

// horner_carries_kernel, grid (1, M): one 1024-thread block per proof; p, t [2][M][n_chunks]
__global__ void __launch_bounds__(1024) horner_carries_many_kernel(const u64 *p, size_t n_chunks, size_t per, const u64 *zt, size_t zt_stride,
                                                                  unsigned which, u64 *t) {
    __shared__ u64 s0[1024], s1[1024];
    const size_t y = blockIdx.y, M = gridDim.y;
    const u64 *p0 = p + y * n_chunks, *p1 = p + (M + y) * n_chunks;
    u64 *t0 = t + y * n_chunks, *t1 = t + (M + y) * n_chunks;
    const gl::ext2 zL = many_point(zt, zt_stride, which);
    const unsigned tid = threadIdx.x;
    const size_t lo = (size_t)tid * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    gl::ext2 loc{0, 0};
    for (size_t m = hi; m-- > lo;) {
        loc = gl::ext_mul(loc, zL);
        loc.a0 = gl::add(loc.a0, p0[m]);
        loc.a1 = gl::add(loc.a1, p1[m]);
    }
    gl::ext2 zP{1, 0};  // zL^per
    for (size_t g = 0; g < per; ++g) zP = gl::ext_mul(zP, zL);
    s0[tid] = lo < n_chunks ? loc.a0 : 0;
    s1[tid] = lo < n_chunks ? loc.a1 : 0;
    __syncthreads();
    gl::ext2 f = zP;
    for (unsigned d = 1; d < 1024; d <<= 1) {
        gl::ext2 add{0, 0};
        if (tid + d < 1024) add = gl::ext_mul(gl::ext2{s0[tid + d], s1[tid + d]}, f);
        __syncthreads();
        s0[tid] = gl::add(s0[tid], add.a0);
        s1[tid] = gl::add(s1[tid], add.a1);
        __syncthreads();
        f = gl::ext_mul(f, f);
    }
    gl::ext2 carry{0, 0};
    if (tid + 1 < 1024) carry = gl::ext2{s0[tid + 1], s1[tid + 1]};
    for (size_t m = hi; m-- > lo;) {
        t0[m] = carry.a0;
        t1[m] = carry.a1;
        carry = gl::ext_mul(carry, zL);
        carry.a0 = gl::add(carry.a0, p0[m]);
        carry.a1 = gl::add(carry.a1, p1[m]);
    }
}

// horner_group_walk_kernel: p, t [2][M][n_groups << group_log], T [2][M][n_groups]
__global__ void __launch_bounds__(256) horner_group_walk_many_kernel(const u64 *p, unsigned group_log, size_t n_groups, const u64 *zt,
                                                                    size_t zt_stride, const u64 *T, u64 *t) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const size_t y = blockIdx.y, M = gridDim.y, n_chunks = n_groups << group_log;
    const u64 *p0 = p + y * n_chunks, *p1 = p + (M + y) * n_chunks;
    u64 *t0 = t + y * n_chunks, *t1 = t + (M + y) * n_chunks;
    const gl::ext2 zL = many_point(zt, zt_stride, 1);
    gl::ext2 carry{T[y * n_groups + g], T[(M + y) * n_groups + g]};
    const size_t base = g << group_log;
    for (size_t i = (size_t)1 << group_log; i-- > 0;) {
        const size_t m = base + i;
        t0[m] = carry.a0;
        t1[m] = carry.a1;
        carry = gl::ext_mul(carry, zL);
        carry.a0 = gl::add(carry.a0, p0[m]);
        carry.a1 = gl::add(carry.a1, p1[m]);
    }
}

// horner_emit_kernel: c, a [2][M][n], t [2][M][n_chunks]; the shift of proof y at shift[y * shift_stride]
__global__ void __launch_bounds__(256) horner_emit_many_kernel(const u64 *c, unsigned chunk_log, size_t n_chunks, const u64 *zt, size_t zt_stride,
                                                              const u64 *t, const u64 *shift_ptr, size_t shift_stride, int accumulate, u64 *a) {
    size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_chunks) return;
    const size_t y = blockIdx.y, M = gridDim.y, n = n_chunks << chunk_log;
    const u64 *c0 = c + y * n, *c1 = c + (M + y) * n;
    u64 *a0 = a + y * n, *a1 = a + (M + y) * n;
    const gl::ext2 z = many_point(zt, zt_stride, 0);
    shift_ptr += y * shift_stride;
    const gl::ext2 shift{shift_ptr[0], shift_ptr[1]};
    gl::ext2 acc{t[y * n_chunks + m], t[(M + y) * n_chunks + m]};
    const size_t base = m << chunk_log;
    for (size_t i = (size_t)1 << chunk_log; i-- > 0;) {
        const size_t k = base + i;
        if (k == n - 1) {  // the padding coefficient of the quotient ("pad back to power of two", oracle.rs:209)
            gl::ext2 prev = accumulate ? gl::ext_mul(gl::ext2{a0[k], a1[k]}, shift) : gl::ext2{0, 0};
            a0[k] = gl::canon(prev.a0);
            a1[k] = gl::canon(prev.a1);
        }
        acc = gl::ext_mul(acc, z);
        acc.a0 = gl::add(acc.a0, c0[k]);
        acc.a1 = gl::add(acc.a1, c1[k]);
        if (k >= 1) {  // quotient[k-1] = b_k
            gl::ext2 prev = accumulate ? gl::ext_mul(gl::ext2{a0[k - 1], a1[k - 1]}, shift) : gl::ext2{0, 0};
            a0[k - 1] = gl::canon(gl::add(prev.a0, acc.a0));
            a1[k - 1] = gl::canon(gl::add(prev.a1, acc.a1));
        }
    }
}

// ---- the query rounds of M proofs (prove_openings_many_core): grid row y = proof ----
// The trees a launch opens, one entry per proof: a matrix (column-major LDE of an initial oracle, or the row-major leaves of a
// round tree), its digest array, the words between columns (column-major only).  A read-only device table, indexed by blockIdx.y.
struct ManyTree {
    const u64 *mat, *dig;
    size_t stride;
};
// Every kernel below writes QUERY-MAJOR into proof y's staging block (out + y * out_stride): query q's record of `rec` words starts at
// q * rec, and this launch fills the words [off, off + w) of it -- the layout of the proof buffers of p2hot.h, so one copy brings a
// proof's buffer back as it is.

// the transcripts before the tail, and back (the grind-miss path): dir 0 saves chs[y] to save[y], 1 restores
__global__ void __launch_bounds__(64) challenger_copy_many_kernel(Challenger *const *__restrict__ chs, Challenger *save, int dir) {
    static_assert(sizeof(Challenger) % 8 == 0, "whole words");
    u64 *a = reinterpret_cast<u64 *>(chs[blockIdx.x]), *b = reinterpret_cast<u64 *>(save + blockIdx.x);
    if (threadIdx.x < sizeof(Challenger) / 8) {
        if (dir)
            a[threadIdx.x] = b[threadIdx.x];
        else
            b[threadIdx.x] = a[threadIdx.x];
    }
}

// query_indices_kernel: rand [M][n_queries] -> idx [M][1 + n_rounds][n_queries]
__global__ void __launch_bounds__(256) query_indices_many_kernel(const u64 *rand, size_t n_queries, unsigned log_n_total, ArityBits ab,
                                                                unsigned n_rounds, u64 *idx) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    rand += (size_t)blockIdx.y * n_queries;
    idx += (size_t)blockIdx.y * (1 + (size_t)n_rounds) * n_queries;
    u64 x = gl::canon(rand[q]) & ((((u64)1) << log_n_total) - 1);
    idx[q] = x;
    for (unsigned r = 0; r < n_rounds; ++r) {
        x >>= ab.b[r];
        idx[(1 + (size_t)r) * n_queries + q] = x;
    }
}

// MerkleTree::get for the m queries of every proof: rows idx[y * idx_stride + q] of proof y's matrix, w words each.  col_major: an
// initial oracle's LDE (p2hot_gather_rows_dev's rows), else a round tree's leaves (gather_rowmajor_kernel).  An index past n_rows
// zeroes its words and raises *oob.
__global__ void __launch_bounds__(256) gather_rows_many_kernel(const ManyTree *__restrict__ trees, int col_major, size_t w, size_t n_rows,
                                                              const u64 *idx, size_t idx_stride, size_t m, u64 *out, size_t out_stride, size_t rec,
                                                              size_t off, unsigned *oob) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * w) return;
    const size_t q = e / w, c = e % w;
    const ManyTree tr = trees[blockIdx.y];
    const u64 r = idx[(size_t)blockIdx.y * idx_stride + q];
    u64 *o = out + (size_t)blockIdx.y * out_stride + q * rec + off + c;
    if (r >= n_rows) {
        *o = 0;
        if (c == 0) atomicOr(oob, 1u);
        return;
    }
    *o = gl::canon(col_major ? tr.mat[c * tr.stride + r] : tr.mat[r * w + c]);
}

// merkle_paths_kernel for the m queries of every proof, from proof y's digest array
__global__ void __launch_bounds__(256) merkle_paths_many_kernel(const ManyTree *__restrict__ trees, unsigned log_leaves, unsigned cap_height,
                                                               const u64 *idx, size_t idx_stride, size_t m, u64 *out, size_t out_stride, size_t rec,
                                                               size_t off, unsigned *oob) {
    const unsigned layers = log_leaves - cap_height;
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (layers == 0 || e >= m * layers) return;
    const size_t q = e / layers;
    const unsigned i = (unsigned)(e % layers);
    const u64 *digests = trees[blockIdx.y].dig;
    const size_t leaf = idx[(size_t)blockIdx.y * idx_stride + q];
    u64 *o = out + (size_t)blockIdx.y * out_stride + q * rec + off + 4 * (size_t)i;
    if (leaf >> log_leaves) {
#pragma unroll
        for (int w = 0; w < 4; ++w) o[w] = 0;
        if (i == 0) atomicOr(oob, 2u);
        return;
    }
    const size_t tree_len = 2 * (((size_t)1 << layers) - 1);
    const size_t pair = (leaf & (((size_t)1 << layers) - 1)) >> i;  // pair_index before this layer's shift
    const size_t parity = pair & 1;
    const size_t siblings_index = ((pair >> 1) << (i + 1)) + ((size_t)1 << i) - 1;
    const u64 *src = digests + 4 * (tree_len * (leaf >> layers) + 2 * siblings_index + (1 - parity));
#pragma unroll
    for (int w = 0; w < 4; ++w) o[w] = src[w];
}

// pow_kernel for M transcripts, grid (blocks, M): the candidates [start, start + count) against transcript y, best[y] by the same
// minimum.  A block of proof y retires at once when best[y] was set by an earlier launch; the launches (pow_search_dev's chunk
// schedule) are shared by all proofs.
__global__ void __launch_bounds__(256) pow_many_kernel(const Challenger *const *__restrict__ chs, unsigned pow_bits, u64 start, u64 count,
                                                      unsigned long long *best) {
    u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const Challenger *ch = chs[blockIdx.y];
    best += blockIdx.y;
    if (*best < (unsigned long long)start) return;
#ifndef P2HOT_EMU
    // the permutation below takes every scalar register (pow_kernel spills four of them into vector lanes): what is only needed
    // after it -- where the minimum goes, the bound -- waits in vector registers instead
    asm volatile("" : "+v"(best), "+v"(pow_bits));
#endif
    u64 s[12];
    const u32 n_in = ch->n_in;
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = ((u32)i < n_in && i < 8) ? ch->in[i < 8 ? i : 0] : ch->state[i];
    const u64 cand = start + t;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if ((u32)i == n_in) s[i] = cand;
    poseidon::permute(s);
    u64 resp = gl::canon(s[7]);
    unsigned lz = resp ? (unsigned)__clzll((long long)resp) : 64u;
    if (lz >= pow_bits) atomicMin(best, (unsigned long long)cand);
}

}  // namespace fri
