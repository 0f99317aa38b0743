// poseidon.hpp -- width-12 Poseidon over Goldilocks, one permutation per lane (state in VGPRs,
// round constants wave-uniform from constant memory -> SGPRs).
//
// Replaces Poseidon::poseidon (plonky2/src/hash/poseidon.rs:767-777), the sponge
// hash_n_to_hash_no_pad (hashing.rs:118-145), compress/two_to_one (hashing.rs:97-114) and
// Hasher::hash_or_noop (plonk/config.rs:63-74).
//
// MI355X-first choices (not the reference's CPU schedule):
//  * gfx950 issues v_mad_u64_u32 (32x32+64) at the ordinary VOP3 rate while the 24-bit multiplies
//    are half rate (measured, tools/ubench.hip), so everything is built from 32x32+64 multiply-adds:
//    a field multiply is 4 of them plus a two-fold reduction; an MDS output is two 12-term
//    multiply-add chains over the 32-bit halves of the state (small constants as inline operands).
//  * The permutation is evaluated in its defining 30-round form (ARK, S-box, MDS; S-box on word 0
//    only in rounds 4..25, poseidon.rs:781-801) rather than the reference's "fast partial round"
//    refactoring: with cheap small-constant MDS rows the sparse-matrix form (22 wide multiplies
//    per partial round plus a 121-multiply pre-matrix) costs more instructions here.  Both forms
//    are the same function (poseidon.rs:944-957); the oracle pins both to the reference KATs.
//  * The constant layer is fused into the preceding MDS: the round constants, pre-split into
//    {lo32, hi32} words, seed the two accumulators straight from SGPRs.  In the partial rounds the
//    constants of the 11 passive words are pushed forward through the (linear) MDS at table-generation
//    time, so those rounds add a single scalar to word 0 and round 26 absorbs the remainder.
//  * The partial rounds run four to a dense pass (three in the last) over integer products of the MDS matrix, written with the projection
//    D = diag(0, 1, .., 1) (a round REPLACES word 0) so that no field subtraction is needed; their scalars are chain addends too.
//  * Round loops stay rolled so the kernel body fits the instruction cache (one batch of partial rounds is peeled: it carries
//    round 26's constant vector).
#pragma once
#include "gl.hpp"
#include "gl_mul3.hpp"
#ifndef P2HOT_EMU
#define P2_CONST_QUAL __constant__  // device constant memory; indices are wave-uniform -> scalar loads
#endif
#define P2_LITERAL_QUAL static constexpr  // entries become instruction-stream immediates (s_mov_b32 literals); constexpr in both builds:
                                          // M^2 below is computed from them at compile time
#include "poseidon_constants.h"

namespace poseidon {
using gl::u32;
using gl::u64;

#define RC P2_POSEIDON_ALL_ROUND_CONSTANTS  // poseidon.rs:59-157
#define RC_SPLIT P2_POSEIDON_PUSHED_ROUND_CONSTANTS_SPLIT  // [r][i] -> {lo32, hi32} as two u64 words; partial rounds: word 0 only

__device__ __forceinline__ u64 sbox7(u64 x) {  // poseidon.rs:690-696
    u64 x2 = gl::sqr(x);
    u64 x4 = gl::sqr(x2);
    u64 x3 = gl::mul(x, x2);
    return gl::mul(x3, x4);
}

// a + c for a round constant c (canonical): the 64-bit add, its wrap as a compare, and the fold-back of 2^64 = 2^32 - 1 as ONE multiply-add
// on the select (hipcc's form of gl::add_canon is a second 64-bit add and two selects: 5 instructions instead of 4)
__device__ __forceinline__ u64 ark(u64 a, u64 c) {
    if (!P2_ASM_INTERPRETED()) return gl::add_canon(a, c);
    const u64 s = a + c;
    const u32 e = s < c ? 0xFFFFFFFFu : 0u;
    u64 r, d;
    P2_ASM_NC("v_mad_u64_u32 %0, %1, %2, 1, %3", (P2_O(, "=v", r), P2_O(, "=&s", d)), (P2_I(, "v", e), P2_I(, "v", s)));
    return r;
}
// A wave-uniform zero the optimiser cannot see through, made where it is used: a constant-table index built on it is loaded THERE
// (s_load) instead of being hoisted out of the leaf loop into SGPRs that are spilled to VGPR lanes and read back with v_readlane --
// VALU instructions -- at every use (24 per constant vector, measured on the ISA)
__device__ __forceinline__ u32 opaque_zero() {
#ifndef P2HOT_EMU
    u32 z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
#else
    return 0;
#endif
}

// The S-box products run the carry-free multiply streams of gl_mul3.hpp.  The one-permutation-per-lane permutation below (leaf sponge,
// Merkle levels, permutation batches) takes gl::mul3cx / mul1cx: the reduction's carry as one add under a lane mask, its borrow behind a
// scalar branch -- 11 vector instructions per product where gl::mul3cg / mul1cg have 14 (profiles/exec_fixups_ab.txt).  The cooperative
// kernels (poseidon4.hpp, poseidon16.hpp: latency-bound launches with lane exchanges between the rounds) and the Poseidon gate's
// constraints (gates.hpp) keep the mul3cg / mul1cg forms: sbox7_asm, sbox7_x3, sbox_layer.
// x^7 of one word with the hand-scheduled multiply (the partial rounds' single S-box)
__device__ __forceinline__ u64 sbox7_asm(u64 x) {
    u64 x2 = gl::mul1cg(x, x);
    u64 x4 = gl::mul1cg(x2, x2);
    u64 x3 = gl::mul1cg(x, x2);
    return gl::mul1cg(x3, x4);
}
__device__ __forceinline__ u64 sbox7_cx(u64 x) {
    u64 x2 = gl::mul1cx(x, x);
    u64 x4 = gl::mul1cx(x2, x2);
    u64 x3 = gl::mul1cx(x, x2);
    return gl::mul1cx(x3, x4);
}

// x^7 of three independent words at once: x2 = x*x; (x3 = x*x2 and x4 = x2*x2 are independent); x7 = x3*x4
__device__ __forceinline__ void sbox7_x3(u64 &a, u64 &b, u64 &c) {
    u64 x[3] = {a, b, c}, x2[3], x3[3], x4[3];
    gl::mul3cg(x, x, x2);
    gl::mul3cg(x, x2, x3);
    gl::mul3cg(x2, x2, x4);
    gl::mul3cg(x3, x4, x);
    a = x[0];
    b = x[1];
    c = x[2];
}
__device__ __forceinline__ void sbox7_x3cx(u64 &a, u64 &b, u64 &c) {
    u64 x[3] = {a, b, c}, x2[3], x3[3], x4[3];
    gl::mul3cx(x, x, x2);
    gl::mul3cx(x, x2, x3);
    gl::mul3cx(x2, x2, x4);
    gl::mul3cx(x3, x4, x);
    a = x[0];
    b = x[1];
    c = x[2];
}

__device__ __forceinline__ void sbox_layer(u64 s[12]) {  // poseidon.rs:712-718
#pragma unroll
    for (int i = 0; i < 12; i += 3) sbox7_x3(s[i], s[i + 1], s[i + 2]);
}
__device__ __forceinline__ void sbox_layer_cx(u64 s[12]) {
#pragma unroll
    for (int i = 0; i < 12; i += 3) sbox7_x3cx(s[i], s[i + 1], s[i + 2]);
}

// Wave-uniform small constant that the optimiser must not see through: keeps c * x as ONE
// v_mad_u64_u32 (SGPR operand) instead of a shift + 64-bit add on a zero-extended register pair.
__device__ __forceinline__ u32 opaque_const(u32 c) {
#ifndef P2HOT_EMU
    asm volatile("" : "+s"(c));
#endif
    return c;
}

// One term of three MDS rows: the six accumulators (lo / hi halves of rows r, r+1, r+2) each take x * C in ONE
// multiply-add.  Written as asm because hipcc re-associates the 12-term chains into two half chains plus a 64-bit add
// (24 extra instructions per layer) and adds the round constants with separate 64-bit adds; here a chain is exactly
// its 12 multiply-adds, the first of which reads the constant from its SGPR pair as the addend.
template <u32 C>
__device__ __forceinline__ void mds_term(u64 (&al)[3], u64 (&ah)[3], u32 l0, u32 h0, u32 l1, u32 h1, u32 l2, u32 h2) {
    if (!P2_ASM_INTERPRETED()) {  // emulator build with the interpreter off (constant-false in the product)
        al[0] += (u64)l0 * C;
        ah[0] += (u64)h0 * C;
        al[1] += (u64)l1 * C;
        ah[1] += (u64)h1 * C;
        al[2] += (u64)l2 * C;
        ah[2] += (u64)h2 * C;
        return;
    }
    u64 d;
    P2_ASM_NC("v_mad_u64_u32 %0, %6, %7, %13, %0\n\t"
              "v_mad_u64_u32 %1, %6, %8, %13, %1\n\t"
              "v_mad_u64_u32 %2, %6, %9, %13, %2\n\t"
              "v_mad_u64_u32 %3, %6, %10, %13, %3\n\t"
              "v_mad_u64_u32 %4, %6, %11, %13, %4\n\t"
              "v_mad_u64_u32 %5, %6, %12, %13, %5",
              (P2_O(, "+v", al[0]), P2_O(, "+v", ah[0]), P2_O(, "+v", al[1]), P2_O(, "+v", ah[1]), P2_O(, "+v", al[2]),
               P2_O(, "+v", ah[2]), P2_O(, "=&s", d)),
              (P2_I(, "v", l0), P2_I(, "v", h0), P2_I(, "v", l1), P2_I(, "v", h1), P2_I(, "v", l2), P2_I(, "v", h2),
               P2_I(, "n", C)));
}
// the first term (C[0] = 17): starts the six chains from the six wave-uniform 64-bit addends k (SGPR pairs) or from 0
template <bool HAS_K>
__device__ __forceinline__ void mds_first(u64 (&al)[3], u64 (&ah)[3], u32 l0, u32 h0, u32 l1, u32 h1, u32 l2, u32 h2,
                                          const u64 *k) {
    if (!P2_ASM_INTERPRETED()) {
        const u64 z[6] = {0, 0, 0, 0, 0, 0};
        const u64 *kk = HAS_K ? k : z;
        al[0] = (u64)l0 * 17u + kk[0];
        ah[0] = (u64)h0 * 17u + kk[1];
        al[1] = (u64)l1 * 17u + kk[2];
        ah[1] = (u64)h1 * 17u + kk[3];
        al[2] = (u64)l2 * 17u + kk[4];
        ah[2] = (u64)h2 * 17u + kk[5];
        return;
    }
    u64 d;
    if (HAS_K) {
        P2_ASM_NC("v_mad_u64_u32 %0, %6, %7, 17, %13\n\t"
                  "v_mad_u64_u32 %1, %6, %8, 17, %14\n\t"
                  "v_mad_u64_u32 %2, %6, %9, 17, %15\n\t"
                  "v_mad_u64_u32 %3, %6, %10, 17, %16\n\t"
                  "v_mad_u64_u32 %4, %6, %11, 17, %17\n\t"
                  "v_mad_u64_u32 %5, %6, %12, 17, %18",
                  (P2_O(, "=&v", al[0]), P2_O(, "=&v", ah[0]), P2_O(, "=&v", al[1]), P2_O(, "=&v", ah[1]),
                   P2_O(, "=&v", al[2]), P2_O(, "=&v", ah[2]), P2_O(, "=&s", d)),
                  (P2_I(, "v", l0), P2_I(, "v", h0), P2_I(, "v", l1), P2_I(, "v", h1), P2_I(, "v", l2), P2_I(, "v", h2),
                   P2_I(, "s", k[0]), P2_I(, "s", k[1]), P2_I(, "s", k[2]), P2_I(, "s", k[3]), P2_I(, "s", k[4]),
                   P2_I(, "s", k[5])));
    } else {
        P2_ASM_NC("v_mad_u64_u32 %0, %6, %7, 17, 0\n\t"
                  "v_mad_u64_u32 %1, %6, %8, 17, 0\n\t"
                  "v_mad_u64_u32 %2, %6, %9, 17, 0\n\t"
                  "v_mad_u64_u32 %3, %6, %10, 17, 0\n\t"
                  "v_mad_u64_u32 %4, %6, %11, 17, 0\n\t"
                  "v_mad_u64_u32 %5, %6, %12, 17, 0",
                  (P2_O(, "=&v", al[0]), P2_O(, "=&v", ah[0]), P2_O(, "=&v", al[1]), P2_O(, "=&v", ah[1]),
                   P2_O(, "=&v", al[2]), P2_O(, "=&v", ah[2]), P2_O(, "=&s", d)),
                  (P2_I(, "v", l0), P2_I(, "v", h0), P2_I(, "v", l1), P2_I(, "v", h1), P2_I(, "v", l2), P2_I(, "v", h2)));
    }
}

// MDS layer fused with the NEXT round's constant layer:
//   y_r = rc_r + sum_i C[i] * x_{(i+r)%12} (+ 8 * x_0 for r = 0)
// circulant first row C = [17,15,41,16,2,28,13,13,39,18,34,20], diag [8,0,...] (poseidon_goldilocks.rs:24-25).
// On gfx950 v_mad_u64_u32 issues at the plain VOP3 rate (tools/ubench), so each output is two
// 12-term multiply-add chains over the 32-bit halves (al, ah < 2^42) and one fold:
//   y = al + ah * 2^32 (mod P), gl::fold3.
// rc2 points at the round's constants split as {lo32, hi32} pairs (RC_SPLIT) or is null.
// `groups` (wave-uniform): bit g set = rows 3g..3g+2 are wanted; the other rows are left stale.
// one MDS row (no constant, not row 0): two 12-term chains and a single-stream fold -- for the LAST layer of a permutation, whose
// reader wants four words (a digest, or the capacity between two absorbs): one triple and this row instead of two triples
template <int R>
__device__ __forceinline__ u64 mds_row(const u32 (&xl)[12], const u32 (&xh)[12]) {
    static_assert(R > 0 && R < 12, "row 0 carries the diagonal term");
    constexpr u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    u64 al = (u64)xl[R] * opaque_const(C[0]), ah = (u64)xh[R] * opaque_const(C[0]);
#pragma unroll
    for (int i = 1; i < 12; ++i) {
        al += (u64)xl[(R + i) % 12] * opaque_const(C[i]);
        ah += (u64)xh[(R + i) % 12] * opaque_const(C[i]);
    }
    return gl::fold1(al, ah);
}

// `single` (wave-uniform; 3, 8 or none): one more row computed on its own (mds_row)
__device__ __forceinline__ void mds_layer(u64 s[12], const u64 *rc2, unsigned groups = 0xFu, int single = -1) {
    u32 xl[12], xh[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        xl[i] = (u32)s[i];
        xh[i] = (u32)(s[i] >> 32);
    }
#pragma unroll
    for (int g = 0; g < 12; g += 3) {  // three rows at a time: six independent chains, then one fold3 stream
        if (!(groups >> (g / 3) & 1u)) continue;
        u64 al[3], ah[3], y[3];
#define P2_X(i) xl[(g + (i)) % 12], xh[(g + (i)) % 12], xl[(g + (i) + 1) % 12], xh[(g + (i) + 1) % 12], xl[(g + (i) + 2) % 12], xh[(g + (i) + 2) % 12]
        if (rc2)
            mds_first<true>(al, ah, P2_X(0), rc2 + 2 * g);
        else
            mds_first<false>(al, ah, P2_X(0), nullptr);
        mds_term<15>(al, ah, P2_X(1));
        mds_term<41>(al, ah, P2_X(2));
        mds_term<16>(al, ah, P2_X(3));
        mds_term<2>(al, ah, P2_X(4));
        mds_term<28>(al, ah, P2_X(5));
        mds_term<13>(al, ah, P2_X(6));
        mds_term<13>(al, ah, P2_X(7));
        mds_term<39>(al, ah, P2_X(8));
        mds_term<18>(al, ah, P2_X(9));
        mds_term<34>(al, ah, P2_X(10));
        mds_term<20>(al, ah, P2_X(11));
#undef P2_X
        if (g == 0) {  // diag [8, 0, ...]: row 0 only
            al[0] += (u64)xl[0] * opaque_const(8);
            ah[0] += (u64)xh[0] * opaque_const(8);
        }
        gl::fold3(al, ah, y);
        s[g] = y[0];
        s[g + 1] = y[1];
        s[g + 2] = y[2];
    }
    if (single == 3)
        s[3] = mds_row<3>(xl, xh);
    else if (single == 8)
        s[8] = mds_row<8>(xl, xh);
}

// M^2 = the integer square of the MDS matrix M[r][c] = C[(c - r) mod 12] + 8 [r = c = 0] (entries < 2^15, rows < 2^17), built
// at compile time from the generated first row and checked against the generated tables it must agree with
struct Mat12 {
    u32 v[144];
};
constexpr Mat12 mds_matrix() {
    Mat12 m{};
    for (int r = 0; r < 12; ++r)
        for (int c = 0; c < 12; ++c) m.v[12 * r + c] = P2_POSEIDON_M1_ROW0[(c - r + 12) % 12] - ((c - r + 12) % 12 == 0 ? 8u : 0u) + (r == 0 && c == 0 ? 8u : 0u);
    return m;
}
constexpr Mat12 mat_mul(const Mat12 &a, const Mat12 &b) {
    Mat12 m{};
    for (int r = 0; r < 12; ++r)
        for (int c = 0; c < 12; ++c) {
            u64 acc = 0;
            for (int k = 0; k < 12; ++k) acc += (u64)a.v[12 * r + k] * b.v[12 * k + c];
            m.v[12 * r + c] = (u32)acc;
        }
    return m;
}
constexpr bool mat_checks() {
    const Mat12 m1 = mds_matrix(), m2 = mat_mul(m1, m1), m3 = mat_mul(m1, m2);
    for (int j = 0; j < 12; ++j) {
        if (m1.v[j] != P2_POSEIDON_M1_ROW0[j] || m2.v[j] != P2_POSEIDON_M2_ROW0[j]) return false;
        if (m1.v[12 * j] != P2_POSEIDON_MCOL0[j] || m2.v[12 * j] != P2_POSEIDON_MCOL0[12 + j]) return false;
    }
    for (int i = 0; i < 144; ++i)
        if (m3.v[i] != P2_POSEIDON_M3[i]) return false;
    return true;
}
static_assert(mat_checks(), "M, M^2, M^3: the compile-time products disagree with the generated tables");
// The partial rounds REPLACE word 0 (y <- M (D y + s e0), D = diag(0, 1, .., 1), s = sbox(y[0] + c)) -- written with D instead of
// with the difference s - y[0], a batch of rounds is linear in (z, s_1, s_2, ..) with NON-NEGATIVE integer coefficients, entry by entry
// at most those of M^2 and M^3, and needs no field subtraction (round 6; a gl::sub is 11 VALU instructions as hipcc writes it):
//   M (D (M z) + s1 e0)                   = (MD) M z + s1 (M e0)
//   M (D (M (D (M z) + s1 e0)) + s2 e0)   = (MD)(MD) M z + s1 (MD) M e0 + s2 (M e0)            MD = M with column 0 zeroed
constexpr Mat12 mat_drop_col0(const Mat12 &a) {
    Mat12 m = a;
    for (int r = 0; r < 12; ++r) m.v[12 * r] = 0;
    return m;
}
P2_LITERAL_QUAL Mat12 MDS1 = mds_matrix();
P2_LITERAL_QUAL Mat12 MDM = mat_mul(mat_drop_col0(mds_matrix()), mds_matrix());
P2_LITERAL_QUAL Mat12 MDMDM = mat_mul(mat_drop_col0(mds_matrix()), mat_mul(mat_drop_col0(mds_matrix()), mds_matrix()));
P2_LITERAL_QUAL Mat12 MDMDMDM = mat_mul(mat_drop_col0(mds_matrix()), MDMDM);  // (MD)^3 M: entries < 2^28.3, rows < 2^31.8

// The four-application pass's rows: (MD)^3 M z + s1 (MD)^2 M e0 + s2 (MD) M e0 + s3 M e0 (+ one constant half).  Each chain
// multiplies 32-bit halves, so a row is below (coefficient sum) * (2^32 - 1) + 2^32 -- 2^63.72 at the largest row: over 2^63 (hence
// gl::fold3w) but below 2^64.  Checked here in 64-bit integers, entry by entry from the same products the kernel multiplies by; a
// fifth application (rows of 2^39.6) does not fit.
constexpr bool pass4_rows_fit() {
    const Mat12 m1 = mds_matrix(), md = mat_drop_col0(m1);
    const Mat12 p1 = mat_mul(md, m1), p2 = mat_mul(md, p1), p3 = mat_mul(md, p2);
    for (int i = 0; i < 144; ++i)
        if (p1.v[i] != MDM.v[i] || p2.v[i] != MDMDM.v[i] || p3.v[i] != MDMDMDM.v[i]) return false;
    for (int r = 0; r < 12; ++r) {
        u64 sum = (u64)p2.v[12 * r] + p1.v[12 * r] + m1.v[12 * r];
        for (int c = 0; c < 12; ++c) {
            u64 e = 0;  // the entry recomputed in 64 bits: the u32 products above must not have truncated
            for (int k = 0; k < 12; ++k) e += (u64)md.v[12 * r + k] * p2.v[12 * k + c];
            if (e != p3.v[12 * r + c]) return false;
            sum += e;
        }
        if (sum > (1ull << 32)) return false;  // (sum + 1) * (2^32 - 1) <= 2^64 - 1
    }
    return true;
}
static_assert(pass4_rows_fit(), "(MD)^3 M: a four-application row would overflow its 64-bit chains");

// Four partial rounds in one dense pass (the algebra of partial_rounds3 below, one round further).  With z the state whose word 0
// already went through round 0's S-box:
//   y1[0] = (M z)[0]                                                  s1 = sbox(y1[0] + c1)
//   y2[0] = ((MD) M z)[0] + s1 M[0][0]                                s2 = sbox(y2[0] + c2)
//   y3[0] = ((MD)^2 M z)[0] + s1 ((MD) M)[0][0] + s2 M[0][0]          s3 = sbox(y3[0] + c3)
//   y4    = (MD)^3 M z + s1 ((MD)^2 M e0) + s2 ((MD) M e0) + s3 (M e0)
// Four rounds cost one 12-row pass (+3 terms per row), three single rows and four S-boxes.  The pass's rows reach 2^63.72
// (pass4_rows_fit): still two 32x32+64 chains each, recombined by the wide fold (gl::fold3w, two instructions more per row than
// gl::fold3).  A fifth application does not fit (rows of 2^39.6 * 2^32).  The scalars ride the chains as in partial_rounds3: c1..c3
// those of this batch's second to fourth round, cn that of the NEXT pass's first round (fused into row 0).
// FIRST: the pass that starts at round 3's MDS -- z is the state after round 3's full S-box layer (no S-box on word 0 here), c1..c3 are
// the scalars of partial rounds 4..6: 1 + 22 applications of M between the two full-round halves take 6 dense passes (this one, four
// batches of four and the three-round tail batch) instead of 8.
template <bool FIRST = false>
__device__ __forceinline__ void partial_rounds4(u64 s[12], u64 c1, u64 c2, u64 c3, u64 cn) {
    u32 xl[12], xh[12];
    const u64 z0 = FIRST ? s[0] : sbox7_cx(s[0]);  // (not FIRST) round 0's scalar is already in s[0]
    xl[0] = (u32)z0;
    xh[0] = (u32)(z0 >> 32);
#pragma unroll
    for (int i = 1; i < 12; ++i) {
        xl[i] = (u32)s[i];
        xh[i] = (u32)(s[i] >> 32);
    }
    u64 al = (u32)c1, ah = c1 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        al += (u64)xl[j] * P2_POSEIDON_M1_ROW0[j];
        ah += (u64)xh[j] * P2_POSEIDON_M1_ROW0[j];
    }
    const u64 s1 = sbox7_cx(gl::fold1(al, ah));
    const u32 s1l = (u32)s1, s1h = (u32)(s1 >> 32);
    al = (u64)s1l * MDS1.v[0] + (u32)c2;
    ah = (u64)s1h * MDS1.v[0] + (c2 >> 32);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        al += (u64)xl[j] * MDM.v[j];
        ah += (u64)xh[j] * MDM.v[j];
    }
    const u64 s2 = sbox7_cx(gl::fold1(al, ah));
    const u32 s2l = (u32)s2, s2h = (u32)(s2 >> 32);
    al = (u64)s1l * MDM.v[0] + (u64)s2l * MDS1.v[0] + (u32)c3;
    ah = (u64)s1h * MDM.v[0] + (u64)s2h * MDS1.v[0] + (c3 >> 32);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        al += (u64)xl[j] * MDMDM.v[j];
        ah += (u64)xh[j] * MDMDM.v[j];
    }
    const u64 s3 = sbox7_cx(gl::fold1(al, ah));  // row 0 of (MD)^2 M: below 2^25 * 2^32
    const u32 s3l = (u32)s3, s3h = (u32)(s3 >> 32);
#pragma unroll
    for (int g = 0; g < 12; g += 3) {
        u64 bl[3], bh[3], y[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int i = g + t;
            bl[t] = (u64)s1l * MDMDM.v[12 * i] + (u64)s2l * MDM.v[12 * i] + (u64)s3l * MDS1.v[12 * i] + (i == 0 ? (u64)(u32)cn : 0);
            bh[t] = (u64)s1h * MDMDM.v[12 * i] + (u64)s2h * MDM.v[12 * i] + (u64)s3h * MDS1.v[12 * i] + (i == 0 ? cn >> 32 : 0);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                bl[t] += (u64)xl[j] * MDMDMDM.v[12 * i + j];
                bh[t] += (u64)xh[j] * MDMDMDM.v[12 * i + j];
            }
        }
        gl::fold3w(bl, bh, y);
        s[g] = y[0];
        s[g + 1] = y[1];
        s[g + 2] = y[2];
    }
}

// Three partial rounds in one dense pass.  A partial round is y <- M (D y + s e0) with s = sbox(y[0] + c); with z the state whose
// word 0 already went through round 0's S-box:
//   y1[0] = (M z)[0]
//   y2[0] = ((MD) M z)[0] + s1 M[0][0]
//   y3    = (MD)(MD) M z + s1 ((MD) M e0) + s2 (M e0)
// and the integer products of the MDS matrix stay small ((MD)(MD) M <= M^3 < 2^21 per entry, < 2^25 per row), so a row is still two
// 32x32+64 multiply-add chains (accumulators < 2^58): three rounds cost one 12-row pass (+2 terms per row), two single rows and three
// S-boxes instead of three 12-row passes.  The matrix entries are s_mov_b32 literals in the instruction stream (P2_LITERAL_QUAL).  (The
// plain power M^4 would not fit -- its rows sum to 1.04 * 2^32 -- but the column-0-dropped product (MD)^3 M does: partial_rounds4
// above runs four rounds a pass; this three-round form is the tail batch.)  The rounds' scalar constants
// (P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 r]) ride the chains as starting addends: c1, c2 those of this batch's second and third round
// (its first is already in s[0]), and cv = the constant VECTOR of the full round that follows, fused into all twelve rows (eleven
// 4-instruction additions less per permutation than adding it afterwards: -0.3 % cycles, profiles/r06_partial_rounds_ab.txt).
__device__ __forceinline__ void partial_rounds3(u64 s[12], u64 c1, u64 c2, const u64 *cv) {
    u32 xl[12], xh[12];
    const u64 z0 = sbox7_cx(s[0]);  // round 0's scalar is already in s[0]: the previous pass fused it into its row 0
    xl[0] = (u32)z0;
    xh[0] = (u32)(z0 >> 32);
#pragma unroll
    for (int i = 1; i < 12; ++i) {
        xl[i] = (u32)s[i];
        xh[i] = (u32)(s[i] >> 32);
    }
    u64 al = (u32)c1, ah = c1 >> 32;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        al += (u64)xl[j] * P2_POSEIDON_M1_ROW0[j];
        ah += (u64)xh[j] * P2_POSEIDON_M1_ROW0[j];
    }
    const u64 s1 = sbox7_cx(gl::fold1(al, ah));
    const u32 s1l = (u32)s1, s1h = (u32)(s1 >> 32);
    al = (u64)s1l * MDS1.v[0] + (u32)c2;
    ah = (u64)s1h * MDS1.v[0] + (c2 >> 32);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        al += (u64)xl[j] * MDM.v[j];
        ah += (u64)xh[j] * MDM.v[j];
    }
    const u64 s2 = sbox7_cx(gl::fold1(al, ah));
    const u32 s2l = (u32)s2, s2h = (u32)(s2 >> 32);
#pragma unroll
    for (int g = 0; g < 12; g += 3) {
        u64 bl[3], bh[3], y[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int i = g + t;
            const u64 ci = cv[i];
            bl[t] = (u64)s1l * MDM.v[12 * i] + (u64)s2l * MDS1.v[12 * i] + (u32)ci;
            bh[t] = (u64)s1h * MDM.v[12 * i] + (u64)s2h * MDS1.v[12 * i] + (ci >> 32);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                bl[t] += (u64)xl[j] * MDMDM.v[12 * i + j];
                bh[t] += (u64)xh[j] * MDMDM.v[12 * i + j];
            }
        }
        gl::fold3(bl, bh, y);
        s[g] = y[0];
        s[g + 1] = y[1];
        s[g + 2] = y[2];
    }
}

// the permutation; output words are NOT canonicalised (callers canonicalise what they emit).
// Round r: ARK(r) was already added by the previous MDS (or up front for r = 0); S-box; MDS + ARK(r+1).
// `out_groups`: which output word triples the caller reads (bit g = words 3g..3g+2), `out_single`: one more word (3 or 8) it reads;
// the last MDS skips the rest.  A digest is words 0..3 = (triple 0, word 3); the capacity a full absorb keeps is words 8..11 =
// (word 8, triple 3): four rows instead of the six of two triples.
__device__ inline void permute(u64 s[12], unsigned out_groups = 0xFu, int out_single = -1) {
    const u32 z0 = opaque_zero();
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = ark(s[i], RC[i + z0]);
    int round = 0;
#pragma unroll 1
    for (int k = 0; k < 3; ++k, ++round) {
        sbox_layer_cx(s);
        mds_layer(s, RC_SPLIT + 24 * (round + 1));
    }
    // round 3's S-box layer; its MDS and partial rounds 4..6 in ONE dense pass (partial_rounds4<true>); no constant is fused into
    // round 3's MDS -- the batched partial rounds add their scalars themselves (the passive part of the partial-round constants
    // is pushed forward through the MDS at table-generation time, see the generator)
    sbox_layer_cx(s);
    partial_rounds4<true>(s, P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 4], P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 5],
                          P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 6], P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 7]);
    round = 7;
    // partial rounds 7..22 in four batches of four (each batch's first scalar was fused into row 0 of the pass before it), 23..25 in
    // one batch of three.  The constant vector of round 26 (which absorbed the pushed remainder) rides that LAST batch's rows; it is its
    // own copy of the code, outside the rolled loop: fused into the loop's accumulators the vector would be 44 more live SGPRs in EVERY
    // batch (measured: 96 v_readlane per batch of SGPR spill traffic, +4 % instructions)
#pragma unroll 1
    for (int k = 0; k < 4; ++k, round += 4)
        partial_rounds4(s, P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * (round + 1)], P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * (round + 2)],
                        P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * (round + 3)], P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * (round + 4)]);
    const u32 z26 = opaque_zero();
    partial_rounds3(s, P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 24], P2_POSEIDON_PUSHED_ROUND_CONSTANTS[12 * 25],
                    P2_POSEIDON_PUSHED_ROUND_CONSTANTS + 12 * 26 + z26);
    round = 26;
#pragma unroll 1
    for (int k = 0; k < 3; ++k, ++round) {
        sbox_layer_cx(s);
        mds_layer(s, RC_SPLIT + 24 * (round + 1));
    }
    sbox_layer_cx(s);
    mds_layer(s, nullptr, out_groups, out_single);
}

// two_to_one (hashing.rs:97-114): state = [l, r, 0^4], permute, first 4 words
__device__ __forceinline__ void two_to_one(const u64 l[4], const u64 r[4], u64 out[4]) {
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s[i] = l[i];
        s[4 + i] = r[i];
        s[8 + i] = 0;
    }
    permute(s, 0x1u, 3);  // words 0..3 only: triple 0 + word 3
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = gl::canon(s[i]);
}

#undef RC
#undef RC_SPLIT
}  // namespace poseidon
