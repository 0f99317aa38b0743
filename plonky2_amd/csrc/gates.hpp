// gates.hpp -- the gate constraints' share of the quotient: evaluate_gate_constraints_base_batch (plonky2/src/plonk/vanishing_poly.rs:702-728)
// on the quotient coset for the eight standard gates of include/p2hot.h (P2HOT_GATE_*), D = 2.
//
// Every gate's constraints are added into ONE vector starting at index 0 (vanishing_poly.rs:722-725) and the reduction by powers of
// alpha is linear, so per point x_i and challenge a
//   gate_sums[a][i] = sum_g filter_g(x_i) * sum_j alpha_a^j c_{g,j}(x_i)
// with filter_g = prod_{k in group, k != row} (k - s) [* (0xFFFFFFFF - s) when the circuit has several selector polynomials]
// (gates/gate.rs:326-333), s = constants[selector_index], and the gate's own constants behind the selectors and the lookup selectors
// (gate.rs:179).  lane = row L of the committed LDE matrices, i = bitrev(L), column-major reads, output [nc][Nq] in natural order:
// the indexing of plonk::quotient_perm_kernel and lookup::lookup_terms_kernel.  Both kernels ADD into `out` (canonical).
//   cheap_gates_kernel    Noop, Constant, PublicInput, Arithmetic, ArithmeticExtension, MulExtension, BaseSum: a wave-uniform loop
//                         over the descriptors, one switch per descriptor
//   poseidon_gate_kernel  PoseidonGate (gates/poseidon.rs:204-283), one descriptor per launch: its 12-word state and the dense layers'
//                         temporaries do not set the register budget of the cheap gates
#pragma once
#include "../../include/p2hot.h"
#include "gl.hpp"
#include "poseidon.hpp"

namespace gates {
using gl::u32;
using gl::u64;

constexpr unsigned MAX_CHEAP = 32;         // descriptors per launch of cheap_gates_kernel (they travel as kernel arguments)
constexpr unsigned POSEIDON_WIRES = 135;   // PoseidonGate::end() (gates/poseidon.rs:99-101)
constexpr unsigned POSEIDON_CONSTRAINTS = 123;

// (wires read, constants read, constraints) of a descriptor; kind must be a known one
__host__ __device__ inline void shape(const p2hot_gate &g, unsigned &wires, unsigned &consts, unsigned &constraints) {
    wires = consts = constraints = 0;
    switch (g.kind) {
        case P2HOT_GATE_CONSTANT: wires = consts = constraints = g.param0; break;
        case P2HOT_GATE_PUBLIC_INPUT: wires = constraints = 4; break;
        case P2HOT_GATE_ARITHMETIC: wires = 4 * g.param0, consts = 2, constraints = g.param0; break;
        case P2HOT_GATE_ARITHMETIC_EXT: wires = 8 * g.param0, consts = 2, constraints = 2 * g.param0; break;
        case P2HOT_GATE_MUL_EXT: wires = 6 * g.param0, consts = 1, constraints = 2 * g.param0; break;
        case P2HOT_GATE_BASE_SUM: wires = constraints = 1 + g.param0; break;
        case P2HOT_GATE_POSEIDON: wires = POSEIDON_WIRES, constraints = POSEIDON_CONSTRAINTS; break;
        case P2HOT_GATE_POSEIDON_MDS: wires = 48, constraints = 24; break;
        case P2HOT_GATE_REDUCING: wires = 3 * g.param0 + 4, constraints = 2 * g.param0; break;
        case P2HOT_GATE_REDUCING_EXT: wires = 4 * g.param0 + 4, constraints = 2 * g.param0; break;
        case P2HOT_GATE_RANDOM_ACCESS: {  // param1 = bits | num_extra_constants << 8
            const unsigned bits = g.param1 & 0xFFu, extra = g.param1 >> 8;
            wires = (2 + (bits < 32 ? 1u << bits : 0u) + bits) * g.param0 + extra, consts = extra, constraints = g.param0 * (bits + 2) + extra;
            break;
        }
        case P2HOT_GATE_EXPONENTIATION: wires = 2 + 2 * g.param0, constraints = g.param0 + 1; break;
        case P2HOT_GATE_COSET_INTERPOLATION: {  // param0 = subgroup_bits, param1 = degree
            const unsigned n = g.param0 < 32 ? 1u << g.param0 : 0u, ni = g.param1 > 1 && n >= 2 ? (n - 2) / (g.param1 - 1) : 0;
            wires = 1 + 2 * n + 4 + 2 * (2 * ni + 1), constraints = 4 + 4 * ni;
            break;
        }
        default: break;
    }
}

// compute_filter (gates/gate.rs:326-333)
__device__ __forceinline__ u64 filter(const p2hot_gate &g, u64 s, bool many_selectors) {
    u64 f = 1;
    for (u32 k = g.group_first; k < g.group_end; ++k)
        if (k != g.row) f = gl::mul(f, gl::sub((u64)k, s));
    if (many_selectors) f = gl::mul(f, gl::sub((u64)0xFFFFFFFFu, s));
    return f;
}

struct Args {
    const u64 *wires, *consts;  // LDE matrices, element (col, L) at col * stride + L; consts -> column 0 of constants_sigmas
    size_t wires_stride, consts_stride;
    const u64 *apow;            // device [nc][apow_stride]: alpha_a^j (wave-uniform)
    u64 *out;                   // device [nc][Nq] natural order, added into
    unsigned log_nq, num_gates, num_selectors, consts_first, apow_stride;  // consts_first = num_selectors + num_lookup_selectors
    u64 pih[4];                 // public_inputs_hash (canonical)
    p2hot_gate gates[MAX_CHEAP];
};

template <int NC>
__global__ void __launch_bounds__(256) cheap_gates_kernel(Args q) {
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const u64 *w = q.wires + L, *lc = q.consts + (size_t)q.consts_first * q.consts_stride + L;
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    for (unsigned gi = 0; gi < q.num_gates; ++gi) {
        const p2hot_gate &g = q.gates[gi];
        u64 acc[NC];
#pragma unroll
        for (int a = 0; a < NC; ++a) acc[a] = 0;
        auto put = [&](unsigned j, u64 term) {  // constraint j of this gate
#pragma unroll
            for (int a = 0; a < NC; ++a) acc[a] = gl::mul_add(term, q.apow[(size_t)a * q.apow_stride + j], acc[a]);
        };
        switch (g.kind) {
            case P2HOT_GATE_CONSTANT:  // constant.rs:126-128
                for (unsigned k = 0; k < g.param0; ++k) put(k, gl::sub(lc[(size_t)k * q.consts_stride], w[(size_t)k * q.wires_stride]));
                break;
            case P2HOT_GATE_PUBLIC_INPUT:  // public_input.rs:108-112
                for (unsigned k = 0; k < 4; ++k) put(k, gl::sub(w[(size_t)k * q.wires_stride], q.pih[k]));
                break;
            case P2HOT_GATE_ARITHMETIC: {  // arithmetic_base.rs:173-184
                const u64 c0 = lc[0], c1 = lc[q.consts_stride];
                for (unsigned k = 0; k < g.param0; ++k) {
                    const u64 *v = w + (size_t)(4 * k) * q.wires_stride;
                    const u64 m0 = v[0], m1 = v[q.wires_stride], ad = v[2 * q.wires_stride], ou = v[3 * q.wires_stride];
                    put(k, gl::sub(ou, gl::mul_add(gl::mul(m0, m1), c0, gl::mul(ad, c1))));
                }
                break;
            }
            case P2HOT_GATE_ARITHMETIC_EXT:  // arithmetic_extension.rs:92-110
            case P2HOT_GATE_MUL_EXT: {       // multiplication_extension.rs:86-101
                const bool arith = g.kind == P2HOT_GATE_ARITHMETIC_EXT;
                const unsigned per = arith ? 8 : 6;
                const u64 c0 = lc[0], c1 = arith ? lc[q.consts_stride] : 0;
                for (unsigned k = 0; k < g.param0; ++k) {
                    const u64 *v = w + (size_t)(per * k) * q.wires_stride;
                    const gl::ext2 m0{v[0], v[q.wires_stride]}, m1{v[2 * q.wires_stride], v[3 * q.wires_stride]};
                    const gl::ext2 pr = gl::ext_mul(m0, m1);
                    u64 r0 = gl::mul(pr.a0, c0), r1 = gl::mul(pr.a1, c0);
                    if (arith) {
                        r0 = gl::mul_add(v[4 * q.wires_stride], c1, r0);
                        r1 = gl::mul_add(v[5 * q.wires_stride], c1, r1);
                    }
                    const u64 *o = v + (size_t)(per - 2) * q.wires_stride;
                    put(2 * k, gl::sub(o[0], r0));
                    put(2 * k + 1, gl::sub(o[q.wires_stride], r1));
                }
                break;
            }
            case P2HOT_GATE_BASE_SUM: {  // base_sum.rs:153-170: limbs on wires 1 .., little endian
                u64 sum = 0, pw = 1;
                for (unsigned k = 0; k < g.param0; ++k) {
                    const u64 limb = w[(size_t)(1 + k) * q.wires_stride];
                    sum = gl::mul_add(limb, pw, sum);
                    pw = gl::mul(pw, (u64)g.param1);
                    u64 range = limb;
                    for (u32 t = 1; t < g.param1; ++t) range = gl::mul(range, gl::sub(limb, (u64)t));
                    put(1 + k, range);
                }
                put(0, gl::sub(sum, w[0]));
                break;
            }
            default: break;  // Noop (noop.rs): no constraints
        }
        const u64 f = filter(g, q.consts[(size_t)g.selector_index * q.consts_stride + L], q.num_selectors > 1);
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(f, acc[a], res[a]);
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 *o = q.out + (size_t)a * nq + i;
        *o = gl::canon(gl::add(*o, res[a]));
    }
}

struct PoseidonArgs {
    const u64 *wires, *consts;
    size_t wires_stride, consts_stride;
    const u64 *apow;
    u64 *out;
    unsigned log_nq, num_selectors, apow_stride;
    p2hot_gate gate;
};

// PoseidonGate::eval_unfiltered_base_one (gates/poseidon.rs:204-283).  Wires: inputs 0..11, outputs 12..23, swap 24, deltas 25..28,
// the S-box inputs of full rounds 1..3 at 29 + 12 (r - 1) + i, of the partial rounds at 65 + r, of the second full rounds at
// 87 + 12 r + i.  After every constrained S-box input the state continues from the WIRE.  The partial rounds are the reference's fast
// form (hash/poseidon.rs:365-373, :415-441, :516-542), because that is the form whose S-box inputs the wires hold: the pushed-constant
// dense passes of poseidon::partial_rounds4 meet other intermediate values.  Full rounds: poseidon.hpp's S-box and MDS layers.
template <int NC>
__global__ void __launch_bounds__(256) poseidon_gate_kernel(PoseidonArgs q) {
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const u64 *w = q.wires + L;
    auto wire = [&](unsigned c) { return w[(size_t)c * q.wires_stride]; };
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    unsigned j = 0;
    auto put = [&](u64 term) {  // the next constraint
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(term, q.apow[(size_t)a * q.apow_stride + j], res[a]);
        ++j;
    };
    u64 s[12];
    {
        const u64 swap = wire(24);
        put(gl::mul(swap, gl::sub(swap, 1)));
        u64 d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 lhs = wire(k), rhs = wire(k + 4);
            d[k] = wire(25 + k);
            put(gl::sub(gl::mul(swap, gl::sub(rhs, lhs)), d[k]));
            s[k] = gl::add(lhs, d[k]);
            s[k + 4] = gl::sub(rhs, d[k]);
        }
#pragma unroll
        for (int k = 8; k < 12; ++k) s[k] = wire(k);
    }
    // first full rounds: round 0's S-box inputs are not wires
#pragma unroll 1
    for (unsigned r = 0; r < 4; ++r) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = gl::add_canon(s[k], P2_POSEIDON_ALL_ROUND_CONSTANTS[12 * r + k]);
        if (r != 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const u64 x = wire(29 + 12 * (r - 1) + k);
                put(gl::sub(s[k], x));
                s[k] = x;
            }
        }
        poseidon::sbox_layer(s);
        poseidon::mds_layer(s, nullptr);
    }
    // partial_first_constant_layer, mds_partial_layer_init: result[c] = sum_{r >= 1} state[r] M[r - 1][c - 1], result[0] = state[0]
    {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = gl::add_canon(s[k], P2_POSEIDON_FAST_PARTIAL_FIRST_ROUND_CONSTANT[k]);
        u64 t[12];
#pragma unroll
        for (int c = 1; c < 12; ++c) t[c] = gl::mul(s[1], P2_POSEIDON_FAST_PARTIAL_ROUND_INITIAL_MATRIX[c - 1]);
#pragma unroll 1
        for (unsigned r = 2; r < 12; ++r) {
            u64 sr = s[2];  // s[r] by a rolled rotation of words 2..11: the state stays in registers
#pragma unroll
            for (int k = 2; k < 11; ++k) s[k] = s[k + 1];
            s[11] = sr;
#pragma unroll
            for (int c = 1; c < 12; ++c) t[c] = gl::mul_add(sr, P2_POSEIDON_FAST_PARTIAL_ROUND_INITIAL_MATRIX[11 * (r - 1) + c - 1], t[c]);
        }
#pragma unroll
        for (int c = 1; c < 12; ++c) s[c] = t[c];
    }
#pragma unroll 1
    for (unsigned r = 0; r < 22; ++r) {
        const u64 x = wire(65 + r);
        put(gl::sub(s[0], x));
        u64 s0 = poseidon::sbox7(x);
        if (r != 21) s0 = gl::add_canon(s0, P2_POSEIDON_FAST_PARTIAL_ROUND_CONSTANTS[r]);
        // mds_partial_layer_fast(r): d = s0 (M_00 = circ[0] + diag[0]) + sum_i state[i] w_hat[r][i - 1]; state[i] += s0 v[r][i - 1]
        u64 d = gl::mul(s0, P2_POSEIDON_MDS_CIRC[0] + P2_POSEIDON_MDS_DIAG[0]);
#pragma unroll
        for (int k = 1; k < 12; ++k) {
            d = gl::mul_add(s[k], P2_POSEIDON_FAST_PARTIAL_ROUND_W_HATS[11 * r + k - 1], d);
            s[k] = gl::mul_add(s0, P2_POSEIDON_FAST_PARTIAL_ROUND_VS[11 * r + k - 1], s[k]);
        }
        s[0] = d;
    }
    // second full rounds: round_ctr = 4 + 22 + r
#pragma unroll 1
    for (unsigned r = 0; r < 4; ++r) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const u64 x = wire(87 + 12 * r + k);
            put(gl::sub(gl::add_canon(s[k], P2_POSEIDON_ALL_ROUND_CONSTANTS[12 * (26 + r) + k]), x));
            s[k] = x;
        }
        poseidon::sbox_layer(s);
        poseidon::mds_layer(s, nullptr);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) put(gl::sub(s[k], wire(12 + k)));
    const u64 f = filter(q.gate, q.consts[(size_t)q.gate.selector_index * q.consts_stride + L], q.num_selectors > 1);
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 *o = q.out + (size_t)a * nq + i;
        *o = gl::canon(gl::mul_add(f, res[a], *o));
    }
}

}  // namespace gates
