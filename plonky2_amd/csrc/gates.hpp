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
#include "kbody_cheap_gates.hpp"
}

// ------------------------------------------------------------------ M witnesses of one circuit (p2hot_quotient_polys_gates_many)
// The gate set, the constants and the selectors are shared; the wires, the alpha powers, the public-inputs hash and the output
// differ per proof.  An M-form kernel takes the single-proof arguments plus a table with one entry per proof, runs grid row
// blockIdx.y for proof y and reads the per-proof fields from table[y] (wave-uniform index, read-only table: scalar loads).  The
// views below carry the member names of the argument structs, so both forms #include one body (the kbody_*.hpp fragments; the
// single-proof kernels keep their tokens and with them their code); the alpha powers and the output of proof y lie
// NC * apow_stride / NC * Nq words behind proof 0's.
// (A pointer read from the table would have no known address space and cost flat loads: the table holds the proof's OFFSET from
// proof 0's matrix, which is a kernel argument.  The views bind the shared fields by reference, so they stay kernel-argument loads;
// the 32-bit stride keeps recursion_gates_many_kernel<4> within the scalar registers -- the host refuses a longer one.)
struct ManyGate {
    ptrdiff_t wires_off;    // this proof's wires LDE matrix, in words from proof 0's
    unsigned wires_stride;  // words between its columns
    unsigned pad_;
    const u64 *wires;       // the same matrix and stride as a pointer and 64 bits, for the one-descriptor kernels (ManyPoseidonView)
    size_t wires_stride64;
    u64 pih[4];             // public_inputs_hash (canonical)
};
template <int NC, class A>
struct ManyView {
    const u64 *wires;
    const u64 *const &consts;
    const unsigned &wires_stride;
    const size_t &consts_stride;
    const u64 *apow;
    u64 *out;
    const unsigned &log_nq, &num_gates, &num_selectors, &consts_first, &apow_stride;
    const u64 *pih;
    const p2hot_gate *gates;
    __device__ ManyView(const A &a, const ManyGate *__restrict__ tab)
        : wires(a.wires + tab[blockIdx.y].wires_off), consts(a.consts), wires_stride(tab[blockIdx.y].wires_stride), consts_stride(a.consts_stride),
          apow(a.apow + (size_t)blockIdx.y * NC * a.apow_stride), out(a.out + (((size_t)blockIdx.y * NC) << a.log_nq)), log_nq(a.log_nq),
          num_gates(a.num_gates), num_selectors(a.num_selectors), consts_first(a.consts_first), apow_stride(a.apow_stride),
          pih(tab[blockIdx.y].pih), gates(a.gates) {}
};
template <int NC>
__global__ void __launch_bounds__(256) cheap_gates_many_kernel(Args shared, const ManyGate *__restrict__ tab) {
    const ManyView<NC, Args> q(shared, tab);
#include "kbody_cheap_gates.hpp"
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
#include "kbody_poseidon_gate.hpp"
}
// PoseidonArgs for proof blockIdx.y of M (the one-descriptor kernels: PoseidonGate here, PoseidonMdsGate in gates_recursion.hpp)
// (poseidon_gate_kernel fills the scalar registers -- 104 of them, most as column bases of its global loads -- and every form of
// the per-proof fields that keeps those loads global spills a few.  Here the matrix comes as the table's POINTER: the loads through
// it are flat loads, which take their whole address from vector registers, and nothing is spilled; tests/test_many_middle_codeobj.py
// and tests/test_gates_codeobj.py hold that.)
template <int NC>
struct ManyPoseidonView {
    const u64 *wires, *consts;
    size_t wires_stride, consts_stride;
    const u64 *apow;
    u64 *out;
    unsigned log_nq, num_selectors, apow_stride;
    const p2hot_gate &gate;
    __device__ ManyPoseidonView(const PoseidonArgs &a, const ManyGate *__restrict__ tab)
        : wires(tab[blockIdx.y].wires), consts(a.consts), wires_stride(tab[blockIdx.y].wires_stride64), consts_stride(a.consts_stride),
          apow(a.apow + (size_t)blockIdx.y * NC * a.apow_stride), out(a.out + (((size_t)blockIdx.y * NC) << a.log_nq)), log_nq(a.log_nq),
          num_selectors(a.num_selectors), apow_stride(a.apow_stride), gate(a.gate) {}
};
template <int NC>
__global__ void __launch_bounds__(256) poseidon_gate_many_kernel(PoseidonArgs shared, const ManyGate *__restrict__ tab) {
    const ManyPoseidonView<NC> q(shared, tab);
#include "kbody_poseidon_gate.hpp"
}

}  // namespace gates
