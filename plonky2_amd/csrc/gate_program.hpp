// gate_program.hpp -- the constraints of user-defined gates in the quotient: evaluate_gate_constraints_base_batch
// (plonky2/src/plonk/vanishing_poly.rs:702-728) for gates that arrive as gate programs (include/p2hot.h, "gate programs"): a gate's
// eval_unfiltered_base_one as a straight-line list of p2hot_air_insn over the gate's frame -- the row's wires, the gate's own
// constants behind the selectors and the lookup selectors (gate.rs:179), the four words of public_inputs_hash.
//
// ONE launch evaluates all program gates of the call.  lane = row L of the committed LDE matrices, i = bitrev(L), column-major reads,
// `out` [nc][Nq] in natural order and added into: the indexing of gates::cheap_gates_kernel.  The loop over the gates' headers, the
// program counter, the opcode and the operand kinds are the same for every lane: headers, instructions, constants, the hash and the
// alpha powers are read through uniform pointers and every branch on them is wave-uniform.  Inside a gate the program counter loop
// is air::eval_kernel's: a temp slot is a runtime index, so slot s of lane t is the LDS word s * blockDim.x + t (a lane only touches
// its own words: no barrier; consecutive lanes read consecutive 8-byte words), sized by the largest num_temps among the programs.
// The j-th CONSTRAINT of a gate is weighted by alpha^j from the table the gate kernels read (reduce_with_powers: every gate starts
// at index 0, vanishing_poly.rs:722-725), the gate's sum by gates::filter, and every lane does one read-modify-write of out[a][i]
// at the end, not one per gate.
#pragma once
#include "../../include/p2hot.h"
#include "air.hpp"
#include "gates.hpp"
#include "gl.hpp"
#include "platform.h"

namespace gateprog {
using gl::u32;
using gl::u64;

constexpr unsigned BLOCK = air::BLOCK;  // the temp file of air.hpp: p2hot_air_max_temps() slots fill 64 KiB of LDS at 256 lanes

// one program gate: the descriptor gates::filter reads (kind unused) and its instructions [insn_first, insn_end) of Args::insns
struct Header {
    p2hot_gate gate;
    u32 insn_first, insn_end, pad;
};
static_assert(sizeof(Header) == 40, "the host lays the headers out in 8-byte words");

struct Args {
    const Header *headers;        // device [num_gates]
    const p2hot_air_insn *insns;  // device: the programs' instructions back to back
    const u64 *constants;         // device, canonical: the programs' constants back to back (CONST indices rebased by the host)
    const u64 *pih;               // device [4]: public_inputs_hash, canonical
    const u64 *wires, *consts;    // LDE matrices, element (col, L) at col * stride + L; consts -> column 0 of constants_sigmas
    size_t wires_stride, consts_stride;
    const u64 *apow;              // device [nc][apow_stride]: alpha_a^j
    u64 *out;                     // device [nc][Nq] natural order, added into
    unsigned log_nq, num_gates, num_selectors, consts_first, apow_stride;  // consts_first = num_selectors + num_lookup_selectors
};

template <int NC>
__global__ void __launch_bounds__(BLOCK) interp_kernel(Args q) {
    P2HOT_DYN_SHARED(u64, temps);
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const u64 *w = q.wires + L, *lc = q.consts + (size_t)q.consts_first * q.consts_stride + L;
    u64 *mine = temps + threadIdx.x;
    const unsigned lanes = blockDim.x;
    auto operand = [&](u32 o) -> u64 {
        const u32 idx = o & air::INDEX_MASK;
        switch (o >> air::KIND_SHIFT) {
            case P2HOT_AIR_LOCAL: return w[(size_t)idx * q.wires_stride];
            case P2HOT_AIR_GATE_CONST: return lc[(size_t)idx * q.consts_stride];
            case P2HOT_AIR_PUBLIC: return q.pih[idx];
            case P2HOT_AIR_CONST: return q.constants[idx];
            default: return mine[(size_t)idx * lanes];
        }
    };
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
    for (unsigned gi = 0; gi < q.num_gates; ++gi) {
        const Header h = q.headers[gi];
        u64 acc[NC];
#pragma unroll
        for (int a = 0; a < NC; ++a) acc[a] = 0;
        const u64 *ap = q.apow;  // alpha_0^j of the next constraint j
        for (unsigned pc = h.insn_first; pc < h.insn_end; ++pc) {
            const p2hot_air_insn in = q.insns[pc];
            const u64 va = operand(in.a);
            if (in.op <= P2HOT_AIR_MUL) {
                const u64 vb = operand(in.b);
                mine[(size_t)in.dst * lanes] = in.op == P2HOT_AIR_ADD ? gl::add(va, vb) : in.op == P2HOT_AIR_SUB ? gl::sub(va, vb) : gl::mul(va, vb);
            } else {
#pragma unroll
                for (int a = 0; a < NC; ++a) acc[a] = gl::mul_add(va, ap[(size_t)a * q.apow_stride], acc[a]);
                ++ap;
            }
        }
        const u64 f = gates::filter(h.gate, q.consts[(size_t)h.gate.selector_index * q.consts_stride + L], q.num_selectors > 1);
#pragma unroll
        for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(f, acc[a], res[a]);
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 *o = q.out + (size_t)a * nq + i;
        *o = gl::canon(gl::add(*o, res[a]));
    }
}

}  // namespace gateprog
