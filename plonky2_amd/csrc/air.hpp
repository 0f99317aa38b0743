// air.hpp -- a STARK's own constraints (Stark::eval_packed_generic, user code in the reference) on the quotient coset of
// compute_quotient_polys (starky/src/prover.rs:488-671), from a constraint program: a straight-line list of p2hot_air_insn over the
// evaluation frame (include/p2hot.h, "constraint program").  eval_kernel interprets the program at every point of the coset and
// leaves ConstraintConsumer::accumulators() (starky/src/constraint_consumer.rs:14-88) in the [nc][Nq] buffer stark::aux_terms_kernel
// reads as its `accs`.
//
// lane = row L of the LDE matrix, indexed as stark::aux_terms_kernel does (i = bitrev(L), next row bitrev(i + 2^qbits mod Nq), x from
// the root table).  The program counter, the opcode and the operand kinds are the same for every lane: the instruction, the
// constants, the public inputs and the alphas are read through uniform pointers and every branch on them is wave-uniform.  A temp
// slot is a runtime index, so the temp file is not a per-lane array (it would live in scratch): slot s of lane t is the LDS word
// s * blockDim.x + t -- a lane only ever touches its own words (no barrier), and consecutive lanes read consecutive 8-byte words.
// LOCAL / NEXT operands load the LDE matrix at col * stride + L / L_next directly; the accumulators are NC register values.
#pragma once
#include "../../include/p2hot.h"
#include "gl.hpp"
#include "ntt.hpp"
#include "platform.h"

namespace air {
using gl::u32;
using gl::u64;

constexpr unsigned BLOCK = 256;
// a workgroup may ask for 64 KiB of LDS without opting in to more: 65536 / (BLOCK lanes * 8 bytes) slots.  (At the cap two
// workgroups share a CU's 160 KiB; a program of four slots leaves the CU to its wave limit.)
constexpr unsigned MAX_TEMPS = (64u << 10) / (BLOCK * 8);
constexpr u32 KIND_SHIFT = 29, INDEX_MASK = (1u << KIND_SHIFT) - 1;

struct Args {
    const p2hot_air_insn *insns;  // device [num_insns]
    const u64 *constants, *publics, *alphas;  // device, canonical: [num_constants], [num_publics], [nc]
    const u64 *trace;             // LDE matrix, element (col, L) at col * stride + L
    size_t stride;
    const u64 *zh;                // device [2 << qbits]: Z_H(g w^i) for i mod 2^qbits, then their inverses (stark::TermArgs::zh)
    const u64 *inv_nx1;           // device [Nq], committed order: 1 / (n (x_L - 1))  (plonk::quot_inv_kernel)
    u64 *out;                     // device [nc][Nq] natural order
    unsigned num_insns, log_nq, qbits;
    u64 last;                     // w_n^-1
    ntt::RootTable roots;
};

template <int NC>
__global__ void __launch_bounds__(BLOCK) eval_kernel(Args q) {
    P2HOT_DYN_SHARED(u64, temps);
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const size_t i_next = (i + ((size_t)1 << q.qbits)) & (nq - 1);
    const size_t L_next = q.log_nq ? (size_t)(__brevll((unsigned long long)i_next) >> (64 - q.log_nq)) : 0;
    const u64 x = gl::mul(gl::COSET_SHIFT, q.log_nq ? ntt::root_pow(q.roots, (u32)(i << (32 - q.log_nq))) : (u64)1);
    const size_t r = i & (((size_t)1 << q.qbits) - 1);
    const u64 l_first = gl::mul(q.zh[r], q.inv_nx1[L]), l_last = gl::mul(q.zh[r], q.inv_nx1[L_next]), z_last = gl::sub(x, q.last);
    u64 *mine = temps + threadIdx.x;
    const unsigned lanes = blockDim.x;
    u64 alpha[NC], acc[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) alpha[a] = q.alphas[a], acc[a] = 0;
    auto operand = [&](u32 o) -> u64 {
        const u32 idx = o & INDEX_MASK;
        switch (o >> KIND_SHIFT) {
            case P2HOT_AIR_LOCAL: return q.trace[(size_t)idx * q.stride + L];
            case P2HOT_AIR_NEXT: return q.trace[(size_t)idx * q.stride + L_next];
            case P2HOT_AIR_PUBLIC: return q.publics[idx];
            case P2HOT_AIR_CONST: return q.constants[idx];
            default: return mine[(size_t)idx * lanes];
        }
    };
    for (unsigned pc = 0; pc < q.num_insns; ++pc) {
        const p2hot_air_insn in = q.insns[pc];
        const u64 va = operand(in.a);
        if (in.op <= P2HOT_AIR_MUL) {
            const u64 vb = operand(in.b);
            mine[(size_t)in.dst * lanes] = in.op == P2HOT_AIR_ADD ? gl::add(va, vb) : in.op == P2HOT_AIR_SUB ? gl::sub(va, vb) : gl::mul(va, vb);
        } else {
            const u64 c = in.op == P2HOT_AIR_CONSTRAINT              ? va
                          : in.op == P2HOT_AIR_CONSTRAINT_TRANSITION ? gl::mul(va, z_last)
                          : in.op == P2HOT_AIR_CONSTRAINT_FIRST_ROW  ? gl::mul(va, l_first)
                                                                     : gl::mul(va, l_last);
#pragma unroll
            for (int a = 0; a < NC; ++a) acc[a] = gl::mul_add(acc[a], alpha[a], c);
        }
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) q.out[(size_t)a * nq + i] = gl::canon(acc[a]);
}

}  // namespace air
