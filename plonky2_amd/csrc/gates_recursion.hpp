// gates_recursion.hpp -- the six gates a recursive verifier circuit adds under standard_recursion_config, next to the eight of
// gates.hpp: PoseidonMds, Reducing, ReducingExtension, RandomAccess, Exponentiation, CosetInterpolation (include/p2hot.h, the second
// enum).  The conventions are gates.hpp's: lane = row L of the committed LDE matrices, i = bitrev(L), column-major reads, every
// challenge in one pass, alpha powers from the wave-uniform table, gates::filter, results ADDED into `out` (canonical).
//   recursion_gates_kernel  Reducing, ReducingExtension, RandomAccess, Exponentiation, CosetInterpolation: a wave-uniform loop over
//                           the descriptors, one switch per descriptor (the shape of cheap_gates_kernel, which stays as it is)
//   mds_gate_kernel         PoseidonMdsGate, one descriptor per launch, one extension component at a time: 12 words of state
// Nothing here indexes a per-lane array dynamically: RandomAccess folds its list through a binary-counter stack whose levels are
// unrolled, CosetInterpolation reads value k from the wire when step k needs it.
#pragma once
#include "gates.hpp"

namespace gates {

constexpr unsigned MAX_SUBGROUP_BITS = 5;   // CosetInterpolation: at most 32 points
constexpr unsigned MAX_ACCESS_BITS = 6;     // RandomAccess: at most 64 list items per copy

__host__ __device__ inline unsigned ra_bits(const p2hot_gate &g) { return g.param1 & 0xFFu; }
__host__ __device__ inline unsigned ra_extra(const p2hot_gate &g) { return g.param1 >> 8; }

// Args plus CosetInterpolation's tables.  two_adic_subgroup(b)[k] = dom[k << (5 - b)], and the barycentric weight of that point
// over the subgroup of order N = 2^b is w_k = 1 / prod_{j != k} (x_k - x_j) = 1 / (N x_k^(N - 1)) = x_k / N
// (field/src/interpolation.rs:53-65 in closed form): ninv[b] = 1 / 2^b.  Both canonical, filled by the host (gates_launch).
struct RecursionArgs : Args {
    u64 dom[1u << MAX_SUBGROUP_BITS];
    u64 ninv[MAX_SUBGROUP_BITS + 1];
};

template <int NC>
__global__ void __launch_bounds__(256) recursion_gates_kernel(RecursionArgs q) {
#include "kbody_recursion_gates.hpp"
}
// proof blockIdx.y of M (gates.hpp, ManyView): the interpolation tables are shared
template <int NC>
struct ManyRecursionView : ManyView<NC, RecursionArgs> {
    const u64 *dom, *ninv;
    __device__ ManyRecursionView(const RecursionArgs &a, const ManyGate *__restrict__ tab) : ManyView<NC, RecursionArgs>(a, tab), dom(a.dom), ninv(a.ninv) {}
};
template <int NC>
__global__ void __launch_bounds__(256) recursion_gates_many_kernel(RecursionArgs shared, const ManyGate *__restrict__ tab) {
    const ManyRecursionView<NC> q(shared, tab);
#include "kbody_recursion_gates.hpp"
}

// PoseidonMdsGate::eval_unfiltered_base_one (gates/poseidon_mds.rs:156-175): input k is the extension element on wires 2k, 2k + 1,
// output k on 24 + 2k, 24 + 2k + 1; constraint pair k = out_k - MDS(inputs)_k.  The MDS entries are base-field constants, so the
// layer acts on each component by itself: poseidon::mds_layer twice, 12 words live.
template <int NC>
__global__ void __launch_bounds__(256) mds_gate_kernel(PoseidonArgs q) {
#include "kbody_mds_gate.hpp"
}
template <int NC>
__global__ void __launch_bounds__(256) mds_gate_many_kernel(PoseidonArgs shared, const ManyGate *__restrict__ tab) {
    const ManyPoseidonView<NC> q(shared, tab);
#include "kbody_mds_gate.hpp"
}

}  // namespace gates
