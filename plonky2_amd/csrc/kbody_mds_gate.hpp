// Kernel body fragment: #included inside mds_gate_kernel and inside its M-proof form mds_gate_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
    const size_t L = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nq = (size_t)1 << q.log_nq;
    if (L >= nq) return;
    const size_t i = q.log_nq ? (size_t)(__brevll((unsigned long long)L) >> (64 - q.log_nq)) : 0;
    const u64 *w = q.wires + L;
    u64 res[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) res[a] = 0;
#pragma unroll 1
    for (unsigned comp = 0; comp < 2; ++comp) {
        u64 s[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = w[(size_t)(2 * k + comp) * q.wires_stride];
        poseidon::mds_layer(s, nullptr);
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const u64 term = gl::sub(w[(size_t)(24 + 2 * k + comp) * q.wires_stride], s[k]);
#pragma unroll
            for (int a = 0; a < NC; ++a) res[a] = gl::mul_add(term, q.apow[(size_t)a * q.apow_stride + 2 * k + comp], res[a]);
        }
    }
    const u64 f = filter(q.gate, q.consts[(size_t)q.gate.selector_index * q.consts_stride + L], q.num_selectors > 1);
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        u64 *o = q.out + (size_t)a * nq + i;
        *o = gl::canon(gl::mul_add(f, res[a], *o));
    }
