// Kernel body fragment: #included inside cheap_gates_kernel and inside its M-proof form cheap_gates_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
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
