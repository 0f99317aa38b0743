// Kernel body fragment: #included inside poseidon_gate_kernel and inside its M-proof form poseidon_gate_many_kernel (plonk.hpp / gates.hpp /
// gates_recursion.hpp), which bind the same names to per-proof values.  One text for both, and the single-proof kernel's tokens --
// hence its code -- stay what they were.  No include guard on purpose.
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
