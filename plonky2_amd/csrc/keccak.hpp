// keccak.hpp -- Keccak-256 leaf sponge, Merkle levels and a batched byte-message hash, one permutation per lane.
//
// KeccakHash<N> (plonky2/src/hash/keccak.rs:104-127): Keccak-256 (keccak_hash::keccak: the original padding, domain byte 0x01)
// of the canonical little-endian bytes of the elements (util/serialization/mod.rs:1254-1260), truncated to N bytes (1..32).
// Digests live in the 32-byte slots the Poseidon trees use (merkle.hpp, node_slot): bytes 0..N of the slot are the digest and
// bytes N..32 are zero, so every reader of the tree (paths, caps, the reference digest layout) carries Keccak trees unchanged.
//
// Keccak-f[1600] keeps its 25 lanes in VGPR pairs (50 VGPRs).  Every step is 32-bit: theta's 5-way column parity is two
// v_bitop3_b32 per half (xor3 = truth table 0x96), the theta update one more, chi one per half (a ^ (~b & c) = 0xD2) and a
// 64-bit rotate two v_alignbit_b32.  The truth table of v_bitop3_b32 is indexed by (src0 << 2) | (src1 << 1) | src2, i.e.
// src0 / src1 / src2 stand for 0xF0 / 0xCC / 0xAA.
#pragma once
#include "gl.hpp"
#include "merkle.hpp"

namespace keccak {
using gl::u32;
using gl::u64;

#ifdef P2HOT_EMU
// plain-C stand-ins for the emulator build: a generic truth-table evaluator and the 64-bit funnel shift
template <unsigned IMM>
static inline u32 bitop3(u32 a, u32 b, u32 c) {
    if (IMM == 0x96) return a ^ b ^ c;     // the two tables Keccak-f uses, word-wide (the grind emulates 2^14 candidates a launch)
    if (IMM == 0xD2) return a ^ (~b & c);
    u32 r = 0;
    for (unsigned i = 0; i < 32; ++i) {
        const unsigned idx = (((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u);
        r |= ((IMM >> idx) & 1u) << i;
    }
    return r;
}
static inline u32 alignbit(u32 hi, u32 lo, u32 s) { return (u32)((((u64)hi << 32) | lo) >> (s & 31)); }
#else
template <unsigned IMM>
__device__ __forceinline__ u32 bitop3(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, IMM); }
__device__ __forceinline__ u32 alignbit(u32 hi, u32 lo, u32 s) { return __builtin_amdgcn_alignbit(hi, lo, s); }
#endif

__device__ __forceinline__ u32 lo(u64 x) { return (u32)x; }
__device__ __forceinline__ u32 hi(u64 x) { return (u32)(x >> 32); }
__device__ __forceinline__ u64 join(u32 h, u32 l) { return ((u64)h << 32) | l; }

template <unsigned IMM>
__device__ __forceinline__ u64 bitop3_64(u64 a, u64 b, u64 c) {
    return join(bitop3<IMM>(hi(a), hi(b), hi(c)), bitop3<IMM>(lo(a), lo(b), lo(c)));
}
__device__ __forceinline__ u64 xor3(u64 a, u64 b, u64 c) { return bitop3_64<0x96>(a, b, c); }
__device__ __forceinline__ u64 chi(u64 a, u64 b, u64 c) { return bitop3_64<0xD2>(a, b, c); }  // a ^ (~b & c)

// rotate left by a compile-time constant n (after unrolling): two funnel shifts, or a swap of the halves
__device__ __forceinline__ u64 rotl(u64 x, unsigned n) {
    if (n == 0) return x;
    if (n == 32) return join(lo(x), hi(x));
    if (n < 32) return join(alignbit(hi(x), lo(x), 32 - n), alignbit(lo(x), hi(x), 32 - n));
    return join(alignbit(lo(x), hi(x), 64 - n), alignbit(hi(x), lo(x), 64 - n));
}

// iota round constants (FIPS 202, Algorithm 5); the round index is wave-uniform -> scalar loads
__constant__ u64 RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
    0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
    0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
    0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// Keccak-f[1600] on lanes s[x + 5y] (FIPS 202 section 3.2)
__device__ __forceinline__ void keccak_f(u64 s[25]) {
#pragma unroll 1
    for (int round = 0; round < 24; ++round) {
        u64 c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = xor3(xor3(s[x], s[x + 5], s[x + 10]), s[x + 15], s[x + 20]);
#pragma unroll
        for (int x = 0; x < 5; ++x) {  // theta: A[x,y] ^= C[x-1] ^ rot(C[x+1], 1)
            const u64 cm = c[(x + 4) % 5], cp = rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) s[x + 5 * y] = xor3(s[x + 5 * y], cm, cp);
        }
        // rho + pi: B[y, 2x + 3y] = rot(A[x, y], r[x, y])
#define P2_KECCAK_RP(x, y, r) b[(y) + 5 * ((2 * (x) + 3 * (y)) % 5)] = rotl(s[(x) + 5 * (y)], r)
        P2_KECCAK_RP(0, 0, 0); P2_KECCAK_RP(1, 0, 1); P2_KECCAK_RP(2, 0, 62); P2_KECCAK_RP(3, 0, 28); P2_KECCAK_RP(4, 0, 27);
        P2_KECCAK_RP(0, 1, 36); P2_KECCAK_RP(1, 1, 44); P2_KECCAK_RP(2, 1, 6); P2_KECCAK_RP(3, 1, 55); P2_KECCAK_RP(4, 1, 20);
        P2_KECCAK_RP(0, 2, 3); P2_KECCAK_RP(1, 2, 10); P2_KECCAK_RP(2, 2, 43); P2_KECCAK_RP(3, 2, 25); P2_KECCAK_RP(4, 2, 39);
        P2_KECCAK_RP(0, 3, 41); P2_KECCAK_RP(1, 3, 45); P2_KECCAK_RP(2, 3, 15); P2_KECCAK_RP(3, 3, 21); P2_KECCAK_RP(4, 3, 8);
        P2_KECCAK_RP(0, 4, 18); P2_KECCAK_RP(1, 4, 2); P2_KECCAK_RP(2, 4, 61); P2_KECCAK_RP(3, 4, 56); P2_KECCAK_RP(4, 4, 14);
#undef P2_KECCAK_RP
#pragma unroll
        for (int y = 0; y < 5; ++y)
#pragma unroll
            for (int x = 0; x < 5; ++x) s[x + 5 * y] = chi(b[x + 5 * y], b[(x + 1) % 5 + 5 * y], b[(x + 2) % 5 + 5 * y]);
        s[0] ^= RC[round];
    }
}

constexpr unsigned RATE_WORDS = 17;  // Keccak-256: 1088-bit rate

// the last block of a message of whole words: `rem` (0..16) words are absorbed, the domain byte goes into word rem and 0x80
// into the top byte of word 16 (pad10*1).  rem is uniform or not; the state is only ever indexed by constants.
__device__ __forceinline__ void pad_words(u64 s[25], unsigned rem, u64 domain) {
#pragma unroll
    for (unsigned i = 0; i < RATE_WORDS; ++i)
        if (i == rem) s[i] ^= domain;
    s[RATE_WORDS - 1] ^= 0x80ull << 56;
}

// the slot of an N-byte digest: bytes 0..N of the state, the rest zero
__device__ __forceinline__ void store_digest(u64 *dst, const u64 s[25], unsigned N) {
#pragma unroll
    for (unsigned i = 0; i < 4; ++i) {
        const unsigned nb = N > 8 * i ? N - 8 * i : 0;  // bytes of word i that belong to the digest
        dst[i] = nb >= 8 ? s[i] : nb ? s[i] & ((1ull << (8 * nb)) - 1) : 0;
    }
}

// KeccakPermutation::permute (hash/keccak.rs:63-94) on the 12 words of a sponge state, in place: h_1 = Keccak-256 of the 96
// canonical little-endian bytes (one block: 12 words, the domain byte in word 12), h_{k+1} = Keccak-256(h_k) (32 bytes, one
// block); the hashes are read as 4 little-endian words each and every word >= p is DROPPED (rejection sampling, not reduction:
// about one word in 2^32) until 12 words are kept -- three hashes, or more after a rejection.  The kept-word count differs
// between lanes only then, so st[] is written by compare-and-select on constant indices: the state stays in registers.
__device__ __forceinline__ void keccak_permutation(u64 st[12]) {
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = i < 12 ? gl::canon(st[i]) : 0;
    pad_words(s, 12, 0x01);
    unsigned kept = 0;
    do {
        keccak_f(s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u64 w = s[i];
            const bool keep = w < gl::P && kept < 12;
#pragma unroll
            for (unsigned j = 0; j < 12; ++j)
                if (keep && j == kept) st[j] = w;
            kept += keep ? 1u : 0u;
        }
        // the next message is this hash: words 0..3 stay, the domain byte follows them
#pragma unroll
        for (int i = 4; i < 25; ++i) s[i] = 0;
        pad_words(s, 4, 0x01);
    } while (kept < 12);
}

// hash_or_noop of every leaf (plonk/config.rs:63-74) for KeccakHash<N>: a leaf of 8W <= N bytes is its canonical bytes
// zero-padded, any other is Keccak-256 of its 8W canonical bytes truncated to N; digest -> level-0 slot
template <class Reader>
__device__ __forceinline__ void leaf_digest(const Reader &rd, unsigned W, size_t L, unsigned N, u64 *dst) {
    if (8 * W <= N) {  // no hash (W <= 4)
#pragma unroll
        for (unsigned i = 0; i < 4; ++i) dst[i] = i < W ? gl::canon(rd(L, i)) : 0;
        return;
    }
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = 0;
    unsigned off = 0;
    for (; off + RATE_WORDS <= W; off += RATE_WORDS) {
#pragma unroll
        for (unsigned i = 0; i < RATE_WORDS; ++i) s[i] ^= gl::canon(rd(L, off + i));
        keccak_f(s);
    }
    const unsigned rem = W - off;
#pragma unroll
    for (unsigned i = 0; i < RATE_WORDS - 1; ++i)
        if (i < rem) s[i] ^= gl::canon(rd(L, off + i));
    pad_words(s, rem, 0x01);
    keccak_f(s);
    store_digest(dst, s, N);
}

template <class Reader>
__global__ void __launch_bounds__(256) keccak_leaves_kernel(Reader rd, unsigned W, size_t leaf_offset, size_t leaf_count,
                                                           unsigned h, unsigned N, u64 *digests, u64 *cap) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= leaf_count) return;
    const size_t L = leaf_offset + t;
    leaf_digest(rd, W, L, N, merkle::node_slot(digests, cap, h, 0, L));
}

// one tree level: node j = Keccak-256(left[0..N] || right[0..N]) truncated (keccak.rs:118-127, merkle_tree.rs:108-112).  The
// 2N-byte message is one block; the right digest starts at byte N: a word shift by N / 8 and a funnel shift by N % 8 bytes.
__global__ void __launch_bounds__(256) keccak_level_kernel(u64 *digests, u64 *cap, unsigned h, unsigned level, size_t n_nodes,
                                                          unsigned N) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_nodes) return;
    const u64 *ch = merkle::node_slot(digests, cap, h, level - 1, 2 * j);  // 8 contiguous words [left, right]
    u64 r[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = ch[4 + i];
#pragma unroll
    for (int i = 4; i < 8; ++i) r[i] = 0;
    const unsigned q = N >> 3, sh = 8 * (N & 7);  // N is uniform: so are the branches
    if (q & 4) {
#pragma unroll
        for (int i = 7; i >= 0; --i) r[i] = i >= 4 ? r[i - 4] : 0;
    }
    if (q & 2) {
#pragma unroll
        for (int i = 7; i >= 0; --i) r[i] = i >= 2 ? r[i - 2] : 0;
    }
    if (q & 1) {
#pragma unroll
        for (int i = 7; i >= 0; --i) r[i] = i >= 1 ? r[i - 1] : 0;
    }
    if (sh) {
#pragma unroll
        for (int i = 7; i >= 0; --i) r[i] = (r[i] << sh) | (i ? r[i - 1] >> (64 - sh) : 0);
    }
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = ch[i] | r[i];  // left bytes N..32 are zero in its slot
#pragma unroll
    for (int i = 4; i < 8; ++i) s[i] = r[i];
#pragma unroll
    for (int i = 8; i < 25; ++i) s[i] = 0;
    const unsigned pw = (2 * N) >> 3;  // the domain byte follows the message: byte 2N
    const u64 pad = 0x01ull << (8 * ((2 * N) & 7));
#pragma unroll
    for (unsigned i = 0; i <= 8; ++i)
        if (i == pw) s[i] ^= pad;
    s[RATE_WORDS - 1] ^= 0x80ull << 56;
    keccak_f(s);
    store_digest(merkle::node_slot(digests, cap, h, level, j), s, N);
}

// `count` messages of msg_bytes bytes each, back to back (message t at msgs + t * msg_bytes, any alignment): the sponge with
// domain byte `domain` (0x01 Keccak-256, 0x06 SHA3-256) -> out[t][0..4] = the 32-byte output
__global__ void __launch_bounds__(256) keccak_bytes_kernel(const unsigned char *msgs, size_t msg_bytes, size_t count, u64 domain,
                                                          u64 *out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const unsigned char *m = msgs + t * msg_bytes;
    u64 s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = 0;
    const size_t blocks = msg_bytes / (8 * RATE_WORDS) + 1;
    for (size_t b = 0; b < blocks; ++b) {
        const size_t base = b * 8 * RATE_WORDS;
#pragma unroll
        for (unsigned i = 0; i < RATE_WORDS; ++i) {
            u64 w = 0;
#pragma unroll 1
            for (unsigned k = 0; k < 8; ++k) {  // (a test primitive: byte loads, one at a time, keep the state the only large array)
                const size_t p = base + 8 * i + k;
                const u64 byte = p < msg_bytes ? m[p] : p == msg_bytes ? domain : 0;
                w |= byte << (8 * k);
            }
            s[i] ^= w;
        }
        if (b + 1 == blocks) s[RATE_WORDS - 1] ^= 0x80ull << 56;
        keccak_f(s);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out[4 * t + i] = s[i];
}

}  // namespace keccak
