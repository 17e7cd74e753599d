// poseidon.h -- the round, the permutation, the sponge and the table of the Poseidon calls (poseidon.hip), kept apart from
// the kernels so that a host program can run them (tests/host_check/poseidon_host.cpp, under FE29_CHECK).
//
//   round r of R_F + R_P:   s[j] += c[r][j];   s[j] <- s[j]^alpha for every j in a full round, for j = 0 in a partial one;   s <- M s
//   the first and the last R_F / 2 rounds are full.  This is the plain definition, the one circomlib's poseidon computes.
//
// One thread holds one state of T <= MAX_WIDTH elements.  The S-box and the matrix rows are real loops over a ROTATING state: the loop
// body always works on s[0] (the S-box) or appends to the end of the new state (a row), and 9 T register moves turn the state by one
// place, so no array is indexed by a loop counter and the body exists once: 6 Montgomery and T Shoup products of code for any width,
// instead of the 6 T + T^2 of the unrolled round.
//
// Arithmetic.  Elements are processed as they stand on the wire (x W, W = 2^256) after fe_unpack; fe_mul(a, b) = a b / R, R = 2^261.  A
// chain of alpha - 1 products on x W leaves x^alpha W c^(alpha - 1), c = W / R = 2^-5; the host multiplies 2^(5 (alpha - 1)) into the
// matrix columns that meet S-boxed elements -- all of them in a full round, column 0 in a partial one -- so the table holds TWO matrices
// and the S-box needs no conversion.  Matrix products are fe_mul_shoup<F, true> by plain integers, which keep the wire form; the round
// constants are added as wire residues.
//
// The table, u32 words, read at wave-uniform addresses:
//   [0, T T 18)               the matrix of the full rounds, row-major, entry (i, j) as 9 limbs of w and 9 of floor(w R / p),
//                             w = M[i][j] 2^(5 (alpha - 1)) mod p
//   [T T 18, 2 T T 18)        the matrix of the partial rounds: column 0 as above, the other columns w = M[i][j]
//   [2 T T 18, + rounds T 9)  the round constants, round-major, 9 limbs of the canonical wire residue each
//
// Bounds (contract at the top of fe29.h; BLS12-381 Fr with R / p = 70.6 is the tightest; checked by the host program at every edge):
//   state at entry    limbs <= 5 2^29, value < 15p: a loaded element (tight, < p), the tag, a sponge lane after absorb (below) or what
//                     the last round left
//   + constant        canonical, tight: limbs <= 6 2^29 = 3 2^30, value < 16p                                     "raw"
//   before the S-box  fe_reduce_small_2p (limbs < 2^32, value < 2^9 p)                                            tight, < 2p
//                     a square needs it: (16p)^2 = 256 p^2 exceeds 0.9 R p = 63 p^2 on BLS12-381 (152 p^2 on BN254)
//   S-box             fe_sqr / fe_mul of tight values below 2p: 4 p^2 < 0.9 R p                                   tight, < 2p
//   matrix product    fe_mul_shoup of an S-boxed (tight, < 2p) or a raw element (limbs <= 3 2^30 < 3 2^30 + 64, value < 16p < R):
//                     < (x / R + 2) p                                                                             tight, < 3p
//   row sum           T <= 5 products added limb-wise, no carry: limbs <= 5 (2^29 - 1), value < 15p               the entry class
// so the state is back in its entry class after EVERY round and the number of rounds does not enter.  A raw element of a partial
// round goes into its Shoup products as it stands; only s[0] is reduced there.
//   absorb            a lane that takes a message element is reduced first (fe_reduce_small_2p: tight, < 2p), then the element (tight,
//                     < p) is added limb-wise: limbs < 2^30, value < 3p -- inside the entry class
//   store             store_elem: fe_reduce_small of limbs < 2^32, value < 2^9 p                                  canonical
#pragma once
#include <stdint.h>
#include <string.h>

#include "fe29.h"
#include "poly_sum.h"

namespace panda_hash {

using panda29::Fe;
using panda29::u32;
typedef uint64_t u64;

constexpr int NL = 9;                      // limbs of every supported scalar field
constexpr int MAX_WIDTH = 5;               // PANDA_POSEIDON_MAX_WIDTH
constexpr unsigned MAX_FULL_ROUNDS = 16, MAX_PARTIAL_ROUNDS = 128;
constexpr unsigned PER_WORKGROUP = 256;    // permutations one workgroup covers, one per thread
constexpr unsigned MAX_LOG = 28;           // n, n x len and the leaves of a tree <= 2^28
constexpr unsigned WIRE_SHIFT = 29 * NL - 256; // R / W = 2^5

constexpr u32 entry_words() { return 2 * NL; }
constexpr u32 matrix_words(unsigned t) { return t * t * entry_words(); }
constexpr u32 table_words(unsigned t, unsigned rounds) { return 2 * matrix_words(t) + rounds * t * NL; }

#if defined(FE29_CHECK)
// value < k p, on limbs of any size
template <class Fr>
inline bool value_below(const Fe<Fr> &v, unsigned k)
{
    u64 a[NL + 1], b[NL + 1], ca = 0, cb = 0;
    for (int i = 0; i < NL; i++) {
        ca += v.l[i];
        cb += (u64)k * Fr::P[i];
        a[i] = ca & panda29::LIMB_MASK, b[i] = cb & panda29::LIMB_MASK;
        ca >>= panda29::LIMB_BITS, cb >>= panda29::LIMB_BITS;
    }
    a[NL] = ca, b[NL] = cb;
    for (int i = NL; i >= 0; i--)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
template <class Fr>
inline void check_class(const Fe<Fr> &v, u64 limb_max, unsigned k)
{
    for (int i = 0; i < NL - 1; i++) assert(v.l[i] <= limb_max && "poseidon: limb out of its class");
    assert(value_below(v, k) && "poseidon: value out of its class");
}
#define PANDA_POSEIDON_ENTRY(v) check_class(v, 5ull << 29, 15)
#define PANDA_POSEIDON_RAW(v) check_class(v, 3ull << 30, 16)
#define PANDA_POSEIDON_TIGHT(v, k) check_class(v, (1ull << 29) - 1, k)
#else
#define PANDA_POSEIDON_ENTRY(v)
#define PANDA_POSEIDON_RAW(v)
#define PANDA_POSEIDON_TIGHT(v, k)
#endif

// x (tight, < 2p) <- x^alpha, with c^(alpha - 1) riding along; alpha is the same in every lane.  3, 4, 5 and 5 products for 5, 7, 11, 17.
template <class Fr>
PANDA_HD void sbox(Fe<Fr> &x, u32 alpha)
{
    Fe<Fr> x2, y;
    panda29::fe_sqr(x2, x);
    panda29::fe_sqr(y, x2);                                      // x^4
    if (alpha >= 11) panda29::fe_sqr(y, y);                      // x^8
    if (alpha == 17) panda29::fe_sqr(y, y);                      // x^16
    if (alpha == 7 || alpha == 11) panda29::fe_mul(y, y, x2);    // x^6, x^10
    panda29::fe_mul(x, y, x);
    PANDA_POSEIDON_TIGHT(x, 2);
}

// One round on a state in the entry class; leaves it in the entry class.  rc: the round's T constants; mat: the matrix of this kind of
// round.  `full` and alpha are the same in every lane.
template <class Fr, int T>
PANDA_HD void apply_round(Fe<Fr> (&s)[T], const u32 *rc, const u32 *mat, bool full, u32 alpha)
{
    static_assert(Fr::N == NL && T >= 2 && T <= MAX_WIDTH, "nine-limb fields, widths 2 .. 5");
#pragma unroll
    for (int j = 0; j < T; j++) {
        PANDA_POSEIDON_ENTRY(s[j]);
#pragma unroll
        for (int i = 0; i < NL; i++) s[j].l[i] += rc[j * NL + i];
        PANDA_POSEIDON_RAW(s[j]);
    }
    const int boxes = full ? T : 1;
#pragma unroll 1
    for (int k = 0; k < boxes; k++) {
        Fe<Fr> x = s[0];
        panda29::fe_reduce_small_2p(x);
        PANDA_POSEIDON_TIGHT(x, 2);
        sbox(x, alpha);
        if (full) { // turn the state: after T turns every element is back in its place
#pragma unroll
            for (int j = 0; j + 1 < T; j++) s[j] = s[j + 1];
            s[T - 1] = x;
        } else
            s[0] = x;
    }
    Fe<Fr> n[T];
#pragma unroll
    for (int j = 0; j < T; j++) panda29::fe_zero(n[j]);
#pragma unroll 1
    for (int i = 0; i < T; i++) {
        const u32 *row = mat + (u32)i * T * entry_words();
        Fe<Fr> acc;
        panda29::fe_mul_shoup<Fr, true>(acc, s[0], row, row + NL);
        PANDA_POSEIDON_TIGHT(acc, 3);
#pragma unroll
        for (int j = 1; j < T; j++) {
            Fe<Fr> pr;
            panda29::fe_mul_shoup<Fr, true>(pr, s[j], row + j * entry_words(), row + j * entry_words() + NL);
            PANDA_POSEIDON_TIGHT(pr, 3);
            panda29::fe_add_nr(acc, acc, pr);
        }
#pragma unroll
        for (int j = 0; j + 1 < T; j++) n[j] = n[j + 1];
        n[T - 1] = acc; // row i is at n[T - 1 - (T - 1 - i)] = n[i] after the last turn
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        s[j] = n[j];
        PANDA_POSEIDON_ENTRY(s[j]);
    }
}

// The permutation: entry class in, entry class out.
template <class Fr, int T>
PANDA_HD void permute(Fe<Fr> (&s)[T], const u32 *table, u32 alpha, u32 full_rounds, u32 partial_rounds)
{
    const u32 half = full_rounds / 2, rounds = full_rounds + partial_rounds;
    const u32 *rc = table + 2 * matrix_words(T);
#pragma unroll 1
    for (u32 r = 0; r < rounds; r++) {
        const bool full = r < half || r >= half + partial_rounds;
        apply_round<Fr, T>(s, rc + r * T * NL, table + (full ? 0u : matrix_words(T)), full, alpha);
    }
}

// The sponge over one message of len >= 1 elements: state (tag, 0, ..), every chunk of T - 1 elements added into s[1 ..] and permuted;
// out = s[0] in the entry class.  load(m, j) fetches element j < len (canonical); len is the same in every lane.
template <class Fr, int T, class Load>
PANDA_HD void sponge(Fe<Fr> &out, const Fe<Fr> &tag, u64 len, Load &&load, const u32 *table, u32 alpha, u32 full_rounds, u32 partial_rounds)
{
    Fe<Fr> s[T];
    s[0] = tag;
#pragma unroll
    for (int j = 1; j < T; j++) panda29::fe_zero(s[j]);
#pragma unroll 1
    for (u64 j0 = 0; j0 < len; j0 += T - 1) {
#pragma unroll
        for (int k = 0; k + 1 < T; k++)
            if (j0 + k < len) {
                Fe<Fr> m;
                load(m, j0 + k);
                panda29::fe_reduce_small_2p(s[1 + k]);
                panda29::fe_add_nr(s[1 + k], s[1 + k], m);
            }
        permute<Fr, T>(s, table, alpha, full_rounds, partial_rounds);
    }
    out = s[0];
}

// ------------------------------------------------------------------------------- host side: checks, the table, the plan

// the 256-bit value of a wire element (HOST, any alignment) is below the modulus
template <class Fr>
inline bool wire_valid(const void *wire)
{
    u32 w[8];
    memcpy(w, wire, sizeof(w));
    for (int i = 7; i >= 0; i--)
        if (w[i] != Fr::PW[i]) return w[i] < Fr::PW[i];
    return false;
}

// x -> x^alpha permutes the field: alpha is prime, so it must not divide p - 1
template <class Fr>
inline bool alpha_valid(unsigned alpha)
{
    if (alpha != 5 && alpha != 7 && alpha != 11 && alpha != 17) return false;
    u64 rem = 0;
    for (int i = 7; i >= 0; i--) rem = ((rem << 32) | Fr::PW[i]) % alpha;
    return rem != 1;
}

inline bool shape_valid(unsigned width, unsigned full_rounds, unsigned partial_rounds)
{
    return width >= 2 && width <= (unsigned)MAX_WIDTH && full_rounds >= 2 && full_rounds <= MAX_FULL_ROUNDS && full_rounds % 2 == 0 &&
           partial_rounds <= MAX_PARTIAL_ROUNDS;
}

// every check of a parameter set; round_constants and mds are HOST arrays of wire elements
template <class Fr>
inline bool params_valid(unsigned width, unsigned alpha, unsigned full_rounds, unsigned partial_rounds, const void *round_constants, const void *mds)
{
    if (!shape_valid(width, full_rounds, partial_rounds) || !alpha_valid<Fr>(alpha) || !round_constants || !mds) return false;
    const size_t n_rc = (size_t)(full_rounds + partial_rounds) * width, n_m = (size_t)width * width;
    for (size_t k = 0; k < n_rc; k++)
        if (!wire_valid<Fr>((const char *)round_constants + 32 * k)) return false;
    for (size_t k = 0; k < n_m; k++)
        if (!wire_valid<Fr>((const char *)mds + 32 * k)) return false;
    return true;
}

// table_words(width, rounds) words from a valid parameter set.  The internal form (w R mod p) that fe_shoup_prepare takes is the wire
// residue doubled WIRE_SHIFT times; alpha - 1 further runs of WIRE_SHIFT doublings are the S-box's factor.
template <class Fr>
inline void build_table(u32 *table, unsigned width, unsigned alpha, unsigned full_rounds, unsigned partial_rounds, const void *round_constants, const void *mds)
{
    const unsigned t = width;
    for (unsigned kind = 0; kind < 2; kind++)
        for (unsigned i = 0; i < t; i++)
            for (unsigned j = 0; j < t; j++) {
                u32 w[8];
                memcpy(w, (const char *)mds + 32 * (size_t)(i * t + j), sizeof(w));
                Fe<Fr> v;
                panda29::fe_unpack(v, w);
                const unsigned doublings = (kind == 0 || j == 0) ? WIRE_SHIFT * alpha : WIRE_SHIFT;
                for (unsigned d = 0; d < doublings; d++) panda_poly::add_canon(v, v, v);
                panda29::FeTw<Fr> tw;
                panda29::fe_shoup_prepare(tw, v);
                u32 *dst = table + kind * matrix_words(t) + (i * t + j) * entry_words();
                memcpy(dst, tw.w, NL * 4);
                memcpy(dst + NL, tw.q, NL * 4);
            }
    u32 *rc = table + 2 * matrix_words(t);
    for (size_t k = 0; k < (size_t)(full_rounds + partial_rounds) * t; k++) {
        u32 w[8];
        memcpy(w, (const char *)round_constants + 32 * k, sizeof(w));
        Fe<Fr> v;
        panda29::fe_unpack(v, w);
        memcpy(rc + k * NL, v.l, NL * 4);
    }
}

// The tree of a^height leaves, a = width - 1: level l = 1 .. height has a^(height - l) nodes at offset level_offset[l - 1] (elements) of the
// node buffer; the last top_levels levels, those of at most PER_WORKGROUP nodes, are one launch.
struct TreePlan {
    u64 leaves, nodes;
    unsigned top_levels, launches;
};
inline bool tree_plan(TreePlan &plan, unsigned width, unsigned height, u64 *level_offset)
{
    if (width < 3 || width > (unsigned)MAX_WIDTH || height < 1 || height > MAX_LOG) return false;
    const u64 a = width - 1;
    u64 leaves = 1;
    for (unsigned l = 0; l < height; l++) {
        leaves *= a;
        if (leaves > ((u64)1 << MAX_LOG)) return false;
    }
    plan.leaves = leaves, plan.nodes = 0, plan.top_levels = 0;
    u64 count = leaves;
    for (unsigned l = 1; l <= height; l++) {
        count /= a;
        if (level_offset) level_offset[l - 1] = plan.nodes;
        plan.nodes += count;
        if (count <= PER_WORKGROUP) plan.top_levels++;
    }
    plan.launches = height - plan.top_levels + 1;
    return true;
}

} // namespace panda_hash
