// poly_terms.h -- the program and the per-element routine of panda_poly_sum_of_products (poly_terms.hip), kept apart from
// the kernel so that a host program can run both (tests/host_check/poly_terms_host.cpp, under FE29_CHECK).
//
//   out[p][i] = s(p, i) * sum_t coeff_t * prod_{f < degree_t} column[c_tf][p][(i + r_tf) mod n]
//
// Arithmetic.  fe_mul(a, b) = a b / R (R = 2^261); a wire residue x W (W = 2^256) is multiplied as it stands after fe_unpack (5.4).  The
// product of a term's d factors, d - 1 fe_mul, is (prod x) W^d / R^(d-1); one more division by R comes with the coefficient's product, so
// the term carries c^d for c = W / R and the host multiplies c^-d into its coefficient: k' = k c^-d is what the program holds, and
// prod * k' / R = k (prod x) on the wire form.  The accumulator is then a plain sum of wire residues, acc <- (acc * ONE + prod * k') / R
// with ONE = R mod p, and the scale's product acc * s' / R wants s' = s c^-1.  A term of degree 0 takes ONE for its product.
//
// Bounds (contract at the top of fe29.h; worst case 64 terms, every operand p - 1, BLS12-381 Fr with R / p = 70.6 the tightest):
//   loaded element    fe_unpack of a canonical residue                  tight, < p
//   running product   fe_mul(prod < 2p, x < p): 2 p^2 < 0.9 R p         tight, < 2p  (exactly < 2 p^2 / R + p)
//   k', s', ONE       reduced on the host / a constant                  tight, < p
//   first term        fe_mul(prod < 2p, k' < p)                         tight, < 2p
//   every other term  fe_mul_add(acc < 2p, ONE < p, prod < 2p, k' < p): 2 p^2 + 2 p^2 = 4 p^2 < 0.9 R p (R / p > 4.5), 27 column terms
//                     of < 2^58 in a u64                                tight, < 2p  (exactly < 4 p^2 / R + p)
//   scale             fe_mul(acc < 2p, s' < p)                          tight, < 2p
//   store             fe_reduce_small (limbs < 2^32, value < 2^9 p)     canonical
// The accumulator is back to tight and < 2p after EVERY term, so the number of terms does not enter; nothing is added or subtracted
// outside a column accumulator, so no loose or raw limb class appears.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fe29.h"

#define PANDA_SOP_PROGRAM_COLUMNS 32
#define PANDA_SOP_PROGRAM_TERMS 64
#define PANDA_SOP_PROGRAM_FACTORS 256
#define PANDA_SOP_PROGRAM_SCALES 16

namespace panda_sop {

using panda29::Fe;
using panda29::u32;
typedef uint64_t u64;

constexpr int NL = 9; // limbs of every supported scalar field
enum ScaleMode : u32 { SCALE_NONE = 0, SCALE_PER_VECTOR = 1, SCALE_CYCLIC = 2 };

// What the kernel reads, at wave-uniform addresses (but for the scales of SCALE_CYCLIC): 5456 bytes in device memory.
struct Program {
    u32 n_terms, n_scales, scale_mode, reserved;
    u64 column[PANDA_SOP_PROGRAM_COLUMNS];       // device addresses of the columns
    u32 term_end[PANDA_SOP_PROGRAM_TERMS];       // term t owns the factors [term_end[t - 1], term_end[t])
    u32 factor[PANDA_SOP_PROGRAM_FACTORS][2];    // {column, rotation reduced to [0, n)}
    u32 coeff[PANDA_SOP_PROGRAM_TERMS][NL];      // k' = k c^-degree, canonical limbs
    u32 scale[PANDA_SOP_PROGRAM_SCALES][NL];     // s' = s c^-1, canonical limbs
};

#if defined(FE29_CHECK)
// tight limbs and a value below 2p: the state every step of the routine leaves
template <class Fr>
inline void check_tight_2p(const Fe<Fr> &v)
{
    u32 twop[NL], carry = 0;
    for (int i = 0; i < NL; i++) {
        const u32 t = 2 * Fr::P[i] + carry;
        twop[i] = i < NL - 1 ? t & panda29::LIMB_MASK : t;
        carry = i < NL - 1 ? t >> panda29::LIMB_BITS : 0;
    }
    for (int i = 0; i < NL - 1; i++) assert(v.l[i] < (1u << 29) && "sum of products: limb not tight");
    bool below = false;
    for (int i = NL - 1; i >= 0; i--)
        if (v.l[i] != twop[i]) {
            below = v.l[i] < twop[i];
            break;
        }
    assert(below && "sum of products: value not below 2p");
}
#define PANDA_SOP_CHECK(v) check_tight_2p(v)
#else
#define PANDA_SOP_CHECK(v)
#endif

// E elements of vector p at the indices i[e] < n: r[e] = s(p, i[e]) * sum of the program's terms.  load(v, column, index) fetches one
// element of vector p.  The term and factor loops depend on the program alone; the state per element is the accumulator, the running
// product and one loaded element, every array indexed by unrolled constants only.
template <class Fr, int E, class Load>
PANDA_HD void evaluate(Fe<Fr> (&r)[E], const Program &P, u32 p, const u32 (&i)[E], u32 n, Load &&load)
{
    static_assert(Fr::N == NL, "the program holds nine-limb constants");
    Fe<Fr> one, prod[E], x[E];
    panda29::fe_one(one);
    const u32 n_terms = P.n_terms;
    auto fetch = [&](u32 f) { // x[e] <- the factor's column at i[e] + rotation, wrapped inside the vector
        const u32 column = P.factor[f][0], rot = P.factor[f][1];
#pragma unroll
        for (int e = 0; e < E; e++) {
            u32 j = i[e] + rot;
            j -= j >= n ? n : 0u;
            load(x[e], column, j);
        }
    };
    u32 f = 0;
    for (u32 t = 0; t < n_terms; t++) {
        const u32 end = P.term_end[t];
        if (f == end) {
#pragma unroll
            for (int e = 0; e < E; e++) prod[e] = one;
        } else {
            fetch(f++);
#pragma unroll
            for (int e = 0; e < E; e++) prod[e] = x[e];
            for (; f < end; f++) {
                fetch(f);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    panda29::fe_mul(prod[e], prod[e], x[e]);
                    PANDA_SOP_CHECK(prod[e]);
                }
            }
        }
        Fe<Fr> k;
        panda29::fe_const(k, P.coeff[t]);
        if (t == 0) {
#pragma unroll
            for (int e = 0; e < E; e++) panda29::fe_mul(r[e], prod[e], k);
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) panda29::fe_mul_add(r[e], r[e], one, prod[e], k);
        }
#pragma unroll
        for (int e = 0; e < E; e++) PANDA_SOP_CHECK(r[e]);
    }
    const u32 mode = P.scale_mode, n_scales = P.n_scales;
    if (mode == SCALE_PER_VECTOR) {
        Fe<Fr> s;
        panda29::fe_const(s, P.scale[p % n_scales]);
#pragma unroll
        for (int e = 0; e < E; e++) panda29::fe_mul(r[e], r[e], s);
    } else if (mode == SCALE_CYCLIC) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            Fe<Fr> s;
            panda29::fe_const(s, P.scale[i[e] % n_scales]);
            panda29::fe_mul(r[e], r[e], s);
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) PANDA_SOP_CHECK(r[e]);
}

// ------------------------------------------------------------------------------- host side: building the program

// c^-1 for c = W / R, in the form fe_mul multiplies (the integer R^2 / W mod p): the inverse of the wire's one, which is the integer
// W mod p and so that form of c (5.4).  One Fermat inversion per field and process.
template <class Fr>
inline const Fe<Fr> &wire_factor_inverse()
{
    static const Fe<Fr> value = [] {
        Fe<Fr> one, c, r;
        panda29::fe_one(one);
        u32 w[8];
        panda29::fe_to_wire(w, one);
        panda29::fe_unpack(c, w);
        panda29::fe_inv(r, c);
        return r;
    }();
    return value;
}

// rotation -> [0, n)
inline u32 reduce_rotation(int32_t rotation, u64 n)
{
    const int64_t m = (int64_t)n, r = (int64_t)rotation % m;
    return (u32)(r < 0 ? r + m : r);
}

// Fills the program from the caller's arrays (already validated: counts within the caps, column indices in range, coefficients and
// scales below the modulus).  columns: device addresses; coeffs / scales: wire elements; factors: {column, rotation} pairs.
template <class Fr>
inline void build_program(Program &P, const void *const *columns, unsigned n_columns, const void *coeffs, const unsigned *degrees, unsigned n_terms,
                          const void *factors, const void *scales, unsigned n_scales, unsigned scale_mode, u64 n)
{
    memset(&P, 0, sizeof(P));
    P.n_terms = n_terms;
    P.scale_mode = scale_mode;
    P.n_scales = scale_mode == SCALE_NONE ? 0 : n_scales;
    for (unsigned c = 0; c < n_columns; c++) P.column[c] = (u64)(uintptr_t)columns[c];
    const Fe<Fr> &cinv = wire_factor_inverse<Fr>();
    unsigned max_degree = 0;
    for (unsigned t = 0; t < n_terms; t++) max_degree = degrees[t] > max_degree ? degrees[t] : max_degree;
    Fe<Fr> pw[PANDA_SOP_PROGRAM_FACTORS + 1]; // c^-d
    panda29::fe_one(pw[0]);
    for (unsigned d = 1; d <= max_degree; d++) panda29::fe_mul(pw[d], pw[d - 1], cinv);
    unsigned f = 0;
    for (unsigned t = 0; t < n_terms; t++) {
        for (unsigned e = 0; e < degrees[t]; e++, f++) {
            u32 column;
            int32_t rotation;
            memcpy(&column, (const char *)factors + 8 * (size_t)f, 4);
            memcpy(&rotation, (const char *)factors + 8 * (size_t)f + 4, 4);
            P.factor[f][0] = column;
            P.factor[f][1] = reduce_rotation(rotation, n);
        }
        P.term_end[t] = f;
        u32 w[8];
        memcpy(w, (const char *)coeffs + 32 * (size_t)t, 32);
        Fe<Fr> k;
        panda29::fe_unpack(k, w);
        panda29::fe_mul(k, k, pw[degrees[t]]);
        panda29::fe_reduce_once(k);
        memcpy(P.coeff[t], k.l, sizeof(k.l));
    }
    for (unsigned j = 0; j < P.n_scales; j++) {
        u32 w[8];
        memcpy(w, (const char *)scales + 32 * (size_t)j, 32);
        Fe<Fr> s;
        panda29::fe_unpack(s, w);
        panda29::fe_mul(s, s, cinv);
        panda29::fe_reduce_once(s);
        memcpy(P.scale[j], s.l, sizeof(s.l));
    }
}

} // namespace panda_sop
