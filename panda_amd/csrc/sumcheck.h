// sumcheck.h -- the program and the per-pair routines of panda_sumcheck_round, panda_mle_fold and panda_mle_eq_table (sumcheck.hip;
// DESIGN.md 5.7), kept apart from the kernels so that a host program can run them (tests/host_check/sumcheck_host.cpp, under FE29_CHECK).
//
//   fold        F[i] = lo + r (hi - lo)
//   round       g(t) = sum_i sum_terms coeff_term prod_{f < degree_term} ( lo_{c_f, i} + t (hi_{c_f, i} - lo_{c_f, i}) ),  t = 0 .. NE - 1
//   eq table    out[x] = prod_j ( x_j r_j + (1 - x_j)(1 - r_j) )
//
// Arithmetic.  The expression is panda_sop::Program as panda_sop::build_program fills it (poly_terms.h): k' = k c^-degree for c = W / R, so
// that prod * k' / R is k (prod x) on the wire form.  lo + t (hi - lo) is linear, so the wire residues of lo and hi give the wire
// residue of the point: it is formed by t additions of the difference, never by a product.  The fold's challenge is held as r' = r c^-1
// (the integer r R mod p), so that fe_mul(hi - lo, r') = (hi - lo) r on the wire form.  The eq table's factors are held as f R mod p and
// multiplied into the wire's one: W prod(f_j R) / R^k = W prod f_j.
//
// Bounds (contract at the top of fe29.h; worst case every operand 0 or p - 1, 64 terms, a term of 256 factors, 8 evaluation points,
// BLS12-381 Fr with R / p = 70.6 the tightest).  Every sum and difference here is taken to its canonical residue at once, so the only
// values that are not canonical are the outputs of fe_mul / fe_mul_add, and they are the ones of poly_terms.h:
//   loaded element    fe_unpack of a canonical residue                                     tight, < p      (canonical)
//   delta = hi - lo   sub_canon: limb-wise a - b with borrows, + p if negative             tight, < p      (canonical)
//   x_0 = lo, x_t = x_(t-1) + delta   add_canon (poly_sum.h): raw limbs < 2^30, value < 2p; fe_carry, fe_reduce_once
//                                                                                          tight, < p      (canonical), for every t
//   running product   first factor: x_t itself, < p; then fe_mul(prod < 2p, x_t < p): 2 p^2 < 0.9 R p
//                                                                                          tight, < 2p     (exactly < 2 p^2 / R + p)
//   k', r', ONE       reduced on the host / a constant                                     tight, < p
//   every term        fe_mul_add(acc < 2p, ONE < p, prod < 2p, k' < p): 4 p^2 < 0.9 R p (R / p > 4.5), 27 column terms of < 2^58 in a
//                     u64; the first term adds to acc = 0                                  tight, < 2p     (exactly < 4 p^2 / R + p)
//   pair's result     fe_reduce_once(acc < 2p)                                             tight, < p      (canonical)
//   fold              fe_mul(delta < p, r' < p): p^2 < 0.9 R p -> tight, < 2p; fe_reduce_once; add_canon(lo, .)
//                                                                                          tight, < p      (canonical)
//   sums over pairs   add_canon of canonical values, in registers, lanes, LDS and memory   tight, < p      (canonical)
//   eq table          fe_mul(h < 2p, f < p): 2 p^2 < 0.9 R p -> tight, < 2p; the stored element fe_reduce_once of it
// The accumulators are back to tight and < 2p after EVERY term and the points canonical after every addition, so neither the term count,
// the factor count, the number of evaluation points nor the pair count enters a bound; no loose or raw value is ever an operand of a
// product.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fe29.h"
#include "poly_sum.h"
#include "poly_terms.h"

#define PANDA_SUMCHECK_PROGRAM_EVALS 8
#define PANDA_MLE_PROGRAM_LOG_N 28

namespace panda_sumcheck {

using panda29::Fe;
using panda29::u32;
using panda_sop::Program;
typedef uint64_t u64;

constexpr int NL = 9; // limbs of every supported scalar field
enum Order : u32 { BIND_LOW = 0, BIND_HIGH = 1 };

// What the round kernel reads, at wave-uniform addresses.  The second part is used by the fused round alone.
struct Round {
    Program prog;                              // columns, terms, factors (rotations all 0), coefficients; no scales
    u64 folded[PANDA_SOP_PROGRAM_COLUMNS];     // device addresses of the folded tables
    u32 store[PANDA_SOP_PROGRAM_FACTORS];      // 1: factor f is the LAST one on its column -- the thread stores the column's folded pair after it
    u32 idle[PANDA_SOP_PROGRAM_COLUMNS];       // the columns no factor names: folded and stored after the terms
    u32 n_idle, n_columns;
    u32 challenge[NL];                         // r' = r c^-1, canonical limbs
    u32 reserved;
};

// The factors of the eq table, (1 - r_j, r_j) as f R mod p; bits >= log_n hold (ONE, ONE).  `one` is the wire's one (W mod p).
struct EqFactors {
    u32 f[PANDA_MLE_PROGRAM_LOG_N][2][NL];
    u32 one[NL];
};

#if defined(FE29_CHECK)
template <class Fr>
inline void check_canonical(const Fe<Fr> &v)
{
    for (int i = 0; i < NL - 1; i++) assert(v.l[i] < (1u << 29) && "sumcheck: limb not tight");
    bool below = false;
    for (int i = NL - 1; i >= 0; i--)
        if (v.l[i] != Fr::P[i]) {
            below = v.l[i] < Fr::P[i];
            break;
        }
    assert(below && "sumcheck: value not below p");
}
#define PANDA_SUMCHECK_CANON(v) check_canonical(v)
#define PANDA_SUMCHECK_TIGHT_2P(v) panda_sop::check_tight_2p(v)
#else
#define PANDA_SUMCHECK_CANON(v)
#define PANDA_SUMCHECK_TIGHT_2P(v)
#endif

// a, b canonical -> a - b canonical: the limb-wise difference with borrows, plus p when it is negative
template <class Fr>
PANDA_HD void sub_canon(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b)
{
    constexpr int N = Fr::N;
    u32 d[N], e[N], borrow = 0, carry = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const u32 t = a.l[i] - b.l[i] - borrow;
        borrow = t >> 31;
        d[i] = i < N - 1 ? t & panda29::LIMB_MASK : t;
    }
#pragma unroll
    for (int i = 0; i < N; i++) { // d + p; with a borrow the top limb wraps back into range
        const u32 t = d[i] + Fr::P[i] + carry;
        carry = i < N - 1 ? t >> panda29::LIMB_BITS : 0u;
        e[i] = i < N - 1 ? t & panda29::LIMB_MASK : t;
    }
#pragma unroll
    for (int i = 0; i < N; i++) r.l[i] = borrow ? e[i] : d[i];
    PANDA_SUMCHECK_CANON(r);
}

// lo, hi canonical wire residues, rc = r' -> F = lo + r (hi - lo), canonical
template <class Fr>
PANDA_HD void fold_canon(Fe<Fr> &F, const Fe<Fr> &lo, const Fe<Fr> &hi, const Fe<Fr> &rc)
{
    Fe<Fr> d, m;
    sub_canon(d, hi, lo);
    panda29::fe_mul(m, d, rc);
    PANDA_SUMCHECK_TIGHT_2P(m);
    panda29::fe_reduce_once(m);
    panda_poly::add_canon(F, lo, m);
    PANDA_SUMCHECK_CANON(F);
}

// One pair: acc[t] = sum_terms coeff prod_f (lo_f + t (hi_f - lo_f)) for t < NE, canonical.  load(lo, hi, f) fetches the pair of factor f's
// column (canonical), in the fused round by folding it.  The term and factor loops depend on the program alone; the state is one
// accumulator and one running product per point, the pair, and the running point, every array indexed by unrolled constants only.
template <class Fr, int NE, class Load>
PANDA_HD void round_pair(Fe<Fr> (&acc)[NE], const Program &P, Load &&load)
{
    static_assert(Fr::N == NL, "the program holds nine-limb constants");
    static_assert(NE >= 1 && NE <= PANDA_SUMCHECK_PROGRAM_EVALS, "evaluation points");
    Fe<Fr> one, prod[NE], lo, delta, x;
    panda29::fe_one(one);
#pragma unroll
    for (int e = 0; e < NE; e++) panda29::fe_zero(acc[e]);
    const u32 n_terms = P.n_terms;
    auto fetch = [&](u32 f) { // lo, delta <- the pair of factor f
        load(lo, delta, f);
        PANDA_SUMCHECK_CANON(lo);
        PANDA_SUMCHECK_CANON(delta);
        sub_canon(delta, delta, lo);
    };
    u32 f = 0;
    for (u32 t = 0; t < n_terms; t++) {
        const u32 end = P.term_end[t];
        if (f == end) {
#pragma unroll
            for (int e = 0; e < NE; e++) prod[e] = one;
        } else {
            fetch(f++);
            x = lo;
#pragma unroll
            for (int e = 0; e < NE; e++) {
                prod[e] = x;
                if (e < NE - 1) panda_poly::add_canon(x, x, delta);
            }
            for (; f < end; f++) {
                fetch(f);
                x = lo;
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    panda29::fe_mul(prod[e], prod[e], x);
                    PANDA_SUMCHECK_TIGHT_2P(prod[e]);
                    if (e < NE - 1) {
                        panda_poly::add_canon(x, x, delta);
                        PANDA_SUMCHECK_CANON(x);
                    }
                }
            }
        }
        Fe<Fr> k;
        panda29::fe_const(k, P.coeff[t]);
#pragma unroll
        for (int e = 0; e < NE; e++) {
            panda29::fe_mul_add(acc[e], acc[e], one, prod[e], k);
            PANDA_SUMCHECK_TIGHT_2P(acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < NE; e++) {
        panda29::fe_reduce_once(acc[e]);
        PANDA_SUMCHECK_CANON(acc[e]);
    }
}

// ------------------------------------------------------------------------------- host side

// a wire element (HOST, any alignment) -> x c^-1, canonical limbs: the form in which fe_mul multiplies a wire residue by x
template <class Fr>
inline void wire_to_multiplier(u32 (&out)[NL], const void *wire)
{
    u32 w[8];
    memcpy(w, wire, 32);
    Fe<Fr> s;
    panda29::fe_unpack(s, w);
    panda29::fe_mul(s, s, panda_sop::wire_factor_inverse<Fr>());
    panda29::fe_reduce_once(s);
    memcpy(out, s.l, sizeof(s.l));
}

// Fills the round's program from the caller's arrays (already validated).  folded / challenge: NULL for the plain round.
template <class Fr>
inline void build_round(Round &R, const void *const *columns, unsigned n_columns, const void *coeffs, const unsigned *degrees, unsigned n_terms,
                        const void *factors, void *const *folded, const void *challenge)
{
    panda_sop::build_program<Fr>(R.prog, columns, n_columns, coeffs, degrees, n_terms, factors, nullptr, 0, panda_sop::SCALE_NONE, 1);
    memset((char *)&R + sizeof(Program), 0, sizeof(Round) - sizeof(Program));
    R.n_columns = n_columns;
    if (!folded) return;
    for (unsigned c = 0; c < n_columns; c++) R.folded[c] = (u64)(uintptr_t)folded[c];
    const unsigned total = n_terms ? R.prog.term_end[n_terms - 1] : 0;
    bool seen[PANDA_SOP_PROGRAM_COLUMNS] = {};
    for (unsigned f = total; f-- > 0;) {
        const u32 c = R.prog.factor[f][0];
        R.store[f] = seen[c] ? 0u : 1u;
        seen[c] = true;
    }
    for (unsigned c = 0; c < n_columns; c++)
        if (!seen[c]) R.idle[R.n_idle++] = c;
    wire_to_multiplier<Fr>(R.challenge, challenge);
}

// the eq table's factors from the point (HOST, log_n wire elements below the modulus)
template <class Fr>
inline void build_eq_factors(EqFactors &T, const void *point, unsigned log_n)
{
    Fe<Fr> one, k_in, wone;
    panda29::fe_one(one);
    panda29::fe_const(k_in, Fr::K_IN);
    u32 w[8];
    panda29::fe_to_wire(w, one);
    panda29::fe_unpack(wone, w);
    memcpy(T.one, wone.l, sizeof(wone.l));
    for (unsigned j = 0; j < PANDA_MLE_PROGRAM_LOG_N; j++) {
        Fe<Fr> f0 = one, f1 = one; // R mod p: the factor 1
        if (j < log_n) {
            Fe<Fr> r, m;
            memcpy(w, (const char *)point + 32 * (size_t)j, 32);
            panda29::fe_unpack(r, w);
            sub_canon(m, wone, r); // (1 - r) W
            panda29::fe_mul(f0, m, k_in);
            panda29::fe_reduce_once(f0);
            panda29::fe_mul(f1, r, k_in);
            panda29::fe_reduce_once(f1);
        }
        memcpy(T.f[j][0], f0.l, sizeof(f0.l));
        memcpy(T.f[j][1], f1.l, sizeof(f1.l));
    }
}

// The eq table's element x from the factors: what the kernel computes in another order (it shares the product over the bits a thread's
// elements have in common).  Canonical.
template <class Fr>
PANDA_HD void eq_element(Fe<Fr> &r, const EqFactors &T, u32 x, unsigned log_n)
{
    Fe<Fr> h;
    panda29::fe_const(h, T.one);
    for (unsigned j = 0; j < log_n; j++) {
        Fe<Fr> f;
        panda29::fe_const(f, T.f[j][(x >> j) & 1]);
        panda29::fe_mul(h, h, f);
        PANDA_SUMCHECK_TIGHT_2P(h);
    }
    panda29::fe_reduce_once(h);
    r = h;
}

} // namespace panda_sumcheck
