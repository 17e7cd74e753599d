// points_mul.h -- what the point-vector scalar multiplication computes per thread (host + device).  points_mul.hip wraps
// these routines in kernels, tests/host_check/points_mul_host.cpp runs the same text on the host under FE29_CHECK.
//
//   out[i] = A_i + k_i P_i        k_i = d_scalars[i] (EACH), the one host scalar (ONE), or c s^i (POWERS); the A_i term is optional
//
// The group law, the stored-point contract and the bounds are those of ec_ntt.h: a thread forms k_i P_i by the same left-to-right
// double-and-add over XYZZ points, adds the affine A_i with xyzz_add, and stores the XYZZ point for the batch normalisation.  Nothing
// here forms a product that ec_ntt.h's scalar_mul and butterfly do not form, and nothing steps round the exceptional cases: k_i = 0 or
// P_i the identity leave the accumulator the identity (so the sum is A_i), A_i = -k_i P_i cancels in xyzz_add, A_i = k_i P_i takes its
// doubling path.  No index is derived from point or scalar data.
//
// Loop length.  The loop runs over `bits` bits, not over 256: the caller counts the significant bits of every lane's integer
// (scalar_bits), takes the wave's maximum and hands it to scalar_mul, which shifts the integer up by 256 - bits and then runs the loop
// of ec_ntt.h's scalar_mul for that many steps.  Any bits >= scalar_bits(k) gives the same point: a leading zero bit doubles the
// identity (a compare).  A wave of 128-bit challenges costs 128 steps.
#pragma once
#include "ec_ntt.h"

namespace panda_pmul {

using panda29::Fe;
using panda29::u32;
using panda29::Xyzz;
using panda_ecntt::norm_blocks; // workgroups of the normalisation over n points
using panda_ecntt::scalar_from_internal;
using panda_ecntt::SCALAR_WORDS;
typedef uint64_t u64;

constexpr unsigned MUL_THREADS = 64;        // one wave per workgroup, as the EC-NTT stages: the 14-limb point takes the register file
using panda_ecntt::MAX_POINTS;              // n of one call: 2^28, the cap of the normalisation
constexpr int POWER_BITS = 28;              // bits of an index below MAX_POINTS
constexpr unsigned MODE_EACH = 0, MODE_ONE = 1, MODE_POWERS = 2; // PANDA_POINTS_MUL_*

// workgroups of the multiplication kernel over n points
PANDA_HD u64 mul_blocks(u64 n) { return (n + MUL_THREADS - 1) / MUL_THREADS; }

// significant bits of the integer in SCALAR_WORDS little-endian words: 0 for zero, 256 for a set top bit
PANDA_HD unsigned scalar_bits(const u32 (&w)[SCALAR_WORDS])
{
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < SCALAR_WORDS; i++)
        if (w[i]) bits = 32u * i + 32u - (unsigned)__builtin_clz(w[i]);
    return bits;
}

// acc = k b over the low `bits` bits of k: scalar_bits(k) <= bits <= 256.  The words stay in registers: the shift is by words in
// three conditional steps and then by bits, no indexed access.
template <class F>
PANDA_HD void scalar_mul(Xyzz<F> &acc, const Xyzz<F> &b, const u32 (&k)[SCALAR_WORDS], unsigned bits)
{
    u32 w[SCALAR_WORDS];
#pragma unroll
    for (int i = 0; i < SCALAR_WORDS; i++) w[i] = k[i];
    const unsigned shift = 32u * SCALAR_WORDS - bits, ws = shift >> 5, bs = shift & 31u; // ws == SCALAR_WORDS only with bits == 0: no step
#pragma unroll
    for (int step = 4; step > 0; step >>= 1) {
        const bool take = (ws & (unsigned)step) != 0;
#pragma unroll
        for (int i = SCALAR_WORDS - 1; i >= 0; i--) w[i] = take ? (i >= step ? w[i - step] : 0u) : w[i];
    }
    if (bs) {
#pragma unroll
        for (int i = SCALAR_WORDS - 1; i > 0; i--) w[i] = (w[i] << bs) | (w[i - 1] >> (32u - bs));
        w[0] <<= bs;
    }
    panda29::xyzz_set_identity(acc);
#pragma unroll 1
    for (unsigned bit = 0; bit < bits; bit++) {
        const bool one = (w[SCALAR_WORDS - 1] >> 31) != 0;
#pragma unroll
        for (int i = SCALAR_WORDS - 1; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 31);
        w[0] <<= 1;
        panda29::xyzz_dbl(acc, acc);
        if (one) panda29::xyzz_add(acc, b);
    }
}

// Montgomery wire residue (32 B) -> the integer's words, as every consumer of a scalar does (fe29.h fe_wire_to_canonical: one product,
// fe_reduce_once, fe_pack).  A wire value at or above the modulus gives the words of some integer below 2^256: other values, same accesses.
template <class Fr>
PANDA_HD void scalar_from_wire(u32 (&w)[SCALAR_WORDS], const u32 *wire)
{
    panda29::fe_wire_to_canonical<Fr>(w, wire);
}

// c, s^(2^b) for b < POWER_BITS, internal form: the by-value table of POWERS
template <class Fr>
struct PowerTable {
    Fe<Fr> c, sq[POWER_BITS];
};
template <class Fr>
PANDA_HD void power_table(PowerTable<Fr> &t, const Fe<Fr> &c, const Fe<Fr> &s)
{
    t.c = c;
    t.sq[0] = s;
    for (int b = 1; b < POWER_BITS; b++) panda29::fe_sqr(t.sq[b], t.sq[b - 1]);
}

// the integer c s^i, i < 2^POWER_BITS: statically indexed products with fe_select, the k_twiddles pattern
template <class Fr>
PANDA_HD void power_scalar(u32 (&w)[SCALAR_WORDS], const PowerTable<Fr> &t, u32 i)
{
    Fe<Fr> acc = t.c, p;
#pragma unroll
    for (int b = 0; b < POWER_BITS; b++) {
        panda29::fe_mul(p, acc, t.sq[b]);
        panda29::fe_select(acc, ((i >> b) & 1u) != 0, p, acc);
    }
    scalar_from_internal(w, acc);
}

// acc += the affine wire point A (x == 0 is the identity)
template <class F>
PANDA_HD void add_affine_wire(Xyzz<F> &acc, const u32 *wire)
{
    Xyzz<F> a;
    panda_ecntt::point_from_affine_wire(a, wire);
    panda29::xyzz_add(acc, a);
}

} // namespace panda_pmul
