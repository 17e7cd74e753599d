// ec_ntt.h -- what the EC-NTT over G1 and the batch affine normalisation compute per thread (host + device).  ec_ntt.hip
// wraps these routines in kernels, tests/host_check/ec_ntt_host.cpp runs the same text on the host under FE29_CHECK.
//
//   out[k] = sum_j omega^(jk) P_j      radix-2 decimation in time over XYZZ points (curve29.h) in the calling thread's arena scratch
//
// Stage s = 1 .. log_n has span m = 2^s: butterfly (g, j), g < n / m, j < m / 2, takes A = x[g m + j], B = x[g m + j + m / 2] and
// w = omega^(j n / m) to (A + w B, A - w B).  The first stage (w = 1 everywhere) reads the affine wire points through the bit reversal;
// the last is followed by normalise_chunk, which writes affine wire points.
//
// Stored points.  Every point a routine here stores meets the stored-point contract of curve29.h with room to spare:
//   X < XB p loose (xyzz_add / xyzz_dbl leave it so), ZZ, ZZZ < 2p tight, and Y < 2p TIGHT -- never the k p - y form.  A negated Y is
//   taken through one product by one (negate_point), so that whichever operand an exceptional case of xyzz_add hands through (an identity
//   on either side) is again a point with Y < 2p, and the next stage may negate it with fe_neg<F, 2> again.
// Values the butterfly forms (units of p; M = SubMargin<F>, NB = SubGrowth<F, 2>):
//   T = w B       X < XB loose, Y < 2 tight, ZZ, ZZZ < 2 tight      (outputs of xyzz_dbl / xyzz_add, or B itself)
//   k p - T.Y     < NB loose                                          (fe_neg<F, 2>; needs T.Y < 2p)
//   (k p - T.Y) 1 < 2 tight                                           (fe_mul by one: NB * 2 < LIM is Bounds<F>'s (2 YB)^2 assertion's); twice per
//                                                                     butterfly: -T for the difference, T again for the sum
//   A + T, A - T  as T                                                (xyzz_add; operands within its stored-point contract)
// No product is formed here that curve29.h does not already form, except the one above and those of normalise_chunk (tight by tight).
//
// The scalar multiplication is a left-to-right double-and-add over the 256 bits of the canonical twiddle, the accumulator starting at the
// identity: leading zero bits double the identity (a compare), a zero bit costs a doubling, a one bit a doubling and an addition.  Where a
// wave's 64 butterflies share their twiddle (n / m >= 64) the words are wave-uniform and so is every branch on them; elsewhere the
// wave pays the doubling and the addition for every bit.  xyzz_dbl and xyzz_add handle P + P, P + (-P) and the identity exactly, and
// nothing here steps round them: B the identity keeps the accumulator the identity, the first one bit ADDS B to the identity (a copy),
// and an accumulator that equals the addend goes through xyzz_add's doubling path.  No index is derived from point data.
#pragma once
#include "curve29.h"

namespace panda_ecntt {

using panda29::Fe;
using panda29::u32;
using panda29::Xyzz;
typedef uint64_t u64;

constexpr unsigned MAX_LOG_N = 26;           // PANDA_EC_NTT_MAX_LOG_N: the MSM's own cap
constexpr unsigned STAGE_THREADS = 64;       // one wave per workgroup: a butterfly may use the whole register file of a SIMD lane
constexpr unsigned NORM_THREADS = 256;       // normalisation workgroup
constexpr unsigned CHUNK = 16;               // points per field inversion
constexpr unsigned UNIFORM_MIN_SHARERS = 64; // butterflies that must share a twiddle for a wave to run uniform
constexpr u64 MAX_POINTS = (u64)1 << 28;     // panda_points_to_affine
constexpr int SCALAR_WORDS = 8;              // every supported scalar field has 256-bit wire elements

// index i < 2^log_n with its log_n bits reversed
PANDA_HD u32 bit_reverse(u32 i, unsigned log_n)
{
    u32 r = 0;
    for (unsigned b = 0; b < log_n; b++) r |= ((i >> b) & 1u) << (log_n - 1 - b);
    return r;
}

// stages of a transform of 2^log_n points in which at least UNIFORM_MIN_SHARERS butterflies share each twiddle (the first, which
// multiplies by nothing, included)
PANDA_HD unsigned uniform_stages(unsigned log_n)
{
    unsigned c = 0;
    for (unsigned s = 1; s <= log_n; s++)
        if (((u64)1 << (log_n - s)) >= UNIFORM_MIN_SHARERS) c++;
    return c;
}

// workgroups of a normalisation over n points
PANDA_HD u64 norm_blocks(u64 n)
{
    const u64 chunks = (n + CHUNK - 1) / CHUNK;
    return (chunks + NORM_THREADS - 1) / NORM_THREADS;
}

// internal form -> the integer's words: a product by the integer 1, fe_reduce_once, fe_pack
template <class Fr>
PANDA_HD void scalar_from_internal(u32 (&w)[SCALAR_WORDS], const Fe<Fr> &a)
{
    Fe<Fr> unit, t;
    panda29::fe_zero(unit);
    unit.l[0] = 1;
    panda29::fe_mul(t, a, unit);
    panda29::fe_reduce_once(t);
    panda29::fe_pack(w, t);
}

// host: a (internal form) has order exactly 2^k, k >= 1: a^(2^(k - 1)) == -1
template <class Fr>
inline bool order_is_pow2(const Fe<Fr> &a, unsigned k)
{
    Fe<Fr> t = a, one, sum;
    for (unsigned i = 0; i + 1 < k; i++) panda29::fe_sqr(t, t);
    panda29::fe_one(one);
    panda29::fe_add(sum, t, one);
    return panda29::fe_is_zero_mod_p(sum);
}

// the two points and the twiddle of butterfly t < n / 2 in stage s (span 2^s): twiddle-major, so that consecutive t share w
struct ButterflyIndex {
    u32 lo, hi, twiddle; // x[lo], x[hi], table index of w = omega^twiddle
};
PANDA_HD ButterflyIndex butterfly_index(u32 t, unsigned log_n, unsigned s)
{
    const unsigned shift = log_n - s;
    const u32 j = t >> shift, g = t & (((u32)1 << shift) - 1);
    ButterflyIndex r;
    r.lo = (g << s) + j;
    r.hi = r.lo + ((u32)1 << (s - 1));
    r.twiddle = j << shift;
    return r;
}

// affine wire point -> XYZZ; x == 0 is the identity
template <class F>
PANDA_HD void point_from_affine_wire(Xyzz<F> &p, const u32 *in)
{
    Fe<F> x, y;
    if (panda29::affine_from_wire(x, y, in))
        panda29::xyzz_set_identity(p);
    else
        panda29::xyzz_from_affine(p, x, y);
}

// p -> -p with Y back below 2p, tight (p.Y < 2p tight)
template <class F>
PANDA_HD void negate_point(Xyzz<F> &p)
{
    Fe<F> t, one;
    panda29::fe_neg<F, 2>(t, p.Y);
    panda29::fe_one(one);
    panda29::fe_mul(p.Y, t, one);
}

// acc = w b: w canonical, SCALAR_WORDS little-endian words
template <class F>
PANDA_HD void scalar_mul(Xyzz<F> &acc, const Xyzz<F> &b, const u32 (&w_in)[SCALAR_WORDS])
{
    u32 w[SCALAR_WORDS];
#pragma unroll
    for (int i = 0; i < SCALAR_WORDS; i++) w[i] = w_in[i];
    panda29::xyzz_set_identity(acc);
#pragma unroll 1
    for (int bit = 0; bit < 32 * SCALAR_WORDS; bit++) {
        const bool one = (w[SCALAR_WORDS - 1] >> 31) != 0;
#pragma unroll
        for (int i = SCALAR_WORDS - 1; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 31); // the words stay in registers: no indexed access
        w[0] <<= 1;
        panda29::xyzz_dbl(acc, acc);
        if (one) panda29::xyzz_add(acc, b);
    }
}

// (A, T) -> (A + T, A - T).  A is read twice through load_a rather than kept beside both sums, and the stages run in place: the
// difference goes to B's slot first (B is dead once T = w B exists), so that the second read of A's slot still finds A; then T is negated
// back and the sum overwrites A.
template <class F, class LoadA, class StoreLo, class StoreHi>
PANDA_HD void butterfly(Xyzz<F> &t, LoadA &&load_a, StoreLo &&store_lo, StoreHi &&store_hi)
{
    Xyzz<F> a;
    negate_point(t);
    load_a(a);
    panda29::xyzz_add(a, t);
    store_hi(a);
    negate_point(t);
    load_a(a);
    panda29::xyzz_add(a, t);
    store_lo(a);
}

// ------------------------------------------------------------------------------------------------- batch normalisation
//
// One inversion for the points [0, count) of a chunk, by Montgomery's trick.  `io` gives the routine its accesses:
//   bool denominator(Fe &d, u32 i)        false: point i is the identity; else d = what its affine form divides by, tight, below 2p
//   void put_prefix(u32 i, const Fe &)    park a value in the OUTPUT slot of point i (the slot is larger than a field element)
//   void get_prefix(Fe &, u32 i)
//   void finish(u32 i, const Fe &dinv)    write the affine wire point from the point and 1 / d
//   void put_identity(u32 i)              all-zero bytes
// Forward, the product of the denominators before point i is parked in i's output slot; then one inversion and the walk back, which
// reads the slot before finish overwrites it.  Identities are skipped both ways, and a chunk of identities alone inverts nothing.
template <class F, class IO>
PANDA_HD void normalise_chunk(IO &io, u32 count)
{
    Fe<F> run, d;
    panda29::fe_one(run);
    bool any = false;
    for (u32 i = 0; i < count; i++) {
        if (!io.denominator(d, i)) continue;
        io.put_prefix(i, run);
        panda29::fe_mul(run, run, d);
        any = true;
    }
    Fe<F> inv;
    if (any)
        panda29::fe_inv(inv, run);
    else
        panda29::fe_one(inv);
    for (u32 k = count; k > 0; k--) {
        const u32 i = k - 1;
        if (!io.denominator(d, i)) {
            io.put_identity(i);
            continue;
        }
        Fe<F> pre, dinv;
        io.get_prefix(pre, i);
        panda29::fe_mul(dinv, inv, pre);
        panda29::fe_mul(inv, inv, d);
        io.finish(i, dinv);
    }
}

// affine wire point from (X, Y) over the given inverse powers
template <class F>
PANDA_HD void affine_wire_out(u32 *out, const Fe<F> &X, const Fe<F> &ix, const Fe<F> &Y, const Fe<F> &iy)
{
    Fe<F> x, y;
    panda29::fe_mul(x, X, ix);
    panda29::fe_mul(y, Y, iy);
    panda29::fe_to_wire(out, x);
    panda29::fe_to_wire(out + F::L, y);
}

// XYZZ: d = ZZZ, 1 / ZZ = (ZZ / ZZZ)^2 as xyzz_to_affine_internal
template <class F>
PANDA_HD void xyzz_affine_wire(u32 *out, const Xyzz<F> &p, const Fe<F> &zi3)
{
    Fe<F> t, zi2;
    panda29::fe_mul(t, p.ZZ, zi3);
    panda29::fe_sqr(zi2, t);
    affine_wire_out(out, p.X, zi2, p.Y, zi3);
}

// X || Y || Z wire triple, Jacobian (x = X / Z^2, y = Y / Z^3) or homogeneous (x = X / Z, y = Y / Z): d = Z
template <class F>
PANDA_HD bool triple_denominator(Fe<F> &d, const u32 *z_wire) // the L words of Z
{
    panda29::fe_from_wire(d, z_wire);
    return !panda29::fe_is_zero_2p(d);
}
template <class F>
PANDA_HD void triple_affine_wire(u32 *out, const u32 *in, const Fe<F> &zi, bool homogeneous)
{
    Fe<F> X, Y, zi2, zi3;
    panda29::fe_from_wire(X, in);
    panda29::fe_from_wire(Y, in + F::L);
    if (homogeneous) {
        affine_wire_out(out, X, zi, Y, zi);
        return;
    }
    panda29::fe_sqr(zi2, zi);
    panda29::fe_mul(zi3, zi2, zi);
    affine_wire_out(out, X, zi2, Y, zi3);
}

} // namespace panda_ecntt
