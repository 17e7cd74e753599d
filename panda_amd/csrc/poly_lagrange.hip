// poly_lagrange.hip -- evaluation-form KZG openings over the scalar fields (panda_poly_evaluate_lagrange,
// panda_poly_divide_linear_lagrange, panda_poly_lagrange_plan): the value at z of the polynomial f of degree < n = 2^log_n
// that a vector of evaluations on the domain x_i = s w^i stands for, and the evaluations of (f(X) - f(z)) / (X - z) on the same domain,
// in natural or bit-reversed order, without a transform.
//
// With u = z / s and off the domain (u^n != 1)
//   f(z) = (u^n - 1) / n  sum_i e_i w^i / (u - w^i) = K (u S1 - S0),   K = (u^n - 1) / n,  S1 = sum_i e_i / (u - w^i),  S0 = sum_i e_i
// (w^i / (u - w^i) = u / (u - w^i) - 1 takes w^i out of the sum), and q_i = (e_i - y) / (x_i - z) = (e_i - y) (-1 / s) / (u - w^i).  On the
// domain (z = x_m; the host finds m, the kernels are handed the position of x_m and never test a denominator for zero) f(z) = e_m is copied,
// the denominator at that position is replaced by one, q_i is the same for i != m and q_m = -(1 / z) sum_{i != m} q_i x_i = -(1 / u) sum_{i
// != m} q_i w^i.
//
// The denominators u - w^i are inverted by the product trick in the launch structure of poly_product.hip -- ONE field inversion per
// call, whatever n, batch and the points are (the denominators do not depend on the vector), and that one on the host -- on the workgroup scan of
// poly_scan.h; no kernel waits for another workgroup.  Tiles of TILE = THREADS * E positions:
//   launch 1  k_lag_den_totals  workgroup a multiplies the denominators of tile a down to one element per point; reads no vector.  In
//                               bit-reversed order a tile is a coset of a subgroup and its product is u^T - w^(cT): k_lag_coset_totals, one
//                               thread per tile, replaces the kernel for points off the domain
//   launch 2  k_lag_seeds       one workgroup per point: the exclusive suffix products of the tile totals seeded with the inverse of the
//                               grand product, and their exclusive prefix products (poly_product.hip's k_product_seeds, inverse form, without
//                               its inversion: the grand product is u^n - 1, or n / u on the domain, and the host hands over its inverse)
//   launch 3  k_lag_eval        workgroup (p, a) loads tile a of vector p ONCE and, for every point off the domain, rebuilds the
//                               denominators, scans them from the two seeds into their inverses and sums e_i / (u - w^i); one partial S1
//                               per point and one partial S0 per tile
//   launch 4  k_lag_values      workgroup (k, p) adds the partials in a fixed order and stores K (u S1 - S0), or copies e_m
//   launch 5  k_lag_quot        (division) workgroup (a, p) rebuilds the inverses of tile a times -1 / s and stores q_i; a thread stores
//                               only positions it loaded, and never the position of x_m, so d_quot == d_evals is safe.  On the domain it
//                               also sums q_i w^i over the tile, launch 3 is not needed, and
//   launch 5' k_lag_fix         one workgroup per vector adds those partials and stores q_m
// Evaluation is launches 1 to 4, division five launches either way (1 2 3 4 5 off the domain, 1 2 4 5 5' on it).
//
// w^i is computed, never loaded.  Position j holds the domain point of exponent sigma(j), sigma the identity or the bit reversal over
// log_n bits; either way sigma(j) = sum over the set bits b of j of sigma(2^b), so w^sigma(j0 + e) = prod_{b in j0} w^sigma(2^b) times
// w^sigma(e) for a run that starts at a multiple j0 of E: the host hands over the log_n - 3 factors of the first product and the E - 1 of
// the second by value as fe_mul_shoup pairs (Domain), and the kernels do not know the order.
//
// Arithmetic and bounds (contract at the top of fe29.h; nine limbs, R = 2^261, R / p >= 70).  Evaluations, y and every sum of them are
// wire residues (x W, W = 2^256); u, w^i, the denominators, their products and inverses are internal residues (x R); fe_mul(a, b) =
// a b / R maps (wire, internal) to wire and (internal, internal) to internal, a product by a plain-integer constant (fe_mul_shoup) keeps
// the form of its operand.
//   w^i           internal one times up to 26 constants by fe_mul_shoup: operand tight and < 3p < R, result tight, < 3p
//   u - w^i       fe_sub<3> of u (tight, < 2p: fe_mul's output) and w^i < 3p: loose, < (2 + KEFF) p; fe_reduce_small_2p: tight, < 2p.
//                 The next point's: fe_add of that and u' - u (fe_sub<2>, reduced: tight, < 2p): loose, < 4p; reduced again.  In the
//                 quotient's on-domain sum w^i comes back as u - (u - w^i), the same way
//   e_i - y       fe_sub<1> of two canonical residues: loose, < (1 + KEFF) p; fe_reduce_small_2p: tight, < 2p
//   products      every operand is the wire's canonical residue (< p), one (< p) or tight and < 2p: 4 p^2 < 0.9 R p; result tight, < 2p
//   sums          every term is a product, fe_reduce_once -> canonical; add_canon (poly_sum.h) keeps canonical, so the number of terms,
//                 tiles and chunks does not enter
//   value         fe_mul_shoup of two canonical sums (< 3p each, tight), fe_sub<3>: loose, < 8p < 2^9 p, what store_elem takes
// Every stored element goes through store_elem.  Every reduction has a fixed order, so results are the same bytes on every run.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"
#include "poly_sum.h"

using namespace panda29;
using namespace panda_poly;

namespace {

constexpr int E = 8;  // positions per thread: the run whose exponents differ by the E - 1 constants of Domain::run
constexpr int LOG_E = 3;
constexpr int CE = 4; // tile totals / partial sums per thread of the one-workgroup kernels
constexpr unsigned TILE = THREADS * E, CHUNK = THREADS * CE;
static_assert(2 * CHUNK == TILE, "the header promises *tile / 2 partials per step of the one-workgroup kernels");
constexpr int MAXP = PANDA_POLY_MAX_POINTS;
constexpr int THREAD_BITS = 8; // bits LOG_E .. LOG_E + 7 of a position are the thread's
static_assert((1 << THREAD_BITS) == THREADS && (1 << LOG_E) == E, "a position is (tile, thread, e)");
constexpr int DOMAIN_BITS = MAX_LOG_ELEMS - LOG_E;
constexpr u32 NONE = 0xFFFFFFFFu; // "this point is off the domain"

// poly_scan.h's operations.  The product: every operand tight and < 2p (bounds above).  The sum: canonical in and out.
struct OpMul {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_one(r); }
    template <class Fr>
    static __device__ __forceinline__ void combine(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b) { fe_mul(r, a, b); }
    template <class Fr, int RUN>
    static __device__ __forceinline__ void run(Fe<Fr> &g, const Fe<Fr> (&x)[RUN])
    {
        g = x[0];
#pragma unroll
        for (int e = 1; e < RUN; e++) fe_mul(g, g, x[e]);
    }
};
struct OpAdd {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_zero(r); }
    template <class Fr>
    static __device__ __forceinline__ void combine(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b) { add_canon(r, a, b); }
    template <class Fr, int RUN>
    static __device__ __forceinline__ void run(Fe<Fr> &g, const Fe<Fr> (&x)[RUN])
    {
        g = x[0];
#pragma unroll
        for (int e = 1; e < RUN; e++) add_canon(g, g, x[e]);
    }
};

// the domain of one call: bit[b] = w^sigma(2^(b + LOG_E)) for LOG_E + b < log_n, run[e - 1] = w^sigma(e) for 0 < e < E (one where
// e >= n); plain integers with their precomputed quotients
template <class Fr>
struct Domain {
    FeTw<Fr> bit[DOMAIN_BITS];
    FeTw<Fr> run[E - 1];
};

// the points of one call: u = z / s (internal form, tight, < 2p), the position of x_m = z, NONE off the domain, and the inverse of the
// product of all n denominators: prod_i (u - w^i) = u^n - 1 off the domain, and with the factor of x_m = z taken out the derivative
// n u^(n-1) = n / u on it.  The host inverts (microseconds); one thread of the device would take a tenth of a millisecond.
template <class Fr>
struct Points {
    Fe<Fr> u[MAXP];
    Fe<Fr> inv[MAXP];
    u32 pos[MAXP];
    unsigned n_points;
};

// the constants of launch 4: K and K u per point
template <class Fr>
struct ValueConsts {
    FeTw<Fr> k[MAXP];
    FeTw<Fr> ku[MAXP];
};

// w[e] = w^sigma(j0 + e), internal form, for the run at j0 = (a, thread, 0).  The thread's bits are a select per constant, the tile's a
// wave-uniform branch.  At most log_n - 3 + E - 1 products.
template <class Fr>
__device__ __forceinline__ void domain_run(Fe<Fr> (&w)[E], const Domain<Fr> &D, unsigned a, unsigned log_n)
{
    Fe<Fr> b;
    fe_one(b);
    const int nbits = (int)log_n - LOG_E;
#pragma unroll
    for (int k = 0; k < THREAD_BITS; k++) {
        if (k < nbits) {
            Fe<Fr> t;
            fe_mul_shoup<Fr, true>(t, b, D.bit[k].w, D.bit[k].q);
            fe_select(b, (threadIdx.x >> k) & 1, t, b);
        }
    }
    for (int k = THREAD_BITS; k < nbits; k++) {
        if ((a >> (k - THREAD_BITS)) & 1) {
            Fe<Fr> t;
            fe_mul_shoup<Fr, true>(t, b, D.bit[k].w, D.bit[k].q);
            b = t;
        }
    }
    w[0] = b;
#pragma unroll
    for (int e = 1; e < E; e++) fe_mul_shoup<Fr, true>(w[e], b, D.run[e - 1].w, D.run[e - 1].q);
}

// the denominator of position j: u - w, tight and < 2p; one at the distinguished position and beyond the vector
template <class Fr>
__device__ __forceinline__ void denominator(Fe<Fr> &d, const Fe<Fr> &u, const Fe<Fr> &w, u32 j, u32 n, u32 pos)
{
    Fe<Fr> one;
    fe_one(one);
    fe_sub<Fr, 3>(d, u, w);
    fe_reduce_small_2p(d);
    fe_select(d, j >= n || j == pos, one, d);
}

// The inverses of the thread's eight denominators from the scans' results: pre = the prefix seed times every denominator before the run,
// suf = the suffix seed (which carries the inverse of the grand product) times every denominator behind it, so T = pre suf is
// 1 / (d[0] .. d[7]).  With the half products h0 = d[0] .. d[3] and h1 = d[4] .. d[7], T h0 = 1 / h1 and T h1 = 1 / h0, and each half is
// the product trick over four elements with three prefixes in registers: a prefix array over the whole run would cost the kernels
// their second wave per SIMD.  f(index, 1 / d[index]) is called for index = 7 down to 0, the index a compile-time constant.  25 products.
template <int I>
struct Idx {
    static constexpr int value = I;
};
template <class Fr, int B, class F>
__device__ __forceinline__ void half_inverses(const Fe<Fr> (&d)[E], Fe<Fr> run, F &f)
{
    Fe<Fr> q1, q2, r;
    fe_mul(q1, d[B], d[B + 1]);
    fe_mul(q2, q1, d[B + 2]);
    fe_mul(r, q2, run);
    f(Idx<B + 3>(), r);
    fe_mul(run, run, d[B + 3]);
    fe_mul(r, q1, run);
    f(Idx<B + 2>(), r);
    fe_mul(run, run, d[B + 2]);
    fe_mul(r, d[B], run);
    f(Idx<B + 1>(), r);
    fe_mul(run, run, d[B + 1]);
    f(Idx<B>(), run);
}
template <class Fr>
__device__ __forceinline__ void half_products(Fe<Fr> &h0, Fe<Fr> &h1, Fe<Fr> &g, const Fe<Fr> (&d)[E])
{
    static_assert(E == 8, "two halves of four");
    fe_mul(h0, d[0], d[1]);
    fe_mul(h0, h0, d[2]);
    fe_mul(h0, h0, d[3]);
    fe_mul(h1, d[4], d[5]);
    fe_mul(h1, h1, d[6]);
    fe_mul(h1, h1, d[7]);
    fe_mul(g, h0, h1);
}
template <class Fr, class F>
__device__ __forceinline__ void for_each_inverse(const Fe<Fr> (&d)[E], const Fe<Fr> &h0, const Fe<Fr> &h1, const Fe<Fr> &pre, const Fe<Fr> &suf, F &&f)
{
    Fe<Fr> T, i;
    fe_mul(T, pre, suf);
    fe_mul(i, T, h0);
    half_inverses<Fr, 4>(d, i, f);
    fe_mul(i, T, h1);
    half_inverses<Fr, 0>(d, i, f);
}

struct PadZero {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_zero(r); }
};

// launch 1: tn[k * tiles + a] = the product of the denominators of tile a at point k.  SKIP: points on the domain need none (evaluation).
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_den_totals(u32 *__restrict__ tn, unsigned log_n, unsigned tiles, bool skip, Domain<Fr> D, Points<Fr> P)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned a = blockIdx.x;
    const u32 n = 1u << log_n, j0 = a * TILE + threadIdx.x * E;
    Fe<Fr> w[E];
    domain_run(w, D, a, log_n);
    for (unsigned k = 0; k < P.n_points; k++) {
        const u32 pos = P.pos[k];
        if (skip && pos != NONE) continue;
        Fe<Fr> d[E], g;
#pragma unroll
        for (int e = 0; e < E; e++) denominator(d[e], P.u[k], w[e], j0 + e, n, pos);
        OpMul::run(g, d);
        block_reduce<OpMul>(g, s_w);
        if (threadIdx.x == 0) store_elem(tn + ((u64)k * tiles + a) * 8, g);
        __syncthreads();
    }
}

// Launch 1 in bit-reversed order: tile a holds the coset w^c H of the subgroup H of order Tn = min(TILE, n), c the reversal of a over the
// tile bits, and prod_{h in H} (u - w^c h) = u^Tn - w^(c Tn) -- no denominator is formed.  tbit[b] = w^(Tn sigma(2^b TILE)), ut[k] =
// u_k^Tn (internal form, tight, < 2p).  Only for points off the domain: a position taken out of the product breaks the identity.
constexpr int TILE_BITS = MAX_LOG_ELEMS - LOG_E - THREAD_BITS;
template <class Fr>
struct CosetTotals {
    FeTw<Fr> tbit[TILE_BITS];
    Fe<Fr> ut[MAXP];
};
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_coset_totals(u32 *__restrict__ tn, unsigned tiles, unsigned tile_bits, CosetTotals<Fr> C, Points<Fr> P)
{
    const unsigned a = blockIdx.x * THREADS + threadIdx.x, k = blockIdx.y;
    if (P.pos[k] != NONE || a >= tiles) return;
    Fe<Fr> b, d;
    fe_one(b);
    for (unsigned bit = 0; bit < tile_bits; bit++) {
        Fe<Fr> t;
        fe_mul_shoup<Fr, true>(t, b, C.tbit[bit].w, C.tbit[bit].q);
        fe_select(b, (a >> bit) & 1, t, b);
    }
    fe_sub<Fr, 3>(d, C.ut[k], b); // as u - w^i
    fe_reduce_small_2p(d);
    store_elem(tn + ((u64)k * tiles + a) * 8, d);
}

// launch 2: one workgroup per point.  tn: the tile totals, replaced by their exclusive prefix products; td receives the exclusive suffix
// products times the inverse of the grand product.
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_seeds(u32 *tn, u32 *td, unsigned tiles, bool skip, Points<Fr> P)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned k = blockIdx.x;
    if (skip && P.pos[k] != NONE) return;
    u32 *N = tn + (u64)k * tiles * 8, *D = td + (u64)k * tiles * 8;
    Fe<Fr> carry = P.inv[k]; // the inverse of the grand product, which the host knows in closed form
    for (unsigned c = tiles_of(tiles, CHUNK); c-- > 0;) {
        const u64 a0 = (u64)c * CHUNK + threadIdx.x * CE;
        Fe<Fr> x[CE], g, s, total;
        load_run<OpMul, Fr, CE>(x, N, a0, tiles);
        OpMul::run(g, x);
        block_scan<OpMul, Fr, true>(s, total, g, carry, s_w);
        carry = total;
#pragma unroll
        for (int e = CE - 1; e >= 0; e--) {
            if (a0 + e < tiles) store_elem(D + (a0 + e) * 8, s);
            if (e > 0) fe_mul(s, s, x[e]);
        }
        __syncthreads();
    }
    fe_one(carry);
    walk_totals<OpMul, Fr, CE, true>(carry, N, N, tiles, s_w);
}

// launch 3: part0[p * tiles + a] = the sum of tile a of vector p; part1[(p * n_points + k) * tiles + a] = sum over the tile of
// e_i / (u_k - w^i) for every point k off the domain
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_eval(const u32 *__restrict__ evals, const u32 *__restrict__ sn, const u32 *__restrict__ sd, u32 *__restrict__ part1,
                                                      u32 *__restrict__ part0, unsigned log_n, unsigned tiles, Domain<Fr> D, Points<Fr> P)
{
    __shared__ u32 s_w[3 * WAVES * NL];
    const unsigned tile_bits = log_n > (unsigned)(LOG_E + THREAD_BITS) ? log_n - (LOG_E + THREAD_BITS) : 0; // tiles = 2^tile_bits
    const unsigned p = blockIdx.x >> tile_bits, a = blockIdx.x & (tiles - 1);
    const u32 n = 1u << log_n, j0 = a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], d[E], zero, one, acc, mine, total, uprev;
    load_run<PadZero, Fr, E>(x, evals + (u64)p * n * 8, j0, n);
    fe_zero(zero);
    fe_one(one);
    OpAdd::run(acc, x);
    block_scan<OpAdd, Fr, false>(mine, total, acc, zero, s_w + 2 * WAVES * NL);
    if (threadIdx.x == 0) store_elem(part0 + ((u64)p * tiles + a) * 8, total);
    unsigned k0 = 0;
    while (k0 < P.n_points && P.pos[k0] != NONE) k0++;
    if (k0 == P.n_points) return;
    {
        Fe<Fr> w[E];
        domain_run(w, D, a, log_n);
        uprev = P.u[k0];
#pragma unroll
        for (int e = 0; e < E; e++) denominator(d[e], uprev, w[e], j0 + e, n, NONE);
    }
    for (unsigned k = k0; k < P.n_points; k++) {
        if (P.pos[k] != NONE) continue;
        __syncthreads(); // s_w is free again
        if (k != k0) { // u_k - w = (u' - w) + (u_k - u'): the domain points are not kept
            Fe<Fr> delta;
            fe_sub<Fr, 2>(delta, P.u[k], uprev);
            fe_reduce_small_2p(delta);
            uprev = P.u[k];
#pragma unroll
            for (int e = 0; e < E; e++) {
                Fe<Fr> t;
                fe_add(t, d[e], delta); // two tight values below 2p
                fe_reduce_small_2p(t);
                fe_select(d[e], j0 + e >= n, one, t);
            }
        }
        Fe<Fr> seed_n, seed_d, h0, h1, g, pre, suf;
        load_elem(seed_n, sn + ((u64)k * tiles + a) * 8);
        load_elem(seed_d, sd + ((u64)k * tiles + a) * 8);
        half_products(h0, h1, g, d);
        block_scan<OpMul, Fr, false>(pre, total, g, seed_n, s_w);
        block_scan<OpMul, Fr, true>(suf, total, g, seed_d, s_w + WAVES * NL);
        fe_zero(acc);
        for_each_inverse(d, h0, h1, pre, suf, [&](auto e, const Fe<Fr> &r) {
            Fe<Fr> t;
            fe_mul(t, x[decltype(e)::value], r); // zero beyond the vector
            fe_reduce_once(t);
            add_canon(acc, acc, t);
        });
        block_scan<OpAdd, Fr, false>(mine, total, acc, zero, s_w + 2 * WAVES * NL);
        if (threadIdx.x == 0) store_elem(part1 + (((u64)p * P.n_points + k) * tiles + a) * 8, total);
    }
}

// launch 4: values[p * n_points + k] = K (u S1 - S0) off the domain, the stored element on it
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_values(const u32 *__restrict__ evals, const u32 *__restrict__ part1, const u32 *__restrict__ part0, u32 *__restrict__ values,
                                                        unsigned log_n, unsigned tiles, Points<Fr> P, ValueConsts<Fr> C)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned p = blockIdx.x / P.n_points, k = blockIdx.x - p * P.n_points;
    const u64 n = (u64)1 << log_n;
    u32 *dst = values + ((u64)p * P.n_points + k) * 8;
    if (P.pos[k] != NONE) {
        if (threadIdx.x == 0) {
            Fe<Fr> v;
            load_elem(v, evals + ((u64)p * n + P.pos[k]) * 8);
            store_elem(dst, v);
        }
        return;
    }
    Fe<Fr> s1, s0;
    fe_zero(s1);
    fe_zero(s0);
    walk_totals<OpAdd, Fr, CE, false>(s1, part1 + ((u64)p * P.n_points + k) * tiles * 8, nullptr, tiles, s_w);
    walk_totals<OpAdd, Fr, CE, false>(s0, part0 + (u64)p * tiles * 8, nullptr, tiles, s_w);
    if (threadIdx.x == 0) {
        Fe<Fr> t1, t0, v;
        fe_mul_shoup<Fr, true>(t1, s1, C.ku[k].w, C.ku[k].q);
        fe_mul_shoup<Fr, true>(t0, s0, C.k[k].w, C.k[k].q);
        fe_sub<Fr, 3>(v, t1, t0);
        store_elem(dst, v);
    }
}

// launch 5: q_i = (e_i - y_p) c / (u - w^i), c = -1 / s, for every position but `pos`.  ON (pos is a position): partq[p * tiles + a] =
// the sum of q_i w^i over those positions of the tile.
template <class Fr, bool ON>
__global__ void __launch_bounds__(THREADS) k_lag_quot(const u32 *evals, u32 *quot, const u32 *__restrict__ sn, const u32 *__restrict__ sd, const u32 *__restrict__ values,
                                                      u32 *__restrict__ partq, unsigned log_n, unsigned tiles, Domain<Fr> D, Fe<Fr> u, u32 pos, Fe<Fr> c)
{
    __shared__ u32 s_w[3 * WAVES * NL];
    const unsigned tile_bits = log_n > (unsigned)(LOG_E + THREAD_BITS) ? log_n - (LOG_E + THREAD_BITS) : 0; // tiles = 2^tile_bits
    const unsigned p = blockIdx.x >> tile_bits, a = blockIdx.x & (tiles - 1);
    const u32 n = 1u << log_n, j0 = a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], d[E], y, seed_n, seed_d, h0, h1, g, pre, suf, total, acc;
    load_run<PadZero, Fr, E>(x, evals + (u64)p * n * 8, j0, n);
    load_elem(y, values + (u64)p * 8);
    load_elem(seed_n, sn + (u64)a * 8);
    load_elem(seed_d, sd + (u64)a * 8);
    fe_mul(seed_d, seed_d, c);
    {
        Fe<Fr> w[E];
        domain_run(w, D, a, log_n);
#pragma unroll
        for (int e = 0; e < E; e++) denominator(d[e], u, w[e], j0 + e, n, pos);
    }
    half_products(h0, h1, g, d);
    block_scan<OpMul, Fr, false>(pre, total, g, seed_n, s_w); // the barriers are behind every load of the workgroup
    block_scan<OpMul, Fr, true>(suf, total, g, seed_d, s_w + WAVES * NL);
    u32 *dst = quot + ((u64)p * n + j0) * 8;
    fe_zero(acc);
    for_each_inverse(d, h0, h1, pre, suf, [&](auto ei, const Fe<Fr> &r) { // r = c / d[e]
        constexpr int e = decltype(ei)::value;
        Fe<Fr> t, q;
        fe_sub<Fr, 1>(t, x[e], y);
        fe_reduce_small_2p(t);
        fe_mul(q, t, r);
        const bool live = j0 + e < n && j0 + e != pos;
        if (live) store_elem(dst + e * 8, q);
        if constexpr (ON) {
            Fe<Fr> w, qw, z;
            fe_sub<Fr, 2>(w, u, d[e]); // w^i = u - (u - w^i) where the position is live
            fe_reduce_small_2p(w);
            fe_mul(qw, q, w);
            fe_reduce_once(qw);
            fe_zero(z);
            fe_select(qw, live, qw, z);
            add_canon(acc, acc, qw);
        }
    });
    if constexpr (ON) {
        Fe<Fr> zero, mine;
        fe_zero(zero);
        block_scan<OpAdd, Fr, false>(mine, total, acc, zero, s_w + 2 * WAVES * NL);
        if (threadIdx.x == 0) store_elem(partq + ((u64)p * tiles + a) * 8, total);
    }
}

// launch 5': quot[p][pos] = cfix * sum of the partials of vector p, cfix = -1 / u
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lag_fix(u32 *__restrict__ quot, const u32 *__restrict__ partq, unsigned log_n, unsigned tiles, u32 pos, FeTw<Fr> cfix)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned p = blockIdx.x;
    Fe<Fr> s;
    fe_zero(s);
    walk_totals<OpAdd, Fr, CE, false>(s, partq + (u64)p * tiles * 8, nullptr, tiles, s_w);
    if (threadIdx.x == 0) {
        Fe<Fr> v;
        fe_mul_shoup<Fr, true>(v, s, cfix.w, cfix.q);
        store_elem(quot + (((u64)p << log_n) + pos) * 8, v);
    }
}

// ------------------------------------------------------------------------------- host side

unsigned bit_reverse(unsigned v, unsigned bits)
{
    unsigned r = 0;
    for (unsigned i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

template <class Fr>
bool same_residue(const Fe<Fr> &a, const Fe<Fr> &b)
{
    u32 wa[8], wb[8];
    fe_to_wire(wa, a);
    fe_to_wire(wb, b);
    return memcmp(wa, wb, sizeof(wa)) == 0;
}

// everything the host derives from (omega, shift, order) and the points; pure arithmetic, no runtime call
template <class Fr>
struct Call {
    unsigned log_n;
    Fe<Fr> pw2[MAX_LOG_ELEMS + 1]; // w^(2^j), internal form
    Fe<Fr> sinv, one;              // 1 / s
    Domain<Fr> dom;
    Points<Fr> pts;
    ValueConsts<Fr> vc;
    FeTw<Fr> cfix[MAXP]; // -1 / u
    CosetTotals<Fr> coset;
    unsigned order;

    // false: omega is not a primitive 2^log_n-th root, or a value is not below the modulus, or the shift is zero
    bool set_domain(unsigned log_n_, const u32 *omega, const u32 *shift, unsigned order_)
    {
        log_n = log_n_, order = order_;
        fe_one(one);
        if (!wire_below_modulus<Fr>(omega) || (shift && !wire_below_modulus<Fr>(shift))) return false;
        fe_from_wire(pw2[0], omega);
        for (unsigned j = 0; j < log_n; j++) fe_sqr(pw2[j + 1], pw2[j]);
        if (log_n == 0) {
            if (!same_residue(pw2[0], one)) return false;
        } else {
            Fe<Fr> t;
            fe_add(t, pw2[log_n - 1], one); // w^(n/2) + 1 = 0
            if (!fe_is_zero_mod_p(t)) return false;
        }
        if (shift) {
            Fe<Fr> s;
            fe_from_wire(s, shift);
            if (fe_is_zero_mod_p(s)) return false;
            fe_inv(sinv, s);
        } else
            sinv = one;
        // w^sigma(2^b): sigma(2^b) = 2^b, or 2^(log_n - 1 - b) in bit-reversed order; one for bits the positions do not have
        auto sig2 = [&](unsigned b) -> const Fe<Fr> & { return b >= log_n ? one : pw2[order == PANDA_DOMAIN_BITREV ? log_n - 1 - b : b]; };
        for (int b = 0; b < DOMAIN_BITS; b++) fe_shoup_prepare(dom.bit[b], sig2(b + LOG_E));
        for (unsigned e = 1; e < (unsigned)E; e++) {
            Fe<Fr> t = one;
            for (unsigned b = 0; b < (unsigned)LOG_E; b++)
                if ((e >> b) & 1) fe_mul(t, t, sig2(b));
            fe_shoup_prepare(dom.run[e - 1], t);
        }
        // w^(Tn sigma(2^b TILE)) in bit-reversed order: sigma(2^b TILE) = 2^(log_n - 1 - b) / TILE, Tn = TILE wherever a tile has bits
        for (unsigned b = 0; b < (unsigned)TILE_BITS; b++) fe_shoup_prepare(coset.tbit[b], b + LOG_E + THREAD_BITS < log_n ? pw2[log_n - 1 - b] : one);
        return true;
    }

    // false: a point is not below the modulus.  u = z / s; on the domain (u^n = 1) the exponent m of u = w^m by Pohlig-Hellman in the
    // 2-group, one bit per step from the lowest, and the position sigma^-1(m).  One field inversion for the whole call: n and the
    // u_k^n - 1 of the points off the domain by the product trick; on the domain 1 / u = u^(n-1), and 1 / w = w^(n-1).
    bool set_points(const u32 *points, unsigned n_points)
    {
        pts.n_points = n_points;
        Fe<Fr> winv = one, inv[MAXP + 1], pre[MAXP + 1], uinv[MAXP], un1[MAXP]; // un1: u^n - 1, canonical
        for (unsigned j = 0; j < log_n; j++) fe_mul(winv, winv, pw2[j]);
        fe_from_u32(inv[0], 1u << log_n);
        for (unsigned k = 0; k < (unsigned)MAXP; k++) {
            fe_zero(pts.u[k]);
            fe_zero(coset.ut[k]);
            fe_zero(pts.inv[k]);
            pts.pos[k] = NONE;
        }
        for (unsigned k = 0; k < n_points; k++) {
            if (!wire_below_modulus<Fr>(points + 8 * k)) return false;
            Fe<Fr> z, u, un;
            fe_from_wire(z, points + 8 * k);
            fe_mul(u, z, sinv);
            pts.u[k] = u;
            un = u;
            uinv[k] = one;
            for (unsigned j = 0; j < log_n; j++) {
                if (j == (unsigned)(LOG_E + THREAD_BITS)) coset.ut[k] = un; // u^TILE
                fe_mul(uinv[k], uinv[k], un); // u^(2^(j+1) - 1)
                fe_sqr(un, un);
            }
            if (log_n <= (unsigned)(LOG_E + THREAD_BITS)) coset.ut[k] = un; // u^n: one ragged tile
            if (same_residue(un, one)) {
                unsigned m = 0;
                Fe<Fr> g = u, wi = winv;
                for (unsigned b = 0; b < log_n; b++) {
                    Fe<Fr> t = g;
                    for (unsigned j = 0; j + 1 + b < log_n; j++) fe_sqr(t, t);
                    if (!same_residue(t, one)) {
                        m |= 1u << b;
                        fe_mul(g, g, wi);
                    }
                    fe_sqr(wi, wi);
                }
                pts.pos[k] = order == PANDA_DOMAIN_BITREV ? bit_reverse(m, log_n) : m;
                inv[1 + k] = one;
            } else {
                Fe<Fr> d;
                fe_sub<Fr, 2>(d, un, one);
                fe_canon(un1[k], d);
                inv[1 + k] = un1[k];
            }
        }
        // inv[i] <- 1 / inv[i]: prefix products, one inversion, back-substitution
        pre[0] = inv[0];
        for (unsigned i = 1; i <= n_points; i++) fe_mul(pre[i], pre[i - 1], inv[i]);
        Fe<Fr> run;
        fe_inv(run, pre[n_points]);
        for (unsigned i = n_points; i > 0; i--) {
            Fe<Fr> t;
            fe_mul(t, run, pre[i - 1]);
            fe_mul(run, run, inv[i]);
            inv[i] = t;
        }
        inv[0] = run;
        const Fe<Fr> &ninv = inv[0];
        for (unsigned k = 0; k < n_points; k++) {
            if (pts.pos[k] != NONE) {
                Fe<Fr> c, cc;
                fe_neg<Fr, 2>(c, uinv[k]);
                fe_canon(cc, c);
                fe_shoup_prepare(cfix[k], cc);
                fe_shoup_prepare(vc.k[k], one);
                fe_shoup_prepare(vc.ku[k], one);
                fe_mul(pts.inv[k], pts.u[k], ninv); // 1 / (n / u)
            } else {
                Fe<Fr> kk, ku;
                fe_mul(kk, un1[k], ninv);
                fe_mul(ku, kk, pts.u[k]);
                fe_shoup_prepare(vc.k[k], kk);
                fe_shoup_prepare(vc.ku[k], ku);
                fe_shoup_prepare(cfix[k], one);
                pts.inv[k] = inv[1 + k]; // 1 / (u^n - 1)
            }
        }
        return true;
    }
};

struct Scratch {
    u32 *tn, *td, *part1, *part0, *values;
};

// A call runs its batch in slices of at most slice_vectors() vectors, so that the per-vector scratch (a partial per tile and point, a
// value per point) stays within SLICE_PARTIALS elements (64 MiB) whatever the batch is: 2^28 one-element vectors at eight points would
// otherwise ask the arena for 128 GiB.  From 2^11 positions a vector on, batch x tiles x points <= 2^20 and a call is one slice.
constexpr u64 SLICE_PARTIALS = (u64)1 << 21;
unsigned slice_vectors(unsigned tiles, unsigned batch, unsigned n_points)
{
    const u64 cap = SLICE_PARTIALS / ((u64)tiles * n_points);
    return cap < 1 ? 1u : (unsigned)(cap < batch ? cap : batch);
}

hipError_t take_all(unsigned tiles, unsigned slice, unsigned n_points, Scratch &s)
{
    const size_t seeds = (size_t)n_points * tiles * 32;
    void *block[5];
    PANDA_TRY(take_scratch({seeds, seeds, (size_t)slice * n_points * tiles * 32, (size_t)slice * tiles * 32, (size_t)slice * n_points * 32}, block));
    s.tn = (u32 *)block[0], s.td = (u32 *)block[1], s.part1 = (u32 *)block[2], s.part0 = (u32 *)block[3], s.values = (u32 *)block[4];
    return hipSuccess;
}

template <class Fr>
bool any_off_domain(const Call<Fr> &c)
{
    bool off = false;
    for (unsigned k = 0; k < c.pts.n_points; k++) off |= c.pts.pos[k] == NONE;
    return off;
}

// launches 1 and 2, once per call: the seeds of every point that takes part.  `skip`: points on the domain take no part (evaluation); a
// division needs their seeds.
template <class Fr>
hipError_t launch_seeds(hipStream_t stream, const Call<Fr> &c, const Scratch &s, bool skip)
{
    const unsigned tiles = tiles_of((u64)1 << c.log_n, TILE), np = c.pts.n_points;
    if (c.order == PANDA_DOMAIN_BITREV && (skip || any_off_domain(c))) { // every point that takes part is off the domain: the totals in closed form
        const unsigned tile_bits = c.log_n > (unsigned)(LOG_E + THREAD_BITS) ? c.log_n - (LOG_E + THREAD_BITS) : 0;
        hipLaunchKernelGGL(k_lag_coset_totals<Fr>, dim3(tiles_of(tiles, THREADS), np), dim3(THREADS), 0, stream, s.tn, tiles, tile_bits, c.coset, c.pts);
    } else
        hipLaunchKernelGGL(k_lag_den_totals<Fr>, dim3(tiles), dim3(THREADS), 0, stream, s.tn, c.log_n, tiles, skip, c.dom, c.pts);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lag_seeds<Fr>, dim3(np), dim3(THREADS), 0, stream, s.tn, s.td, tiles, skip, c.pts);
    return hipGetLastError();
}

// launches 3 and 4 for `count` vectors from d_evals: the values of every point at s.values[p * n_points + k].  Launch 3 runs when some
// point is off the domain.  Grids are one-dimensional, count x tiles <= 2^28 workgroups.
template <class Fr>
hipError_t launch_values(hipStream_t stream, const u32 *d_evals, unsigned count, const Call<Fr> &c, const Scratch &s)
{
    const unsigned tiles = tiles_of((u64)1 << c.log_n, TILE), np = c.pts.n_points;
    if (any_off_domain(c)) {
        hipLaunchKernelGGL(k_lag_eval<Fr>, dim3(count * tiles), dim3(THREADS), 0, stream, d_evals, (const u32 *)s.tn, (const u32 *)s.td, s.part1, s.part0, c.log_n, tiles, c.dom,
                           c.pts);
        PANDA_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lag_values<Fr>, dim3(count * np), dim3(THREADS), 0, stream, d_evals, (const u32 *)s.part1, (const u32 *)s.part0, s.values, c.log_n, tiles, c.pts, c.vc);
    return hipGetLastError();
}

template <class Fr>
hipError_t run_evaluate(hipStream_t stream, const void *d_evals, unsigned batch, const Call<Fr> &c, void *values)
{
    const unsigned np = c.pts.n_points, tiles = tiles_of((u64)1 << c.log_n, TILE), slice = slice_vectors(tiles, batch, np);
    if (panda::extent_too_short(d_evals, ((size_t)batch << c.log_n) * 32)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    Scratch s;
    PANDA_TRY(take_all(tiles, slice, np, s));
    PANDA_TRY(launch_seeds<Fr>(stream, c, s, true));
    for (unsigned first = 0; first < batch; first += slice) { // stream order keeps a slice's values until their copy has run
        const unsigned count = batch - first < slice ? batch - first : slice;
        PANDA_TRY(launch_values<Fr>(stream, (const u32 *)d_evals + ((size_t)first << c.log_n) * 8, count, c, s));
        PANDA_TRY(hipMemcpyAsync((char *)values + (size_t)first * np * 32, s.values, (size_t)count * np * 32, hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t run_divide(hipStream_t stream, const void *d_evals, void *d_quot, unsigned batch, const Call<Fr> &c, void *remainders)
{
    const size_t bytes = ((size_t)batch << c.log_n) * 32;
    if (panda::extent_too_short(d_evals, bytes) || panda::extent_too_short(d_quot, bytes)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    const unsigned tiles = tiles_of((u64)1 << c.log_n, TILE), slice = slice_vectors(tiles, batch, 1);
    Scratch s;
    PANDA_TRY(take_all(tiles, slice, 1, s));
    PANDA_TRY(launch_seeds<Fr>(stream, c, s, false));
    const u32 pos = c.pts.pos[0];
    Fe<Fr> negsinv, t;
    fe_neg<Fr, 2>(t, c.sinv);
    fe_canon(negsinv, t);
    for (unsigned first = 0; first < batch; first += slice) {
        const unsigned count = batch - first < slice ? batch - first : slice;
        const size_t off = ((size_t)first << c.log_n) * 8;
        const u32 *e = (const u32 *)d_evals + off;
        u32 *q = (u32 *)d_quot + off;
        PANDA_TRY(launch_values<Fr>(stream, e, count, c, s));
        if (pos == NONE)
            hipLaunchKernelGGL((k_lag_quot<Fr, false>), dim3(count * tiles), dim3(THREADS), 0, stream, e, q, (const u32 *)s.tn, (const u32 *)s.td, (const u32 *)s.values, s.part0,
                               c.log_n, tiles, c.dom, c.pts.u[0], pos, negsinv);
        else {
            hipLaunchKernelGGL((k_lag_quot<Fr, true>), dim3(count * tiles), dim3(THREADS), 0, stream, e, q, (const u32 *)s.tn, (const u32 *)s.td, (const u32 *)s.values, s.part0,
                               c.log_n, tiles, c.dom, c.pts.u[0], pos, negsinv);
            PANDA_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_lag_fix<Fr>, dim3(count), dim3(THREADS), 0, stream, q, (const u32 *)s.part0, c.log_n, tiles, pos, c.cfix[0]);
        }
        PANDA_TRY(hipGetLastError());
        if (remainders) PANDA_TRY(hipMemcpyAsync((char *)remainders + (size_t)first * 32, s.values, (size_t)count * 32, hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);
}

bool lag_shape_invalid(unsigned log_n, unsigned batch) { return log_n > MAX_LOG_ELEMS || shape_invalid((u64)1 << log_n, batch); }

} // namespace

extern "C" {

// Evaluation of evaluation-form vectors: see include/panda_interface.h.  Every check but the extents comes before any runtime call.
panda_error panda_poly_evaluate_lagrange(unsigned field, const void *d_evals, unsigned log_n, unsigned batch, const void *omega, const void *shift, unsigned order,
                                         const void *points, unsigned n_points, void *values, panda_stream stream)
{
    if (field > 2 || lag_shape_invalid(log_n, batch) || order > PANDA_DOMAIN_BITREV || n_points == 0 || n_points > PANDA_POLY_MAX_POINTS || !d_evals || !omega || !points ||
        !values)
        return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) {
        typedef decltype(fr) Fr;
        Call<Fr> c;
        if (!c.set_domain(log_n, (const u32 *)omega, (const u32 *)shift, order) || !c.set_points((const u32 *)points, n_points)) return panda_error_invalid_value;
        return static_cast<panda_error>(run_evaluate<Fr>(s, d_evals, batch, c, values));
    });
}

// Division by X - z of evaluation-form vectors: see include/panda_interface.h.  Every check but the extents comes before any runtime call.
panda_error panda_poly_divide_linear_lagrange(unsigned field, const void *d_evals, void *d_quot, unsigned log_n, unsigned batch, const void *omega, const void *shift,
                                              unsigned order, const void *point, void *remainders, panda_stream stream)
{
    if (field > 2 || lag_shape_invalid(log_n, batch) || order > PANDA_DOMAIN_BITREV || !d_evals || !d_quot || !omega || !point) return panda_error_invalid_value;
    if (bad_pair(d_evals, d_quot, ((size_t)batch << log_n) * 32)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) {
        typedef decltype(fr) Fr;
        Call<Fr> c;
        if (!c.set_domain(log_n, (const u32 *)omega, (const u32 *)shift, order) || !c.set_points((const u32 *)point, 1)) return panda_error_invalid_value;
        return static_cast<panda_error>(run_divide<Fr>(s, d_evals, d_quot, batch, c, remainders));
    });
}

panda_error panda_poly_lagrange_plan(unsigned log_n, unsigned batch, unsigned n_points, unsigned *tile, unsigned *launches_evaluate, unsigned *launches_divide,
                                     unsigned *inversions_per_vector_and_point)
{
    if (lag_shape_invalid(log_n, batch) || n_points == 0 || n_points > PANDA_POLY_MAX_POINTS) return panda_error_invalid_value;
    if (tile) *tile = TILE;
    if (launches_evaluate) *launches_evaluate = 4;
    if (launches_divide) *launches_divide = 5;
    if (inversions_per_vector_and_point) *inversions_per_vector_and_point = 1;
    return panda_success;
}

} // extern "C"
