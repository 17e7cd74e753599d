// poly_product.hip -- batch inversion and grand products over the scalar fields (panda_field_batch_inverse, panda_poly_grand_product,
// panda_poly_product_plan): the inverse of every element of a vector, and Z_i = prod_{j < i} num_j / den_j -- the
// permutation argument's running product -- with ONE field inversion per vector.
//
//   1 / x_i = (prod_{j < i} x_j) (prod_{j > i} x_j) / prod_all x          Z_i = (prod_{j < i} num_j) (prod_{j >= i} den_j) / prod_all den
//
// so every output is an exclusive prefix product times a suffix product times the inverse of the vector's grand product (Z_0 = 1 comes out
// of the formula).  Reduce-then-scan over tiles of TILE = THREADS * E elements, the launch structure of poly.hip, on the workgroup scan of poly_scan.h
// with the operation OpMul below; no kernel waits for another workgroup:
//   launch 1  k_product_totals  workgroup (p, a) multiplies tile a of vector p down to one element per operand (two for the product call)
//   launch 2  k_product_seeds   one workgroup per vector, CHUNK = THREADS * CE tile totals per step, three walks over the totals: the grand
//                               denominator product, inverted ONCE and multiplied by the call's constant (below); from the last chunk down the
//                               exclusive suffix products of the denominator totals, seeded with that inverse; from the first chunk up the
//                               exclusive prefix products of the numerator totals.  The seeds replace the totals; totals[p] goes to the values.
//   launch 3  k_product_apply   workgroup (p, a) reloads its tile and runs the in-tile prefix and suffix scans from its two seeds.  A thread
//                               stores only the indices it loaded itself, so d_out may be any of the inputs.
// Elements beyond n read as one.  The inverse call replaces a zero by one on load and stores zero at its index.  In the product call a zero
// denominator makes the grand product zero, fe_inv(0) = 0, every suffix seed of the vector zero and with them all n outputs and totals[p].
//
// Arithmetic.  fe_mul(a, b) = a b / R is the field's product on residues x R (R = 2^261).  A wire residue x W (W = 2^256) is that form of
// c x, c = W / R = 2^-5, and is multiplied as it stands (fe_unpack only).  The formulas above are homogeneous: behind every output of the
// inverse call stand n - 1 factors over n, behind every output of the product call n over n, so the power of c they leave is c^-1 and
// c^0 WHATEVER n is, and one constant multiplied into the vector's single inverse -- c^2 and c in that form, i.e. the integers W^2 / R and
// W mod p -- puts every output on the wire form.  d_den == NULL runs the product call with every denominator the wire's one, which keeps
// it homogeneous.  Bounds: every operand of every product is an unpacked canonical residue (tight, < p) or the output of fe_mul (tight,
// < 2p); 4 p^2 < 0.9 R p for all three fields (R / p >= 70).  Nothing is added or subtracted.  Every stored element goes through
// store_elem's reduction.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"

using namespace panda29;
using namespace panda_poly;

namespace {

constexpr int E = 4;  // elements of either operand per thread (the resource listing)
constexpr int CE = 4; // tile totals per thread of the seed kernel
constexpr unsigned TILE = THREADS * E, CHUNK = THREADS * CE;

enum Mode { INVERSE = 0, PRODUCT = 1, RUNNING = 2 }; // RUNNING: PRODUCT with d_den == NULL

// poly_scan.h's operation: the field's product.  Every operand of every product is tight, < 2p (bounds above); the run is the plain chain.
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

// the run from index j0 of the denominators of vector p: loaded for PRODUCT; for RUNNING (den is NULL) `fill` below n and one beyond
template <class Fr, int MODE>
__device__ __forceinline__ void load_den(Fe<Fr> (&x)[E], const u32 *den, unsigned p, u64 j0, u64 n, const Fe<Fr> &fill)
{
    if constexpr (MODE == PRODUCT)
        load_run<OpMul, Fr, E>(x, den + (u64)p * n * 8, j0, n);
    else {
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (j0 + e < n)
                x[e] = fill;
            else
                fe_one(x[e]);
        }
    }
}

// zeros -> one; bit e of the result: x[e] was zero
template <class Fr, int RUN>
__device__ __forceinline__ unsigned mask_zeros(Fe<Fr> (&x)[RUN])
{
    unsigned mask = 0;
    Fe<Fr> one;
    fe_one(one);
#pragma unroll
    for (int e = 0; e < RUN; e++) {
        const bool z = fe_all_zero(x[e]);
        mask |= z ? 1u << e : 0u;
        fe_select(x[e], z, one, x[e]);
    }
    return mask;
}

// launch 1: tn[blk] (and td[blk], but for INVERSE) = the product of tile a = blk % tiles of vector p = blk / tiles
template <class Fr, int MODE>
__global__ void __launch_bounds__(THREADS) k_product_totals(const u32 *__restrict__ num, const u32 *__restrict__ den, u32 *__restrict__ tn, u32 *__restrict__ td, u64 n,
                                                            unsigned tiles, Fe<Fr> fill)
{
    __shared__ u32 s_w[2 * WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const u64 j0 = (u64)a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], g;
    load_run<OpMul, Fr, E>(x, num + (u64)p * n * 8, j0, n);
    if constexpr (MODE == INVERSE) mask_zeros<Fr, E>(x);
    OpMul::run(g, x);
    block_reduce<OpMul>(g, s_w);
    if (threadIdx.x == 0) store_elem(tn + (u64)blk * 8, g);
    if constexpr (MODE != INVERSE) {
        load_den<Fr, MODE>(x, den, p, j0, n, fill);
        OpMul::run(g, x);
        block_reduce<OpMul>(g, s_w + WAVES * NL);
        if (threadIdx.x == 0) store_elem(td + (u64)blk * 8, g);
    }
}

// launch 2: one workgroup per vector.  INV: both operands are tn (read only in the first two walks) and td only receives the suffix
// seeds; otherwise td is replaced in place, every thread storing the indices it loaded.  fold: the call's constant.
template <class Fr, bool INV>
__global__ void __launch_bounds__(THREADS) k_product_seeds(u32 *tn, u32 *td, u32 *__restrict__ values, unsigned tiles, Fe<Fr> fold)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned p = blockIdx.x;
    u32 *N = tn + (u64)p * tiles * 8, *D = td + (u64)p * tiles * 8;
    const u32 *Din = INV ? N : D;
    Fe<Fr> carry, inv;
    // the grand product of the denominator totals and its inverse
    fe_one(carry);
    walk_totals<OpMul, Fr, CE, false>(carry, Din, nullptr, tiles, s_w);
    fe_inv(inv, carry); // zero for zero
    fe_mul(inv, inv, fold);
    // suffix seeds, from the last chunk down: D_a = inv * prod_{b > a} den total b.  walk_totals' steps the other way round, spelled out:
    // through a REV parameter of that function this kernel's INV form came out at five waves per SIMD instead of four.
    carry = inv;
    for (unsigned k = tiles_of(tiles, CHUNK); k-- > 0;) {
        const u64 a0 = (u64)k * CHUNK + threadIdx.x * CE;
        Fe<Fr> x[CE], g, s, total;
        load_run<OpMul, Fr, CE>(x, Din, a0, tiles);
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
    // prefix seeds, from the first chunk up: N_a = prod_{b < a} num total b
    fe_one(carry);
    walk_totals<OpMul, Fr, CE, true>(carry, N, N, tiles, s_w);
    if constexpr (!INV) {
        if (threadIdx.x == 0) {
            fe_mul(carry, carry, inv);
            store_elem(values + (u64)p * 8, carry);
        }
    }
}

// launch 3: the outputs of tile a of vector p from the seeds sn[blk], sd[blk]
template <class Fr, int MODE>
__global__ void __launch_bounds__(THREADS) k_product_apply(const u32 *num, const u32 *den, u32 *out, const u32 *__restrict__ sn, const u32 *__restrict__ sd, u64 n,
                                                           unsigned tiles, Fe<Fr> fill)
{
    __shared__ u32 s_w[2 * WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const u64 j0 = (u64)a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], d[E], gn, gd;
    unsigned zeros = 0;
    load_run<OpMul, Fr, E>(x, num + (u64)p * n * 8, j0, n);
    if constexpr (MODE == INVERSE) {
        zeros = mask_zeros<Fr, E>(x);
#pragma unroll
        for (int e = 0; e < E; e++) d[e] = x[e];
    } else
        load_den<Fr, MODE>(d, den, p, j0, n, fill);
    OpMul::run(gn, x);
    if constexpr (MODE == INVERSE)
        gd = gn;
    else
        OpMul::run(gd, d);
    Fe<Fr> seed_n, seed_d, pre, suf, total;
    load_elem(seed_n, sn + (u64)blk * 8);
    load_elem(seed_d, sd + (u64)blk * 8);
    block_scan<OpMul, Fr, false>(pre, total, gn, seed_n, s_w);
    block_scan<OpMul, Fr, true>(suf, total, gd, seed_d, s_w + WAVES * NL);
    // x[e] <- the exclusive prefix product at element e
#pragma unroll
    for (int e = 0; e < E; e++) {
        const Fe<Fr> t = x[e];
        x[e] = pre;
        if (e < E - 1) fe_mul(pre, pre, t);
    }
    // the suffix product from the run's right end down: exclusive of element e for the inverse, inclusive for the product
    u32 *dst = out + ((u64)p * n + j0) * 8;
#pragma unroll
    for (int e = E - 1; e >= 0; e--) {
        if constexpr (MODE != INVERSE) fe_mul(suf, suf, d[e]);
        Fe<Fr> r;
        fe_mul(r, x[e], suf);
        if constexpr (MODE == INVERSE) {
            if ((zeros >> e) & 1) fe_zero(r);
            if (e > 0) fe_mul(suf, suf, d[e]);
        }
        if (j0 + e < n) store_elem(dst + e * 8, r);
    }
}

// ------------------------------------------------------------------------------- host side

// two totals per tile and a value per vector
hipError_t take_totals(u64 n, unsigned batch, u32 **d_tn, u32 **d_td, u32 **d_values)
{
    const size_t tbytes = (size_t)batch * tiles_of(n, TILE) * 32;
    void *block[3];
    PANDA_TRY(take_scratch({tbytes, tbytes, (size_t)batch * 32}, block));
    *d_tn = (u32 *)block[0], *d_td = (u32 *)block[1], *d_values = (u32 *)block[2];
    return hipSuccess;
}

// the wire's one as the kernels hold it: the integer W mod p, which is c = W / R in the form fe_mul multiplies
template <class Fr>
void wire_one(Fe<Fr> &c)
{
    Fe<Fr> one;
    fe_one(one);
    u32 w[8];
    fe_to_wire(w, one);
    fe_unpack(c, w);
}

template <class Fr, int MODE>
hipError_t launch_all(hipStream_t stream, const u32 *d_num, const u32 *d_den, u32 *d_out, u64 n, unsigned batch, u32 *d_tn, u32 *d_td, u32 *d_values)
{
    Fe<Fr> c, fold;
    wire_one(c);
    if (MODE == INVERSE)
        fe_mul(fold, c, c); // c^2
    else
        fold = c;
    const unsigned tiles = tiles_of(n, TILE);
    hipLaunchKernelGGL((k_product_totals<Fr, MODE>), dim3(batch * tiles), dim3(THREADS), 0, stream, d_num, d_den, d_tn, d_td, n, tiles, c);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_product_seeds<Fr, MODE == INVERSE>), dim3(batch), dim3(THREADS), 0, stream, d_tn, d_td, d_values, tiles, fold);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_product_apply<Fr, MODE>), dim3(batch * tiles), dim3(THREADS), 0, stream, d_num, d_den, d_out, (const u32 *)d_tn, (const u32 *)d_td, n, tiles, c);
    return hipGetLastError();
}

template <class Fr>
hipError_t call_inverse(hipStream_t stream, const void *d_in, void *d_out, u64 n)
{
    const size_t bytes = (size_t)n * 32;
    if (panda::extent_too_short(d_in, bytes) || panda::extent_too_short(d_out, bytes)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    u32 *d_tn = nullptr, *d_td = nullptr, *d_values = nullptr;
    PANDA_TRY(take_totals(n, 1, &d_tn, &d_td, &d_values));
    PANDA_TRY((launch_all<Fr, INVERSE>(stream, (const u32 *)d_in, nullptr, (u32 *)d_out, n, 1, d_tn, d_td, d_values)));
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t call_product(hipStream_t stream, const void *d_num, const void *d_den, void *d_out, u64 n, unsigned batch, void *totals)
{
    const size_t bytes = (size_t)batch * n * 32;
    if (panda::extent_too_short(d_num, bytes) || (d_den && panda::extent_too_short(d_den, bytes)) || panda::extent_too_short(d_out, bytes)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    u32 *d_tn = nullptr, *d_td = nullptr, *d_values = nullptr;
    PANDA_TRY(take_totals(n, batch, &d_tn, &d_td, &d_values));
    if (d_den)
        PANDA_TRY((launch_all<Fr, PRODUCT>(stream, (const u32 *)d_num, (const u32 *)d_den, (u32 *)d_out, n, batch, d_tn, d_td, d_values)));
    else
        PANDA_TRY((launch_all<Fr, RUNNING>(stream, (const u32 *)d_num, nullptr, (u32 *)d_out, n, batch, d_tn, d_td, d_values)));
    if (totals) PANDA_TRY(hipMemcpyAsync(totals, d_values, (size_t)batch * 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The inverse of every element: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_field_batch_inverse(unsigned field, const void *d_in, void *d_out, uint64_t n, panda_stream stream)
{
    if (field > 2 || shape_invalid(n, 1) || !d_in || !d_out || bad_pair(d_in, d_out, (size_t)n * 32)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(call_inverse<decltype(fr)>(s, d_in, d_out, n)); });
}

// The running product of num / den: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_poly_grand_product(unsigned field, const void *d_num, const void *d_den, void *d_out, uint64_t n, unsigned batch, void *totals, panda_stream stream)
{
    if (field > 2 || shape_invalid(n, batch) || !d_num || !d_out) return panda_error_invalid_value;
    const size_t bytes = (size_t)batch * n * 32;
    if (bad_pair(d_num, d_out, bytes) || (d_den && (bad_pair(d_den, d_out, bytes) || bad_pair(d_num, d_den, bytes)))) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(call_product<decltype(fr)>(s, d_num, d_den, d_out, n, batch, totals)); });
}

panda_error panda_poly_product_plan(uint64_t n, unsigned batch, unsigned *tile_inverse, unsigned *tile_product, unsigned *carry_chunk, unsigned *launches)
{
    if (shape_invalid(n, batch)) return panda_error_invalid_value;
    if (tile_inverse) *tile_inverse = TILE;
    if (tile_product) *tile_product = TILE;
    if (carry_chunk) *carry_chunk = CHUNK;
    if (launches) *launches = 3;
    return panda_success;
}

} // extern "C"
