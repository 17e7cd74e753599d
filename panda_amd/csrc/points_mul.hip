// points_mul.hip -- element-wise scalar multiplication of a vector of G1 points (panda_points_scalar_mul, panda_points_scalar_mul_plan);
// DESIGN.md 5.10.  points_mul.h holds what a thread computes and the loop-length rule, ec_ntt.h the group law's bounds and the batch
// normalisation; this file holds the kernels and the host side.
//
// A call over n points runs, on the caller's stream:
//   k_points_mul<F, Fr, MODE, ADD>   point i: the integer k_i (EACH: the wire residue taken to the integer; ONE: the words by value;
//                                    POWERS: c s^i from the by-value table), the wave's longest bit count, k_i P_i over that many
//                                    steps, + A_i with ADD; the XYZZ point goes to arena scratch
//   k_normalise<F>                   of ec_ntt.hip through enqueue_normalise: XYZZ -> affine wire points in d_out, one inversion per
//                                    CHUNK points (ec_ntt.h normalise_chunk)
// d_out is written by the second launch only, after every input has been read: it may be d_points or d_addend.  One wave per workgroup
// in the first kernel; no kernel waits for another workgroup, there are no atomics and no LDS.  In ONE mode the words are kernel
// arguments, so they and every branch on them are scalar; in EACH and POWERS a wave pays the doubling and the addition for every step.
// The point loads and stores, the sizes and the curve dispatch are point_vec.h's, shared with ec_ntt.hip.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "point_vec.h"
#include "points_mul.h"
#include "poly_elem.h"

using namespace panda29;
using namespace panda_ecntt;
using namespace panda_pmul;
using panda_poly::ranges_overlap;
using panda_poly::take_scratch;

namespace {

// ------------------------------------------------------------------------------------------------- kernels
// what a mode passes by value
template <class Fr, unsigned MODE>
struct MulArgs {}; // EACH: nothing
template <class Fr>
struct MulArgs<Fr, MODE_ONE> {
    u32 w[SCALAR_WORDS]; // the integer
};
template <class Fr>
struct MulArgs<Fr, MODE_POWERS> {
    PowerTable<Fr> table;
};

// the largest of the wave's values, in every lane (one wave per workgroup, all 64 lanes present)
__device__ __forceinline__ unsigned wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

template <class F, class Fr, unsigned MODE, bool ADD>
__global__ void __launch_bounds__(MUL_THREADS) k_points_mul(const u32 *__restrict__ points, const u32 *__restrict__ scalars, const u32 *__restrict__ addend,
                                                            u32 *__restrict__ pts, u64 n, const MulArgs<Fr, MODE> args)
{
    const u64 i = (u64)blockIdx.x * MUL_THREADS + threadIdx.x;
    const bool live = i < n; // the last wave's tail runs the loop with k = 0 over the identity and stores nothing
    u32 k[SCALAR_WORDS] = {};
    unsigned bits;
    if constexpr (MODE == MODE_ONE) {
#pragma unroll
        for (int j = 0; j < SCALAR_WORDS; j++) k[j] = args.w[j];
        bits = scalar_bits(k);
    } else {
        if (live) {
            if constexpr (MODE == MODE_EACH) {
                u32 wire[SCALAR_WORDS];
                copy_words_in<SCALAR_WORDS>(wire, scalars + i * SCALAR_WORDS);
                scalar_from_wire<Fr>(k, wire);
            } else
                power_scalar(k, args.table, (u32)i);
        }
        bits = wave_max(scalar_bits(k));
    }
    Xyzz<F> p, acc;
    xyzz_set_identity(p);
    if (live) load_affine(p, points, i);
    panda_pmul::scalar_mul(acc, p, k, bits);
    if (!live) return;
    if constexpr (ADD) {
        u32 w[2 * F::L];
        copy_words_in<2 * F::L>(w, addend + i * (2 * F::L));
        add_affine_wire(acc, w);
    }
    store_point(pts, i, acc);
}

// ------------------------------------------------------------------------------------------------- the host side
bool shape_invalid(unsigned curve, unsigned mode, u64 n) { return curve > 2 || mode > MODE_POWERS || n == 0 || n > MAX_POINTS; }

template <class F, class Fr, unsigned MODE>
hipError_t launch_mul(hipStream_t stream, const void *d_points, const void *d_scalars, const void *d_addend, u32 *pts, u64 n, const MulArgs<Fr, MODE> &args)
{
    const dim3 grid((unsigned)mul_blocks(n)), block(MUL_THREADS);
    if (d_addend)
        hipLaunchKernelGGL((k_points_mul<F, Fr, MODE, true>), grid, block, 0, stream, (const u32 *)d_points, (const u32 *)d_scalars, (const u32 *)d_addend, pts, n, args);
    else
        hipLaunchKernelGGL((k_points_mul<F, Fr, MODE, false>), grid, block, 0, stream, (const u32 *)d_points, (const u32 *)d_scalars, (const u32 *)nullptr, pts, n, args);
    return hipGetLastError();
}

// h: the host scalars of the mode in internal form (ONE: h[0]; POWERS: h[0] = c, h[1] = s)
template <class F, class Fr>
hipError_t run_points_mul(unsigned curve, hipStream_t stream, unsigned mode, const void *d_points, const void *d_scalars, const Fe<Fr> (&h)[2], const void *d_addend,
                          void *d_out, u64 n)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    void *block[1];
    PANDA_TRY(take_scratch({(size_t)n * sizeof(Xyzz<F>)}, block));
    u32 *pts = (u32 *)block[0];
    if (mode == MODE_EACH) {
        PANDA_TRY((launch_mul<F, Fr, MODE_EACH>(stream, d_points, d_scalars, d_addend, pts, n, MulArgs<Fr, MODE_EACH>())));
    } else if (mode == MODE_ONE) {
        MulArgs<Fr, MODE_ONE> a;
        scalar_from_internal(a.w, h[0]);
        PANDA_TRY((launch_mul<F, Fr, MODE_ONE>(stream, d_points, nullptr, d_addend, pts, n, a)));
    } else {
        MulArgs<Fr, MODE_POWERS> a;
        power_table(a.table, h[0], h[1]);
        PANDA_TRY((launch_mul<F, Fr, MODE_POWERS>(stream, d_points, nullptr, d_addend, pts, n, a)));
    }
    PANDA_TRY(enqueue_normalise(curve, stream, pts, (u32 *)d_out, n));
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The calls: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_points_scalar_mul(unsigned curve, unsigned mode, const void *d_points, const void *d_scalars, const void *h_scalars, const void *d_addend,
                                    void *d_out, uint64_t n, panda_stream stream)
{
    if (shape_invalid(curve, mode, n) || !d_points || !d_out) return panda_error_invalid_value;
    if (mode == MODE_EACH ? (!d_scalars || h_scalars) : (!h_scalars || d_scalars)) return panda_error_invalid_value;
    const size_t bytes = (size_t)n * affine_bytes(curve);
    // d_out may be one of the point inputs exactly; every other overlap among the three is refused
    if (d_out != d_points && ranges_overlap(d_out, bytes, d_points, bytes)) return panda_error_invalid_value;
    if (d_addend) {
        if (d_out != d_addend && ranges_overlap(d_out, bytes, d_addend, bytes)) return panda_error_invalid_value;
        if (ranges_overlap(d_points, bytes, d_addend, bytes)) return panda_error_invalid_value;
    }
    if (panda::extent_too_short(d_points, bytes) || panda::extent_too_short(d_out, bytes) || (d_addend && panda::extent_too_short(d_addend, bytes)) ||
        (d_scalars && panda::extent_too_short(d_scalars, (size_t)n * 4 * SCALAR_WORDS)))
        return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_curve(curve, [&](auto fq, auto fr) {
        typedef decltype(fq) F;
        typedef decltype(fr) Fr;
        Fe<Fr> h[2];
        fe_zero(h[0]), fe_zero(h[1]);
        for (unsigned j = 0; j < mode; j++) { // ONE: one scalar, POWERS: two
            u32 w[SCALAR_WORDS];
            memcpy(w, (const char *)h_scalars + j * sizeof w, sizeof w);
            if (!panda_poly::wire_below_modulus<Fr>(w)) return panda_error_invalid_value;
            fe_from_wire(h[j], w);
        }
        return static_cast<panda_error>(run_points_mul<F, Fr>(curve, s, mode, d_points, d_scalars, h, d_addend, d_out, n));
    });
}

panda_error panda_points_scalar_mul_plan(unsigned curve, unsigned mode, uint64_t n, unsigned *launches, size_t *scratch_bytes)
{
    if (shape_invalid(curve, mode, n)) return panda_error_invalid_value;
    if (launches) *launches = 2;
    if (scratch_bytes) *scratch_bytes = panda::align256((size_t)n * xyzz_bytes(curve)) + 256;
    return panda_success;
}

} // extern "C"
