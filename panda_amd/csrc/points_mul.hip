// points_mul.hip -- element-wise scalar multiplication of a vector of G1 points (panda_points_scalar_mul, panda_points_scalar_mul_plan);
// DESIGN.md 5.10.  points_mul.h holds what a thread computes and the loop-length rule, ec_ntt.h the group law's bounds and the batch
// normalisation; this file holds the kernels and the host side.
//
// A call over n points runs, on the caller's stream:
//   k_points_mul<F, Fr, MODE, ADD>   point i: the integer k_i (EACH: the wire residue taken to the integer; ONE: the words by value;
//                                    POWERS: c s^i from the by-value table), the wave's longest bit count, k_i P_i over that many
//                                    steps, + A_i with ADD; the XYZZ point goes to arena scratch
//   k_points_normalise<F>            XYZZ -> affine wire points in d_out, one inversion per CHUNK points (ec_ntt.h normalise_chunk)
// d_out is written by the second launch only, after every input has been read: it may be d_points or d_addend.  One wave per workgroup
// in the first kernel; no kernel waits for another workgroup, there are no atomics and no LDS.  In ONE mode the words are kernel
// arguments, so they and every branch on them are scalar; in EACH and POWERS a wave pays the doubling and the addition for every step.
// The point loads and stores and the normalisation's accessors repeat those of ec_ntt.hip, whose kernels are left as they are.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "points_mul.h"
#include "poly_elem.h"

using namespace panda29;
using namespace panda_ecntt;
using namespace panda_pmul;
using panda_poly::ranges_overlap;
using panda_poly::take_scratch;

namespace {

// ------------------------------------------------------------------------------------------------- loads and stores
template <int WORDS>
__device__ __forceinline__ void copy_words_in(u32 *dst, const u32 *src)
{
    static_assert(WORDS % 4 == 0, "whole uint4s");
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
#pragma unroll
    for (int i = 0; i < WORDS / 4; i++) {
        const uint4 v = s4[i];
        dst[4 * i] = v.x, dst[4 * i + 1] = v.y, dst[4 * i + 2] = v.z, dst[4 * i + 3] = v.w;
    }
}
template <int WORDS>
__device__ __forceinline__ void copy_words_out(u32 *dst, const u32 *src)
{
    static_assert(WORDS % 4 == 0, "whole uint4s");
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int i = 0; i < WORDS / 4; i++) d4[i] = make_uint4(src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
}

// a scratch point is the four elements' limbs as they stand: 4 N words
template <class F>
__device__ __forceinline__ void load_point(Xyzz<F> &p, const u32 *pts, u64 i)
{
    constexpr int N = F::N;
    u32 w[4 * N];
    copy_words_in<4 * N>(w, pts + i * (4 * N));
#pragma unroll
    for (int k = 0; k < N; k++) p.X.l[k] = w[k], p.Y.l[k] = w[N + k], p.ZZ.l[k] = w[2 * N + k], p.ZZZ.l[k] = w[3 * N + k];
}
template <class F>
__device__ __forceinline__ void store_point(u32 *pts, u64 i, const Xyzz<F> &p)
{
    constexpr int N = F::N;
    u32 w[4 * N];
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = p.X.l[k], w[N + k] = p.Y.l[k], w[2 * N + k] = p.ZZ.l[k], w[3 * N + k] = p.ZZZ.l[k];
    copy_words_out<4 * N>(pts + i * (4 * N), w);
}

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
    constexpr int L = F::L;
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
    if (live) {
        u32 w[2 * L];
        copy_words_in<2 * L>(w, points + i * (2 * L));
        point_from_affine_wire(p, w);
    }
    panda_pmul::scalar_mul(acc, p, k, bits);
    if (!live) return;
    if constexpr (ADD) {
        u32 w[2 * L];
        copy_words_in<2 * L>(w, addend + i * (2 * L));
        add_affine_wire(acc, w);
    }
    store_point(pts, i, acc);
}

// the accesses of normalise_chunk over scratch points; `first` is the chunk's first point, every index below n by the caller's count
template <class F>
struct XyzzChunk {
    const u32 *__restrict__ pts;
    u32 *__restrict__ out;
    u64 first;
    __device__ __forceinline__ bool denominator(Fe<F> &d, u32 i) const
    {
        constexpr int N = F::N;
        const u32 *src = pts + (first + i) * (4 * N);
        u32 nz = 0;
#pragma unroll
        for (int k = 0; k < N; k++) nz |= src[2 * N + k], d.l[k] = src[3 * N + k];
        return nz != 0;
    }
    __device__ __forceinline__ void put_prefix(u32 i, const Fe<F> &v) const
    {
        u32 *dst = out + (first + i) * (2 * F::L);
#pragma unroll
        for (int k = 0; k < F::N; k++) dst[k] = v.l[k];
    }
    __device__ __forceinline__ void get_prefix(Fe<F> &v, u32 i) const
    {
        const u32 *src = out + (first + i) * (2 * F::L);
#pragma unroll
        for (int k = 0; k < F::N; k++) v.l[k] = src[k];
    }
    __device__ __forceinline__ void finish(u32 i, const Fe<F> &dinv) const
    {
        Xyzz<F> p;
        load_point(p, pts, first + i);
        u32 w[2 * F::L];
        xyzz_affine_wire(w, p, dinv);
        copy_words_out<2 * F::L>(out + (first + i) * (2 * F::L), w);
    }
    __device__ __forceinline__ void put_identity(u32 i) const
    {
        u32 w[2 * F::L] = {};
        copy_words_out<2 * F::L>(out + (first + i) * (2 * F::L), w);
    }
};
static_assert(2 * Bn254Fq::L >= Bn254Fq::N && 2 * Bls377Fq::L >= Bls377Fq::N && 2 * Bls381Fq::L >= Bls381Fq::N, "an output slot holds a prefix product");

template <class F>
__global__ void __launch_bounds__(NORM_THREADS) k_points_normalise(const u32 *__restrict__ pts, u32 *__restrict__ out, u64 n)
{
    const u64 first = ((u64)blockIdx.x * NORM_THREADS + threadIdx.x) * CHUNK;
    if (first >= n) return;
    XyzzChunk<F> io = {pts, out, first};
    normalise_chunk<F>(io, n - first < CHUNK ? (u32)(n - first) : CHUNK);
}

// ------------------------------------------------------------------------------------------------- the host side
template <class Fn>
inline auto with_curve(unsigned curve, Fn &&f)
{
    switch (curve) {
    case 0: return f(Bn254Fq(), Bn254Fr());
    case 1: return f(Bls377Fq(), Bls377Fr());
    default: return f(Bls381Fq(), Bls381Fr());
    }
}

size_t affine_bytes(unsigned curve) { return curve == 0 ? 64 : 96; }
size_t xyzz_bytes(unsigned curve) { return curve == 0 ? 4 * 9 * 4 : 4 * 14 * 4; }
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
hipError_t run_points_mul(hipStream_t stream, unsigned mode, const void *d_points, const void *d_scalars, const Fe<Fr> (&h)[2], const void *d_addend, void *d_out,
                          u64 n)
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
    hipLaunchKernelGGL((k_points_normalise<F>), dim3((unsigned)norm_blocks(n)), dim3(NORM_THREADS), 0, stream, (const u32 *)pts, (u32 *)d_out, n);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

static_assert(sizeof(Xyzz<Bn254Fq>) == 144 && sizeof(Xyzz<Bls377Fq>) == 224 && sizeof(Xyzz<Bls381Fq>) == 224, "the scratch point of the plan");

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
        return static_cast<panda_error>(run_points_mul<F, Fr>(s, mode, d_points, d_scalars, h, d_addend, d_out, n));
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
