// ec_ntt.hip -- the discrete Fourier transform over G1 points (panda_ec_ntt, panda_ec_ntt_plan) and the batch conversion of MSM result
// triples to affine points (panda_points_to_affine, panda_points_to_affine_plan); DESIGN.md 5.9.  ec_ntt.h holds what a thread computes,
// the bounds and the treatment of the exceptional cases, point_vec.h the point loads and stores shared with points_mul.hip; this file
// holds the kernels and the host side.
//
// A transform of n = 2^log_n points runs, on the caller's stream:
//   k_twiddles     log_n >= 2: the n / 2 canonical (plain-integer) powers of the root, 32 B each, into scratch.  Built by every call: a
//                  table entry is log_n field products, a butterfly several thousand.
//   k_first        stage 1 (w = 1): reads the affine wire points through the bit reversal, writes A + B, A - B as XYZZ into scratch
//   k_stage        stages 2 .. log_n in place over the scratch points, one launch each; butterfly t = blockIdx 64 + lane is twiddle-major
//                  (ec_ntt.h butterfly_index), so where n / m >= 64 a wave's lanes share w: k_stage<F, true> takes the words through
//                  readfirstlane, so they and every branch on them are scalar.  k_stage<F, false> runs the other stages.
//   k_scale        inverse only: every point times n^-1, one scalar for the launch (uniform everywhere)
//   k_normalise    XYZZ -> affine wire points in d_out, one inversion per CHUNK points (ec_ntt.h normalise_chunk); the prefix products
//                  are parked in the output slots themselves, so the normalisation needs no scratch of its own.  Compiled here only:
//                  points_mul.hip reaches it through enqueue_normalise (point_vec.h)
// No kernel waits for another workgroup and there are no atomics; every launch is ordered by the stream.  The stage kernels are one wave
// per workgroup (__launch_bounds__(64)): the 14-limb butterfly takes the 256 VGPRs, keeps a few values in AGPRs and needs no scratch memory.
// The intermediate points and the table live in the calling thread's arena (released by panda_ntt_tear_down).
#include <string.h>

#include "ec_ntt.h"
#include "fe29.h"
#include "panda_internal.h"
#include "point_vec.h"
#include "poly_elem.h"

using namespace panda29;
using namespace panda_ecntt;
using panda_poly::ranges_overlap;
using panda_poly::take_scratch;

namespace {

struct ScalarWords {
    u32 w[SCALAR_WORDS];
};

// ------------------------------------------------------------------------------------------------- kernels
template <class Fr>
struct RootPowers {
    Fe<Fr> sq[MAX_LOG_N]; // sq[b] = root^(2^b), internal form
};

// table[i] = root^i as a plain integer below r, i < half
template <class Fr>
__global__ void __launch_bounds__(256) k_twiddles(u32 *__restrict__ table, u32 half, const RootPowers<Fr> rp)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= half) return;
    Fe<Fr> acc, t;
    fe_one(acc);
#pragma unroll
    for (int b = 0; b < (int)MAX_LOG_N - 1; b++) { // statically indexed; i < 2^25
        fe_mul(t, acc, rp.sq[b]);
        fe_select(acc, ((i >> b) & 1u) != 0, t, acc);
    }
    u32 w[SCALAR_WORDS];
    scalar_from_internal(w, acc);
    copy_words_out<SCALAR_WORDS>(table + (u64)i * SCALAR_WORDS, w);
}

// stage 1, or the lone point of log_n == 0
template <class F>
__global__ void __launch_bounds__(STAGE_THREADS) k_first(const u32 *__restrict__ in, u32 *__restrict__ pts, unsigned log_n)
{
    const u32 t = blockIdx.x * STAGE_THREADS + threadIdx.x;
    if (log_n == 0) {
        if (t == 0) {
            Xyzz<F> p;
            load_affine(p, in, 0);
            store_point(pts, 0, p);
        }
        return;
    }
    if (t >= ((u32)1 << (log_n - 1))) return;
    const u32 ia = bit_reverse(2 * t, log_n), ib = bit_reverse(2 * t + 1, log_n);
    Xyzz<F> b;
    load_affine(b, in, ib);
    butterfly(b, [&](Xyzz<F> &a) { load_affine(a, in, ia); }, [&](const Xyzz<F> &v) { store_point(pts, 2 * (u64)t, v); },
              [&](const Xyzz<F> &v) { store_point(pts, 2 * (u64)t + 1, v); });
}

template <class F, bool UNIFORM>
__global__ void __launch_bounds__(STAGE_THREADS) k_stage(u32 *pts, const u32 *__restrict__ table, unsigned log_n, unsigned s)
{
    const u32 t = blockIdx.x * STAGE_THREADS + threadIdx.x;
    if (t >= ((u32)1 << (log_n - 1))) return; // only where n / 2 < 64: the whole wave's tail, and the stage is not a uniform one
    const ButterflyIndex ix = butterfly_index(t, log_n, s);
    u32 w[SCALAR_WORDS];
    copy_words_in<SCALAR_WORDS>(w, table + (u64)ix.twiddle * SCALAR_WORDS);
    if (UNIFORM) {
#pragma unroll
        for (int i = 0; i < SCALAR_WORDS; i++) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
    }
    Xyzz<F> b, wb;
    load_point(b, pts, ix.hi);
    scalar_mul(wb, b, w);
    butterfly(wb, [&](Xyzz<F> &a) { load_point(a, pts, ix.lo); }, [&](const Xyzz<F> &v) { store_point(pts, ix.lo, v); },
              [&](const Xyzz<F> &v) { store_point(pts, ix.hi, v); });
}

template <class F>
__global__ void __launch_bounds__(STAGE_THREADS) k_scale(u32 *pts, u32 n, const ScalarWords k)
{
    const u32 i = blockIdx.x * STAGE_THREADS + threadIdx.x;
    if (i >= n) return;
    Xyzz<F> p, r;
    load_point(p, pts, i);
    scalar_mul(r, p, k.w);
    store_point(pts, i, r);
}

// the output side of normalise_chunk's accesses: `first` is the chunk's first point, every index below n by the caller's count.  A
// prefix product is parked in the point's own output slot (point_vec.h asserts that it fits).
template <class F>
struct OutSlots {
    u32 *__restrict__ out;
    u64 first;
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
    __device__ __forceinline__ void put_identity(u32 i) const
    {
        u32 w[2 * F::L] = {};
        copy_words_out<2 * F::L>(out + (first + i) * (2 * F::L), w);
    }
};

// the accesses of normalise_chunk over scratch points
template <class F>
struct XyzzChunk : OutSlots<F> {
    const u32 *__restrict__ pts;
    using OutSlots<F>::first;
    using OutSlots<F>::out;
    __device__ __forceinline__ bool denominator(Fe<F> &d, u32 i) const
    {
        constexpr int N = F::N;
        const u32 *src = pts + (first + i) * (4 * N);
        u32 nz = 0;
#pragma unroll
        for (int k = 0; k < N; k++) nz |= src[2 * N + k], d.l[k] = src[3 * N + k];
        return nz != 0;
    }
    __device__ __forceinline__ void finish(u32 i, const Fe<F> &dinv) const
    {
        Xyzz<F> p;
        load_point(p, pts, first + i);
        u32 w[2 * F::L];
        xyzz_affine_wire(w, p, dinv);
        copy_words_out<2 * F::L>(out + (first + i) * (2 * F::L), w);
    }
};

// the same over X || Y || Z wire triples
template <class F>
struct TripleChunk : OutSlots<F> {
    const u32 *__restrict__ in;
    bool homogeneous;
    using OutSlots<F>::first;
    using OutSlots<F>::out;
    __device__ __forceinline__ bool denominator(Fe<F> &d, u32 i) const
    {
        u32 z[F::L];
        copy_words_in<F::L>(z, in + (first + i) * (3 * F::L) + 2 * F::L);
        return triple_denominator<F>(d, z);
    }
    __device__ __forceinline__ void finish(u32 i, const Fe<F> &dinv) const
    {
        u32 t[3 * F::L], w[2 * F::L];
        copy_words_in<2 * F::L>(t, in + (first + i) * (3 * F::L));
        triple_affine_wire<F>(w, t, dinv, homogeneous);
        copy_words_out<2 * F::L>(out + (first + i) * (2 * F::L), w);
    }
};

template <class F>
__global__ void __launch_bounds__(NORM_THREADS) k_normalise(const u32 *__restrict__ pts, u32 *__restrict__ out, u64 n)
{
    const u64 first = ((u64)blockIdx.x * NORM_THREADS + threadIdx.x) * CHUNK;
    if (first >= n) return;
    XyzzChunk<F> io = {{out, first}, pts};
    normalise_chunk<F>(io, n - first < CHUNK ? (u32)(n - first) : CHUNK);
}

template <class F>
__global__ void __launch_bounds__(NORM_THREADS) k_normalise_triples(const u32 *__restrict__ in, u32 *__restrict__ out, u64 n, bool homogeneous)
{
    const u64 first = ((u64)blockIdx.x * NORM_THREADS + threadIdx.x) * CHUNK;
    if (first >= n) return;
    TripleChunk<F> io = {{out, first}, in, homogeneous};
    normalise_chunk<F>(io, n - first < CHUNK ? (u32)(n - first) : CHUNK);
}

// ------------------------------------------------------------------------------------------------- the host side
unsigned ntt_launches(unsigned log_n, unsigned direction)
{
    if (log_n == 0) return 2;
    return (log_n >= 2 ? 1u : 0u) + log_n + (direction == PANDA_EC_NTT_INVERSE ? 1u : 0u) + 1u;
}
size_t ntt_scratch_bytes(unsigned curve, unsigned log_n)
{
    const size_t n = (size_t)1 << log_n;
    return panda::align256(n * xyzz_bytes(curve)) + panda::align256((n / 2 ? n / 2 : 1) * 4 * SCALAR_WORDS) + 2 * 256;
}

// the forward root of a transform of 2^log_n points: below the modulus, and for log_n >= 1 of order exactly 2^log_n
template <class Fr>
bool root_valid(const u32 *omega_wire, unsigned log_n, Fe<Fr> &root)
{
    if (log_n == 0) { // a copy: omega is not read
        fe_one(root);
        return true;
    }
    if (!panda_poly::wire_below_modulus<Fr>(omega_wire)) return false;
    fe_from_wire(root, omega_wire);
    return order_is_pow2(root, log_n); // root^(n / 2) == -1
}

template <class F, class Fr>
hipError_t run_ec_ntt(unsigned curve, hipStream_t stream, const void *d_in, void *d_out, unsigned log_n, bool inverse, const Fe<Fr> &omega)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    const u32 n = (u32)1 << log_n, half = n / 2;
    void *block[2]; // the points, the table
    PANDA_TRY(take_scratch({(size_t)n * sizeof(Xyzz<F>), (size_t)(half ? half : 1) * 4 * SCALAR_WORDS}, block));
    u32 *pts = (u32 *)block[0], *table = (u32 *)block[1];
    Fe<Fr> root = omega;
    if (inverse && log_n > 0) fe_inv(root, omega);
    if (log_n >= 2) {
        RootPowers<Fr> rp;
        Fe<Fr> one;
        fe_one(one);
        for (unsigned b = 0; b < MAX_LOG_N; b++) {
            rp.sq[b] = b == 0 ? root : one;
            if (b > 0 && b + 1 < log_n) fe_sqr(rp.sq[b], rp.sq[b - 1]); // bits of i < n / 2 only
        }
        hipLaunchKernelGGL((k_twiddles<Fr>), dim3((half + 255) / 256), dim3(256), 0, stream, table, half, rp);
        PANDA_TRY(hipGetLastError());
    }
    const unsigned blocks = half > STAGE_THREADS ? half / STAGE_THREADS : 1;
    hipLaunchKernelGGL((k_first<F>), dim3(blocks), dim3(STAGE_THREADS), 0, stream, (const u32 *)d_in, pts, log_n);
    PANDA_TRY(hipGetLastError());
    for (unsigned s = 2; s <= log_n; s++) {
        if ((n >> s) >= UNIFORM_MIN_SHARERS)
            hipLaunchKernelGGL((k_stage<F, true>), dim3(blocks), dim3(STAGE_THREADS), 0, stream, pts, (const u32 *)table, log_n, s);
        else
            hipLaunchKernelGGL((k_stage<F, false>), dim3(blocks), dim3(STAGE_THREADS), 0, stream, pts, (const u32 *)table, log_n, s);
        PANDA_TRY(hipGetLastError());
    }
    if (inverse && log_n > 0) {
        Fe<Fr> nf, ninv;
        fe_from_u32(nf, n);
        fe_inv(ninv, nf);
        ScalarWords k;
        scalar_from_internal(k.w, ninv);
        hipLaunchKernelGGL((k_scale<F>), dim3((n + STAGE_THREADS - 1) / STAGE_THREADS), dim3(STAGE_THREADS), 0, stream, pts, n, k);
        PANDA_TRY(hipGetLastError());
    }
    PANDA_TRY(enqueue_normalise(curve, stream, pts, (u32 *)d_out, n));
    return hipStreamSynchronize(stream);
}

template <class F>
hipError_t run_to_affine(hipStream_t stream, const void *d_in, void *d_out, u64 n, bool homogeneous)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    hipLaunchKernelGGL((k_normalise_triples<F>), dim3((unsigned)norm_blocks(n)), dim3(NORM_THREADS), 0, stream, (const u32 *)d_in, (u32 *)d_out, n, homogeneous);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

} // namespace

hipError_t panda_ecntt::enqueue_normalise(unsigned curve, hipStream_t stream, const u32 *pts, u32 *out, u64 n)
{
    return with_curve(curve, [&](auto fq, auto) {
        hipLaunchKernelGGL((k_normalise<decltype(fq)>), dim3((unsigned)norm_blocks(n)), dim3(NORM_THREADS), 0, stream, pts, out, n);
        return hipGetLastError();
    });
}

extern "C" {

// The calls: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_ec_ntt(unsigned curve, const void *d_in, void *d_out, unsigned log_n, unsigned direction, const void *omega, panda_stream stream)
{
    if (curve > 2 || log_n > MAX_LOG_N || direction > PANDA_EC_NTT_INVERSE || !d_in || !d_out || !omega) return panda_error_invalid_value;
    const size_t bytes = ((size_t)1 << log_n) * affine_bytes(curve);
    if (d_in != d_out && ranges_overlap(d_in, bytes, d_out, bytes)) return panda_error_invalid_value;
    if (panda::extent_too_short(d_in, bytes) || panda::extent_too_short(d_out, bytes)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_curve(curve, [&](auto fq, auto fr) {
        typedef decltype(fq) F;
        typedef decltype(fr) Fr;
        u32 w[SCALAR_WORDS] = {};
        if (log_n > 0) memcpy(w, omega, sizeof w);
        Fe<Fr> root;
        if (!root_valid<Fr>(w, log_n, root)) return panda_error_invalid_value;
        return static_cast<panda_error>(run_ec_ntt<F, Fr>(curve, s, d_in, d_out, log_n, direction == PANDA_EC_NTT_INVERSE, root));
    });
}

panda_error panda_ec_ntt_plan(unsigned curve, unsigned log_n, unsigned direction, unsigned *launches, size_t *scratch_bytes, unsigned *uniform_stages)
{
    if (curve > 2 || log_n > MAX_LOG_N || direction > PANDA_EC_NTT_INVERSE) return panda_error_invalid_value;
    if (launches) *launches = ntt_launches(log_n, direction);
    if (scratch_bytes) *scratch_bytes = ntt_scratch_bytes(curve, log_n);
    if (uniform_stages) *uniform_stages = panda_ecntt::uniform_stages(log_n);
    return panda_success;
}

panda_error panda_points_to_affine(unsigned curve, const void *d_in, panda_msm_result_coordinate_type in_type, void *d_out, uint64_t n, panda_stream stream)
{
    if (curve > 2 || !d_in || !d_out || n == 0 || n > MAX_POINTS || (in_type != JACOBIAN && in_type != PROJECTIVE)) return panda_error_invalid_value;
    const size_t out_bytes = (size_t)n * affine_bytes(curve), in_bytes = out_bytes / 2 * 3;
    if (ranges_overlap(d_in, in_bytes, d_out, out_bytes)) return panda_error_invalid_value;
    if (panda::extent_too_short(d_in, in_bytes) || panda::extent_too_short(d_out, out_bytes)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_curve(curve, [&](auto fq, auto) { return static_cast<panda_error>(run_to_affine<decltype(fq)>(s, d_in, d_out, n, in_type == PROJECTIVE)); });
}

panda_error panda_points_to_affine_plan(uint64_t n, unsigned *chunk, unsigned *launches)
{
    if (n == 0 || n > MAX_POINTS) return panda_error_invalid_value;
    if (chunk) *chunk = CHUNK;
    if (launches) *launches = 1;
    return panda_success;
}

} // extern "C"
