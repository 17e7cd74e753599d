// poly.hip -- polynomial evaluation and division by X - z over the scalar fields, for KZG openings (panda_poly_evaluate,
// panda_poly_divide_linear, panda_poly_plan).
//
// With the suffix Horner values S_j = sum_{i >= j} c_i z^(i-j) (S_j = c_j + z S_(j+1), S_n = 0): f(z) = S_0 and the quotient of f by
// X - z is q_j = S_(j+1).  Evaluation is a reduction, division a suffix scan of a linear recurrence with the constant multiplier z.
// Both run as reduce-then-scan over tiles of TILE = THREADS * E coefficients; no kernel waits for another workgroup:
//   launch 1  k_poly_totals   workgroup (p, a) reduces tile a of polynomial p to L_a = sum_{i in tile} c_i z^(i - a TILE): every thread
//                             Horner over its E consecutive elements, lanes combined with z^E, z^2E, ... by cross-lane moves, the four
//                             waves through LDS with z^(64 E)
//   launch 2  k_poly_carries  one workgroup per polynomial runs the same recurrence over the totals with the multiplier y = z^TILE,
//                             CHUNK = THREADS * CE totals per step from the last chunk down: C_a = L_(a+1) + y C_(a+1), the S at tile a's
//                             right edge, replaces L_a in place; S_0 = L_0 + y C_0 is the remainder / the value
//   launch 3  k_poly_apply    workgroup (p, a) loads its tile, rescans the per-thread aggregates seeded with C_a, and every thread runs
//                             q_j = c_(j+1) + z q_(j+1) down from its own right edge.  A thread stores only what it has loaded itself and
//                             what crosses workgroups comes from launches 1 and 2, so d_quot == d_coeffs is safe.
// Coefficients beyond n read as zero, so ragged tails (n no multiple of E, 64 E, TILE; a short last chunk) take the same code.  The
// padded load is poly_scan.h's; the scan itself is this file's own: a recurrence with per-step multipliers handed over by value
// (Ladder), not a scan of elements under one operation.
//
// Arithmetic: the multipliers of one call (z, z^(E 2^s), y, y^(CE 2^s)) are wave-uniform; they are derived on the host and handed
// to the kernels by value as (w, floor(w R / p)) pairs for fe_mul_shoup<F, UNIFORM>.  The constant is the plain integer z, so
// wire-form residues map to wire-form residues without conversion.  Bounds: a product is tight and below (1 + x / R + 2^-23) p; a
// Horner step adds a tight coefficient to it without carries (limbs < 2^30, fine as the next product's operand); the scan steps
// normalise (fe_add).  No value exceeds (2^256 / p + 16) p < R / 4, and every stored element goes through fe_reduce_small.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"

using namespace panda29;
using namespace panda_poly;

namespace {

constexpr int E = 8;                    // coefficients per thread
constexpr int CE = 4;                   // tile totals per thread of the carry kernel
constexpr unsigned TILE = THREADS * E, CHUNK = THREADS * CE;
constexpr int LADDER = 7;               // m^(RUN 2^s), s = 0 .. 6: six cross-lane steps and the wave's width

// what a run reads beyond the end of its vector (poly_scan.h: load_run)
struct PadZero {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_zero(r); }
};

// the multipliers of one launch: the step m of the recurrence and m^(RUN 2^s), RUN the elements a thread covers
template <class Fr>
struct Ladder {
    FeTw<Fr> m;
    FeTw<Fr> pw[LADDER];
};

// v += w t, normalised
template <class Fr>
__device__ __forceinline__ void axpy(Fe<Fr> &v, const Fe<Fr> &t, const FeTw<Fr> &w)
{
    Fe<Fr> pr;
    fe_mul_shoup<Fr, true>(pr, t, w.w, w.q);
    fe_add(v, v, pr);
}

// the value `d` lanes up, zero past the end of the wave (the select per limb: built on poly_scan.h's lane_shift k_poly_totals lost a wave)
template <class Fr>
__device__ __forceinline__ void lanes_up(Fe<Fr> &r, const Fe<Fr> &v, unsigned d, unsigned lane)
{
    const bool in = lane + d < 64;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const u32 t = __shfl_down(v.l[i], d, 64);
        r.l[i] = in ? t : 0u;
    }
}

// sum_e x[e] m^e: Horner from the run's right end; RUN - 1 products, limbs < 2^30
template <class Fr, int RUN>
__device__ __forceinline__ void run_horner(Fe<Fr> &g, const Fe<Fr> (&x)[RUN], const FeTw<Fr> &m)
{
    g = x[RUN - 1];
#pragma unroll
    for (int e = RUN - 2; e >= 0; e--) {
        Fe<Fr> pr;
        fe_mul_shoup<Fr, true>(pr, g, m.w, m.q);
        fe_add_nr(g, x[e], pr);
    }
}

// lane 0 <- sum_l v_l m^(RUN l) over the wave
template <class Fr>
__device__ __forceinline__ void wave_reduce(Fe<Fr> &v, const Ladder<Fr> &L, unsigned lane)
{
#pragma unroll
    for (int s = 0; s < 6; s++) {
        Fe<Fr> t;
        lanes_up(t, v, 1u << s, lane);
        axpy(v, t, L.pw[s]);
    }
}

// lane l <- sum_{u >= l} v_u m^(RUN (u - l)): the inclusive suffix scan of the wave
template <class Fr>
__device__ __forceinline__ void wave_suffix_scan(Fe<Fr> &v, const Ladder<Fr> &L, unsigned lane)
{
    wave_reduce(v, L, lane); // the same steps; lanes_up's zeros make every lane's partial sum exact
}

// The workgroup's 256 runs x[t][0 .. RUN) stand for THREADS * RUN consecutive elements of the recurrence s_i = x_i + m s_(i+1); `edge`
// (the same in every thread) is s just right of the last run.  On return `right` is s just right of the calling thread's run and
// `total` (the same in every thread) s at the first run's first element.  One barrier; the caller must put another one before s_w is
// reused.  Products per thread: RUN - 1 (run) + 6 (wave totals) + WAVES (across the waves) + 1 (seed) + 6 (scan).
template <class Fr, int RUN>
__device__ __forceinline__ void block_suffix_scan(Fe<Fr> &right, Fe<Fr> &total, const Fe<Fr> (&x)[RUN], const Fe<Fr> &edge, const Ladder<Fr> &L, u32 *s_w)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Fe<Fr> g, r;
    run_horner<Fr, RUN>(g, x, L.m);
    r = g;
    wave_reduce(r, L, lane);
    if (lane == 0) lds_put(s_w + wave * NL, r.l);
    __syncthreads();
    // s at each wave's right edge, from the last wave down; what is left after wave 0 is the total
    Fe<Fr> y = edge, mine = edge;
#pragma unroll
    for (int w = WAVES - 1; w >= 0; w--) {
        Fe<Fr> t;
        lds_get(t, s_w + w * NL);
        axpy(t, y, L.pw[6]);
        y = t;
        if ((int)wave == w - 1) mine = y;
    }
    total = y;
    // the wave's scan, its last lane seeded with the wave's edge
    Fe<Fr> seed;
    fe_mul_shoup<Fr, true>(seed, mine, L.pw[0].w, L.pw[0].q);
    if (lane == 63) fe_add(g, g, seed);
    wave_suffix_scan(g, L, lane);
    lanes_up(right, g, 1, lane);
    if (lane == 63) right = mine;
}

// launch 1: totals[blk] = L_a of tile a = blk % tiles of polynomial p = blk / tiles
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_poly_totals(const u32 *__restrict__ c, u32 *__restrict__ totals, u64 n, unsigned tiles, Ladder<Fr> L)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 j0 = (u64)a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], g;
    load_run<PadZero, Fr, E>(x, c + (u64)p * n * 8, j0, n);
    run_horner<Fr, E>(g, x, L.m);
    wave_reduce(g, L, lane);
    if (lane == 0) lds_put(s_w + wave * NL, g.l);
    __syncthreads();
    if (threadIdx.x == 0) {
        Fe<Fr> y;
        lds_get(y, s_w + (WAVES - 1) * NL);
#pragma unroll
        for (int w = WAVES - 2; w >= 0; w--) {
            Fe<Fr> t;
            lds_get(t, s_w + w * NL);
            axpy(t, y, L.pw[6]);
            y = t;
        }
        store_elem(totals + (u64)blk * 8, y);
    }
}

// launch 2: one workgroup per polynomial; L is the ladder of y = z^TILE with runs of CE.  CARRIES: the totals are replaced by the
// carries C_a (division); without, only the value is produced (evaluation).  value (p) goes to values[p * vstride + voff].
template <class Fr, bool CARRIES>
__global__ void __launch_bounds__(THREADS) k_poly_carries(u32 *__restrict__ totals, u32 *__restrict__ values, unsigned tiles, unsigned vstride, unsigned voff, Ladder<Fr> L)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned p = blockIdx.x;
    u32 *T = totals + (u64)p * tiles * 8;
    Fe<Fr> carry;
    fe_zero(carry);
    for (unsigned k = (tiles + CHUNK - 1) / CHUNK; k-- > 0;) {
        const unsigned a0 = k * CHUNK + threadIdx.x * CE;
        Fe<Fr> x[CE], s, total;
        load_run<PadZero, Fr, CE>(x, T, a0, tiles);
        block_suffix_scan<Fr, CE>(s, total, x, carry, L, s_w);
        carry = total;
        fe_reduce_small_2p(carry); // keeps the value bounded over any number of chunks
        if constexpr (CARRIES) {
#pragma unroll
            for (int e = CE - 1; e >= 0; e--) {
                if (a0 + e < tiles) store_elem(T + (u64)(a0 + e) * 8, s);
                if (e > 0) {
                    Fe<Fr> pr;
                    fe_mul_shoup<Fr, true>(pr, s, L.m.w, L.m.q);
                    fe_add_nr(s, x[e], pr);
                }
            }
        }
        __syncthreads(); // s_w is written again in the next chunk
    }
    if (threadIdx.x == 0) store_elem(values + ((u64)p * vstride + voff) * 8, carry);
}

// launch 3: q_j = S_(j+1) for tile a of polynomial p, seeded with carries[blk] = C_a
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_poly_apply(const u32 *c, u32 *q, const u32 *__restrict__ carries, u64 n, unsigned tiles, Ladder<Fr> L)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const u64 j0 = (u64)a * TILE + threadIdx.x * E;
    u32 *dst = q + ((u64)p * n + j0) * 8;
    Fe<Fr> x[E], edge, s, total;
    load_run<PadZero, Fr, E>(x, c + (u64)p * n * 8, j0, n);
    load_elem(edge, carries + (u64)blk * 8);
    block_suffix_scan<Fr, E>(s, total, x, edge, L, s_w); // the barrier inside is behind every load of the workgroup
#pragma unroll
    for (int e = E - 1; e >= 0; e--) {
        if (j0 + e < n) store_elem(dst + e * 8, s);
        if (e > 0) {
            Fe<Fr> pr;
            fe_mul_shoup<Fr, true>(pr, s, L.m.w, L.m.q);
            fe_add_nr(s, x[e], pr);
        }
    }
}

// ------------------------------------------------------------------------------- host side

// m (internal form) and m^(run 2^s) as precomputed-quotient pairs; *next = m^(run 2^(LADDER + 1)) = m^(run THREADS), the step one level up
template <class Fr>
void make_ladder(Ladder<Fr> &L, const Fe<Fr> &m, unsigned run, Fe<Fr> *next)
{
    fe_shoup_prepare(L.m, m);
    Fe<Fr> pw;
    fe_pow_u64(pw, m, run);
    for (int s = 0; s < LADDER; s++) {
        fe_shoup_prepare(L.pw[s], pw);
        fe_sqr(pw, pw);
    }
    fe_sqr(pw, pw); // run * 2^8
    static_assert(THREADS == 256, "the ladder's last rung squared twice is the workgroup's width");
    if (next) *next = pw;
}

bool point_valid(unsigned field, const void *pt)
{
    u32 w[8];
    memcpy(w, pt, sizeof(w));
    return with_field(field, [&](auto fr) { return wire_below_modulus<decltype(fr)>(w); });
}

// tile totals and n_values values per polynomial
hipError_t take_totals(u64 n, unsigned batch, unsigned n_values, u32 **d_totals, u32 **d_values)
{
    void *block[2];
    PANDA_TRY(take_scratch({(size_t)batch * tiles_of(n, TILE) * 32, (size_t)batch * n_values * 32}, block));
    *d_totals = (u32 *)block[0], *d_values = (u32 *)block[1];
    return hipSuccess;
}

// launches 1 and 2 for one point: the values land at d_values[p * vstride + voff]; with `carries` the totals become the carries
template <class Fr>
hipError_t sweep(hipStream_t stream, const u32 *d_coeffs, u64 n, unsigned batch, const u32 *point_wire, u32 *d_totals, u32 *d_values, unsigned vstride,
                 unsigned voff, bool carries, Ladder<Fr> &lz)
{
    Fe<Fr> z, y;
    fe_from_wire(z, point_wire);
    make_ladder<Fr>(lz, z, E, &y); // y = z^TILE
    Ladder<Fr> ly;
    make_ladder<Fr>(ly, y, CE, nullptr);
    const unsigned tiles = tiles_of(n, TILE);
    hipLaunchKernelGGL(k_poly_totals<Fr>, dim3(batch * tiles), dim3(THREADS), 0, stream, d_coeffs, d_totals, n, tiles, lz);
    PANDA_TRY(hipGetLastError());
    if (carries)
        hipLaunchKernelGGL((k_poly_carries<Fr, true>), dim3(batch), dim3(THREADS), 0, stream, d_totals, d_values, tiles, vstride, voff, ly);
    else
        hipLaunchKernelGGL((k_poly_carries<Fr, false>), dim3(batch), dim3(THREADS), 0, stream, d_totals, d_values, tiles, vstride, voff, ly);
    return hipGetLastError();
}

template <class Fr>
hipError_t run_evaluate(hipStream_t stream, const void *d_coeffs, u64 n, unsigned batch, const u32 *points, unsigned n_points, void *values)
{
    if (panda::extent_too_short(d_coeffs, (size_t)batch * n * 32)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    u32 *d_totals = nullptr, *d_values = nullptr;
    PANDA_TRY(take_totals(n, batch, n_points, &d_totals, &d_values));
    for (unsigned k = 0; k < n_points; k++) { // one sweep over the coefficients per point
        Ladder<Fr> lz;
        PANDA_TRY(sweep<Fr>(stream, (const u32 *)d_coeffs, n, batch, points + 8 * k, d_totals, d_values, n_points, k, false, lz));
    }
    PANDA_TRY(hipMemcpyAsync(values, d_values, (size_t)batch * n_points * 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t run_divide(hipStream_t stream, const void *d_coeffs, void *d_quot, u64 n, unsigned batch, const u32 *point, void *remainders)
{
    const size_t bytes = (size_t)batch * n * 32;
    if (panda::extent_too_short(d_coeffs, bytes) || panda::extent_too_short(d_quot, bytes)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    u32 *d_totals = nullptr, *d_values = nullptr;
    PANDA_TRY(take_totals(n, batch, 1, &d_totals, &d_values));
    Ladder<Fr> lz;
    PANDA_TRY(sweep<Fr>(stream, (const u32 *)d_coeffs, n, batch, point, d_totals, d_values, 1, 0, true, lz));
    const unsigned tiles = tiles_of(n, TILE);
    hipLaunchKernelGGL(k_poly_apply<Fr>, dim3(batch * tiles), dim3(THREADS), 0, stream, (const u32 *)d_coeffs, (u32 *)d_quot, d_totals, n, tiles, lz);
    PANDA_TRY(hipGetLastError());
    if (remainders) PANDA_TRY(hipMemcpyAsync(remainders, d_values, (size_t)batch * 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// Evaluation at up to PANDA_POLY_MAX_POINTS points: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_poly_evaluate(unsigned field, const void *d_coeffs, uint64_t n, unsigned batch, const void *points, unsigned n_points, void *values,
                                panda_stream stream)
{
    if (field > 2 || shape_invalid(n, batch) || n_points == 0 || n_points > PANDA_POLY_MAX_POINTS || !d_coeffs || !points || !values) return panda_error_invalid_value;
    for (unsigned k = 0; k < n_points; k++)
        if (!point_valid(field, (const char *)points + 32 * k)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_evaluate<decltype(fr)>(s, d_coeffs, n, batch, (const u32 *)points, n_points, values)); });
}

// Division by X - z: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_poly_divide_linear(unsigned field, const void *d_coeffs, void *d_quot, uint64_t n, unsigned batch, const void *point, void *remainders,
                                     panda_stream stream)
{
    if (field > 2 || shape_invalid(n, batch) || !d_coeffs || !d_quot || !point || !point_valid(field, point)) return panda_error_invalid_value;
    if (bad_pair(d_coeffs, d_quot, (size_t)batch * n * 32)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_divide<decltype(fr)>(s, d_coeffs, d_quot, n, batch, (const u32 *)point, remainders)); });
}

panda_error panda_poly_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *carry_chunk, unsigned *launches_evaluate, unsigned *launches_divide)
{
    if (shape_invalid(n, batch)) return panda_error_invalid_value;
    if (tile) *tile = TILE;
    if (carry_chunk) *carry_chunk = CHUNK;
    if (launches_evaluate) *launches_evaluate = 2;
    if (launches_divide) *launches_divide = 3;
    return panda_success;
}

} // extern "C"
