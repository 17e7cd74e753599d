// poly_sum.hip -- exclusive running sums over the scalar fields, the accumulator of a logUp lookup argument (panda_poly_running_sum,
// panda_poly_running_sum_plan): out[p][0] = 0, out[p][i] = sum_{j < i} in[p][j], totals[p] = the whole sum.
//
// Reduce-then-scan over tiles of TILE = THREADS * E elements, the launch structure of poly_product.hip, on the workgroup scan of
// poly_scan.h with the operation OpAdd below: k_sum_totals (tile sums), k_sum_seeds (one workgroup per vector: exclusive prefix sums of
// the tile sums in place, the grand sum to the values), k_sum_apply (in-tile scan from the seed; a thread stores only the indices it
// loaded, so d_out may be d_in).  Totals only: the first two launches, no seeds stored.  A sum of wire residues is the wire residue of
// the sum: no constants.  Bounds: poly_sum.h.
#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"
#include "poly_sum.h"

using namespace panda29;
using namespace panda_poly;

namespace {

constexpr int E = 4;  // elements per thread (poly_sum.h: RUN_MAX)
constexpr int CE = 4; // tile sums per thread of the seed kernel
constexpr unsigned TILE = THREADS * E, CHUNK = THREADS * CE;
static_assert(E <= RUN_MAX && CE <= RUN_MAX, "a thread's run must stay within sum_run's bound");

// poly_scan.h's operation: the field's sum, canonical in and out (poly_sum.h), so everything that crosses a lane, LDS or memory is canonical
struct OpAdd {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_zero(r); }
    template <class Fr>
    static __device__ __forceinline__ void combine(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b) { add_canon(r, a, b); }
    template <class Fr, int RUN>
    static __device__ __forceinline__ void run(Fe<Fr> &g, const Fe<Fr> (&x)[RUN]) { sum_run<Fr, RUN>(g, x); }
};

// launch 1: tt[blk] = the sum of tile a = blk % tiles of vector p = blk / tiles
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sum_totals(const u32 *__restrict__ in, u32 *__restrict__ tt, u64 n, unsigned tiles)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    Fe<Fr> x[E], g, zero, mine, total;
    load_run<OpAdd, Fr, E>(x, in + (u64)p * n * 8, (u64)a * TILE + threadIdx.x * E, n);
    OpAdd::run(g, x);
    fe_zero(zero);
    block_scan<OpAdd, Fr, false>(mine, total, g, zero, s_w);
    if (threadIdx.x == 0) store_elem(tt + (u64)blk * 8, total);
}

// launch 2: one workgroup per vector.  SEEDS: the tile sums are replaced by their exclusive prefix sums, every thread storing the indices
// it loaded.  values[p] = the vector's sum.
template <class Fr, bool SEEDS>
__global__ void __launch_bounds__(THREADS) k_sum_seeds(u32 *tt, u32 *__restrict__ values, unsigned tiles)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned p = blockIdx.x;
    u32 *T = tt + (u64)p * tiles * 8;
    Fe<Fr> sum;
    fe_zero(sum);
    walk_totals<OpAdd, Fr, CE, SEEDS>(sum, T, T, tiles, s_w);
    if (threadIdx.x == 0) store_elem(values + (u64)p * 8, sum);
}

// launch 3: the outputs of tile a of vector p from the seed seeds[blk]
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sum_apply(const u32 *in, u32 *out, const u32 *__restrict__ seeds, u64 n, unsigned tiles)
{
    __shared__ u32 s_w[WAVES * NL];
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const u64 j0 = (u64)a * TILE + threadIdx.x * E;
    Fe<Fr> x[E], g, seed, pre, total;
    load_run<OpAdd, Fr, E>(x, in + (u64)p * n * 8, j0, n);
    OpAdd::run(g, x);
    load_elem(seed, seeds + (u64)blk * 8);
    block_scan<OpAdd, Fr, false>(pre, total, g, seed, s_w);
    u32 *dst = out + ((u64)p * n + j0) * 8;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (j0 + e < n) store_elem(dst + e * 8, pre);
        if (e < E - 1) add_canon(pre, pre, x[e]);
    }
}

template <class Fr>
hipError_t call_running_sum(hipStream_t stream, const void *d_in, void *d_out, u64 n, unsigned batch, void *totals)
{
    const size_t bytes = (size_t)batch * n * 32;
    if (panda::extent_too_short(d_in, bytes) || (d_out && panda::extent_too_short(d_out, bytes))) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    const unsigned tiles = tiles_of(n, TILE);
    const size_t vbytes = (size_t)batch * 32;
    void *block[2]; // a sum per tile, a value per vector
    PANDA_TRY(take_scratch({(size_t)batch * tiles * 32, vbytes}, block));
    u32 *d_tt = (u32 *)block[0], *d_values = (u32 *)block[1];
    hipLaunchKernelGGL((k_sum_totals<Fr>), dim3(batch * tiles), dim3(THREADS), 0, stream, (const u32 *)d_in, d_tt, n, tiles);
    PANDA_TRY(hipGetLastError());
    if (d_out) {
        hipLaunchKernelGGL((k_sum_seeds<Fr, true>), dim3(batch), dim3(THREADS), 0, stream, d_tt, d_values, tiles);
        PANDA_TRY(hipGetLastError());
        hipLaunchKernelGGL((k_sum_apply<Fr>), dim3(batch * tiles), dim3(THREADS), 0, stream, (const u32 *)d_in, (u32 *)d_out, (const u32 *)d_tt, n, tiles);
    } else
        hipLaunchKernelGGL((k_sum_seeds<Fr, false>), dim3(batch), dim3(THREADS), 0, stream, d_tt, d_values, tiles);
    PANDA_TRY(hipGetLastError());
    if (totals) PANDA_TRY(hipMemcpyAsync(totals, d_values, vbytes, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The exclusive running sum: see include/panda_interface.h.  Every check but the extents comes before any runtime call.
panda_error panda_poly_running_sum(unsigned field, const void *d_in, void *d_out, uint64_t n, unsigned batch, void *totals, panda_stream stream)
{
    if (field > 2 || shape_invalid(n, batch) || !d_in || (!d_out && !totals)) return panda_error_invalid_value;
    if (d_out && bad_pair(d_in, d_out, (size_t)batch * n * 32)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(call_running_sum<decltype(fr)>(s, d_in, d_out, n, batch, totals)); });
}

panda_error panda_poly_running_sum_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *carry_chunk, unsigned *launches_scan, unsigned *launches_total)
{
    if (shape_invalid(n, batch)) return panda_error_invalid_value;
    if (tile) *tile = TILE;
    if (carry_chunk) *carry_chunk = CHUNK;
    if (launches_scan) *launches_scan = 3;
    if (launches_total) *launches_total = 2;
    return panda_success;
}

} // extern "C"
