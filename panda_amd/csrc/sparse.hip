// sparse.hip -- sparse matrix-vector products over the scalar fields, the first step of every R1CS prover (panda_sparse_matvec,
// panda_sparse_check, panda_sparse_plan):
//
//   out[p][r] = sum_{k in row r} values[k] z[p][col[k]]        CSR: row r holds the nonzeros row_ptr[r] .. row_ptr[r + 1] - 1
//
// The work is split by nonzeros, not by rows (sparse.h: the routines, the arithmetic, the bounds, why no access leaves its buffer).  `out`
// and the heads are zeroed by memsets -- the wire zero is all-zero bytes, so empty rows and nnz == 0 cost nothing more -- then two launches:
//   k_sparse_tile   workgroup (p, t) covers the nonzeros [t TILE, (t + 1) TILE) for vector p, E consecutive ones per thread.  Threads 0
//                   and 64 find the tile's first and last row, every thread the row of its first nonzero between them; products two to a
//                   reduction, sums inside row segments, a segmented scan over (flag, value) across lanes (shuffles) and waves (LDS).  A
//                   row's last thread of the tile stores out[p][row] if the row began in the tile, head[p][t] if it began earlier.
//   k_sparse_fixup  wave (p, t), t >= 1: if the row of nonzero t TILE began in tile t - 1, the wave adds head[p][t ..] of every tile the
//                   row reaches into out[p][row], FIXUP_CHUNK heads per step.  One wave per row, so no row is touched twice.
// No kernel waits for another workgroup, there are no atomics on elements, and field addition is exact: the bytes are the same on every
// run.  panda_sparse_check is one launch that dereferences nothing through an index and keeps the smallest (class, index) by atomicMin on
// a packed u64, as the lookup's first_missing does.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"
#include "poly_sum.h"
#include "sparse.h"

using namespace panda29;
using namespace panda_poly; // THREADS, WAVES, load_elem, lane_shift, lds_put / lds_get, ranges_overlap, with_field, take_scratch
using panda_sparse::FIXUP_CHUNK;
using panda_sparse::Segments;
using panda_sparse::TILE;

static_assert(THREADS == panda_sparse::TILE_THREADS, "a tile is one workgroup");
static_assert(FIXUP_CHUNK == 64, "a fix-up step is one head per lane");
static_assert(panda_sparse::MAX_LOG == MAX_LOG_ELEMS, "the caps are those of every other call");

namespace {

constexpr int SE = NL + 1; // LDS words of a wave's scan element: the value's limbs and the flag

// a canonical value -> 32 bytes
template <class Fr>
__device__ __forceinline__ void store_canon(u32 *__restrict__ dst, const Fe<Fr> &v)
{
    u32 w8[8];
    fe_pack(w8, v);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    d4[0] = make_uint4(w8[0], w8[1], w8[2], w8[3]);
    d4[1] = make_uint4(w8[4], w8[5], w8[6], w8[7]);
}

// the loads of sparse.h's routines; every index has been bounded by the routine that calls them
template <class Fr>
struct DeviceAccess {
    const u32 *__restrict__ rp, *__restrict__ cl, *__restrict__ vl, *__restrict__ zv;
    __device__ __forceinline__ u32 row_ptr(u32 i) const { return rp[i]; }
    __device__ __forceinline__ u32 col(u32 k) const { return cl[k]; }
    __device__ __forceinline__ void value(Fe<Fr> &v, u32 k) const { load_elem(v, vl + (u64)k * 8); }
    __device__ __forceinline__ void z(Fe<Fr> &v, u32 c) const { load_elem(v, zv + (u64)c * 8); }
};

// launch 1: blk = p * tiles + t
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sparse_tile(const u32 *__restrict__ row_ptr, const u32 *__restrict__ col, const u32 *__restrict__ values,
                                                         const u32 *__restrict__ z, u32 *__restrict__ out, u32 *__restrict__ head, u32 n_rows, u32 n_cols,
                                                         u32 nnz, u32 tiles, const Fe<Fr> cinv)
{
    __shared__ u32 s_rows[2];
    __shared__ u32 s_w[WAVES * SE];
    const u32 blk = blockIdx.x, p = blk / tiles, t = blk - p * tiles;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 first = t * TILE, last = (nnz - first < TILE ? nnz : first + TILE) - 1; // t < tiles: first < nnz
    const DeviceAccess<Fr> access = {row_ptr, col, values, z + (u64)p * n_cols * 8};
    auto rp = [&](u32 i) { return row_ptr[i]; };
    if (threadIdx.x == 0) s_rows[0] = panda_sparse::row_of(rp, first, 0u, n_rows - 1);
    if (threadIdx.x == 64) s_rows[1] = panda_sparse::row_of(rp, last, 0u, n_rows - 1);
    __syncthreads();
    const u32 r_lo = s_rows[0], r_hi = s_rows[1] < r_lo ? r_lo : s_rows[1];

    const u32 k0 = first + threadIdx.x * panda_sparse::E;
    const u32 n_live = k0 >= nnz ? 0u : (nnz - k0 < (u32)panda_sparse::E ? nnz - k0 : (u32)panda_sparse::E);
    const bool force = n_live > 0 && (threadIdx.x == THREADS - 1 || k0 + panda_sparse::E >= nnz);
    Segments<Fr> S;
    panda_sparse::thread_segments(S, access, k0, n_live, force, r_lo, r_hi, n_cols);

    // the segmented scan of (flag, open): inclusive in the wave, the waves' last elements through LDS
    u32 f = S.flag;
    Fe<Fr> v = S.open;
#pragma unroll
    for (int s = 0; s < 6; s++) {
        const unsigned d = 1u << s;
        Fe<Fr> o, cv;
        u32 cf;
        lane_shift<Fr, false>(o, v, d);
        const u32 of = __shfl_up(f, d, 64);
        panda_sparse::seg_combine(cf, cv, of, o, f, v);
        const bool in = lane >= d;
        fe_select(v, in, cv, v);
        f = in ? cf : f;
    }
    if (lane == 63) {
        lds_put(s_w + wave * SE, v.l);
        s_w[wave * SE + NL] = f;
    }
    __syncthreads();
    u32 pf = 0;
    Fe<Fr> pv;
    fe_zero(pv);
#pragma unroll
    for (int w = 0; w < WAVES - 1; w++)
        if ((int)wave > w) {
            Fe<Fr> tv;
            lds_get(tv, s_w + w * SE);
            panda_sparse::seg_combine(pf, pv, pf, pv, s_w[w * SE + NL], tv);
        }
    Fe<Fr> ex, zero;
    fe_zero(zero);
    lane_shift<Fr, false>(ex, v, 1);
    u32 exf = __shfl_up(f, 1, 64);
    fe_select(ex, lane == 0, zero, ex);
    exf = lane == 0 ? 0u : exf;
    panda_sparse::seg_combine(pf, pv, pf, pv, exf, ex);

    u32 *out_p = out + (u64)p * n_rows * 8, *head_t = head + (u64)blk * 8;
    panda_sparse::emit(S, pf, pv, cinv, [&](bool in_tile, u32 row, const Fe<Fr> &total) { store_canon(in_tile ? out_p + (u64)row * 8 : head_t, total); });
}

// launch 2: blk = p * groups + g; wave w of it is tile t = g * WAVES + w + 1
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sparse_fixup(const u32 *__restrict__ row_ptr, u32 *out, const u32 *__restrict__ head, u32 n_rows, u32 tiles,
                                                          u32 groups)
{
    const u32 blk = blockIdx.x, p = blk / groups, g = blk - p * groups;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 t = g * WAVES + wave + 1;
    if (t >= tiles) return; // the whole wave; the kernel has no barrier
    auto rp = [&](u32 i) { return row_ptr[i]; };
    u32 r, t_last;
    if (!panda_sparse::fixup_span(r, t_last, rp, t, n_rows, tiles)) return; // the same in every lane
    const u32 *head_p = head + (u64)p * tiles * 8;
    Fe<Fr> sum;
    panda_sparse::fixup_lane_sum(sum, [&](Fe<Fr> &h, u32 j) { load_elem(h, head_p + (u64)j * 8); }, t, t_last, lane);
#pragma unroll
    for (int s = 5; s >= 0; s--) { // lane l < d adds lane l + d: lane 0 ends with the wave's sum
        Fe<Fr> o;
        lane_shift<Fr, true>(o, sum, 1u << s);
        add_canon(sum, sum, o);
    }
    if (lane == 0) {
        u32 *dst = out + ((u64)p * n_rows + r) * 8;
        Fe<Fr> have;
        load_elem(have, dst);
        add_canon(have, have, sum);
        store_canon(dst, have);
    }
}

// the 256-bit value of a wire element is below the modulus (poly_elem.h's wire_below_modulus, for the device)
template <class Fr>
__device__ __forceinline__ bool words_below_modulus(const u32 (&w)[8])
{
    bool below = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const u32 pw = Fr::PW[i];
        if (!decided && w[i] != pw) {
            below = w[i] < pw;
            decided = true;
        }
    }
    return below;
}

// the check: thread i looks at row_ptr[i], row_ptr[i + 1], col[i] and values[i]; nothing is addressed through what it reads
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sparse_check(const u32 *__restrict__ row_ptr, const u32 *__restrict__ col, const u32 *__restrict__ values, u32 n_rows,
                                                          u32 n_cols, u32 nnz, unsigned long long *result)
{
    const u32 i = blockIdx.x * THREADS + threadIdx.x;
    u64 key = ~(u64)0;
    auto found = [&](u32 cls, u32 where) {
        const u64 k = ((u64)cls << 32) | where;
        key = k < key ? k : key;
    };
    if (i == 0 && row_ptr[0] != 0) found(1, 0);
    if (i < n_rows && row_ptr[i] > row_ptr[i + 1]) found(2, i);
    if (i == n_rows && row_ptr[n_rows] != nnz) found(3, 0);
    if (i < nnz) {
        if (col[i] >= n_cols) found(4, i);
        const uint4 *s4 = reinterpret_cast<const uint4 *>(values + (u64)i * 8);
        const uint4 lo = s4[0], hi = s4[1];
        const u32 w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        if (!words_below_modulus<Fr>(w)) found(5, i);
    }
    if (key != ~(u64)0 && key < *(volatile unsigned long long *)result) atomicMin(result, (unsigned long long)key);
}

// ------------------------------------------------------------------------------------------------- the checks that need no runtime call

bool matrix_valid(unsigned field, const panda_csr_matrix *m, u64 batch)
{
    if (field > 2 || !m || !m->d_row_ptr) return false;
    if (!panda_sparse::shape_valid(m->n_rows, m->n_cols, m->nnz, batch)) return false;
    return m->nnz == 0 || (m->d_col && m->d_values);
}

bool matrix_too_short(const panda_csr_matrix &m)
{
    if (panda::extent_too_short(m.d_row_ptr, (size_t)(m.n_rows + 1) * 4)) return true;
    return m.nnz > 0 && (panda::extent_too_short(m.d_col, (size_t)m.nnz * 4) || panda::extent_too_short(m.d_values, (size_t)m.nnz * 32));
}

bool matvec_arguments_valid(unsigned field, const panda_csr_matrix *m, const void *d_z, void *d_out, unsigned batch)
{
    if (!matrix_valid(field, m, batch) || !d_z || !d_out) return false;
    const size_t out_bytes = (size_t)batch * m->n_rows * 32, z_bytes = (size_t)batch * m->n_cols * 32;
    if (ranges_overlap(d_out, out_bytes, d_z, z_bytes) || ranges_overlap(d_out, out_bytes, m->d_row_ptr, (size_t)(m->n_rows + 1) * 4)) return false;
    if (m->nnz > 0 && (ranges_overlap(d_out, out_bytes, m->d_col, (size_t)m->nnz * 4) || ranges_overlap(d_out, out_bytes, m->d_values, (size_t)m->nnz * 32)))
        return false;
    return !(matrix_too_short(*m) || panda::extent_too_short(d_z, z_bytes) || panda::extent_too_short(d_out, out_bytes));
}

size_t matvec_scratch_bytes(u64 nnz, unsigned batch) { return panda::align256((size_t)batch * panda_sparse::tiles_of_nnz(nnz) * 32) + 256; }
unsigned matvec_launches(u64 nnz) { return nnz == 0 ? 0u : nnz <= TILE ? 1u : 2u; }

// ------------------------------------------------------------------------------------------------- the calls

template <class Fr>
hipError_t run_matvec(hipStream_t stream, const panda_csr_matrix &m, const void *d_z, void *d_out, unsigned batch)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    const u32 n_rows = (u32)m.n_rows, n_cols = (u32)m.n_cols, nnz = (u32)m.nnz, tiles = panda_sparse::tiles_of_nnz(m.nnz);
    PANDA_TRY(hipMemsetAsync(d_out, 0, (size_t)batch * n_rows * 32, stream));
    if (nnz > 0) {
        const u64 blocks = (u64)batch * tiles;
        if (blocks > 0x7FFFFFFFu) return hipErrorOutOfMemory; // the heads alone would be 64 GB
        void *block[1]; // a head per vector and tile
        PANDA_TRY(take_scratch({(size_t)blocks * 32}, block));
        u32 *d_head = (u32 *)block[0];
        PANDA_TRY(hipMemsetAsync(d_head, 0, (size_t)blocks * 32, stream));
        hipLaunchKernelGGL((k_sparse_tile<Fr>), dim3((unsigned)blocks), dim3(THREADS), 0, stream, (const u32 *)m.d_row_ptr, (const u32 *)m.d_col,
                           (const u32 *)m.d_values, (const u32 *)d_z, (u32 *)d_out, d_head, n_rows, n_cols, nnz, tiles, panda_sop::wire_factor_inverse<Fr>());
        PANDA_TRY(hipGetLastError());
        if (tiles > 1) {
            const u32 groups = (tiles - 1 + WAVES - 1) / WAVES;
            hipLaunchKernelGGL((k_sparse_fixup<Fr>), dim3((unsigned)((u64)batch * groups)), dim3(THREADS), 0, stream, (const u32 *)m.d_row_ptr, (u32 *)d_out,
                               (const u32 *)d_head, n_rows, tiles, groups);
            PANDA_TRY(hipGetLastError());
        }
    }
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t run_check(hipStream_t stream, const panda_csr_matrix &m, unsigned *defect, uint64_t *where)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    void *block[1]; // the smallest (class << 32) | index
    PANDA_TRY(take_scratch({8}, block));
    PANDA_TRY(hipMemsetAsync(block[0], 0xFF, 8, stream));
    const u64 span = m.n_rows + 1 > m.nnz ? m.n_rows + 1 : m.nnz;
    hipLaunchKernelGGL((k_sparse_check<Fr>), dim3((unsigned)((span + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, (const u32 *)m.d_row_ptr,
                       (const u32 *)m.d_col, (const u32 *)m.d_values, (u32)m.n_rows, (u32)m.n_cols, (u32)m.nnz, (unsigned long long *)block[0]);
    PANDA_TRY(hipGetLastError());
    uint64_t host = 0;
    PANDA_TRY(hipMemcpyAsync(&host, block[0], 8, hipMemcpyDeviceToHost, stream));
    PANDA_TRY(hipStreamSynchronize(stream));
    const unsigned cls = host == ~(uint64_t)0 ? 0u : (unsigned)(host >> 32);
    if (defect) *defect = cls;
    if (where) *where = (cls == 2 || cls == 4 || cls == 5) ? (host & 0xFFFFFFFFu) : ~(uint64_t)0;
    return hipSuccess;
}

} // namespace

extern "C" {

// The calls: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_sparse_matvec(unsigned field, const panda_csr_matrix *m, const void *d_z, void *d_out, unsigned batch, panda_stream stream)
{
    if (!matvec_arguments_valid(field, m, d_z, d_out, batch)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_matvec<decltype(fr)>(s, *m, d_z, d_out, batch)); });
}

panda_error panda_sparse_check(unsigned field, const panda_csr_matrix *m, unsigned *defect, uint64_t *where, panda_stream stream)
{
    if (!matrix_valid(field, m, 1) || (!defect && !where) || matrix_too_short(*m)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_check<decltype(fr)>(s, *m, defect, where)); });
}

panda_error panda_sparse_plan(uint64_t n_rows, uint64_t n_cols, uint64_t nnz, unsigned batch, unsigned *tile, unsigned *carry_chunk, size_t *scratch_bytes,
                              unsigned *launches)
{
    if (!panda_sparse::shape_valid(n_rows, n_cols, nnz, batch)) return panda_error_invalid_value;
    if (tile) *tile = TILE;
    if (carry_chunk) *carry_chunk = FIXUP_CHUNK;
    if (scratch_bytes) *scratch_bytes = nnz == 0 ? 0 : matvec_scratch_bytes(nnz, batch);
    if (launches) *launches = matvec_launches(nnz);
    return panda_success;
}

} // extern "C"
