// poly_terms.hip -- fused sum-of-products evaluation over device columns (panda_poly_sum_of_products, panda_poly_sum_of_products_plan;
// DESIGN.md 5.5): the quotient step of a PLONK / halo2 / Groth16 prover's round and every other element-wise polynomial expression,
//
//   out[p][i] = s(p, i) * sum_t coeff_t * prod_{f < degree_t} column[c_tf][p][(i + r_tf) mod n]
//
// in registers and in ONE pass over HBM.  One launch: workgroup (p, a) covers tile a of vector p, TILE = THREADS * E elements, thread t the
// elements a TILE + e THREADS + t (a wave's loads of one factor are 2 KB end to end).  The expression is data: the host folds the wire
// form's constants into the coefficients and scales (poly_terms.h: arithmetic, bounds), copies the program -- column pointers, reduced
// rotations, term offsets, coefficients, scales -- into the calling thread's arena scratch, and the kernel walks it at wave-uniform
// addresses.  A thread loads everything it needs before it stores, and stores only the indices it owns; with every factor on a column
// that IS d_out at rotation 0 no other thread reads what it writes, which is the in-place rule the entry point enforces.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"
#include "poly_terms.h"

using namespace panda29;
using namespace panda_poly; // store_elem, shape_invalid, ranges_overlap, wire_below_modulus
using panda_sop::Program;

static_assert(PANDA_SOP_MAX_COLUMNS == PANDA_SOP_PROGRAM_COLUMNS && PANDA_SOP_MAX_TERMS == PANDA_SOP_PROGRAM_TERMS &&
                  PANDA_SOP_MAX_FACTORS == PANDA_SOP_PROGRAM_FACTORS && PANDA_SOP_MAX_SCALES == PANDA_SOP_PROGRAM_SCALES,
              "the program's arrays are the interface's caps");
static_assert(PANDA_SOP_SCALE_NONE == panda_sop::SCALE_NONE && PANDA_SOP_SCALE_PER_VECTOR == panda_sop::SCALE_PER_VECTOR &&
                  PANDA_SOP_SCALE_CYCLIC == panda_sop::SCALE_CYCLIC,
              "scale modes");
static_assert(sizeof(panda_sop_factor) == 8, "build_program reads factors as {u32, i32} pairs");

namespace {

constexpr int E = 2; // elements per thread (the resource listing)
constexpr unsigned TILE = THREADS * E;

// load_elem from a device address held as an integer: the cast names the global address space, which the compiler cannot infer for an
// address read out of the program (a generic pointer would make every column load a flat_load)
template <class Fr>
__device__ __forceinline__ void load_global(Fe<Fr> &v, u64 address)
{
    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
    typedef const u32x4 __attribute__((address_space(1))) *global_u32x4;
    const global_u32x4 s4 = (global_u32x4)address;
    const u32x4 lo = s4[0], hi = s4[1];
    const u32 w8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    fe_unpack(v, w8);
}

template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sum_of_products(const Program *__restrict__ prog, u32 *out, u32 n, unsigned tiles)
{
    const unsigned blk = blockIdx.x, p = blk / tiles, a = blk - p * tiles;
    const u64 base = (u64)p * n;
    u32 i[E];
    bool live[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const u32 j = a * TILE + e * THREADS + threadIdx.x;
        live[e] = j < n;
        i[e] = live[e] ? j : 0u; // a lane beyond n computes element 0 and stores nothing
    }
    Fe<Fr> r[E];
    panda_sop::evaluate<Fr, E>(r, *prog, p, i, n, [&](Fe<Fr> &v, u32 column, u32 j) {
        load_global(v, prog->column[column] + (base + j) * 32);
    });
#pragma unroll
    for (int e = 0; e < E; e++)
        if (live[e]) store_elem(out + (base + i[e]) * 8, r[e]);
}

// `count` wire elements (HOST, any alignment), each below the modulus
template <class Fr>
bool elements_valid(const void *wire, unsigned count)
{
    for (unsigned k = 0; k < count; k++) {
        u32 w[8];
        memcpy(w, (const char *)wire + 32 * (size_t)k, sizeof(w));
        if (!wire_below_modulus<Fr>(w)) return false;
    }
    return true;
}

template <class Fr>
bool constants_valid(const panda_sop_expression &x)
{
    return elements_valid<Fr>(x.coeffs, x.n_terms) && (x.scale_mode == PANDA_SOP_SCALE_NONE || elements_valid<Fr>(x.scales, x.n_scales));
}

// every check of the entry point that needs no runtime call
bool arguments_valid(unsigned field, const panda_sop_expression *x, const void *d_out, u64 n, unsigned batch)
{
    if (field > 2 || shape_invalid(n, batch) || !x || !d_out || !x->columns || !x->coeffs || !x->degrees) return false;
    if (x->n_columns == 0 || x->n_columns > PANDA_SOP_MAX_COLUMNS || x->n_terms == 0 || x->n_terms > PANDA_SOP_MAX_TERMS) return false;
    if (x->scale_mode > PANDA_SOP_SCALE_CYCLIC) return false;
    if (x->scale_mode != PANDA_SOP_SCALE_NONE && (!x->scales || x->n_scales == 0 || x->n_scales > PANDA_SOP_MAX_SCALES)) return false;
    unsigned total = 0;
    for (unsigned t = 0; t < x->n_terms; t++) {
        if (x->degrees[t] > PANDA_SOP_MAX_FACTORS) return false;
        total += x->degrees[t];
        if (total > PANDA_SOP_MAX_FACTORS) return false;
    }
    if (total > 0 && !x->factors) return false;
    for (unsigned f = 0; f < total; f++)
        if (x->factors[f].column >= x->n_columns) return false;
    const size_t bytes = (size_t)batch * n * 32;
    bool in_place[PANDA_SOP_MAX_COLUMNS];
    for (unsigned c = 0; c < x->n_columns; c++) {
        if (!x->columns[c]) return false;
        in_place[c] = ranges_overlap(x->columns[c], bytes, d_out, bytes);
        if (in_place[c] && x->columns[c] != d_out) return false; // a partial overlap
    }
    for (unsigned f = 0; f < total; f++)
        if (in_place[x->factors[f].column] && panda_sop::reduce_rotation(x->factors[f].rotation, n) != 0) return false;
    return with_field(field, [&](auto fr) { return constants_valid<decltype(fr)>(*x); });
}

template <class Fr>
hipError_t run(hipStream_t stream, const panda_sop_expression &x, void *d_out, u64 n, unsigned batch)
{
    const size_t bytes = (size_t)batch * n * 32;
    if (panda::extent_too_short(d_out, bytes)) return hipErrorInvalidValue;
    for (unsigned c = 0; c < x.n_columns; c++)
        if (panda::extent_too_short(x.columns[c], bytes)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    void *block[1]; // the program
    PANDA_TRY(take_scratch({sizeof(Program)}, block));
    Program *d_prog = (Program *)block[0];
    Program prog; // lives until the synchronise below
    panda_sop::build_program<Fr>(prog, x.columns, x.n_columns, x.coeffs, x.degrees, x.n_terms, x.factors, x.scales, x.n_scales, x.scale_mode, n);
    PANDA_TRY(hipMemcpyAsync(d_prog, &prog, sizeof(Program), hipMemcpyHostToDevice, stream));
    const unsigned tiles = tiles_of(n, TILE);
    hipLaunchKernelGGL(k_sum_of_products<Fr>, dim3(batch * tiles), dim3(THREADS), 0, stream, (const Program *)d_prog, (u32 *)d_out, (u32)n, tiles);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The sum of products: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_poly_sum_of_products(unsigned field, const panda_sop_expression *expr, void *d_out, uint64_t n, unsigned batch, panda_stream stream)
{
    if (!arguments_valid(field, expr, d_out, n, batch)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run<decltype(fr)>(s, *expr, d_out, n, batch)); });
}

panda_error panda_poly_sum_of_products_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *launches)
{
    if (shape_invalid(n, batch)) return panda_error_invalid_value;
    if (tile) *tile = TILE;
    if (launches) *launches = 1;
    return panda_success;
}

} // extern "C"
