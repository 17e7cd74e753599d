// sumcheck.hip -- sumcheck rounds over multilinear tables (panda_sumcheck_round, panda_mle_fold, panda_mle_eq_table, panda_sumcheck_plan;
// DESIGN.md 5.7): the step HyperPlonk, Spartan, GKR, Lasso / Jolt and every zerocheck are built on.  A table is 2^k wire elements; a round
// binds one variable, the lowest (pair i = f[2i], f[2i+1]) or the highest (f[i], f[i + 2^(k-1)]):
//
//   fold        F[i] = lo + r (hi - lo)
//   round       g(t) = sum_i sum_terms coeff_term prod_f ( lo_{c_f, i} + t (hi_{c_f, i} - lo_{c_f, i}) ),  t = 0 .. n_evals - 1
//
// The round is two launches.  k_sumcheck_round: workgroup a covers the pairs a THREADS .. (a + 1) THREADS - 1, one pair per thread (the
// resource listing in 5.7 is why); a thread walks the expression -- panda_sop::Program, the data-driven expression of the sum of products
// -- at the NE points with one accumulator and one running product per point (sumcheck.h: arithmetic, bounds), the workgroup adds the
// threads' sums and stores tt[t][a].  k_sumcheck_totals: workgroup t adds the tile sums of point t.  The fused round binds the previous
// challenge in the same pass: a thread's pair is then a pair of FOLDED elements, each folded in registers from its two source elements;
// the thread stores the two folded elements of a column after the last factor that reads the column, and never reads them back.  Field
// addition is exact, so the bytes do not depend on the order of the sums.  No kernel waits for another workgroup; no atomics.
#include <string.h>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poly_scan.h"
#include "poly_sum.h"
#include "sumcheck.h"

using namespace panda29;
using namespace panda_poly; // tiles_of, block_reduce, walk_totals, ranges_overlap, wire_below_modulus, take_scratch
using panda_sumcheck::EqFactors;
using panda_sumcheck::Round;

static_assert(PANDA_SUMCHECK_MAX_EVALS == PANDA_SUMCHECK_PROGRAM_EVALS, "evaluation points");
static_assert(PANDA_MLE_BIND_LOW == panda_sumcheck::BIND_LOW && PANDA_MLE_BIND_HIGH == panda_sumcheck::BIND_HIGH, "binding orders");
static_assert(PANDA_MLE_PROGRAM_LOG_N == MAX_LOG_ELEMS, "the eq table's factor array covers every size");
static_assert(sizeof(panda_sop_factor) == 8, "build_program reads factors as {u32, i32} pairs");

namespace {

constexpr int CE = 4;                       // tile sums per thread of the second level
constexpr unsigned TILE_PAIRS = THREADS;    // one pair per thread
constexpr unsigned CHUNK = THREADS * CE;
constexpr int EQ_BITS = 3, EQ_E = 1 << EQ_BITS; // the eq kernel: a thread's elements differ in bits 8 .. 10 of the index
constexpr unsigned EQ_TILE = THREADS * EQ_E;
static_assert(THREADS == 256, "the eq kernel takes bits 0 .. 7 of an index from the thread");

// poly_scan.h's operation: the field's sum, canonical in and out (poly_sum.h)
struct OpAdd {
    template <class Fr>
    static __device__ __forceinline__ void identity(Fe<Fr> &r) { fe_zero(r); }
    template <class Fr>
    static __device__ __forceinline__ void combine(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b) { add_canon(r, a, b); }
    template <class Fr, int RUN>
    static __device__ __forceinline__ void run(Fe<Fr> &g, const Fe<Fr> (&x)[RUN]) { sum_run<Fr, RUN>(g, x); }
};

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

// an element at a device address held as an integer: the casts name the global address space, which the compiler cannot infer for an
// address read out of the program (a generic pointer would make every access a flat one)
template <class Fr>
__device__ __forceinline__ void load_global(Fe<Fr> &v, u64 address)
{
    typedef const u32x4 __attribute__((address_space(1))) *global_u32x4;
    const global_u32x4 s4 = (global_u32x4)address;
    const u32x4 lo = s4[0], hi = s4[1];
    const u32 w8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    fe_unpack(v, w8);
}
// a canonical value
template <class Fr>
__device__ __forceinline__ void store_global(u64 address, const Fe<Fr> &v)
{
    typedef u32x4 __attribute__((address_space(1))) *global_u32x4;
    u32 w8[8];
    fe_pack(w8, v);
    const global_u32x4 d4 = (global_u32x4)address;
    u32x4 lo, hi;
    lo.x = w8[0], lo.y = w8[1], lo.z = w8[2], lo.w = w8[3];
    hi.x = w8[4], hi.y = w8[5], hi.z = w8[6], hi.w = w8[7];
    d4[0] = lo;
    d4[1] = hi;
}

// pair i of a table of 2 * pairs elements: the indices of lo and hi
__device__ __forceinline__ void pair_of(u32 &lo, u32 &hi, u32 i, u32 pairs, u32 order)
{
    lo = order ? i : 2 * i;
    hi = order ? i + pairs : 2 * i + 1;
}

// launch 1.  pairs: the pairs the sums run over -- of the tables as they stand, or (FUSED) of the folded tables, whose elements jl, jh a
// thread folds from the source pairs of 4 * pairs elements.  tt[t * tiles + a] = the sum of point t over tile a.  A lane past the end
// computes pair 0, stores nothing and contributes zero, so no load sits under a divergent branch.
template <class Fr, int NE, bool FUSED>
__global__ void __launch_bounds__(THREADS) k_sumcheck_round(const Round *__restrict__ rd, u32 *__restrict__ tt, u32 pairs, u32 order, unsigned tiles)
{
    __shared__ u32 s_w[WAVES * NL];
    const u32 j = blockIdx.x * TILE_PAIRS + threadIdx.x;
    const bool live = j < pairs;
    const u32 i = live ? j : 0u;
    u32 jl, jh;
    pair_of(jl, jh, i, pairs, order);
    Fe<Fr> acc[NE];
    if constexpr (FUSED) {
        u32 l0, l1, h0, h1; // F[jl] from the source elements l0, l1 and F[jh] from h0, h1
        pair_of(l0, l1, jl, 2 * pairs, order);
        pair_of(h0, h1, jh, 2 * pairs, order);
        Fe<Fr> rc;
        fe_const(rc, rd->challenge);
        auto folded_pair = [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 column, bool store) {
            const u64 src = rd->prog.column[column];
            Fe<Fr> a0, a1, b0, b1;
            load_global(a0, src + (u64)l0 * 32);
            load_global(a1, src + (u64)l1 * 32);
            load_global(b0, src + (u64)h0 * 32);
            load_global(b1, src + (u64)h1 * 32);
            panda_sumcheck::fold_canon(lo, a0, a1, rc);
            panda_sumcheck::fold_canon(hi, b0, b1, rc);
            if (store && live) {
                const u64 dst = rd->folded[column];
                store_global(dst + (u64)jl * 32, lo);
                store_global(dst + (u64)jh * 32, hi);
            }
        };
        panda_sumcheck::round_pair<Fr, NE>(acc, rd->prog, [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 f) {
            folded_pair(lo, hi, rd->prog.factor[f][0], rd->store[f] != 0);
        });
        const u32 n_idle = rd->n_idle;
        for (u32 q = 0; q < n_idle; q++) {
            Fe<Fr> lo, hi;
            folded_pair(lo, hi, rd->idle[q], true);
        }
    } else {
        panda_sumcheck::round_pair<Fr, NE>(acc, rd->prog, [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 f) {
            const u64 src = rd->prog.column[rd->prog.factor[f][0]];
            load_global(lo, src + (u64)jl * 32);
            load_global(hi, src + (u64)jh * 32);
        });
    }
    Fe<Fr> zero;
    fe_zero(zero);
#pragma unroll
    for (int e = 0; e < NE; e++) {
        Fe<Fr> g;
        fe_select(g, live, acc[e], zero);
        block_reduce<OpAdd, Fr>(g, s_w);
        if (threadIdx.x == 0) store_elem(tt + ((u64)e * tiles + blockIdx.x) * 8, g);
        __syncthreads(); // s_w is free again
    }
}

// launch 2: workgroup t adds the tile sums of point t
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_sumcheck_totals(u32 *tt, u32 *__restrict__ values, unsigned tiles)
{
    __shared__ u32 s_w[WAVES * NL];
    u32 *T = tt + (u64)blockIdx.x * tiles * 8;
    Fe<Fr> sum;
    fe_zero(sum);
    walk_totals<OpAdd, Fr, CE, false>(sum, T, T, tiles, s_w);
    if (threadIdx.x == 0) store_elem(values + (u64)blockIdx.x * 8, sum);
}

// the fold alone: workgroup (a, c) covers the outputs a THREADS .. of column c.  A thread loads its pair before it stores its element,
// and with BIND_HIGH the element's index is the index of its lo: in place no other thread reads what it writes.
struct FoldArgs {
    u64 src[PANDA_SOP_PROGRAM_COLUMNS], dst[PANDA_SOP_PROGRAM_COLUMNS];
    u32 challenge[NL];
};
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_mle_fold(const FoldArgs args, u32 half, u32 order)
{
    const u32 j = blockIdx.x * THREADS + threadIdx.x;
    const bool live = j < half;
    const u32 i = live ? j : 0u;
    u32 il, ih;
    pair_of(il, ih, i, half, order);
    const u64 src = args.src[blockIdx.y], dst = args.dst[blockIdx.y];
    Fe<Fr> lo, hi, rc, F;
    fe_const(rc, args.challenge);
    load_global(lo, src + (u64)il * 32);
    load_global(hi, src + (u64)ih * 32);
    panda_sumcheck::fold_canon(F, lo, hi, rc);
    if (live) store_global(dst + (u64)i * 32, F);
}

// the eq table: thread t of workgroup a computes the EQ_E elements x = a EQ_TILE + e THREADS + t, which differ in bits 8 .. 10 alone: the
// product over every other bit once (bits 0 .. 7 select per lane, the bits from 11 up are the workgroup's), then the 2 + 4 + 8 products of
// the expansion.  Bits from log_n up carry the factor one.  A wave's stores of one e are 2 KB end to end.
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_mle_eq_table(const EqFactors *__restrict__ T, u32 *__restrict__ out, u32 n, u32 log_n)
{
    const u32 x0 = blockIdx.x * EQ_TILE + threadIdx.x;
    Fe<Fr> e[EQ_E];
    fe_const(e[0], T->one);
    for (u32 j = 0; j < log_n; j++) {
        if (j >= 8 && j < 8 + EQ_BITS) continue;
        Fe<Fr> f0, f1, f;
        fe_const(f0, T->f[j][0]);
        fe_const(f1, T->f[j][1]);
        fe_select(f, ((x0 >> j) & 1) != 0, f1, f0);
        fe_mul(e[0], e[0], f);
    }
#pragma unroll
    for (int b = EQ_BITS - 1; b >= 0; b--) {
        Fe<Fr> f0, f1;
        fe_const(f0, T->f[8 + b][0]);
        fe_const(f1, T->f[8 + b][1]);
#pragma unroll
        for (int base = 0; base < EQ_E; base += 2 << b) {
            fe_mul(e[base + (1 << b)], e[base], f1);
            fe_mul(e[base], e[base], f0);
        }
    }
#pragma unroll
    for (int k = 0; k < EQ_E; k++) {
        const u32 x = x0 + k * THREADS;
        fe_reduce_once(e[k]);
        if (x < n) store_global((u64)(uintptr_t)out + (u64)x * 32, e[k]);
    }
}

// ------------------------------------------------------------------------------------------------- the checks that need no runtime call

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

// Where the folded tables may lie (tables of 2^log_n elements, folded ones of half that).  The folded ranges are pairwise disjoint.
// folded[c] == columns[c] exactly is in place: with BIND_HIGH a thread writes only positions it alone reads, after it has read them
// ("Aliasing") -- as long as no other column shows the same bytes to another factor, so columns[c] may then overlap no
// other column.  Every other overlap of a folded range with a column is refused; with BIND_LOW a thread's output i lies where thread
// i / 2 reads, so in place is refused.
bool folds_valid(const void *const *columns, void *const *folded, unsigned n_columns, unsigned log_n, unsigned order)
{
    const size_t bytes = (size_t)32 << log_n, half = bytes / 2;
    for (unsigned c = 0; c < n_columns; c++)
        if (!columns[c] || !folded[c]) return false;
    for (unsigned c = 0; c < n_columns; c++) {
        for (unsigned d = 0; d < c; d++)
            if (ranges_overlap(folded[c], half, folded[d], half)) return false;
        for (unsigned d = 0; d < n_columns; d++) {
            if (!ranges_overlap(folded[c], half, columns[d], bytes)) continue;
            if (d != c || folded[c] != columns[c] || order != PANDA_MLE_BIND_HIGH) return false;
            for (unsigned o = 0; o < n_columns; o++)
                if (o != c && ranges_overlap(columns[c], bytes, columns[o], bytes)) return false;
        }
    }
    return true;
}

bool round_shape_valid(unsigned log_n, unsigned fused, unsigned n_evals)
{
    return fused <= 1 && log_n >= 1 + fused && log_n <= MAX_LOG_ELEMS && n_evals >= 1 && n_evals <= PANDA_SUMCHECK_MAX_EVALS;
}

bool round_arguments_valid(unsigned field, const panda_sop_expression *x, unsigned log_n, unsigned order, unsigned n_evals, const void *challenge,
                           void *const *folded, const void *evals)
{
    if (field > 2 || order > 1 || !x || !evals || (challenge == nullptr) != (folded == nullptr)) return false;
    if (!round_shape_valid(log_n, folded ? 1 : 0, n_evals)) return false;
    if (!x->columns || !x->coeffs || !x->degrees || x->scale_mode != PANDA_SOP_SCALE_NONE) return false;
    if (x->n_columns == 0 || x->n_columns > PANDA_SOP_MAX_COLUMNS || x->n_terms == 0 || x->n_terms > PANDA_SOP_MAX_TERMS) return false;
    unsigned total = 0;
    for (unsigned t = 0; t < x->n_terms; t++) {
        if (x->degrees[t] > PANDA_SOP_MAX_FACTORS) return false;
        total += x->degrees[t];
        if (total > PANDA_SOP_MAX_FACTORS) return false;
    }
    if (total > 0 && !x->factors) return false;
    for (unsigned f = 0; f < total; f++)
        if (x->factors[f].column >= x->n_columns || x->factors[f].rotation != 0) return false;
    for (unsigned c = 0; c < x->n_columns; c++)
        if (!x->columns[c]) return false;
    if (folded && !folds_valid(x->columns, folded, x->n_columns, log_n, order)) return false;
    return with_field(field, [&](auto fr) {
        typedef decltype(fr) Fr;
        return elements_valid<Fr>(x->coeffs, x->n_terms) && (!challenge || elements_valid<Fr>(challenge, 1));
    });
}

// ------------------------------------------------------------------------------------------------- the calls

template <class Fr, bool FUSED>
void launch_round(hipStream_t stream, unsigned ne, unsigned tiles, const Round *d_round, u32 *d_tt, u32 pairs, u32 order)
{
#define PANDA_SUMCHECK_LAUNCH(NE) \
    hipLaunchKernelGGL((k_sumcheck_round<Fr, NE, FUSED>), dim3(tiles), dim3(THREADS), 0, stream, d_round, d_tt, pairs, order, tiles)
    switch (ne) {
    case 2: PANDA_SUMCHECK_LAUNCH(2); break;
    case 3: PANDA_SUMCHECK_LAUNCH(3); break;
    case 4: PANDA_SUMCHECK_LAUNCH(4); break;
    case 6: PANDA_SUMCHECK_LAUNCH(6); break;
    default: PANDA_SUMCHECK_LAUNCH(8); break;
    }
#undef PANDA_SUMCHECK_LAUNCH
}

// the kernel's point count: register arrays are indexed by constants, so a few counts are compiled and the sums beyond n_evals dropped
unsigned compiled_evals(unsigned n_evals) { return n_evals <= 2 ? 2 : n_evals <= 4 ? n_evals : n_evals <= 6 ? 6 : 8; }

template <class Fr>
hipError_t run_round(hipStream_t stream, const panda_sop_expression &x, unsigned log_n, unsigned order, unsigned n_evals, const void *challenge,
                     void *const *folded, void *evals)
{
    const size_t bytes = (size_t)32 << log_n;
    for (unsigned c = 0; c < x.n_columns; c++) {
        if (panda::extent_too_short(x.columns[c], bytes)) return hipErrorInvalidValue;
        if (folded && panda::extent_too_short(folded[c], bytes / 2)) return hipErrorInvalidValue;
    }
    PANDA_TRY(panda::order_after_null_stream(stream));
    const u32 pairs = (u32)1 << (log_n - (folded ? 2 : 1));
    const unsigned tiles = tiles_of(pairs, TILE_PAIRS), ne = compiled_evals(n_evals);
    void *block[3]; // the program, a sum per point and tile, a value per point
    PANDA_TRY(take_scratch({sizeof(Round), (size_t)ne * tiles * 32, (size_t)PANDA_SUMCHECK_MAX_EVALS * 32}, block));
    Round *d_round = (Round *)block[0];
    u32 *d_tt = (u32 *)block[1], *d_values = (u32 *)block[2];
    Round round; // lives until the synchronise below
    panda_sumcheck::build_round<Fr>(round, x.columns, x.n_columns, x.coeffs, x.degrees, x.n_terms, x.factors, folded, challenge);
    PANDA_TRY(hipMemcpyAsync(d_round, &round, sizeof(Round), hipMemcpyHostToDevice, stream));
    if (folded)
        launch_round<Fr, true>(stream, ne, tiles, d_round, d_tt, pairs, order);
    else
        launch_round<Fr, false>(stream, ne, tiles, d_round, d_tt, pairs, order);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_sumcheck_totals<Fr>), dim3(n_evals), dim3(THREADS), 0, stream, d_tt, d_values, tiles);
    PANDA_TRY(hipGetLastError());
    PANDA_TRY(hipMemcpyAsync(evals, d_values, (size_t)n_evals * 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t run_fold(hipStream_t stream, const void *const *columns, void *const *folded, unsigned n_columns, unsigned log_n, unsigned order,
                    const void *challenge)
{
    const size_t bytes = (size_t)32 << log_n;
    for (unsigned c = 0; c < n_columns; c++)
        if (panda::extent_too_short(columns[c], bytes) || panda::extent_too_short(folded[c], bytes / 2)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    FoldArgs args;
    memset(&args, 0, sizeof(args));
    for (unsigned c = 0; c < n_columns; c++) {
        args.src[c] = (u64)(uintptr_t)columns[c];
        args.dst[c] = (u64)(uintptr_t)folded[c];
    }
    panda_sumcheck::wire_to_multiplier<Fr>(args.challenge, challenge);
    const u32 half = (u32)1 << (log_n - 1);
    hipLaunchKernelGGL((k_mle_fold<Fr>), dim3(tiles_of(half, THREADS), n_columns), dim3(THREADS), 0, stream, args, half, (u32)order);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

template <class Fr>
hipError_t run_eq_table(hipStream_t stream, const void *point, unsigned log_n, void *d_out)
{
    const u32 n = (u32)1 << log_n;
    if (panda::extent_too_short(d_out, (size_t)n * 32)) return hipErrorInvalidValue;
    PANDA_TRY(panda::order_after_null_stream(stream));
    void *block[1]; // the factors
    PANDA_TRY(take_scratch({sizeof(EqFactors)}, block));
    EqFactors factors; // lives until the synchronise below
    panda_sumcheck::build_eq_factors<Fr>(factors, point, log_n);
    PANDA_TRY(hipMemcpyAsync(block[0], &factors, sizeof(EqFactors), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL((k_mle_eq_table<Fr>), dim3(tiles_of(n, EQ_TILE)), dim3(THREADS), 0, stream, (const EqFactors *)block[0], (u32 *)d_out, n, (u32)log_n);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The calls: see include/panda_interface.h.  Every check but the extents comes before any runtime call.
panda_error panda_sumcheck_round(unsigned field, const panda_sop_expression *expr, unsigned log_n, unsigned order, unsigned n_evals, const void *challenge,
                                 void *const *folded, void *evals, panda_stream stream)
{
    if (!round_arguments_valid(field, expr, log_n, order, n_evals, challenge, folded, evals)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) {
        return static_cast<panda_error>(run_round<decltype(fr)>(s, *expr, log_n, order, n_evals, challenge, folded, evals));
    });
}

panda_error panda_mle_fold(unsigned field, const void *const *columns, void *const *folded, unsigned n_columns, unsigned log_n, unsigned order,
                           const void *challenge, panda_stream stream)
{
    if (field > 2 || order > 1 || !columns || !folded || !challenge || n_columns == 0 || n_columns > PANDA_SOP_MAX_COLUMNS) return panda_error_invalid_value;
    if (log_n < 1 || log_n > MAX_LOG_ELEMS || !folds_valid(columns, folded, n_columns, log_n, order)) return panda_error_invalid_value;
    if (!with_field(field, [&](auto fr) { return elements_valid<decltype(fr)>(challenge, 1); })) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_fold<decltype(fr)>(s, columns, folded, n_columns, log_n, order, challenge)); });
}

panda_error panda_mle_eq_table(unsigned field, const void *point, unsigned log_n, void *d_out, panda_stream stream)
{
    if (field > 2 || log_n > MAX_LOG_ELEMS || !d_out || !point) return panda_error_invalid_value;
    if (!with_field(field, [&](auto fr) { return elements_valid<decltype(fr)>(point, log_n); })) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) { return static_cast<panda_error>(run_eq_table<decltype(fr)>(s, point, log_n, d_out)); });
}

panda_error panda_sumcheck_plan(unsigned log_n, unsigned fused, unsigned n_evals, unsigned *tile_pairs, unsigned *carry_chunk, unsigned *launches)
{
    if (!round_shape_valid(log_n, fused, n_evals)) return panda_error_invalid_value;
    if (tile_pairs) *tile_pairs = TILE_PAIRS;
    if (carry_chunk) *carry_chunk = CHUNK;
    if (launches) *launches = 2;
    return panda_success;
}

} // extern "C"
