// lookup.hip -- the join of a logUp lookup argument (panda_lookup_multiplicities, panda_lookup_plan, panda_lookup_home_slot).
// The argument's other step that is not field arithmetic on columns, the running sum, is poly_sum.hip.
//
// Multiplicities: m_j = the number of (column, index) pairs whose element equals table[j], counted at the FIRST row of every table value
// and zero at its later duplicates.  A join through an open-addressing hash table of 2^log_slots >= 2 n_table slots in the arena, linear
// probing from the home slot of lookup.h's hash, wrapping at the end.  A slot is one u64, (fingerprint << 32) | row, all ones when empty,
// and a u32 counter.  Three launches on the caller's stream; the launch boundary is the only ordering relied on, every loop is bounded
// by the slot count and no thread waits for a value another workgroup writes:
//   launch 1  k_lookup_build   one thread per table row j: walk from the home slot; atomicCAS(slot, empty, key_j) claims an empty slot; a
//                              taken slot with the same fingerprint has its occupant's element fetched from d_table (read-only input) and
//                              compared on all 256 bits: equal -> atomicMin(slot, key_j) and stop, else the next slot.  Equal elements
//                              have equal fingerprints, so the minimum of the keys is the minimum of the rows.
//   launch 2  k_lookup_probe   one thread per (column, index): the same walk with plain loads (nothing writes the slots in this launch);
//                              a full match adds one to the slot's counter, an empty slot is a miss.  The lanes of a wave that hit one
//                              slot are combined into one atomicAdd (ballot, popcount, the first lane adds): up to HOT_ROUNDS distinct
//                              slots per wave that way, what is left adds by itself.  Misses: one add of the popcount per wave, and the
//                              first missing lane -- the smallest (column, index) of the wave -- does the atomicMin.
//   launch 3  k_lookup_finish  one thread per table row j: the counter of the slot its walk ended in if that slot holds j, else zero;
//                              count -> wire by one fe_mul with a host constant, store_elem.
// Why the result does not depend on the arrival order: DESIGN.md 5.6.
#include <string.h>

#include "fe29.h"
#include "lookup.h"
#include "panda_internal.h"
#include "poly_elem.h"

using namespace panda29;
using namespace panda_poly;
using namespace panda_lookup;

namespace {

constexpr u64 EMPTY = ~(u64)0;
constexpr u32 NO_SLOT = ~(u32)0;
constexpr int HOT_ROUNDS = 4; // distinct slots of a wave combined by ballot before the remaining lanes add singly

struct Columns {
    const u32 *p[PANDA_LOOKUP_PROGRAM_COLUMNS];
};

__device__ __forceinline__ void load_words(u32 (&w)[8], const u32 *__restrict__ src)
{
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    const uint4 lo = s4[0], hi = s4[1];
    w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
}

__device__ __forceinline__ unsigned long long ballot64(bool b) { return __ballot(b); }

// launch 1
__global__ void __launch_bounds__(THREADS) k_lookup_build(const u32 *__restrict__ table, u32 n_table, unsigned long long *keys, u32 *__restrict__ slot_of,
                                                          unsigned log_slots)
{
    const u32 j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= n_table) return;
    u32 w[8], h, fp;
    load_words(w, table + (u64)j * 8);
    hash_elem(w, h, fp);
    const u32 slots = 1u << log_slots, mask = slots - 1;
    const u64 key = ((u64)fp << 32) | j;
    u32 s = home_slot(h, log_slots), found = NO_SLOT;
    for (u32 step = 0; step < slots; step++, s = (s + 1) & mask) {
        const u64 old = atomicCAS(&keys[s], (unsigned long long)EMPTY, (unsigned long long)key);
        if (old == EMPTY) {
            found = s;
            break;
        }
        if ((u32)(old >> 32) == fp) {
            u32 o[8];
            load_words(o, table + (u64)(u32)old * 8);
            if (words_equal(w, o)) {
                atomicMin(&keys[s], (unsigned long long)key);
                found = s;
                break;
            }
        }
    }
    slot_of[j] = found;
}

// launch 2: blockIdx.y is the column, so the column pointer is uniform in the workgroup
__global__ void __launch_bounds__(THREADS) k_lookup_probe(const u32 *__restrict__ table, Columns cols, u32 n, const unsigned long long *__restrict__ keys,
                                                          u32 *counts, unsigned long long *missing, unsigned long long *first_missing, unsigned log_slots)
{
    const u32 c = blockIdx.y, i = blockIdx.x * THREADS + threadIdx.x;
    const bool active = i < n;
    const u32 slots = 1u << log_slots, mask = slots - 1;
    u32 hit = NO_SLOT;
    bool miss = false;
    if (active) {
        u32 w[8], h, fp;
        load_words(w, cols.p[c] + (u64)i * 8);
        hash_elem(w, h, fp);
        u32 s = home_slot(h, log_slots);
        miss = true; // a table without an empty slot does not exist (slots >= 2 n_table); the bound below only ends the loop
        for (u32 step = 0; step < slots; step++, s = (s + 1) & mask) {
            const u64 k = keys[s];
            if (k == EMPTY) break;
            if ((u32)(k >> 32) == fp) {
                u32 o[8];
                load_words(o, table + (u64)(u32)k * 8);
                if (words_equal(w, o)) {
                    hit = s;
                    miss = false;
                    break;
                }
            }
        }
    }
    // hits: the lanes of the wave that found the same slot add once
    const unsigned lane = threadIdx.x & 63;
    bool pending = hit != NO_SLOT;
#pragma unroll 1
    for (int round = 0; round < HOT_ROUNDS; round++) {
        const unsigned long long todo = ballot64(pending);
        if (todo == 0) break;
        const int leader = __ffsll((long long)todo) - 1;
        const u32 slot = __shfl(hit, leader, 64);
        const bool same = pending && hit == slot;
        const unsigned long long group = ballot64(same);
        if ((int)lane == leader) atomicAdd(&counts[slot], (u32)__popcll(group));
        pending = pending && !same;
    }
    if (pending) atomicAdd(&counts[hit], 1u);
    // misses: one add per wave; the lanes hold increasing (c, i), so the first missing lane holds the wave's smallest pair
    const unsigned long long lost = ballot64(miss);
    if (lost != 0 && (int)lane == __ffsll((long long)lost) - 1) {
        atomicAdd(missing, (unsigned long long)__popcll(lost));
        atomicMin(first_missing, ((unsigned long long)c << 32) | i);
    }
}

// launch 3
template <class Fr>
__global__ void __launch_bounds__(THREADS) k_lookup_finish(u32 n_table, const unsigned long long *__restrict__ keys, const u32 *__restrict__ counts,
                                                           const u32 *__restrict__ slot_of, u32 *__restrict__ mult, Fe<Fr> K)
{
    const u32 j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= n_table) return;
    const u32 s = slot_of[j];
    u32 count = 0;
    if (s != NO_SLOT && (u32)keys[s] == j) count = counts[s];
    Fe<Fr> r;
    count_to_wire(r, count, K);
    store_elem(mult + (u64)j * 8, r);
}

struct LookupScratch {
    unsigned long long *keys, *first_missing, *missing;
    u32 *counts, *slot_of;
    size_t ones_bytes, zero_bytes; // the runs the two memsets fill, from keys and from counts
};

// keys | first_missing (filled with ones), counts | missing (filled with zeros), slot_of
size_t lookup_scratch_bytes(u64 n_table, unsigned log_slots)
{
    const size_t slots = (size_t)1 << log_slots;
    return panda::align256(slots * 8 + 8) + panda::align256(slots * 4 + 8) + panda::align256((size_t)n_table * 4) + 768;
}

hipError_t take_lookup_scratch(u64 n_table, unsigned log_slots, LookupScratch &S)
{
    const size_t slots = (size_t)1 << log_slots;
    panda::Arena &arena = panda::thread_arena();
    PANDA_TRY(arena.reserve(lookup_scratch_bytes(n_table, log_slots)));
    S.ones_bytes = slots * 8 + 8;
    S.zero_bytes = panda::align256(slots * 4) + 8;
    char *a = (char *)arena.take(S.ones_bytes), *b = (char *)arena.take(S.zero_bytes);
    S.slot_of = (u32 *)arena.take((size_t)n_table * 4);
    if (!a || !b || !S.slot_of) return hipErrorOutOfMemory;
    S.keys = (unsigned long long *)a;
    S.first_missing = (unsigned long long *)(a + slots * 8);
    S.counts = (u32 *)b;
    S.missing = (unsigned long long *)(b + panda::align256(slots * 4)); // eight-byte aligned behind the counters
    return hipSuccess;
}

template <class Fr>
hipError_t call_multiplicities(hipStream_t stream, const void *d_table, u64 n_table, const void *const *columns, unsigned n_columns, u64 n, void *d_mult, uint64_t *missing,
                               uint64_t *first_missing)
{
    if (panda::extent_too_short(d_table, (size_t)n_table * 32) || panda::extent_too_short(d_mult, (size_t)n_table * 32)) return hipErrorInvalidValue;
    Columns cols = {};
    for (unsigned c = 0; c < n_columns; c++) {
        if (panda::extent_too_short(columns[c], (size_t)n * 32)) return hipErrorInvalidValue;
        cols.p[c] = (const u32 *)columns[c];
    }
    PANDA_TRY(panda::order_after_null_stream(stream));
    const unsigned log_slots = log_slots_of(n_table);
    LookupScratch S;
    PANDA_TRY(take_lookup_scratch(n_table, log_slots, S));
    PANDA_TRY(hipMemsetAsync(S.keys, 0xFF, S.ones_bytes, stream));
    PANDA_TRY(hipMemsetAsync(S.counts, 0, S.zero_bytes, stream));
    Fe<Fr> K;
    count_constant(K);
    const unsigned row_blocks = (unsigned)((n_table + THREADS - 1) / THREADS), col_blocks = (unsigned)((n + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(k_lookup_build, dim3(row_blocks), dim3(THREADS), 0, stream, (const u32 *)d_table, (u32)n_table, S.keys, S.slot_of, log_slots);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lookup_probe, dim3(col_blocks, n_columns), dim3(THREADS), 0, stream, (const u32 *)d_table, cols, (u32)n, (const unsigned long long *)S.keys, S.counts,
                       S.missing, S.first_missing, log_slots);
    PANDA_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_lookup_finish<Fr>), dim3(row_blocks), dim3(THREADS), 0, stream, (u32)n_table, (const unsigned long long *)S.keys, (const u32 *)S.counts,
                       (const u32 *)S.slot_of, (u32 *)d_mult, K);
    PANDA_TRY(hipGetLastError());
    uint64_t host[2] = {0, 0};
    PANDA_TRY(hipMemcpyAsync(&host[0], S.missing, 8, hipMemcpyDeviceToHost, stream));
    PANDA_TRY(hipMemcpyAsync(&host[1], S.first_missing, 8, hipMemcpyDeviceToHost, stream));
    PANDA_TRY(hipStreamSynchronize(stream));
    if (missing) *missing = host[0];
    if (first_missing) *first_missing = host[1];
    return hipSuccess;
}

bool lookup_shape_invalid(u64 n_table, unsigned n_columns, u64 n)
{
    const u64 cap = (u64)1 << MAX_LOG_ELEMS;
    return n_table == 0 || n_table > cap || n_columns == 0 || n_columns > PANDA_LOOKUP_PROGRAM_COLUMNS || n == 0 || n > cap || (u64)n_columns * n > cap;
}

} // namespace

extern "C" {

// Multiplicities of a lookup: see include/panda_interface.h.  Every check but the extents comes before any runtime call.
panda_error panda_lookup_multiplicities(unsigned field, const void *d_table, uint64_t n_table, const void *const *columns, unsigned n_columns, uint64_t n, void *d_mult,
                                        uint64_t *missing, uint64_t *first_missing, panda_stream stream)
{
    if (field > 2 || lookup_shape_invalid(n_table, n_columns, n) || !d_table || !columns || !d_mult) return panda_error_invalid_value;
    const size_t tbytes = (size_t)n_table * 32, cbytes = (size_t)n * 32;
    if (ranges_overlap(d_mult, tbytes, d_table, tbytes)) return panda_error_invalid_value;
    for (unsigned c = 0; c < n_columns; c++)
        if (!columns[c] || ranges_overlap(d_mult, tbytes, columns[c], cbytes)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(field, [&](auto fr) {
        return static_cast<panda_error>(call_multiplicities<decltype(fr)>(s, d_table, n_table, columns, n_columns, n, d_mult, missing, first_missing));
    });
}

panda_error panda_lookup_plan(uint64_t n_table, unsigned n_columns, uint64_t n, unsigned *log_slots, size_t *scratch_bytes, unsigned *launches)
{
    if (lookup_shape_invalid(n_table, n_columns, n)) return panda_error_invalid_value;
    const unsigned l = log_slots_of(n_table);
    if (log_slots) *log_slots = l;
    if (scratch_bytes) *scratch_bytes = lookup_scratch_bytes(n_table, l);
    if (launches) *launches = 3;
    return panda_success;
}

panda_error panda_lookup_home_slot(unsigned field, const void *elem, unsigned log_slots, uint64_t *slot)
{
    if (field > 2 || !elem || !slot || log_slots == 0 || log_slots > MAX_LOG_SLOTS) return panda_error_invalid_value;
    u32 w[8], h, fp;
    memcpy(w, elem, 32);
    hash_elem(w, h, fp);
    *slot = home_slot(h, log_slots);
    return panda_success;
}

} // extern "C"
