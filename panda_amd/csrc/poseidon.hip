// poseidon.hip -- Poseidon over the scalar fields: the permutation, a sponge hash and a Merkle tree on device-resident wire elements
// (panda_poseidon_create / _destroy / _permute / _hash / _merkle_tree / _plan).  poseidon.h holds the round, the
// permutation, the sponge, the table layout, the arithmetic and the bounds; here are the kernels, one thread per permutation, and the
// entry points:
//   k_permute    thread i permutes the state at element i T; it loads its T elements before it stores any, so d_out == d_in is in place
//   k_hash       thread i runs the sponge over message i; element j is at i msg_stride + j elem_stride.  A level of a tree that is wider
//                than a workgroup is this kernel with len = a, contiguous
//   k_tree_top   ONE workgroup takes the levels of at most PER_WORKGROUP nodes, a workgroup barrier between two levels
// The table of a handle is read at wave-uniform addresses.  No kernel waits for another workgroup, there are no atomics and no flags,
// every stored element is canonical: the bytes are the same on every run.
#include <string.h>

#include <mutex>
#include <set>
#include <type_traits>
#include <vector>

#include "fe29.h"
#include "panda_internal.h"
#include "poly_elem.h"
#include "poseidon.h"

using namespace panda29;
using namespace panda_poly; // load_elem, store_elem, ranges_overlap, bad_pair, with_field
using panda_hash::PER_WORKGROUP;

static_assert(PANDA_POSEIDON_MAX_WIDTH == panda_hash::MAX_WIDTH, "the interface's cap");
static_assert(PER_WORKGROUP == THREADS, "one permutation per thread of a workgroup");
static_assert(panda_hash::MAX_LOG == MAX_LOG_ELEMS, "the caps are those of every other call");

namespace {

// what a kernel needs of a handle
struct Shape {
    const u32 *table;
    u32 alpha, full_rounds, partial_rounds;
};

template <class Fr, int T>
__global__ void __launch_bounds__(THREADS) k_permute(const Shape P, const u32 *in, u32 *out, u32 n)
{
    const u32 i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    Fe<Fr> s[T];
#pragma unroll
    for (int j = 0; j < T; j++) load_elem(s[j], in + ((u64)i * T + j) * 8);
    panda_hash::permute<Fr, T>(s, P.table, P.alpha, P.full_rounds, P.partial_rounds);
#pragma unroll
    for (int j = 0; j < T; j++) store_elem(out + ((u64)i * T + j) * 8, s[j]);
}

template <class Fr, int T>
__global__ void __launch_bounds__(THREADS) k_hash(const Shape P, const u32 *__restrict__ in, u32 *__restrict__ out, u32 n, u64 len, u64 msg_stride,
                                                  u64 elem_stride, const Fe<Fr> tag)
{
    const u32 i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const u32 *msg = in + (u64)i * msg_stride * 8;
    Fe<Fr> h;
    panda_hash::sponge<Fr, T>(h, tag, len, [&](Fe<Fr> &m, u64 j) { load_elem(m, msg + j * elem_stride * 8); }, P.table, P.alpha, P.full_rounds,
                                  P.partial_rounds);
    store_elem(out + (u64)i * 8, h);
}

// levels `first` .. height of a tree of arity a = T - 1; level l has `count` a^(height - l) <= PER_WORKGROUP nodes.  Level 1 reads the
// leaves, every other level the level below it in `nodes`; offset: elements of `nodes` before level `first`.
template <class Fr, int T>
__global__ void __launch_bounds__(THREADS) k_tree_top(const Shape P, const u32 *leaves, u32 *nodes, u32 first, u32 height, u32 count, u64 offset,
                                                      const Fe<Fr> tag)
{
    constexpr u32 A = T - 1;
    const u32 *src = first == 1 ? leaves : nodes + (offset - (u64)count * A) * 8;
    u32 *dst = nodes + offset * 8;
    for (u32 l = first; l <= height; l++) {
        if (threadIdx.x < count) {
            Fe<Fr> s[T];
            s[0] = tag;
#pragma unroll
            for (int j = 1; j < T; j++) load_elem(s[j], src + ((u64)threadIdx.x * A + (j - 1)) * 8);
            panda_hash::permute<Fr, T>(s, P.table, P.alpha, P.full_rounds, P.partial_rounds);
            store_elem(dst + (u64)threadIdx.x * 8, s[0]);
        }
        __syncthreads(); // the level is in memory before the same workgroup reads it
        src = dst;
        dst += (u64)count * 8;
        count /= A;
    }
}

// ------------------------------------------------------------------------------------------------- handles

struct Handle {
    unsigned field, width, alpha, full_rounds, partial_rounds;
    void *d_table;
    size_t table_bytes;
};

std::mutex g_lock;
std::set<Handle *> g_live;

// the handle's record if it is live; a copy, so that a concurrent destroy cannot pull it away under a call's checks
bool find_handle(panda_poseidon p, Handle &out)
{
    std::lock_guard<std::mutex> hold(g_lock);
    auto it = g_live.find(static_cast<Handle *>(p.handle));
    if (!p.handle || it == g_live.end()) return false;
    out = **it;
    return true;
}

Shape shape_of(const Handle &h) { return {(const u32 *)h.d_table, h.alpha, h.full_rounds, h.partial_rounds}; }

template <class Fr>
bool tag_to_fe(Fe<Fr> &tag, const void *wire)
{
    if (!wire || !panda_hash::wire_valid<Fr>(wire)) return false;
    u32 w[8];
    memcpy(w, wire, sizeof(w));
    fe_unpack(tag, w);
    return true;
}

// f(std::integral_constant<int, T>()) for the width
template <class F>
inline auto with_width(unsigned width, F &&f)
{
    switch (width) {
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 5>());
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + THREADS - 1) / THREADS); }

template <class Fr, int T>
hipError_t run_permute(hipStream_t stream, const Handle &h, const void *d_in, void *d_out, u64 n)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    hipLaunchKernelGGL((k_permute<Fr, T>), dim3(blocks_of(n)), dim3(THREADS), 0, stream, shape_of(h), (const u32 *)d_in, (u32 *)d_out, (u32)n);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

template <class Fr, int T>
hipError_t run_hash(hipStream_t stream, const Handle &h, const void *d_in, u64 len, u64 msg_stride, u64 elem_stride, const Fe<Fr> &tag, void *d_out, u64 n)
{
    PANDA_TRY(panda::order_after_null_stream(stream));
    hipLaunchKernelGGL((k_hash<Fr, T>), dim3(blocks_of(n)), dim3(THREADS), 0, stream, shape_of(h), (const u32 *)d_in, (u32 *)d_out, (u32)n, len, msg_stride,
                       elem_stride, tag);
    PANDA_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);
}

template <class Fr, int T>
hipError_t run_tree(hipStream_t stream, const Handle &h, const void *d_leaves, unsigned height, const Fe<Fr> &tag, void *d_nodes, void *root)
{
    constexpr u64 A = T - 1;
    panda_hash::TreePlan plan;
    u64 offset[panda_hash::MAX_LOG];
    panda_hash::tree_plan(plan, T, height, offset); // the entry point has checked the shape
    PANDA_TRY(panda::order_after_null_stream(stream));
    const u32 *src = (const u32 *)d_leaves;
    u32 *nodes = (u32 *)d_nodes;
    u64 count = plan.leaves / A;
    unsigned l = 1;
    for (; l + plan.top_levels <= height; l++, count /= A) { // the wide levels
        u32 *dst = nodes + offset[l - 1] * 8;
        hipLaunchKernelGGL((k_hash<Fr, T>), dim3(blocks_of(count)), dim3(THREADS), 0, stream, shape_of(h), src, dst, (u32)count, A, A, (u64)1, tag);
        PANDA_TRY(hipGetLastError());
        src = dst;
    }
    hipLaunchKernelGGL((k_tree_top<Fr, T>), dim3(1), dim3(THREADS), 0, stream, shape_of(h), (const u32 *)d_leaves, nodes, (u32)l, (u32)height, (u32)count,
                       offset[l - 1], tag);
    PANDA_TRY(hipGetLastError());
    if (root) PANDA_TRY(hipMemcpyAsync(root, nodes + (plan.nodes - 1) * 8, 32, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace

extern "C" {

// The calls: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_poseidon_create(unsigned field, const panda_poseidon_params *params, panda_poseidon *out)
{
    if (field > 2 || !params || !out) return panda_error_invalid_value;
    const unsigned t = params->width, rf = params->full_rounds, rp = params->partial_rounds;
    const bool valid = with_field(field, [&](auto fr) {
        return panda_hash::params_valid<decltype(fr)>(t, params->alpha, rf, rp, params->round_constants, params->mds);
    });
    if (!valid) return panda_error_invalid_value;
    std::vector<u32> table(panda_hash::table_words(t, rf + rp));
    with_field(field, [&](auto fr) {
        panda_hash::build_table<decltype(fr)>(table.data(), t, params->alpha, rf, rp, params->round_constants, params->mds);
        return 0;
    });
    const size_t bytes = table.size() * 4;
    void *d_table = nullptr;
    panda_error rc = panda_malloc(&d_table, bytes);
    if (rc != panda_success) return rc;
    rc = static_cast<panda_error>(hipMemcpy(d_table, table.data(), bytes, hipMemcpyHostToDevice));
    if (rc != panda_success) {
        panda_free(d_table);
        return rc;
    }
    Handle *h = new Handle{field, t, params->alpha, rf, rp, d_table, bytes};
    {
        std::lock_guard<std::mutex> hold(g_lock);
        g_live.insert(h);
    }
    out->handle = h;
    return panda_success;
}

panda_error panda_poseidon_destroy(panda_poseidon p)
{
    Handle *h = static_cast<Handle *>(p.handle);
    {
        std::lock_guard<std::mutex> hold(g_lock);
        if (!h || g_live.erase(h) == 0) return panda_error_invalid_value;
    }
    const panda_error rc = panda_free(h->d_table);
    delete h;
    return rc;
}

panda_error panda_poseidon_permute(panda_poseidon p, const void *d_in, void *d_out, uint64_t n, panda_stream stream)
{
    Handle h;
    if (!find_handle(p, h) || !d_in || !d_out || shape_invalid(n, 1)) return panda_error_invalid_value;
    const size_t bytes = (size_t)n * h.width * 32;
    if (bad_pair(d_in, d_out, bytes) || panda::extent_too_short(d_in, bytes) || panda::extent_too_short(d_out, bytes)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(h.field, [&](auto fr) {
        return with_width(h.width, [&](auto t) { return static_cast<panda_error>(run_permute<decltype(fr), decltype(t)::value>(s, h, d_in, d_out, n)); });
    });
}

panda_error panda_poseidon_hash(panda_poseidon p, const void *d_in, uint64_t len, uint64_t msg_stride, uint64_t elem_stride, const void *tag, void *d_out,
                                uint64_t n, panda_stream stream)
{
    Handle h;
    const u64 cap = (u64)1 << panda_hash::MAX_LOG, stride_cap = cap;
    if (!find_handle(p, h) || !d_in || !d_out || !tag || len == 0 || n == 0 || len > cap || n > cap || n * len > cap) return panda_error_invalid_value;
    if (msg_stride > stride_cap || elem_stride > stride_cap) return panda_error_invalid_value; // the extent below stays inside 64 bits
    const size_t in_bytes = (size_t)((n - 1) * msg_stride + (len - 1) * elem_stride + 1) * 32, out_bytes = (size_t)n * 32;
    if (ranges_overlap(d_in, in_bytes, d_out, out_bytes) || panda::extent_too_short(d_in, in_bytes) || panda::extent_too_short(d_out, out_bytes))
        return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(h.field, [&](auto fr) {
        typedef decltype(fr) Fr;
        Fe<Fr> t0;
        if (!tag_to_fe(t0, tag)) return panda_error_invalid_value;
        return with_width(h.width, [&](auto t) {
            return static_cast<panda_error>(run_hash<Fr, decltype(t)::value>(s, h, d_in, len, msg_stride, elem_stride, t0, d_out, n));
        });
    });
}

panda_error panda_poseidon_merkle_tree(panda_poseidon p, const void *d_leaves, unsigned height, const void *tag, void *d_nodes, void *root,
                                       panda_stream stream)
{
    Handle h;
    panda_hash::TreePlan plan;
    if (!find_handle(p, h) || !d_leaves || !d_nodes || !tag || !panda_hash::tree_plan(plan, h.width, height, nullptr)) return panda_error_invalid_value;
    const size_t leaf_bytes = (size_t)plan.leaves * 32, node_bytes = (size_t)plan.nodes * 32;
    if (ranges_overlap(d_leaves, leaf_bytes, d_nodes, node_bytes) || panda::extent_too_short(d_leaves, leaf_bytes) ||
        panda::extent_too_short(d_nodes, node_bytes))
        return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    return with_field(h.field, [&](auto fr) {
        typedef decltype(fr) Fr;
        Fe<Fr> t0;
        if (!tag_to_fe(t0, tag)) return panda_error_invalid_value;
        switch (h.width) {
        case 3: return static_cast<panda_error>(run_tree<Fr, 3>(s, h, d_leaves, height, t0, d_nodes, root));
        case 4: return static_cast<panda_error>(run_tree<Fr, 4>(s, h, d_leaves, height, t0, d_nodes, root));
        default: return static_cast<panda_error>(run_tree<Fr, 5>(s, h, d_leaves, height, t0, d_nodes, root));
        }
    });
}

panda_error panda_poseidon_plan(unsigned width, unsigned height, unsigned *per_workgroup, uint64_t *nodes, uint64_t *level_offset, unsigned *top_levels,
                                unsigned *launches)
{
    panda_hash::TreePlan plan;
    if (!panda_hash::tree_plan(plan, width, height, nullptr)) return panda_error_invalid_value;
    panda_hash::tree_plan(plan, width, height, level_offset);
    if (per_workgroup) *per_workgroup = PER_WORKGROUP;
    if (nodes) *nodes = plan.nodes;
    if (top_levels) *top_levels = plan.top_levels;
    if (launches) *launches = plan.launches;
    return panda_success;
}

} // extern "C"
