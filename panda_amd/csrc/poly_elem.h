// poly_elem.h -- what poly.hip, poly_product.hip, poly_sum.hip, poly_terms.hip and lookup.hip share: the 32-byte element load / store,
// the LDS moves of a 9-limb value, and on the host the dispatch over the scalar field, the arena scratch of a call and the shape,
// overlap and modulus checks of the entry points.  The workgroup scan over these elements is poly_scan.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fe29.h"
#include "panda_internal.h"

namespace panda_poly {

using panda29::Fe;
using panda29::u32;
typedef uint64_t u64;

constexpr int NL = 9;                   // limbs of every supported scalar field
constexpr int THREADS = 256, WAVES = 4; // per workgroup
constexpr unsigned MAX_LOG_ELEMS = 28;  // batch x n <= 2^28, as for the batched transforms

template <class Fr>
__device__ __forceinline__ void load_elem(Fe<Fr> &v, const u32 *__restrict__ src)
{
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    const uint4 lo = s4[0], hi = s4[1];
    const u32 w8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    panda29::fe_unpack(v, w8);
}

// any value the kernels hold (limbs < 2^32, < 2^9 p) -> canonical -> 32 bytes
template <class Fr>
__device__ __forceinline__ void store_elem(u32 *__restrict__ dst, Fe<Fr> v)
{
    panda29::fe_reduce_small(v);
    u32 w8[8];
    panda29::fe_pack(w8, v);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    d4[0] = make_uint4(w8[0], w8[1], w8[2], w8[3]);
    d4[1] = make_uint4(w8[4], w8[5], w8[6], w8[7]);
}

__device__ __forceinline__ void lds_put(u32 *s, const u32 *l)
{
#pragma unroll
    for (int i = 0; i < NL; i++) s[i] = l[i];
}
template <class Fr>
__device__ __forceinline__ void lds_get(Fe<Fr> &r, const u32 *s)
{
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = s[i];
}

inline bool shape_invalid(u64 n, unsigned batch)
{
    const u64 cap = (u64)1 << MAX_LOG_ELEMS;
    return n == 0 || batch == 0 || n > cap || (u64)batch * n > cap;
}

// the 256-bit value of a wire element is below the modulus
template <class Fr>
inline bool wire_below_modulus(const u32 *w)
{
    for (int i = Fr::L - 1; i >= 0; i--)
        if (w[i] != Fr::PW[i]) return w[i] < Fr::PW[i];
    return false;
}

inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// two ranges of the same length may be one range or disjoint
inline bool bad_pair(const void *a, const void *b, size_t bytes) { return a != b && ranges_overlap(a, bytes, b, bytes); }

// f(Fr()) with the scalar field's parameter type; the entry points refuse field > 2 before they get here
template <class F>
inline auto with_field(unsigned field, F &&f)
{
    switch (field) {
    case 0: return f(panda29::Bn254Fr());
    case 1: return f(panda29::Bls377Fr());
    default: return f(panda29::Bls381Fr());
    }
}

// the per-call scratch of the calling host thread (its arena, released by panda_ntt_tear_down): N blocks of the given sizes, each
// aligned to 256 bytes.  A repeated call with the same sizes allocates nothing.
template <int N>
inline hipError_t take_scratch(const size_t (&bytes)[N], void *(&block)[N])
{
    size_t total = 256 * N;
    for (int i = 0; i < N; i++) total += panda::align256(bytes[i]);
    panda::Arena &arena = panda::thread_arena();
    PANDA_TRY(arena.reserve(total));
    for (int i = 0; i < N; i++)
        if (!(block[i] = arena.take(bytes[i]))) return hipErrorOutOfMemory;
    return hipSuccess;
}

} // namespace panda_poly
