// lookup.h -- what the kernels of lookup.hip share with the host: the hash of panda_lookup_multiplicities' join (the kernels and
// panda_lookup_home_slot run THIS code, so they cannot drift apart) and the count -> wire conversion of its last launch; kept apart
// from the kernels so that a host program can run both (tests/host_check/lookup_host.cpp, under FE29_CHECK).  DESIGN.md 5.6.
//
// Bounds (contract at the top of fe29.h; the three scalar fields have nine limbs and p < 2^255):
//   count -> wire     fe_mul((c, 0, .., 0), K): c <= 2^28 < 2^29 is a tight limb vector, K canonical: c K < 2^29 p < 0.9 R p
//                                                                               tight, < 2p; store_elem -> canonical
#pragma once
#include <stdint.h>

#include "fe29.h"

#define PANDA_LOOKUP_PROGRAM_COLUMNS 32

namespace panda_lookup {

using panda29::Fe;
using panda29::u32;
typedef uint64_t u64;

constexpr unsigned MAX_LOG_SLOTS = 29; // 2^29 >= 2 x 2^28 table rows

// ------------------------------------------------------------------------------- the hash
// Two 32-bit words out of all eight of the element: `h`, whose top log_slots bits are the home slot, and a fingerprint `fp` kept beside
// the row index in the slot, which lets a walk pass most occupants of another value without fetching their element.  Both are the
// murmur3 word mix with different seeds and round constants; the final avalanche makes every input bit reach the top bits of h.
PANDA_HD u32 rotl32(u32 x, unsigned r) { return (x << r) | (x >> (32 - r)); }
PANDA_HD u32 fmix32(u32 h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
PANDA_HD void hash_elem(const u32 (&w)[8], u32 &h, u32 &fp)
{
    u32 a = 0x9E3779B9u, b = 0x7F4A7C15u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u32 k = w[i] * 0xCC9E2D51u;
        k = rotl32(k, 15) * 0x1B873593u;
        a = rotl32(a ^ k, 13) * 5u + 0xE6546B64u;
        u32 m = (w[i] + (u32)i) * 0x2545F491u;
        m = rotl32(m, 11) * 0x9E3779B1u;
        b = rotl32(b ^ m, 17) * 5u + 0x52DCE729u;
    }
    h = fmix32(a ^ 32u);
    fp = fmix32(b ^ 32u);
}
// 1 <= log_slots <= MAX_LOG_SLOTS
PANDA_HD u32 home_slot(u32 h, unsigned log_slots) { return h >> (32 - log_slots); }

// the smallest table of 2^log_slots >= 2 n_table slots: at least half of it stays empty, so every walk ends at an empty slot
inline unsigned log_slots_of(u64 n_table)
{
    unsigned l = 1;
    while (((u64)1 << l) < 2 * n_table) l++;
    return l;
}

PANDA_HD bool words_equal(const u32 (&a)[8], const u32 (&b)[8])
{
    u32 d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
    return d == 0;
}

// ------------------------------------------------------------------------------- count -> wire
// K = W R mod p (W = 2^256, R = 2^261), canonical: fe_mul((c, 0, ..), K) = c K / R = c W, the wire form of the integer c.
template <class Fr>
inline void count_constant(Fe<Fr> &K)
{
    Fe<Fr> one, w, r2;
    panda29::fe_one(one);
    u32 ww[8];
    panda29::fe_to_wire(ww, one); // the integer W mod p
    panda29::fe_unpack(w, ww);
    panda29::fe_const(r2, Fr::K_TOINT); // R^2 mod p
    panda29::fe_mul(K, w, r2);
    panda29::fe_reduce_once(K);
}
// c <= 2^28; r tight, < 2p
template <class Fr>
PANDA_HD void count_to_wire(Fe<Fr> &r, u32 c, const Fe<Fr> &K)
{
    Fe<Fr> v;
    panda29::fe_zero(v);
    v.l[0] = c;
    panda29::fe_mul(r, v, K);
}

} // namespace panda_lookup
