// Host build of the product's Fq2 arithmetic over BLS12-377's Fq (fe29.h / fe29_ext2.h, Ext2<Bls377Fq> = Fq[u] / (u^2 + 5): the
// coordinate field of BLS12-377 G2) with FE29_CHECK instrumentation (128-bit shadow column accumulators, limb-range asserts).  Test
// infrastructure: compiled by tests/test_bls377_g2.py with g++.  Elements cross the boundary in the INTERNAL form -- 2 x 14 limbs of
// 29 bits, Montgomery radix 2^406 -- so that the tests can hand in operands at the edge of the documented input bounds.
#define FE29_CHECK 1
#include "../../panda_amd/csrc/curve29.h"

#include <stddef.h>

using namespace panda29;

typedef Ext2<Bls377Fq> Fq2;
static_assert(Ext2NonResidue<Bls377Fq>::value == -5, "BLS12-377's Fq2 is built with u^2 = -5");

extern "C" {

// op 0: a b, 1: a^2, 2: a b + c d, 3: 1 / a (0 -> 0); N = 28 limbs per element
int h377_fq2_op(int op, u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t n)
{
    constexpr int N = Fq2::N;
    for (size_t i = 0; i < n; i++) {
        Fe<Fq2> x, y, z, w, o;
        for (int k = 0; k < N; k++) {
            x.l[k] = a[i * N + k];
            y.l[k] = b ? b[i * N + k] : 0;
            z.l[k] = c ? c[i * N + k] : 0;
            w.l[k] = d ? d[i * N + k] : 0;
        }
        switch (op) {
        case 0: fe_mul(o, x, y); break;
        case 1: fe_sqr(o, x); break;
        case 2: fe_mul_add(o, x, y, z, w); break;
        case 3: fe_inv(o, x); break;
        default: return 1;
        }
        for (int k = 0; k < N; k++) r[i * N + k] = o.l[k];
    }
    return 0;
}

// the c0 step of every product, t0 - 5 t1, on its own: t0, t1 tight (limbs < 2^29, value < 2p) in; tight, < 2p out
int h377_c0(u32 *r, const u32 *t0, const u32 *t1, size_t n)
{
    constexpr int N = Bls377Fq::N;
    for (size_t i = 0; i < n; i++) {
        Fe<Bls377Fq> x, y, o;
        for (int k = 0; k < N; k++) {
            x.l[k] = t0[i * N + k];
            y.l[k] = t1[i * N + k];
        }
        ext2_c0(o, x, y);
        for (int k = 0; k < N; k++) r[i * N + k] = o.l[k];
    }
    return 0;
}

// fe_reduce_small_2p over Bls377Fq (top limb of p = 0: the two-limb quotient estimate): 14 limbs < 2^32, value < 2^9 p in; tight, < 2p out
int h377_reduce_small_2p(u32 *r, const u32 *a, size_t n)
{
    constexpr int N = Bls377Fq::N;
    for (size_t i = 0; i < n; i++) {
        Fe<Bls377Fq> x;
        for (int k = 0; k < N; k++) x.l[k] = a[i * N + k];
        fe_reduce_small_2p(x);
        for (int k = 0; k < N; k++) r[i * N + k] = x.l[k];
    }
    return 0;
}

} // extern "C"
