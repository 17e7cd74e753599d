// Host twin of panda_debug_fe_internal: the op table of panda_amd/csrc/fe29_debug_ops.h on internal-form limbs, built for the HOST with
// FE29_CHECK instrumentation (128-bit shadow column accumulators, limb-range asserts).  Test infrastructure: compiled by
// tests/test_fe29_device_edges.py with g++.  Field ids as panda_debug_fe_internal: 0..5 the base fields of panda_debug_field_op,
// 6 / 7 / 8 Fq2 over BN254, BLS12-381 and BLS12-377 Fq.
#define FE29_CHECK 1
#include "../../panda_amd/csrc/fe29_debug_ops.h"

using namespace panda29;

template <class F>
static int run(unsigned op, u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t n)
{
    if (!fe29_debug_supported<F>(op)) return 1;
    for (size_t i = 0; i < n; i++) fe29_debug_op<F>(op, r, a, b, c, d, i);
    return 0;
}

extern "C" {
int h29_fe_internal(unsigned field_id, unsigned op, u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t n)
{
    switch (field_id) {
    case 0: return run<Bn254Fq>(op, r, a, b, c, d, n);
    case 1: return run<Bn254Fr>(op, r, a, b, c, d, n);
    case 2: return run<Bls377Fq>(op, r, a, b, c, d, n);
    case 3: return run<Bls377Fr>(op, r, a, b, c, d, n);
    case 4: return run<Bls381Fq>(op, r, a, b, c, d, n);
    case 5: return run<Bls381Fr>(op, r, a, b, c, d, n);
    case 6: return run<Ext2<Bn254Fq>>(op, r, a, b, c, d, n);
    case 7: return run<Ext2<Bls381Fq>>(op, r, a, b, c, d, n);
    case 8: return run<Ext2<Bls377Fq>>(op, r, a, b, c, d, n);
    }
    return 1;
}
}
