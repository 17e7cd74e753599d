// Host twin of panda_debug_xyzz_internal: the op table of panda_amd/csrc/curve29_debug_ops.h on internal-form points, built for the HOST
// with FE29_CHECK instrumentation (128-bit shadow column accumulators, limb-range asserts in every product, subtraction and negation).
// Test infrastructure: compiled by tests/test_xyzz_device_edges.py with g++.  Curve ids as panda_debug_curve_op: 0 / 1 / 2 = BN254,
// BLS12-377, BLS12-381 G1, 3 / 4 / 6 = G2 over BN254, BLS12-381, BLS12-377.  The two quad ops run xyzz_add / xyzz_dbl here.
#define FE29_CHECK 1
#include "../../panda_amd/csrc/curve29_debug_ops.h"

using namespace panda29;

template <class F>
static int run(unsigned op, u32 *r, const u32 *a, const u32 *b, size_t n)
{
    if (!xyzz_debug_supported<F>(op)) return 1;
    for (size_t i = 0; i < n; i++) xyzz_debug_op<F>(op, r, a, b, i, 0);
    return 0;
}

template <class F>
static int bounds(int *out)
{
    typedef Bounds<F> B;
    const int v[7] = {B::M, B::XB, B::YB, B::PB, B::RB, B::VB, B::NB};
    for (int i = 0; i < 7; i++) out[i] = v[i];
    return 0;
}

extern "C" {
int h29_xyzz_internal(unsigned curve, unsigned op, u32 *r, const u32 *a, const u32 *b, size_t n)
{
    switch (curve) {
    case 0: return run<Bn254Fq>(op, r, a, b, n);
    case 1: return run<Bls377Fq>(op, r, a, b, n);
    case 2: return run<Bls381Fq>(op, r, a, b, n);
    case 3: return run<Ext2<Bn254Fq>>(op, r, a, b, n);
    case 4: return run<Ext2<Bls381Fq>>(op, r, a, b, n);
    case 6: return run<Ext2<Bls377Fq>>(op, r, a, b, n);
    }
    return 1;
}

// M, XB, YB, PB, RB, VB, NB of Bounds<F>
int h29_curve_bounds(unsigned curve, int *out)
{
    switch (curve) {
    case 0: return bounds<Bn254Fq>(out);
    case 1: return bounds<Bls377Fq>(out);
    case 2: return bounds<Bls381Fq>(out);
    case 3: return bounds<Ext2<Bn254Fq>>(out);
    case 4: return bounds<Ext2<Bls381Fq>>(out);
    case 6: return bounds<Ext2<Bls377Fq>>(out);
    }
    return 1;
}
}
