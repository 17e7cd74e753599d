// curve29_debug_ops.h -- one table of the XYZZ group operations on INTERNAL-form points, shared by the device diagnostics
// (debug_gen.hip, panda_debug_xyzz_internal) and the FE29_CHECK host build (tests/host_check/curve29_internal_host.cpp), so that both
// run the very same formulas of curve29.h on the very same limbs.  No wire conversion on the way in: a stored point is the 4 W u32
// limbs store_xyzz writes (X, Y, ZZ, ZZZ; W = F::N limbs each, 2 N_base for Fq2) and an affine base is 2 W limbs (x, y), so an operand
// can sit anywhere inside the lazy-reduction contract of curve29.h -- X up to (8+M) p, Y = k p - y, a raw negated base y -- including
// its edges, which no canonical wire point reaches.
//
// Element i of every array is at i * (width of that operand).  Ops (a: stored point, b: second operand, r: output):
//   MADD_CORE            rare = xyzz_madd_core(a, bx, by); r = the point (unchanged when rare != 0), then one word holding rare   (4 W + 1)
//   MADD                 xyzz_madd(a, bx, by, base_identity); base_identity <=> all 2 W limbs of b are zero                      (4 W)
//   MADD_NEG             the same after fe_neg<F, 1> on by (by canonical, below p)
//   MADD_NEG_RAW         the same after fe_neg_raw<F, 1>: the raw value goes into xyzz_madd_core (and the rare doubling) un-normalised;
//                        an identity accumulator takes fe_norm of it, as k_accumulate does                  (RawOperandOk fields)
//   MADD_TRACE           r = P, R, PP as xyzz_madd_core forms them (3 W): only there to prove what the test vectors reach
//   DBL_AFFINE           xyzz_dbl_affine(r, bx, by)                                                                             (4 W)
//   DBL                  xyzz_dbl(r, a)                                                                                         (4 W)
//   ADD                  xyzz_add(a, b), b a stored point; with the out-of-line doubling of the field that has one              (4 W)
//   ADD_QUAD, DBL_QUAD   xyzz_add_quad / xyzz_dbl_quad of curve29_quad.h, one quad of lanes per element; r holds what each of the four
//                        lanes ended with, as four copies (16 W).  The host runs xyzz_add / xyzz_dbl and writes its result four times.
//   TO_JACOBIAN_WIRE, TO_HOMOGENEOUS_WIRE   the output conversions from a loose stored point: 3 L wire words
//   TO_AFFINE_INTERNAL   xyzz_to_affine_internal(x, y, a): 2 W limbs; a is not the identity
// The heavy operations are out of line, one copy per field, and debug_gen.hip's other kernels call the same copies.
#pragma once
#include <stddef.h>

#include "curve29.h"
#include "fe29_debug_ops.h"
#if defined(__HIPCC__)
#include "curve29_quad.h"
#endif

namespace panda29 {

enum Xyzz29DebugOp : unsigned {
    XYZZ_DBG_MADD_CORE = 0,
    XYZZ_DBG_MADD = 1,
    XYZZ_DBG_MADD_NEG = 2,
    XYZZ_DBG_MADD_NEG_RAW = 3,
    XYZZ_DBG_MADD_TRACE = 4,
    XYZZ_DBG_DBL_AFFINE = 5,
    XYZZ_DBG_DBL = 6,
    XYZZ_DBG_ADD = 7,
    XYZZ_DBG_ADD_QUAD = 8,
    XYZZ_DBG_DBL_QUAD = 9,
    XYZZ_DBG_TO_JACOBIAN_WIRE = 10,
    XYZZ_DBG_TO_HOMOGENEOUS_WIRE = 11,
    XYZZ_DBG_TO_AFFINE_INTERNAL = 12,
    XYZZ_DBG_OPS = 13
};

template <class F>
PANDA_HD constexpr bool xyzz_debug_supported(unsigned op)
{
    return op < XYZZ_DBG_OPS && (op != XYZZ_DBG_MADD_NEG_RAW || RawOperandOk<F>::value);
}

// the two ops that take four lanes per element
PANDA_HD constexpr bool xyzz_debug_is_quad(unsigned op) { return op == XYZZ_DBG_ADD_QUAD || op == XYZZ_DBG_DBL_QUAD; }

// Out-of-line copies of the heavy group operations: the diagnostics are not timed, and inlining every operation for every curve made
// debug_gen.hip the longest compile of the library.
template <class F>
FE29_DEBUG_FN void to_affine_outlined(Fe<F> &x, Fe<F> &y, const Xyzz<F> &p)
{
    xyzz_to_affine_internal(x, y, p);
}
template <class F>
FE29_DEBUG_FN void madd_outlined(Xyzz<F> &acc, const Fe<F> &x, const Fe<F> &y, bool inf)
{
    xyzz_madd(acc, x, y, inf);
}
template <class F>
FE29_DEBUG_FN void add_outlined(Xyzz<F> &acc, const Xyzz<F> &q)
{
    xyzz_add(acc, q);
}
template <class F>
FE29_DEBUG_FN void dbl_outlined(Xyzz<F> &r, const Xyzz<F> &p)
{
    xyzz_dbl(r, p);
}
template <class F>
FE29_DEBUG_FN int madd_core_outlined(Xyzz<F> &acc, const Fe<F> &x, const Fe<F> &y)
{
    return xyzz_madd_core(acc, x, y);
}
template <class F>
FE29_DEBUG_FN void dbl_affine_outlined(Xyzz<F> &r, const Fe<F> &x, const Fe<F> &y)
{
    xyzz_dbl_affine(r, x, y);
}
#if defined(__HIPCC__)
// the four-lane addition / doubling (what the MSM's fix-up and bucket-reduction trees run)
template <class F>
__device__ __noinline__ void add_quad_outlined(Xyzz<F> &acc, const Xyzz<F> &q, unsigned role)
{
    xyzz_add_quad(acc, q, role);
}
template <class F>
__device__ __noinline__ void dbl_quad_outlined(Xyzz<F> &r, const Xyzz<F> &p, unsigned role)
{
    xyzz_dbl_quad(r, p, role);
}
#endif

template <class F>
PANDA_HD void xyzz_debug_load(Xyzz<F> &p, const u32 *src)
{
    fe29_debug_load(p.X, src, 0);
    fe29_debug_load(p.Y, src, 1);
    fe29_debug_load(p.ZZ, src, 2);
    fe29_debug_load(p.ZZZ, src, 3);
}
template <class F>
PANDA_HD void xyzz_debug_store(u32 *dst, const Xyzz<F> &p)
{
    fe29_debug_store(dst, p.X, 0);
    fe29_debug_store(dst, p.Y, 1);
    fe29_debug_store(dst, p.ZZ, 2);
    fe29_debug_store(dst, p.ZZZ, 3);
}
// an affine base (2 W limbs); true when every limb is zero: the identity
template <class F>
PANDA_HD bool xyzz_debug_load_base(Fe<F> &x, Fe<F> &y, const u32 *src)
{
    fe29_debug_load(x, src, 0);
    fe29_debug_load(y, src, 1);
    return fe_all_zero(x) && fe_all_zero(y);
}

template <class F>
FE29_DEBUG_FN void xyzz_dbg_madd_core(u32 *r, const u32 *a, const u32 *b, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> acc;
    Fe<F> x, y;
    xyzz_debug_load(acc, a + i * 4 * W);
    xyzz_debug_load_base(x, y, b + i * 2 * W);
    const int rare = madd_core_outlined(acc, x, y);
    xyzz_debug_store(r + i * (4 * W + 1), acc);
    r[i * (4 * W + 1) + 4 * W] = (u32)rare;
}

// NEG: 0 = the base as it is, 1 = fe_neg<F, 1> on its y, 2 = fe_neg_raw<F, 1>
template <class F, int NEG>
FE29_DEBUG_FN void xyzz_dbg_madd(u32 *r, const u32 *a, const u32 *b, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> acc;
    Fe<F> x, y;
    xyzz_debug_load(acc, a + i * 4 * W);
    const bool inf = xyzz_debug_load_base(x, y, b + i * 2 * W);
    if constexpr (NEG == 1) {
        Fe<F> ny;
        fe_neg<F, 1>(ny, y);
        y = ny;
    }
    if constexpr (NEG == 2) {
        Fe<F> ny;
        fe_neg_raw<F, 1>(ny, y);
        if (inf) {
            // nothing to add
        } else if (xyzz_is_identity(acc)) {
            Fe<F> ty;
            fe_norm(ty, ny); // a raw negated y must not be stored
            xyzz_from_affine(acc, x, ty);
        } else {
            const int rare = madd_core_outlined(acc, x, ny);
            if (rare == 1)
                dbl_affine_outlined(acc, x, ny);
            else if (rare == 2)
                xyzz_set_identity(acc);
        }
    } else
        madd_outlined(acc, x, y, inf);
    xyzz_debug_store(r + i * 4 * W, acc);
}

// P, R, PP: the first lines of xyzz_madd_core, up to the test that picks the rare branches.  A COPY (the hot function is not edited to
// export them): whoever changes how xyzz_madd_core forms P, R or PP changes these lines with it.  tests/test_xyzz_device_edges.py ties
// the two together on the shared vectors: PP is 0 or p here exactly where MADD_CORE returns rare != 0, and R = 0 mod p exactly where
// rare = 1.
template <class F>
FE29_DEBUG_FN void xyzz_dbg_madd_trace(u32 *r, const u32 *a, const u32 *b, size_t i)
{
    typedef Bounds<F> B;
    constexpr int W = F::N;
    Xyzz<F> acc;
    Fe<F> bx, by, U2, S2, P, R, PP;
    xyzz_debug_load(acc, a + i * 4 * W);
    xyzz_debug_load_base(bx, by, b + i * 2 * W);
    fe_mul(U2, bx, acc.ZZ);
    fe_sub<F, B::XB>(P, U2, acc.X);
    fe_mul(S2, by, acc.ZZZ);
    fe_sub<F, B::YB>(R, S2, acc.Y);
    fe_sqr(PP, P);
    fe29_debug_store(r + i * 3 * W, P, 0);
    fe29_debug_store(r + i * 3 * W, R, 1);
    fe29_debug_store(r + i * 3 * W, PP, 2);
}

template <class F>
FE29_DEBUG_FN void xyzz_dbg_dbl_affine(u32 *r, const u32 *b, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> o;
    Fe<F> x, y;
    xyzz_debug_load_base(x, y, b + i * 2 * W);
    dbl_affine_outlined(o, x, y);
    xyzz_debug_store(r + i * 4 * W, o);
}

// COPIES = 4: the host's stand-in for the quad op
template <class F, int COPIES>
FE29_DEBUG_FN void xyzz_dbg_dbl(u32 *r, const u32 *a, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> p, o;
    xyzz_debug_load(p, a + i * 4 * W);
    dbl_outlined(o, p);
    for (int c = 0; c < COPIES; c++) xyzz_debug_store(r + (i * COPIES + c) * 4 * W, o);
}

template <class F, int COPIES>
FE29_DEBUG_FN void xyzz_dbg_add(u32 *r, const u32 *a, const u32 *b, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> p, q;
    xyzz_debug_load(p, a + i * 4 * W);
    xyzz_debug_load(q, b + i * 4 * W);
    add_outlined(p, q);
    for (int c = 0; c < COPIES; c++) xyzz_debug_store(r + (i * COPIES + c) * 4 * W, p);
}

#if defined(__HIP_DEVICE_COMPILE__)
// every lane of the quad calls these with the same i and its own role = lane & 3
template <class F>
__device__ __noinline__ void xyzz_dbg_add_quad(u32 *r, const u32 *a, const u32 *b, size_t i, unsigned role)
{
    constexpr int W = F::N;
    Xyzz<F> p, q;
    xyzz_debug_load(p, a + i * 4 * W);
    xyzz_debug_load(q, b + i * 4 * W);
    add_quad_outlined(p, q, role);
    xyzz_debug_store(r + (i * 4 + role) * 4 * W, p);
}
template <class F>
__device__ __noinline__ void xyzz_dbg_dbl_quad(u32 *r, const u32 *a, size_t i, unsigned role)
{
    constexpr int W = F::N;
    Xyzz<F> p, o;
    xyzz_debug_load(p, a + i * 4 * W);
    dbl_quad_outlined(o, p, role);
    xyzz_debug_store(r + (i * 4 + role) * 4 * W, o);
}
#endif

template <class F, bool HOMOGENEOUS>
FE29_DEBUG_FN void xyzz_dbg_to_wire(u32 *r, const u32 *a, size_t i)
{
    constexpr int W = F::N, L = F::L;
    Xyzz<F> p;
    u32 w[3 * L];
    xyzz_debug_load(p, a + i * 4 * W);
    if constexpr (HOMOGENEOUS)
        xyzz_to_homogeneous_wire(w, p);
    else
        xyzz_to_jacobian_wire(w, p);
#pragma unroll
    for (int k = 0; k < 3 * L; k++) r[i * 3 * L + k] = w[k];
}

template <class F>
FE29_DEBUG_FN void xyzz_dbg_to_affine(u32 *r, const u32 *a, size_t i)
{
    constexpr int W = F::N;
    Xyzz<F> p;
    Fe<F> x, y;
    xyzz_debug_load(p, a + i * 4 * W);
    to_affine_outlined(x, y, p);
    fe29_debug_store(r + i * 2 * W, x, 0);
    fe29_debug_store(r + i * 2 * W, y, 1);
}

// Runs op on element i; role = lane & 3 for the two quad ops on the device (every lane of the quad makes the call), 0 otherwise.
// Returns 1, having touched nothing, for a (field, op) pair outside the table.  WHICH picks the part of the table a caller compiles:
// XYZZ_DBG_ALL (the host twin), XYZZ_DBG_SEQUENTIAL or XYZZ_DBG_QUAD (the device's one-lane and four-lane kernels: an op of the other
// part returns 1 there).
enum Xyzz29DebugPart : int { XYZZ_DBG_ALL = 0, XYZZ_DBG_SEQUENTIAL = 1, XYZZ_DBG_QUAD = 2 };

template <class F, int WHICH = XYZZ_DBG_ALL>
PANDA_HD int xyzz_debug_op(unsigned op, u32 *r, const u32 *a, const u32 *b, size_t i, unsigned role)
{
    if (!xyzz_debug_supported<F>(op)) return 1;
    (void)role;
    if (xyzz_debug_is_quad(op)) {
        if constexpr (WHICH == XYZZ_DBG_SEQUENTIAL) {
            return 1;
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
            if (op == XYZZ_DBG_ADD_QUAD)
                xyzz_dbg_add_quad<F>(r, a, b, i, role);
            else
                xyzz_dbg_dbl_quad<F>(r, a, i, role);
#else
            if (op == XYZZ_DBG_ADD_QUAD)
                xyzz_dbg_add<F, 4>(r, a, b, i);
            else
                xyzz_dbg_dbl<F, 4>(r, a, i);
#endif
            return 0;
        }
    }
    if constexpr (WHICH == XYZZ_DBG_QUAD) {
        return 1;
    } else {
        switch (op) {
        case XYZZ_DBG_MADD_CORE: xyzz_dbg_madd_core<F>(r, a, b, i); break;
        case XYZZ_DBG_MADD: xyzz_dbg_madd<F, 0>(r, a, b, i); break;
        case XYZZ_DBG_MADD_NEG: xyzz_dbg_madd<F, 1>(r, a, b, i); break;
        case XYZZ_DBG_MADD_NEG_RAW:
            if constexpr (RawOperandOk<F>::value) xyzz_dbg_madd<F, 2>(r, a, b, i);
            break;
        case XYZZ_DBG_MADD_TRACE: xyzz_dbg_madd_trace<F>(r, a, b, i); break;
        case XYZZ_DBG_DBL_AFFINE: xyzz_dbg_dbl_affine<F>(r, b, i); break;
        case XYZZ_DBG_DBL: xyzz_dbg_dbl<F, 1>(r, a, i); break;
        case XYZZ_DBG_ADD: xyzz_dbg_add<F, 1>(r, a, b, i); break;
        case XYZZ_DBG_TO_JACOBIAN_WIRE: xyzz_dbg_to_wire<F, false>(r, a, i); break;
        case XYZZ_DBG_TO_HOMOGENEOUS_WIRE: xyzz_dbg_to_wire<F, true>(r, a, i); break;
        default: xyzz_dbg_to_affine<F>(r, a, i); break;
        }
        return 0;
    }
}

} // namespace panda29
