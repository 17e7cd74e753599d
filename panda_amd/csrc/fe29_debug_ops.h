// fe29_debug_ops.h -- one table of fe29 operations on INTERNAL-form limbs, shared by the device diagnostics (debug_gen.hip,
// panda_debug_fe_internal) and the FE29_CHECK host build (tests/host_check/fe29_internal_host.cpp), so that both run the very same
// call sequence on the very same limbs.  On the device this is the generated asm column chains of fe29_chain.h (FE29_DEVICE_CHAINS);
// on the host, the plain loops with 128-bit shadow accumulators.  No wire conversion: an element is the N u32 limbs Fe<F> holds (2 N
// for Fq2), so operands can sit anywhere inside the bounds contract of fe29.h, including its edges.
//
// Element i of every array is at i * (width of that operand).  Ops (a, b, c, d: inputs; r: output):
//   MUL            r = fe_mul(a, b)                                  SQR   r = fe_sqr(a)
//   MUL_ADD        r = fe_mul_add(a, b, c, d)
//   SUB_RAW2_MUL   r = fe_mul(fe_sub_raw<F,2>(a, b), c)              SUB_RAW8_MUL   the same with KB = 8        (9-limb fields)
//   MUL_ADD_NEG_RAW r = fe_mul_add(a, b, c, fe_neg_raw<F,2>(d))                                                   (9-limb fields)
//   SHOUP          r = fe_mul_shoup<F,false>(a, w = b, wq = c)                                                   (9-limb fields)
//   SHOUP_UNIFORM  r = fe_mul_shoup<F,true>(a, w = b, wq = c) with constant i / 64 for element i (one per wave)  (9-limb fields)
//   BFLY2, BFLY3   r = fe_mul_shoup<F,false>(fe_sub_raw_bias<F,8,U>(a, b), w = c, wq = d), U = 2, 3              (9-limb fields)
//   SHOUP_PREPARE  r = (t.w, t.q) of fe_shoup_prepare(t, a): 2 N limbs out                                       (base fields)
//   REDUCE_MAD     r = fe_reduce_mad_2p(a)      (fields with a wide top limb of p)
//   REDUCE_SMALL   r = fe_reduce_small_2p(a)    (base fields)
//   INV            r = fe_inv(a)
//   EXT2_C0        Fq2 only: r = (ext2_c0(a.c0, a.c1), 0) -- t0 + beta t1 of the two components of a
// Each op is out of line (the diagnostics are not timed; inlining all of them would dominate the build).
#pragma once
#include <stddef.h>

#include "fe29.h"

#if defined(__HIPCC__)
#define FE29_DEBUG_FN __host__ __device__ __noinline__
#else
#define FE29_DEBUG_FN __attribute__((noinline))
#endif

namespace panda29 {

enum Fe29DebugOp : unsigned {
    FE29_DBG_MUL = 0,
    FE29_DBG_SQR = 1,
    FE29_DBG_MUL_ADD = 2,
    FE29_DBG_SUB_RAW2_MUL = 3,
    FE29_DBG_SUB_RAW8_MUL = 4,
    FE29_DBG_MUL_ADD_NEG_RAW = 5,
    FE29_DBG_SHOUP = 6,
    FE29_DBG_SHOUP_UNIFORM = 7,
    FE29_DBG_BFLY2 = 8,
    FE29_DBG_BFLY3 = 9,
    FE29_DBG_SHOUP_PREPARE = 10,
    FE29_DBG_REDUCE_MAD = 11,
    FE29_DBG_REDUCE_SMALL = 12,
    FE29_DBG_INV = 13,
    FE29_DBG_EXT2_C0 = 14,
    FE29_DBG_OPS = 15
};

template <class F>
PANDA_HD constexpr bool fe29_debug_supported(unsigned op)
{
    if constexpr (IsExt2<F>::value) {
        return op == FE29_DBG_MUL || op == FE29_DBG_SQR || op == FE29_DBG_MUL_ADD || op == FE29_DBG_INV || op == FE29_DBG_EXT2_C0;
    } else {
        switch (op) {
        case FE29_DBG_MUL:
        case FE29_DBG_SQR:
        case FE29_DBG_MUL_ADD:
        case FE29_DBG_INV:
        case FE29_DBG_SHOUP_PREPARE:
        case FE29_DBG_REDUCE_SMALL: return true;
        case FE29_DBG_SUB_RAW2_MUL:
        case FE29_DBG_SUB_RAW8_MUL:
        case FE29_DBG_MUL_ADD_NEG_RAW:
        case FE29_DBG_SHOUP:
        case FE29_DBG_SHOUP_UNIFORM:
        case FE29_DBG_BFLY2:
        case FE29_DBG_BFLY3: return RawOperandOk<F>::value;
        case FE29_DBG_REDUCE_MAD: return F::P[F::N - 1] >= (1u << 16);
        default: return false;
        }
    }
}

// the constant of a wave-uniform product: every lane of the wave loaded the same word, and the product wants it in a scalar register
PANDA_HD u32 fe29_debug_uniform(u32 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

template <class F>
PANDA_HD void fe29_debug_load(Fe<F> &x, const u32 *src, size_t i)
{
#pragma unroll
    for (int k = 0; k < F::N; k++) x.l[k] = src[i * F::N + k];
}
template <class F>
PANDA_HD void fe29_debug_store(u32 *dst, const Fe<F> &x, size_t i)
{
#pragma unroll
    for (int k = 0; k < F::N; k++) dst[i * F::N + k] = x.l[k];
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_mul(u32 *r, const u32 *a, const u32 *b, size_t i)
{
    Fe<F> x, y, z;
    fe29_debug_load(x, a, i);
    fe29_debug_load(y, b, i);
    fe_mul(z, x, y);
    fe29_debug_store(r, z, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_sqr(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x, z;
    fe29_debug_load(x, a, i);
    fe_sqr(z, x);
    fe29_debug_store(r, z, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_mul_add(u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t i)
{
    Fe<F> x, y, z, w, o;
    fe29_debug_load(x, a, i);
    fe29_debug_load(y, b, i);
    fe29_debug_load(z, c, i);
    fe29_debug_load(w, d, i);
    fe_mul_add(o, x, y, z, w);
    fe29_debug_store(r, o, i);
}

template <class F, int KB>
FE29_DEBUG_FN void fe29_dbg_sub_raw_mul(u32 *r, const u32 *a, const u32 *b, const u32 *c, size_t i)
{
    Fe<F> x, y, z, t, o;
    fe29_debug_load(x, a, i);
    fe29_debug_load(y, b, i);
    fe29_debug_load(z, c, i);
    fe_sub_raw<F, KB>(t, x, y);
    fe_mul(o, t, z);
    fe29_debug_store(r, o, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_mul_add_neg_raw(u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t i)
{
    Fe<F> x, y, z, w, t, o;
    fe29_debug_load(x, a, i);
    fe29_debug_load(y, b, i);
    fe29_debug_load(z, c, i);
    fe29_debug_load(w, d, i);
    fe_neg_raw<F, 2>(t, w);
    fe_mul_add(o, x, y, z, t);
    fe29_debug_store(r, o, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_shoup(u32 *r, const u32 *a, const u32 *w, const u32 *wq, size_t i)
{
    Fe<F> x, o;
    u32 tw[F::N], tq[F::N];
    fe29_debug_load(x, a, i);
#pragma unroll
    for (int k = 0; k < F::N; k++) {
        tw[k] = w[i * F::N + k];
        tq[k] = wq[i * F::N + k];
    }
    fe_mul_shoup<F, false>(o, x, tw, tq);
    fe29_debug_store(r, o, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_shoup_uniform(u32 *r, const u32 *a, const u32 *w, const u32 *wq, size_t i)
{
    Fe<F> x, o;
    u32 tw[F::N], tq[F::N];
    fe29_debug_load(x, a, i);
    const size_t j = i / 64; // the same in every lane of a wave: the address below is wave-uniform
#pragma unroll
    for (int k = 0; k < F::N; k++) {
        tw[k] = fe29_debug_uniform(w[j * F::N + k]);
        tq[k] = fe29_debug_uniform(wq[j * F::N + k]);
    }
    fe_mul_shoup<F, true>(o, x, tw, tq);
    fe29_debug_store(r, o, i);
}

template <class F, int U>
FE29_DEBUG_FN void fe29_dbg_bfly(u32 *r, const u32 *a, const u32 *b, const u32 *w, const u32 *wq, size_t i)
{
    Fe<F> x, y, t, o;
    u32 tw[F::N], tq[F::N];
    fe29_debug_load(x, a, i);
    fe29_debug_load(y, b, i);
#pragma unroll
    for (int k = 0; k < F::N; k++) {
        tw[k] = w[i * F::N + k];
        tq[k] = wq[i * F::N + k];
    }
    fe_sub_raw_bias<F, 8, U>(t, x, y);
    fe_mul_shoup<F, false>(o, t, tw, tq);
    fe29_debug_store(r, o, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_shoup_prepare(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x;
    FeTw<F> t;
    fe29_debug_load(x, a, i);
    fe_shoup_prepare(t, x);
#pragma unroll
    for (int k = 0; k < F::N; k++) {
        r[i * 2 * F::N + k] = t.w[k];
        r[i * 2 * F::N + F::N + k] = t.q[k];
    }
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_reduce_mad(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x;
    fe29_debug_load(x, a, i);
    fe_reduce_mad_2p(x);
    fe29_debug_store(r, x, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_reduce_small(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x;
    fe29_debug_load(x, a, i);
    fe_reduce_small_2p(x);
    fe29_debug_store(r, x, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_inv(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x, z;
    fe29_debug_load(x, a, i);
    fe_inv(z, x);
    fe29_debug_store(r, z, i);
}

template <class F>
FE29_DEBUG_FN void fe29_dbg_ext2_c0(u32 *r, const u32 *a, size_t i)
{
    Fe<F> x, o;
    fe29_debug_load(x, a, i);
    ext2_c0(ext_c0(o), ext_c0(x), ext_c1(x));
    fe_zero(ext_c1(o));
    fe29_debug_store(r, o, i);
}

// Runs op on element i.  Returns 1, having touched nothing, for a (field, op) pair outside the table.
template <class F>
PANDA_HD int fe29_debug_op(unsigned op, u32 *r, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t i)
{
    if (!fe29_debug_supported<F>(op)) return 1;
    switch (op) {
    case FE29_DBG_MUL: fe29_dbg_mul<F>(r, a, b, i); break;
    case FE29_DBG_SQR: fe29_dbg_sqr<F>(r, a, i); break;
    case FE29_DBG_MUL_ADD: fe29_dbg_mul_add<F>(r, a, b, c, d, i); break;
    case FE29_DBG_INV: fe29_dbg_inv<F>(r, a, i); break;
    default:
        if constexpr (IsExt2<F>::value) {
            fe29_dbg_ext2_c0<F>(r, a, i); // the one further op of Fq2
        } else {
            switch (op) {
            case FE29_DBG_SHOUP_PREPARE: fe29_dbg_shoup_prepare<F>(r, a, i); break;
            case FE29_DBG_REDUCE_SMALL: fe29_dbg_reduce_small<F>(r, a, i); break;
            case FE29_DBG_REDUCE_MAD:
                if constexpr (F::P[F::N - 1] >= (1u << 16)) fe29_dbg_reduce_mad<F>(r, a, i);
                break;
            default:
                if constexpr (RawOperandOk<F>::value) {
                    switch (op) {
                    case FE29_DBG_SUB_RAW2_MUL: fe29_dbg_sub_raw_mul<F, 2>(r, a, b, c, i); break;
                    case FE29_DBG_SUB_RAW8_MUL: fe29_dbg_sub_raw_mul<F, 8>(r, a, b, c, i); break;
                    case FE29_DBG_MUL_ADD_NEG_RAW: fe29_dbg_mul_add_neg_raw<F>(r, a, b, c, d, i); break;
                    case FE29_DBG_SHOUP: fe29_dbg_shoup<F>(r, a, b, c, i); break;
                    case FE29_DBG_SHOUP_UNIFORM: fe29_dbg_shoup_uniform<F>(r, a, b, c, i); break;
                    case FE29_DBG_BFLY2: fe29_dbg_bfly<F, 2>(r, a, b, c, d, i); break;
                    default: fe29_dbg_bfly<F, 3>(r, a, b, c, d, i); break;
                    }
                }
            }
        }
    }
    return 0;
}

} // namespace panda29
