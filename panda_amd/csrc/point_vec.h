// point_vec.h -- the device-side store of G1 point vectors that ec_ntt.hip, points_mul.hip and kzg_open_all.hip share (HIP only: ec_ntt.h
// stays plain C++ for the host checks).  The affine wire point and the XYZZ scratch point as a thread loads and stores them, the sizes
// of both, the curve dispatch, and the launcher of the one normalisation kernel (ec_ntt.hip k_normalise).
#pragma once
#include <hip/hip_runtime.h>

#include "ec_ntt.h"

namespace panda_ecntt {

using panda29::Bls377Fq;
using panda29::Bls377Fr;
using panda29::Bls381Fq;
using panda29::Bls381Fr;
using panda29::Bn254Fq;
using panda29::Bn254Fr;

// ------------------------------------------------------------------------------------------------- loads and stores
// n32 u32 words, 16-byte aligned on both sides
template <int WORDS>
__device__ __forceinline__ void copy_words_in(u32 *dst, const u32 *__restrict__ src)
{
    static_assert(WORDS % 4 == 0, "whole uint4s");
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
#pragma unroll
    for (int i = 0; i < WORDS / 4; i++) {
        const uint4 v = s4[i];
        dst[4 * i] = v.x, dst[4 * i + 1] = v.y, dst[4 * i + 2] = v.z, dst[4 * i + 3] = v.w;
    }
}
template <int WORDS>
__device__ __forceinline__ void copy_words_out(u32 *__restrict__ dst, const u32 *src)
{
    static_assert(WORDS % 4 == 0, "whole uint4s");
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int i = 0; i < WORDS / 4; i++) d4[i] = make_uint4(src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
}

// a scratch point is the four elements' limbs as they stand: 4 N words
template <class F>
__device__ __forceinline__ void load_point(Xyzz<F> &p, const u32 *__restrict__ pts, u64 i)
{
    constexpr int N = F::N;
    u32 w[4 * N];
    copy_words_in<4 * N>(w, pts + i * (4 * N));
#pragma unroll
    for (int k = 0; k < N; k++) p.X.l[k] = w[k], p.Y.l[k] = w[N + k], p.ZZ.l[k] = w[2 * N + k], p.ZZZ.l[k] = w[3 * N + k];
}
template <class F>
__device__ __forceinline__ void store_point(u32 *__restrict__ pts, u64 i, const Xyzz<F> &p)
{
    constexpr int N = F::N;
    u32 w[4 * N];
#pragma unroll
    for (int k = 0; k < N; k++) w[k] = p.X.l[k], w[N + k] = p.Y.l[k], w[2 * N + k] = p.ZZ.l[k], w[3 * N + k] = p.ZZZ.l[k];
    copy_words_out<4 * N>(pts + i * (4 * N), w);
}

template <class F>
__device__ __forceinline__ void load_affine(Xyzz<F> &p, const u32 *__restrict__ wire, u64 i)
{
    constexpr int L = F::L;
    u32 w[2 * L];
    copy_words_in<2 * L>(w, wire + i * (2 * L));
    point_from_affine_wire(p, w);
}

// ------------------------------------------------------------------------------------------------- the host side
// f(Fq(), Fr()) for a G1 curve id; the entry points refuse curve > 2 before they get here
template <class Fn>
inline auto with_curve(unsigned curve, Fn &&f)
{
    switch (curve) {
    case 0: return f(Bn254Fq(), Bn254Fr());
    case 1: return f(Bls377Fq(), Bls377Fr());
    default: return f(Bls381Fq(), Bls381Fr());
    }
}

inline size_t affine_bytes(unsigned curve) { return curve == 0 ? 64 : 96; }
inline size_t xyzz_bytes(unsigned curve) { return curve == 0 ? 4 * 9 * 4 : 4 * 14 * 4; }

static_assert(sizeof(Xyzz<Bn254Fq>) == 144 && sizeof(Xyzz<Bls377Fq>) == 224 && sizeof(Xyzz<Bls381Fq>) == 224, "the scratch point of the plans");
static_assert(2 * Bn254Fq::L >= Bn254Fq::N && 2 * Bls377Fq::L >= Bls377Fq::N && 2 * Bls381Fq::L >= Bls381Fq::N, "an output slot holds a prefix product");

// XYZZ scratch points -> affine wire points in `out`, one inversion per CHUNK points (ec_ntt.hip k_normalise): launches on the stream,
// returns the launch's error and does not wait
hipError_t enqueue_normalise(unsigned curve, hipStream_t stream, const u32 *pts, u32 *out, u64 n);

} // namespace panda_ecntt
