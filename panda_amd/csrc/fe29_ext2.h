// fe29_ext2.h -- the quadratic extension B[u] / (u^2 - beta) on fe29 elements: the coordinate field of G2.  beta is a quadratic
// non-residue of the base field, chosen per field by Ext2NonResidue: -1 where -1 is a non-residue (BN254, BLS12-381), -5 for
// BLS12-377, whose p = 1 mod 4 makes -1 a square.  Included at the end of fe29.h.
//
// Ext2<B> is a field descriptor like Bn254Fq, so curve29.h's group law and the MSM kernels instantiate over it unchanged:
// Fe<Ext2<B>> is c0's limbs followed by c1's (2 N limbs, 2 L wire words: c0 || c1, the order arkworks serialises Fp2 in).
// Every arithmetic function of fe29.h that carries between limbs has an overload here that works on the halves; each half
// meets the contract of the base function it stands in for (products tight and below 2p, sums and differences loose), so
// the per-formula bounds of curve29.h hold component by component.  Products are schoolbook:
//   (a0 + a1 u)(b0 + b1 u) = (a0 b0 + beta a1 b1) + (a0 b1 + a1 b0) u
// four base products, each within the very bound curve29.h asserts for the product it stands in for (fusing a0 b1 + a1 b0
// under one reduction would need twice that), then a subtraction / addition and a multiply-free reduction back below 2p.
// a b + c d fuses the products that belong to DIFFERENT terms -- a_i b_j + c_i d_j -- which is exactly the sum curve29.h
// bounds for fe_mul_add.  No raw (un-normalised) operands.
//
// beta = -5 (ext2_c0): 5 t1 of a tight product t1 (< 2p, limbs < 2^29) is below 10p, but its limbs reach 5 2^29 -- past the 2^31 - 4
// fe_sub admits for a subtrahend.  c0 is therefore formed limb by limb as t0 + K p - 5 t1 with K p's limbs raised to a bias of 6 2^29
// (ext2_kp6, K = 10 + SubMargin = 16 for BLS12-377's Fq): no limb underflows, none reaches 2^32 (tight t0 is below 2^29), the value is
// below 18p, and fe_reduce_small_2p -- limbs <= 2^32 - 8, value < 2^9 p in -- takes it without a carry pass in front.  The fields with
// beta = -1 compile to exactly the code they had before the trait.
#pragma once

namespace panda29 {

template <class B>
struct Ext2 {
    typedef B Base;
    static constexpr int N = 2 * B::N;
    static constexpr int L = 2 * B::L;
    static constexpr int BITS = B::BITS;
    static constexpr long long HEADROOM = B::HEADROOM;
};

// beta of Fq2 = B[u] / (u^2 - beta): -1 unless the field says otherwise
template <class B>
struct Ext2NonResidue {
    static constexpr int value = -1;
};
// BLS12-377: p = 1 mod 4 (-1 is a square); -5 is a non-residue and is the beta arkworks builds its Fq2 with
template <>
struct Ext2NonResidue<Bls377Fq> {
    static constexpr int value = -5;
};

template <class B>
struct SubMargin<Ext2<B>> : SubMargin<B> {
};
template <class B, int KB>
struct SubGrowth<Ext2<B>, KB> : SubGrowth<B, KB> {
};
template <class B>
struct RawOperandOk<Ext2<B>> {
    static constexpr bool value = false;
};

template <class B>
PANDA_HD void fe_one(Fe<Ext2<B>> &r)
{
    fe_one(ext_c0(r));
    fe_zero(ext_c1(r));
}

template <class B>
PANDA_HD void fe_norm(Fe<Ext2<B>> &r, const Fe<Ext2<B>> &t)
{
    fe_norm(ext_c0(r), ext_c0(t));
    fe_norm(ext_c1(r), ext_c1(t));
}

template <class B>
PANDA_HD void fe_carry(Fe<Ext2<B>> &a)
{
    fe_carry(ext_c0(a));
    fe_carry(ext_c1(a));
}

template <class B>
PANDA_HD void fe_reduce_once(Fe<Ext2<B>> &a)
{
    fe_reduce_once(ext_c0(a));
    fe_reduce_once(ext_c1(a));
}

template <class B>
PANDA_HD void fe_reduce_small_2p(Fe<Ext2<B>> &a)
{
    fe_reduce_small_2p(ext_c0(a));
    fe_reduce_small_2p(ext_c1(a));
}

// KP[K] with the per-limb bias raised from 4 2^29 to 6 2^29 (same value, K p): t0 + bias - 5 t1 neither underflows for t1 limbs up to
// 5 (2^29 - 1) nor overflows 32 bits for tight t0 (below 8 2^29)
template <class B, int K>
PANDA_HD constexpr u32 ext2_kp6(int i)
{
    return i == 0 ? B::KP[K][0] + (2u << LIMB_BITS) : (i < B::N - 1 ? B::KP[K][i] + (2u << LIMB_BITS) - 2u : B::KP[K][i] - 2u);
}

// c0 = t0 + beta t1 for tight t0, t1 (< 2p each), tight and below 2p
template <class B>
PANDA_HD void ext2_c0(Fe<B> &c0, const Fe<B> &t0, const Fe<B> &t1)
{
    constexpr int NR = Ext2NonResidue<B>::value;
    if constexpr (NR == -1) {
        fe_sub<B, 2>(c0, t0, t1); // < (2 + 2 + M) p, loose
    } else {
        // t0 - 5 t1 + K p limb by limb, no carry pass: 5 t1 < 10p, K = 10 + M; the sum is below (2 + KEFF[K]) p and its limbs at most
        // 2^32 - 8 (t0 + 6 2^29 + a limb of K p), which is the input fe_reduce_small_2p takes (it starts with a sequential carry)
        static_assert(NR == -5, "Ext2: beta = -1 or -5");
        constexpr int K = 10 + SubMargin<B>::value;
        static_assert(ext2_kp6<B, K>(B::N - 1) >= 5 * (2 * B::P[B::N - 1] + 1), "Ext2: K p too small for the top limb of 5 t1");
#pragma unroll
        for (int i = 0; i < B::N; i++) {
            const u32 kp = ext2_kp6<B, K>(i);
#if defined(FE29_CHECK)
            assert((i == B::N - 1 || (t0.l[i] < (1u << LIMB_BITS) && t1.l[i] < (1u << LIMB_BITS))) && "ext2_c0: tight operands");
            assert((u64)t0.l[i] + kp >= 5ull * t1.l[i] && (u64)t0.l[i] + kp - 5ull * t1.l[i] < (1ull << 32) && "ext2_c0 limb range");
#endif
            c0.l[i] = t0.l[i] + kp - 5u * t1.l[i];
        }
    }
    fe_reduce_small_2p(c0); // tight, < 2p
}

// (a0 b0 + beta a1 b1) + (a0 b1 + a1 b0) u; components tight, < 2p.  Every a_i b_j within the base contract of fe_mul.
template <class B>
PANDA_HD void fe_mul(Fe<Ext2<B>> &r, const Fe<Ext2<B>> &a, const Fe<Ext2<B>> &b)
{
    Fe<B> t0, t1, t2, t3, c0, c1;
    fe_mul(t0, ext_c0(a), ext_c0(b));
    fe_mul(t1, ext_c1(a), ext_c1(b));
    fe_mul(t2, ext_c0(a), ext_c1(b));
    fe_mul(t3, ext_c1(a), ext_c0(b));
    ext2_c0(c0, t0, t1);
    fe_add_nr(c1, t2, t3);    // < 4p, limbs < 2^30
    fe_reduce_small_2p(c1);
    ext_c0(r) = c0;
    ext_c1(r) = c1;
}

// (a0^2 + beta a1^2) + 2 a0 a1 u
template <class B>
PANDA_HD void fe_sqr(Fe<Ext2<B>> &r, const Fe<Ext2<B>> &a)
{
    Fe<B> t0, t1, c0, c1, m;
    fe_sqr(t0, ext_c0(a));
    fe_sqr(t1, ext_c1(a));
    fe_mul(m, ext_c0(a), ext_c1(a));
    ext2_c0(c0, t0, t1);
    fe_add_nr(c1, m, m); // < 4p, limbs < 2^30
    fe_reduce_small_2p(c1);
    ext_c0(r) = c0;
    ext_c1(r) = c1;
}

// a b + c d.  Each fused pair a_i b_j + c_i d_j is the sum the base fe_mul_add is specified for (value < 0.9 R p is what the
// caller's bound on a b + c d means component by component).
template <class B>
PANDA_HD void fe_mul_add(Fe<Ext2<B>> &r, const Fe<Ext2<B>> &a, const Fe<Ext2<B>> &b, const Fe<Ext2<B>> &c, const Fe<Ext2<B>> &d)
{
    Fe<B> p0, p1, q0, q1, c0, c1;
    fe_mul_add(p0, ext_c0(a), ext_c0(b), ext_c0(c), ext_c0(d)); // a0 b0 + c0 d0
    fe_mul_add(p1, ext_c1(a), ext_c1(b), ext_c1(c), ext_c1(d)); // a1 b1 + c1 d1
    fe_mul_add(q0, ext_c0(a), ext_c1(b), ext_c0(c), ext_c1(d)); // a0 b1 + c0 d1
    fe_mul_add(q1, ext_c1(a), ext_c0(b), ext_c1(c), ext_c0(d)); // a1 b0 + c1 d0
    ext2_c0(c0, p0, p1);                                         // p0 + beta p1
    fe_add_nr(c1, q0, q1);
    fe_reduce_small_2p(c1);
    ext_c0(r) = c0;
    ext_c1(r) = c1;
}

// both components 0 or p (tight values below 2p)
template <class B>
PANDA_HD bool fe_is_zero_2p(const Fe<Ext2<B>> &a)
{
    return fe_is_zero_2p(ext_c0(a)) && fe_is_zero_2p(ext_c1(a));
}

template <class B>
PANDA_HD void fe_unpack(Fe<Ext2<B>> &r, const u32 *w)
{
    fe_unpack(ext_c0(r), w);
    fe_unpack(ext_c1(r), w + B::L);
}

template <class B>
PANDA_HD void fe_pack(u32 *w, const Fe<Ext2<B>> &a)
{
    fe_pack(w, ext_c0(a));
    fe_pack(w + B::L, ext_c1(a));
}

template <class B>
PANDA_HD void fe_from_wire(Fe<Ext2<B>> &r, const u32 *w)
{
    fe_from_wire(ext_c0(r), w);
    fe_from_wire(ext_c1(r), w + B::L);
}

template <class B>
PANDA_HD void fe_to_wire(u32 *w, const Fe<Ext2<B>> &a)
{
    fe_to_wire(w, ext_c0(a));
    fe_to_wire(w + B::L, ext_c1(a));
}

template <class B>
PANDA_HD void fe_from_u32(Fe<Ext2<B>> &r, u32 v)
{
    fe_from_u32(ext_c0(r), v);
    fe_zero(ext_c1(r));
}

// 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 - beta a1^2); 0 -> 0 (the norm of a non-zero element is non-zero: beta is a non-residue)
template <class B>
PANDA_HD void fe_inv(Fe<Ext2<B>> &r, const Fe<Ext2<B>> &a)
{
    Fe<B> n, ni, c0, c1, t;
    if constexpr (Ext2NonResidue<B>::value == -1) {
        fe_mul_add(n, ext_c0(a), ext_c0(a), ext_c1(a), ext_c1(a));
    } else {
        Fe<B> a5; // -beta a1 = 5 a1: limbs < 5 (2^29 + 8) for tight or loose a1, carried once (loose)
#pragma unroll
        for (int i = 0; i < B::N; i++) a5.l[i] = ext_c1(a).l[i] * (u32)(-Ext2NonResidue<B>::value);
        fe_norm(a5, a5);
        fe_mul_add(n, ext_c0(a), ext_c0(a), a5, ext_c1(a));
    }
    fe_inv(ni, n);
    fe_mul(c0, ext_c0(a), ni);
    fe_mul(t, ext_c1(a), ni);
    fe_neg<B, 2>(c1, t);
    fe_reduce_small_2p(c1);
    ext_c0(r) = c0;
    ext_c1(r) = c1;
}

} // namespace panda29
