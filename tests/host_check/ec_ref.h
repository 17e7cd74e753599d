// ec_ref.h -- what the host programs of the G1 point code (ec_ntt_host.cpp, points_mul_host.cpp) check against: the AFFINE group law in
// integer arithmetic of this file's own (416-bit words, bit-serial products, binary-GCD inverses), the three curves, and the conversions
// between that world and the routines under test.  Nothing here shares code with fe29.h / curve29.h beyond those routines, which run
// under FE29_CHECK (every column accumulator and every limb range of fe29.h is asserted).  A program includes this file first, seeds
// g_rng, and prints "ok <g_checks>" at its end; any failed CHECK aborts with a message.
#pragma once
#define FE29_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../panda_amd/csrc/ec_ntt.h"

using namespace panda29;
using panda_ecntt::SCALAR_WORDS;

static long g_checks = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        g_checks++;                                     \
        if (!(c)) {                                     \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            exit(1);                                    \
        }                                               \
    } while (0)

// ------------------------------------------------------------------------------------------------- integers of 13 words
constexpr int W = 13;
struct Big {
    uint32_t w[W];
    Big() { memset(w, 0, sizeof w); }
    explicit Big(uint64_t v)
    {
        memset(w, 0, sizeof w);
        w[0] = (uint32_t)v, w[1] = (uint32_t)(v >> 32);
    }
};
static int cmp(const Big &a, const Big &b)
{
    for (int i = W - 1; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static bool is_zero(const Big &a) { return cmp(a, Big()) == 0; }
static Big add(const Big &a, const Big &b)
{
    Big r;
    uint64_t c = 0;
    for (int i = 0; i < W; i++) c += (uint64_t)a.w[i] + b.w[i], r.w[i] = (uint32_t)c, c >>= 32;
    return r;
}
static Big sub(const Big &a, const Big &b) // a >= b
{
    Big r;
    int64_t c = 0;
    for (int i = 0; i < W; i++) c += (int64_t)a.w[i] - b.w[i], r.w[i] = (uint32_t)c, c >>= 32;
    return r;
}
static Big shr1(const Big &a)
{
    Big r;
    for (int i = 0; i < W; i++) r.w[i] = (a.w[i] >> 1) | (i + 1 < W ? a.w[i + 1] << 31 : 0);
    return r;
}
static Big shl1(const Big &a)
{
    Big r;
    for (int i = W - 1; i >= 0; i--) r.w[i] = (a.w[i] << 1) | (i ? a.w[i - 1] >> 31 : 0);
    return r;
}
static bool bit(const Big &a, int i) { return (a.w[i >> 5] >> (i & 31)) & 1; }
static int bits(const Big &a)
{
    for (int i = 32 * W - 1; i >= 0; i--)
        if (bit(a, i)) return i + 1;
    return 0;
}
static Big from_hex(const char *s)
{
    Big r;
    for (; *s; s++) {
        for (int k = 0; k < 4; k++) r = shl1(r);
        r.w[0] |= (uint32_t)(*s <= '9' ? *s - '0' : (*s | 32) - 'a' + 10);
    }
    return r;
}
static Big times(const Big &p, int k)
{
    Big r;
    for (int i = 0; i < k; i++) r = add(r, p);
    return r;
}
static Big mod_add(const Big &a, const Big &b, const Big &p)
{
    Big r = add(a, b);
    return cmp(r, p) >= 0 ? sub(r, p) : r;
}
static Big mod_sub(const Big &a, const Big &b, const Big &p) { return cmp(a, b) >= 0 ? sub(a, b) : sub(add(a, p), b); }
static Big mod_mul(const Big &a, const Big &b, const Big &p)
{
    Big r;
    for (int i = bits(a) - 1; i >= 0; i--) {
        r = mod_add(r, r, p);
        if (bit(a, i)) r = mod_add(r, b, p);
    }
    return r;
}
static Big mod_pow(const Big &a, const Big &e, const Big &p)
{
    Big r(1);
    for (int i = bits(e) - 1; i >= 0; i--) {
        r = mod_mul(r, r, p);
        if (bit(e, i)) r = mod_mul(r, a, p);
    }
    return r;
}
static Big mod_inv(const Big &a, const Big &p) // binary extended Euclid, p odd, a != 0 mod p
{
    Big u = a, v = p, x1(1), x2;
    const Big one(1);
    while (cmp(u, one) != 0 && cmp(v, one) != 0) {
        while (!(u.w[0] & 1)) u = shr1(u), x1 = (x1.w[0] & 1) ? shr1(add(x1, p)) : shr1(x1);
        while (!(v.w[0] & 1)) v = shr1(v), x2 = (x2.w[0] & 1) ? shr1(add(x2, p)) : shr1(x2);
        if (cmp(u, v) >= 0)
            u = sub(u, v), x1 = mod_sub(x1, x2, p);
        else
            v = sub(v, u), x2 = mod_sub(x2, x1, p);
    }
    return cmp(u, one) == 0 ? x1 : x2;
}

static uint64_t g_rng; // xorshift; each program sets its own seed before its first draw
static uint64_t rnd()
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}

// ------------------------------------------------------------------------------------------------- the affine law
struct Pt {
    bool inf = true;
    Big x, y;
};
static bool same(const Pt &a, const Pt &b) { return a.inf == b.inf && (a.inf || (cmp(a.x, b.x) == 0 && cmp(a.y, b.y) == 0)); }
static Pt neg(const Pt &a, const Big &p)
{
    Pt r = a;
    if (!a.inf) r.y = mod_sub(Big(), a.y, p);
    return r;
}
static Pt ec_add(const Pt &P, const Pt &Q, const Big &p)
{
    if (P.inf) return Q;
    if (Q.inf) return P;
    Big lam;
    if (cmp(P.x, Q.x) == 0) {
        if (is_zero(mod_add(P.y, Q.y, p))) return Pt();
        const Big xx = mod_mul(P.x, P.x, p);
        lam = mod_mul(mod_add(mod_add(xx, xx, p), xx, p), mod_inv(mod_add(P.y, P.y, p), p), p);
    } else
        lam = mod_mul(mod_sub(Q.y, P.y, p), mod_inv(mod_sub(Q.x, P.x, p), p), p);
    Pt r;
    r.inf = false;
    r.x = mod_sub(mod_sub(mod_mul(lam, lam, p), P.x, p), Q.x, p);
    r.y = mod_sub(mod_mul(lam, mod_sub(P.x, r.x, p), p), P.y, p);
    return r;
}
static Pt ec_mul(const Big &k, const Pt &P, const Big &p)
{
    Pt r;
    for (int i = bits(k) - 1; i >= 0; i--) {
        r = ec_add(r, r, p);
        if (bit(k, i)) r = ec_add(r, P, p);
    }
    return r;
}

// ------------------------------------------------------------------------------------------------- the curves
// y^2 = x^3 + b over p with the generator (gx, gy), in hex; fr_generator generates the scalar field's multiplicative group
struct CurveText {
    const char *name, *p, *gx, *gy;
    unsigned b, fr_generator;
};
static const CurveText BN254 = {"bn254", "30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47", "1", "2", 3, 5};
static const CurveText BLS12_377 = {"bls12_377", "01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001",
                                    "008848DEFE740A67C8FC6225BF87FF5485951E2CAA9D41BB188282C8BD37CB5CD5481512FFCD394EEAB9B16EB21BE9EF",
                                    "01914A69C5102EFF1F674F5D30AFEEC4BD7FB348CA3E52D96D182AD44FB82305C2FE3D3634A9591AFD82DE55559C8EA6", 1, 22};
static const CurveText BLS12_381 = {"bls12_381", "1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB",
                                    "17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB",
                                    "08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1", 4, 7};

template <class F>
struct Curve {
    Big p, r, R, Rinv, b; // R = 2^(32 L) mod p
    Pt g;
    int r_bits;
};
// the curve of a text, its modulus checked word by word against the parameter table of the field under test
template <class F, class Fr>
static Curve<F> make_curve(const CurveText &text)
{
    Curve<F> c;
    c.p = from_hex(text.p);
    for (int i = 0; i < Fr::L; i++) c.r.w[i] = Fr::PW[i];
    for (int i = 0; i < F::L; i++) CHECK(c.p.w[i] == F::PW[i], "%s: the modulus of the parameter table", text.name);
    c.r_bits = bits(c.r);
    c.R = Big(1);
    for (int i = 0; i < 32 * F::L; i++) c.R = mod_add(c.R, c.R, c.p);
    c.Rinv = mod_inv(c.R, c.p);
    c.b = Big(text.b);
    c.g.inf = false, c.g.x = from_hex(text.gx), c.g.y = from_hex(text.gy);
    return c;
}

// ------------------------------------------------------------------------------------------------- between the two worlds
template <class F>
static void to_wire(uint32_t *w, const Big &x, const Curve<F> &c)
{
    const Big m = mod_mul(x, c.R, c.p);
    for (int i = 0; i < F::L; i++) w[i] = m.w[i];
}
template <class F>
static Big from_wire_words(const uint32_t *w, const Curve<F> &c)
{
    Big m;
    for (int i = 0; i < F::L; i++) m.w[i] = w[i];
    CHECK(cmp(m, c.p) < 0, "a wire coordinate is not canonical");
    return mod_mul(m, c.Rinv, c.p);
}
template <class F>
static void affine_wire(uint32_t *w, const Pt &P, const Curve<F> &c)
{
    memset(w, 0, 8 * F::L);
    if (P.inf) return;
    to_wire<F>(w, P.x, c);
    to_wire<F>(w + F::L, P.y, c);
}
template <class F>
static Pt affine_from_wire_words(const uint32_t *w, const Curve<F> &c)
{
    Pt r;
    bool nz = false;
    for (int i = 0; i < 2 * F::L; i++) nz |= w[i] != 0;
    if (!nz) return r;
    r.inf = false;
    r.x = from_wire_words<F>(w, c);
    r.y = from_wire_words<F>(w + F::L, c);
    return r;
}
template <class F>
static Big limb_value(const Fe<F> &a)
{
    Big r;
    for (int i = F::N - 1; i >= 0; i--) {
        for (int k = 0; k < 29; k++) r = shl1(r);
        r = add(r, Big(a.l[i]));
    }
    return r;
}
// the stored-point bounds of ec_ntt.h
template <class F>
static void check_stored(const Xyzz<F> &P, const Curve<F> &c, const char *what)
{
    if (xyzz_is_identity(P)) return;
    const Big p2 = times(c.p, 2);
    for (int i = 0; i < F::N - 1; i++) {
        CHECK(P.Y.l[i] < (1u << 29) && P.ZZ.l[i] < (1u << 29) && P.ZZZ.l[i] < (1u << 29), "%s: Y / ZZ / ZZZ limb %d not tight", what, i);
        CHECK(P.X.l[i] <= (1u << 29) + 8, "%s: X limb %d not loose", what, i);
    }
    CHECK(cmp(limb_value(P.Y), p2) < 0, "%s: Y >= 2p", what);
    CHECK(cmp(limb_value(P.ZZ), p2) < 0 && cmp(limb_value(P.ZZZ), p2) < 0, "%s: ZZ / ZZZ >= 2p", what);
    CHECK(cmp(limb_value(P.X), times(c.p, Bounds<F>::XB)) < 0, "%s: X >= XB p", what);
}
template <class F>
static Pt to_ref(const Xyzz<F> &P, const Curve<F> &c)
{
    if (xyzz_is_identity(P)) return Pt();
    Fe<F> x, y;
    xyzz_to_affine_internal(x, y, P);
    uint32_t w[2 * F::L];
    fe_to_wire(w, x);
    fe_to_wire(w + F::L, y);
    Pt r;
    r.inf = false;
    r.x = from_wire_words<F>(w, c);
    r.y = from_wire_words<F>(w + F::L, c);
    return r;
}
template <class F>
static Xyzz<F> from_ref(const Pt &P, const Curve<F> &c)
{
    uint32_t w[2 * F::L];
    affine_wire<F>(w, P, c);
    Xyzz<F> r;
    panda_ecntt::point_from_affine_wire(r, w);
    return r;
}
static void scalar_words(uint32_t (&w)[SCALAR_WORDS], const Big &k)
{
    for (int i = 0; i < SCALAR_WORDS; i++) w[i] = k.w[i];
}

// a second representative of a point: (3 P) - (2 P) through the routines, so ZZ != 1
template <class F>
static Xyzz<F> projective_form(const Pt &P, const Curve<F> &c)
{
    Xyzz<F> b = from_ref(P, c), t3, t2;
    uint32_t w[SCALAR_WORDS];
    scalar_words(w, Big(3));
    panda_ecntt::scalar_mul(t3, b, w);
    scalar_words(w, Big(2));
    panda_ecntt::scalar_mul(t2, b, w);
    panda_ecntt::negate_point(t2);
    xyzz_add(t3, t2);
    CHECK(same(to_ref(t3, c), P), "projective_form");
    check_stored(t3, c, "projective_form");
    return t3;
}
