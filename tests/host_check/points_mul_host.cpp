// points_mul_host.cpp -- the routines of panda_amd/csrc/points_mul.h on the host under FE29_CHECK (every column accumulator and every limb
// range of fe29.h is asserted), against the AFFINE group law in integer arithmetic of this file's own (416-bit words, bit-serial
// products, binary-GCD inverses), as tests/host_check/ec_ntt_host.cpp does for ec_ntt.h.  For the three curves:
//   scalar_bits / scalar_mul   k in {0, 1, 2, r - 1, one with the top bit of r set, the single bit 2^77, a 64-bit and a 128-bit value}: every
//                              loop length from k's own bit count up to 256 gives k P; the base in affine and in XYZZ form; P the identity
//   add_affine_wire            A the identity, A generic, A = k P (the doubling path), A = -k P (the identity)
//   scalar_from_wire           Montgomery wire residue -> the integer
//   power_table / power_scalar c s^i for i in {0, 1, 2^27 + 5, 2^28 - 1} against modular exponentiation
// Every stored point is checked against the stored-point bounds of ec_ntt.h.  Prints "ok <checks>"; any failure aborts with a message.
// Build: g++ -O2 -std=c++17 (tests/test_points_mul.py does).
#define FE29_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../panda_amd/csrc/points_mul.h"

using namespace panda29;
using namespace panda_pmul;

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

// ------------------------------------------------------------------------------------------------- between the two worlds
template <class F>
struct Curve {
    Big p, r, R, Rinv; // R = 2^(32 L) mod p
    Pt g;
    int r_bits;
};
template <class F>
static void affine_wire(uint32_t *w, const Pt &P, const Curve<F> &c)
{
    memset(w, 0, 8 * F::L);
    if (P.inf) return;
    const Big x = mod_mul(P.x, c.R, c.p), y = mod_mul(P.y, c.R, c.p);
    for (int i = 0; i < F::L; i++) w[i] = x.w[i], w[F::L + i] = y.w[i];
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
static Big limb_value(const Fe<F> &a)
{
    Big r;
    for (int i = F::N - 1; i >= 0; i--) {
        for (int k = 0; k < 29; k++) r = shl1(r);
        r = add(r, Big(a.l[i]));
    }
    return r;
}
static Big times(const Big &p, int k)
{
    Big r;
    for (int i = 0; i < k; i++) r = add(r, p);
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
static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}
static Big random_words(int words)
{
    Big r;
    for (int i = 0; i < words; i++) r.w[i] = (uint32_t)rnd();
    r.w[words - 1] |= 0x80000000u; // exactly 32 * words bits
    return r;
}

// one copy of each routine under test per field: every call site would otherwise inline the whole group law again
template <class F>
__attribute__((noinline)) static void mul(Xyzz<F> &acc, const Xyzz<F> &b, const uint32_t (&k)[SCALAR_WORDS], unsigned len)
{
    scalar_mul(acc, b, k, len);
}
template <class F>
__attribute__((noinline)) static void add_wire(Xyzz<F> &acc, const uint32_t *wire)
{
    add_affine_wire(acc, wire);
}

// a second representative of a point: (3 P) - (2 P) through the routines, so ZZ != 1
template <class F>
static Xyzz<F> projective_form(const Pt &P, const Curve<F> &c)
{
    Xyzz<F> b = from_ref(P, c), t3, t2;
    uint32_t w[SCALAR_WORDS];
    scalar_words(w, Big(3));
    mul(t3, b, w, 2);
    scalar_words(w, Big(2));
    mul(t2, b, w, 2);
    panda_ecntt::negate_point(t2);
    xyzz_add(t3, t2);
    CHECK(same(to_ref(t3, c), P), "projective_form");
    check_stored(t3, c, "projective_form");
    return t3;
}

template <class F, class Fr>
static void run_curve(const char *name, const char *p_hex, const char *gx, const char *gy)
{
    Curve<F> c;
    c.p = from_hex(p_hex);
    for (int i = 0; i < Fr::L; i++) c.r.w[i] = Fr::PW[i];
    for (int i = 0; i < F::L; i++) CHECK(c.p.w[i] == F::PW[i], "%s: the modulus of the parameter table", name);
    c.r_bits = bits(c.r);
    c.R = Big(1);
    for (int i = 0; i < 32 * F::L; i++) c.R = mod_add(c.R, c.R, c.p);
    c.Rinv = mod_inv(c.R, c.p);
    c.g.inf = false, c.g.x = from_hex(gx), c.g.y = from_hex(gy);
    CHECK(ec_mul(c.r, c.g, c.p).inf, "%s: order of the generator", name);
    Big seed = random_words(7);
    const Pt P = ec_mul(seed, c.g, c.p), Q = ec_mul(Big(11), c.g, c.p);
    Xyzz<F> id;
    xyzz_set_identity(id);

    Big top, single;
    top.w[(c.r_bits - 1) >> 5] = 1u << ((c.r_bits - 1) & 31);
    single.w[77 >> 5] = 1u << (77 & 31);
    const Big ks[] = {Big(), Big(1), Big(2), sub(c.r, Big(1)), add(top, Big(5)), single, random_words(2), random_words(4)};
    const int want_bits[] = {0, 1, 2, c.r_bits, c.r_bits, 78, 64, 128};
    for (int ki = 0; ki < 8; ki++) {
        const Big &k = ks[ki];
        CHECK(cmp(k, c.r) < 0, "%s: scalar range", name);
        uint32_t kw[SCALAR_WORDS];
        scalar_words(kw, k);
        const unsigned own = scalar_bits(kw);
        CHECK((int)own == want_bits[ki] && (int)own == bits(k), "%s: scalar_bits of scalar %d", name, ki);
        const Pt kP = ec_mul(k, P, c.p);
        const Xyzz<F> forms[2] = {from_ref(P, c), projective_form(P, c)};
        for (unsigned len = own; len <= 256; len++) {
            Xyzz<F> t;
            mul(t, forms[len & 1], kw, len);
            CHECK(same(to_ref(t, c), kP), "%s: scalar %d over %u bits", name, ki, len);
            check_stored(t, c, "scalar_mul");
            Xyzz<F> o;
            mul(o, id, kw, len);
            CHECK(xyzz_is_identity(o), "%s: scalar %d times the identity over %u bits", name, ki, len);
        }
        // the addend: the identity, a generic point, k P itself and -k P, after the shortest and the longest loop
        const Pt addends[] = {Pt(), Q, kP, neg(kP, c.p)};
        for (unsigned len : {own, 256u}) {
            for (int ai = 0; ai < 4; ai++) {
                for (int form = 0; form < 2; form++) {
                    Xyzz<F> t;
                    mul(t, forms[form], kw, len);
                    uint32_t aw[2 * F::L];
                    affine_wire<F>(aw, addends[ai], c);
                    if (addends[ai].inf) aw[F::L] = 7; // x == 0 alone marks the identity
                    add_wire(t, aw);
                    CHECK(same(to_ref(t, c), ec_add(addends[ai], kP, c.p)), "%s: scalar %d addend %d", name, ki, ai);
                    if (ai == 3) CHECK(xyzz_is_identity(t), "%s: A = -k P leaves the identity", name);
                    check_stored(t, c, "add_affine_wire");
                }
                Xyzz<F> o;
                mul(o, id, kw, len);
                uint32_t aw[2 * F::L];
                affine_wire<F>(aw, addends[ai], c);
                add_wire(o, aw);
                CHECK(same(to_ref(o, c), addends[ai]), "%s: the identity times scalar %d, addend %d", name, ki, ai);
                check_stored(o, c, "add_affine_wire over the identity");
            }
        }
    }
    {
        uint32_t kw[SCALAR_WORDS];
        scalar_words(kw, sub(c.r, Big(1)));
        Xyzz<F> t;
        mul(t, from_ref(Q, c), kw, scalar_bits(kw));
        CHECK(same(to_ref(t, c), neg(Q, c.p)), "%s: (r - 1) P = -P", name);
    }

    // scalars: the wire residue to the integer, and c s^i
    Big Rr(1);
    for (int i = 0; i < 256; i++) Rr = mod_add(Rr, Rr, c.r);
    auto fr_wire = [&](uint32_t (&w)[SCALAR_WORDS], const Big &v) { scalar_words(w, mod_mul(v, Rr, c.r)); };
    const Big values[] = {Big(), Big(1), sub(c.r, Big(1)), random_words(4), mod_mul(random_words(7), random_words(7), c.r)};
    for (const Big &v : values) {
        uint32_t wire[SCALAR_WORDS], out[SCALAR_WORDS], want[SCALAR_WORDS];
        fr_wire(wire, v);
        scalar_from_wire<Fr>(out, wire);
        scalar_words(want, v);
        CHECK(memcmp(out, want, sizeof out) == 0, "%s: scalar_from_wire", name);
    }
    const Big cs[][2] = {{Big(1), Big(1)}, {Big(3), Big(5)}, {values[4], mod_mul(random_words(6), random_words(7), c.r)}, {Big(), values[3]}, {values[3], Big()}};
    for (const auto &pair : cs) {
        uint32_t wire[SCALAR_WORDS];
        Fe<Fr> fc, fs;
        fr_wire(wire, pair[0]);
        fe_from_wire(fc, wire);
        fr_wire(wire, pair[1]);
        fe_from_wire(fs, wire);
        PowerTable<Fr> table;
        power_table(table, fc, fs);
        for (uint32_t i : {0u, 1u, (1u << 27) + 5u, (1u << 28) - 1u}) {
            uint32_t out[SCALAR_WORDS], want[SCALAR_WORDS];
            power_scalar(out, table, i);
            scalar_words(want, mod_mul(pair[0], mod_pow(pair[1], Big(i), c.r), c.r));
            CHECK(memcmp(out, want, sizeof out) == 0, "%s: c s^%u", name, i);
        }
    }
    CHECK(mul_blocks(1) == 1 && mul_blocks(64) == 1 && mul_blocks(65) == 2 && mul_blocks((u64)1 << 28) == (u64)1 << 22, "mul_blocks");
    CHECK(norm_blocks(1) == 1 && norm_blocks(4096) == 1 && norm_blocks(4097) == 2 && norm_blocks((u64)1 << 28) == (u64)1 << 16, "norm_blocks");
}

int main()
{
    run_curve<Bn254Fq, Bn254Fr>("bn254", "30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47", "1", "2");
    run_curve<Bls377Fq, Bls377Fr>("bls12_377", "01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001",
                                  "008848DEFE740A67C8FC6225BF87FF5485951E2CAA9D41BB188282C8BD37CB5CD5481512FFCD394EEAB9B16EB21BE9EF",
                                  "01914A69C5102EFF1F674F5D30AFEEC4BD7FB348CA3E52D96D182AD44FB82305C2FE3D3634A9591AFD82DE55559C8EA6");
    run_curve<Bls381Fq, Bls381Fr>("bls12_381", "1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB",
                                  "17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB",
                                  "08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1");
    printf("ok %ld\n", g_checks);
    return 0;
}
