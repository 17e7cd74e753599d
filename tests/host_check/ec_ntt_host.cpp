// ec_ntt_host.cpp -- the routines of panda_amd/csrc/ec_ntt.h on the host under FE29_CHECK (every column accumulator and every limb range
// of fe29.h is asserted), against the AFFINE group law in integer arithmetic of this file's own (416-bit words, bit-serial products,
// binary-GCD inverses): nothing here shares code with fe29.h / curve29.h beyond the routines under test.  For the three curves:
//   scalar_mul     twiddles 1, 2, 3, r - 1, r - 2 (top bit set), 2^(bits - 1) + 5, random; the base in affine and in XYZZ form; B the identity
//   butterfly      generic operands; B, A, both the identity; w B = A; w B = -A; every stored point checked against the stored-point bounds
//   a transform    n = 8 through bit_reverse / butterfly_index / scalar_mul / butterfly / normalise_chunk against the definition
//   normalise_chunk over XYZZ points and over Jacobian and homogeneous triples: identities only, first and last the identity, a single
//                  point, through accessors that check every index
// Prints "ok <checks>"; any failure aborts with a message.  Build: g++ -O2 -std=c++17 (tests/test_ec_ntt.py does).
#define FE29_CHECK 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../panda_amd/csrc/ec_ntt.h"

using namespace panda29;
using namespace panda_ecntt;

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
    Big p, r, R, Rinv, b; // R = 2^(32 L) mod p
    Pt g;
    int r_bits;
};
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
template <class F>
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
    const Big p2 = times<F>(c.p, 2);
    for (int i = 0; i < F::N - 1; i++) {
        CHECK(P.Y.l[i] < (1u << 29) && P.ZZ.l[i] < (1u << 29) && P.ZZZ.l[i] < (1u << 29), "%s: Y / ZZ / ZZZ limb %d not tight", what, i);
        CHECK(P.X.l[i] <= (1u << 29) + 8, "%s: X limb %d not loose", what, i);
    }
    CHECK(cmp(limb_value(P.Y), p2) < 0, "%s: Y >= 2p", what);
    CHECK(cmp(limb_value(P.ZZ), p2) < 0 && cmp(limb_value(P.ZZZ), p2) < 0, "%s: ZZ / ZZZ >= 2p", what);
    CHECK(cmp(limb_value(P.X), times<F>(c.p, Bounds<F>::XB)) < 0, "%s: X >= XB p", what);
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
    point_from_affine_wire(r, w);
    return r;
}
static void scalar_words(uint32_t (&w)[SCALAR_WORDS], const Big &k)
{
    for (int i = 0; i < SCALAR_WORDS; i++) w[i] = k.w[i];
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}
static Big random_below(const Big &m)
{
    Big r;
    for (int i = 0; i < 8; i++) r.w[i] = (uint32_t)rnd();
    r.w[7] &= 0x0FFFFFFF; // below 2^252: below every r here
    (void)m;
    return r;
}

// a second representative of a point: (3 P) - (2 P) through the routines, so ZZ != 1
template <class F>
static Xyzz<F> projective_form(const Pt &P, const Curve<F> &c)
{
    Xyzz<F> b = from_ref(P, c), t3, t2;
    uint32_t w[SCALAR_WORDS];
    scalar_words(w, Big(3));
    scalar_mul(t3, b, w);
    scalar_words(w, Big(2));
    scalar_mul(t2, b, w);
    negate_point(t2);
    xyzz_add(t3, t2);
    CHECK(same(to_ref(t3, c), P), "projective_form");
    check_stored(t3, c, "projective_form");
    return t3;
}

template <class F>
static void run_butterfly(const Xyzz<F> &A, const Xyzz<F> &B, const Big &w, const Curve<F> &c, const char *what)
{
    uint32_t ww[SCALAR_WORDS];
    scalar_words(ww, w);
    Xyzz<F> t, lo, hi;
    scalar_mul(t, B, ww);
    const Pt a = to_ref(A, c), wb = ec_mul(w, to_ref(B, c), c.p);
    CHECK(same(to_ref(t, c), wb), "%s: w B", what);
    check_stored(t, c, what);
    int loads = 0;
    butterfly(t, [&](Xyzz<F> &x) { x = A, loads++; }, [&](const Xyzz<F> &v) { lo = v; }, [&](const Xyzz<F> &v) { hi = v; });
    CHECK(loads == 2, "%s: loads", what);
    CHECK(same(to_ref(lo, c), ec_add(a, wb, c.p)), "%s: A + w B", what);
    CHECK(same(to_ref(hi, c), ec_add(a, neg(wb, c.p), c.p)), "%s: A - w B", what);
    check_stored(lo, c, what);
    check_stored(hi, c, what);
    // the outputs are operands of the next stage: once more, with the roles swapped
    Xyzz<F> t2 = hi, lo2, hi2;
    butterfly(t2, [&](Xyzz<F> &x) { x = lo; }, [&](const Xyzz<F> &v) { lo2 = v; }, [&](const Xyzz<F> &v) { hi2 = v; });
    CHECK(same(to_ref(lo2, c), ec_add(a, a, c.p)), "%s: second stage sum", what);
    CHECK(same(to_ref(hi2, c), ec_add(wb, wb, c.p)), "%s: second stage difference", what);
    check_stored(lo2, c, what);
    check_stored(hi2, c, what);
}

// index-checking accessors for normalise_chunk
template <class F>
struct HostXyzz {
    const std::vector<Xyzz<F>> &pts;
    std::vector<uint32_t> &out;
    uint32_t count;
    mutable std::vector<int> parked;
    bool denominator(Fe<F> &d, uint32_t i) const
    {
        CHECK(i < count, "denominator index");
        d = pts[i].ZZZ;
        return !xyzz_is_identity(pts[i]);
    }
    void put_prefix(uint32_t i, const Fe<F> &v) const
    {
        CHECK(i < count && !parked[i], "put_prefix index");
        parked[i] = 1;
        memcpy(&out[(size_t)i * 2 * F::L], v.l, 4 * F::N);
    }
    void get_prefix(Fe<F> &v, uint32_t i) const
    {
        CHECK(i < count && parked[i] == 1, "get_prefix of a slot that holds none");
        memcpy(v.l, &out[(size_t)i * 2 * F::L], 4 * F::N);
    }
    void finish(uint32_t i, const Fe<F> &dinv) const
    {
        CHECK(i < count && parked[i] == 1, "finish index");
        parked[i] = 2;
        xyzz_affine_wire(&out[(size_t)i * 2 * F::L], pts[i], dinv);
    }
    void put_identity(uint32_t i) const
    {
        CHECK(i < count && !parked[i], "put_identity index");
        memset(&out[(size_t)i * 2 * F::L], 0, 8 * F::L);
    }
};
template <class F>
struct HostTriples {
    const std::vector<uint32_t> &in;
    std::vector<uint32_t> &out;
    uint32_t count;
    bool homogeneous;
    bool denominator(Fe<F> &d, uint32_t i) const
    {
        CHECK(i < count, "denominator index");
        return triple_denominator<F>(d, &in[(size_t)i * 3 * F::L + 2 * F::L]);
    }
    void put_prefix(uint32_t i, const Fe<F> &v) const
    {
        CHECK(i < count, "put_prefix index");
        memcpy(&out[(size_t)i * 2 * F::L], v.l, 4 * F::N);
    }
    void get_prefix(Fe<F> &v, uint32_t i) const
    {
        CHECK(i < count, "get_prefix index");
        memcpy(v.l, &out[(size_t)i * 2 * F::L], 4 * F::N);
    }
    void finish(uint32_t i, const Fe<F> &dinv) const
    {
        CHECK(i < count, "finish index");
        triple_affine_wire<F>(&out[(size_t)i * 2 * F::L], &in[(size_t)i * 3 * F::L], dinv, homogeneous);
    }
    void put_identity(uint32_t i) const
    {
        CHECK(i < count, "put_identity index");
        memset(&out[(size_t)i * 2 * F::L], 0, 8 * F::L);
    }
};

template <class F>
static void check_normalise_xyzz(const std::vector<Xyzz<F>> &pts, const Curve<F> &c, const char *what)
{
    const uint32_t n = (uint32_t)pts.size();
    std::vector<uint32_t> out((size_t)n * 2 * F::L + 8, 0xA5A5A5A5u);
    HostXyzz<F> io = {pts, out, n, std::vector<int>(n, 0)};
    normalise_chunk<F>(io, n);
    for (uint32_t i = 0; i < n; i++) CHECK(same(affine_from_wire_words<F>(&out[(size_t)i * 2 * F::L], c), to_ref(pts[i], c)), "%s: point %u", what, i);
    for (int k = 0; k < 8; k++) CHECK(out[(size_t)n * 2 * F::L + k] == 0xA5A5A5A5u, "%s: wrote behind the chunk", what);
}

template <class F>
static void check_normalise_triples(const std::vector<Pt> &pts, bool homogeneous, const Curve<F> &c, const char *what)
{
    const uint32_t n = (uint32_t)pts.size();
    std::vector<uint32_t> in((size_t)n * 3 * F::L), out((size_t)n * 2 * F::L + 8, 0xA5A5A5A5u);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t *t = &in[(size_t)i * 3 * F::L];
        if (pts[i].inf) { // Z == 0, X and Y arbitrary
            to_wire<F>(t, Big(rnd() | 1), c);
            to_wire<F>(t + F::L, Big(rnd() | 1), c);
            memset(t + 2 * F::L, 0, 4 * F::L);
            continue;
        }
        const Big z = Big(rnd() | 2), z2 = mod_mul(z, z, c.p), z3 = mod_mul(z2, z, c.p);
        to_wire<F>(t, mod_mul(pts[i].x, homogeneous ? z : z2, c.p), c);
        to_wire<F>(t + F::L, mod_mul(pts[i].y, homogeneous ? z : z3, c.p), c);
        to_wire<F>(t + 2 * F::L, z, c);
    }
    HostTriples<F> io = {in, out, n, homogeneous};
    normalise_chunk<F>(io, n);
    for (uint32_t i = 0; i < n; i++) CHECK(same(affine_from_wire_words<F>(&out[(size_t)i * 2 * F::L], c), pts[i]), "%s: point %u", what, i);
    for (int k = 0; k < 8; k++) CHECK(out[(size_t)n * 2 * F::L + k] == 0xA5A5A5A5u, "%s: wrote behind the chunk", what);
}

template <class F, class Fr>
static void run_curve(const char *name, const char *p_hex, const char *gx, const char *gy, unsigned b, unsigned fr_generator)
{
    Curve<F> c;
    c.p = from_hex(p_hex);
    for (int i = 0; i < Fr::L; i++) c.r.w[i] = Fr::PW[i];
    for (int i = 0; i < F::L; i++) CHECK(c.p.w[i] == F::PW[i], "%s: the modulus of the parameter table", name);
    c.r_bits = bits(c.r);
    c.R = Big(1);
    for (int i = 0; i < 32 * F::L; i++) c.R = mod_add(c.R, c.R, c.p);
    c.Rinv = mod_inv(c.R, c.p);
    CHECK(cmp(mod_mul(c.R, c.Rinv, c.p), Big(1)) == 0, "mod_inv");
    c.b = Big(b);
    c.g.inf = false, c.g.x = from_hex(gx), c.g.y = from_hex(gy);
    auto on_curve = [&](const Pt &P) { return P.inf || cmp(mod_mul(P.y, P.y, c.p), mod_add(mod_mul(mod_mul(P.x, P.x, c.p), P.x, c.p), c.b, c.p)) == 0; };
    CHECK(on_curve(c.g), "%s: generator", name);
    CHECK(ec_mul(c.r, c.g, c.p).inf, "%s: order of the generator", name);

    const Pt P5 = ec_mul(Big(5), c.g, c.p), P7 = ec_mul(Big(7), c.g, c.p), PR = ec_mul(random_below(c.r), c.g, c.p);
    CHECK(on_curve(P5) && on_curve(PR), "ec_mul");
    Xyzz<F> id;
    xyzz_set_identity(id);

    // scalar_mul
    Big top;
    top.w[(c.r_bits - 1) >> 5] = 1u << ((c.r_bits - 1) & 31);
    const Big twiddles[] = {Big(1), Big(2), Big(3), sub(c.r, Big(1)), sub(c.r, Big(2)), add(top, Big(5)), random_below(c.r), random_below(c.r)};
    for (const Big &w : twiddles) {
        CHECK(cmp(w, c.r) < 0 || cmp(w, add(top, Big(5))) == 0, "twiddle range");
        uint32_t ww[SCALAR_WORDS];
        scalar_words(ww, w);
        for (int form = 0; form < 2; form++) {
            const Xyzz<F> B = form ? projective_form(PR, c) : from_ref(PR, c);
            Xyzz<F> t;
            scalar_mul(t, B, ww);
            CHECK(same(to_ref(t, c), ec_mul(w, PR, c.p)), "%s: scalar_mul form %d", name, form);
            check_stored(t, c, "scalar_mul");
        }
        Xyzz<F> t;
        scalar_mul(t, id, ww);
        CHECK(xyzz_is_identity(t), "%s: w * identity", name);
    }
    {
        uint32_t ww[SCALAR_WORDS];
        scalar_words(ww, sub(c.r, Big(1)));
        Xyzz<F> t;
        scalar_mul(t, from_ref(P5, c), ww);
        CHECK(same(to_ref(t, c), neg(P5, c.p)), "%s: (r - 1) P = -P", name);
    }

    // butterflies
    const Big w_top = sub(c.r, Big(2)), w_rand = random_below(c.r);
    const Big ws[] = {Big(1), sub(c.r, Big(1)), w_top, w_rand};
    for (const Big &w : ws) {
        const Pt wB = ec_mul(w, P7, c.p);
        for (int form = 0; form < 2; form++) {
            const Xyzz<F> B = form ? projective_form(P7, c) : from_ref(P7, c);
            run_butterfly(form ? projective_form(P5, c) : from_ref(P5, c), B, w, c, "generic");
            run_butterfly(id, B, w, c, "A the identity");
            run_butterfly(form ? projective_form(P5, c) : from_ref(P5, c), id, w, c, "B the identity");
            run_butterfly(id, id, w, c, "both the identity");
            run_butterfly(form ? projective_form(wB, c) : from_ref(wB, c), B, w, c, "w B = A");
            run_butterfly(form ? from_ref(neg(wB, c.p), c) : projective_form(neg(wB, c.p), c), B, w, c, "w B = -A");
        }
    }

    // a transform of 8 points against the definition: P_j = s_j G, out[k] = (sum_j s_j omega^(jk)) G
    {
        const unsigned log_n = 3, n = 8;
        const Big e = shr1(shr1(shr1(sub(c.r, Big(1)))));
        const Big omega = mod_pow(Big(fr_generator), e, c.r);
        CHECK(cmp(mod_pow(omega, Big(4), c.r), sub(c.r, Big(1))) == 0, "%s: omega^4 = -1", name);
        Big s[8];
        std::vector<Xyzz<F>> x(n);
        for (unsigned j = 0; j < n; j++) {
            s[j] = j == 2 ? Big() : j == 5 ? s[1] : random_below(c.r); // an identity and a repeated point among the inputs
            x[j] = from_ref(ec_mul(s[j], c.g, c.p), c);
        }
        std::vector<Xyzz<F>> v(n);
        for (unsigned i = 0; i < n; i++) v[i] = x[bit_reverse(i, log_n)];
        CHECK(bit_reverse(1, 3) == 4 && bit_reverse(6, 3) == 3 && bit_reverse(0, 0) == 0, "bit_reverse");
        for (unsigned st = 1; st <= log_n; st++) {
            std::vector<int> seen(n, 0);
            for (uint32_t t = 0; t < n / 2; t++) {
                const ButterflyIndex ix = butterfly_index(t, log_n, st);
                CHECK(ix.lo < n && ix.hi < n && ix.twiddle < n / 2 && !seen[ix.lo] && !seen[ix.hi], "butterfly_index");
                seen[ix.lo] = seen[ix.hi] = 1;
                uint32_t ww[SCALAR_WORDS];
                scalar_words(ww, mod_pow(omega, Big(ix.twiddle), c.r));
                Xyzz<F> wb;
                scalar_mul(wb, v[ix.hi], ww);
                // in place, as the stage kernel runs it: the second read of A's slot comes after the first store
                butterfly(wb, [&](Xyzz<F> &o) { o = v[ix.lo]; }, [&](const Xyzz<F> &o) { v[ix.lo] = o; }, [&](const Xyzz<F> &o) { v[ix.hi] = o; });
            }
        }
        for (unsigned k = 0; k < n; k++) {
            Big sum;
            for (unsigned j = 0; j < n; j++) sum = mod_add(sum, mod_mul(s[j], mod_pow(omega, Big(j * k), c.r), c.r), c.r);
            CHECK(same(to_ref(v[k], c), ec_mul(sum, c.g, c.p)), "%s: transform output %u", name, k);
            check_stored(v[k], c, "transform");
        }
        check_normalise_xyzz(v, c, "transform outputs");
        CHECK(uniform_stages(6) == 0 && uniform_stages(7) == 1 && uniform_stages(12) == 6 && uniform_stages(26) == 20, "uniform_stages");
    }

    // normalisation
    {
        std::vector<Xyzz<F>> some = {id, projective_form(P5, c), from_ref(P7, c), id, id, projective_form(PR, c), projective_form(P7, c), id};
        check_normalise_xyzz(some, c, "first and last the identity");
        check_normalise_xyzz(std::vector<Xyzz<F>>(CHUNK, id), c, "identities only");
        check_normalise_xyzz(std::vector<Xyzz<F>>(1, projective_form(PR, c)), c, "one point");
        check_normalise_xyzz(std::vector<Xyzz<F>>(1, id), c, "one identity");
        std::vector<Xyzz<F>> full;
        for (unsigned i = 0; i < CHUNK; i++) full.push_back(projective_form(ec_mul(Big(i + 2), c.g, c.p), c));
        check_normalise_xyzz(full, c, "a full chunk");
        const Pt inf;
        for (int h = 0; h < 2; h++) {
            check_normalise_triples<F>({inf, P5, P7, inf, inf, PR, P7, inf}, h != 0, c, "triples: first and last the identity");
            check_normalise_triples<F>(std::vector<Pt>(CHUNK, inf), h != 0, c, "triples: identities only");
            check_normalise_triples<F>({PR}, h != 0, c, "triples: one point");
            std::vector<Pt> many;
            for (unsigned i = 0; i < CHUNK; i++) many.push_back(ec_mul(Big(i + 1), c.g, c.p));
            check_normalise_triples<F>(many, h != 0, c, "triples: a full chunk");
        }
    }
}

int main()
{
    run_curve<Bn254Fq, Bn254Fr>("bn254", "30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47", "1", "2", 3, 5);
    run_curve<Bls377Fq, Bls377Fr>("bls12_377", "01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001",
                                  "008848DEFE740A67C8FC6225BF87FF5485951E2CAA9D41BB188282C8BD37CB5CD5481512FFCD394EEAB9B16EB21BE9EF",
                                  "01914A69C5102EFF1F674F5D30AFEEC4BD7FB348CA3E52D96D182AD44FB82305C2FE3D3634A9591AFD82DE55559C8EA6", 1, 22);
    run_curve<Bls381Fq, Bls381Fr>("bls12_381", "1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB",
                                  "17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB",
                                  "08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1", 4, 7);
    printf("ok %ld\n", g_checks);
    return 0;
}
