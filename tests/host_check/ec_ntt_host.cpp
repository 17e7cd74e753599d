// ec_ntt_host.cpp -- the routines of panda_amd/csrc/ec_ntt.h on the host under FE29_CHECK (every column accumulator and every limb range
// of fe29.h is asserted), against the affine group law in integer arithmetic of ec_ref.h.  For the three curves:
//   scalar_mul     twiddles 1, 2, 3, r - 1, r - 2 (top bit set), 2^(bits - 1) + 5, random; the base in affine and in XYZZ form; B the identity
//   butterfly      generic operands; B, A, both the identity; w B = A; w B = -A; every stored point checked against the stored-point bounds
//   a transform    n = 8 through bit_reverse / butterfly_index / scalar_mul / butterfly / normalise_chunk against the definition
//   normalise_chunk over XYZZ points and over Jacobian and homogeneous triples: identities only, first and last the identity, a single
//                  point, through accessors that check every index
// Prints "ok <checks>"; any failure aborts with a message.  Build: g++ -O2 -std=c++17 (tests/test_ec_ntt.py does).
#include "ec_ref.h"

#include <vector>

using namespace panda_ecntt;

static Big random_below(const Big &m)
{
    Big r;
    for (int i = 0; i < 8; i++) r.w[i] = (uint32_t)rnd();
    r.w[7] &= 0x0FFFFFFF; // below 2^252: below every r here
    (void)m;
    return r;
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
static void run_curve(const CurveText &text)
{
    const char *name = text.name;
    const Curve<F> c = make_curve<F, Fr>(text);
    CHECK(cmp(mod_mul(c.R, c.Rinv, c.p), Big(1)) == 0, "mod_inv");
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
        const Big omega = mod_pow(Big(text.fr_generator), e, c.r);
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
    g_rng = 0x9E3779B97F4A7C15ull;
    run_curve<Bn254Fq, Bn254Fr>(BN254);
    run_curve<Bls377Fq, Bls377Fr>(BLS12_377);
    run_curve<Bls381Fq, Bls381Fr>(BLS12_381);
    printf("ok %ld\n", g_checks);
    return 0;
}
