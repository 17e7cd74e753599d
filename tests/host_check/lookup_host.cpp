// Host run of what panda_amd/csrc/lookup.h and poly_sum.h share between the kernels of lookup.hip and poly_sum.hip and the host, built
// with FE29_CHECK (128-bit shadow column accumulators in fe_mul, the limb-range assertion of fe_carry):
//   * the hash: `lookup_host hash <log_slots> <64 hex digits, the 32 bytes of an element in memory order> ...` prints the home slot of
//     every element, which the test compares with panda_lookup_home_slot;
//   * without arguments: the count -> wire conversion for the counts 0, 1, 2^28 - 1, 2^28 and the running sum's addition chains at
//     their stated bound (sum_run of RUN_MAX elements, every operand p - 1; add_canon of two), the three fields, against 256-bit
//     modular arithmetic written here.  Prints "ok <checks>" and exits 0.
// Test infrastructure: compiled and run by tests/test_lookup.py with g++.
#define FE29_CHECK 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../panda_amd/csrc/lookup.h"
#include "../../panda_amd/csrc/poly_sum.h"

using namespace panda29;
using namespace panda_lookup;
using namespace panda_poly;

namespace {

struct U256 {
    u64 w[4];
};

bool geq(const U256 &a, const U256 &b)
{
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
u64 add(U256 &r, const U256 &a, const U256 &b)
{
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (u64)c;
        c >>= 64;
    }
    return (u64)c;
}
void sub(U256 &r, const U256 &a, const U256 &b)
{
    u64 borrow = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        r.w[i] = (u64)d;
        borrow = (u64)(d >> 64) & 1;
    }
}
U256 addmod(const U256 &p, const U256 &a, const U256 &b) // a, b < p
{
    U256 r;
    const u64 carry = add(r, a, b);
    if (carry || geq(r, p)) sub(r, r, p);
    return r;
}
U256 mulmod(const U256 &p, const U256 &a, const U256 &b)
{
    U256 r = {{0, 0, 0, 0}};
    for (int bit = 255; bit >= 0; bit--) {
        r = addmod(p, r, r);
        if ((b.w[bit >> 6] >> (bit & 63)) & 1) r = addmod(p, r, a);
    }
    return r;
}
U256 from_words(const u32 *w)
{
    U256 r;
    for (int i = 0; i < 4; i++) r.w[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
    return r;
}
void to_words(u32 *w, const U256 &a)
{
    for (int i = 0; i < 4; i++) {
        w[2 * i] = (u32)a.w[i];
        w[2 * i + 1] = (u32)(a.w[i] >> 32);
    }
}

long checked = 0;

template <class Fr>
void expect(const Fe<Fr> &got_fe, const U256 &want, const char *what)
{
    u32 got[8], w[8];
    fe_pack(got, got_fe);
    to_words(w, want);
    if (memcmp(got, w, 32) != 0) {
        fprintf(stderr, "mismatch: %s\n", what);
        exit(1);
    }
    checked++;
}

template <class Fr>
void canonical_limbs(const Fe<Fr> &v)
{
    for (int i = 0; i < Fr::N - 1; i++)
        if (v.l[i] >= (1u << 29)) abort();
}

template <class Fr, int E>
void run_sums(const U256 &p, const U256 &value)
{
    u32 w[8];
    to_words(w, value);
    Fe<Fr> x[E], g;
    U256 want = {{0, 0, 0, 0}};
    for (int e = 0; e < E; e++) {
        fe_unpack(x[e], w);
        want = addmod(p, want, value);
    }
    sum_run<Fr, E>(g, x);
    canonical_limbs(g);
    expect(g, want, "sum_run");
    // the exclusive prefix chain of a thread: E - 1 add_canon from a canonical seed
    Fe<Fr> pre = g;
    U256 acc = want;
    for (int e = 0; e < E; e++) {
        add_canon(pre, pre, x[e]);
        canonical_limbs(pre);
        acc = addmod(p, acc, value);
        expect(pre, acc, "add_canon");
    }
}

template <class Fr>
void run_field()
{
    const U256 p = from_words(Fr::PW), one = {{1, 0, 0, 0}}, zero = {{0, 0, 0, 0}};
    U256 pm1, w = one;
    sub(pm1, p, one);
    for (int i = 0; i < 256; i++) w = addmod(p, w, w); // W mod p
    Fe<Fr> K;
    count_constant(K);
    canonical_limbs(K);
    const u32 counts[] = {0u, 1u, (1u << 28) - 1, 1u << 28, 2u, 12345u, 1u << 27};
    for (u32 c : counts) {
        Fe<Fr> r;
        count_to_wire(r, c, K);
        fe_reduce_small(r); // what store_elem does
        expect(r, mulmod(p, U256{{c, 0, 0, 0}}, w), "count_to_wire");
    }
    const U256 values[] = {pm1, zero, one, w};
    for (const U256 &v : values) {
        run_sums<Fr, 1>(p, v);
        run_sums<Fr, 2>(p, v);
        run_sums<Fr, 4>(p, v); // the kernels' run
        run_sums<Fr, RUN_MAX>(p, v);
    }
}

int hex_digit(char c)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && strcmp(argv[1], "hash") == 0) {
        const unsigned log_slots = (unsigned)atoi(argv[2]);
        if (log_slots == 0 || log_slots > MAX_LOG_SLOTS) return 2;
        for (int a = 3; a < argc; a++) {
            if (strlen(argv[a]) != 64) return 2;
            unsigned char bytes[32];
            for (int i = 0; i < 32; i++) {
                const int hi = hex_digit(argv[a][2 * i]), lo = hex_digit(argv[a][2 * i + 1]);
                if (hi < 0 || lo < 0) return 2;
                bytes[i] = (unsigned char)(hi * 16 + lo);
            }
            u32 w[8], h, fp;
            memcpy(w, bytes, 32);
            hash_elem(w, h, fp);
            printf("%u\n", home_slot(h, log_slots));
        }
        return 0;
    }
    run_field<Bn254Fr>();
    run_field<Bls377Fr>();
    run_field<Bls381Fr>();
    printf("ok %ld\n", checked);
    return 0;
}
