// Stand-alone host check of fe_words_neg (panda_amd/csrc/fe29.h): p - y on the packed 32-bit words of a canonical y, as k_accumulate
// applies it to the y of a row under a negative digit.  Test infrastructure: compiled and run by tests/test_fe_words_neg_host.py.
//   fe_words_neg_host <field>      field: 0 BN254 Fq, 1 BN254 Fr, 2 BLS12-377 Fq, 4 BLS12-381 Fq (the ids of panda_debug_field_op)
// reads one value per line from stdin (L words of 8 hex digits, least significant first, separated by blanks) and prints, per value,
// the L words of the result followed by the N limbs fe_unpack makes of them.  Both the out-of-place and the in-place call are made;
// the program exits with 2 if they differ.
#include <stdio.h>
#include <stdlib.h>

#include "../../panda_amd/csrc/fe29.h"

using namespace panda29;

template <class F>
static int run()
{
    constexpr int L = F::L, N = F::N;
    u32 w[L];
    for (;;) {
        for (int i = 0; i < L; i++)
            if (scanf("%x", &w[i]) != 1) return i == 0 ? 0 : 1;
        u32 r[L], in_place[L];
        fe_words_neg<F>(r, w);
        for (int i = 0; i < L; i++) in_place[i] = w[i];
        fe_words_neg<F>(in_place, in_place);
        for (int i = 0; i < L; i++)
            if (in_place[i] != r[i]) return 2;
        Fe<F> y;
        fe_unpack(y, r);
        for (int i = 0; i < L; i++) printf("%08x ", r[i]);
        for (int i = 0; i < N; i++) printf("%08x%c", y.l[i], i == N - 1 ? '\n' : ' ');
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) return 64;
    switch (atoi(argv[1])) {
    case 0: return run<Bn254Fq>();
    case 1: return run<Bn254Fr>();
    case 2: return run<Bls377Fq>();
    case 4: return run<Bls381Fq>();
    }
    return 64;
}
