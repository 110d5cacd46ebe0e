// What the host admits a basis extension and a key inner product with, read off the launch structs (tests/test_limit_moduli_oracle.py): the
// REAL host code -- DevModup::init of lr_host.hpp (lazy_terms, exact_terms, word_barrett, wide_ok) and keymac_wide_ok of lr_abi_ckks.cpp --
// compiled with g++ against the host-only HIP stand-in and the recording launch stubs of tests/cpp/hipstub/, which keep the tables of the last
// extension launch and the `wide` flags of the last key inner product.  Arguments, any number of groups:
//   ext    <name> <logN> <|Q|> <|P|> <input limbs> q.. p..     one ModUpSplitQP, default options and ext_narrow
//   keymac <name> <logN> <|Q|> <|P|> q.. p..                   one SwitchKeys at the top level, default options and keymac_narrow
// One line per group and option set:  "ext <name> <option> lazy_terms exact_terms word_barrett wide_ok input_limbs"
//                                     "keymac <name> <option> beta wide(Q part) wide(P part)"
// Exit code 0 = every call went through.  Nothing here computes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern thread_local int g_stub_last_ext[5];
extern thread_local int g_stub_last_keymac_wide[2];
}

int main(int argc, char **argv) {
    int a = 1;
    while (a < argc) {
        const bool ext = std::strcmp(argv[a], "ext") == 0;
        const char *name = argv[a + 1];
        const int logn = std::atoi(argv[a + 2]), nq = std::atoi(argv[a + 3]), np = std::atoi(argv[a + 4]);
        const int n_in = ext ? std::atoi(argv[a + 5]) : nq;
        a += ext ? 6 : 5;
        std::vector<uint64_t> Q, P;
        for (int i = 0; i < nq; ++i) Q.push_back(std::strtoull(argv[a++], nullptr, 10));
        for (int i = 0; i < np; ++i) P.push_back(std::strtoull(argv[a++], nullptr, 10));
        const uint64_t N = (uint64_t)1 << logn;
        for (int narrow = 0; narrow < 2; ++narrow) {
            lr_options opt;
            OK(lr_options_init(&opt));
            (ext ? opt.ext_narrow : opt.keymac_narrow) = narrow;
            lr_context *cq = nullptr, *cp = nullptr;
            OK(lr_context_create_ex(N, Q.data(), nq, 0, &opt, &cq));
            OK(lr_context_create_ex(N, P.data(), np, 0, &opt, &cp));
            if (ext) {
                lr_bext *bx = nullptr;
                lr_poly *pq = nullptr, *pp = nullptr;
                OK(lr_bext_create(cq, cp, &bx));
                OK(lr_poly_alloc(cq, nq, 1, &pq));
                OK(lr_poly_alloc(cp, np, 1, &pp));
                OK(lr_modup_split_qp(bx, n_in - 1, pq, pp));
                std::printf("ext %s %s %d %d %d %d %d\n", name, narrow ? "ext_narrow" : "default", lr::g_stub_last_ext[0], lr::g_stub_last_ext[1],
                            lr::g_stub_last_ext[2], lr::g_stub_last_ext[3], lr::g_stub_last_ext[4]);
                OK(lr_poly_free(pq));
                OK(lr_poly_free(pp));
                OK(lr_bext_destroy(bx));
            } else {
                const int beta = (nq + np - 1) / np;
                lr_ckks_plan *pl = nullptr;
                lr_poly *key = nullptr, *cx = nullptr, *o0 = nullptr, *o1 = nullptr;
                OK(lr_ckks_plan_create_ex(cq, cp, 1, &opt, &pl));
                OK(lr_poly_alloc(cq, nq + np, 2 * beta, &key));
                OK(lr_poly_alloc(cq, nq, 1, &cx));
                OK(lr_poly_alloc(cq, nq, 1, &o0));
                OK(lr_poly_alloc(cq, nq, 1, &o1));
                OK(lr_ckks_switch_keys(pl, nq - 1, cx, key, o0, o1));
                std::printf("keymac %s %s %d %d %d\n", name, narrow ? "keymac_narrow" : "default", beta, lr::g_stub_last_keymac_wide[0],
                            lr::g_stub_last_keymac_wide[1]);
                for (lr_poly *p : {key, cx, o0, o1}) OK(lr_poly_free(p));
                OK(lr_ckks_plan_destroy(pl));
            }
            OK(lr_context_destroy(cq));
            OK(lr_context_destroy(cp));
        }
    }
    return g_fail.load() ? 1 : 0;
}
