// The modular primitives of lr_arith.hpp on the host (tests/test_host_logic.py), at the moduli where the lazy bounds are tight and on the
// operand corners, against unsigned __int128:
//   * mul_shoup_lazy, mul_shoup_lazy_lowreg: congruent to v * w, in [0, 4q) for ANY 64-bit v, and equal to the exact Shoup product plus
//     0, 1 or 2 times q (the "deficit at most 2" of the quotient estimate, lr_arith.hpp:102-104);
//   * mul_shoup_exact: congruent, in [0, 2q);
//   * bred / bred_constant, bred_add / bred_add_constant, mred / mred_constant, mform / mform_constant, inv_mform: the canonical forms equal
//     the residue, the constant forms are congruent and below 2q.
// Arguments: the moduli (decimal).  Prints "shoup_products: checks N, failures F"; exit code 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lr_arith.hpp"

using lr::u128;
using lr::u64;

static long long g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        ++g_checks;                                            \
        if (!(cond)) {                                         \
            if (++g_fail <= 20) {                              \
                std::fprintf(stderr, "CHECK failed: %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);             \
                std::fprintf(stderr, "\n");                    \
            }                                                  \
        }                                                      \
    } while (0)

static u64 mulmod(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }

// a twiddle whose companion has both words near 0xFFFFFFFF: the dropped partial products of the quotient estimate are then largest
static u64 high_companion(u64 q) {
    const u64 slack = (u64)((((u128)1) << 64) / q) + 2;
    const u128 target = (((u128)1) << 64) - 1 - slack;
    return (u64)((target * q + ((((u128)1) << 64) - 1)) >> 64);
}

static void check_modulus(u64 q) {
    const u64 M = ~(u64)0;
    const u128 uu = ~(u128)0 / q;                      // floor(2^128 / q): q is odd
    const u64 u_hi = (u64)(uu >> 64), u_lo = (u64)uu;
    u64 qinv = 1;
    for (int i = 0; i < 7; ++i) qinv *= 2 - q * qinv;  // q^-1 mod 2^64
    const u64 r64 = (u64)((((u128)1) << 64) % q);      // 2^64 mod q
    u64 r64_inv = 1;                                   // 2^-64 mod q, by Fermat
    {
        u64 base = r64, e = q - 2;
        while (e) {
            if (e & 1) r64_inv = mulmod(r64_inv, base, q);
            base = mulmod(base, base, q);
            e >>= 1;
        }
    }
    std::vector<u64> ws = {1, 2, (q - 1) / 2, q - 2, q - 1, high_companion(q)};
    std::vector<u64> vs = {0, 1, q - 1, q, 2 * q - 1, 4 * q - 1, 0xFFFFFFFFull, 1ull << 32, (1ull << 63) - 1, 1ull << 63, M,
                           (1ull << 32) | 0xFFFFFFFFull, ((q >> 32) << 32) | 0xFFFFFFFFull, 0xFFFFFFFF00000000ull, 0x7FFFFFFEFFFFFFFFull,
                           (M / q) * q - 1, (M / q) * q, (M / q) * q + 1};
    for (u64 w : ws) {
        CHECK(w > 0 && w < q, "twiddle %llu", (unsigned long long)w);
        const u64 s = lr::shoup_companion(w, q);
        for (u64 v : vs) {
            const u64 want = mulmod(v % q, w, q);
            const u64 exact = lr::mul_shoup_exact(v, w, s, q);
            CHECK(exact % q == want && exact < 2 * q, "exact q=%llu v=%llu w=%llu", (unsigned long long)q, (unsigned long long)v, (unsigned long long)w);
            // the exact product as an unbounded integer: v*w - floor(v*s / 2^64) * q
            const u128 true_exact = (u128)v * w - (u128)(u64)(((u128)v * s) >> 64) * q;
            CHECK(true_exact == exact, "exact wraps q=%llu v=%llu w=%llu", (unsigned long long)q, (unsigned long long)v, (unsigned long long)w);
            for (int low = 0; low < 2; ++low) {
                const u64 r = low ? lr::mul_shoup_lazy_lowreg(v, w, s, q) : lr::mul_shoup_lazy(v, w, s, q);
                CHECK(r % q == want, "lazy%d congruence q=%llu v=%llu w=%llu", low, (unsigned long long)q, (unsigned long long)v, (unsigned long long)w);
                CHECK(r < 4 * q, "lazy%d range q=%llu v=%llu w=%llu r=%llu", low, (unsigned long long)q, (unsigned long long)v, (unsigned long long)w, (unsigned long long)r);
                CHECK(r >= exact && (r - exact) % q == 0 && (r - exact) / q <= 2, "lazy%d deficit q=%llu v=%llu w=%llu", low, (unsigned long long)q,
                      (unsigned long long)v, (unsigned long long)w);
            }
        }
    }
    // Barrett and Montgomery forms: canonical operands for the products, any 64-bit value for the single-operand reductions
    std::vector<u64> cs = {0, 1, 2, (q - 1) / 2, (q + 1) / 2, q - 2, q - 1, 0xFFFFFFFFull % q, (1ull << 32) % q, high_companion(q)};
    for (u64 x : cs)
        for (u64 y : cs) {
            const u64 want = mulmod(x, y, q);
            CHECK(lr::bred(x, y, q, u_hi, u_lo) == want, "bred q=%llu x=%llu y=%llu", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y);
            const u64 bc = lr::bred_constant(x, y, q, u_hi, u_lo);
            CHECK(bc % q == want && bc < 2 * q, "bred_constant q=%llu x=%llu y=%llu", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y);
            const u64 wantm = mulmod(want, r64_inv, q);
            CHECK(lr::mred(x, y, q, qinv) == wantm, "mred q=%llu x=%llu y=%llu", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y);
            const u64 mc = lr::mred_constant(x, y, q, qinv);
            CHECK(mc % q == wantm && mc < 2 * q, "mred_constant q=%llu x=%llu y=%llu", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y);
        }
    for (u64 v : vs) {
        CHECK(lr::bred_add(v, q, u_hi) == v % q, "bred_add q=%llu v=%llu", (unsigned long long)q, (unsigned long long)v);
        const u64 bc = lr::bred_add_constant(v, q, u_hi);
        CHECK(bc % q == v % q && bc < 2 * q, "bred_add_constant q=%llu v=%llu", (unsigned long long)q, (unsigned long long)v);
        // MRed with a lazy first operand, as the kernels use it (x * y < q * 2^64)
        for (u64 y : cs) {
            const u64 wantm = mulmod(mulmod(v % q, y, q), r64_inv, q);
            CHECK(lr::mred(v, y, q, qinv) == wantm, "mred lazy q=%llu v=%llu y=%llu", (unsigned long long)q, (unsigned long long)v, (unsigned long long)y);
        }
    }
    for (u64 a : cs) {
        CHECK(lr::mform(a, q, u_hi, u_lo) == mulmod(a, r64, q), "mform q=%llu a=%llu", (unsigned long long)q, (unsigned long long)a);
        const u64 mc = lr::mform_constant(a, q, u_hi, u_lo);
        CHECK(mc % q == mulmod(a, r64, q) && mc < 2 * q, "mform_constant q=%llu a=%llu", (unsigned long long)q, (unsigned long long)a);
        CHECK(lr::inv_mform(a, q, qinv) == mulmod(a, r64_inv, q), "inv_mform q=%llu a=%llu", (unsigned long long)q, (unsigned long long)a);
        CHECK(lr::inv_mform(lr::mform(a, q, u_hi, u_lo), q, qinv) == a, "round trip q=%llu a=%llu", (unsigned long long)q, (unsigned long long)a);
    }
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) check_modulus(std::strtoull(argv[i], nullptr, 10));
    std::printf("shoup_products: moduli %d, checks %lld, failures %lld\n", argc - 1, g_checks, g_fail);
    return g_fail || argc < 2 ? 1 : 0;
}
